// seg_eval.hip -- the part-segmentation metrics of the reference's `validate` (tools/runner_unify_seg.py:301-367) on the device, so
// no log-probability leaves it (utils/evaluate.py SegMetric, upp_hip/infer.py SegEvalStep):
//   * upp_seg_iou_counts     : per point the first arg-max of the log-probabilities inside its shape's category (np.argmax: a NaN
//                              wins, the first one first), then integer histograms -- per shape and part the intersection, predicted
//                              and target counts, per part the seen and correct counts, the correct points -- added into an int32
//                              scratch (one integer atomic per non-zero bin and workgroup: the sums do not depend on arrival order).
//   * upp_seg_iou_accumulate : one workgroup turns the scratch into the per-shape IoUs (float64, sequential in part order, then one
//                              division: np.mean of fewer than 8 values), adds them into per-category sums in shape order, adds the
//                              int64 counters, and zeroes the scratch it read (no memset: the next evaluation, captured or not,
//                              finds it clean).
// The part table is data: part -> category (P) and category -> [lo, lo + n) (C, 2).  Wave64, vector stores only, no float atomics.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPoints = 256;            // points per workgroup of upp_seg_iou_counts: one per thread
constexpr int kMaxParts = 1024;         // P limit: 5 P + 1 int32 LDS bins (and C <= kBlock: one thread per category)

// np.argmax order: (a, ia) replaces the running best (b, ib) scanned in index order?  A NaN best is never replaced; a NaN a replaces
// any number; otherwise only a strictly larger value (equal values: the lower index stays).
__device__ __forceinline__ bool replaces(float a, float best) {
    if (best != best) return false;
    return a != a || a > best;
}

// Scratch layout (int32), for a call with B shapes and P parts:
//   [0, BP) intersection  [BP, 2BP) predicted  [2BP, 3BP) target  (shape b, part lo + k at b*P + k)
//   [3BP, 3BP + P) seen   [3BP + P, 3BP + 2P) correct   [3BP + 2P] correct points
__global__ __launch_bounds__(kBlock) void seg_iou_counts_kernel(const float *__restrict__ logp, long long ld,
                                                                const int64_t *__restrict__ target, const int32_t *__restrict__ part_cat,
                                                                const int32_t *__restrict__ cat_range, int N, int P, int C, int n_valid,
                                                                int64_t *__restrict__ pred, int32_t *__restrict__ scratch, int B) {
    __shared__ int s_bins[5 * kMaxParts + 1];
    const int b = blockIdx.y;
    const int n0 = blockIdx.x * kPoints;
    const long long BP = (long long)B * P;
    int *s_inter = s_bins, *s_pred = s_bins + P, *s_tgt = s_bins + 2 * P, *s_seen = s_bins + 3 * P, *s_corr = s_bins + 4 * P;
    int *s_total = s_bins + 5 * P;
    for (int i = threadIdx.x; i < 5 * P + 1; i += kBlock) s_bins[i] = 0;
    __syncthreads();

    const int64_t t0 = target[(long long)b * N];
    int cat = -1;
    if (t0 >= 0 && t0 < P) cat = part_cat[t0];
    int lo = 0, cnt = 0;
    if (cat >= 0 && cat < C) {
        lo = cat_range[2 * cat];
        cnt = cat_range[2 * cat + 1];
        if (lo < 0 || cnt < 1 || lo + cnt > P) cnt = 0;
    }
    const bool counted = b < n_valid && cnt > 0;        // an invalid shape: upp_seg_iou_accumulate counts it, its pred is -1

    const int n = n0 + threadIdx.x;
    if (n < N) {
        const long long row = (long long)b * N + n;
        int64_t p = -1;
        if (cnt > 0) {
            const float *x = logp + row * ld + lo;
            float best = x[0];
            int bk = 0;
            for (int k = 1; k < cnt; ++k) {
                const float v = x[k];
                if (replaces(v, best)) { best = v; bk = k; }
            }
            p = lo + bk;
        }
        if (pred) pred[row] = p;
        if (counted) {
            const int64_t t = target[row];
            const bool hit = p == t;
            if (hit) atomicAdd(s_total, 1);
            if (t >= 0 && t < P) {
                atomicAdd(&s_seen[t], 1);
                if (hit) atomicAdd(&s_corr[t], 1);
            }
            atomicAdd(&s_pred[p - lo], 1);
            if (t >= lo && t < lo + cnt) {
                atomicAdd(&s_tgt[t - lo], 1);
                if (hit) atomicAdd(&s_inter[t - lo], 1);
            }
        }
    }
    __syncthreads();
    if (!counted) return;
    int32_t *g_shape = scratch + (long long)b * P;
    int32_t *g_part = scratch + 3 * BP;
    for (int i = threadIdx.x; i < 5 * P + 1; i += kBlock) {
        const int v = s_bins[i];
        if (v == 0) continue;
        if (i < 3 * P) {
            const int which = i / P, k = i - which * P;
            atomicAdd(g_shape + which * BP + k, v);
        } else {
            atomicAdd(g_part + (i - 3 * P), v);
        }
    }
}

// One workgroup, shapes in chunks of kBlock.  Thread j : the IoU of shape chunk + j (into LDS and shape_iou).  Thread c < C : category
// c's sum and count over the chunk's shapes, in shape order.  Thread l : the part counters.  Then every thread zeroes the scratch.
__global__ __launch_bounds__(kBlock) void seg_iou_accumulate_kernel(int32_t *__restrict__ scratch, const int64_t *__restrict__ target,
                                                                    const int32_t *__restrict__ part_cat,
                                                                    const int32_t *__restrict__ cat_range, int B, int N, int P, int C,
                                                                    int n_valid, double *__restrict__ shape_iou,
                                                                    int32_t *__restrict__ shape_cat, double *__restrict__ cat_sum,
                                                                    int64_t *__restrict__ cat_cnt, int64_t *__restrict__ part_seen,
                                                                    int64_t *__restrict__ part_correct, int64_t *__restrict__ counters) {
    __shared__ int s_invalid[kBlock];
    __shared__ double s_iou[kBlock];
    __shared__ int s_cat[kBlock];
    const int tid = threadIdx.x;
    const long long BP = (long long)B * P;
    const int32_t *g_inter = scratch, *g_pred = scratch + BP, *g_tgt = scratch + 2 * BP;
    int invalid = 0;
    double csum = tid < C ? cat_sum[tid] : 0.0;
    int64_t ccnt = 0;
    for (int base = 0; base < n_valid; base += kBlock) {
        const int b = base + tid;
        if (b < n_valid) {
            const int64_t t0 = target[(long long)b * N];
            int cat = -1, lo = 0, cnt = 0;
            if (t0 >= 0 && t0 < P) cat = part_cat[t0];
            if (cat >= 0 && cat < C) {
                lo = cat_range[2 * cat];
                cnt = cat_range[2 * cat + 1];
                if (lo < 0 || cnt < 1 || lo + cnt > P) cnt = 0;
            }
            double iou = __builtin_nan("");
            if (cnt == 0) {
                ++invalid;
                cat = -1;
            } else {
                double sum = 0.0;
                for (int k0 = 0; k0 < cnt; k0 += 8) {           // 8 parts' counts in flight, then the sum in part order
                    int I[8], U[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const long long at = (long long)b * P + k0 + j;
                        const bool in = k0 + j < cnt;
                        I[j] = in ? g_inter[at] : 0;
                        U[j] = in ? g_tgt[at] + g_pred[at] : 0;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (k0 + j >= cnt) break;
                        const int u = U[j] - I[j];
                        sum = __dadd_rn(sum, u == 0 ? 1.0 : __ddiv_rn((double)I[j], (double)u));
                    }
                }
                iou = __ddiv_rn(sum, (double)cnt);
            }
            shape_cat[b] = cat;
            shape_iou[b] = iou;
            s_cat[tid] = cat;
            s_iou[tid] = iou;
        }
        __syncthreads();
        if (tid < C) {
            const int m = min(kBlock, n_valid - base);
            for (int j = 0; j < m; ++j) {
                if (s_cat[j] != tid) continue;
                csum = __dadd_rn(csum, s_iou[j]);
                ++ccnt;
            }
        }
        __syncthreads();
    }
    if (tid < C) {
        cat_sum[tid] = csum;
        cat_cnt[tid] += ccnt;
    }
    s_invalid[tid] = invalid;
    const int32_t *g_seen = scratch + 3 * BP, *g_corr = g_seen + P;
    for (int l = tid; l < P; l += kBlock) {
        part_seen[l] += g_seen[l];
        part_correct[l] += g_corr[l];
    }
    __syncthreads();
    if (tid == 0) {
        long long bad = 0;
        for (int w = 0; w < kBlock; ++w) bad += s_invalid[w];
        counters[0] += g_seen[2 * P];
        counters[1] += (int64_t)n_valid * N;
        counters[2] += bad;
    }
    __syncthreads();                    // every read of the scratch is done
    const long long total = 3 * BP + 2 * (long long)P + 1;
    for (long long i = tid; i < total; i += kBlock) scratch[i] = 0;
}

}  // namespace

extern "C" int upp_seg_iou_counts(const float *logp, long long ld, const int64_t *target, const int32_t *part_cat,
                                  const int32_t *cat_range, int B, int N, int P, int C, int n_valid, int64_t *pred, int32_t *scratch,
                                  void *stream) {
    if (!logp || !target || !part_cat || !cat_range || !scratch || B < 1 || N < 1 || P < 1 || C < 1 || ld < P) return UPP_E_BADARG;
    if (P > kMaxParts || C > kBlock || n_valid < 0 || n_valid > B || B > 65535 || (long long)B * N > 0x7fffffffLL) return UPP_E_RANGE;
    const dim3 grid((N + kPoints - 1) / kPoints, B);
    hipLaunchKernelGGL(seg_iou_counts_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, logp, ld, target, part_cat, cat_range, N, P, C,
                       n_valid, pred, scratch, B);
    return upp_launch_status();
}

extern "C" int upp_seg_iou_accumulate(int32_t *scratch, const int64_t *target, const int32_t *part_cat, const int32_t *cat_range, int B,
                                      int N, int P, int C, int n_valid, double *shape_iou, int32_t *shape_cat, double *cat_sum,
                                      int64_t *cat_cnt, int64_t *part_seen, int64_t *part_correct, int64_t *counters, void *stream) {
    if (!scratch || !target || !part_cat || !cat_range || !shape_iou || !shape_cat || !cat_sum || !cat_cnt || !part_seen ||
        !part_correct || !counters || B < 1 || N < 1 || P < 1 || C < 1)
        return UPP_E_BADARG;
    if (P > kMaxParts || C > kBlock || n_valid < 0 || n_valid > B || B > 65535 || (long long)B * N > 0x7fffffffLL) return UPP_E_RANGE;
    hipLaunchKernelGGL(seg_iou_accumulate_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, scratch, target, part_cat, cat_range, B,
                       N, P, C, n_valid, shape_iou, shape_cat, cat_sum, cat_cnt, part_seen, part_correct, counters);
    return upp_launch_status();
}
