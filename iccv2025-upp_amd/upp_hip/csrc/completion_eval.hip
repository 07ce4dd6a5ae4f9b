// completion_eval.hip -- the point-completion metrics of the reference's pre-task `validate` (tools/runner_pretask.py:314-426,
// utils/metrics.py:48-111) on the device, so no per-point distance leaves it (utils/evaluate.py CompletionMetric,
// upp_hip/infer.py CompletionEvalStep).  The nearest neighbours come from upp_chamfer_fwd; these kernels only reduce them:
//   * upp_completion_cloud_metrics : one workgroup per cloud pair.  float64 means of d1, d2, sqrt d1, sqrt d2 (strided per-thread sums,
//                                    then a fixed LDS tree: bit-identical from run to run); with `detail` also the F-Score counts
//                                    (the Chamfer partner's distance recomputed in float64, sqrt(d) < th), F, and whether a point of
//                                    either cloud has the f32 coordinate sum (x + y) + z == 0 (the ignore_zeros rule of the metric CDs).
//   * upp_completion_masked_cd     : the ignore_zeros CDs of the flagged pairs: a brute-force nearest-neighbour search that skips the
//                                    zero-sum points of both clouds.  Each workgroup reads its pair's flag on the device and returns at
//                                    once when it is 0: no host sync, capturable, one near-empty launch in the common case.
//   * upp_completion_accumulate    : one workgroup adds the per-(cloud, viewpoint) rows of the real clouds into the run's sums in the
//                                    reference's order (cloud-major, then viewpoint), sequentially, in float64.
// The per-cloud rows are written whole by every launch (nothing is accumulated into them), so there is no scratch to clear and no
// memset.  Wave64, vector stores only, no atomics.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kStat = 8;        // doubles per cloud row: mean d1, mean d2, mean sqrt d1, mean sqrt d2, F, CDL1, CDL2, 0
constexpr int kCount = 4;       // int32 per cloud row: precision count, recall count, has a zero-sum point, 0

__device__ __forceinline__ bool zero_sum(const float *p) { return (p[0] + p[1]) + p[2] == 0.0f; }

// Euclidean distance in float64 from f32 coordinates, as a float64 KD-tree over them computes it: ((dx dx + dy dy) + dz dz), sqrt.
__device__ __forceinline__ double dist64(const float *a, const float *b) {
    const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
}

// Fixed-shape tree over kBlock values (the same shape on every run: deterministic).
__device__ __forceinline__ void tree_sum(double *s, int tid) {
#pragma unroll
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (tid < w) s[tid] = __dadd_rn(s[tid], s[tid + w]);
        __syncthreads();
    }
}
__device__ __forceinline__ void tree_sum(int *s, int tid) {
#pragma unroll
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
}

// One direction of one pair: sums of d and sqrt d (float64) over this thread's points, the F-Score count, the zero-sum flag.
__device__ __forceinline__ void direction(const float *__restrict__ self, const float *__restrict__ other, const float *__restrict__ dist,
                                          const int32_t *__restrict__ idx, int n, int m, double th, bool detail, int tid, double &sd,
                                          double &sq, int &hits, int &zero) {
    sd = 0.0; sq = 0.0; hits = 0;
    for (int i = tid; i < n; i += kBlock) {
        const double d = (double)dist[i];
        sd = __dadd_rn(sd, d);
        sq = __dadd_rn(sq, sqrt(d));
        if (detail) {
            const float *p = self + (size_t)i * 3;
            const int j = idx[i];
            if (j >= 0 && j < m && dist64(p, other + (size_t)j * 3) < th) ++hits;
            zero |= zero_sum(p) ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(kBlock) void completion_cloud_metrics_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                                          const float *__restrict__ dist1, const int32_t *__restrict__ idx1,
                                                                          const float *__restrict__ dist2, const int32_t *__restrict__ idx2,
                                                                          int n, int m, double th, int detail, double *__restrict__ stats,
                                                                          int32_t *__restrict__ counts) {
    __shared__ double s_d[4][kBlock];
    __shared__ int s_i[3][kBlock];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *p1 = xyz1 + (size_t)b * n * 3, *p2 = xyz2 + (size_t)b * m * 3;
    int zero = 0, h1, h2;
    double s1, q1, s2, q2;
    direction(p1, p2, dist1 + (size_t)b * n, idx1 + (size_t)b * n, n, m, th, detail != 0, tid, s1, q1, h1, zero);
    direction(p2, p1, dist2 + (size_t)b * m, idx2 + (size_t)b * m, m, n, th, detail != 0, tid, s2, q2, h2, zero);
    s_d[0][tid] = s1; s_d[1][tid] = s2; s_d[2][tid] = q1; s_d[3][tid] = q2;
    s_i[0][tid] = h1; s_i[1][tid] = h2; s_i[2][tid] = zero;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) tree_sum(s_d[k], tid);
#pragma unroll
    for (int k = 0; k < 3; ++k) tree_sum(s_i[k], tid);
    if (tid == 0) {
        const double md1 = __ddiv_rn(s_d[0][0], (double)n), md2 = __ddiv_rn(s_d[1][0], (double)m);
        const double mq1 = __ddiv_rn(s_d[2][0], (double)n), mq2 = __ddiv_rn(s_d[3][0], (double)m);
        double f = 0.0;
        if (detail) {                    // utils/metrics.py:73-79: 2 * recall * precision / (recall + precision) if recall + precision else 0
            const double prec = __ddiv_rn((double)s_i[0][0], (double)n), rec = __ddiv_rn((double)s_i[1][0], (double)m);
            const double den = __dadd_rn(rec, prec);
            f = den != 0.0 ? __ddiv_rn(__dmul_rn(__dmul_rn(2.0, rec), prec), den) : 0.0;
        }
        double *o = stats + (size_t)b * kStat;
        o[0] = md1; o[1] = md2; o[2] = mq1; o[3] = mq2; o[4] = f;
        o[5] = __ddiv_rn(__dadd_rn(mq1, mq2), 2.0);           // the ignore_zeros CDs: these unless the masked pass replaces them
        o[6] = __dadd_rn(md1, md2);
        o[7] = 0.0;
        int32_t *c = counts + (size_t)b * kCount;
        c[0] = detail ? s_i[0][0] : 0;
        c[1] = detail ? s_i[1][0] : 0;
        c[2] = (detail && s_i[2][0] != 0) ? 1 : 0;
        c[3] = 0;
    }
}

// One direction of the masked search: per non-zero-sum point of `self` the f32 squared distance to the nearest non-zero-sum point of
// `other` (sumsq3, upp_chamfer_fwd's arithmetic), summed in float64 with its sqrt; `cnt` the points that took part.
__device__ __forceinline__ void masked_direction(const float *__restrict__ self, const float *__restrict__ other, int n, int m, int tid,
                                                 double &sd, double &sq, int &cnt) {
    sd = 0.0; sq = 0.0; cnt = 0;
    for (int i = tid; i < n; i += kBlock) {
        const float *p = self + (size_t)i * 3;
        if (zero_sum(p)) continue;
        const float x = p[0], y = p[1], z = p[2];
        float best = __builtin_inff();
        for (int j = 0; j < m; ++j) {
            const float *q = other + (size_t)j * 3;
            const float ox = q[0], oy = q[1], oz = q[2];
            if ((ox + oy) + oz == 0.0f) continue;
            const float d = sumsq3(ox - x, oy - y, oz - z);
            best = d < best ? d : best;
        }
        sd = __dadd_rn(sd, (double)best);
        sq = __dadd_rn(sq, sqrt((double)best));
        ++cnt;
    }
}

__global__ __launch_bounds__(kBlock) void completion_masked_cd_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2, int n,
                                                                      int m, const int32_t *__restrict__ counts, double *__restrict__ stats) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (counts[(size_t)b * kCount + 2] == 0) return;          // (uniform per workgroup: no zero-sum point, the unmasked CDs stand)
    __shared__ double s_d[4][kBlock];
    __shared__ int s_i[2][kBlock];
    const float *p1 = xyz1 + (size_t)b * n * 3, *p2 = xyz2 + (size_t)b * m * 3;
    double s1, q1, s2, q2;
    int c1, c2;
    masked_direction(p1, p2, n, m, tid, s1, q1, c1);
    masked_direction(p2, p1, m, n, tid, s2, q2, c2);
    s_d[0][tid] = s1; s_d[1][tid] = s2; s_d[2][tid] = q1; s_d[3][tid] = q2;
    s_i[0][tid] = c1; s_i[1][tid] = c2;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) tree_sum(s_d[k], tid);
#pragma unroll
    for (int k = 0; k < 2; ++k) tree_sum(s_i[k], tid);
    if (tid == 0) {
        double *o = stats + (size_t)b * kStat;
        const int n1 = s_i[0][0], n2 = s_i[1][0];
        if (n1 == 0 || n2 == 0) {                             // a cloud left without points: torch.mean of an empty tensor
            o[5] = __builtin_nan("");
            o[6] = __builtin_nan("");
        } else {
            const double md1 = __ddiv_rn(s_d[0][0], (double)n1), md2 = __ddiv_rn(s_d[1][0], (double)n2);
            const double mq1 = __ddiv_rn(s_d[2][0], (double)n1), mq2 = __ddiv_rn(s_d[3][0], (double)n2);
            o[5] = __ddiv_rn(__dadd_rn(mq1, mq2), 2.0);
            o[6] = __dadd_rn(md1, md2);
        }
    }
}

// One workgroup.  Threads 0-3: the four loss sums (x 1000), thread 4: the counters; threads c (strided): category c's sums of F,
// CDL1 x 1000 and CDL2 x 1000.  Every sum runs over cloud b < n_valid, then viewpoint v (row v B + b), sequentially.
__global__ __launch_bounds__(kBlock) void completion_accumulate_kernel(const double *__restrict__ sparse, const double *__restrict__ dense,
                                                                       const int64_t *__restrict__ category, int V, int B, int C,
                                                                       int n_valid, double *__restrict__ loss_sum,
                                                                       int64_t *__restrict__ counters, double *__restrict__ cat_sum,
                                                                       int64_t *__restrict__ cat_cnt) {
    const int tid = threadIdx.x;
    if (tid < 4) {
        const double *s = tid < 2 ? sparse : dense;
        const bool l1 = (tid & 1) == 0;
        double acc = loss_sum[tid];
        for (int b = 0; b < n_valid; ++b)
            for (int v = 0; v < V; ++v) {
                const double *r = s + ((size_t)v * B + b) * kStat;
                const double loss = l1 ? __ddiv_rn(__dadd_rn(r[2], r[3]), 2.0) : __dadd_rn(r[0], r[1]);
                acc = __dadd_rn(acc, __dmul_rn(loss, 1000.0));
            }
        loss_sum[tid] = acc;
    } else if (tid == 4) {
        long long bad = 0;
        if (category)
            for (int b = 0; b < n_valid; ++b) bad += (category[b] < 0 || category[b] >= C) ? 1 : 0;
        counters[0] += (int64_t)n_valid * V;
        counters[1] += bad * V;
    }
    if (!category) return;
    for (int c = tid; c < C; c += kBlock) {
        double f = cat_sum[(size_t)c * 3], l1 = cat_sum[(size_t)c * 3 + 1], l2 = cat_sum[(size_t)c * 3 + 2];
        long long cnt = 0;
        for (int b = 0; b < n_valid; ++b) {
            if (category[b] != c) continue;
            for (int v = 0; v < V; ++v) {
                const double *r = dense + ((size_t)v * B + b) * kStat;
                f = __dadd_rn(f, r[4]);
                l1 = __dadd_rn(l1, __dmul_rn(r[5], 1000.0));
                l2 = __dadd_rn(l2, __dmul_rn(r[6], 1000.0));
                ++cnt;
            }
        }
        cat_sum[(size_t)c * 3] = f;
        cat_sum[(size_t)c * 3 + 1] = l1;
        cat_sum[(size_t)c * 3 + 2] = l2;
        cat_cnt[c] += cnt;
    }
}

constexpr int kMaxRows = 1 << 20;          // clouds per call
constexpr int kMaxPoints = 1 << 22;        // points per cloud
constexpr int kMaxCategories = 4096;
constexpr int kMaxViews = 64;

}  // namespace

extern "C" int upp_completion_cloud_metrics(const float *xyz1, const float *xyz2, const float *dist1, const int32_t *idx1,
                                            const float *dist2, const int32_t *idx2, int B, int n, int m, double th, int detail,
                                            double *stats, int32_t *counts, void *stream) {
    if (!xyz1 || !xyz2 || !dist1 || !idx1 || !dist2 || !idx2 || !stats || !counts || B < 1 || n < 1 || m < 1) return UPP_E_BADARG;
    if (!(th > 0.0) || th == __builtin_inf() || (detail != 0 && detail != 1)) return UPP_E_BADARG;
    if (B > kMaxRows || n > kMaxPoints || m > kMaxPoints) return UPP_E_RANGE;
    hipLaunchKernelGGL(completion_cloud_metrics_kernel, dim3(B), dim3(kBlock), 0, (hipStream_t)stream, xyz1, xyz2, dist1, idx1, dist2,
                       idx2, n, m, th, detail, stats, counts);
    return upp_launch_status();
}

extern "C" int upp_completion_masked_cd(const float *xyz1, const float *xyz2, int B, int n, int m, const int32_t *counts, double *stats,
                                        void *stream) {
    if (!xyz1 || !xyz2 || !counts || !stats || B < 1 || n < 1 || m < 1) return UPP_E_BADARG;
    if (B > kMaxRows || n > kMaxPoints || m > kMaxPoints) return UPP_E_RANGE;
    hipLaunchKernelGGL(completion_masked_cd_kernel, dim3(B), dim3(kBlock), 0, (hipStream_t)stream, xyz1, xyz2, n, m, counts, stats);
    return upp_launch_status();
}

extern "C" int upp_completion_accumulate(const double *sparse, const double *dense, const int64_t *category, int V, int B, int C,
                                         int n_valid, double *loss_sum, int64_t *counters, double *cat_sum, int64_t *cat_cnt,
                                         void *stream) {
    if (!sparse || !dense || !loss_sum || !counters || V < 1 || B < 1) return UPP_E_BADARG;
    if (category && (!cat_sum || !cat_cnt || C < 1)) return UPP_E_BADARG;
    if (V > kMaxViews || (long long)V * B > kMaxRows || C > kMaxCategories || n_valid < 0 || n_valid > B) return UPP_E_RANGE;
    hipLaunchKernelGGL(completion_accumulate_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, sparse, dense, category, V, B,
                       category ? C : 0, n_valid, loss_sum, counters, cat_sum, cat_cnt);
    return upp_launch_status();
}
