// knn_points.hip -- pytorch3d.ops.knn_points / knn_gather for gfx950 (include/upp_hip.h "the pytorch3d.ops surface").
//
// Forward: knn.hip's mapping for points of any dimension 1 <= D <= 32 and both norms.  One wavefront per query, four per workgroup; the
// cloud p2 is staged through the LDS in chunks shared by the four waves, transposed to [d][point] so that a lane per point reads
// consecutive words (conflict-free) in every step of the d loop; the chunk length follows from D (12,288 floats of LDS: 4,096 points at
// D = 3, 384 at D = 32).  The query's coordinates sit one per lane and reach the d loop through v_readlane, so no per-lane array is
// indexed at run time (nothing in scratch).  The K best are knn.hip's lane-resident sorted list (lane j = j-th nearest), a survivor is
// inserted with one DPP wave shift: before the first strictly greater entry, so the order is ascending (distance, index).  The lengths
// are read by the kernel (int64 on the device, clamped to [0, P]): no host read-back, and every output element -- padding included -- is
// written here, nothing is zero-filled by the caller.  No prefilter pass: its second sweep over the cloud costs D LDS reads per point,
// the insertions it saves do not grow with D.
//
// Backward: g_p1 and the per-slot terms t by one thread per (cloud, query, coordinate); g_p2 (and knn_gather's gradient) by a row
// scatter-add, either f32 atomics into an array this file zeroes with a kernel, or det_scan.h's ordered pull.
#include "common.h"
#include "det_scan.h"

namespace {

constexpr int kKpWaves = 4;
constexpr int kKpFloats = 12288;          // floats of one staged chunk (48 KiB); + kKpPad for the row padding below
constexpr int kKpPad = 64;
constexpr int kKpMaxD = 32, kKpMaxK = 64;
constexpr int kBlock = 256;
constexpr long long kGridCap = 65535LL * 16;

// points per chunk and the row stride of the [d][point] image.  The stride's low bits spread the D rows over the banks for the staging
// WRITES (32 consecutive floats of p2 are 32 / D points x D rows); the reads are consecutive words whatever the stride.
__host__ __device__ static inline int kp_chunk(int D) { return (kKpFloats / D) & ~63; }
__host__ __device__ static inline int kp_stride(int D) { return kp_chunk(D) + (D > 1 ? (32 + D - 1) / D : 0); }

__device__ __forceinline__ int kp_len(const int64_t *lengths, int b, int P) {
    if (!lengths) return P;
    const int64_t v = lengths[b];
    return v < 0 ? 0 : (v > (int64_t)P ? P : (int)v);
}

template <int NORM>
__global__ __launch_bounds__(64 * kKpWaves) void knn_points_kernel(const float *__restrict__ p1, const float *__restrict__ p2,
                                                                   const int64_t *__restrict__ lengths1, const int64_t *__restrict__ lengths2,
                                                                   float *__restrict__ dists, int64_t *__restrict__ idx,
                                                                   float *__restrict__ nn, int P1, int P2, int D, int K) {
    __shared__ float chunk[kKpFloats + kKpPad];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int tile_x, b;
    xcd_cloud_tile(tile_x, b);                            // whole clouds per XCD, as knn_kernel
    const int len1 = kp_len(lengths1, b, P1), len2 = kp_len(lengths2, b, P2);
    const int q_raw = tile_x * kKpWaves + wave;
    const bool q_live = q_raw < P1;
    const int q = q_live ? q_raw : P1 - 1;                // surplus waves shadow the last query (they must reach the barriers)
    const float *rp = p2 + (size_t)b * P2 * D;
    const float qv = lane < D ? p1[((size_t)b * P1 + q) * D + lane] : 0.0f;      // coordinate `lane` of the query
    const int CH = kp_chunk(D), ST = kp_stride(D);

    uint32_t ld = 0xFFFFFFFFu;  // lane j: distance bits of the j-th nearest so far
    uint32_t lr = 0;            //         its index in p2
    uint32_t thr = 0xFFFFFFFFu; // bits of the K-th entry

    // rows past lengths1 are padding: a workgroup that holds nothing else skips the search (uniform over the workgroup)
    const int n2 = tile_x * kKpWaves < len1 ? len2 : 0;
    const int q256 = (64 * kKpWaves) / D, r256 = (64 * kKpWaves) - q256 * D;
    for (int c0 = 0; c0 < n2; c0 += CH) {
        const int len = min(CH, n2 - c0);
        __syncthreads();
        {   // p2[c0 .. c0 + len) -> chunk[d][point]: coalesced reads, (point, d) of flat element i advanced without a division per element
            const float *src = rp + (size_t)c0 * D;
            const int n = len * D;
            int pt = (int)threadIdx.x / D, dd = (int)threadIdx.x - pt * D;
            for (int i0 = threadIdx.x; i0 < n; i0 += 64 * kKpWaves * 4) {
                float t[4];
                int at[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u * 64 * kKpWaves;
                    t[u] = i < n ? src[i] : 0.0f;
                    at[u] = dd * ST + pt;
                    pt += q256; dd += r256;
                    if (dd >= D) { dd -= D; ++pt; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i0 + u * 64 * kKpWaves < n) chunk[at[u]] = t[u];
            }
        }
        __syncthreads();
        for (int s0 = 0; s0 < len; s0 += 64) {
            const int r = s0 + lane;
            const int rc = r < len ? r : len - 1;
            float acc = 0.0f;
            for (int d = 0; d < D; ++d) {
                const float diff = chunk[d * ST + rc] - __uint_as_float(readlane_u32(__float_as_uint(qv), d));
                acc = NORM == 2 ? __builtin_fmaf(diff, diff, acc) : __fadd_rn(acc, __builtin_fabsf(diff));
            }
            const uint32_t db = r < len ? __float_as_uint(acc) : 0xFFFFFFFFu;
            unsigned long long mask = __ballot(db < thr);
            while (mask) {
                const int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                const uint32_t dc = readlane_u32(db, l);
                if (dc < thr) {  // re-test: thr shrinks while the batch is consumed
                    const uint32_t rn = (uint32_t)(c0 + s0 + l);
                    const uint32_t ld_left = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ld, DPP_WAVE_SHR1, 0xF, 0xF, false);
                    const uint32_t lr_left = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lr, DPP_WAVE_SHR1, 0xF, 0xF, false);
                    const bool gt = ld > dc;            // my entry moves up one lane
                    const bool gtl = ld_left > dc;      // so does my left neighbour's (lane 0: 0 > dc is false)
                    ld = gt ? (gtl ? ld_left : dc) : ld;
                    lr = gt ? (gtl ? lr_left : rn) : lr;
                    thr = readlane_u32(ld, K - 1);
                }
            }
        }
    }

    if (!q_live) return;
    // slot k is filled when the query is a real row and the list reached it (k < min(K, lengths2): an unfilled entry keeps all-ones bits)
    const bool row = q < len1;
    const bool filled = row && ld != 0xFFFFFFFFu;
    const size_t o = ((size_t)b * P1 + q) * K;
    if (lane < K) {
        idx[o + lane] = filled ? (int64_t)lr : 0;
        dists[o + lane] = filled ? __uint_as_float(ld) : 0.0f;
    }
    if (nn) {
        for (int k = 0; k < K; ++k) {
            const uint32_t j = readlane_u32(lr, k);
            const bool f = row && readlane_u32(ld, k) != 0xFFFFFFFFu;          // (uniform)
            if (lane < D) nn[(o + k) * D + lane] = f ? rp[(size_t)j * D + lane] : 0.0f;
        }
    }
}

// g_p1[n][i][d] = +0.0f, then + t[n][i][k][d] in ascending k;  t = (2 g) * diff (norm 2) or sign(diff) * g (norm 1), diff = p1 - p2[idx],
// 0.0f in padded slots (and where an index handed in lies outside [0, P2)).  One thread per (n, i, d).
template <int NORM>
__global__ __launch_bounds__(kBlock) void knn_points_bwd_kernel(const float *__restrict__ p1, const float *__restrict__ p2,
                                                                const int64_t *__restrict__ idx, const float *__restrict__ grad_dists,
                                                                const int64_t *__restrict__ lengths1, const int64_t *__restrict__ lengths2,
                                                                float *__restrict__ g_p1, float *__restrict__ t, int P1, int P2, int D, int K,
                                                                long long total) {
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long long)gridDim.x * kBlock) {
        const int d = (int)(e % D);
        const long long ni = e / D;
        const int i = (int)(ni % P1), b = (int)(ni / P1);
        const int kv = kp_len(lengths1, b, P1) > i ? min(K, kp_len(lengths2, b, P2)) : 0;
        const float x = p1[e];
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) {
            float tv = 0.0f;
            if (k < kv) {
                const int64_t j = idx[ni * K + k];
                if (j >= 0 && j < (int64_t)P2) {
                    const float diff = x - p2[((size_t)b * P2 + (size_t)j) * D + d];
                    const float g = grad_dists[ni * K + k];
                    if (NORM == 2) tv = __fmul_rn(__fmul_rn(2.0f, g), diff);
                    else tv = diff > 0.0f ? g : (diff < 0.0f ? -g : 0.0f);
                    acc = __fadd_rn(acc, tv);
                }
            }
            t[(ni * K + k) * D + d] = tv;
        }
        g_p1[e] = acc;
    }
}

// slot (l, k) of cloud b takes part when l < rows[b] and k < slots[b] (either list may be absent) and its index lies in [0, M)
__device__ __forceinline__ bool kp_slot(const int64_t *rows, const int64_t *slots, int b, int l, int k, int L, int K) {
    return l < kp_len(rows, b, L) && k < kp_len(slots, b, K);
}

__global__ __launch_bounds__(kBlock) void knn_gather_kernel(const float *__restrict__ x, const int64_t *__restrict__ idx,
                                                            const int64_t *__restrict__ lengths, float *__restrict__ out, int M, int L, int K,
                                                            int U, long long total) {
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long long)gridDim.x * kBlock) {
        const int u = (int)(e % U);
        const long long s = e / U;
        const int k = (int)(s % K);
        const int b = (int)(s / ((long long)L * K));
        const int64_t j = idx[s];
        const bool ok = k < kp_len(lengths, b, K) && j >= 0 && j < (int64_t)M;
        out[e] = ok ? x[((size_t)b * M + (size_t)j) * U + u] : 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void knn_scatter_add_kernel(const float *__restrict__ src, const int64_t *__restrict__ idx,
                                                                 const int64_t *__restrict__ rows, const int64_t *__restrict__ slots,
                                                                 float *__restrict__ out, int M, int L, int K, int U, int negate,
                                                                 long long total) {
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long long)gridDim.x * kBlock) {
        const int u = (int)(e % U);
        const long long s = e / U;
        const int k = (int)(s % K);
        const long long bl = s / K;
        const int l = (int)(bl % L), b = (int)(bl / L);
        const int64_t j = idx[s];
        if (kp_slot(rows, slots, b, l, k, L, K) && j >= 0 && j < (int64_t)M) {
            const float v = src[e];
            atomicAdd(&out[((size_t)b * M + (size_t)j) * U + u], negate ? -v : v);
        }
    }
}

// out[b][r][u] = +0.0f, then + (or -) src[b][l][k][u] for every (l, k) that takes part and has idx[b][l][k] == r, in ascending l * K + k
// (include/upp_hip.h): a job of det_scan.h's det_scatter_kernel.  As GatherJob (group.hip) a workgroup owns 256 target rows of one cloud
// and kDetCh of the U columns.
struct KnnScatterJob {
    const float *__restrict__ src;
    const int64_t *__restrict__ idx;
    const int64_t *__restrict__ rows;
    const int64_t *__restrict__ slots;
    float *__restrict__ out;
    int B, M, L, K, U, negate;
    struct Item : DetItem { const int64_t *ib; const float *sb; int nrows, nslots; };          // (the cloud's idx and src)
    __host__ __device__ long long items() const { return B * det_groups(U) * det_tiles(M); }
    __device__ __forceinline__ Item item(long long it) const {
        const DetItem w = det_item(it, U, M, (long long)L * K);
        return {w, idx + (size_t)w.b * w.S, src + (size_t)w.b * w.S * U, len_of(rows, w.b, L), len_of(slots, w.b, K)};
    }
    // kp_len() read through the constant address space, as a `const __restrict__` kernel argument is read (one scalar load an item):
    // nothing writes the lengths while a kernel runs, and `__restrict__` on a struct member does not tell the compiler so
    __device__ static __forceinline__ int len_of(const int64_t *lengths, long long b, int P) {
        if (!lengths) return P;
        const int64_t v = ((const __attribute__((address_space(4))) int64_t *)lengths)[b];
        return v < 0 ? 0 : (v > (int64_t)P ? P : (int)v);
    }
    __device__ __forceinline__ void first(const Item &, long long, float (&)[kDetCh]) const {}
    __device__ __forceinline__ void stage(const Item &w, long long c0, int i, int32_t &key, float *v) const {
        const long long s = c0 + i;
        const int64_t j = w.ib[s];
        const bool ok = (int)(s / K) < w.nrows && (int)(s % K) < w.nslots && j >= 0 && j < (int64_t)M;
        key = ok ? (int32_t)j : -1;
#pragma unroll
        for (int c = 0; c < kDetCh; ++c) {
            const float x = w.ch0 + c < U ? w.sb[(size_t)s * U + w.ch0 + c] : 0.0f;
            v[c] = negate ? -x : x;
        }
    }
    __device__ __forceinline__ void store(const Item &w, long long r, const float (&acc)[kDetCh]) const {
#pragma unroll
        for (int c = 0; c < kDetCh; ++c)
            if (w.ch0 + c < U) out[((size_t)w.b * M + r) * U + w.ch0 + c] = acc[c];
    }
};

// the shared argument checks of the gather / scatter entry points: (N, M, L, K, U)
static int kp_rows_args(const void *a, const void *b, const void *c, int N, int M, int L, int K, int U) {
    if (!a || !b || !c || N < 0 || M < 1 || L < 1 || K < 1 || U < 1) return UPP_E_BADARG;
    if ((long long)L * K > 0x7FFFFFFFLL || (long long)M * U > 0x7FFFFFFFLL) return UPP_E_RANGE;
    return 0;
}

}  // namespace

extern "C" int upp_knn_points(const float *p1, const float *p2, const int64_t *lengths1, const int64_t *lengths2, float *dists, int64_t *idx,
                              float *nn, int N, int P1, int P2, int D, int K, int norm, void *stream) {
    if (!p1 || !p2 || !dists || !idx || N < 0 || P1 < 1 || P2 < 1 || D < 1 || K < 1 || (norm != 1 && norm != 2)) return UPP_E_BADARG;
    if (D > kKpMaxD || K > kKpMaxK) return UPP_E_RANGE;
    if (N == 0) return 0;
    if (N > 65535) return UPP_E_RANGE;
    dim3 grid((P1 + kKpWaves - 1) / kKpWaves, N);
    hipStream_t st = (hipStream_t)stream;
    if (norm == 2)
        hipLaunchKernelGGL((knn_points_kernel<2>), grid, dim3(64 * kKpWaves), 0, st, p1, p2, lengths1, lengths2, dists, idx, nn, P1, P2, D, K);
    else
        hipLaunchKernelGGL((knn_points_kernel<1>), grid, dim3(64 * kKpWaves), 0, st, p1, p2, lengths1, lengths2, dists, idx, nn, P1, P2, D, K);
    return upp_launch_status();
}

extern "C" int upp_knn_points_bwd(const float *p1, const float *p2, const int64_t *idx, const float *grad_dists, const int64_t *lengths1,
                                  const int64_t *lengths2, float *g_p1, float *t, int N, int P1, int P2, int D, int K, int norm,
                                  void *stream) {
    if (!p1 || !p2 || !idx || !grad_dists || !g_p1 || !t || N < 0 || P1 < 1 || P2 < 1 || D < 1 || K < 1 || (norm != 1 && norm != 2))
        return UPP_E_BADARG;
    if (D > kKpMaxD || K > kKpMaxK) return UPP_E_RANGE;
    if (N == 0) return 0;
    const long long total = (long long)N * P1 * D;
    hipStream_t st = (hipStream_t)stream;
    if (norm == 2)
        hipLaunchKernelGGL((knn_points_bwd_kernel<2>), dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, st, p1, p2, idx, grad_dists, lengths1, lengths2,
                           g_p1, t, P1, P2, D, K, total);
    else
        hipLaunchKernelGGL((knn_points_bwd_kernel<1>), dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, st, p1, p2, idx, grad_dists, lengths1, lengths2,
                           g_p1, t, P1, P2, D, K, total);
    return upp_launch_status();
}

extern "C" int upp_knn_gather(const float *x, const int64_t *idx, const int64_t *lengths, float *out, int N, int M, int L, int K, int U,
                              void *stream) {
    const int rc = kp_rows_args(x, idx, out, N, M, L, K, U);
    if (rc) return rc;
    if (N == 0) return 0;
    const long long total = (long long)N * L * K * U;
    hipLaunchKernelGGL(knn_gather_kernel, dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, x, idx, lengths, out, M, L, K, U, total);
    return upp_launch_status();
}

extern "C" int upp_knn_scatter_add(const float *src, const int64_t *idx, const int64_t *rows, const int64_t *slots, float *out, int N, int M,
                                   int L, int K, int U, int negate, void *stream) {
    const int rc = kp_rows_args(src, idx, out, N, M, L, K, U);
    if (rc) return rc;
    if (N == 0) return 0;
    upp_zero_async(out, (long long)N * M * U, (hipStream_t)stream);
    const long long total = (long long)N * L * K * U;
    hipLaunchKernelGGL(knn_scatter_add_kernel, dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, src, idx, rows, slots, out, M, L, K,
                       U, negate ? 1 : 0, total);
    return upp_launch_status();
}

extern "C" int upp_knn_scatter_add_det(const float *src, const int64_t *idx, const int64_t *rows, const int64_t *slots, float *out, int N,
                                       int M, int L, int K, int U, int negate, void *stream) {
    const int rc = kp_rows_args(src, idx, out, N, M, L, K, U);
    if (rc) return rc;
    if (N == 0) return 0;
    det_launch<kDetCh>(KnnScatterJob{src, idx, rows, slots, out, N, M, L, K, U, negate ? 1 : 0}, stream);
    return upp_launch_status();
}
