// query_select.hip -- the query selection of AdaPoinTr for gfx950 (include/upp_hip.h "query selection"; reference
// models/AdaPoinTr.py:855-865: argsort of the ranking scores, expand, gather, cat with the denoising points).
//
// One workgroup per cloud, its scores as total-order images in the LDS, rank by counting (the order of upp_argsort_rows, descending);
// the backward builds the inverse map in the LDS and writes every row of g_cand once: no atomics, nothing is zeroed beforehand.
#include "common.h"

namespace {

constexpr int kQsMaxM = 4096;

// the total-order image of upp_argsort_rows: -0 == +0, NaN above +inf
__device__ __forceinline__ uint32_t qs_key(float v) {
    if (v != v) return 0xFFFFFFFFu;
    const uint32_t u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// blockIdx.x = cloud.  rank of i = how many j come before it (greater score, or equal score and lower index); the first Q ranks are kept
__global__ __launch_bounds__(256) void qs_fwd_kernel(const float *__restrict__ score, const float *__restrict__ cand,
                                                     const float *__restrict__ extra, float *__restrict__ out, int *__restrict__ order, int M,
                                                     int Q, int D) {
    __shared__ __attribute__((aligned(16))) uint32_t sk[kQsMaxM];
    const size_t b = blockIdx.x;
    const float *s = score + b * M;
    for (int i = threadIdx.x; i < M; i += 256) sk[i] = qs_key(s[i]);
    __syncthreads();
    const float *cb = cand + b * M * 3;
    float *ob = out + b * (size_t)(Q + D) * 3;
    for (int i = threadIdx.x; i < M; i += 256) {
        const uint32_t mine = sk[i];
        int rank = 0, j = 0;
        for (; j + 4 <= M; j += 4) {                          // (every lane reads the same address: LDS broadcast)
            const uint4 v = *reinterpret_cast<const uint4 *>(sk + j);
            rank += (v.x > mine || (v.x == mine && j < i)) + (v.y > mine || (v.y == mine && j + 1 < i)) +
                    (v.z > mine || (v.z == mine && j + 2 < i)) + (v.w > mine || (v.w == mine && j + 3 < i));
        }
        for (; j < M; ++j) rank += sk[j] > mine || (sk[j] == mine && j < i);
        if (rank < Q) {
            order[b * Q + rank] = i;
            ob[(size_t)rank * 3 + 0] = cb[(size_t)i * 3 + 0];
            ob[(size_t)rank * 3 + 1] = cb[(size_t)i * 3 + 1];
            ob[(size_t)rank * 3 + 2] = cb[(size_t)i * 3 + 2];
        }
    }
    if (D > 0) {
        const float *eb = extra + b * (size_t)D * 3;
        for (int i = threadIdx.x; i < D * 3; i += 256) ob[(size_t)Q * 3 + i] = eb[i];
    }
}

// blockIdx.x = cloud.  inv[i] = the rank that picked candidate i, or -1; every row of g_cand is written here, once
__global__ __launch_bounds__(256) void qs_bwd_kernel(const float *__restrict__ g_out, const int *__restrict__ order, float *__restrict__ g_cand,
                                                     float *__restrict__ g_extra, int M, int Q, int D) {
    __shared__ int inv[kQsMaxM];
    const size_t b = blockIdx.x;
    for (int i = threadIdx.x; i < M; i += 256) inv[i] = -1;
    __syncthreads();
    for (int r = threadIdx.x; r < Q; r += 256) {
        const int i = order[b * Q + r];
        if ((unsigned)i < (unsigned)M) inv[i] = r;             // (an index outside the cloud is dropped, never written through)
    }
    __syncthreads();
    const float *gb = g_out + b * (size_t)(Q + D) * 3;
    float *gc = g_cand + b * M * 3;
    for (int e = threadIdx.x; e < M * 3; e += 256) {
        const int i = e / 3, r = inv[i];
        gc[e] = r >= 0 ? gb[(size_t)r * 3 + (e - i * 3)] : 0.0f;
    }
    if (D > 0) {
        float *ge = g_extra + b * (size_t)D * 3;
        for (int i = threadIdx.x; i < D * 3; i += 256) ge[i] = gb[(size_t)Q * 3 + i];
    }
}

static int qs_args(int B, int M, int Q, int D) {
    if (B < 1 || M < 1 || Q < 1 || D < 0) return UPP_E_BADARG;
    if (M > kQsMaxM || Q > M || (long long)Q + D > 0x7FFFFFFFLL / 3 / B) return UPP_E_RANGE;
    return 0;
}

}  // namespace

extern "C" int upp_query_select_fwd(const float *score, const float *cand, const float *extra, float *out, int *order, int B, int M, int Q,
                                    int D, void *stream) {
    if (!score || !cand || !out || !order || (D > 0 && !extra)) return UPP_E_BADARG;
    const int rc = qs_args(B, M, Q, D);
    if (rc) return rc;
    hipLaunchKernelGGL(qs_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, score, cand, extra, out, order, M, Q, D);
    return upp_launch_status();
}

extern "C" int upp_query_select_bwd(const float *g_out, const int *order, float *g_cand, float *g_extra, int B, int M, int Q, int D,
                                    void *stream) {
    if (!g_out || !order || !g_cand || (D > 0 && !g_extra)) return UPP_E_BADARG;
    const int rc = qs_args(B, M, Q, D);
    if (rc) return rc;
    hipLaunchKernelGGL(qs_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, g_out, order, g_cand, g_extra, M, Q, D);
    return upp_launch_status();
}
