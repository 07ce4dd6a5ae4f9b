// group.hip -- index gathers of the grouping stage and their scatter-add backwards.
//
//  * upp_gather_fwd/bwd: pointnet2_ops gather_points_kernel / gather_points_grad_kernel
//    (sampling_gpu.cu), behind pointnet2_utils.gather_operation, reference utils/misc.py:19.
//  * upp_group_fwd/bwd: the torch indexing of Group.forward, reference
//    models/Point_MAE_unify.py:73-88 (flat gather + centre subtraction).
// All four are pure HBM-bound byte movers: flat grid-stride kernels, one
// element per lane, coalesced on the dense side.
#include "common.h"
#include "det_scan.h"

namespace {

constexpr int kBlock = 256;
constexpr long long kGridCap = 2048;  // 256 CUs x 8 blocks, grid-stride the rest

// out[b,c,j] = feat[b,c,idx[b,j]]
__global__ void gather_fwd_kernel(const float *__restrict__ feat, const int32_t *__restrict__ idx, float *__restrict__ out,
                                  int C, int N, int M, long long total) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int j = (int)(i % M);
        const long long bc = i / M;
        const long long b = bc / C;
        out[i] = feat[bc * N + idx[b * M + j]];
    }
}

// grad_feat[b,c,idx[b,j]] += grad_out[b,c,j]
__global__ void gather_bwd_kernel(const float *__restrict__ grad_out, const int32_t *__restrict__ idx,
                                  float *__restrict__ grad_feat, int C, int N, int M, long long total) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int j = (int)(i % M);
        const long long bc = i / M;
        const long long b = bc / C;
        atomicAdd(&grad_feat[bc * N + idx[b * M + j]], grad_out[i]);
    }
}

// out[b,g,k,c] = xyz[b, idx[b,g,k], c] - center[b,g,c]
__global__ void group_fwd_kernel(const float *__restrict__ xyz, const float *__restrict__ center,
                                 const int64_t *__restrict__ idx, float *__restrict__ out, int N, int G, int K,
                                 long long total) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int c = (int)(i % 3);
        const long long e = i / 3;            // (b,g,k)
        const long long bg = e / K;           // (b,g)
        const long long b = bg / G;
        const long long r = idx[e];
        out[i] = xyz[(b * N + r) * 3 + c] - center[bg * 3 + c];
    }
}

// grad_xyz[b, idx[b,g,k], c] += grad_out[b,g,k,c]
__global__ void group_bwd_xyz_kernel(const float *__restrict__ grad_out, const int64_t *__restrict__ idx,
                                     float *__restrict__ grad_xyz, int N, int G, int K, long long total) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int c = (int)(i % 3);
        const long long e = i / 3;
        const long long b = e / ((long long)G * K);
        const long long r = idx[e];
        atomicAdd(&grad_xyz[(b * N + r) * 3 + c], grad_out[i]);
    }
}

// grad_center[b,g,c] = -sum_k grad_out[b,g,k,c]   (k ascending: deterministic)
__global__ void group_bwd_center_kernel(const float *__restrict__ grad_out, float *__restrict__ grad_center, int K,
                                        long long total) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int c = (int)(i % 3);
        const long long bg = i / 3;
        float s = 0.0f;
        for (int k = 0; k < K; ++k) s += grad_out[(bg * K + k) * 3 + c];
        grad_center[i] = -s;
    }
}

// Backward of the FPS centre gather (reference utils/misc.py:19 gather_operation under autograd: stage 2 and the pre-task recipe, where the
// sampled coordinates carry a gradient): g_xyz (B,N,3) = 0 everywhere except rows idx[b][j], which receive g_centers[b][j].  ONE launch, one
// workgroup per cloud: the cloud's slice is zeroed, then the M rows are added -- torch.zeros + an int32 -> int64 index copy + the scatter
// kernel were three launches per FPS call.  FPS indices of a cloud are distinct unless it has fewer distinct points than samples; equal
// indices are added atomically (two addends commute exactly; three or more depend on order in the last bit, as torch's index_add does).
__global__ __launch_bounds__(256) void fps_gather_bwd_kernel(const float *__restrict__ g_centers, const int32_t *__restrict__ idx,
                                                             float *__restrict__ g_xyz, int N, int M) {
    const int b = blockIdx.x;
    float *gx = g_xyz + (size_t)b * N * 3;
    for (int i = threadIdx.x; i < N * 3; i += 256) gx[i] = 0.0f;
    __syncthreads();                                  // (the zeros of this workgroup's own slice are visible to its own atomics)
    for (int i = threadIdx.x; i < M * 3; i += 256) {
        const int j = i / 3, c = i - 3 * j;
        const int r = idx[(size_t)b * M + j];
        if (r >= 0 && r < N) atomicAdd(&gx[(size_t)r * 3 + c], g_centers[((size_t)b * M + j) * 3 + c]);
    }
}

// ---- the deterministic siblings (include/upp_hip.h "deterministic scatter-adds"): two jobs of det_scan.h's det_scatter_kernel -----------
// out[b][r][0..2] = +0.0f, then + val[b][s][0..2] for every source s with idx[b][s] == r, in ascending s: the xyz gradient of the grouping
// gather (IdxT = int64, s = g * K + k) and of the FPS centre gather (int32).  Every row is written (rows that nobody references: +0.0f),
// so the caller zero-fills nothing.  Indices outside [0, N) are skipped.
template <typename IdxT>
struct Rows3Job {
    const float *__restrict__ val;
    const IdxT *__restrict__ idx;
    float *__restrict__ out;
    int B, N;
    long long S;
    __host__ __device__ long long items() const { return B * det_tiles(N); }
    __device__ __forceinline__ DetItem item(long long it) const { return det_item(it, 1, N, S); }
    __device__ __forceinline__ void first(const DetItem &, long long, float (&)[3]) const {}
    __device__ __forceinline__ void stage(const DetItem &w, long long c0, int i, int32_t &key, float *v) const {
        const IdxT k = (idx + (size_t)w.b * S + c0)[i];
        key = (k >= 0 && k < (IdxT)N) ? (int32_t)k : -1;
        const float *p = val + ((size_t)w.b * S + c0) * 3 + i * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    }
    __device__ __forceinline__ void store(const DetItem &w, long long r, const float (&acc)[3]) const {
        float *o = out + ((size_t)w.b * N + r) * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
};

// grad_feat[b][ch][r] = +0.0f, then + grad_out[b][ch][j] for every j with idx[b][j] == r, in ascending j.  A workgroup owns 256 targets of
// one cloud and kDetCh channels: the key chunk it stages serves all of them.
struct GatherJob {
    const float *__restrict__ grad_out;
    const int32_t *__restrict__ idx;
    float *__restrict__ grad_feat;
    int B, C, N, M;
    __host__ __device__ long long items() const { return B * det_groups(C) * det_tiles(N); }
    __device__ __forceinline__ DetItem item(long long it) const { return det_item(it, C, N, M); }
    __device__ __forceinline__ void first(const DetItem &, long long, float (&)[kDetCh]) const {}
    __device__ __forceinline__ void stage(const DetItem &w, long long c0, int i, int32_t &key, float *v) const {
        const int s = (int)c0 + i;                                      // (M is an int)
        const int k = (idx + (size_t)w.b * M)[s];
        key = (k >= 0 && k < N) ? k : -1;
#pragma unroll
        for (int c = 0; c < kDetCh; ++c) v[c] = w.ch0 + c < C ? grad_out[((size_t)w.b * C + w.ch0 + c) * M + s] : 0.0f;
    }
    __device__ __forceinline__ void store(const DetItem &w, long long r, const float (&acc)[kDetCh]) const {
#pragma unroll
        for (int c = 0; c < kDetCh; ++c)
            if (w.ch0 + c < C) grad_feat[((size_t)w.b * C + w.ch0 + c) * N + r] = acc[c];
    }
};

}  // namespace

extern "C" int upp_gather_fwd(const float *feat, const int32_t *idx, float *out, int B, int C, int N, int M, void *stream) {
    if (!feat || !idx || !out || B < 0 || C < 0 || N < 1 || M < 0) return UPP_E_BADARG;
    const long long total = (long long)B * C * M;
    if (total == 0) return 0;
    hipLaunchKernelGGL(gather_fwd_kernel, dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, feat, idx, out, C, N, M, total);
    return upp_launch_status();
}

extern "C" int upp_gather_bwd(const float *grad_out, const int32_t *idx, float *grad_feat, int B, int C, int N, int M, void *stream) {
    if (!grad_out || !idx || !grad_feat || B < 0 || C < 0 || N < 1 || M < 0) return UPP_E_BADARG;
    const long long total = (long long)B * C * M;
    if (total == 0) return 0;
    hipLaunchKernelGGL(gather_bwd_kernel, dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, grad_out, idx, grad_feat, C, N, M, total);
    return upp_launch_status();
}

extern "C" int upp_fps_gather_bwd(const float *g_centers, const int32_t *idx, float *g_xyz, int B, int N, int M, void *stream) {
    if (!g_centers || !idx || !g_xyz || B < 0 || N < 1 || M < 0) return UPP_E_BADARG;
    if (B == 0) return 0;
    hipLaunchKernelGGL(fps_gather_bwd_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, g_centers, idx, g_xyz, N, M);
    return upp_launch_status();
}

extern "C" int upp_group_fwd(const float *xyz, const float *center, const int64_t *idx, float *out, int B, int N, int G, int K, void *stream) {
    if (!xyz || !center || !idx || !out || B < 0 || N < 1 || G < 0 || K < 0) return UPP_E_BADARG;
    const long long total = (long long)B * G * K * 3;
    if (total == 0) return 0;
    hipLaunchKernelGGL(group_fwd_kernel, dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, xyz, center, idx, out, N, G, K, total);
    return upp_launch_status();
}

extern "C" int upp_group_bwd(const float *grad_out, const int64_t *idx, float *grad_xyz, float *grad_center, int B, int N, int G, int K, void *stream) {
    if (!grad_out || !idx || B < 0 || N < 1 || G < 0 || K < 0) return UPP_E_BADARG;
    const long long total = (long long)B * G * K * 3;
    if (total == 0) return 0;
    if (grad_xyz)
        hipLaunchKernelGGL(group_bwd_xyz_kernel, dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, grad_out, idx, grad_xyz, N, G, K, total);
    if (grad_center) {
        const long long tc = (long long)B * G * 3;
        hipLaunchKernelGGL(group_bwd_center_kernel, dim3(grid_for(tc, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, grad_out, grad_center, K, tc);
    }
    return upp_launch_status();
}

extern "C" int upp_gather_bwd_det(const float *grad_out, const int32_t *idx, float *grad_feat, int B, int C, int N, int M, void *stream) {
    if (!grad_out || !idx || !grad_feat || B < 0 || C < 0 || N < 1 || M < 0) return UPP_E_BADARG;
    if (B == 0 || C == 0) return 0;
    det_launch<kDetCh>(GatherJob{grad_out, idx, grad_feat, B, C, N, M}, stream);
    return upp_launch_status();
}

extern "C" int upp_fps_gather_bwd_det(const float *g_centers, const int32_t *idx, float *g_xyz, int B, int N, int M, void *stream) {
    if (!g_centers || !idx || !g_xyz || B < 0 || N < 1 || M < 0) return UPP_E_BADARG;
    if (B == 0) return 0;
    det_launch<3>(Rows3Job<int32_t>{g_centers, idx, g_xyz, B, N, (long long)M}, stream);
    return upp_launch_status();
}

extern "C" int upp_group_bwd_det(const float *grad_out, const int64_t *idx, float *grad_xyz, float *grad_center, int B, int N, int G, int K,
                                 void *stream) {
    if (!grad_out || !idx || B < 0 || N < 1 || G < 0 || K < 0) return UPP_E_BADARG;
    if (B == 0) return 0;
    if (grad_xyz) det_launch<3>(Rows3Job<int64_t>{grad_out, idx, grad_xyz, B, N, (long long)G * K}, stream);
    const long long tc = (long long)B * G * 3;
    if (grad_center && tc > 0 && K > 0)            // (k ascending already: the sibling's kernel, launched as the sibling launches it)
        hipLaunchKernelGGL(group_bwd_center_kernel, dim3(grid_for(tc, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, grad_out, grad_center, K, tc);
    return upp_launch_status();
}
