// pointnet2.hip -- the rest of the pointnet2_ops operator surface for gfx950: ball_query, three_nn, three_interpolate and
// grouping_operation (pointnet2_ops 3.0.0: ball_query_gpu.cu, interpolate_gpu.cu, group_points_gpu.cu behind
// pointnet2_utils.ball_query / three_nn / three_interpolate / grouping_operation; the reference calls three_nn and three_interpolate
// from models/Transformer_utils.py:225-230).  The upstream CUDA sources were not available when this was written: the rules are
// RESTATED from them in include/upp_hip.h ("the pointnet2_ops surface"), as was done for FPS and kNN, and are unpinned until they can
// be compared with the CUDA kernels' output.
//
// Mapping of the two searches: one lane per query, 128 queries of one cloud per workgroup; the searched cloud goes through the LDS in
// tiles of 1,024 points stored as float4, and every lane reads the SAME point per step (one ds_read_b128, a broadcast: no bank
// conflict), in ascending index -- which is the order both rules are stated in.  ball_query stops early: a wave whose lanes all hold
// nsample indices skips the arithmetic, and the workgroup leaves the tile loop once both of its waves are done.
// Squared distances: sumsq3() of common.h on the f32 differences, the library's convention (oracle/upp_oracle.c).
//
// The two interpolation kernels and the channels-first scatter-adds are byte movers: flat grid-stride kernels, coalesced on the dense
// side.  grouping_operation IS gather_operation on the flattened (P S) index list -- upstream's two kernels differ in nothing else --
// so upp_grouping_* validate their own arguments and hand over to upp_gather_*.
#include "common.h"
#include "det_scan.h"

namespace {

constexpr int kQueries = 128;      // queries per workgroup, one per lane (2 waves)
constexpr int kTile = 1024;        // searched points per LDS tile (16 KiB as float4)
constexpr int kBlock = 256;        // the flat kernels
constexpr long long kGridCap = 2048;  // 256 CUs x 8 blocks, grid-stride the rest

// points [c0, c0 + len) of a (N,3) cloud -> tile[0 .. len) as (x, y, z, 0); 12 independent loads in flight per thread
__device__ __forceinline__ void stage_points(float4 *tile, const float *__restrict__ cloud, int c0, int len, int tid) {
    for (int i0 = tid; i0 < len; i0 += kQueries * 4) {
        float t[4][3];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = min(i0 + q * kQueries, len - 1);
            const float *s = cloud + (size_t)(c0 + i) * 3;
            t[q][0] = s[0]; t[q][1] = s[1]; t[q][2] = s[2];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * kQueries;
            if (i < len) tile[i] = make_float4(t[q][0], t[q][1], t[q][2], 0.0f);
        }
    }
}

// idx[b][j][0 .. nsample): the first nsample k (ascending) with |xyz[b][k] - new_xyz[b][j]|^2 < radius^2; the first hit fills every slot
// first, a query without a hit yields zeros.  Every slot is written here: nothing is zero-filled by the caller.
__global__ __launch_bounds__(kQueries) void ball_query_kernel(const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                              int32_t *__restrict__ idx, float r2, int nsample, int N, int P) {
    __shared__ __attribute__((aligned(16))) float4 tile[kTile];
    int tile_x, b;
    xcd_cloud_tile(tile_x, b);                            // whole clouds per XCD: the searched cloud is fetched into ONE L2
    const int j = tile_x * kQueries + (int)threadIdx.x;
    const bool live = j < P;
    const int jc = live ? j : P - 1;                      // surplus lanes shadow the last query and write nothing
    const float *q = new_xyz + ((size_t)b * P + jc) * 3;
    const float qx = q[0], qy = q[1], qz = q[2];
    const float *cloud = xyz + (size_t)b * N * 3;
    int32_t *out = idx + ((size_t)b * P + jc) * nsample;
    int cnt = live ? 0 : nsample;
    for (int c0 = 0; c0 < N; c0 += kTile) {
        if (!__syncthreads_or(cnt < nsample)) break;      // (also the barrier in front of the next staging)
        const int len = min(kTile, N - c0);
        stage_points(tile, cloud, c0, len, threadIdx.x);
        __syncthreads();
        for (int s0 = 0; s0 < len; s0 += 64) {
            if (__ballot(cnt < nsample) == 0) break;      // this wave is done: the other one may still need the tiles
            const int s1 = min(len, s0 + 64);
            for (int k = s0; k < s1; ++k) {
                const float4 p = tile[k];
                const float d2 = sumsq3(qx - p.x, qy - p.y, qz - p.z);
                if (d2 < r2 && cnt < nsample) {
                    if (cnt == 0)
                        for (int l = 0; l < nsample; ++l) out[l] = c0 + k;
                    out[cnt] = c0 + k;
                    ++cnt;
                }
            }
        }
    }
    if (live && cnt == 0)
        for (int l = 0; l < nsample; ++l) out[l] = 0;
}

// the three nearest known points of every unknown point: strict-'<' cascade over ascending k (equal distances keep the lower index
// first), bests start at +inf and indices at 0, dist = sqrtf(squared distance) (IEEE, correctly rounded)
__global__ __launch_bounds__(kQueries) void three_nn_kernel(const float *__restrict__ unknown, const float *__restrict__ known,
                                                            float *__restrict__ dist, int32_t *__restrict__ idx, int n, int m) {
    __shared__ __attribute__((aligned(16))) float4 tile[kTile];
    int tile_x, b;
    xcd_cloud_tile(tile_x, b);
    const int j = tile_x * kQueries + (int)threadIdx.x;
    const int jc = j < n ? j : n - 1;
    const float *u = unknown + ((size_t)b * n + jc) * 3;
    const float ux = u[0], uy = u[1], uz = u[2];
    const float *cloud = known + (size_t)b * m * 3;
    float b1 = __builtin_inff(), b2 = __builtin_inff(), b3 = __builtin_inff();
    int i1 = 0, i2 = 0, i3 = 0;
    for (int c0 = 0; c0 < m; c0 += kTile) {
        const int len = min(kTile, m - c0);
        __syncthreads();
        stage_points(tile, cloud, c0, len, threadIdx.x);
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < len; ++k) {
            const float4 p = tile[k];
            const float d = sumsq3(ux - p.x, uy - p.y, uz - p.z);
            const int kk = c0 + k;
            const bool lt1 = d < b1, lt2 = d < b2, lt3 = d < b3;
            b3 = lt2 ? b2 : (lt3 ? d : b3);
            i3 = lt2 ? i2 : (lt3 ? kk : i3);
            b2 = lt1 ? b1 : (lt2 ? d : b2);
            i2 = lt1 ? i1 : (lt2 ? kk : i2);
            b1 = lt1 ? d : b1;
            i1 = lt1 ? kk : i1;
        }
    }
    if (j < n) {
        const size_t o = ((size_t)b * n + j) * 3;
        dist[o + 0] = sqrtf(b1); dist[o + 1] = sqrtf(b2); dist[o + 2] = sqrtf(b3);
        idx[o + 0] = i1; idx[o + 1] = i2; idx[o + 2] = i3;
    }
}

// out[b][c][i] = (w0 * f[i0] + w1 * f[i1]) + w2 * f[i2]: three products and two sums, each rounded once (no fma).  An index outside
// [0, m) reads 0.0f.
__global__ void three_interpolate_fwd_kernel(const float *__restrict__ feat, const int32_t *__restrict__ idx, const float *__restrict__ weight,
                                             float *__restrict__ out, int C, int m, int n, long long total) {
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long long)gridDim.x * kBlock) {
        const int i = (int)(e % n);
        const long long bc = e / n;
        const long long b = bc / C;
        const int32_t *ip = idx + ((size_t)b * n + i) * 3;
        const float *wp = weight + ((size_t)b * n + i) * 3;
        const float *f = feat + (size_t)bc * m;
        float t[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int r = ip[q];
            t[q] = __fmul_rn(wp[q], (r >= 0 && r < m) ? f[r] : 0.0f);
        }
        out[e] = __fadd_rn(__fadd_rn(t[0], t[1]), t[2]);
    }
}

// grad_feat[b][c][idx[b][i][q]] += grad_out[b][c][i] * weight[b][i][q]   (f32 atomics into a caller-zeroed buffer)
__global__ void three_interpolate_bwd_kernel(const float *__restrict__ grad_out, const int32_t *__restrict__ idx, const float *__restrict__ weight,
                                             float *__restrict__ grad_feat, int C, int m, int n, long long total) {
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long long)gridDim.x * kBlock) {
        const int i = (int)(e % n);
        const long long bc = e / n;
        const long long b = bc / C;
        const int32_t *ip = idx + ((size_t)b * n + i) * 3;
        const float *wp = weight + ((size_t)b * n + i) * 3;
        const float g = grad_out[e];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int r = ip[q];
            if (r >= 0 && r < m) atomicAdd(&grad_feat[(size_t)bc * m + r], __fmul_rn(g, wp[q]));
        }
    }
}

// grad_feat[b][ch][r] = +0.0f, then + grad_out[b][ch][i] * weight[b][i][q] for every (i, q) with idx[b][i][q] == r, in ascending
// i * 3 + q (include/upp_hip.h "deterministic scatter-adds"): a job of det_scan.h's det_scatter_kernel.  As GatherJob (group.hip) a
// workgroup owns 256 targets of one cloud and kDetCh channels; the products are formed once per source while staging.
struct InterpolateJob {
    const float *__restrict__ grad_out;
    const int32_t *__restrict__ idx;
    const float *__restrict__ weight;
    float *__restrict__ grad_feat;
    int B, C, m, n;
    __host__ __device__ long long items() const { return B * det_groups(C) * det_tiles(m); }
    __device__ __forceinline__ DetItem item(long long it) const { return det_item(it, C, m, 3LL * n); }
    __device__ __forceinline__ void first(const DetItem &, long long, float (&)[kDetCh]) const {}
    __device__ __forceinline__ void stage(const DetItem &w, long long c0, int i, int32_t &key, float *v) const {
        const long long s = c0 + i;
        const int k = idx[(size_t)w.b * w.S + s];
        const float wt = weight[(size_t)w.b * w.S + s];
        key = (k >= 0 && k < m) ? k : -1;
#pragma unroll
        for (int c = 0; c < kDetCh; ++c)
            v[c] = w.ch0 + c < C ? __fmul_rn(grad_out[((size_t)w.b * C + w.ch0 + c) * n + s / 3], wt) : 0.0f;
    }
    __device__ __forceinline__ void store(const DetItem &w, long long r, const float (&acc)[kDetCh]) const {
#pragma unroll
        for (int c = 0; c < kDetCh; ++c)
            if (w.ch0 + c < C) grad_feat[((size_t)w.b * C + w.ch0 + c) * m + r] = acc[c];
    }
};

}  // namespace

extern "C" int upp_ball_query(const float *xyz, const float *new_xyz, float radius, int nsample, int32_t *idx, int B, int N, int P,
                              void *stream) {
    if (!xyz || !new_xyz || !idx || B < 0 || N < 1 || P < 1 || nsample < 1) return UPP_E_BADARG;
    if (!(radius > 0.0f) || !__builtin_isfinite(radius)) return UPP_E_BADARG;
    if (B == 0) return 0;
    if (B > 65535) return UPP_E_RANGE;
    const float r2 = radius * radius;                     // formed in f32 (-ffp-contract=off: one rounded product)
    hipLaunchKernelGGL(ball_query_kernel, dim3((P + kQueries - 1) / kQueries, B), dim3(kQueries), 0, (hipStream_t)stream, xyz, new_xyz, idx,
                       r2, nsample, N, P);
    return upp_launch_status();
}

extern "C" int upp_three_nn(const float *unknown, const float *known, float *dist, int32_t *idx, int B, int n, int m, void *stream) {
    if (!unknown || !known || !dist || !idx || B < 0 || n < 1 || m < 1) return UPP_E_BADARG;
    if (B == 0) return 0;
    if (B > 65535) return UPP_E_RANGE;
    hipLaunchKernelGGL(three_nn_kernel, dim3((n + kQueries - 1) / kQueries, B), dim3(kQueries), 0, (hipStream_t)stream, unknown, known, dist,
                       idx, n, m);
    return upp_launch_status();
}

extern "C" int upp_three_interpolate_fwd(const float *features, const int32_t *idx, const float *weight, float *out, int B, int C, int m,
                                         int n, void *stream) {
    if (!features || !idx || !weight || !out || B < 0 || C < 1 || m < 1 || n < 1) return UPP_E_BADARG;
    if (B == 0) return 0;
    const long long total = (long long)B * C * n;
    hipLaunchKernelGGL(three_interpolate_fwd_kernel, dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, features, idx, weight, out, C,
                       m, n, total);
    return upp_launch_status();
}

extern "C" int upp_three_interpolate_bwd(const float *grad_out, const int32_t *idx, const float *weight, float *grad_features, int B, int C,
                                         int m, int n, void *stream) {
    if (!grad_out || !idx || !weight || !grad_features || B < 0 || C < 1 || m < 1 || n < 1) return UPP_E_BADARG;
    if (B == 0) return 0;
    const long long total = (long long)B * C * n;
    hipLaunchKernelGGL(three_interpolate_bwd_kernel, dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, grad_out, idx, weight,
                       grad_features, C, m, n, total);
    return upp_launch_status();
}

extern "C" int upp_three_interpolate_bwd_det(const float *grad_out, const int32_t *idx, const float *weight, float *grad_features, int B,
                                             int C, int m, int n, void *stream) {
    if (!grad_out || !idx || !weight || !grad_features || B < 0 || C < 1 || m < 1 || n < 1) return UPP_E_BADARG;
    if (B == 0) return 0;
    det_launch<kDetCh>(InterpolateJob{grad_out, idx, weight, grad_features, B, C, m, n}, stream);
    return upp_launch_status();
}

// grouping_operation: features (B,C,N), idx (B,P,S) -> (B,C,P,S) is gather_operation with M = P S
static int grouping_args(const void *a, const void *b, const void *c, int B, int C, int N, int P, int S) {
    if (!a || !b || !c || B < 0 || C < 1 || N < 1 || P < 1 || S < 1) return UPP_E_BADARG;
    if ((long long)P * S > 0x7FFFFFFFLL) return UPP_E_RANGE;
    return 0;
}

extern "C" int upp_grouping_fwd(const float *features, const int32_t *idx, float *out, int B, int C, int N, int P, int S, void *stream) {
    const int rc = grouping_args(features, idx, out, B, C, N, P, S);
    return rc ? rc : upp_gather_fwd(features, idx, out, B, C, N, P * S, stream);
}

extern "C" int upp_grouping_bwd(const float *grad_out, const int32_t *idx, float *grad_features, int B, int C, int N, int P, int S,
                                void *stream) {
    const int rc = grouping_args(grad_out, idx, grad_features, B, C, N, P, S);
    return rc ? rc : upp_gather_bwd(grad_out, idx, grad_features, B, C, N, P * S, stream);
}

extern "C" int upp_grouping_bwd_det(const float *grad_out, const int32_t *idx, float *grad_features, int B, int C, int N, int P, int S,
                                    void *stream) {
    const int rc = grouping_args(grad_out, idx, grad_features, B, C, N, P, S);
    return rc ? rc : upp_gather_bwd_det(grad_out, idx, grad_features, B, C, N, P * S, stream);
}
