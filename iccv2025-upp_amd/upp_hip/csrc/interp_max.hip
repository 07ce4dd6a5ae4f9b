// interp_max.hip -- the interpolate-max of AdaPoinTr's deformable graph attention for gfx950 (include/upp_hip.h "deformable graph
// attention"; reference models/Transformer_utils.py:623-775).  knn_map of [f - q ; q] is W1 f + (W2 - W1) q + b and f is a three-point
// interpolation, so with the per-point products PW = v W1^T and Bq = q (W2 - W1)^T + b what is left is
//   y[b,n,s,o] = Bq[b,n,o] + sum_j w3[b,n k+s,j] PW[b,idx3[b,n k+s,j],o],   out = lrelu(max_s y)
// -- gather-bound, no GEMM, and y is never stored:
//   im_fwd_kernel   one wave per (b, n, 64-channel chunk), lane = channel: a slot is three weighted 256-byte row reads into one register;
//                   the running maximum and its slot stay in registers
//   im_bwd_kernel   g = g_out * lrelu'(out) (out > 0 exactly where the maximum is: no row is read again), d_Bq = g, and -- kAtomic -- the
//                   three products w3 * g of the arg slot added to d_PW by f32 atomics; <false> leaves d_PW to InterpMaxJob, a job of
//                   det_scan.h's det_scatter_kernel
// A wave's item is wave-uniform (readfirstlane), so idx3 / w3 travel through the scalar cache in the forward.  No LDS, no scratch, no
// per-lane array.  The NaN rule, lrelu and lrelu' are those of the norm-free ec_apply_kernel / ec_bwd_apply_kernel (edge_conv.hip).
#include "deform_row.h"

namespace {

constexpr int kImMaxK = kDaMaxK, kImMaxO = 1024;      // (the slots are the deformable family's: deform_row.h)
constexpr int kImWaves = 4;           // waves (items) per workgroup
constexpr long long kImGridCap = 65536;

__device__ __forceinline__ int im_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ float im_lrelu(float z, float slope) { return z > 0.0f ? z : z * slope; }            // (ec_apply_kernel's)
__device__ __forceinline__ float im_lrelu_grad(float z, float slope) { return z > 0.0f ? 1.0f : slope; }        // (ec_lrelu_grad)

// blockIdx.x * 4 + wave = item (b, n, chunk), grid-stride.  The lanes beyond O in the last chunk read channel O - 1 and store nothing.
__global__ __launch_bounds__(64 * kImWaves) void im_fwd_kernel(const float *__restrict__ PW, const float *__restrict__ Bq,
                                                               const int32_t *__restrict__ idx3, const float *__restrict__ w3,
                                                               float *__restrict__ out, uint8_t *__restrict__ arg, float slope, int N, int NK,
                                                               int k, int O, int chunks, long long items) {
    const int lane = threadIdx.x & 63;
    for (long long it = (long long)blockIdx.x * kImWaves + im_wave(); it < items; it += (long long)gridDim.x * kImWaves) {
        const int c0 = (int)(it % chunks) * 64, ch = min(c0 + lane, O - 1);
        const long long bn = it / chunks, b = bn / N;
        const float bq = Bq[bn * O + ch];
        const float *Pb = PW + b * NK * O + ch;
        float mx = -__builtin_inff();
        int a = 0;
        for (int s = 0; s < k; ++s) {
            const long long e = (bn * k + s) * 3;
            float y = bq;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = idx3[e + j];
                if ((unsigned)i < (unsigned)NK) y = __builtin_fmaf(w3[e + j], Pb[(long long)i * O], y);
            }
            if (y > mx) { mx = y; a = s; }                  // the first maximum wins: lowest s; a NaN never wins
        }
        if (c0 + lane < O) {
            out[bn * O + ch] = im_lrelu(mx, slope);
            arg[bn * O + ch] = (uint8_t)a;
        }
    }
}

// The backward of one item.  out > 0 exactly where the maximum m is (m * slope <= 0 for m <= 0), so lrelu'(m) is read off out.
template <bool kAtomic>
__global__ __launch_bounds__(64 * kImWaves) void im_bwd_kernel(const float *__restrict__ g_out, const float *__restrict__ out,
                                                               const uint8_t *__restrict__ arg, const int32_t *__restrict__ idx3,
                                                               const float *__restrict__ w3, float *__restrict__ d_Bq, float *__restrict__ d_PW,
                                                               float slope, int N, int NK, int k, int O, int chunks, long long items) {
    const int lane = threadIdx.x & 63;
    for (long long it = (long long)blockIdx.x * kImWaves + im_wave(); it < items; it += (long long)gridDim.x * kImWaves) {
        const int c0 = (int)(it % chunks) * 64, ch = min(c0 + lane, O - 1);
        const bool live = c0 + lane < O;
        const long long bn = it / chunks, b = bn / N;
        const float g = __fmul_rn(g_out[bn * O + ch], im_lrelu_grad(out[bn * O + ch], slope));
        if (live) d_Bq[bn * O + ch] = g;
        if (kAtomic) {
            const long long e = (bn * k + min((int)arg[bn * O + ch], k - 1)) * 3;      // (per lane: the arg is the channel's)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = idx3[e + j];
                if (live && (unsigned)i < (unsigned)NK) atomicAdd(d_PW + (b * NK + i) * O + ch, __fmul_rn(w3[e + j], g));
            }
        }
    }
}

// d_PW[b][r][o] = +0.0f, then + w3[b][n k + arg][j] * g[b][n][o] for every source (n, j) with idx3[b][n k + arg[b][n][o]][j] == r, in
// ascending 3 n + j (include/upp_hip.h).  The arg is per channel and the body's key per source, so the walk is over ALL (n k + s) 3 + j
// sources of the cloud, and a channel whose arg is another slot stages +0.0f: x + 0.0f == x from a +0.0f start, so the bits are those
// of the walk over the arg slots alone.  A source none of whose kDetCh channels chose its slot takes no part (key -1).
struct InterpMaxJob {
    const float *__restrict__ g_out;
    const float *__restrict__ out;
    const uint8_t *__restrict__ arg;
    const int32_t *__restrict__ idx3;
    const float *__restrict__ w3;
    float *__restrict__ d_PW;
    float slope;
    int B, N, NK, k, O;
    __host__ __device__ long long items() const { return (long long)B * det_groups(O) * det_tiles(NK); }
    __device__ __forceinline__ DetItem item(long long it) const { return det_item(it, O, NK, 3LL * N * k); }
    __device__ __forceinline__ void first(const DetItem &, long long, float (&)[kDetCh]) const {}
    __device__ __forceinline__ void stage(const DetItem &w, long long c0, int i, int32_t &key, float *v) const {
        const long long src = c0 + i, ns = src / 3, bn = w.b * N + ns / k;
        const int s = (int)(ns % k);
        const int r = idx3[w.b * w.S + src];
        const float wt = w3[w.b * w.S + src];
        bool any = false;
#pragma unroll
        for (int c = 0; c < kDetCh; ++c) {
            const long long e = bn * O + min(w.ch0 + c, O - 1);
            const bool hit = w.ch0 + c < O && min((int)arg[e], k - 1) == s;
            v[c] = hit ? __fmul_rn(wt, __fmul_rn(g_out[e], im_lrelu_grad(out[e], slope))) : 0.0f;
            any |= hit;
        }
        key = any && (unsigned)r < (unsigned)NK ? r : -1;
    }
    __device__ __forceinline__ void store(const DetItem &w, long long r, const float (&acc)[kDetCh]) const {
#pragma unroll
        for (int c = 0; c < kDetCh; ++c)
            if (w.ch0 + c < O) d_PW[(w.b * NK + r) * O + w.ch0 + c] = acc[c];
    }
};

static int im_args(bool ptrs, float slope, int B, int N, int NK, int k, int O) {
    if (!ptrs || B < 1 || N < 1 || NK < 1 || k < 1 || O < 1 || !(slope >= 0.0f && slope <= 1.0f)) return UPP_E_BADARG;
    if (k > kImMaxK || O > kImMaxO || B > 65535) return UPP_E_RANGE;
    if (!da_fits((long long)B * NK * O) || !da_fits((long long)B * N * O) || !da_fits((long long)B * N * k * 3)) return UPP_E_RANGE;
    return 0;
}

static int im_bwd(bool det, const float *g_out, const float *out, const uint8_t *arg, const int32_t *idx3, const float *w3, float *d_Bq,
                  float *d_PW, float slope, int B, int N, int NK, int k, int O, void *stream) {
    const int rc = im_args(g_out && out && arg && idx3 && w3 && d_Bq && d_PW, slope, B, N, NK, k, O);
    if (rc) return rc;
    const int chunks = (O + 63) / 64;
    const long long items = (long long)B * N * chunks;
    const dim3 grid(grid_for(items, kImWaves, kImGridCap)), block(64 * kImWaves);
    if (det) {
        hipLaunchKernelGGL(im_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, g_out, out, arg, idx3, w3, d_Bq, d_PW, slope, N, NK, k, O,
                           chunks, items);
        det_launch<kDetCh>(InterpMaxJob{g_out, out, arg, idx3, w3, d_PW, slope, B, N, NK, k, O}, stream);
    } else {
        upp_zero_async(d_PW, (long long)B * NK * O, (hipStream_t)stream);
        hipLaunchKernelGGL(im_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, g_out, out, arg, idx3, w3, d_Bq, d_PW, slope, N, NK, k, O,
                           chunks, items);
    }
    return upp_launch_status();
}

}  // namespace

extern "C" int upp_interp_max_fwd(const float *PW, const float *Bq, const int32_t *idx3, const float *w3, float *out, uint8_t *arg,
                                  float slope, int B, int N, int NK, int k, int O, void *stream) {
    const int rc = im_args(PW && Bq && idx3 && w3 && out && arg, slope, B, N, NK, k, O);
    if (rc) return rc;
    const int chunks = (O + 63) / 64;
    const long long items = (long long)B * N * chunks;
    hipLaunchKernelGGL(im_fwd_kernel, dim3(grid_for(items, kImWaves, kImGridCap)), dim3(64 * kImWaves), 0, (hipStream_t)stream, PW, Bq, idx3, w3,
                       out, arg, slope, N, NK, k, O, chunks, items);
    return upp_launch_status();
}

extern "C" int upp_interp_max_bwd(const float *g_out, const float *out, const uint8_t *arg, const int32_t *idx3, const float *w3,
                                  float *d_Bq, float *d_PW, float slope, int B, int N, int NK, int k, int O, void *stream) {
    return im_bwd(false, g_out, out, arg, idx3, w3, d_Bq, d_PW, slope, B, N, NK, k, O, stream);
}

extern "C" int upp_interp_max_bwd_det(const float *g_out, const float *out, const uint8_t *arg, const int32_t *idx3, const float *w3,
                                      float *d_Bq, float *d_PW, float slope, int B, int N, int NK, int k, int O, void *stream) {
    return im_bwd(true, g_out, out, arg, idx3, w3, d_Bq, d_PW, slope, B, N, NK, k, O, stream);
}
