// deform_attn.hip -- the deformable local cross-attention of AdaPoinTr for gfx950 (include/upp_hip.h "deformable local
// cross-attention"; reference models/Transformer_utils.py:269-491).  What is left of the module after its per-point products is
// gather-bound and has no GEMM in it:
//   da_offset_kernel   shift = pos[idx] + tanh(W3 gelu(LayerNorm(A[idx] + Bq))): one wave per (b, g, n, s) row, the C = 64 H values of
//                      the row in H registers per lane (channel = 64 i + lane), nothing but the three coordinates stored; <true> scales
//                      the tanh by half the extent of the k listed positions (the `improved` modules: deformable within a local ball)
//   da_fwd_kernel      one wave per (b, n, head), lane = channel of the head: the key and value rows of a neighbour slot are 3 G
//                      weighted 256-byte row reads each and live in registers only; scores by a wave sum, softmax over the <= 32 slots
//                      on the lanes, ctx by an fma chain over the slots
//   da_bwd_kernel      the same walk twice (value rows for dp, key rows for d_q); d_PK / d_PV by f32 atomics (256 contiguous bytes per
//                      wave instruction: deform_row.h's da_scatter) or, <false>, left to DeformJob -- a job of det_scan.h's
//                      det_scatter_kernel
// A wave's item is wave-uniform (readfirstlane), so idx3 / w3 travel through the scalar cache.  No LDS, no scratch: every per-lane array
// is indexed by a fully unrolled, guarded loop.
#include "deform_row.h"

namespace {

constexpr int kDaWaves = 4;           // waves (items) per workgroup
constexpr long long kDaGridCap = 65536;

__device__ __forceinline__ int da_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ float da_lane(float v, int l) { return __uint_as_float(readlane_u32(__float_as_uint(v), l)); }

// blockIdx.x * 4 + wave = row (b, g, n, s), grid-stride.  LayerNorm: biased variance, two passes over the registers; every sum is the
// lane's partial over its H channels in ascending channel, then wave_sum_f32's fixed tree.  kBall (upp_deform_offset_ball_fwd): the tanh is
// scaled by half the extent of the k listed positions of (b, n), whose slots sit on lanes 0 ... k-1; one slot outside the cloud and
// every row of that (b, n) is NaN.
template <bool kBall>
__global__ __launch_bounds__(256) void da_offset_kernel(const float *__restrict__ A, const float *__restrict__ Bq, const long long *__restrict__ idx,
                                                        const float *__restrict__ pos, const float *__restrict__ gamma,
                                                        const float *__restrict__ beta, const float *__restrict__ W3, float *__restrict__ shift,
                                                        float eps, int G, int N, int NK, int k, int H, long long rows) {
    const int lane = threadIdx.x & 63, C = H * 64;
    float ga[kDaMaxH], be[kDaMaxH], w0[kDaMaxH], w1[kDaMaxH], w2[kDaMaxH];
#pragma unroll
    for (int i = 0; i < kDaMaxH; ++i) {
        const bool on = i < H;
        const int c = on ? i * 64 + lane : 0;
        ga[i] = on ? gamma[c] : 0.0f;
        be[i] = on ? beta[c] : 0.0f;
        w0[i] = on ? W3[c] : 0.0f;
        w1[i] = on ? W3[C + c] : 0.0f;
        w2[i] = on ? W3[2 * C + c] : 0.0f;
    }
    const float fC = (float)C;
    for (long long row = (long long)blockIdx.x * kDaWaves + da_wave(); row < rows; row += (long long)gridDim.x * kDaWaves) {
        const int s = (int)(row % k);
        const long long t = row / k;
        const int n = (int)(t % N);
        const long long bg = t / N, b = bg / G;
        const long long j0 = idx[(b * N + n) * k + s];
        bool valid = (unsigned long long)j0 < (unsigned long long)NK;            // (a row outside the cloud is never read through)
        const long long j = valid ? j0 : 0;
        float half = 1.0f;                                                       // lane d < 3: 0.5 (max_s - min_s) of coordinate d
        if (kBall) {
            const long long jl0 = idx[(b * N + n) * k + min(lane, k - 1)];
            const bool ok = (unsigned long long)jl0 < (unsigned long long)NK;
            valid = __ballot(!ok) == 0;
            const float *pl = pos + (b * NK + (ok ? jl0 : 0)) * 3;
            const float r0 = wave_max_f32(pl[0]) - -wave_max_f32(-pl[0]);        // (the lanes beyond k repeat slot k - 1)
            const float r1 = wave_max_f32(pl[1]) - -wave_max_f32(-pl[1]);
            const float r2 = wave_max_f32(pl[2]) - -wave_max_f32(-pl[2]);
            half = __fmul_rn(0.5f, lane == 0 ? r0 : (lane == 1 ? r1 : r2));
        }
        const float *a = A + (bg * NK + j) * C, *bq = Bq + (bg * N + n) * C;
        float y[kDaMaxH], part = 0.0f;
#pragma unroll
        for (int i = 0; i < kDaMaxH; ++i) {
            y[i] = i < H ? a[i * 64 + lane] + bq[i * 64 + lane] : 0.0f;
            if (i < H) part += y[i];
        }
        const float mean = wave_sum_f32(part) / fC;
        part = 0.0f;
#pragma unroll
        for (int i = 0; i < kDaMaxH; ++i)
            if (i < H) { const float d = y[i] - mean; part = __builtin_fmaf(d, d, part); }
        const float rstd = 1.0f / sqrtf(wave_sum_f32(part) / fC + eps);
        float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
#pragma unroll
        for (int i = 0; i < kDaMaxH; ++i)
            if (i < H) {
                const float z = (y[i] - mean) * rstd * ga[i] + be[i];
                const float h = 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f));
                d0 = __builtin_fmaf(h, w0[i], d0);
                d1 = __builtin_fmaf(h, w1[i], d1);
                d2 = __builtin_fmaf(h, w2[i], d2);
            }
        d0 = wave_sum_f32(d0);
        d1 = wave_sum_f32(d1);
        d2 = wave_sum_f32(d2);
        if (lane < 3) {
            const float d = lane == 0 ? d0 : (lane == 1 ? d1 : d2);
            const float off = kBall ? __fmul_rn(tanhf(d), half) : tanhf(d);
            shift[row * 3 + lane] = valid ? __fadd_rn(pos[(b * NK + j) * 3 + lane], off) : __builtin_nanf("");
        }
    }
}

// blockIdx.x * 4 + wave = item (b, n, h), grid-stride.  score_s sits on lane s; p (B,N,H,k) is saved for the backward.
__global__ __launch_bounds__(256) void da_fwd_kernel(const float *__restrict__ q, const float *__restrict__ PK, const float *__restrict__ PV,
                                                     const float *__restrict__ bk, const float *__restrict__ bv, const int32_t *__restrict__ idx3,
                                                     const float *__restrict__ w3, float *__restrict__ ctx, float *__restrict__ p, float scale,
                                                     int N, int NK, int k, int H, int G, long long items) {
    const int lane = threadIdx.x & 63, C = H * 64;
    for (long long it = (long long)blockIdx.x * kDaWaves + da_wave(); it < items; it += (long long)gridDim.x * kDaWaves) {
        const auto [bn, b, n, ch] = da_item(it, N, H, lane);
        const float qv = q[bn * C + ch], kb = bk ? bk[ch] : 0.0f, vb = bv ? bv[ch] : 0.0f;
        float sc = 0.0f;
        for (int s = 0; s < k; ++s) {
            const float key = da_row(PK, kb, idx3, w3, b, n, s, G, N, NK, k, C, ch);
            const float d = scale * wave_sum_f32(qv * key);
            if (lane == s) sc = d;
        }
        const float m = wave_max_f32(lane < k ? sc : -3.402823466e38f);
        const float e = lane < k ? expf(sc - m) : 0.0f;
        const float pr = e / wave_sum_f32(e);
        if (lane < k) p[it * k + lane] = pr;
        float acc = 0.0f;
        for (int s = 0; s < k; ++s) {
            const float val = da_row(PV, vb, idx3, w3, b, n, s, G, N, NK, k, C, ch);
            acc = __builtin_fmaf(da_lane(pr, s), val, acc);
        }
        ctx[bn * C + ch] = acc;
    }
}

// The backward of one item: value rows again for dp, ds = p (dp - sum p dp) on the lanes (saved: DeformJob reads it), key rows again for
// d_q = scale * (fma chain over ascending s).  d_key_s = (scale ds_s) q and d_val_s = p_s d_ctx need no row; kAtomic adds w3 times them
// to d_PK / d_PV (zeroed by the entry point).  d_krow (B,N,C) or NULL = sum_s d_key_s in ascending s, the rows of d_bk.
template <bool kAtomic>
__global__ __launch_bounds__(256) void da_bwd_kernel(const float *__restrict__ q, const float *__restrict__ PK, const float *__restrict__ PV,
                                                     const float *__restrict__ bk, const float *__restrict__ bv, const int32_t *__restrict__ idx3,
                                                     const float *__restrict__ w3, const float *__restrict__ p, const float *__restrict__ d_ctx,
                                                     float *__restrict__ d_q, float *__restrict__ d_PK, float *__restrict__ d_PV,
                                                     float *__restrict__ d_krow, float *__restrict__ ds_out, float scale, int N, int NK, int k,
                                                     int H, int G, long long items) {
    const int lane = threadIdx.x & 63, C = H * 64;
    for (long long it = (long long)blockIdx.x * kDaWaves + da_wave(); it < items; it += (long long)gridDim.x * kDaWaves) {
        const auto [bn, b, n, ch] = da_item(it, N, H, lane);
        const float qv = q[bn * C + ch], dc = d_ctx[bn * C + ch], kb = bk ? bk[ch] : 0.0f, vb = bv ? bv[ch] : 0.0f;
        const float pr = lane < k ? p[it * k + lane] : 0.0f;
        float dp = 0.0f;
        for (int s = 0; s < k; ++s) {
            const float val = da_row(PV, vb, idx3, w3, b, n, s, G, N, NK, k, C, ch);
            const float d = wave_sum_f32(dc * val);
            if (lane == s) dp = d;
        }
        const float ds = pr * (dp - wave_sum_f32(pr * dp));
        if (lane < k) ds_out[it * k + lane] = ds;
        float dq = 0.0f, dkb = 0.0f;
        for (int s = 0; s < k; ++s) {
            const float key = da_row(PK, kb, idx3, w3, b, n, s, G, N, NK, k, C, ch);
            const float dss = da_lane(ds, s);
            dq = __builtin_fmaf(dss, key, dq);
            const float dk = __fmul_rn(__fmul_rn(scale, dss), qv);
            dkb = __fadd_rn(dkb, dk);
            if (kAtomic) da_scatter(d_PK, d_PV, dk, __fmul_rn(da_lane(pr, s), dc), idx3, w3, b, n, s, G, N, NK, k, C, ch);
        }
        d_q[bn * C + ch] = scale * dq;
        if (d_krow) d_krow[bn * C + ch] = dkb;
    }
}

// d_PK[b][g][r][ch] = +0.0f, then + w3 * ((scale * ds) * q) for every source (n, s, j) of (b, g) with idx3 == r, in ascending
// (n k + s) 3 + j; d_PV likewise with w3 * (p * d_ctx) (include/upp_hip.h).  A workgroup owns 256 target points of one (b, g) and kDetCh
// channels of both arrays (NV = 2 kDetCh: the keys staged once serve both); a source's values are formed while staging.
struct DeformJob {
    const float *__restrict__ q;
    const float *__restrict__ d_ctx;
    const float *__restrict__ p;
    const float *__restrict__ ds;
    const int32_t *__restrict__ idx3;
    const float *__restrict__ w3;
    float *__restrict__ d_PK;
    float *__restrict__ d_PV;
    float scale;
    int B, G, N, NK, k, H;
    __host__ __device__ long long items() const { return (long long)B * G * det_groups(H * 64) * det_tiles(NK); }
    __device__ __forceinline__ DetItem item(long long it) const { return det_item(it, H * 64, NK, 3LL * N * k); }      // (cloud = b G + g)
    __device__ __forceinline__ void first(const DetItem &, long long, float (&)[2 * kDetCh]) const {}
    __device__ __forceinline__ void stage(const DetItem &w, long long c0, int i, int32_t &key, float *v) const {
        const long long src = c0 + i, ns = src / 3, n = ns / k, bn = (w.b / G) * N + n;
        const int s = (int)(ns % k), C = H * 64;
        const int r = idx3[w.b * w.S + src];
        const float wt = w3[w.b * w.S + src];
        key = (unsigned)r < (unsigned)NK ? r : -1;
        const long long e = (bn * H + (w.ch0 >> 6)) * k + s;                   // (kDetCh channels never straddle a head)
        const float sds = __fmul_rn(scale, ds[e]), ps = p[e];
#pragma unroll
        for (int c = 0; c < kDetCh; ++c) {
            v[c] = __fmul_rn(wt, __fmul_rn(sds, q[bn * C + w.ch0 + c]));
            v[kDetCh + c] = __fmul_rn(wt, __fmul_rn(ps, d_ctx[bn * C + w.ch0 + c]));
        }
    }
    __device__ __forceinline__ void store(const DetItem &w, long long r, const float (&acc)[2 * kDetCh]) const {
        const long long o = (w.b * NK + r) * (H * 64) + w.ch0;
#pragma unroll
        for (int c = 0; c < kDetCh; ++c) { d_PK[o + c] = acc[c]; d_PV[o + c] = acc[kDetCh + c]; }
    }
};

// (the arrays: p / ds, PK / PV, q-sized rows per group, idx3 / w3)
static int da_check(int B, int N, int NK, int k, int H, int G) {
    return da_sizes(B, N, NK, k, H, G, {{B, N, k, H}, {B, G, NK, 64, H}, {B, G, N, 64, H}, {B, G, N, k, 3}});
}

static int da_bwd(bool det, const float *q, const float *PK, const float *PV, const float *bk, const float *bv, const int32_t *idx3,
                  const float *w3, const float *p, const float *d_ctx, float *d_q, float *d_PK, float *d_PV, float *d_krow, float *ds,
                  float scale, int B, int N, int NK, int k, int H, int G, void *stream) {
    if (!q || !PK || !PV || !idx3 || !w3 || !p || !d_ctx || !d_q || !d_PK || !d_PV || !ds || !da_positive(scale)) return UPP_E_BADARG;
    const int rc = da_check(B, N, NK, k, H, G);
    if (rc) return rc;
    const long long items = (long long)B * N * H;
    const dim3 grid(grid_for(items, kDaWaves, kDaGridCap));
    if (det) {
        hipLaunchKernelGGL(da_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, q, PK, PV, bk, bv, idx3, w3, p, d_ctx, d_q, d_PK,
                           d_PV, d_krow, ds, scale, N, NK, k, H, G, items);
        det_launch<2 * kDetCh>(DeformJob{q, d_ctx, p, ds, idx3, w3, d_PK, d_PV, scale, B, G, N, NK, k, H}, stream);
    } else {
        const long long n = (long long)B * G * NK * 64 * H;
        upp_zero_async(d_PK, n, (hipStream_t)stream);
        upp_zero_async(d_PV, n, (hipStream_t)stream);
        hipLaunchKernelGGL(da_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, q, PK, PV, bk, bv, idx3, w3, p, d_ctx, d_q, d_PK,
                           d_PV, d_krow, ds, scale, N, NK, k, H, G, items);
    }
    return upp_launch_status();
}

static int da_offset(bool ball, const float *A, const float *Bq, const int64_t *idx, const float *pos, const float *gamma, const float *beta,
                     const float *W3, float *shift, float eps, int B, int G, int N, int NK, int k, int C, void *stream) {
    if (!A || !Bq || !idx || !pos || !gamma || !beta || !W3 || !shift || !da_positive(eps) || C < 1) return UPP_E_BADARG;
    if (C % 64) return UPP_E_RANGE;
    const int rc = da_check(B, N, NK, k, C / 64, G);
    if (rc) return rc;
    const long long rows = (long long)B * G * N * k;
    const dim3 grid(grid_for(rows, kDaWaves, kDaGridCap));
    const long long *list = reinterpret_cast<const long long *>(idx);
    if (ball)
        hipLaunchKernelGGL(da_offset_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, A, Bq, list, pos, gamma, beta, W3, shift, eps, G, N,
                           NK, k, C / 64, rows);
    else
        hipLaunchKernelGGL(da_offset_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, A, Bq, list, pos, gamma, beta, W3, shift, eps, G, N,
                           NK, k, C / 64, rows);
    return upp_launch_status();
}

}  // namespace

extern "C" int upp_deform_offset_fwd(const float *A, const float *Bq, const int64_t *idx, const float *pos, const float *gamma,
                                     const float *beta, const float *W3, float *shift, float eps, int B, int G, int N, int NK, int k, int C,
                                     void *stream) {
    return da_offset(false, A, Bq, idx, pos, gamma, beta, W3, shift, eps, B, G, N, NK, k, C, stream);
}

extern "C" int upp_deform_offset_ball_fwd(const float *A, const float *Bq, const int64_t *idx, const float *pos, const float *gamma,
                                          const float *beta, const float *W3, float *shift, float eps, int B, int G, int N, int NK, int k,
                                          int C, void *stream) {
    return da_offset(true, A, Bq, idx, pos, gamma, beta, W3, shift, eps, B, G, N, NK, k, C, stream);
}

extern "C" int upp_deform_attn_fwd(const float *q, const float *PK, const float *PV, const float *bk, const float *bv, const int32_t *idx3,
                                   const float *w3, float *ctx, float *p, float scale, int B, int N, int NK, int k, int H, int G,
                                   void *stream) {
    if (!q || !PK || !PV || !idx3 || !w3 || !ctx || !p || !da_positive(scale)) return UPP_E_BADARG;
    const int rc = da_check(B, N, NK, k, H, G);
    if (rc) return rc;
    const long long items = (long long)B * N * H;
    hipLaunchKernelGGL(da_fwd_kernel, dim3(grid_for(items, kDaWaves, kDaGridCap)), dim3(256), 0, (hipStream_t)stream, q, PK, PV, bk, bv, idx3,
                       w3, ctx, p, scale, N, NK, k, H, G, items);
    return upp_launch_status();
}

extern "C" int upp_deform_attn_bwd(const float *q, const float *PK, const float *PV, const float *bk, const float *bv, const int32_t *idx3,
                                   const float *w3, const float *p, const float *d_ctx, float *d_q, float *d_PK, float *d_PV, float *d_krow,
                                   float *ds, float scale, int B, int N, int NK, int k, int H, int G, void *stream) {
    return da_bwd(false, q, PK, PV, bk, bv, idx3, w3, p, d_ctx, d_q, d_PK, d_PV, d_krow, ds, scale, B, N, NK, k, H, G, stream);
}

extern "C" int upp_deform_attn_bwd_det(const float *q, const float *PK, const float *PV, const float *bk, const float *bv,
                                       const int32_t *idx3, const float *w3, const float *p, const float *d_ctx, float *d_q, float *d_PK,
                                       float *d_PV, float *d_krow, float *ds, float scale, int B, int N, int NK, int k, int H, int G,
                                       void *stream) {
    return da_bwd(true, q, PK, PV, bk, bv, idx3, w3, p, d_ctx, d_q, d_PK, d_PV, d_krow, ds, scale, B, N, NK, k, H, G, stream);
}
