// norm_pool.hip -- "LayerNorm, then pool over the tokens" of the full fine-tuning models, with the LayerNorm's parameter gradients
// (reference models/Point_MAE_cp.py:582-587 PointTransformer, models/Point_MAE_segment.py:413-424 PointTransformer_seg):
//   upp_cls_pool_bwd_ln : upp_cls_pool_bwd's g_x (that very kernel) + g_gamma / g_beta from the 1 + D rows per sample that carry a
//                         gradient (row 0 and the arg-max rows) -- the dense (B,L,D) gradient is never walked for them.
//   upp_tap_pool_fwd    : x = [LN(f0) | LN(f1) | LN(f2)], its max / arg-max / mean over the tokens and the saved statistics, one launch.
//   upp_tap_pool_bwd    : the three pooled gradients folded into one row gradient, the row-LayerNorm backward per (row, tap) and the
//                         parameter gradients through per-workgroup partials: two launches.
// The LayerNorm arithmetic is rowln_core.h's (the bits of upp_rowln_fwd / upp_rowln_bwd).  Every sum below has an order fixed by the
// sizes alone; no atomics; every output element is written by a kernel.
#include "common.h"
#include "rowln_core.h"

namespace {

constexpr int kTW = 16;      // waves per workgroup of tap_pool_fwd_kernel
constexpr int kRW = 16;      // waves per workgroup of the partial-sum kernel

// grid (3, B): one workgroup per (tap, sample).  Phase 1: the waves stride the G rows -- LayerNorm, x and the statistics.  Phase 2,
// behind a workgroup barrier: one thread per column walks its G values of x in ascending g (they sit in this CU's cache / the L2):
// running maximum with the first-maximum / first-NaN rule of group_max_fwd_kernel and cls_pool_fwd_kernel, and the sum one rounded
// addition at a time.
__global__ __launch_bounds__(64 * kTW) void tap_pool_fwd_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                                const float *__restrict__ f2, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, float eps, float *x,
                                                                float *__restrict__ gmax, int32_t *__restrict__ arg,
                                                                float *__restrict__ gmean, float *__restrict__ mean,
                                                                float *__restrict__ rstd, int G, int C) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tap = blockIdx.x, b = blockIdx.y;
    const float *f = tap == 0 ? f0 : (tap == 1 ? f1 : f2);
    const size_t ldx = (size_t)3 * C;
    int cc[kRowE];
    float gv[kRowE], bv[kRowE];
#pragma unroll
    for (int e = 0; e < kRowE; ++e) { cc[e] = min(lane + 64 * e, C - 1); gv[e] = gamma[cc[e]]; bv[e] = beta[cc[e]]; }
    for (int g = wave; g < G; g += kTW) {
        const size_t row = (size_t)b * G + g;
        float v[kRowE];
#pragma unroll
        for (int e = 0; e < kRowE; ++e) v[e] = f[row * C + cc[e]];
#pragma unroll
        for (int e = 0; e < kRowE; ++e) v[e] = lane + 64 * e < C ? v[e] : 0.0f;
        float mu, rs;
        rowln_stats(v, lane, C, eps, mu, rs);
#pragma unroll
        for (int e = 0; e < kRowE; ++e) {
            const int c = lane + 64 * e;
            if (c < C) x[row * ldx + (size_t)tap * C + c] = rowln_affine(v[e], mu, rs, gv[e], bv[e]);
        }
        if (lane == 0) { mean[row * 3 + tap] = mu; rstd[row * 3 + tap] = rs; }
    }
    __threadfence_block();
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 64 * kTW) {
        const float *col = x + (size_t)b * G * ldx + (size_t)tap * C + c;
        float best = col[0], sum = col[0];
        int bi = 0;
        for (int g0 = 1; g0 < G; g0 += 8) {                        // eight independent loads in flight
            float h[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) h[q] = col[(size_t)min(g0 + q, G - 1) * ldx];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (g0 + q >= G) continue;
                sum += h[q];
                if (h[q] > best || (h[q] != h[q] && best == best)) { best = h[q]; bi = g0 + q; }
            }
        }
        const size_t o = (size_t)b * ldx + (size_t)tap * C + c;
        gmax[o] = best; arg[o] = bi; gmean[o] = sum / (float)G;
    }
}

// One wave per row, four rows per workgroup; the wave walks the three taps: t = d_x + d_gmean / G + [g == arg] d_gmax, the row-LayerNorm
// backward, and this row's parameter-gradient terms summed over the taps ascending.  The workgroup's four rows are then summed in wave
// order into part (workgroups, 2, C) = [d_gamma | d_beta] partials.
__global__ __launch_bounds__(256) void tap_pool_bwd_kernel(const float *__restrict__ d_x, const float *__restrict__ d_gmax,
                                                           const float *__restrict__ d_gmean, const float *__restrict__ f0,
                                                           const float *__restrict__ f1, const float *__restrict__ f2,
                                                           const float *__restrict__ mean, const float *__restrict__ rstd,
                                                           const float *__restrict__ gamma, const int32_t *__restrict__ arg,
                                                           float *__restrict__ d_f0, float *__restrict__ d_f1, float *__restrict__ d_f2,
                                                           float *__restrict__ part, int rows, int G, int C) {
    __shared__ float lnp[2][4][64 * kRowE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = blockIdx.x * 4 + wave;
    const float fG = (float)G;
    float pgam[kRowE], pbet[kRowE];
#pragma unroll
    for (int e = 0; e < kRowE; ++e) { pgam[e] = 0.0f; pbet[e] = 0.0f; }
    if (row < rows) {
        const int b = row / G, g = row - b * G;
        const size_t ldx = (size_t)3 * C;
        int cc[kRowE];
        float gm[kRowE];
#pragma unroll
        for (int e = 0; e < kRowE; ++e) { cc[e] = min(lane + 64 * e, C - 1); gm[e] = gamma[cc[e]]; }
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            const float *f = tap == 0 ? f0 : (tap == 1 ? f1 : f2);
            float *df = tap == 0 ? d_f0 : (tap == 1 ? d_f1 : d_f2);
            float dxv[kRowE], dmx[kRowE], dmn[kRowE], xo[kRowE];
            int am[kRowE];
#pragma unroll
            for (int e = 0; e < kRowE; ++e) {
                const size_t o = (size_t)b * ldx + (size_t)tap * C + cc[e];
                dxv[e] = d_x[(size_t)row * ldx + (size_t)tap * C + cc[e]];
                dmx[e] = d_gmax[o]; dmn[e] = d_gmean[o]; am[e] = arg[o];
                xo[e] = f[(size_t)row * C + cc[e]];
            }
            const float mu = mean[(size_t)row * 3 + tap], rs = rstd[(size_t)row * 3 + tap];
            float t[kRowE], dx[kRowE], xh[kRowE];
#pragma unroll
            for (int e = 0; e < kRowE; ++e) t[e] = (dxv[e] + dmn[e] / fG) + (am[e] == g ? dmx[e] : 0.0f);
            rowln_bwd_row(t, gm, xo, mu, rs, lane, C, dx, xh);
#pragma unroll
            for (int e = 0; e < kRowE; ++e) {
                const int c = lane + 64 * e;
                if (c < C) {
                    df[(size_t)row * C + c] = dx[e];
                    pgam[e] += t[e] * xh[e];
                    pbet[e] += t[e];
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < kRowE; ++e) { lnp[0][wave][lane + 64 * e] = pgam[e]; lnp[1][wave][lane + 64 * e] = pbet[e]; }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        part[((size_t)blockIdx.x * 2 + 0) * C + c] = (lnp[0][0][c] + lnp[0][1][c]) + (lnp[0][2][c] + lnp[0][3][c]);
        part[((size_t)blockIdx.x * 2 + 1) * C + c] = (lnp[1][0][c] + lnp[1][1][c]) + (lnp[1][2][c] + lnp[1][3][c]);
    }
}

// out[w] = sum over the n partial rows part[i][w] (W = 2 C columns: d_gamma then d_beta).  grid ceil(W / 64); lane = column; wave k sums the
// k-th run of ceil(n / kRW) consecutive partials in ascending order, the kRW run sums are then added in wave order.
__global__ __launch_bounds__(64 * kRW) void part_sum_kernel(const float *__restrict__ part, int n, int C, float *__restrict__ d_gamma,
                                                            float *__restrict__ d_beta) {
    __shared__ float sp[kRW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = 2 * C, w = blockIdx.x * 64 + lane;
    const int per = (n + kRW - 1) / kRW, i0 = wave * per, i1 = min(n, i0 + per);
    float s = 0.0f;
    if (w < W) {
        for (int j0 = i0; j0 < i1; j0 += 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = part[(size_t)min(j0 + q, i1 - 1) * W + w];
#pragma unroll
            for (int q = 0; q < 8; ++q) if (j0 + q < i1) s += v[q];
        }
    }
    sp[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && w < W) {
        float a = sp[0][lane];
#pragma unroll
        for (int k = 1; k < kRW; ++k) a += sp[k][lane];
        if (w < C) d_gamma[w] = a; else d_beta[w - C] = a;
    }
}

// g_gamma[d] = sum over (b, l) ascending of g_h[b][l][d] * xhat[b][l][d], g_beta[d] = sum of g_h[b][l][d], over the rows that carry a
// gradient: row 0 (g_feat[b][d]) and row amax[b][d] >= 1 (g_feat[b][D + d]).  One thread per column.
__global__ __launch_bounds__(64) void cls_pool_param_grad_kernel(const float *__restrict__ g_feat, const float *__restrict__ x,
                                                                 const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                 const int32_t *__restrict__ amax, float *__restrict__ g_gamma,
                                                                 float *__restrict__ g_beta, int B, int L, int D) {
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (d >= D) return;
    float sg = 0.0f, sb = 0.0f;
    for (int b0 = 0; b0 < B; b0 += 8) {                            // eight samples' loads in flight (two dependent rounds), summed in sample order
        int t[8];
        float g0[8], g1[8], h0[8], h1[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int b = min(b0 + q, B - 1);
            t[q] = amax[(size_t)b * D + d];
            g0[q] = g_feat[(size_t)b * 2 * D + d]; g1[q] = g_feat[(size_t)b * 2 * D + D + d];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int b = min(b0 + q, B - 1);
            const int tq = min(max(t[q], 1), L - 1);                // (the forward writes 1 .. L-1; a foreign table cannot reach outside x)
            const size_t r0 = (size_t)b * L, r1 = r0 + tq;
            h0[q] = (x[r0 * D + d] - mean[r0]) * rstd[r0];
            h1[q] = (x[r1 * D + d] - mean[r1]) * rstd[r1];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (b0 + q >= B) continue;
            sg = __builtin_fmaf(g0[q], h0[q], sg); sb += g0[q];
            sg = __builtin_fmaf(g1[q], h1[q], sg); sb += g1[q];
        }
    }
    g_gamma[d] = sg; g_beta[d] = sb;
}

int tap_pool_args(int B, int G, int C) {
    if (B < 1 || G < 1 || C < 1) return UPP_E_BADARG;
    if (B > 65535 || G > UPP_ATTN_MAX_L || C < 4 || C > 64 * kRowE || C % 4 != 0) return UPP_E_RANGE;
    return 0;
}

}  // namespace

extern "C" int upp_cls_pool_bwd_ln(const float *g_feat, const float *x, const float *mean, const float *rstd, const float *gamma,
                                   const int32_t *amax, float *g_x, float *g_gamma, float *g_beta, int B, int L, int D, void *stream) {
    if (!g_feat || !x || !mean || !rstd || !gamma || !amax || !g_x || !g_gamma || !g_beta || B < 1 || L < 2 || D < 1) return UPP_E_BADARG;
    if (D > 64 * kRowE) return UPP_E_RANGE;
    const int rc = upp_cls_pool_bwd(g_feat, x, mean, rstd, gamma, amax, g_x, B, L, D, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(cls_pool_param_grad_kernel, dim3((D + 63) / 64), dim3(64), 0, (hipStream_t)stream, g_feat, x, mean, rstd, amax,
                       g_gamma, g_beta, B, L, D);
    return upp_launch_status();
}

extern "C" int upp_tap_pool_fwd(const float *f0, const float *f1, const float *f2, const float *gamma, const float *beta, float eps,
                                float *x, float *gmax, int32_t *arg, float *gmean, float *mean, float *rstd, int B, int G, int C,
                                void *stream) {
    if (!f0 || !f1 || !f2 || !gamma || !beta || !x || !gmax || !arg || !gmean || !mean || !rstd) return UPP_E_BADARG;
    const int rc = tap_pool_args(B, G, C);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(tap_pool_fwd_kernel, dim3(3, B), dim3(64 * kTW), 0, (hipStream_t)stream, f0, f1, f2, gamma, beta, eps, x, gmax, arg,
                       gmean, mean, rstd, G, C);
    return upp_launch_status();
}

extern "C" long long upp_tap_pool_part_floats(int B, int G, int C) {
    if (tap_pool_args(B, G, C) != 0) return 0;
    return (((long long)B * G + 3) / 4) * 2 * C;
}

extern "C" int upp_tap_pool_bwd(const float *d_x, const float *d_gmax, const float *d_gmean, const float *f0, const float *f1,
                                const float *f2, const float *mean, const float *rstd, const float *gamma, const int32_t *arg,
                                float *part, float *d_f0, float *d_f1, float *d_f2, float *d_gamma, float *d_beta, int B, int G, int C,
                                void *stream) {
    if (!d_x || !d_gmax || !d_gmean || !f0 || !f1 || !f2 || !mean || !rstd || !gamma || !arg || !part || !d_f0 || !d_f1 || !d_f2 ||
        !d_gamma || !d_beta)
        return UPP_E_BADARG;
    const int rc = tap_pool_args(B, G, C);
    if (rc != 0) return rc;
    const long long rows = (long long)B * G;                       // <= 65535 * UPP_ATTN_MAX_L: row indices and the partial count fit an int
    const int nwg = (int)((rows + 3) / 4);
    hipLaunchKernelGGL(tap_pool_bwd_kernel, dim3(nwg), dim3(256), 0, (hipStream_t)stream, d_x, d_gmax, d_gmean, f0, f1, f2, mean, rstd, gamma,
                       arg, d_f0, d_f1, d_f2, part, (int)rows, G, C);
    int st = upp_launch_status();
    if (st != 0) return st;
    hipLaunchKernelGGL(part_sum_kernel, dim3((2 * C + 63) / 64), dim3(64 * kRW), 0, (hipStream_t)stream, part, nwg, C, d_gamma, d_beta);
    return upp_launch_status();
}
