// rowln_core.h -- the row LayerNorm of the library, forward and backward, as the one piece of device code its row kernels share
// (block.hip rowln_fwd / rowln_bwd, norm_pool.hip tap_pool_fwd / tap_pool_bwd): a kernel that calls these produces the bits of
// upp_rowln_fwd / upp_rowln_bwd for the same row.
// One wavefront per row; lane l holds columns l, l + 64, ... (kRowE slots -> D <= 512); a slot past D holds 0.
#pragma once
#include "common.h"

constexpr int kRowE = 8;

// mean and 1 / sqrt(var + eps) of a row: v[e] = the row's element at column lane + 64 e, 0 past D.
__device__ __forceinline__ void rowln_stats(const float (&v)[kRowE], int lane, int D, float eps, float &mean, float &rstd) {
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < kRowE; ++e) s += v[e];
    mean = wave_sum_f32(s) / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int e = 0; e < kRowE; ++e) { const int c = lane + 64 * e; const float dv = c < D ? v[e] - mean : 0.0f; q = __builtin_fmaf(dv, dv, q); }
    rstd = 1.0f / sqrtf(wave_sum_f32(q) / (float)D + eps);
}

__device__ __forceinline__ float rowln_affine(float v, float mean, float rstd, float gamma, float beta) {
    return __builtin_fmaf((v - mean) * rstd, gamma, beta);
}

// dx = rstd * (dy - mean(dy) - xhat * mean(dy * xhat)),  dy = gh * gamma;  xh = xhat (0 past D) is left for the parameter gradients
// (d_gamma += gh * xh, d_beta += gh).  dx of a slot past D is not meaningful.
__device__ __forceinline__ void rowln_bwd_row(const float (&gh)[kRowE], const float (&gm)[kRowE], const float (&xo)[kRowE], float mean,
                                              float rstd, int lane, int D, float (&dx)[kRowE], float (&xh)[kRowE]) {
    float dy[kRowE], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int e = 0; e < kRowE; ++e) {
        const bool ok = lane + 64 * e < D;
        dy[e] = ok ? gh[e] * gm[e] : 0.0f;
        xh[e] = ok ? (xo[e] - mean) * rstd : 0.0f;
        s1 += dy[e];
        s2 = __builtin_fmaf(dy[e], xh[e], s2);
    }
    s1 = wave_sum_f32(s1) / (float)D;
    s2 = wave_sum_f32(s2) / (float)D;
#pragma unroll
    for (int e = 0; e < kRowE; ++e) dx[e] = rstd * (dy[e] - s1 - xh[e] * s2);
}
