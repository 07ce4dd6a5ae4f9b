// deform_row.h -- the one row builder of the deformable attention kernels: deform_attn.hip (da_fwd_kernel, da_bwd_kernel) and
// region_attn.hip (ra_fwd_kernel, ra_bwd_kernel) compile this statement, so an interpolated key / value row has the same bits in both.
#pragma once
#include "common.h"

// bias[ch], then fma(w3, P[idx3], .) for ascending g, then ascending j: the key (or value) row of slot s of query (b, n), channel ch.
// An index outside [0, NK) contributes nothing.
__device__ __forceinline__ float da_row(const float *__restrict__ P, float bias, const int32_t *__restrict__ idx3, const float *__restrict__ w3,
                                        long long b, int n, int s, int G, int N, int NK, int k, int C, int ch) {
    float r = bias;
    for (int g = 0; g < G; ++g) {
        const long long bg = b * G + g, e = ((bg * N + n) * k + s) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = idx3[e + j];
            if ((unsigned)i < (unsigned)NK) r = __builtin_fmaf(w3[e + j], P[(bg * NK + i) * C + ch], r);
        }
    }
    return r;
}
