// deform_row.h -- what the deformable attention kernels share: deform_attn.hip (da_*), region_attn.hip (ra_*) and, for the host-side
// limits only, interp_max.hip (im_*).  The row builder da_row and its transpose da_scatter are compiled from this one statement each, so
// an interpolated key / value row and its atomic scatter have the same bits and the same order in both attention files.  Also here: the
// item decode of the four attention kernels and the entry points' limits and size check.
#pragma once
#include <initializer_list>
#include "det_scan.h"

constexpr int kDaMaxH = 16;           // heads (C = 64 H <= 1024)
constexpr int kDaMaxK = 32;           // neighbour slots: one lane each in da_fwd_kernel's softmax, one register each in ra_*_kernel

// item it = (b N + n) H + h of a wave whose lane is the channel of head h -> bn = b N + n, b, n, ch = 64 h + lane
struct DaItem { long long bn, b; int n, ch; };
__device__ __forceinline__ DaItem da_item(long long it, int N, int H, int lane) {
    const int h = (int)(it % H), ch = h * 64 + lane;
    const long long bn = it / H, b = bn / N;
    return {bn, b, (int)(bn % N), ch};
}

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

// da_row's transpose by f32 atomics: d_PK[idx3] += w3 * dk, then d_PV[idx3] += w3 * dv, for ascending g, then ascending j, of slot s of
// query (b, n), channel ch (256 contiguous bytes per wave instruction).  An index outside [0, NK) takes nothing.
__device__ __forceinline__ void da_scatter(float *__restrict__ d_PK, float *__restrict__ d_PV, float dk, float dv,
                                           const int32_t *__restrict__ idx3, const float *__restrict__ w3, long long b, int n, int s, int G,
                                           int N, int NK, int k, int C, int ch) {
    for (int g = 0; g < G; ++g) {
        const long long bg = b * G + g, e = ((bg * N + n) * k + s) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = idx3[e + j];
            if ((unsigned)i < (unsigned)NK) {
                const float w = w3[e + j];
                atomicAdd(d_PK + (bg * NK + i) * C + ch, __fmul_rn(w, dk));
                atomicAdd(d_PV + (bg * NK + i) * C + ch, __fmul_rn(w, dv));
            }
        }
    }
}

static inline bool da_fits(long long v) { return v < 0x80000000LL; }                            // an element count a 32-bit index reaches
static inline bool da_positive(float v) { return v > 0.0f && __builtin_isfinite(v); }           // scale, eps

// The sizes of an entry point: UPP_E_BADARG for one below 1, UPP_E_RANGE outside the served range or for an array -- each given by its
// factors, multiplied only once the sizes are known to be in range -- of 2^31 elements or more.
static inline int da_sizes(int B, int N, int NK, int k, int H, int G, std::initializer_list<std::initializer_list<long long>> arrays) {
    if (B < 1 || N < 1 || NK < 1 || k < 1 || H < 1 || G < 1) return UPP_E_BADARG;
    if (H > kDaMaxH || k > kDaMaxK || H % G || B > 65535) return UPP_E_RANGE;
    for (const auto &factors : arrays) {
        long long v = 1;
        for (const long long f : factors) v *= f;
        if (!da_fits(v)) return UPP_E_RANGE;
    }
    return 0;
}
