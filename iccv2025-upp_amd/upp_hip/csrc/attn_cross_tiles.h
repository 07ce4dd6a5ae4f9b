// attn_cross_tiles.h -- what the kernels of attn_cross.hip and attn_prefix.hip share: the 64 x 64 block geometry, the staging of operand
// rows into the LDS, the per-row statistics of the backward kernels and the recomputation of P and dS of one block.  The prefix-visibility
// mask of attn_prefix.hip is a template parameter (MASK) of xattn_p_ds; with MASK = false the code is attn_cross.hip's own.
#pragma once
#include "attn_tiles.h"

namespace {

constexpr int kSB = 64;          // rows of a query block and of a key block
constexpr int kSW = 4;           // waves per workgroup (one per SIMD)
constexpr int kTile = kSB * kLD; // floats of one staged (64 x 64) operand block

// rows [0, valid) x 64 of NARR sources (row stride rs floats) -> dst[a][kSB][kLD], rows >= valid zero (never read); all loads first
template <int NARR>
__device__ __forceinline__ void stage_rows(float *const (&dst)[NARR], const float *const (&src)[NARR], const size_t (&rs)[NARR], int valid) {
    constexpr int IT = kSB * 16 / (64 * kSW);
    float4 v[NARR][IT];
#pragma unroll
    for (int a = 0; a < NARR; ++a)
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = threadIdx.x + it * 64 * kSW;
            const int r = i >> 4, c = (i & 15) * 4;
            v[a][it] = r < valid ? *reinterpret_cast<const float4 *>(src[a] + (size_t)r * rs[a] + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
    for (int a = 0; a < NARR; ++a)
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = threadIdx.x + it * 64 * kSW;
            float *d = dst[a] + (i >> 4) * kLD + (i & 15) * 4;
            d[0] = v[a][it].x; d[1] = v[a][it].y; d[2] = v[a][it].z; d[3] = v[a][it].w;
        }
}

// delta_i = dO_i . O_i and lse_i of the `valid` rows behind g / o / l (rows >= valid: 0) -- 16 rows per wave, four per iteration, lane = channel
__device__ __forceinline__ void xattn_row_stats(const float *__restrict__ g, const float *__restrict__ o, const float *__restrict__ l,
                                                size_t cs, int valid, float *delta, float *lses, int wave, int lane) {
    for (int i0 = wave * (kSB / kSW); i0 < (wave + 1) * (kSB / kSW); i0 += 4) {
        float gv[4], ov[4], lv[4], d[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool ok = i0 + t < valid;
            gv[t] = ok ? g[(size_t)(i0 + t) * cs + lane] : 0.0f;
            ov[t] = ok ? o[(size_t)(i0 + t) * cs + lane] : 0.0f;
            lv[t] = (ok && lane == 0) ? l[i0 + t] : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) d[t] = wave_sum_f32(gv[t] * ov[t]);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (lane == 0) { delta[i0 + t] = d[t]; lses[i0 + t] = lv[t]; }
    }
}

// sum over the 32 lanes that share lk (a fixed combination order)
__device__ __forceinline__ float half_wave_sum_f32(float v, int lk) {
    v += __uint_as_float(dpp_u32<DPP_QUAD_XOR1>(__float_as_uint(v)));
    v += __uint_as_float(dpp_u32<DPP_QUAD_XOR2>(__float_as_uint(v)));
    v += __uint_as_float(dpp_u32<DPP_ROW_HALF_MIRROR>(__float_as_uint(v)));
    v += __uint_as_float(dpp_u32<DPP_ROW_MIRROR>(__float_as_uint(v)));
    const float a = __uint_as_float(readlane_u32(__float_as_uint(v), 0));
    const float b = __uint_as_float(readlane_u32(__float_as_uint(v), 16));
    const float c = __uint_as_float(readlane_u32(__float_as_uint(v), 32));
    const float d = __uint_as_float(readlane_u32(__float_as_uint(v), 48));
    return lk ? c + d : a + b;
}

// Prefix visibility (include/upp_hip.h "denoising-query attention"): query row q0 + i sees key k0 + j when the row is at or beyond split_q
// or the key is below split_k.
struct PrefixMask {
    int q0, k0, split_q, split_k;
    __device__ __forceinline__ bool sees(int i, int j) const { return q0 + i >= split_q || k0 + j < split_k; }
};

// P = exp(S scale - lse) and dS = P (dO V^T - delta) scale of one (64 query x 64 key) block into the strips Ps / Ds; entries of query
// rows >= qv and keys >= kv are zero.  Waves 0, 1 compute the two S tiles of query rows 32 it ..., waves 2, 3 the two dP tiles (two
// accumulator chains per wave); dP stays in registers until P is in the LDS.  `one` (Lk <= 64, uniform over the grid): delta is the
// row sum of P dP of this block instead of the `delta` strip.  MASK: entries that `m` hides are zero as well, by a select on the index and
// not by arithmetic on the score (a NaN score of a hidden key gives P = 0).  Ends on a barrier.
template <bool MASK>
__device__ __forceinline__ void xattn_p_ds(const float *Qb, const float *Gb, const float *Ks, const float *Vs, float *Ps, float *Ds,
                                           const float *lses, const float *delta, int qv, int kv, float scale, bool one, int wave, int lr,
                                           int lk, const PrefixMask m = PrefixMask()) {
    const int it = wave & 1;
    const bool dp = wave >= 2;
    f32x16 acc[2];
    zero(acc[0]); zero(acc[1]);
    const float *a = (dp ? Gb : Qb) + it * 32 * kLD, *bsrc = dp ? Vs : Ks;
    const float *const bt[2] = {bsrc, bsrc + 32 * kLD};
    mfma_tiles_k<false, true, 64, 2>(acc, a, kLD, bt, kLD, lr, lk);
    if (!dp) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = it * 32 + tile_row(r, lk), j = n * 32 + lr;
                Ps[i * kLD + j] = (i < qv && j < kv && (!MASK || m.sees(i, j))) ? exp_neg(acc[n][r] * scale - lses[i]) : 0.0f;
            }
    }
    __syncthreads();
    if (dp) {
        if (one) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = it * 32 + tile_row(r, lk);
                const float p0 = Ps[i * kLD + lr], p1 = Ps[i * kLD + 32 + lr];             // zero outside (qv, kv) and where hidden
                const float d = half_wave_sum_f32(p0 * acc[0][r] + p1 * acc[1][r], lk);
                Ds[i * kLD + lr] = (i < qv && lr < kv && (!MASK || m.sees(i, lr))) ? p0 * (acc[0][r] - d) * scale : 0.0f;
                Ds[i * kLD + 32 + lr] = (i < qv && 32 + lr < kv && (!MASK || m.sees(i, 32 + lr))) ? p1 * (acc[1][r] - d) * scale : 0.0f;
            }
        } else {
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = it * 32 + tile_row(r, lk), j = n * 32 + lr;
                    Ds[i * kLD + j] = (i < qv && j < kv && (!MASK || m.sees(i, j))) ? Ps[i * kLD + j] * (acc[n][r] - delta[i]) * scale : 0.0f;
                }
        }
    }
    __syncthreads();
}

constexpr size_t kFwdCrossLds = ((size_t)4 * kTile + 3 * kSB) * sizeof(float);     // 66 KB: two workgroups per CU
constexpr size_t kBwdCrossLds = ((size_t)6 * kTile + 2 * kSB) * sizeof(float);     // 98 KB: one workgroup per CU
static_assert(2 * kFwdCrossLds <= 160 * 1024 && kBwdCrossLds <= 160 * 1024, "LDS budget");

bool bad_stride(long long rs, int H) { return rs < (long long)H * 64 || rs % 4 != 0; }

}  // namespace
