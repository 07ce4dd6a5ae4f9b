// attn_cross.hip -- attention whose queries and keys come from two sequences (CrossAttention of the PoinTr family, reference
// models/Transformer.py:120-155), head dim 64, on FP32 MFMA.  Contract: include/upp_hip.h upp_xattn_fwd / upp_xattn_bwd.
//
// The structure, the block walk and the accumulation order are those of attn_stream.hip with the two lengths (Lq queries, Lk keys) and
// the three operand bases (q, k, v, each with its own row stride) separated; for Lq == Lk and operands that are views of one packed qkv
// the two files give the same bits wherever attn_stream.hip is dispatched.  One family serves every 1 <= Lq, Lk <= UPP_ATTN_MAX_L:
//   forward    : one workgroup (4 waves) per (sample, head, 64-row query block); K / V stream through the LDS in 64-key blocks in
//                ascending order under the online softmax; writes ctx and lse.
//   backward kv: one workgroup per (sample, head, 64-key block), walks the query blocks in ascending order: dV_j += P^T dO_i,
//                dK_j += dS^T Q_i.
//   backward q : one workgroup per (sample, head, query block), walks the key blocks in ascending order: dQ_i += dS K_j.
// Both backward kernels recompute P = exp(s scale - lse) and dS = P (dO V^T - delta) scale.  With more than one key block
// delta_i = sum_c dO_ic O_ic (from ctx, as attn_stream.hip forms it).  With a single key block (Lk <= 64) the whole softmax row is in
// the block, and delta_i = sum_j P_ij dP_ij is formed from the block's own P and dP -- the sum the torch formulation takes -- so that a
// row with one key (P = 1) has dS = 0 exactly, not the rounding difference between two summation orders.
// Every output element is written by exactly one workgroup and sums run in ascending block order: no atomics, no workspace, no memset,
// two runs give the same bits.  Keys >= Lk of the last block have P = 0 exactly and zero K / V rows; query rows >= Lq are zero rows in
// the LDS that are never read from global memory and never stored.
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

__global__ __launch_bounds__(64 * kSW) void xattn_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                             const float *__restrict__ v, float *__restrict__ ctx,
                                                             float *__restrict__ lse, int Lq, int Lk, int H, int nqb, size_t q_rs,
                                                             size_t k_rs, size_t v_rs, float scale) {
    extern __shared__ float sm[];
    float *Qb = sm, *Ks = Qb + kTile, *Vs = Ks + kTile, *Ss = Vs + kTile, *ms = Ss + kTile, *ls = ms + kSB, *al = ls + kSB;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lk = lane >> 5;
    const int wg = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int bh = wg / nqb, qb = wg - bh * nqb, b = bh / H, hh = bh - b * H;
    const int q0 = qb * kSB, qv = min(kSB, Lq - q0);
    const float *qbase = q + (size_t)b * Lq * q_rs + (size_t)hh * 64;
    const float *kbase = k + (size_t)b * Lk * k_rs + (size_t)hh * 64;
    const float *vbase = v + (size_t)b * Lk * v_rs + (size_t)hh * 64;
    {
        float *const dst[1] = {Qb};
        const float *const src[1] = {qbase + (size_t)q0 * q_rs};
        const size_t strides[1] = {q_rs};
        stage_rows<1>(dst, src, strides, qv);
    }
    if (threadIdx.x < kSB) { ms[threadIdx.x] = -__builtin_inff(); ls[threadIdx.x] = 0.0f; }
    const int it = wave & 1, jt = wave >> 1;             // S tile (it, jt) and O tile (it, channels 32 jt ...)
    f32x16 o; zero(o);
    for (int k0 = 0; k0 < Lk; k0 += kSB) {
        const int kv = min(kSB, Lk - k0);                // >= 1: every key block holds a real key, so no row max stays -inf
        {
            float *const dst[2] = {Ks, Vs};
            const float *const src[2] = {kbase + (size_t)k0 * k_rs, vbase + (size_t)k0 * v_rs};
            const size_t strides[2] = {k_rs, v_rs};
            stage_rows<2>(dst, src, strides, kv);
        }
        __syncthreads();
        {
            f32x16 s; zero(s);
            mfma_tile_k<false, true, 64>(s, Qb + it * 32 * kLD, kLD, Ks + jt * 32 * kLD, kLD, lr, lk);
#pragma unroll
            for (int r = 0; r < 16; ++r) Ss[(it * 32 + tile_row(r, lk)) * kLD + jt * 32 + lr] = s[r] * scale;
        }
        __syncthreads();
        // online softmax of this block's 64 columns: 16 rows per wave, four per iteration, lane = key
        for (int i0 = wave * (kSB / kSW); i0 < (wave + 1) * (kSB / kSW); i0 += 4) {
            float s[4], mo[4], mn[4], p[4], sum[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = lane < kv ? Ss[(i0 + t) * kLD + lane] : -__builtin_inff();
#pragma unroll
            for (int t = 0; t < 4; ++t) { mo[t] = ms[i0 + t]; mn[t] = fmaxf(mo[t], wave_max_f32(s[t])); }
#pragma unroll
            for (int t = 0; t < 4; ++t) p[t] = lane < kv ? exp_neg(s[t] - mn[t]) : 0.0f;       // keys >= Lk contribute exactly nothing
#pragma unroll
            for (int t = 0; t < 4; ++t) sum[t] = wave_sum_f32(p[t]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                Ss[(i0 + t) * kLD + lane] = p[t];
                if (lane == 0) {
                    const float a = exp_neg(mo[t] - mn[t]);                  // first block: exp(-inf) = 0 against l = 0 and O = 0
                    ms[i0 + t] = mn[t];
                    ls[i0 + t] = ls[i0 + t] * a + sum[t];
                    al[i0 + t] = a;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= al[it * 32 + tile_row(r, lk)];
        mfma_tile_k<false, false, 64>(o, Ss + it * 32 * kLD, kLD, Vs + jt * 32, kLD, lr, lk);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = it * 32 + tile_row(r, lk);
        if (i < qv) ctx[((size_t)b * Lq + q0 + i) * (H * 64) + hh * 64 + jt * 32 + lr] = o[r] / ls[i];
    }
    if ((int)threadIdx.x < qv) lse[((size_t)b * H + hh) * Lq + q0 + threadIdx.x] = ms[threadIdx.x] + logf(ls[threadIdx.x]);
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

// P = exp(S scale - lse) and dS = P (dO V^T - delta) scale of one (64 query x 64 key) block into the strips Ps / Ds; entries of query
// rows >= qv and keys >= kv are zero.  Waves 0, 1 compute the two S tiles of query rows 32 it ..., waves 2, 3 the two dP tiles (two
// accumulator chains per wave); dP stays in registers until P is in the LDS.  `one` (Lk <= 64, uniform over the grid): delta is the
// row sum of P dP of this block instead of the `delta` strip.  Ends on a barrier.
__device__ __forceinline__ void xattn_p_ds(const float *Qb, const float *Gb, const float *Ks, const float *Vs, float *Ps, float *Ds,
                                           const float *lses, const float *delta, int qv, int kv, float scale, bool one, int wave, int lr,
                                           int lk) {
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
                Ps[i * kLD + j] = (i < qv && j < kv) ? exp_neg(acc[n][r] * scale - lses[i]) : 0.0f;
            }
    }
    __syncthreads();
    if (dp) {
        if (one) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = it * 32 + tile_row(r, lk);
                const float p0 = Ps[i * kLD + lr], p1 = Ps[i * kLD + 32 + lr];             // zero outside (qv, kv)
                const float d = half_wave_sum_f32(p0 * acc[0][r] + p1 * acc[1][r], lk);
                Ds[i * kLD + lr] = (i < qv && lr < kv) ? p0 * (acc[0][r] - d) * scale : 0.0f;
                Ds[i * kLD + 32 + lr] = (i < qv && 32 + lr < kv) ? p1 * (acc[1][r] - d) * scale : 0.0f;
            }
        } else {
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = it * 32 + tile_row(r, lk), j = n * 32 + lr;
                    Ds[i * kLD + j] = (i < qv && j < kv) ? Ps[i * kLD + j] * (acc[n][r] - delta[i]) * scale : 0.0f;
                }
        }
    }
    __syncthreads();
}

// dK and dV of one key block.  Waves 0, 1: dV rows 32 jt ... (both channel tiles), waves 2, 3: dK rows 32 jt ...; the accumulators
// stay in registers across the walk over the query blocks and are stored once.
__global__ __launch_bounds__(64 * kSW) void xattn_bwd_kv_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                const float *__restrict__ v, const float *__restrict__ ctx,
                                                                const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                                                float *__restrict__ d_k, float *__restrict__ d_v, int Lq, int Lk, int H,
                                                                int nkb, size_t q_rs, size_t k_rs, size_t v_rs, size_t dk_rs,
                                                                size_t dv_rs, float scale) {
    extern __shared__ float sm[];
    float *Ks = sm, *Vs = Ks + kTile, *Qb = Vs + kTile, *Gb = Qb + kTile, *Ps = Gb + kTile, *Ds = Ps + kTile, *delta = Ds + kTile, *lses = delta + kSB;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lk = lane >> 5;
    const int wg = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int bh = wg / nkb, kb = wg - bh * nkb, b = bh / H, hh = bh - b * H;
    const int k0 = kb * kSB, kv = min(kSB, Lk - k0);
    const bool one = nkb == 1;
    const size_t cs = (size_t)H * 64;
    const float *qbase = q + (size_t)b * Lq * q_rs + (size_t)hh * 64;
    const float *kbase = k + (size_t)b * Lk * k_rs + (size_t)hh * 64;
    const float *vbase = v + (size_t)b * Lk * v_rs + (size_t)hh * 64;
    float *dkbase = d_k + (size_t)b * Lk * dk_rs + (size_t)hh * 64;
    float *dvbase = d_v + (size_t)b * Lk * dv_rs + (size_t)hh * 64;
    const float *gbase = d_ctx + (size_t)b * Lq * cs + (size_t)hh * 64;
    const float *obase = ctx + (size_t)b * Lq * cs + (size_t)hh * 64;
    const float *lbase = lse + ((size_t)b * H + hh) * Lq;
    {
        float *const dst[2] = {Ks, Vs};
        const float *const src[2] = {kbase + (size_t)k0 * k_rs, vbase + (size_t)k0 * v_rs};
        const size_t strides[2] = {k_rs, v_rs};
        stage_rows<2>(dst, src, strides, kv);
    }
    const int jt = wave & 1;
    const bool dk = wave >= 2;
    f32x16 acc[2];
    zero(acc[0]); zero(acc[1]);
    for (int q0 = 0; q0 < Lq; q0 += kSB) {
        const int qv = min(kSB, Lq - q0);
        {
            float *const dst[2] = {Qb, Gb};
            const float *const src[2] = {qbase + (size_t)q0 * q_rs, gbase + (size_t)q0 * cs};
            const size_t strides[2] = {q_rs, cs};
            stage_rows<2>(dst, src, strides, qv);
        }
        xattn_row_stats(gbase + (size_t)q0 * cs, obase + (size_t)q0 * cs, lbase + q0, cs, qv, delta, lses, wave, lane);
        __syncthreads();
        xattn_p_ds(Qb, Gb, Ks, Vs, Ps, Ds, lses, delta, qv, kv, scale, one, wave, lr, lk);
        {   // dV += P^T dO_i (waves 0, 1), dK += dS^T Q_i (waves 2, 3): the contraction runs over the block's 64 query rows
            const float *a = (dk ? Ds : Ps) + jt * 32, *bsrc = dk ? Qb : Gb;
            const float *const bt[2] = {bsrc, bsrc + 32};
            mfma_tiles_k<true, false, 64, 2>(acc, a, kLD, bt, kLD, lr, lk);
        }
        __syncthreads();
    }
    float *obase_w = dk ? dkbase : dvbase;
    const size_t ors = dk ? dk_rs : dv_rs;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jt * 32 + tile_row(r, lk);
            if (j < kv) obase_w[(size_t)(k0 + j) * ors + n * 32 + lr] = acc[n][r];
        }
}

// dQ of one query block.  Wave (it, kh) accumulates dQ rows 32 it ... (both channel tiles) over keys 32 kh ... 32 kh + 31 of every key
// block; the two halves are added once at the end (kh = 0 first), through the LDS.
__global__ __launch_bounds__(64 * kSW) void xattn_bwd_q_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                               const float *__restrict__ v, const float *__restrict__ ctx,
                                                               const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                                               float *__restrict__ d_q, int Lq, int Lk, int H, int nqb, size_t q_rs,
                                                               size_t k_rs, size_t v_rs, size_t dq_rs, float scale) {
    extern __shared__ float sm[];
    float *Ks = sm, *Vs = Ks + kTile, *Qb = Vs + kTile, *Gb = Qb + kTile, *Ps = Gb + kTile, *Ds = Ps + kTile, *delta = Ds + kTile, *lses = delta + kSB;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lk = lane >> 5;
    const int wg = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int bh = wg / nqb, qb = wg - bh * nqb, b = bh / H, hh = bh - b * H;
    const int q0 = qb * kSB, qv = min(kSB, Lq - q0);
    const bool one = Lk <= kSB;
    const size_t cs = (size_t)H * 64;
    const float *qbase = q + (size_t)b * Lq * q_rs + (size_t)hh * 64;
    const float *kbase = k + (size_t)b * Lk * k_rs + (size_t)hh * 64;
    const float *vbase = v + (size_t)b * Lk * v_rs + (size_t)hh * 64;
    float *dbase = d_q + (size_t)b * Lq * dq_rs + (size_t)hh * 64;
    const float *gbase = d_ctx + (size_t)b * Lq * cs + (size_t)hh * 64;
    const float *obase = ctx + (size_t)b * Lq * cs + (size_t)hh * 64;
    {
        float *const dst[2] = {Qb, Gb};
        const float *const src[2] = {qbase + (size_t)q0 * q_rs, gbase + (size_t)q0 * cs};
        const size_t strides[2] = {q_rs, cs};
        stage_rows<2>(dst, src, strides, qv);
    }
    xattn_row_stats(gbase + (size_t)q0 * cs, obase + (size_t)q0 * cs, lse + ((size_t)b * H + hh) * Lq + q0, cs, qv, delta, lses, wave, lane);
    const int it = wave & 1, kh = wave >> 1;
    f32x16 acc[2];
    zero(acc[0]); zero(acc[1]);
    for (int k0 = 0; k0 < Lk; k0 += kSB) {
        const int kv = min(kSB, Lk - k0);
        {
            float *const dst[2] = {Ks, Vs};
            const float *const src[2] = {kbase + (size_t)k0 * k_rs, vbase + (size_t)k0 * v_rs};
            const size_t strides[2] = {k_rs, v_rs};
            stage_rows<2>(dst, src, strides, kv);
        }
        __syncthreads();
        xattn_p_ds(Qb, Gb, Ks, Vs, Ps, Ds, lses, delta, qv, kv, scale, one, wave, lr, lk);
        {
            const float *const bt[2] = {Ks + kh * 32 * kLD, Ks + kh * 32 * kLD + 32};
            mfma_tiles_k<false, false, 32, 2>(acc, Ds + it * 32 * kLD + kh * 32, kLD, bt, kLD, lr, lk);
        }
        __syncthreads();
    }
    if (kh) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) Ps[(it * 32 + tile_row(r, lk)) * kLD + n * 32 + lr] = acc[n][r];
    }
    __syncthreads();
    if (!kh) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = it * 32 + tile_row(r, lk);
                if (i < qv) dbase[(size_t)(q0 + i) * dq_rs + n * 32 + lr] = acc[n][r] + Ps[i * kLD + n * 32 + lr];
            }
    }
}

constexpr size_t kFwdCrossLds = ((size_t)4 * kTile + 3 * kSB) * sizeof(float);     // 66 KB: two workgroups per CU
constexpr size_t kBwdCrossLds = ((size_t)6 * kTile + 2 * kSB) * sizeof(float);     // 98 KB: one workgroup per CU
static_assert(2 * kFwdCrossLds <= 160 * 1024 && kBwdCrossLds <= 160 * 1024, "LDS budget");

bool bad_stride(long long rs, int H) { return rs < (long long)H * 64 || rs % 4 != 0; }

}  // namespace

extern "C" int upp_xattn_fwd(const float *q, const float *k, const float *v, float *ctx, float *lse, int B, int Lq, int Lk, int H,
                             int head_dim, long long q_rs, long long k_rs, long long v_rs, float scale, void *stream) {
    if (!q || !k || !v || !ctx || !lse || B < 0 || Lq < 1 || Lk < 1 || H < 1) return UPP_E_BADARG;
    if (head_dim != 64 || Lq > UPP_ATTN_MAX_L || Lk > UPP_ATTN_MAX_L) return UPP_E_RANGE;
    if (bad_stride(q_rs, H) || bad_stride(k_rs, H) || bad_stride(v_rs, H)) return UPP_E_BADARG;
    if (B == 0) return 0;
    static std::atomic<bool> raised{false};
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(xattn_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFwdCrossLds);
        if (e != hipSuccess) return (int)e;
        raised = true;
    }
    const int nqb = (Lq + kSB - 1) / kSB;
    hipLaunchKernelGGL(xattn_fwd_kernel, dim3(B * H * nqb), dim3(64 * kSW), kFwdCrossLds, (hipStream_t)stream, q, k, v, ctx, lse, Lq, Lk, H,
                       nqb, (size_t)q_rs, (size_t)k_rs, (size_t)v_rs, scale);
    return upp_launch_status();
}

extern "C" int upp_xattn_bwd(const float *q, const float *k, const float *v, const float *ctx, const float *d_ctx, const float *lse,
                             float *d_q, float *d_k, float *d_v, int B, int Lq, int Lk, int H, int head_dim, long long q_rs,
                             long long k_rs, long long v_rs, long long dq_rs, long long dk_rs, long long dv_rs, float scale, void *stream) {
    if (!q || !k || !v || !ctx || !d_ctx || !lse || !d_q || !d_k || !d_v || B < 0 || Lq < 1 || Lk < 1 || H < 1) return UPP_E_BADARG;
    if (head_dim != 64 || Lq > UPP_ATTN_MAX_L || Lk > UPP_ATTN_MAX_L) return UPP_E_RANGE;
    if (bad_stride(q_rs, H) || bad_stride(k_rs, H) || bad_stride(v_rs, H) || bad_stride(dq_rs, H) || bad_stride(dk_rs, H) || bad_stride(dv_rs, H))
        return UPP_E_BADARG;
    if (B == 0) return 0;
    static std::atomic<bool> raised{false};
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(xattn_bwd_kv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBwdCrossLds);
        if (e != hipSuccess) return (int)e;
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(xattn_bwd_q_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBwdCrossLds);
        if (e != hipSuccess) return (int)e;
        raised = true;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nqb = (Lq + kSB - 1) / kSB, nkb = (Lk + kSB - 1) / kSB;
    hipLaunchKernelGGL(xattn_bwd_kv_kernel, dim3(B * H * nkb), dim3(64 * kSW), kBwdCrossLds, st, q, k, v, ctx, d_ctx, lse, d_k, d_v, Lq, Lk, H,
                       nkb, (size_t)q_rs, (size_t)k_rs, (size_t)v_rs, (size_t)dk_rs, (size_t)dv_rs, scale);
    int rc = upp_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(xattn_bwd_q_kernel, dim3(B * H * nqb), dim3(64 * kSW), kBwdCrossLds, st, q, k, v, ctx, d_ctx, lse, d_q, Lq, Lk, H,
                       nqb, (size_t)q_rs, (size_t)k_rs, (size_t)v_rs, (size_t)dq_rs, scale);
    return upp_launch_status();
}
