// attn_stream.hip -- the streaming attention family on FP32 MFMA, head dim 64: one set of kernel bodies behind three sets of entry points.
//   self-attention    upp_attn_fwd / upp_attn_bwd (block.hip) for 161 ... UPP_ATTN_MAX_L tokens of a packed qkv (models with more than 128
//                     groups; reference models/Point_MAE_pretask_dev.py:186-193): attn_stream_*_kernel
//   cross-attention   upp_xattn_fwd / upp_xattn_bwd, queries and keys from two sequences, 1 <= Lq, Lk <= UPP_ATTN_MAX_L, each operand with
//                     its own row stride (CrossAttention of the PoinTr family, reference models/Transformer.py:120-155): xattn_*_kernel
//   prefix visibility upp_xattn_prefix_fwd / upp_xattn_prefix_bwd: cross-attention in which query rows i < split_q see the keys
//                     j < split_k and rows i >= split_q see all Lk keys (AdaPoinTr's denoising queries, reference models/AdaPoinTr.py:217-229
//                     with models/Transformer_utils.py:100-120, where Lq = Lk = L and both splits are L - D): xattn_prefix_*_kernel
// Contracts: include/upp_hip.h.
//
// The walk.  Nothing of length L stays resident: a workgroup (4 waves) owns one 64-row block and streams the other side through the LDS in
// blocks of 64 rows, in ascending order.
//   forward    : one workgroup per (sample, head, query block).  Per key block S = Q_b K_j^T (4 tiles, one per wave) -> online softmax
//                in the LDS strip (running row max m and row sum l; P = exp(s - m_new)) -> O = O * exp(m_old - m_new) + P V_j (one
//                accumulator tile per wave, in registers across the whole walk).  At the end O / l and lse = m + log l.
//   backward kv: one workgroup per (sample, head, key block), walks the query blocks: dV_j += P^T dO_i, dK_j += dS^T Q_i.
//   backward q : one workgroup per (sample, head, query block), walks the key blocks: dQ_i += dS K_j; each wave sums one half of every key
//                block's keys and the two halves are added once at the end, keys 0 ... 31 first.
//                Both recompute P = exp(s scale - lse) and dS = P (dO V^T - delta) scale.
// Summation order.  Every output element is written by exactly one workgroup and sums run in ascending block order: no atomics, no
// workspace, no memset, two runs give the same bits.  Keys >= Lk of the last block have P = 0 exactly and zero K / V rows; query rows >= Lq
// are zero rows in the LDS that are never read from global memory and never stored.  Every product is a set of 32x32 tiles of
// v_mfma_f32_32x32x2_f32 (attn_tiles.h).
// The mask rule (MASK).  A select on (row, key) stands wherever the unmasked kernels select on `key < kv`: a hidden key's score becomes -inf
// before the row maximum and its P and dS are the constant 0, whatever the score was (a NaN included) -- no arithmetic on a hidden score
// reaches a result.  Walks are shorter: a query block wholly below split_q stops at the key block that holds split_k - 1 and stages only the
// keys below split_k of it (the rest are zero rows, as keys >= Lk are); a key block wholly at or beyond split_k starts its query walk at the
// block that holds split_q.  A query block that straddles split_q walks every key block; its rows below split_q see nothing in the blocks
// beyond split_k, where their maximum, sum and accumulator pass through with a rescale factor that is the constant 1.  split_k >= 1 leaves
// every row a visible key in the first block, so no row maximum stays -inf.  A row's result does not depend on the rows that share its
// block, so rows < split_q carry the bits of upp_xattn_fwd on the first split_k keys and rows >= split_q those of upp_xattn_fwd on all keys;
// with split_q == 0 or split_k == Lk every select is true and every walk is whole: the bits are the unmasked kernels'.
// The single-block delta rule (SINGLE).  With more than one key block delta_i = sum_c dO_ic O_ic, from ctx.  Where every key that the rows
// of a query block see lies in one key block (Lk <= 64, or a block wholly below split_q with split_k <= 64), the whole softmax row is in the
// block and delta_i = sum_j P_ij dP_ij is formed from the block's own P and dP -- the sum the torch formulation takes -- so that a row with
// one key (P = 1) has dS = 0 exactly, not the rounding difference between two summation orders.
// Instantiations.  Every mask test is guarded by the compile-time flag (`!MASK || ...`, `MASK && ...`), so the unmasked kernels hold no
// trace of the splits; splits of (0, Lk) at run time would not fold.  The self-attention kernels are <MASK = false, SINGLE = false>: they are
// dispatched beyond 160 tokens only, where the single-block form can never be taken, and with it compiled in the two backward kernels
// carry 63 more VGPRs and about 1,000 more instructions.  They derive q, k, v (and d_k, d_v) from the packed operand inside the kernel; for
// Lq == Lk and operands that are views of one packed qkv the cross-attention kernels <false, true> give the same bits.  The
// prefix-visibility kernels are <true, true>.
#include <initializer_list>

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
__device__ __forceinline__ void stream_row_stats(const float *__restrict__ g, const float *__restrict__ o, const float *__restrict__ l,
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
// accumulator chains per wave); dP stays in registers until P is in the LDS.  `one` (uniform over the workgroup; compiled in under SINGLE
// only): delta is the row sum of P dP of this block instead of the `delta` strip.  MASK: entries that `m` hides are zero as well, by a
// select on the index and not by arithmetic on the score (a NaN score of a hidden key gives P = 0).  Ends on a barrier.
template <bool MASK, bool SINGLE>
__device__ __forceinline__ void xattn_p_ds(const float *Qb, const float *Gb, const float *Ks, const float *Vs, float *Ps, float *Ds,
                                           const float *lses, const float *delta, int qv, int kv, float scale, bool one, int wave, int lr,
                                           int lk, const PrefixMask m) {
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
        if (SINGLE && one) {
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

// ctx and lse of one query block
template <bool MASK>
__device__ __forceinline__ void stream_fwd(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                           float *__restrict__ ctx, float *__restrict__ lse, int Lq, int Lk, int H, int nqb, size_t q_rs,
                                           size_t k_rs, size_t v_rs, float scale, int split_q, int split_k) {
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
    const int kend = MASK && q0 + qv <= split_q ? split_k : Lk;     // keys this block walks: a block wholly below split_q stops at split_k
    for (int k0 = 0; k0 < kend; k0 += kSB) {
        const int kv = min(kSB, kend - k0);              // >= 1; the first block holds key 0, which every row sees: no row max stays -inf
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
            bool see[4];                                 // this lane's key is visible to row i0 + t: decided on indices alone
#pragma unroll
            for (int t = 0; t < 4; ++t) see[t] = lane < kv && (!MASK || q0 + i0 + t >= split_q || k0 + lane < split_k);
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = see[t] ? Ss[(i0 + t) * kLD + lane] : -__builtin_inff();
#pragma unroll
            for (int t = 0; t < 4; ++t) { mo[t] = ms[i0 + t]; mn[t] = fmaxf(mo[t], wave_max_f32(s[t])); }
#pragma unroll
            for (int t = 0; t < 4; ++t) p[t] = see[t] ? exp_neg(s[t] - mn[t]) : 0.0f;          // hidden keys and keys >= Lk contribute exactly nothing
#pragma unroll
            for (int t = 0; t < 4; ++t) sum[t] = wave_sum_f32(p[t]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                Ss[(i0 + t) * kLD + lane] = p[t];
                if (lane == 0) {
                    // first block: exp(-inf) = 0 against l = 0 and O = 0.  A row below split_q in a block beyond split_k sees no key:
                    // its maximum is unchanged, its sum is 0 and its rescale factor is the constant 1.
                    const bool any = !MASK || q0 + i0 + t >= split_q || k0 < split_k;
                    const float a = any ? exp_neg(mo[t] - mn[t]) : 1.0f;
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

// dK and dV of one key block.  Waves 0, 1: dV rows 32 jt ... (both channel tiles), waves 2, 3: dK rows 32 jt ...; the accumulators
// stay in registers across the walk over the query blocks and are stored once.
template <bool MASK, bool SINGLE>
__device__ __forceinline__ void stream_bwd_kv(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                              const float *__restrict__ ctx, const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                              float *__restrict__ d_k, float *__restrict__ d_v, int Lq, int Lk, int H, int nkb, size_t q_rs,
                                              size_t k_rs, size_t v_rs, size_t dk_rs, size_t dv_rs, float scale, int split_q, int split_k) {
    extern __shared__ float sm[];
    float *Ks = sm, *Vs = Ks + kTile, *Qb = Vs + kTile, *Gb = Qb + kTile, *Ps = Gb + kTile, *Ds = Ps + kTile, *delta = Ds + kTile, *lses = delta + kSB;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lk = lane >> 5;
    const int wg = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int bh = wg / nkb, kb = wg - bh * nkb, b = bh / H, hh = bh - b * H;
    const int k0 = kb * kSB, kv = min(kSB, Lk - k0);
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
    const int qbegin = MASK && k0 >= split_k ? split_q / kSB * kSB : 0;     // a key block wholly beyond split_k is seen by rows >= split_q only
    for (int q0 = qbegin; q0 < Lq; q0 += kSB) {
        const int qv = min(kSB, Lq - q0);
        // the single-key-block form of the row sum wherever every key a row of this query block sees lies in one key block: Lk <= 64, or a
        // block wholly below split_q with split_k <= 64 (uniform over the block; the dQ kernel decides the same way)
        const bool one = SINGLE && (MASK && q0 + qv <= split_q ? split_k : Lk) <= kSB;
        {
            float *const dst[2] = {Qb, Gb};
            const float *const src[2] = {qbase + (size_t)q0 * q_rs, gbase + (size_t)q0 * cs};
            const size_t strides[2] = {q_rs, cs};
            stage_rows<2>(dst, src, strides, qv);
        }
        stream_row_stats(gbase + (size_t)q0 * cs, obase + (size_t)q0 * cs, lbase + q0, cs, qv, delta, lses, wave, lane);
        __syncthreads();
        xattn_p_ds<MASK, SINGLE>(Qb, Gb, Ks, Vs, Ps, Ds, lses, delta, qv, kv, scale, one, wave, lr, lk, PrefixMask{q0, k0, split_q, split_k});
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
template <bool MASK, bool SINGLE>
__device__ __forceinline__ void stream_bwd_q(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                             const float *__restrict__ ctx, const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                             float *__restrict__ d_q, int Lq, int Lk, int H, int nqb, size_t q_rs, size_t k_rs, size_t v_rs,
                                             size_t dq_rs, float scale, int split_q, int split_k) {
    extern __shared__ float sm[];
    float *Ks = sm, *Vs = Ks + kTile, *Qb = Vs + kTile, *Gb = Qb + kTile, *Ps = Gb + kTile, *Ds = Ps + kTile, *delta = Ds + kTile, *lses = delta + kSB;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lk = lane >> 5;
    const int wg = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int bh = wg / nqb, qb = wg - bh * nqb, b = bh / H, hh = bh - b * H;
    const int q0 = qb * kSB, qv = min(kSB, Lq - q0);
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
    stream_row_stats(gbase + (size_t)q0 * cs, obase + (size_t)q0 * cs, lse + ((size_t)b * H + hh) * Lq + q0, cs, qv, delta, lses, wave, lane);
    const int it = wave & 1, kh = wave >> 1;
    f32x16 acc[2];
    zero(acc[0]); zero(acc[1]);
    const int kend = MASK && q0 + qv <= split_q ? split_k : Lk;     // as in the forward
    const bool one = SINGLE && kend <= kSB;                         // every key this block's rows see lies in one key block
    for (int k0 = 0; k0 < kend; k0 += kSB) {
        const int kv = min(kSB, kend - k0);
        {
            float *const dst[2] = {Ks, Vs};
            const float *const src[2] = {kbase + (size_t)k0 * k_rs, vbase + (size_t)k0 * v_rs};
            const size_t strides[2] = {k_rs, v_rs};
            stage_rows<2>(dst, src, strides, kv);
        }
        __syncthreads();
        xattn_p_ds<MASK, SINGLE>(Qb, Gb, Ks, Vs, Ps, Ds, lses, delta, qv, kv, scale, one, wave, lr, lk, PrefixMask{q0, k0, split_q, split_k});
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

// ---- the nine kernels: names and parameter lists are what profiles, tests and DESIGN.md know them by
#define STREAM_KERNEL __global__ __launch_bounds__(64 * kSW) void

STREAM_KERNEL attn_stream_fwd_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, float *__restrict__ lse, int L, int H, int nqb,
                                     float scale) {
    const size_t rs = (size_t)3 * H * 64;
    stream_fwd<false>(qkv, qkv + H * 64, qkv + 2 * H * 64, ctx, lse, L, L, H, nqb, rs, rs, rs, scale, 0, 0);
}

STREAM_KERNEL attn_stream_bwd_kv_kernel(const float *__restrict__ qkv, const float *__restrict__ ctx, const float *__restrict__ d_ctx,
                                        const float *__restrict__ lse, float *__restrict__ d_qkv, int L, int H, int nkb, float scale) {
    const size_t rs = (size_t)3 * H * 64;
    stream_bwd_kv<false, false>(qkv, qkv + H * 64, qkv + 2 * H * 64, ctx, d_ctx, lse, d_qkv + H * 64, d_qkv + 2 * H * 64, L, L, H, nkb, rs, rs,
                                rs, rs, rs, scale, 0, 0);
}

STREAM_KERNEL attn_stream_bwd_q_kernel(const float *__restrict__ qkv, const float *__restrict__ ctx, const float *__restrict__ d_ctx,
                                       const float *__restrict__ lse, float *__restrict__ d_qkv, int L, int H, int nqb, float scale) {
    const size_t rs = (size_t)3 * H * 64;
    stream_bwd_q<false, false>(qkv, qkv + H * 64, qkv + 2 * H * 64, ctx, d_ctx, lse, d_qkv, L, L, H, nqb, rs, rs, rs, rs, scale, 0, 0);
}

STREAM_KERNEL xattn_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, float *__restrict__ ctx,
                               float *__restrict__ lse, int Lq, int Lk, int H, int nqb, size_t q_rs, size_t k_rs, size_t v_rs, float scale) {
    stream_fwd<false>(q, k, v, ctx, lse, Lq, Lk, H, nqb, q_rs, k_rs, v_rs, scale, 0, 0);
}

STREAM_KERNEL xattn_bwd_kv_kernel(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                  const float *__restrict__ ctx, const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                  float *__restrict__ d_k, float *__restrict__ d_v, int Lq, int Lk, int H, int nkb, size_t q_rs, size_t k_rs,
                                  size_t v_rs, size_t dk_rs, size_t dv_rs, float scale) {
    stream_bwd_kv<false, true>(q, k, v, ctx, d_ctx, lse, d_k, d_v, Lq, Lk, H, nkb, q_rs, k_rs, v_rs, dk_rs, dv_rs, scale, 0, 0);
}

STREAM_KERNEL xattn_bwd_q_kernel(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                 const float *__restrict__ ctx, const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                 float *__restrict__ d_q, int Lq, int Lk, int H, int nqb, size_t q_rs, size_t k_rs, size_t v_rs, size_t dq_rs,
                                 float scale) {
    stream_bwd_q<false, true>(q, k, v, ctx, d_ctx, lse, d_q, Lq, Lk, H, nqb, q_rs, k_rs, v_rs, dq_rs, scale, 0, 0);
}

STREAM_KERNEL xattn_prefix_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                      float *__restrict__ ctx, float *__restrict__ lse, int Lq, int Lk, int H, int nqb, size_t q_rs, size_t k_rs,
                                      size_t v_rs, float scale, int split_q, int split_k) {
    stream_fwd<true>(q, k, v, ctx, lse, Lq, Lk, H, nqb, q_rs, k_rs, v_rs, scale, split_q, split_k);
}

STREAM_KERNEL xattn_prefix_bwd_kv_kernel(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                         const float *__restrict__ ctx, const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                         float *__restrict__ d_k, float *__restrict__ d_v, int Lq, int Lk, int H, int nkb, size_t q_rs,
                                         size_t k_rs, size_t v_rs, size_t dk_rs, size_t dv_rs, float scale, int split_q, int split_k) {
    stream_bwd_kv<true, true>(q, k, v, ctx, d_ctx, lse, d_k, d_v, Lq, Lk, H, nkb, q_rs, k_rs, v_rs, dk_rs, dv_rs, scale, split_q, split_k);
}

STREAM_KERNEL xattn_prefix_bwd_q_kernel(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                        const float *__restrict__ ctx, const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                        float *__restrict__ d_q, int Lq, int Lk, int H, int nqb, size_t q_rs, size_t k_rs, size_t v_rs,
                                        size_t dq_rs, float scale, int split_q, int split_k) {
    stream_bwd_q<true, true>(q, k, v, ctx, d_ctx, lse, d_q, Lq, Lk, H, nqb, q_rs, k_rs, v_rs, dq_rs, scale, split_q, split_k);
}
#undef STREAM_KERNEL

constexpr size_t kFwdStreamLds = ((size_t)4 * kTile + 3 * kSB) * sizeof(float);     // 66 KB: two workgroups per CU
constexpr size_t kBwdStreamLds = ((size_t)6 * kTile + 2 * kSB) * sizeof(float);     // 98 KB: one workgroup per CU
static_assert(2 * kFwdStreamLds <= 160 * 1024 && kBwdStreamLds <= 160 * 1024, "LDS budget");

// raises Kernel's dynamic-LDS limit on the first call, then launches it on `blocks` workgroups
template <auto Kernel, typename... Args>
int launch_stream(size_t lds, int blocks, hipStream_t st, Args... args) {
    static std::atomic<bool> raised{false};
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        raised = true;
    }
    hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(64 * kSW), lds, st, args...);
    return upp_launch_status();
}

int blocks_of(int L) { return (L + kSB - 1) / kSB; }

// what the upp_xattn_* entry points refuse, in the order tests/test_cross_attention_host.py and tests/test_prefix_attention_host.py pin;
// `splits` is null for the unmasked pair.  The caller returns 0 for B == 0 after this.
int xattn_refusal(std::initializer_list<const void *> ptrs, int B, int Lq, int Lk, int H, int head_dim, std::initializer_list<long long> strides,
                  const int *splits) {
    for (const void *p : ptrs)
        if (!p) return UPP_E_BADARG;
    if (B < 0 || Lq < 1 || Lk < 1 || H < 1) return UPP_E_BADARG;
    if (head_dim != 64 || Lq > UPP_ATTN_MAX_L || Lk > UPP_ATTN_MAX_L) return UPP_E_RANGE;
    for (long long rs : strides)
        if (rs < (long long)H * 64 || rs % 4 != 0) return UPP_E_BADARG;
    if (splits && (splits[0] < 0 || splits[0] > Lq || splits[1] < 1 || splits[1] > Lk)) return UPP_E_BADARG;
    return 0;
}

}  // namespace

// called by upp_attn_fwd / upp_attn_bwd (block.hip) for 160 < L <= UPP_ATTN_MAX_L
int upp_attn_fwd_stream(const float *qkv, float *ctx, float *lse, int B, int L, int H, float scale, hipStream_t st) {
    const int nqb = blocks_of(L);
    return launch_stream<attn_stream_fwd_kernel>(kFwdStreamLds, B * H * nqb, st, qkv, ctx, lse, L, H, nqb, scale);
}

int upp_attn_bwd_stream(const float *qkv, const float *ctx, const float *d_ctx, const float *lse, float *d_qkv, int B, int L, int H,
                        float scale, hipStream_t st) {
    const int nb = blocks_of(L);
    if (int rc = launch_stream<attn_stream_bwd_kv_kernel>(kBwdStreamLds, B * H * nb, st, qkv, ctx, d_ctx, lse, d_qkv, L, H, nb, scale)) return rc;
    return launch_stream<attn_stream_bwd_q_kernel>(kBwdStreamLds, B * H * nb, st, qkv, ctx, d_ctx, lse, d_qkv, L, H, nb, scale);
}

extern "C" int upp_xattn_fwd(const float *q, const float *k, const float *v, float *ctx, float *lse, int B, int Lq, int Lk, int H,
                             int head_dim, long long q_rs, long long k_rs, long long v_rs, float scale, void *stream) {
    if (int rc = xattn_refusal({q, k, v, ctx, lse}, B, Lq, Lk, H, head_dim, {q_rs, k_rs, v_rs}, nullptr)) return rc;
    if (B == 0) return 0;
    const int nqb = blocks_of(Lq);
    return launch_stream<xattn_fwd_kernel>(kFwdStreamLds, B * H * nqb, (hipStream_t)stream, q, k, v, ctx, lse, Lq, Lk, H, nqb, (size_t)q_rs,
                                           (size_t)k_rs, (size_t)v_rs, scale);
}

extern "C" int upp_xattn_bwd(const float *q, const float *k, const float *v, const float *ctx, const float *d_ctx, const float *lse,
                             float *d_q, float *d_k, float *d_v, int B, int Lq, int Lk, int H, int head_dim, long long q_rs,
                             long long k_rs, long long v_rs, long long dq_rs, long long dk_rs, long long dv_rs, float scale, void *stream) {
    if (int rc = xattn_refusal({q, k, v, ctx, d_ctx, lse, d_q, d_k, d_v}, B, Lq, Lk, H, head_dim, {q_rs, k_rs, v_rs, dq_rs, dk_rs, dv_rs}, nullptr))
        return rc;
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int nqb = blocks_of(Lq), nkb = blocks_of(Lk);
    if (int rc = launch_stream<xattn_bwd_kv_kernel>(kBwdStreamLds, B * H * nkb, st, q, k, v, ctx, d_ctx, lse, d_k, d_v, Lq, Lk, H, nkb, (size_t)q_rs,
                                                    (size_t)k_rs, (size_t)v_rs, (size_t)dk_rs, (size_t)dv_rs, scale))
        return rc;
    return launch_stream<xattn_bwd_q_kernel>(kBwdStreamLds, B * H * nqb, st, q, k, v, ctx, d_ctx, lse, d_q, Lq, Lk, H, nqb, (size_t)q_rs,
                                             (size_t)k_rs, (size_t)v_rs, (size_t)dq_rs, scale);
}

extern "C" int upp_xattn_prefix_fwd(const float *q, const float *k, const float *v, float *ctx, float *lse, int B, int Lq, int Lk, int H,
                                    int head_dim, long long q_rs, long long k_rs, long long v_rs, float scale, int split_q, int split_k, void *stream) {
    const int splits[2] = {split_q, split_k};
    if (int rc = xattn_refusal({q, k, v, ctx, lse}, B, Lq, Lk, H, head_dim, {q_rs, k_rs, v_rs}, splits)) return rc;
    if (B == 0) return 0;
    const int nqb = blocks_of(Lq);
    return launch_stream<xattn_prefix_fwd_kernel>(kFwdStreamLds, B * H * nqb, (hipStream_t)stream, q, k, v, ctx, lse, Lq, Lk, H, nqb, (size_t)q_rs,
                                                  (size_t)k_rs, (size_t)v_rs, scale, split_q, split_k);
}

extern "C" int upp_xattn_prefix_bwd(const float *q, const float *k, const float *v, const float *ctx, const float *d_ctx, const float *lse,
                                    float *d_q, float *d_k, float *d_v, int B, int Lq, int Lk, int H, int head_dim, long long q_rs,
                                    long long k_rs, long long v_rs, long long dq_rs, long long dk_rs, long long dv_rs, float scale, int split_q, int split_k,
                                    void *stream) {
    const int splits[2] = {split_q, split_k};
    if (int rc = xattn_refusal({q, k, v, ctx, d_ctx, lse, d_q, d_k, d_v}, B, Lq, Lk, H, head_dim, {q_rs, k_rs, v_rs, dq_rs, dk_rs, dv_rs}, splits))
        return rc;
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int nqb = blocks_of(Lq), nkb = blocks_of(Lk);
    if (int rc = launch_stream<xattn_prefix_bwd_kv_kernel>(kBwdStreamLds, B * H * nkb, st, q, k, v, ctx, d_ctx, lse, d_k, d_v, Lq, Lk, H, nkb,
                                                           (size_t)q_rs, (size_t)k_rs, (size_t)v_rs, (size_t)dk_rs, (size_t)dv_rs, scale, split_q, split_k))
        return rc;
    return launch_stream<xattn_prefix_bwd_q_kernel>(kBwdStreamLds, B * H * nqb, st, q, k, v, ctx, d_ctx, lse, d_q, Lq, Lk, H, nqb, (size_t)q_rs,
                                                    (size_t)k_rs, (size_t)v_rs, (size_t)dq_rs, scale, split_q, split_k);
}
