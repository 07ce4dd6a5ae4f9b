// attn_prefix.hip -- cross-attention under a prefix-visibility mask: query rows i < split_q see the keys j < split_k, query rows
// i >= split_q see all Lk keys (the denoising queries of AdaPoinTr's decoder, reference models/AdaPoinTr.py:217-229 with
// models/Transformer_utils.py:100-120, where Lq = Lk = L and both splits are L - D).  Head dim 64, FP32 MFMA.  Contract: include/upp_hip.h
// upp_xattn_prefix_fwd / upp_xattn_prefix_bwd.
//
// The three kernels are those of attn_cross.hip (64-row query blocks, K / V streamed in 64-key blocks in ascending order under the online
// softmax; backward: one kernel per key block for dK / dV, one per query block for dQ; the same LDS budgets) with
//   * a select on (row, key) wherever attn_cross.hip selects on `key < kv`: a hidden key's score becomes -inf before the row maximum and
//     its P and dS are the constant 0, whatever the score was (a NaN included) -- no arithmetic on a hidden score reaches a result;
//   * shorter walks: a query block wholly below split_q stops at the key block that holds split_k - 1 and stages only the keys below
//     split_k of it (the rest are zero rows, as keys >= Lk are); a key block wholly at or beyond split_k starts its query walk at the block
//     that holds split_q;
//   * the single-key-block form of the softmax-backward row sum (delta from the block's own P dP) for every query block whose rows see
//     one key block only: Lk <= 64 as in attn_cross.hip, and a block wholly below split_q when split_k <= 64 -- a prefix row that sees
//     one key has P = 1 and d_q = d_k = 0 exactly;
//   * a query block that straddles split_q walks every key block; its rows below split_q see nothing in the blocks beyond split_k, where
//     their maximum, sum and accumulator pass through with a rescale factor that is the constant 1.
// split_k >= 1 leaves every row a visible key in the first block, so no row maximum stays -inf.  With split_q == 0 or split_k == Lk every
// select is true and every walk is whole: the operations, and so the bits, are attn_cross.hip's.  A row's result does not depend on the
// rows that share its block, so rows < split_q carry the bits of upp_xattn_fwd on the first split_k keys and rows >= split_q those of
// upp_xattn_fwd on all keys.  Every output element is written by exactly one workgroup: no atomics, no workspace, no memset.
#include "attn_cross_tiles.h"

namespace {

__global__ __launch_bounds__(64 * kSW) void xattn_prefix_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                    const float *__restrict__ v, float *__restrict__ ctx,
                                                                    float *__restrict__ lse, int Lq, int Lk, int H, int nqb, size_t q_rs,
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
    const int kend = q0 + qv <= split_q ? split_k : Lk;  // keys this block walks: a block wholly below split_q stops at split_k
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
            for (int t = 0; t < 4; ++t) see[t] = lane < kv && (q0 + i0 + t >= split_q || k0 + lane < split_k);
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
                    const bool any = q0 + i0 + t >= split_q || k0 < split_k;
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
__global__ __launch_bounds__(64 * kSW) void xattn_prefix_bwd_kv_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                       const float *__restrict__ v, const float *__restrict__ ctx,
                                                                       const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                                                       float *__restrict__ d_k, float *__restrict__ d_v, int Lq, int Lk, int H,
                                                                       int nkb, size_t q_rs, size_t k_rs, size_t v_rs, size_t dk_rs,
                                                                       size_t dv_rs, float scale, int split_q, int split_k) {
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
    const int qbegin = k0 >= split_k ? split_q / kSB * kSB : 0;     // a key block wholly beyond split_k is seen by rows >= split_q only
    for (int q0 = qbegin; q0 < Lq; q0 += kSB) {
        const int qv = min(kSB, Lq - q0);
        // the single-key-block form of the row sum wherever every key a row of this query block sees lies in one key block: Lk <= 64, or a
        // block wholly below split_q with split_k <= 64 (uniform over the block; the dQ kernel decides the same way)
        const bool one = (q0 + qv <= split_q ? split_k : Lk) <= kSB;
        {
            float *const dst[2] = {Qb, Gb};
            const float *const src[2] = {qbase + (size_t)q0 * q_rs, gbase + (size_t)q0 * cs};
            const size_t strides[2] = {q_rs, cs};
            stage_rows<2>(dst, src, strides, qv);
        }
        xattn_row_stats(gbase + (size_t)q0 * cs, obase + (size_t)q0 * cs, lbase + q0, cs, qv, delta, lses, wave, lane);
        __syncthreads();
        xattn_p_ds<true>(Qb, Gb, Ks, Vs, Ps, Ds, lses, delta, qv, kv, scale, one, wave, lr, lk, PrefixMask{q0, k0, split_q, split_k});
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
__global__ __launch_bounds__(64 * kSW) void xattn_prefix_bwd_q_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                      const float *__restrict__ v, const float *__restrict__ ctx,
                                                                      const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                                                      float *__restrict__ d_q, int Lq, int Lk, int H, int nqb, size_t q_rs,
                                                                      size_t k_rs, size_t v_rs, size_t dq_rs, float scale, int split_q, int split_k) {
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
    xattn_row_stats(gbase + (size_t)q0 * cs, obase + (size_t)q0 * cs, lse + ((size_t)b * H + hh) * Lq + q0, cs, qv, delta, lses, wave, lane);
    const int it = wave & 1, kh = wave >> 1;
    f32x16 acc[2];
    zero(acc[0]); zero(acc[1]);
    const int kend = q0 + qv <= split_q ? split_k : Lk;             // as in the forward kernel
    const bool one = kend <= kSB;                                   // every key this block's rows see lies in one key block
    for (int k0 = 0; k0 < kend; k0 += kSB) {
        const int kv = min(kSB, kend - k0);
        {
            float *const dst[2] = {Ks, Vs};
            const float *const src[2] = {kbase + (size_t)k0 * k_rs, vbase + (size_t)k0 * v_rs};
            const size_t strides[2] = {k_rs, v_rs};
            stage_rows<2>(dst, src, strides, kv);
        }
        __syncthreads();
        xattn_p_ds<true>(Qb, Gb, Ks, Vs, Ps, Ds, lses, delta, qv, kv, scale, one, wave, lr, lk, PrefixMask{q0, k0, split_q, split_k});
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

}  // namespace

extern "C" int upp_xattn_prefix_fwd(const float *q, const float *k, const float *v, float *ctx, float *lse, int B, int Lq, int Lk, int H,
                                    int head_dim, long long q_rs, long long k_rs, long long v_rs, float scale, int split_q, int split_k, void *stream) {
    if (!q || !k || !v || !ctx || !lse || B < 0 || Lq < 1 || Lk < 1 || H < 1) return UPP_E_BADARG;
    if (head_dim != 64 || Lq > UPP_ATTN_MAX_L || Lk > UPP_ATTN_MAX_L) return UPP_E_RANGE;
    if (bad_stride(q_rs, H) || bad_stride(k_rs, H) || bad_stride(v_rs, H)) return UPP_E_BADARG;
    if (split_q < 0 || split_q > Lq || split_k < 1 || split_k > Lk) return UPP_E_BADARG;
    if (B == 0) return 0;
    static std::atomic<bool> raised{false};
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(xattn_prefix_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFwdCrossLds);
        if (e != hipSuccess) return (int)e;
        raised = true;
    }
    const int nqb = (Lq + kSB - 1) / kSB;
    hipLaunchKernelGGL(xattn_prefix_fwd_kernel, dim3(B * H * nqb), dim3(64 * kSW), kFwdCrossLds, (hipStream_t)stream, q, k, v, ctx, lse, Lq, Lk, H,
                       nqb, (size_t)q_rs, (size_t)k_rs, (size_t)v_rs, scale, split_q, split_k);
    return upp_launch_status();
}

extern "C" int upp_xattn_prefix_bwd(const float *q, const float *k, const float *v, const float *ctx, const float *d_ctx, const float *lse,
                                    float *d_q, float *d_k, float *d_v, int B, int Lq, int Lk, int H, int head_dim, long long q_rs,
                                    long long k_rs, long long v_rs, long long dq_rs, long long dk_rs, long long dv_rs, float scale, int split_q, int split_k,
                                    void *stream) {
    if (!q || !k || !v || !ctx || !d_ctx || !lse || !d_q || !d_k || !d_v || B < 0 || Lq < 1 || Lk < 1 || H < 1) return UPP_E_BADARG;
    if (head_dim != 64 || Lq > UPP_ATTN_MAX_L || Lk > UPP_ATTN_MAX_L) return UPP_E_RANGE;
    if (bad_stride(q_rs, H) || bad_stride(k_rs, H) || bad_stride(v_rs, H) || bad_stride(dq_rs, H) || bad_stride(dk_rs, H) || bad_stride(dv_rs, H))
        return UPP_E_BADARG;
    if (split_q < 0 || split_q > Lq || split_k < 1 || split_k > Lk) return UPP_E_BADARG;
    if (B == 0) return 0;
    static std::atomic<bool> raised{false};
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(xattn_prefix_bwd_kv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBwdCrossLds);
        if (e != hipSuccess) return (int)e;
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(xattn_prefix_bwd_q_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBwdCrossLds);
        if (e != hipSuccess) return (int)e;
        raised = true;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nqb = (Lq + kSB - 1) / kSB, nkb = (Lk + kSB - 1) / kSB;
    hipLaunchKernelGGL(xattn_prefix_bwd_kv_kernel, dim3(B * H * nkb), dim3(64 * kSW), kBwdCrossLds, st, q, k, v, ctx, d_ctx, lse, d_k, d_v, Lq, Lk, H,
                       nkb, (size_t)q_rs, (size_t)k_rs, (size_t)v_rs, (size_t)dk_rs, (size_t)dv_rs, scale, split_q, split_k);
    int rc = upp_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(xattn_prefix_bwd_q_kernel, dim3(B * H * nqb), dim3(64 * kSW), kBwdCrossLds, st, q, k, v, ctx, d_ctx, lse, d_q, Lq, Lk, H,
                       nqb, (size_t)q_rs, (size_t)k_rs, (size_t)v_rs, (size_t)dq_rs, scale, split_q, split_k);
    return upp_launch_status();
}
