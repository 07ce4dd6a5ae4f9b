// attn_stream.hip -- attention core on FP32 MFMA for sequences of 161 ... UPP_ATTN_MAX_L tokens, head dim 64 (models with more than 128
// groups: 256 / 512 groups for 4096 / 8192-point clouds).  Same contract as attn_flash16.hip (L <= 96) and attn_long.hip (L <= 160); see
// include/upp_hip.h upp_attn_fwd / upp_attn_bwd and reference models/Point_MAE_pretask_dev.py:186-193.
//
// Nothing of length L stays resident: a workgroup (4 waves) owns one 64-row block and streams the other side through the LDS in blocks
// of 64 rows, in ascending order.
//   forward    : one workgroup per (sample, head, query block).  Per key block S = Q_b K_j^T (4 tiles, one per wave) -> online softmax
//                in the LDS strip (running row max m and row sum l; P = exp(s - m_new)) -> O = O * exp(m_old - m_new) + P V_j (one
//                accumulator tile per wave, in registers across the whole walk).  At the end O / l and lse = m + log l.
//   backward kv: one workgroup per (sample, head, key block), walks the query blocks: dV_j += P^T dO_i, dK_j += dS^T Q_i.
//   backward q : one workgroup per (sample, head, query block), walks the key blocks: dQ_i += dS K_j.
//                Both recompute P = exp(s scale - lse) and dS = P (dO V^T - delta) scale, delta_i = sum_c dO_ic O_ic formed in-kernel.
// Every element of d_qkv is written by exactly one workgroup, sums run in ascending block order: no atomics, no workspace, no memset, and
// two runs give the same bits.  Keys >= L of the last block have P = 0 exactly and zero K / V rows; query rows >= L are zero rows that are
// never stored.  Every product is a set of 32x32 tiles of v_mfma_f32_32x32x2_f32 (attn_tiles.h).
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

__global__ __launch_bounds__(64 * kSW) void attn_stream_fwd_kernel(const float *__restrict__ qkv, float *__restrict__ ctx,
                                                                   float *__restrict__ lse, int L, int H, int nqb, float scale) {
    extern __shared__ float sm[];
    float *Qb = sm, *Ks = Qb + kTile, *Vs = Ks + kTile, *Ss = Vs + kTile, *ms = Ss + kTile, *ls = ms + kSB, *al = ls + kSB;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lk = lane >> 5;
    const int wg = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int bh = wg / nqb, qb = wg - bh * nqb, b = bh / H, hh = bh - b * H;
    const int q0 = qb * kSB, qv = min(kSB, L - q0);
    const size_t rs = (size_t)3 * H * 64;
    const float *base = qkv + (size_t)b * L * rs + (size_t)hh * 64;
    {
        float *const dst[1] = {Qb};
        const float *const src[1] = {base + (size_t)q0 * rs};
        const size_t strides[1] = {rs};
        stage_rows<1>(dst, src, strides, qv);
    }
    if (threadIdx.x < kSB) { ms[threadIdx.x] = -__builtin_inff(); ls[threadIdx.x] = 0.0f; }
    const int it = wave & 1, jt = wave >> 1;             // S tile (it, jt) and O tile (it, channels 32 jt ...)
    f32x16 o; zero(o);
    for (int k0 = 0; k0 < L; k0 += kSB) {
        const int kv = min(kSB, L - k0);                 // >= 1: every key block holds a real key, so no row max stays -inf
        {
            float *const dst[2] = {Ks, Vs};
            const float *const src[2] = {base + (size_t)k0 * rs + H * 64, base + (size_t)k0 * rs + 2 * H * 64};
            const size_t strides[2] = {rs, rs};
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
            for (int q = 0; q < 4; ++q) s[q] = lane < kv ? Ss[(i0 + q) * kLD + lane] : -__builtin_inff();
#pragma unroll
            for (int q = 0; q < 4; ++q) { mo[q] = ms[i0 + q]; mn[q] = fmaxf(mo[q], wave_max_f32(s[q])); }
#pragma unroll
            for (int q = 0; q < 4; ++q) p[q] = lane < kv ? exp_neg(s[q] - mn[q]) : 0.0f;       // keys >= L contribute exactly nothing
#pragma unroll
            for (int q = 0; q < 4; ++q) sum[q] = wave_sum_f32(p[q]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                Ss[(i0 + q) * kLD + lane] = p[q];
                if (lane == 0) {
                    const float a = exp_neg(mo[q] - mn[q]);                  // first block: exp(-inf) = 0 against l = 0 and O = 0
                    ms[i0 + q] = mn[q];
                    ls[i0 + q] = ls[i0 + q] * a + sum[q];
                    al[i0 + q] = a;
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
        if (i < qv) ctx[((size_t)b * L + q0 + i) * (H * 64) + hh * 64 + jt * 32 + lr] = o[r] / ls[i];
    }
    if ((int)threadIdx.x < qv) lse[((size_t)b * H + hh) * L + q0 + threadIdx.x] = ms[threadIdx.x] + logf(ls[threadIdx.x]);
}

// delta_i = dO_i . O_i and lse_i of the `valid` rows behind g / o / l (rows >= valid: 0) -- 16 rows per wave, four per iteration, lane = channel
__device__ __forceinline__ void stream_row_stats(const float *__restrict__ g, const float *__restrict__ o, const float *__restrict__ l,
                                                 size_t cs, int valid, float *delta, float *lses, int wave, int lane) {
    for (int i0 = wave * (kSB / kSW); i0 < (wave + 1) * (kSB / kSW); i0 += 4) {
        float gv[4], ov[4], lv[4], d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool ok = i0 + q < valid;
            gv[q] = ok ? g[(size_t)(i0 + q) * cs + lane] : 0.0f;
            ov[q] = ok ? o[(size_t)(i0 + q) * cs + lane] : 0.0f;
            lv[q] = (ok && lane == 0) ? l[i0 + q] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = wave_sum_f32(gv[q] * ov[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (lane == 0) { delta[i0 + q] = d[q]; lses[i0 + q] = lv[q]; }
    }
}

// P = exp(S scale - lse) and dS = P (dO V^T - delta) scale of one (64 query x 64 key) block into the strips Ps / Ds; entries of query
// rows >= qv and keys >= kv are zero.  Waves 0, 1 compute the two S tiles of query rows 32 it ..., waves 2, 3 the two dP tiles (two
// accumulator chains per wave); dP stays in registers until P is in the LDS.  Ends on a barrier.
__device__ __forceinline__ void stream_p_ds(const float *Qb, const float *Gb, const float *Ks, const float *Vs, float *Ps, float *Ds,
                                            const float *lses, const float *delta, int qv, int kv, float scale, int wave, int lr, int lk) {
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
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = it * 32 + tile_row(r, lk), j = n * 32 + lr;
                Ds[i * kLD + j] = (i < qv && j < kv) ? Ps[i * kLD + j] * (acc[n][r] - delta[i]) * scale : 0.0f;
            }
    }
    __syncthreads();
}

// dK and dV of one key block.  Waves 0, 1: dV rows 32 jt ... (both channel tiles), waves 2, 3: dK rows 32 jt ...; the accumulators
// stay in registers across the walk over the query blocks and are stored once.
__global__ __launch_bounds__(64 * kSW) void attn_stream_bwd_kv_kernel(const float *__restrict__ qkv, const float *__restrict__ ctx,
                                                                      const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                                                      float *__restrict__ d_qkv, int L, int H, int nkb, float scale) {
    extern __shared__ float sm[];
    float *Ks = sm, *Vs = Ks + kTile, *Qb = Vs + kTile, *Gb = Qb + kTile, *Ps = Gb + kTile, *Ds = Ps + kTile, *delta = Ds + kTile, *lses = delta + kSB;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lk = lane >> 5;
    const int wg = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int bh = wg / nkb, kb = wg - bh * nkb, b = bh / H, hh = bh - b * H;
    const int k0 = kb * kSB, kv = min(kSB, L - k0);
    const size_t rs = (size_t)3 * H * 64, cs = (size_t)H * 64;
    const float *base = qkv + (size_t)b * L * rs + (size_t)hh * 64;
    float *dbase = d_qkv + (size_t)b * L * rs + (size_t)hh * 64;
    const float *gbase = d_ctx + (size_t)b * L * cs + (size_t)hh * 64;
    const float *obase = ctx + (size_t)b * L * cs + (size_t)hh * 64;
    const float *lbase = lse + ((size_t)b * H + hh) * L;
    {
        float *const dst[2] = {Ks, Vs};
        const float *const src[2] = {base + (size_t)k0 * rs + H * 64, base + (size_t)k0 * rs + 2 * H * 64};
        const size_t strides[2] = {rs, rs};
        stage_rows<2>(dst, src, strides, kv);
    }
    const int jt = wave & 1;
    const bool dk = wave >= 2;
    f32x16 acc[2];
    zero(acc[0]); zero(acc[1]);
    for (int q0 = 0; q0 < L; q0 += kSB) {
        const int qv = min(kSB, L - q0);
        {
            float *const dst[2] = {Qb, Gb};
            const float *const src[2] = {base + (size_t)q0 * rs, gbase + (size_t)q0 * cs};
            const size_t strides[2] = {rs, cs};
            stage_rows<2>(dst, src, strides, qv);
        }
        stream_row_stats(gbase + (size_t)q0 * cs, obase + (size_t)q0 * cs, lbase + q0, cs, qv, delta, lses, wave, lane);
        __syncthreads();
        stream_p_ds(Qb, Gb, Ks, Vs, Ps, Ds, lses, delta, qv, kv, scale, wave, lr, lk);
        {   // dV += P^T dO_i (waves 0, 1), dK += dS^T Q_i (waves 2, 3): the contraction runs over the block's 64 query rows
            const float *a = (dk ? Ds : Ps) + jt * 32, *bsrc = dk ? Qb : Gb;
            const float *const bt[2] = {bsrc, bsrc + 32};
            mfma_tiles_k<true, false, 64, 2>(acc, a, kLD, bt, kLD, lr, lk);
        }
        __syncthreads();
    }
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jt * 32 + tile_row(r, lk);
            if (j < kv) dbase[(size_t)(k0 + j) * rs + (dk ? 1 : 2) * H * 64 + n * 32 + lr] = acc[n][r];
        }
}

// dQ of one query block.  Wave (it, kh) accumulates dQ rows 32 it ... (both channel tiles) over keys 32 kh ... 32 kh + 31 of every key
// block; the two halves are added once at the end (kh = 0 first), through the LDS.
__global__ __launch_bounds__(64 * kSW) void attn_stream_bwd_q_kernel(const float *__restrict__ qkv, const float *__restrict__ ctx,
                                                                     const float *__restrict__ d_ctx, const float *__restrict__ lse,
                                                                     float *__restrict__ d_qkv, int L, int H, int nqb, float scale) {
    extern __shared__ float sm[];
    float *Ks = sm, *Vs = Ks + kTile, *Qb = Vs + kTile, *Gb = Qb + kTile, *Ps = Gb + kTile, *Ds = Ps + kTile, *delta = Ds + kTile, *lses = delta + kSB;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lk = lane >> 5;
    const int wg = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int bh = wg / nqb, qb = wg - bh * nqb, b = bh / H, hh = bh - b * H;
    const int q0 = qb * kSB, qv = min(kSB, L - q0);
    const size_t rs = (size_t)3 * H * 64, cs = (size_t)H * 64;
    const float *base = qkv + (size_t)b * L * rs + (size_t)hh * 64;
    float *dbase = d_qkv + (size_t)b * L * rs + (size_t)hh * 64;
    const float *gbase = d_ctx + (size_t)b * L * cs + (size_t)hh * 64;
    const float *obase = ctx + (size_t)b * L * cs + (size_t)hh * 64;
    {
        float *const dst[2] = {Qb, Gb};
        const float *const src[2] = {base + (size_t)q0 * rs, gbase + (size_t)q0 * cs};
        const size_t strides[2] = {rs, cs};
        stage_rows<2>(dst, src, strides, qv);
    }
    stream_row_stats(gbase + (size_t)q0 * cs, obase + (size_t)q0 * cs, lse + ((size_t)b * H + hh) * L + q0, cs, qv, delta, lses, wave, lane);
    const int it = wave & 1, kh = wave >> 1;
    f32x16 acc[2];
    zero(acc[0]); zero(acc[1]);
    for (int k0 = 0; k0 < L; k0 += kSB) {
        const int kv = min(kSB, L - k0);
        {
            float *const dst[2] = {Ks, Vs};
            const float *const src[2] = {base + (size_t)k0 * rs + H * 64, base + (size_t)k0 * rs + 2 * H * 64};
            const size_t strides[2] = {rs, rs};
            stage_rows<2>(dst, src, strides, kv);
        }
        __syncthreads();
        stream_p_ds(Qb, Gb, Ks, Vs, Ps, Ds, lses, delta, qv, kv, scale, wave, lr, lk);
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
                if (i < qv) dbase[(size_t)(q0 + i) * rs + n * 32 + lr] = acc[n][r] + Ps[i * kLD + n * 32 + lr];
            }
    }
}

constexpr size_t kFwdStreamLds = ((size_t)4 * kTile + 3 * kSB) * sizeof(float);     // 66 KB: two workgroups per CU
constexpr size_t kBwdStreamLds = ((size_t)6 * kTile + 2 * kSB) * sizeof(float);     // 98 KB: one workgroup per CU
static_assert(2 * kFwdStreamLds <= 160 * 1024 && kBwdStreamLds <= 160 * 1024, "LDS budget");

}  // namespace

// called by upp_attn_fwd / upp_attn_bwd (block.hip) for 160 < L <= UPP_ATTN_MAX_L
int upp_attn_fwd_stream(const float *qkv, float *ctx, float *lse, int B, int L, int H, float scale, hipStream_t st) {
    static std::atomic<bool> raised{false};
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(attn_stream_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFwdStreamLds);
        if (e != hipSuccess) return (int)e;
        raised = true;
    }
    const int nqb = (L + kSB - 1) / kSB;
    hipLaunchKernelGGL(attn_stream_fwd_kernel, dim3(B * H * nqb), dim3(64 * kSW), kFwdStreamLds, st, qkv, ctx, lse, L, H, nqb, scale);
    return upp_launch_status();
}

int upp_attn_bwd_stream(const float *qkv, const float *ctx, const float *d_ctx, const float *lse, float *d_qkv, int B, int L, int H,
                        float scale, hipStream_t st) {
    static std::atomic<bool> raised{false};
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(attn_stream_bwd_kv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBwdStreamLds);
        if (e != hipSuccess) return (int)e;
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(attn_stream_bwd_q_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBwdStreamLds);
        if (e != hipSuccess) return (int)e;
        raised = true;
    }
    const int nb = (L + kSB - 1) / kSB;
    hipLaunchKernelGGL(attn_stream_bwd_kv_kernel, dim3(B * H * nb), dim3(64 * kSW), kBwdStreamLds, st, qkv, ctx, d_ctx, lse, d_qkv, L, H, nb, scale);
    int rc = upp_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(attn_stream_bwd_q_kernel, dim3(B * H * nb), dim3(64 * kSW), kBwdStreamLds, st, qkv, ctx, d_ctx, lse, d_qkv, L, H, nb, scale);
    return upp_launch_status();
}
