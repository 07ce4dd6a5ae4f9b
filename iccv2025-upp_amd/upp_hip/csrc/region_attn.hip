// region_attn.hip -- the region-wise deformable attention of AdaPoinTr for gfx950 (include/upp_hip.h "region-wise deformable
// attention"; reference models/Transformer_utils.py:159-266, block token `rw_deform`).  Every token gathers its k neighbours' query rows
// and runs a k x k softmax attention per head against k interpolated key / value rows, then keeps the per-channel maximum over the k
// context rows.  What is left after the per-point products is gather-bound and has no GEMM in it:
//   ra_fwd_kernel   Q_t, key_s staged in the LDS (lane = channel), the k^2 scores by lane = (t, s) pair, the row softmax by lane = t,
//                   ctx_t[ch] by lane = channel with the value rows in one register (never stored) and p read back as LDS broadcasts
//   ra_bwd_kernel   the same staging plus the value rows; p recomputed by the forward's statement (it is never stored: a saved
//                   (B,N,H,k,k) array would be k / 64 of a (B,N,k,C) tensor, the largest thing the node kept); dp and ds through the
//                   LDS; d_Q_t, d_key_s, d_val_s by lane = channel; <true> adds them to d_q / d_PK / d_PV by f32 atomics, <false> stores them to the caller's rows workspace for
//                   upp_knn_scatter_add_det (d_q) and RegionJob, a job of det_scan.h's det_scatter_kernel (d_PK, d_PV)
// Mapping that was chosen: ONE WAVE PER WORKGROUP, one item (b, n, head) at a time, grid-stride.  A k x k score matrix is k^2 dot
// products of 64 channels: as wave sums (the sibling's way) that is 1,024 DPP trees at k = 32, so the rows go through the LDS once
// (row stride 68 floats: 16-byte aligned for ds_read_b128, and 16 lanes on 16 different rows touch all 64 banks) and each lane owns
// ceil(k^2 / 64) pairs.  A one-wave workgroup makes __syncthreads() a wave-local fence, so items need not march in step across waves.
// The DPP-wave-sum variant was not built and the two were not timed against each other.
// Resources (hipcc -O3 --offload-arch=gfx950, the tree's flags, -Rpass-analysis=kernel-resource-usage): see the figures beside each
// kernel; neither uses private (scratch) memory.  Dynamic LDS: forward (2 k 68 + k (k + 1)) floats = 21,632 bytes at k = 32, 4,640 at
// k = 8; backward (3 k 68 + 2 k (k + 1) + 128) floats = 35,072 bytes at k = 32, 7,616 at k = 8.  Per-lane arrays (ctx_t, d_Q_t) are
// indexed by fully unrolled, guarded loops only.
#include "deform_row.h"

namespace {

constexpr int kRaRow = 68;            // LDS row stride of a 64-channel row, floats
constexpr long long kRaGridCap = 262144;

__host__ __device__ constexpr int ra_fwd_lds(int k) { return 2 * k * kRaRow + k * (k + 1); }
__host__ __device__ constexpr int ra_bwd_lds(int k) { return 3 * k * kRaRow + 2 * k * (k + 1) + 128; }

// fma(a[c], b[c], .) from +0 over the 64 channels in ascending c; a and b are 16-byte aligned LDS rows
__device__ __forceinline__ float ra_dot64(const float *a, const float *b) {
    float d = 0.0f;
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
        const float4 x = *reinterpret_cast<const float4 *>(a + c), y = *reinterpret_cast<const float4 *>(b + c);
        d = __builtin_fmaf(x.x, y.x, d);
        d = __builtin_fmaf(x.y, y.y, d);
        d = __builtin_fmaf(x.z, y.z, d);
        d = __builtin_fmaf(x.w, y.w, d);
    }
    return d;
}

// Q_t = q[b, idx[b,n,t]] (a zero row for an index outside [0, N)), key_t and -- V != NULL -- val_t of item (b, n, head) into the LDS;
// lane = channel, every global row read one coalesced 256-byte segment
__device__ __forceinline__ void ra_stage(float *Q, float *K, float *V, const float *__restrict__ q, const long long *__restrict__ idx,
                                         const float *__restrict__ PK, const float *__restrict__ PV, float kb, float vb,
                                         const int32_t *__restrict__ idx3, const float *__restrict__ w3, long long b, int n, int G, int N,
                                         int NK, int k, int C, int ch, int lane) {
    for (int t = 0; t < k; ++t) {
        const long long j = idx[(b * N + n) * k + t];
        Q[t * kRaRow + lane] = (unsigned long long)j < (unsigned long long)N ? q[(b * N + j) * C + ch] : 0.0f;
        K[t * kRaRow + lane] = da_row(PK, kb, idx3, w3, b, n, t, G, N, NK, k, C, ch);
        if (V) V[t * kRaRow + lane] = da_row(PV, vb, idx3, w3, b, n, t, G, N, NK, k, C, ch);
    }
}

// P[t][s] = softmax_s(scale * Q_t . key_s) of the staged rows: the k^2 scores by lane = (t, s) pair, then row t on lane t -- its maximum,
// expf, the sum in ascending s, one division per element.  The forward and the backward compile this one statement, so the backward's
// recomputed p has the forward's bits.  Ends with the rows visible to every lane.
__device__ __forceinline__ void ra_probs(const float *Q, const float *K, float *P, float scale, int k, int lane) {
    const int kk = k * k, ps = k + 1;
    for (int e = lane; e < kk; e += 64) {
        const int t = e / k, s = e - t * k;
        P[t * ps + s] = scale * ra_dot64(Q + t * kRaRow, K + s * kRaRow);
    }
    __syncthreads();
    if (lane < k) {
        float *row = P + lane * ps;
        float m = row[0];
        for (int s = 1; s < k; ++s) m = fmaxf(m, row[s]);
        float sum = 0.0f;
        for (int s = 0; s < k; ++s) {
            const float e = expf(row[s] - m);
            row[s] = e;
            sum += e;
        }
        for (int s = 0; s < k; ++s) row[s] = row[s] / sum;
    }
    __syncthreads();
}

// blockIdx.x = item (b, n, h), grid-stride.  109 VGPRs, 106 SGPRs, 0 bytes of scratch.
__global__ __launch_bounds__(64) void ra_fwd_kernel(const float *__restrict__ q, const long long *__restrict__ idx, const float *__restrict__ PK,
                                                    const float *__restrict__ PV, const float *__restrict__ bk, const float *__restrict__ bv,
                                                    const int32_t *__restrict__ idx3, const float *__restrict__ w3, float *__restrict__ out,
                                                    uint8_t *__restrict__ arg, float scale, int N, int NK, int k, int H, int G,
                                                    long long items) {
    extern __shared__ __attribute__((aligned(16))) float ra_lds[];
    float *Q = ra_lds, *K = Q + k * kRaRow, *P = K + k * kRaRow;
    const int lane = threadIdx.x, C = H * 64, ps = k + 1;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const auto [bn, b, n, ch] = da_item(it, N, H, lane);
        const float kb = bk ? bk[ch] : 0.0f, vb = bv ? bv[ch] : 0.0f;
        __syncthreads();                                                         // the previous item's LDS reads are done
        ra_stage(Q, K, nullptr, q, idx, PK, PV, kb, vb, idx3, w3, b, n, G, N, NK, k, C, ch, lane);
        __syncthreads();
        ra_probs(Q, K, P, scale, k, lane);
        float ctx[kDaMaxK];
#pragma unroll
        for (int t = 0; t < kDaMaxK; ++t) ctx[t] = 0.0f;
        for (int s = 0; s < k; ++s) {
            const float val = da_row(PV, vb, idx3, w3, b, n, s, G, N, NK, k, C, ch);
#pragma unroll
            for (int t = 0; t < kDaMaxK; ++t)
                if (t < k) ctx[t] = __builtin_fmaf(P[t * ps + s], val, ctx[t]);
        }
        float mx = -__builtin_inff();
        int a = 0;
#pragma unroll
        for (int t = 0; t < kDaMaxK; ++t)
            if (t < k && ctx[t] > mx) { mx = ctx[t]; a = t; }                   // the first maximum wins: lowest t; a NaN never wins
        out[bn * C + ch] = mx;
        arg[bn * C + ch] = (uint8_t)a;
    }
}

// The backward of one item.  kAtomic: d_q, d_PK, d_PV (zeroed by the entry point) take f32 atomics; otherwise the three planes of `rows`
// (3,B,N,k,C) take d_Q_t, d_key_s, d_val_s.  d_krow / d_vrow (B,N,C) or NULL = sum_s d_key_s / d_val_s in ascending s.
// 98 VGPRs (both forms), 106 SGPRs, 0 bytes of scratch.
template <bool kAtomic>
__global__ __launch_bounds__(64) void ra_bwd_kernel(const float *__restrict__ q, const long long *__restrict__ idx, const float *__restrict__ PK,
                                                    const float *__restrict__ PV, const float *__restrict__ bk, const float *__restrict__ bv,
                                                    const int32_t *__restrict__ idx3, const float *__restrict__ w3,
                                                    const uint8_t *__restrict__ arg, const float *__restrict__ d_out, float *__restrict__ d_q,
                                                    float *__restrict__ d_PK, float *__restrict__ d_PV, float *__restrict__ d_krow,
                                                    float *__restrict__ d_vrow, float *__restrict__ rows, float scale, int B, int N, int NK,
                                                    int k, int H, int G, long long items) {
    extern __shared__ __attribute__((aligned(16))) float ra_lds[];
    const int lane = threadIdx.x, C = H * 64, kk = k * k, ps = k + 1;
    float *Q = ra_lds, *K = Q + k * kRaRow, *V = K + k * kRaRow, *gL = V + k * kRaRow;
    int *aL = reinterpret_cast<int *>(gL + 64);
    float *P = gL + 128, *D = P + k * ps;
    const long long plane = (long long)B * N * k * C;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const auto [bn, b, n, ch] = da_item(it, N, H, lane);
        const float kb = bk ? bk[ch] : 0.0f, vb = bv ? bv[ch] : 0.0f;
        const float gv = d_out[bn * C + ch];
        const int a = min((int)arg[bn * C + ch], k - 1);
        __syncthreads();                                                         // the previous item's LDS reads are done
        ra_stage(Q, K, V, q, idx, PK, PV, kb, vb, idx3, w3, b, n, G, N, NK, k, C, ch, lane);
        gL[lane] = gv;
        aL[lane] = a;
        __syncthreads();
        ra_probs(Q, K, P, scale, k, lane);                                       // p again: the forward's statement on the same rows
        for (int e = lane; e < kk; e += 64) {                                   // dp[t,s] = sum over the channels whose arg is t, ascending c
            const int t = e / k, s = e - t * k;
            const float *v = V + s * kRaRow;
            float d = 0.0f;
#pragma unroll
            for (int c = 0; c < 64; c += 4) {
                const float4 x = *reinterpret_cast<const float4 *>(v + c), g4 = *reinterpret_cast<const float4 *>(gL + c);
                const int4 a4 = *reinterpret_cast<const int4 *>(aL + c);
                d = a4.x == t ? __builtin_fmaf(g4.x, x.x, d) : d;
                d = a4.y == t ? __builtin_fmaf(g4.y, x.y, d) : d;
                d = a4.z == t ? __builtin_fmaf(g4.z, x.z, d) : d;
                d = a4.w == t ? __builtin_fmaf(g4.w, x.w, d) : d;
            }
            D[t * ps + s] = d;
        }
        __syncthreads();
        if (lane < k) {                                                          // row t = lane: ds = p (dp - sum_s p dp), the sum an fma chain in ascending s
            const float *pr = P + lane * ps;
            float *dr = D + lane * ps;
            float r = 0.0f;
            for (int s = 0; s < k; ++s) r = __builtin_fmaf(pr[s], dr[s], r);
            for (int s = 0; s < k; ++s) dr[s] = pr[s] * (dr[s] - r);
        }
        __syncthreads();
        float dq[kDaMaxK], dkb = 0.0f, dvb = 0.0f;
#pragma unroll
        for (int t = 0; t < kDaMaxK; ++t) dq[t] = 0.0f;
        for (int s = 0; s < k; ++s) {
            const float key = K[s * kRaRow + lane];
#pragma unroll
            for (int t = 0; t < kDaMaxK; ++t)
                if (t < k) dq[t] = __builtin_fmaf(D[t * ps + s], key, dq[t]);
            float acc = 0.0f;
            for (int t = 0; t < k; ++t) acc = __builtin_fmaf(D[t * ps + s], Q[t * kRaRow + lane], acc);
            const float dk = __fmul_rn(scale, acc), dv = __fmul_rn(P[a * ps + s], gv);
            dkb = __fadd_rn(dkb, dk);
            dvb = __fadd_rn(dvb, dv);
            if (kAtomic) {
                da_scatter(d_PK, d_PV, dk, dv, idx3, w3, b, n, s, G, N, NK, k, C, ch);
            } else {
                rows[plane + (bn * k + s) * C + ch] = dk;
                rows[2 * plane + (bn * k + s) * C + ch] = dv;
            }
        }
#pragma unroll
        for (int t = 0; t < kDaMaxK; ++t)
            if (t < k) {
                const float v = __fmul_rn(scale, dq[t]);
                if (kAtomic) {
                    const long long j = idx[bn * k + t];
                    if ((unsigned long long)j < (unsigned long long)N) atomicAdd(d_q + (b * N + j) * C + ch, v);
                } else {
                    rows[(bn * k + t) * C + ch] = v;
                }
            }
        if (d_krow) d_krow[bn * C + ch] = dkb;
        if (d_vrow) d_vrow[bn * C + ch] = dvb;
    }
}

// d_PK[b][g][r][ch] = +0.0f, then + w3 * d_key_s for every source (n, s, j) of (b, g) with idx3 == r, in ascending (n k + s) 3 + j; d_PV
// likewise with d_val_s (include/upp_hip.h).  d_key / d_val are planes 1 and 2 of the rows workspace.  A workgroup owns 256 target
// points of one (b, g) and kDetCh channels of both arrays (NV = 2 kDetCh: the keys staged once serve both).
struct RegionJob {
    const float *__restrict__ d_key;
    const float *__restrict__ d_val;
    const int32_t *__restrict__ idx3;
    const float *__restrict__ w3;
    float *__restrict__ d_PK;
    float *__restrict__ d_PV;
    int B, G, N, NK, k, H;
    __host__ __device__ long long items() const { return (long long)B * G * det_groups(H * 64) * det_tiles(NK); }
    __device__ __forceinline__ DetItem item(long long it) const { return det_item(it, H * 64, NK, 3LL * N * k); }      // (cloud = b G + g)
    __device__ __forceinline__ void first(const DetItem &, long long, float (&)[2 * kDetCh]) const {}
    __device__ __forceinline__ void stage(const DetItem &w, long long c0, int i, int32_t &key, float *v) const {
        const long long src = c0 + i, ns = src / 3, o = (((w.b / G) * N * k) + ns) * (H * 64) + w.ch0;   // (ns = n k + s: the row of the plane)
        const int r = idx3[w.b * w.S + src];
        const float wt = w3[w.b * w.S + src];
        key = (unsigned)r < (unsigned)NK ? r : -1;
#pragma unroll
        for (int c = 0; c < kDetCh; ++c) {
            v[c] = __fmul_rn(wt, d_key[o + c]);
            v[kDetCh + c] = __fmul_rn(wt, d_val[o + c]);
        }
    }
    __device__ __forceinline__ void store(const DetItem &w, long long r, const float (&acc)[2 * kDetCh]) const {
        const long long o = (w.b * NK + r) * (H * 64) + w.ch0;
#pragma unroll
        for (int c = 0; c < kDetCh; ++c) { d_PK[o + c] = acc[c]; d_PV[o + c] = acc[kDetCh + c]; }
    }
};

// (the arrays: PK / PV, the rows workspace, idx3 / w3)
static int ra_check(int B, int N, int NK, int k, int H, int G) {
    return da_sizes(B, N, NK, k, H, G, {{B, G, NK, 64, H}, {3, B, N, k, 64, H}, {B, G, N, k, 3}});
}

static int ra_bwd(bool det, const float *q, const int64_t *idx, const float *PK, const float *PV, const float *bk, const float *bv,
                  const int32_t *idx3, const float *w3, const uint8_t *arg, const float *d_out, float *d_q, float *d_PK,
                  float *d_PV, float *d_krow, float *d_vrow, float *rows, float scale, int B, int N, int NK, int k, int H, int G,
                  void *stream) {
    if (!q || !idx || !PK || !PV || !idx3 || !w3 || !arg || !d_out || !d_q || !d_PK || !d_PV || (det && !rows) || !da_positive(scale))
        return UPP_E_BADARG;
    const int rc = ra_check(B, N, NK, k, H, G);
    if (rc) return rc;
    const long long items = (long long)B * N * H;
    const dim3 grid(grid_for(items, 1, kRaGridCap));
    const size_t lds = sizeof(float) * ra_bwd_lds(k);
    const long long *list = reinterpret_cast<const long long *>(idx);
    if (det) {
        hipLaunchKernelGGL(ra_bwd_kernel<false>, grid, dim3(64), lds, (hipStream_t)stream, q, list, PK, PV, bk, bv, idx3, w3, arg, d_out, d_q,
                           d_PK, d_PV, d_krow, d_vrow, rows, scale, B, N, NK, k, H, G, items);
        const int rq = upp_knn_scatter_add_det(rows, idx, nullptr, nullptr, d_q, B, N, N, k, 64 * H, 0, stream);
        if (rq) return rq;
        const long long plane = (long long)B * N * k * 64 * H;
        det_launch<2 * kDetCh>(RegionJob{rows + plane, rows + 2 * plane, idx3, w3, d_PK, d_PV, B, G, N, NK, k, H}, stream);
    } else {
        const long long n = (long long)B * G * NK * 64 * H;
        upp_zero_async(d_q, (long long)B * N * 64 * H, (hipStream_t)stream);
        upp_zero_async(d_PK, n, (hipStream_t)stream);
        upp_zero_async(d_PV, n, (hipStream_t)stream);
        hipLaunchKernelGGL(ra_bwd_kernel<true>, grid, dim3(64), lds, (hipStream_t)stream, q, list, PK, PV, bk, bv, idx3, w3, arg, d_out, d_q,
                           d_PK, d_PV, d_krow, d_vrow, rows, scale, B, N, NK, k, H, G, items);
    }
    return upp_launch_status();
}

}  // namespace

extern "C" int upp_region_attn_fwd(const float *q, const int64_t *idx, const float *PK, const float *PV, const float *bk, const float *bv,
                                   const int32_t *idx3, const float *w3, float *out, uint8_t *arg, float scale, int B, int N, int NK,
                                   int k, int H, int G, void *stream) {
    if (!q || !idx || !PK || !PV || !idx3 || !w3 || !out || !arg || !da_positive(scale)) return UPP_E_BADARG;
    const int rc = ra_check(B, N, NK, k, H, G);
    if (rc) return rc;
    const long long items = (long long)B * N * H;
    hipLaunchKernelGGL(ra_fwd_kernel, dim3(grid_for(items, 1, kRaGridCap)), dim3(64), sizeof(float) * ra_fwd_lds(k), (hipStream_t)stream, q,
                       reinterpret_cast<const long long *>(idx), PK, PV, bk, bv, idx3, w3, out, arg, scale, N, NK, k, H, G, items);
    return upp_launch_status();
}

extern "C" int upp_region_attn_bwd(const float *q, const int64_t *idx, const float *PK, const float *PV, const float *bk, const float *bv,
                                   const int32_t *idx3, const float *w3, const uint8_t *arg, const float *d_out,
                                   float *d_q, float *d_PK, float *d_PV, float *d_krow, float *d_vrow, float scale, int B, int N, int NK,
                                   int k, int H, int G, void *stream) {
    return ra_bwd(false, q, idx, PK, PV, bk, bv, idx3, w3, arg, d_out, d_q, d_PK, d_PV, d_krow, d_vrow, nullptr, scale, B, N, NK, k, H, G,
                  stream);
}

extern "C" int upp_region_attn_bwd_det(const float *q, const int64_t *idx, const float *PK, const float *PV, const float *bk,
                                       const float *bv, const int32_t *idx3, const float *w3, const uint8_t *arg,
                                       const float *d_out, float *d_q, float *d_PK, float *d_PV, float *d_krow, float *d_vrow, float *rows,
                                       float scale, int B, int N, int NK, int k, int H, int G, void *stream) {
    return ra_bwd(true, q, idx, PK, PV, bk, bv, idx3, w3, arg, d_out, d_q, d_PK, d_PV, d_krow, d_vrow, rows, scale, B, N, NK, k, H, G,
                  stream);
}
