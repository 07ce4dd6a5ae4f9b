// edge_conv.hip -- the edge convolution of a DGCNN layer as a gather-normalise-max over a neighbour list, for gfx950
// (include/upp_hip.h "edge convolution"; reference models/dgcnn_group.py:91-144, models/Transformer.py:176-213).
//
// The 1x1 conv of [f_j - f_i ; f_i] is W1 f_j + (W2 - W1) f_i: two per-POINT products A (B,Nk,O) and Bq (B,Nq,O) that the caller makes
// with its Linear kernels.  What is left is  y[b,q,k,o] = A[b, idx[b,q,k], o] + Bq[b,q,o],  GroupNorm over (O / G channels, Nq, K),
// LeakyReLU and the max over k -- here without ever storing y:
//   forward   ec_stats_kernel (per-wavefront (sum, M2) partials of y) -> ec_finalize_kernel (Chan's combination in f64, fixed order)
//             -> ec_apply_kernel (the extreme y per channel, one z, LeakyReLU);                     no norm: ec_apply_kernel alone
//   backward  ec_bwd_reduce_kernel (per-wavefront sums of g_z and g_z xhat) -> ec_bwd_group_kernel (m1, m2) + ec_bwd_param_kernel
//             (g_gamma, g_beta) -> ec_bwd_apply_kernel (g_y per (q, k): g_Bq, and g_A by f32 atomics or -- deterministic -- stored
//             for upp_knn_scatter_add_det);                                                         no norm: ec_bwd_apply_kernel alone
// Mapping: a wavefront owns query rows, lane = channel (O > 64: chunks of 64 channels in turn).  The K neighbour indices of a row are
// loaded once by lanes 0 ... K-1 and reach the gathers through v_readlane, so every gather address is wave-uniform base + lane; the
// gathers of up to 16 neighbour rows are issued before the arithmetic that consumes them (as prop_pool_fwd_kernel).  No per-lane array
// is indexed at run time.  Sums that cross wavefronts go through partials in the caller's workspace and are added in a fixed order: no
// atomics except the g_A scatter, nothing is memset.
#include "common.h"

namespace {

constexpr int kEcWaves = 4;        // wavefronts per workgroup
constexpr int kEcRows = 8;         // query rows of one statistics slab (one wavefront)
constexpr int kEcBatch = 16;       // neighbour rows gathered before the arithmetic
constexpr int kEcMaxK = 64, kEcMaxO = 512;
constexpr int kEcParamWaves = 16;

__host__ __device__ static inline int ec_slabs(int Nq) { return (Nq + kEcRows - 1) / kEcRows; }

// neighbour index of lane `lane` (k = lane) of query row `row`, clamped into [0, Nk): an index outside is a caller's error, not a fault
__device__ __forceinline__ uint32_t ec_index(const int64_t *__restrict__ idx, size_t row, int K, int Nk, int lane) {
    const int64_t j = lane < K ? idx[row * K + lane] : 0;
    return (uint32_t)(j < 0 ? 0 : (j >= (int64_t)Nk ? Nk - 1 : j));
}

__device__ __forceinline__ float ec_lrelu_grad(float z, float slope) { return z > 0.0f ? 1.0f : slope; }

// sum of one double per thread over a 256-thread workgroup, the same tree every time
__device__ __forceinline__ double ec_block_sum(double v, double *sh, int tid) {
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}

// part[((b * slabs + slab) * 2 + 0) * O + c] = sum of y over the slab's rows and their K neighbours, [.. + 1 ..] = M2 about the slab's
// mean; from sums shifted by the slab's first value (no cancellation when |mean| >> std), as bn_rows_partial_kernel.
__global__ __launch_bounds__(64 * kEcWaves) void ec_stats_kernel(const float *__restrict__ A, const float *__restrict__ Bq,
                                                                 const int64_t *__restrict__ idx, float *__restrict__ part, int Nk, int Nq,
                                                                 int K, int O, int slabs) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, slab = blockIdx.x * kEcWaves + wave;
    if (slab >= slabs) return;
    const int q0 = slab * kEcRows, q1 = min(Nq, q0 + kEcRows);
    const float *Ab = A + (size_t)b * Nk * O;
    for (int c0 = 0; c0 < O; c0 += 64) {
        const int c = min(c0 + lane, O - 1);               // clamped: no branch around the loads
        float shift = 0.0f, a1 = 0.0f, a2 = 0.0f;
        for (int q = q0; q < q1; ++q) {
            const size_t row = (size_t)b * Nq + q;
            const uint32_t jv = ec_index(idx, row, K, Nk, lane);
            const float bq = Bq[row * O + c];
            for (int k0 = 0; k0 < K; k0 += kEcBatch) {
                float v[kEcBatch];
#pragma unroll
                for (int t = 0; t < kEcBatch; ++t) v[t] = Ab[(size_t)readlane_u32(jv, min(k0 + t, K - 1)) * O + c];
#pragma unroll
                for (int t = 0; t < kEcBatch; ++t) {
                    if (k0 + t < K) {                      // (uniform)
                        const float y = v[t] + bq;
                        if (q == q0 && k0 + t == 0) shift = y;
                        const float d = y - shift;
                        a1 += d;
                        a2 = __builtin_fmaf(d, d, a2);
                    }
                }
            }
        }
        if (c0 + lane < O) {
            const float n = (float)((q1 - q0) * K);
            float *p = part + ((size_t)b * slabs + slab) * 2 * O;
            p[c] = __builtin_fmaf(shift, n, a1);
            p[O + c] = a2 - a1 * a1 / n;
        }
    }
}

// mean / rstd of one (sample, group) from the slab partials of its O / G channels: two passes in f64,
//   mean = sum_i S_i / N;   M2 = sum_i [ M2_i + n_i (S_i / n_i - mean)^2 ]          (bn_finalize_rows_kernel's combination)
__global__ __launch_bounds__(256) void ec_finalize_kernel(const float *__restrict__ part, float *__restrict__ mean, float *__restrict__ rstd,
                                                          int slabs, int Nq, int K, int O, int G, float eps) {
    __shared__ double sh[256];
    const int tid = threadIdx.x, b = blockIdx.x / G, g = blockIdx.x - b * G, cpg = O / G;
    const float *pb = part + (size_t)b * slabs * 2 * O;
    const int items = slabs * cpg;
    double s = 0.0;
    for (int i = tid; i < items; i += 256) {
        const int sl = i / cpg, ch = g * cpg + (i - sl * cpg);
        s += (double)pb[(size_t)sl * 2 * O + ch];
    }
    const double N = (double)cpg * (double)Nq * (double)K;
    const double mu = ec_block_sum(s, sh, tid) / N;
    double q = 0.0;
    for (int i = tid; i < items; i += 256) {
        const int sl = i / cpg, ch = g * cpg + (i - sl * cpg);
        const double nb = (double)((min(Nq, (sl + 1) * kEcRows) - sl * kEcRows) * K);
        const double d = (double)pb[(size_t)sl * 2 * O + ch] / nb - mu;
        q += (double)pb[(size_t)sl * 2 * O + O + ch] + nb * d * d;
    }
    const double m2 = ec_block_sum(q, sh, tid);
    if (tid == 0) {
        const float var = (float)(m2 / N);
        mean[blockIdx.x] = (float)mu;
        rstd[blockIdx.x] = 1.0f / sqrtf((var > 0.0f ? var : 0.0f) + eps);
    }
}

// out[b,q,o] = lrelu(z at the extreme y), arg[b,q,o] by the rule of include/upp_hip.h.  z and lrelu are monotone in y per channel (every
// rounded step is), so the maximum over k of lrelu(z) IS lrelu(z(max y)) for gamma rstd > 0 and lrelu(z(min y)) for < 0.
template <bool NORM>
__global__ __launch_bounds__(64 * kEcWaves) void ec_apply_kernel(const float *__restrict__ A, const float *__restrict__ Bq,
                                                                 const int64_t *__restrict__ idx, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, const float *__restrict__ mean,
                                                                 const float *__restrict__ rstd, float slope, float *__restrict__ out,
                                                                 uint8_t *__restrict__ arg, int Nk, int Nq, int K, int O, int G) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, q = blockIdx.x * kEcWaves + wave;
    if (q >= Nq) return;
    const float *Ab = A + (size_t)b * Nk * O;
    const size_t row = (size_t)b * Nq + q;
    const uint32_t jv = ec_index(idx, row, K, Nk, lane);
    const int cpg = NORM ? O / G : 1;
    for (int c0 = 0; c0 < O; c0 += 64) {
        const int c = min(c0 + lane, O - 1);
        const float bq = Bq[row * O + c];
        float mx = -__builtin_inff(), mn = __builtin_inff(), y0 = 0.0f;
        int amx = 0, amn = 0;
        for (int k0 = 0; k0 < K; k0 += kEcBatch) {
            float v[kEcBatch];
#pragma unroll
            for (int t = 0; t < kEcBatch; ++t) v[t] = Ab[(size_t)readlane_u32(jv, min(k0 + t, K - 1)) * O + c];
#pragma unroll
            for (int t = 0; t < kEcBatch; ++t) {
                if (k0 + t < K) {
                    const float y = v[t] + bq;
                    if (k0 + t == 0) y0 = y;
                    if (y > mx) { mx = y; amx = k0 + t; }          // the first extreme wins: lowest k
                    if (y < mn) { mn = y; amn = k0 + t; }
                }
            }
        }
        float z = mx;
        int a = amx;
        if (NORM) {
            const int bg = b * G + c / cpg;
            const float mu = mean[bg], rs = rstd[bg], ga = gamma[c], be = beta[c];
            const float s = ga * rs;
            const float ysel = s > 0.0f ? mx : (s < 0.0f ? mn : y0);
            a = s > 0.0f ? amx : (s < 0.0f ? amn : 0);
            z = ((ysel - mu) * rs) * ga + be;
        }
        if (c0 + lane < O) {
            out[row * O + c] = z > 0.0f ? z : z * slope;
            arg[row * O + c] = (uint8_t)a;
        }
    }
}

// per slab and channel: part[.. 0 ..] = sum_q g_z, part[.. 1 ..] = sum_q g_z xhat, over the slab's rows in ascending q (g_z lives at
// k = arg only).  The eight rows' arg, index and A loads are issued as three rounds of independent loads.
__global__ __launch_bounds__(64 * kEcWaves) void ec_bwd_reduce_kernel(const float *__restrict__ g_out, const float *__restrict__ A,
                                                                      const float *__restrict__ Bq, const int64_t *__restrict__ idx,
                                                                      const uint8_t *__restrict__ arg, const float *__restrict__ gamma,
                                                                      const float *__restrict__ beta, const float *__restrict__ mean,
                                                                      const float *__restrict__ rstd, float slope, float *__restrict__ part,
                                                                      int Nk, int Nq, int K, int O, int G, int slabs) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, slab = blockIdx.x * kEcWaves + wave;
    if (slab >= slabs) return;
    const int q0 = slab * kEcRows, q1 = min(Nq, q0 + kEcRows), cpg = O / G;
    const float *Ab = A + (size_t)b * Nk * O;
    for (int c0 = 0; c0 < O; c0 += 64) {
        const int c = min(c0 + lane, O - 1);
        const int bg = b * G + c / cpg;
        const float mu = mean[bg], rs = rstd[bg], ga = gamma[c], be = beta[c];
        int a[kEcRows];
        float go[kEcRows], bq[kEcRows], av[kEcRows];
        int64_t j[kEcRows];
#pragma unroll
        for (int r = 0; r < kEcRows; ++r) {
            const size_t e = ((size_t)b * Nq + min(q0 + r, q1 - 1)) * O + c;
            a[r] = min((int)arg[e], K - 1);
            go[r] = g_out[e];
            bq[r] = Bq[e];
        }
#pragma unroll
        for (int r = 0; r < kEcRows; ++r) j[r] = idx[((size_t)b * Nq + min(q0 + r, q1 - 1)) * K + a[r]];
#pragma unroll
        for (int r = 0; r < kEcRows; ++r) {
            const int64_t jj = j[r] < 0 ? 0 : (j[r] >= (int64_t)Nk ? Nk - 1 : j[r]);
            av[r] = Ab[(size_t)jj * O + c];
        }
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int r = 0; r < kEcRows; ++r) {
            if (q0 + r < q1) {
                const float xh = ((av[r] + bq[r]) - mu) * rs;
                const float gz = go[r] * ec_lrelu_grad(xh * ga + be, slope);
                s0 += gz;
                s1 += gz * xh;
            }
        }
        if (c0 + lane < O) {
            float *p = part + ((size_t)b * slabs + slab) * 2 * O;
            p[c] = s0;
            p[O + c] = s1;
        }
    }
}

// ms[(b * G + g) * 2 + 0] = m1 = mean(gamma g_z), [.. + 1] = m2 = mean(gamma g_z xhat) over the group's O / G x Nq x K values
__global__ __launch_bounds__(256) void ec_bwd_group_kernel(const float *__restrict__ part, const float *__restrict__ gamma,
                                                           float *__restrict__ ms, int slabs, int Nq, int K, int O, int G) {
    __shared__ double sh[256];
    const int tid = threadIdx.x, b = blockIdx.x / G, g = blockIdx.x - b * G, cpg = O / G;
    const float *pb = part + (size_t)b * slabs * 2 * O;
    const int items = slabs * cpg;
    double s0 = 0.0, s1 = 0.0;
    for (int i = tid; i < items; i += 256) {
        const int sl = i / cpg, ch = g * cpg + (i - sl * cpg);
        const double ga = (double)gamma[ch];
        s0 += ga * (double)pb[(size_t)sl * 2 * O + ch];
        s1 += ga * (double)pb[(size_t)sl * 2 * O + O + ch];
    }
    const double N = (double)cpg * (double)Nq * (double)K;
    const double t0 = ec_block_sum(s0, sh, tid);
    const double t1 = ec_block_sum(s1, sh, tid);
    if (tid == 0) {
        ms[(size_t)blockIdx.x * 2 + 0] = (float)(t0 / N);
        ms[(size_t)blockIdx.x * 2 + 1] = (float)(t1 / N);
    }
}

// g_beta[o] = sum over (b, slab) of part[.. 0 ..], g_gamma[o] of part[.. 1 ..]: lane = channel, wave w owns items w, w + 16, ... (f64,
// eight loads in flight), the 16 waves combined in wave order
__global__ __launch_bounds__(64 * kEcParamWaves) void ec_bwd_param_kernel(const float *__restrict__ part, float *__restrict__ g_gamma,
                                                                          float *__restrict__ g_beta, int items, int O) {
    __shared__ double sh[2][kEcParamWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, cc = min(c, O - 1);
    double s0 = 0.0, s1 = 0.0;
    for (int i0 = wave; i0 < items; i0 += kEcParamWaves * 8) {
        float p0[8], p1[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int i = min(i0 + kEcParamWaves * t, items - 1);
            p0[t] = part[(size_t)i * 2 * O + cc];
            p1[t] = part[(size_t)i * 2 * O + O + cc];
        }
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (i0 + kEcParamWaves * t < items) { s0 += (double)p0[t]; s1 += (double)p1[t]; }
    }
    sh[0][wave][lane] = s0;
    sh[1][wave][lane] = s1;
    __syncthreads();
    if (wave == 0 && c < O) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int w = 0; w < kEcParamWaves; ++w) { t0 += sh[0][w][lane]; t1 += sh[1][w][lane]; }
        g_beta[c] = (float)t0;
        g_gamma[c] = (float)t1;
    }
}

// g_y[b,q,k,o] = rstd (gamma g_z - m1 - xhat m2)  (no norm: g_z), g_Bq[b,q,o] = sum_k g_y in ascending k, and g_A[b, idx[b,q,k], o] += g_y
// by f32 atomics (one wave-instruction adds O contiguous floats of one row) -- or, gy != NULL, g_y is stored for the ordered scatter.
template <bool NORM>
__global__ __launch_bounds__(64 * kEcWaves) void ec_bwd_apply_kernel(const float *__restrict__ g_out, const float *__restrict__ A,
                                                                     const float *__restrict__ Bq, const int64_t *__restrict__ idx,
                                                                     const uint8_t *__restrict__ arg, const float *__restrict__ gamma,
                                                                     const float *__restrict__ beta, const float *__restrict__ mean,
                                                                     const float *__restrict__ rstd, const float *__restrict__ ms, float slope,
                                                                     float *__restrict__ g_A, float *__restrict__ g_Bq, float *__restrict__ gy,
                                                                     int Nk, int Nq, int K, int O, int G) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, q = blockIdx.x * kEcWaves + wave;
    if (q >= Nq) return;
    const float *Ab = A + (size_t)b * Nk * O;
    float *gAb = g_A + (size_t)b * Nk * O;
    const size_t row = (size_t)b * Nq + q;
    const uint32_t jv = ec_index(idx, row, K, Nk, lane);
    const int cpg = NORM ? O / G : 1;
    for (int c0 = 0; c0 < O; c0 += 64) {
        const int c = min(c0 + lane, O - 1);
        const bool live = c0 + lane < O;
        const float bq = Bq[row * O + c], go = g_out[row * O + c];
        const int a = arg[row * O + c];
        float mu = 0.0f, rs = 1.0f, ga = 1.0f, be = 0.0f, m1 = 0.0f, m2 = 0.0f;
        if (NORM) {
            const int bg = b * G + c / cpg;
            mu = mean[bg]; rs = rstd[bg]; ga = gamma[c]; be = beta[c];
            m1 = ms[(size_t)bg * 2]; m2 = ms[(size_t)bg * 2 + 1];
        }
        float acc = 0.0f;
        for (int k0 = 0; k0 < K; k0 += kEcBatch) {
            float v[kEcBatch];
#pragma unroll
            for (int t = 0; t < kEcBatch; ++t) v[t] = Ab[(size_t)readlane_u32(jv, min(k0 + t, K - 1)) * O + c];
#pragma unroll
            for (int t = 0; t < kEcBatch; ++t) {
                if (k0 + t < K) {
                    const int k = k0 + t;
                    const float y = v[t] + bq;
                    float g;
                    if (NORM) {
                        const float xh = (y - mu) * rs;
                        const float gz = k == a ? go * ec_lrelu_grad(xh * ga + be, slope) : 0.0f;
                        g = rs * ((ga * gz - m1) - xh * m2);
                    } else {
                        g = k == a ? go * ec_lrelu_grad(y, slope) : 0.0f;
                    }
                    acc += g;
                    if (live) {
                        if (gy) gy[(row * K + k) * O + c] = g;
                        else if (NORM || k == a) atomicAdd(&gAb[(size_t)readlane_u32(jv, k) * O + c], g);
                    }
                }
            }
        }
        if (live) g_Bq[row * O + c] = acc;
    }
}

static int ec_args(const void *A, const void *Bq, const void *idx, const void *gamma, const void *beta, const void *mean, const void *rstd,
                   const void *work, float slope, int G, int B, int Nk, int Nq, int K, int O) {
    if (!A || !Bq || !idx || B < 0 || Nk < 1 || Nq < 1 || K < 1 || O < 1 || G < 0 || !(slope >= 0.0f && slope <= 1.0f)) return UPP_E_BADARG;
    if (G > 0 && (!gamma || !beta || !mean || !rstd || !work)) return UPP_E_BADARG;
    if (K > kEcMaxK || O > kEcMaxO || (G > 0 && O % G != 0) || B > 65535) return UPP_E_RANGE;
    if (Nq > 0x3FFFFFFF || (long long)Nq * K > 0x7FFFFFFFLL || (long long)Nk * O > 0x7FFFFFFFLL || (long long)Nq * O > 0x7FFFFFFFLL) return UPP_E_RANGE;
    return 0;
}

}  // namespace

extern "C" long long upp_edge_conv_work_floats(int B, int Nq, int O) {
    if (B < 0 || Nq < 1 || O < 1) return 0;
    return (long long)B * ec_slabs(Nq) * 2 * O + 2LL * B * O;
}

extern "C" int upp_edge_conv_fwd(const float *A, const float *Bq, const int64_t *idx, const float *gamma, const float *beta, float eps,
                                 float slope, int G, float *out, uint8_t *arg, float *mean, float *rstd, float *work, int B, int Nk, int Nq,
                                 int K, int O, void *stream) {
    if (!out || !arg || !(eps >= 0.0f)) return UPP_E_BADARG;
    const int rc = ec_args(A, Bq, idx, gamma, beta, mean, rstd, work, slope, G, B, Nk, Nq, K, O);
    if (rc) return rc;
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 rows_grid((Nq + kEcWaves - 1) / kEcWaves, B), block(64 * kEcWaves);
    if (G > 0) {
        const int slabs = ec_slabs(Nq);
        hipLaunchKernelGGL(ec_stats_kernel, dim3((slabs + kEcWaves - 1) / kEcWaves, B), block, 0, st, A, Bq, idx, work, Nk, Nq, K, O, slabs);
        hipLaunchKernelGGL(ec_finalize_kernel, dim3(B * G), dim3(256), 0, st, work, mean, rstd, slabs, Nq, K, O, G, eps);
        hipLaunchKernelGGL((ec_apply_kernel<true>), rows_grid, block, 0, st, A, Bq, idx, gamma, beta, mean, rstd, slope, out, arg, Nk, Nq, K,
                           O, G);
    } else {
        hipLaunchKernelGGL((ec_apply_kernel<false>), rows_grid, block, 0, st, A, Bq, idx, gamma, beta, mean, rstd, slope, out, arg, Nk, Nq, K,
                           O, 1);
    }
    return upp_launch_status();
}

extern "C" int upp_edge_conv_bwd(const float *g_out, const float *A, const float *Bq, const int64_t *idx, const uint8_t *arg,
                                 const float *gamma, const float *beta, const float *mean, const float *rstd, float slope, int G, float *g_A,
                                 float *g_Bq, float *g_gamma, float *g_beta, float *work, float *g_y, int B, int Nk, int Nq, int K, int O,
                                 void *stream) {
    if (!g_out || !arg || !g_A || !g_Bq || (G > 0 && (!g_gamma || !g_beta))) return UPP_E_BADARG;
    const int rc = ec_args(A, Bq, idx, gamma, beta, mean, rstd, work, slope, G, B, Nk, Nq, K, O);
    if (rc) return rc;
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 rows_grid((Nq + kEcWaves - 1) / kEcWaves, B), block(64 * kEcWaves);
    if (!g_y) upp_zero_async(g_A, (long long)B * Nk * O, st);
    if (G > 0) {
        const int slabs = ec_slabs(Nq);
        float *ms = work + (size_t)B * slabs * 2 * O;
        hipLaunchKernelGGL(ec_bwd_reduce_kernel, dim3((slabs + kEcWaves - 1) / kEcWaves, B), block, 0, st, g_out, A, Bq, idx, arg, gamma, beta,
                           mean, rstd, slope, work, Nk, Nq, K, O, G, slabs);
        hipLaunchKernelGGL(ec_bwd_group_kernel, dim3(B * G), dim3(256), 0, st, work, gamma, ms, slabs, Nq, K, O, G);
        hipLaunchKernelGGL(ec_bwd_param_kernel, dim3((O + 63) / 64), dim3(64 * kEcParamWaves), 0, st, work, g_gamma, g_beta, B * slabs, O);
        hipLaunchKernelGGL((ec_bwd_apply_kernel<true>), rows_grid, block, 0, st, g_out, A, Bq, idx, arg, gamma, beta, mean, rstd, ms, slope,
                           g_A, g_Bq, g_y, Nk, Nq, K, O, G);
    } else {
        hipLaunchKernelGGL((ec_bwd_apply_kernel<false>), rows_grid, block, 0, st, g_out, A, Bq, idx, arg, gamma, beta, mean, rstd,
                           (const float *)nullptr, slope, g_A, g_Bq, g_y, Nk, Nq, K, O, 1);
    }
    const int launched = upp_launch_status();
    if (launched || !g_y) return launched;
    return upp_knn_scatter_add_det(g_y, idx, nullptr, nullptr, g_A, B, Nk, Nq, K, O, 0, stream);
}
