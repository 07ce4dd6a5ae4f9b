// expand.hip -- a 1x1 conv over [u (J, varying) ; f (constant along an axis)] as broadcast + small-J term + BatchNorm + LeakyReLU, for gfx950
// (include/upp_hip.h "broadcast expand"; reference models/PoinTr.py:27-58 Fold.folding1[0] / folding2[0], models/Transformer.py:324-332,413-416 mlp_query[0]).
//
// With W = [Wu | Wf] the conv is (Wf f_r + b) + Wu u[r,s]: one per-ROW product P (R,O) the caller makes with its Linear kernels, and
//   y[r,s,o] = P[r,o] + sum_j U[.,s,j] Wu[o,j]        (J <= 4),
// normalised per channel over all R S values, activated and written as h (R,S,O) -- here without ever storing y, the concatenation or g_y:
//   forward   ex_stats_kernel (per row block and channel: the block's mean and M2 of y) -> ex_finalize_kernel (Chan's combination in f64,
//             fixed order) -> ex_apply_kernel (the streaming write of h);                                  no / eval norm: ex_apply_kernel alone
//   backward  ex_bwd_reduce_kernel (per row block and channel: sums of g_z and g_z xhat) -> ex_bwd_param_kernel (g_gamma, g_beta, m1, m2)
//             -> ex_bwd_apply_kernel (g_y per element: g_P, g_U, per-block partials of g_Wu) -> ex_bwd_wu_kernel (g_Wu);
//                                                                                        no norm: ex_bwd_apply_kernel + ex_bwd_wu_kernel
// Mapping, the same in every row kernel: a workgroup of 4 wavefronts owns rows; wavefront w owns the positions s = w, w + 4, ... of a
// row; a lane owns V = 4 consecutive channels (V = 1 when O is no multiple of 4 or a pointer is not 16-byte aligned), 64 V channels per
// pass, passes in turn for wider O.  So one wave-instruction loads or stores 1 KB of one (r, s) row with 16 bytes per lane, P's row and
// the Wu columns of a pass sit in registers for all of the row's positions, and U[., s, :] is a wave-uniform address.  Sums over s cross
// the four wavefronts through the LDS in wavefront order, sums over channels (g_U) go through the DPP tree of wave_sum_f32 and, for O
// wider than one pass, are added pass after pass by the lane that owns the element; sums over rows go through per-block partials in the
// caller's workspace, added in f64 in a fixed order.  Every output element is written by one workgroup: no atomics, nothing is zeroed.
#include "common.h"

namespace {

constexpr int kExWaves = 4;          // wavefronts per workgroup
constexpr int kExMaxO = 1024, kExMaxJ = 4;
constexpr int kExBlockElems = 256;   // a statistics block holds about this many (r, s) positions: whole rows, at least one

__host__ __device__ static inline int ex_block_rows(int S) { return S >= kExBlockElems ? 1 : kExBlockElems / S; }
__host__ __device__ static inline int ex_blocks(int R, int S) { const int rb = ex_block_rows(S); return (R + rb - 1) / rb; }

enum { kExNone = 0, kExTrain = 1, kExEval = 2 };

template <int V>
__device__ __forceinline__ void ex_load(float (&d)[V], const float *__restrict__ p) {
    if (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
        d[0] = p[0];
    }
}
template <int V>
__device__ __forceinline__ void ex_store(float *__restrict__ p, const float (&d)[V]) {
    if (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(d[0], d[1], d[2], d[3]);
    else p[0] = d[0];
}

// the V channels of this lane in one pass: P's row entry is loaded per row, the rest once per pass
template <int V>
struct ExChan {
    float w[V][kExMaxJ];
    float mu[V], rs[V], ga[V], be[V];
};

template <int V, bool NORM>
__device__ __forceinline__ void ex_chan(ExChan<V> &ch, const float *__restrict__ Wu, const float *__restrict__ mean,
                                        const float *__restrict__ rstd, const float *__restrict__ gamma, const float *__restrict__ beta, int c,
                                        int J) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
#pragma unroll
        for (int j = 0; j < kExMaxJ; ++j) ch.w[v][j] = Wu[(size_t)(c + v) * J + min(j, J - 1)];
    }
    if (NORM) {
        ex_load<V>(ch.mu, mean + c); ex_load<V>(ch.rs, rstd + c); ex_load<V>(ch.ga, gamma + c); ex_load<V>(ch.be, beta + c);
    }
}

// U[., s, 0 ... J-1] (a wave-uniform address; the slots past J repeat the last one and are not used)
__device__ __forceinline__ void ex_u(float (&u)[kExMaxJ], const float *__restrict__ Urow, int s, int J) {
#pragma unroll
    for (int j = 0; j < kExMaxJ; ++j) u[j] = Urow[(size_t)s * J + min(j, J - 1)];
}

// y = P + (U0 Wu0, then fma in ascending j): include/upp_hip.h "broadcast expand"
template <int V>
__device__ __forceinline__ void ex_y(float (&y)[V], const float (&p)[V], const ExChan<V> &ch, const float (&u)[kExMaxJ], int J) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float t = u[0] * ch.w[v][0];
        if (J > 1) t = __builtin_fmaf(u[1], ch.w[v][1], t);
        if (J > 2) t = __builtin_fmaf(u[2], ch.w[v][2], t);
        if (J > 3) t = __builtin_fmaf(u[3], ch.w[v][3], t);
        y[v] = p[v] + t;
    }
}

// sum of one double per thread over a 256-thread workgroup, the same tree every time (as ec_block_sum)
__device__ __forceinline__ double ex_block_sum(double v, double *sh, int tid) {
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}

// part[(blk * 2 + 0) * O + c] = mean of y over the block's rows x S positions, [.. + 1 ..] = M2 about that mean; from sums shifted by
// the block's first value (no cancellation when |mean| >> std; a constant channel gives its value and 0 exactly).
template <int V>
__global__ __launch_bounds__(64 * kExWaves) void ex_stats_kernel(const float *__restrict__ P, const float *__restrict__ U, long long ustride,
                                                                 const float *__restrict__ Wu, float *__restrict__ part, int R, int S, int O,
                                                                 int J) {
    __shared__ float sh[2][kExWaves][64 * V];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int blk = blockIdx.x, rb = ex_block_rows(S), r0 = blk * rb, r1 = rb < R - r0 ? r0 + rb : R;
    for (int c0 = 0; c0 < O; c0 += 64 * V) {
        const bool live = c0 + lane * V < O;
        const int c = live ? c0 + lane * V : 0;                 // clamped: no branch around the loads
        ExChan<V> ch;
        ex_chan<V, false>(ch, Wu, nullptr, nullptr, nullptr, nullptr, c, J);
        float shift[V], a1[V], a2[V], p[V], u[kExMaxJ], y[V];
        ex_load<V>(p, P + (size_t)r0 * O + c);
        ex_u(u, U + (size_t)r0 * ustride, 0, J);
        ex_y<V>(shift, p, ch, u, J);
#pragma unroll
        for (int v = 0; v < V; ++v) a1[v] = a2[v] = 0.0f;
        for (int r = r0; r < r1; ++r) {
            ex_load<V>(p, P + (size_t)r * O + c);
            const float *Ur = U + (size_t)r * ustride;
            for (int s = wave; s < S; s += kExWaves) {
                ex_u(u, Ur, s, J);
                ex_y<V>(y, p, ch, u, J);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float d = y[v] - shift[v];
                    a1[v] += d;
                    a2[v] = __builtin_fmaf(d, d, a2[v]);
                }
            }
        }
        __syncthreads();                                        // (the previous pass has read sh)
#pragma unroll
        for (int v = 0; v < V; ++v) { sh[0][wave][lane * V + v] = a1[v]; sh[1][wave][lane * V + v] = a2[v]; }
        __syncthreads();
        if (wave == 0 && live) {
            const float n = (float)((r1 - r0) * S);
            float m[V], q[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int i = lane * V + v;
                const float s1 = ((sh[0][0][i] + sh[0][1][i]) + sh[0][2][i]) + sh[0][3][i];
                const float s2 = ((sh[1][0][i] + sh[1][1][i]) + sh[1][2][i]) + sh[1][3][i];
                m[v] = shift[v] + s1 / n;
                q[v] = s2 - s1 * s1 / n;
            }
            ex_store<V>(part + ((size_t)blk * 2 + 0) * O + c, m);
            ex_store<V>(part + ((size_t)blk * 2 + 1) * O + c, q);
        }
    }
}

// mean / biased variance / rstd of one channel from its block partials: two passes in f64,
//   mean = sum_i n_i m_i / N;   M2 = sum_i [ M2_i + n_i (m_i - mean)^2 ]
__global__ __launch_bounds__(256) void ex_finalize_kernel(const float *__restrict__ part, float *__restrict__ mean, float *__restrict__ var,
                                                          float *__restrict__ rstd, int blocks, int R, int S, int O, float eps) {
    __shared__ double sh[256];
    const int tid = threadIdx.x, c = blockIdx.x, rb = ex_block_rows(S);
    double s = 0.0;
    for (int i = tid; i < blocks; i += 256) {
        const double nb = (double)min((long long)rb, (long long)R - (long long)i * rb) * (double)S;
        s += nb * (double)part[((size_t)i * 2) * O + c];
    }
    const double N = (double)R * (double)S;
    const double mu = ex_block_sum(s, sh, tid) / N;
    double q = 0.0;
    for (int i = tid; i < blocks; i += 256) {
        const double nb = (double)min((long long)rb, (long long)R - (long long)i * rb) * (double)S;
        const double d = (double)part[((size_t)i * 2) * O + c] - mu;
        q += (double)part[((size_t)i * 2 + 1) * O + c] + nb * d * d;
    }
    const double m2 = ex_block_sum(q, sh, tid);
    if (tid == 0) {
        const float vr = (float)(m2 / N);
        mean[c] = (float)mu;
        var[c] = vr > 0.0f ? vr : 0.0f;
        rstd[c] = 1.0f / sqrtf((vr > 0.0f ? vr : 0.0f) + eps);
    }
}

// h[r,s,o] = lrelu(z): blockIdx.x = row, blockIdx.y = a chunk of `chunk` positions (any chunking writes the same bits)
template <int V, bool NORM>
__global__ __launch_bounds__(64 * kExWaves) void ex_apply_kernel(const float *__restrict__ P, const float *__restrict__ U, long long ustride,
                                                                 const float *__restrict__ Wu, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, const float *__restrict__ mean,
                                                                 const float *__restrict__ rstd, float slope, float *__restrict__ h, int S,
                                                                 int O, int J, int chunk) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.x, s0 = blockIdx.y * chunk, s1 = min(S, s0 + chunk);
    const float *Ur = U + (size_t)r * ustride;
    for (int c0 = 0; c0 < O; c0 += 64 * V) {
        const bool live = c0 + lane * V < O;
        const int c = live ? c0 + lane * V : 0;
        ExChan<V> ch;
        ex_chan<V, NORM>(ch, Wu, mean, rstd, gamma, beta, c, J);
        float p[V];
        ex_load<V>(p, P + (size_t)r * O + c);
        for (int s = s0 + wave; s < s1; s += kExWaves) {
            float u[kExMaxJ], y[V], o[V];
            ex_u(u, Ur, s, J);
            ex_y<V>(y, p, ch, u, J);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float z = NORM ? ((y[v] - ch.mu[v]) * ch.rs[v]) * ch.ga[v] + ch.be[v] : y[v];
                o[v] = z > 0.0f ? z : z * slope;
            }
            if (live) ex_store<V>(h + ((size_t)r * S + s) * O + c, o);
        }
    }
}

// per row block and channel: part[(blk * 2 + 0) * O + c] = sum g_z, [.. + 1 ..] = sum g_z xhat; rows ascending, a wavefront's positions
// ascending, the four wavefronts in order
template <int V>
__global__ __launch_bounds__(64 * kExWaves) void ex_bwd_reduce_kernel(const float *__restrict__ g_h, const float *__restrict__ P,
                                                                      const float *__restrict__ U, long long ustride,
                                                                      const float *__restrict__ Wu, const float *__restrict__ gamma,
                                                                      const float *__restrict__ beta, const float *__restrict__ mean,
                                                                      const float *__restrict__ rstd, float slope, float *__restrict__ part,
                                                                      int R, int S, int O, int J) {
    __shared__ float sh[2][kExWaves][64 * V];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int blk = blockIdx.x, rb = ex_block_rows(S), r0 = blk * rb, r1 = rb < R - r0 ? r0 + rb : R;
    for (int c0 = 0; c0 < O; c0 += 64 * V) {
        const bool live = c0 + lane * V < O;
        const int c = live ? c0 + lane * V : 0;
        ExChan<V> ch;
        ex_chan<V, true>(ch, Wu, mean, rstd, gamma, beta, c, J);
        float a0[V], a1[V];
#pragma unroll
        for (int v = 0; v < V; ++v) a0[v] = a1[v] = 0.0f;
        for (int r = r0; r < r1; ++r) {
            float p[V];
            ex_load<V>(p, P + (size_t)r * O + c);
            const float *Ur = U + (size_t)r * ustride;
            for (int s = wave; s < S; s += kExWaves) {
                float u[kExMaxJ], y[V], g[V];
                ex_u(u, Ur, s, J);
                ex_load<V>(g, g_h + ((size_t)r * S + s) * O + c);
                ex_y<V>(y, p, ch, u, J);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float xh = (y[v] - ch.mu[v]) * ch.rs[v];
                    const float gz = g[v] * (xh * ch.ga[v] + ch.be[v] > 0.0f ? 1.0f : slope);
                    a0[v] += gz;
                    a1[v] = __builtin_fmaf(gz, xh, a1[v]);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < V; ++v) { sh[0][wave][lane * V + v] = a0[v]; sh[1][wave][lane * V + v] = a1[v]; }
        __syncthreads();
        if (wave == 0 && live) {
            float t0[V], t1[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int i = lane * V + v;
                t0[v] = ((sh[0][0][i] + sh[0][1][i]) + sh[0][2][i]) + sh[0][3][i];
                t1[v] = ((sh[1][0][i] + sh[1][1][i]) + sh[1][2][i]) + sh[1][3][i];
            }
            ex_store<V>(part + ((size_t)blk * 2 + 0) * O + c, t0);
            ex_store<V>(part + ((size_t)blk * 2 + 1) * O + c, t1);
        }
    }
}

// g_beta[c] = sum over the blocks of part[.. 0 ..], g_gamma[c] of part[.. 1 ..] (f64, fixed tree); ms[2 c] = m1 = g_beta / N,
// ms[2 c + 1] = m2 = g_gamma / N
__global__ __launch_bounds__(256) void ex_bwd_param_kernel(const float *__restrict__ part, float *__restrict__ g_gamma,
                                                           float *__restrict__ g_beta, float *__restrict__ ms, int blocks, int R, int S, int O) {
    __shared__ double sh[256];
    const int tid = threadIdx.x, c = blockIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int i = tid; i < blocks; i += 256) {
        s0 += (double)part[((size_t)i * 2) * O + c];
        s1 += (double)part[((size_t)i * 2 + 1) * O + c];
    }
    const double t0 = ex_block_sum(s0, sh, tid);
    const double t1 = ex_block_sum(s1, sh, tid);
    if (tid == 0) {
        const double N = (double)R * (double)S;
        g_beta[c] = (float)t0;
        g_gamma[c] = (float)t1;
        ms[2 * (size_t)c] = (float)(t0 / N);
        ms[2 * (size_t)c + 1] = (float)(t1 / N);
    }
}

// g_y per element, never stored:  MODE train: (rstd gamma) ((g_z - m1) - xhat m2);  eval: (rstd gamma) g_z;  none: g_z.
//   g_P[r,c] = sum_s g_y  (a wavefront's positions ascending, the four wavefronts in order)
//   g_U[r,s,j] = sum_c g_y Wu[c,j]  (the lane's V channels ascending, wave_sum_f32's tree, passes ascending); skipped when g_U == NULL
//   wpart[(blk * J + j) * O + c] = sum over the block's rows and positions of g_y U[., s, j]
template <int V, int MODE>
__global__ __launch_bounds__(64 * kExWaves) void ex_bwd_apply_kernel(const float *__restrict__ g_h, const float *__restrict__ P,
                                                                     const float *__restrict__ U, long long ustride,
                                                                     const float *__restrict__ Wu, const float *__restrict__ gamma,
                                                                     const float *__restrict__ beta, const float *__restrict__ mean,
                                                                     const float *__restrict__ rstd, const float *__restrict__ ms, float slope,
                                                                     float *__restrict__ g_P, float *g_U, float *__restrict__ wpart, int R,
                                                                     int S, int O, int J) {
    __shared__ float sh[kExWaves][64 * V];
    __shared__ float shw[kExMaxJ][kExWaves][64 * V];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int blk = blockIdx.x, rb = ex_block_rows(S), r0 = blk * rb, r1 = rb < R - r0 ? r0 + rb : R;
    for (int c0 = 0; c0 < O; c0 += 64 * V) {
        const bool live = c0 + lane * V < O;
        const int c = live ? c0 + lane * V : 0;
        ExChan<V> ch;
        ex_chan<V, MODE != kExNone>(ch, Wu, mean, rstd, gamma, beta, c, J);
        float m1[V], m2[V], sc[V], aw[V][kExMaxJ];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            m1[v] = MODE == kExTrain ? ms[2 * (size_t)(c + v)] : 0.0f;
            m2[v] = MODE == kExTrain ? ms[2 * (size_t)(c + v) + 1] : 0.0f;
            sc[v] = MODE != kExNone ? ch.rs[v] * ch.ga[v] : 1.0f;
#pragma unroll
            for (int j = 0; j < kExMaxJ; ++j) aw[v][j] = 0.0f;
        }
        for (int r = r0; r < r1; ++r) {
            float p[V], ap[V];
            ex_load<V>(p, P + (size_t)r * O + c);
#pragma unroll
            for (int v = 0; v < V; ++v) ap[v] = 0.0f;
            const float *Ur = U + (size_t)r * ustride;
            for (int s = wave; s < S; s += kExWaves) {
                float u[kExMaxJ], y[V], g[V], gu[kExMaxJ];
                ex_u(u, Ur, s, J);
                ex_load<V>(g, g_h + ((size_t)r * S + s) * O + c);
                ex_y<V>(y, p, ch, u, J);
#pragma unroll
                for (int j = 0; j < kExMaxJ; ++j) gu[j] = 0.0f;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    float gy;
                    if (MODE == kExNone) {
                        gy = g[v] * (y[v] > 0.0f ? 1.0f : slope);
                    } else {
                        const float xh = (y[v] - ch.mu[v]) * ch.rs[v];
                        const float gz = g[v] * (xh * ch.ga[v] + ch.be[v] > 0.0f ? 1.0f : slope);
                        gy = MODE == kExTrain ? sc[v] * ((gz - m1[v]) - xh * m2[v]) : sc[v] * gz;
                    }
                    if (!live) gy = 0.0f;
                    ap[v] += gy;
#pragma unroll
                    for (int j = 0; j < kExMaxJ; ++j) {
                        aw[v][j] = __builtin_fmaf(gy, u[j], aw[v][j]);
                        gu[j] = __builtin_fmaf(gy, ch.w[v][j], gu[j]);
                    }
                }
                if (g_U) {                                                      // (uniform)
#pragma unroll
                    for (int j = 0; j < kExMaxJ; ++j) {
                        if (j < J) {
                            const float t = wave_sum_f32(gu[j]);
                            if (lane == 0) {
                                float *dst = g_U + ((size_t)r * S + s) * J + j;
                                *dst = c0 == 0 ? t : *dst + t;                   // this lane wrote it in the previous pass
                            }
                        }
                    }
                }
            }
            __syncthreads();                                                    // (the previous row has read sh)
#pragma unroll
            for (int v = 0; v < V; ++v) sh[wave][lane * V + v] = ap[v];
            __syncthreads();
            if (wave == 0 && live) {
                float t[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const int i = lane * V + v;
                    t[v] = ((sh[0][i] + sh[1][i]) + sh[2][i]) + sh[3][i];
                }
                ex_store<V>(g_P + (size_t)r * O + c, t);
            }
        }
        __syncthreads();                                                        // (the previous pass has read shw)
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int j = 0; j < kExMaxJ; ++j) shw[j][wave][lane * V + v] = aw[v][j];
        __syncthreads();
        if (wave == 0 && live) {
#pragma unroll
            for (int j = 0; j < kExMaxJ; ++j) {
                if (j < J) {
                    float t[V];
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const int i = lane * V + v;
                        t[v] = ((shw[j][0][i] + shw[j][1][i]) + shw[j][2][i]) + shw[j][3][i];
                    }
                    ex_store<V>(wpart + ((size_t)blk * J + j) * O + c, t);
                }
            }
        }
    }
}

// g_Wu[c,j] = sum over the blocks of wpart[(blk * J + j) * O + c]  (f64, fixed tree)
__global__ __launch_bounds__(256) void ex_bwd_wu_kernel(const float *__restrict__ wpart, float *__restrict__ g_Wu, int blocks, int O, int J) {
    __shared__ double sh[256];
    const int tid = threadIdx.x, c = blockIdx.x;
    for (int j = 0; j < J; ++j) {
        double s = 0.0;
        for (int i = tid; i < blocks; i += 256) s += (double)wpart[((size_t)i * J + j) * O + c];
        const double t = ex_block_sum(s, sh, tid);
        if (tid == 0) g_Wu[(size_t)c * J + j] = (float)t;
    }
}

static int ex_args(const void *P, const void *U, const void *Wu, const void *gamma, const void *beta, const void *mean, const void *rstd,
                   float slope, int mode, int R, int S, int O, int J) {
    if (!P || !U || !Wu || R < 1 || S < 1 || O < 1 || J < 1 || mode < kExNone || mode > kExEval || !(slope >= 0.0f && slope <= 1.0f))
        return UPP_E_BADARG;
    if (mode != kExNone && (!gamma || !beta || !mean || !rstd)) return UPP_E_BADARG;
    if (J > kExMaxJ || O > kExMaxO || (long long)R * S > 0x7FFFFFFFLL / O) return UPP_E_RANGE;
    return 0;
}

static bool ex_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" long long upp_expand_work_floats(int R, int S, int O) {
    if (R < 1 || S < 1 || O < 1) return 0;
    return (long long)ex_blocks(R, S) * O * (2 + kExMaxJ) + 2LL * O;
}

extern "C" int upp_expand_fwd(const float *P, const float *U, int per_row, const float *Wu, const float *gamma, const float *beta, float eps,
                              float slope, int mode, float *h, float *mean, float *var, float *rstd, float *work, int R, int S, int O, int J,
                              void *stream) {
    if (!h || !(eps >= 0.0f)) return UPP_E_BADARG;
    const int rc = ex_args(P, U, Wu, gamma, beta, mean, rstd, slope, mode, R, S, O, J);
    if (rc) return rc;
    if (mode == kExTrain && (!var || !work)) return UPP_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const long long ustride = per_row ? (long long)S * J : 0;
    const bool v4 = O % 4 == 0 && ex_aligned16(P) && ex_aligned16(h) && (mode == kExNone || (ex_aligned16(gamma) && ex_aligned16(beta) &&
                    ex_aligned16(mean) && ex_aligned16(rstd))) && (mode != kExTrain || ex_aligned16(work));
    const dim3 block(64 * kExWaves);
    if (mode == kExTrain) {
        const int blocks = ex_blocks(R, S);
        if (v4) hipLaunchKernelGGL((ex_stats_kernel<4>), dim3(blocks), block, 0, st, P, U, ustride, Wu, work, R, S, O, J);
        else hipLaunchKernelGGL((ex_stats_kernel<1>), dim3(blocks), block, 0, st, P, U, ustride, Wu, work, R, S, O, J);
        hipLaunchKernelGGL(ex_finalize_kernel, dim3(O), dim3(256), 0, st, work, mean, var, rstd, blocks, R, S, O, eps);
    }
    // about 2048 workgroups of at least 8 positions each; the grid's y extent stays far below 65536
    int chunks = (2048 + R - 1) / R;
    chunks = max(1, min(chunks, (S + 7) / 8));
    const int chunk = (S + chunks - 1) / chunks;
    const dim3 grid(R, (S + chunk - 1) / chunk);
    if (mode != kExNone) {
        if (v4) hipLaunchKernelGGL((ex_apply_kernel<4, true>), grid, block, 0, st, P, U, ustride, Wu, gamma, beta, mean, rstd, slope, h, S, O, J, chunk);
        else hipLaunchKernelGGL((ex_apply_kernel<1, true>), grid, block, 0, st, P, U, ustride, Wu, gamma, beta, mean, rstd, slope, h, S, O, J, chunk);
    } else {
        if (v4) hipLaunchKernelGGL((ex_apply_kernel<4, false>), grid, block, 0, st, P, U, ustride, Wu, gamma, beta, mean, rstd, slope, h, S, O, J, chunk);
        else hipLaunchKernelGGL((ex_apply_kernel<1, false>), grid, block, 0, st, P, U, ustride, Wu, gamma, beta, mean, rstd, slope, h, S, O, J, chunk);
    }
    return upp_launch_status();
}

extern "C" int upp_expand_bwd(const float *g_h, const float *P, const float *U, int per_row, const float *Wu, const float *gamma,
                              const float *beta, const float *mean, const float *rstd, float slope, int mode, float *g_P, float *g_U,
                              float *g_Wu, float *g_gamma, float *g_beta, float *work, int R, int S, int O, int J, void *stream) {
    if (!g_h || !g_P || !g_Wu || !work || (mode != kExNone && (!g_gamma || !g_beta))) return UPP_E_BADARG;
    const int rc = ex_args(P, U, Wu, gamma, beta, mean, rstd, slope, mode, R, S, O, J);
    if (rc) return rc;
    if (g_U && !per_row) return UPP_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const long long ustride = per_row ? (long long)S * J : 0;
    const int blocks = ex_blocks(R, S);
    float *ms = work + (size_t)blocks * 2 * O, *wpart = ms + 2 * (size_t)O;
    const bool v4 = O % 4 == 0 && ex_aligned16(P) && ex_aligned16(g_h) && ex_aligned16(g_P) && ex_aligned16(work) &&
                    (mode == kExNone || (ex_aligned16(gamma) && ex_aligned16(beta) && ex_aligned16(mean) && ex_aligned16(rstd)));
    const dim3 grid(blocks), block(64 * kExWaves);
    if (mode != kExNone) {
        if (v4) hipLaunchKernelGGL((ex_bwd_reduce_kernel<4>), grid, block, 0, st, g_h, P, U, ustride, Wu, gamma, beta, mean, rstd, slope, work, R, S, O, J);
        else hipLaunchKernelGGL((ex_bwd_reduce_kernel<1>), grid, block, 0, st, g_h, P, U, ustride, Wu, gamma, beta, mean, rstd, slope, work, R, S, O, J);
        hipLaunchKernelGGL(ex_bwd_param_kernel, dim3(O), dim3(256), 0, st, work, g_gamma, g_beta, ms, blocks, R, S, O);
    }
#define UPP_EX_BWD(V, MODE)                                                                                                                   \
    hipLaunchKernelGGL((ex_bwd_apply_kernel<V, MODE>), grid, block, 0, st, g_h, P, U, ustride, Wu, gamma, beta, mean, rstd, (const float *)ms, \
                       slope, g_P, g_U, wpart, R, S, O, J)
    if (mode == kExTrain) { if (v4) UPP_EX_BWD(4, kExTrain); else UPP_EX_BWD(1, kExTrain); }
    else if (mode == kExEval) { if (v4) UPP_EX_BWD(4, kExEval); else UPP_EX_BWD(1, kExEval); }
    else { if (v4) UPP_EX_BWD(4, kExNone); else UPP_EX_BWD(1, kExNone); }
#undef UPP_EX_BWD
    hipLaunchKernelGGL(ex_bwd_wu_kernel, dim3(O), dim3(256), 0, st, (const float *)wpart, g_Wu, blocks, O, J);
    return upp_launch_status();
}
