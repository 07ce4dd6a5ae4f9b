// eval.hip -- the two device pieces of a captured, vote-batched evaluation (upp_hip/infer.py EvalStep) around the model's
// eval-mode forward, replacing the torch glue of the reference's test loop (tools/runner_module.py:427-490, utils/evaluate.py):
//   * upp_vote_points : the V random subsets of the FPS-ordered superset, each scale/translate-augmented, gathered vote-major
//                       into ONE (V*B, N, 3) batch (3 V torch launches plus the advanced indexing of every vote).
//   * upp_vote_reduce : mean over the votes, arg-max, and the (correct, total) counters (torch's mean / argmax / == / sum, whose
//                       reductions would put memset nodes into a captured graph).
// Both are kernel launches only, wave64, vector stores only.
#include "common.h"

namespace {

constexpr int kBlock = 256;

constexpr long long kGridCap = 4096;

// out[(v*B + b), i, c] = superset[b, pick[v,i], c] * scale[v,b,c] + shift[v,b,c]   (two roundings: torch's `pc * s + t`)
// A pick outside [0, S) is never dereferenced: its point is written as NaN.
__global__ __launch_bounds__(kBlock) void vote_points_kernel(const float *__restrict__ superset, const int32_t *__restrict__ pick,
                                                             const float *__restrict__ scale, const float *__restrict__ shift,
                                                             float *__restrict__ out, int B, int S, int N, long long total) {
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long long)gridDim.x * kBlock) {
        const int c = (int)(e % 3);
        const long long p = e / 3;                 // ((v*B + b)*N + i)
        const int i = (int)(p % N);
        const long long vb = p / N;                // v*B + b
        const int b = (int)(vb % B);
        const int v = (int)(vb / B);
        const int j = pick[(long long)v * N + i];
        float x = (j >= 0 && j < S) ? superset[((long long)b * S + j) * 3 + c] : __builtin_nanf("");
        if (scale) x = __fmul_rn(x, scale[vb * 3 + c]);
        if (shift) x = __fadd_rn(x, shift[vb * 3 + c]);
        out[e] = x;
    }
}

// (a, ia) ranks before (b, ib)?  NaN above everything (torch.max / argmax), equal values: the lower index.
__device__ __forceinline__ bool ranks_first(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

// One workgroup.  Wave w takes the rows b = w, w + waves, ...; lane l the classes l, l + 64, ...
//   m[b][c] = (sum_{v = 0..V-1} logits[v*B + b][c]) / V,  pred[b] = first arg-max of m[b];  counters += (#correct of b < n_valid, n_valid)
__global__ __launch_bounds__(kBlock) void vote_reduce_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                             int V, int B, int C, int n_valid, int64_t *__restrict__ pred,
                                                             int64_t *__restrict__ counters) {
    __shared__ int s_correct[kBlock / UPP_WAVE];
    const int lane = threadIdx.x & (UPP_WAVE - 1);
    const int wave = threadIdx.x / UPP_WAVE;
    const int waves = blockDim.x / UPP_WAVE;
    const float fv = (float)V;
    int correct = 0;
    for (int b = wave; b < B; b += waves) {
        float best = -__builtin_inff();
        int bi = 0x7fffffff;
        for (int c = lane; c < C; c += UPP_WAVE) {
            float s = 0.0f;
            for (int v = 0; v < V; ++v) s = __fadd_rn(s, logits[((long long)v * B + b) * C + c]);
            const float m = __fdiv_rn(s, fv);
            if (ranks_first(m, c, best, bi)) { best = m; bi = c; }
        }
#pragma unroll
        for (int off = UPP_WAVE / 2; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off, UPP_WAVE);
            const int oi = __shfl_xor(bi, off, UPP_WAVE);
            if (ranks_first(ob, oi, best, bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) {
            pred[b] = (int64_t)bi;
            if (b < n_valid && (int64_t)bi == labels[b]) ++correct;
        }
    }
    if (lane == 0) s_correct[wave] = correct;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long n = 0;
        for (int w = 0; w < waves; ++w) n += s_correct[w];
        counters[0] += n;
        counters[1] += n_valid;
    }
}

}  // namespace

extern "C" int upp_vote_points(const float *superset, const int32_t *pick, const float *scale, const float *shift, float *out,
                               int B, int S, int N, int V, void *stream) {
    if (!superset || !pick || !out || B < 1 || S < 1 || N < 1 || V < 1) return UPP_E_BADARG;
    if ((long long)V * B > 0x7fffffffLL) return UPP_E_RANGE;
    const long long total = (long long)V * B * N * 3;
    hipLaunchKernelGGL(vote_points_kernel, dim3(grid_for(total, kBlock, kGridCap)), dim3(kBlock), 0, (hipStream_t)stream, superset, pick, scale, shift,
                       out, B, S, N, total);
    return upp_launch_status();
}

extern "C" int upp_vote_reduce(const float *logits, const int64_t *labels, int V, int B, int C, int n_valid, int64_t *pred,
                               int64_t *counters, void *stream) {
    if (!logits || !labels || !pred || !counters || V < 1 || B < 1 || C < 1) return UPP_E_BADARG;
    if (n_valid < 0 || n_valid > B || (long long)V * B > 0x7fffffffLL) return UPP_E_RANGE;
    hipLaunchKernelGGL(vote_reduce_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, logits, labels, V, B, C, n_valid, pred,
                       counters);
    return upp_launch_status();
}
