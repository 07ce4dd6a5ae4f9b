// ragged.hip -- per-cloud operators over a PACKED batch of clouds of different lengths: all points back to back in one (T, 3) array,
// cloud b is rows offsets[b] ... offsets[b+1]-1 (offsets: B + 1 int64 on the device).  The sampling kernel of this layout is the
// ragged form of fps_kernel (fps.hip: upp_fps_ragged); here is the step in front of it.
//
// cloud_norm_ragged_kernel: the reference's pc_norm (datasets/RealSensorDataset.py:59-65), which numpy evaluates in float64:
//       m = np.max(np.sqrt(np.sum(p ** 2, axis=1))) * 2;   out = (p / m).astype(float32)
// restated so that the result is the same bits:
//   * np.sum over an axis of length 3 is the sequential (x*x + y*y) + z*z, every product and sum rounded on its own: written with
//     __dmul_rn / __dadd_rn, which the compiler never contracts into an fma;
//   * an IEEE square root is monotone, so max_i sqrt(s_i) = sqrt(max_i s_i): ONE sqrt per cloud, and the maximum itself is exact in
//     any order -- the reduction over lanes and waves needs no fixed tree;
//   * p / m is an IEEE double division, then one rounding to float32 (round to nearest even, as numpy's astype and torch's .float()).
// One workgroup per cloud, two passes over its points (the second one hits the L2); plain vector loads and stores, no atomics, nothing
// to zero.  Precondition: finite coordinates (np.max propagates a NaN, fmax drops it).
#include "common.h"

namespace {

constexpr int kNormThreads = 256;

template <typename TIn>
__global__ __launch_bounds__(kNormThreads) void cloud_norm_ragged_kernel(const TIn *__restrict__ xyz, const int64_t *__restrict__ offsets,
                                                                         float *__restrict__ out, double *__restrict__ scale, int max_len) {
    __shared__ double part[kNormThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long first = offsets[b];
    long long n = offsets[b + 1] - first;
    n = n > max_len ? max_len : n;                       // a wrong promise of the caller: never past the cloud's own rows
    if (n < 1) {                                         // (refused by the Python layer; here: nothing to read, nothing to scale)
        if (scale && tid == 0) scale[b] = 0.0;
        return;
    }
    const TIn *p = xyz + first * 3;
    float *o = out + first * 3;
    double mx = 0.0;
    for (long long i = tid; i < n; i += kNormThreads) {
        const double x = (double)p[3 * i], y = (double)p[3 * i + 1], z = (double)p[3 * i + 2];
        const double s = __dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z));
        mx = fmax(mx, s);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d, 64));
    if ((tid & 63) == 0) part[tid >> 6] = mx;
    __syncthreads();
    mx = part[0];
#pragma unroll
    for (int w = 1; w < kNormThreads / 64; ++w) mx = fmax(mx, part[w]);
    const double m = __dmul_rn(__dsqrt_rn(mx), 2.0);
    if (scale && tid == 0) scale[b] = m;
    for (long long e = tid; e < 3 * n; e += kNormThreads) o[e] = (float)__ddiv_rn((double)p[e], m);
}

template <typename TIn>
int launch_norm(const TIn *xyz, const int64_t *offsets, float *out, double *scale, int B, int max_len, void *stream) {
    if (!xyz || !offsets || !out || B < 0 || max_len < 1) return UPP_E_BADARG;
    if (B == 0) return 0;
    hipLaunchKernelGGL((cloud_norm_ragged_kernel<TIn>), dim3(B), dim3(kNormThreads), 0, (hipStream_t)stream, xyz, offsets, out, scale, max_len);
    return upp_launch_status();
}

}  // namespace

extern "C" int upp_cloud_norm_ragged(const double *xyz, const int64_t *offsets, float *out, double *scale, int B, int max_len, void *stream) {
    return launch_norm(xyz, offsets, out, scale, B, max_len, stream);
}

extern "C" int upp_cloud_norm_ragged_f32(const float *xyz, const int64_t *offsets, float *out, double *scale, int B, int max_len, void *stream) {
    return launch_norm(xyz, offsets, out, scale, B, max_len, stream);
}
