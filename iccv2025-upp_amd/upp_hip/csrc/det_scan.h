// det_scan.h -- the deterministic (`_det`) siblings of the scatter-add backward kernels: ONE kernel body, det_scatter_kernel, and one
// small Job per operator.  The entry points and the files that hold their jobs:
//   upp_chamfer_bwd_det                                  ChamferJob          chamfer.hip
//   upp_group_bwd_det, upp_fps_gather_bwd_det            Rows3Job<IdxT>      group.hip
//   upp_gather_bwd_det, upp_grouping_bwd_det             GatherJob           group.hip     (grouping IS gather on the flat index list)
//   upp_three_interpolate_bwd_det                        InterpolateJob      pointnet2.hip
//   upp_knn_scatter_add_det, upp_edge_conv_bwd's g_A     KnnScatterJob       knn_points.hip
//   upp_deform_attn_bwd_det                              DeformJob           deform_attn.hip (values formed on the fly while staging)
//   upp_interp_max_bwd_det                               InterpMaxJob        interp_max.hip (a channel whose arg is another slot stages +0.0f)
//   upp_region_attn_bwd_det's d_PK / d_PV                RegionJob           region_attn.hip (sources read from the caller's rows workspace)
// (upp_emd_matchcost_det is an ordered sum of tile costs, not a scatter: emd.hip.)
//
// A scatter-add by f32 atomics sums each target's contributions in whatever order the hardware retires them.  Here every TARGET is
// one lane, and the lane walks the source list of its cloud in ASCENDING source index: a chunk of source keys (and the NV values
// each source contributes) is staged in the LDS by the whole workgroup, then every lane compares the keys with its own target and
// adds on a match -- one f32 addition at a time, in source order, whatever the lanes beside it do.  No inverse list, no sort, no
// integer atomics, no scratch, and no size limit: a cloud of any length goes through the same chunk loop.
//
// Cost: every workgroup of 256 targets reads all S sources of its cloud, so a cloud costs ceil(T / 256) x S staged sources and
// T x S / 64 wave-level key compares (four keys per ds_read_b128, all lanes the same address: a broadcast) -- O(T S) like the
// forward nearest-neighbour kernels, against O(S) atomics.  The index distribution does not change that figure: a target that owns
// EVERY source adds S terms in one dependent chain (S x one v_add_f32 latency, ~10 us at S = 3,000) while its wave's other lanes
// idle; nothing is ranked or sorted, so nothing goes quadratic.
#pragma once
#include "common.h"

constexpr int kDetThreads = 256;      // targets per workgroup, one per lane
constexpr int kDetChunk = 1024;       // sources per LDS chunk
constexpr int kDetCh = 4;             // channels per workgroup of the channels-first and row-of-U jobs

// acc[v] += vals[i][v] for every i < len4 (ascending) whose key equals `target`.  keys[len .. len4) hold -1 (len4 = len rounded up
// to 4); a lane without a target passes -2.  __fadd_rn: the addition stays an addition whatever the contraction setting.
template <int NV>
__device__ __forceinline__ void det_pull(const int32_t *keys, const float *vals, int len4, int target, float (&acc)[NV]) {
    for (int i = 0; i < len4; i += 4) {
        const int4 k = *reinterpret_cast<const int4 *>(keys + i);
        if (k.x == target || k.y == target || k.z == target || k.w == target) {
            const int kk[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (kk[q] == target) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) acc[v] = __fadd_rn(acc[v], vals[(i + q) * NV + v]);
                }
        }
    }
}

// grid of a det launch: one workgroup per (cloud, channel group, tile of targets) item, grid-stride beyond 16,384 workgroups
static inline unsigned det_grid(long long items) { return (unsigned)(items < 1 ? 1 : (items > 16384 ? 16384 : items)); }

__host__ __device__ static inline long long det_tiles(int T) { return (T + kDetThreads - 1) / kDetThreads; }      // tiles of 256 targets
__host__ __device__ static inline long long det_groups(int C) { return (C + kDetCh - 1) / kDetCh; }               // groups of kDetCh channels

// item -> (cloud b, first channel ch0 of the group, first target row0 of the tile) for a job whose clouds all have T targets and S sources
// and whose workgroups own kDetCh of C channels (C = 1: no channel groups)
struct DetItem { long long b; int ch0; long long row0; int T; long long S; };
__device__ __forceinline__ DetItem det_item(long long it, int C, int T, long long S) {
    const long long tiles = det_tiles(T), per = det_groups(C) * tiles, b = it / per, rest = it - b * per;
    return {b, (int)(rest / tiles) * kDetCh, (rest % tiles) * kDetThreads, T, S};
}

// The body of every `_det` scatter-add.  A workgroup serves one item: a tile of 256 targets (one per lane) of one cloud, for the NV values
// a source contributes (3 coordinates, or kDetCh channels: the key chunk staged once serves all of them).  What differs between the
// operators is the Job, a struct passed by value:
//   long long items()                      how many items the launch has (host and device)
//   Item item(it)                          item `it` decoded; Item has row0 (the tile's first target), T (targets of the cloud) and
//                                          S (sources of the cloud) beside whatever the job's other members need (cloud, channel group)
//   void first(item, r, acc)               the term target r adds to its +0.0f before any source (Chamfer's own term; nothing elsewhere)
//   void stage(item, c0, i, key, v)        the key of source c0 + i (-1: takes no part) and its NV values, written straight into the LDS
//                                          slot.  c0, the chunk's first source, is 64-bit and the same in every lane (it belongs on a
//                                          scalar base pointer); i < 1,024 is the lane's slot in the chunk
//   void store(item, r, acc)               the finished target r
// Every target of every item is stored, sources or none: the caller zero-fills nothing.
template <int NV, typename Job>
__global__ __launch_bounds__(kDetThreads) void det_scatter_kernel(const Job job) {
    __shared__ __attribute__((aligned(16))) int32_t keys[kDetChunk];
    __shared__ float vals[kDetChunk * NV];
    const int tid = threadIdx.x;
    const long long items = job.items();
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const auto w = job.item(it);
        const long long r = w.row0 + tid;
        const int target = r < w.T ? (int)r : -2;                       // (a surplus lane matches no key, the pad's -1 included)
        float acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = 0.0f;
        if (r < w.T) job.first(w, r, acc);
        for (long long c0 = 0; c0 < w.S; c0 += kDetChunk) {             // (64-bit: L * K and 3 n sources may pass 2^31)
            const int len = (int)min((long long)kDetChunk, w.S - c0), len4 = (len + 3) & ~3;
            __syncthreads();                                            // the previous chunk has been pulled by every lane
#pragma unroll
            for (int i = tid; i < kDetChunk; i += kDetThreads) {
                if (i < len) job.stage(w, c0, i, keys[i], vals + i * NV);
                else if (i < len4) keys[i] = -1;                        // det_pull reads four keys at a time
            }
            __syncthreads();
            det_pull<NV>(keys, vals, len4, target, acc);
        }
        if (r < w.T) job.store(w, r, acc);
    }
}

template <int NV, typename Job>
static inline void det_launch(const Job &job, void *stream) {
    hipLaunchKernelGGL((det_scatter_kernel<NV, Job>), dim3(det_grid(job.items())), dim3(kDetThreads), 0, (hipStream_t)stream, job);
}
