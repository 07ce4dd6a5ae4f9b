// det_scan.h -- the ordered "pull" behind the deterministic (`_det`) siblings of the scatter-add backward kernels
// (upp_chamfer_bwd_det, upp_group_bwd_det, upp_gather_bwd_det, upp_fps_gather_bwd_det, upp_three_interpolate_bwd_det,
// upp_grouping_bwd_det).
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

// grid of a det launch: one workgroup per (cloud, tile of targets) item, grid-stride beyond 16,384 workgroups
static inline unsigned det_grid(long long items) { return (unsigned)(items < 1 ? 1 : (items > 16384 ? 16384 : items)); }
