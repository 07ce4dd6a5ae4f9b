/*
 * upp_hip.h -- C ABI of libupp_hip.so, the MI355X (gfx950) implementation of
 * the UPP / Point-MAE hot-path operators.
 *
 * This is the drop-in boundary: every entry point replaces one native
 * operator the reference binds through a torch C++/CUDA extension (file:line
 * of the replaced interface is cited per function).  The signatures use only
 * plain device pointers, sizes and a HIP stream (passed as void*): no torch
 * types, no allocation inside the library, and no global state other than the
 * four documented options of upp_set_option() below (the *_ex entry points take
 * the kernel variant of a measurement as an ARGUMENT; the library never reads
 * the environment -- `grep getenv csrc/` is empty since ABI 5).  The caller owns
 * every buffer (including scratch) and the library never synchronises; all
 * work is enqueued on `stream` (hipStream_t; NULL = the default stream), and
 * all of it is KERNEL LAUNCHES: every entry point may be captured into a HIP
 * graph (the step drivers do so), and on ROCm 7.2.0 a memset node of a graph
 * works in its first replay only -- the library imports four runtime symbols
 * (hipLaunchKernel, hipFuncSetAttribute, hipGetLastError, hipGetErrorString;
 * tests/test_abi.py) and zeroes buffers with a kernel.
 *
 * Return value: 0 on success; a negative UPP_E_* code for an argument the
 * kernels cannot serve (nothing is launched); a positive value is a
 * hipError_t from the launch.  upp_error_string() renders either.
 *
 * All tensors are dense row-major ("contiguous") f32 unless noted; indices
 * are int32 or int64 exactly as the reference operators return them.
 */
#ifndef UPP_HIP_H
#define UPP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UPP_ABI_VERSION 5   /* 5 (round 6): the measured-slower experiments left the library: upp_ln_adapter_fwd_next, upp_linear_sb_resid_f32,
                               upp_linear_sb_ln_f32, upp_linear_sb_ln_usable (and the PRO = 2 instantiations, the wave-specialised weight-gradient kernel and the
                               nine environment reads behind them); + upp_set_option / upp_get_option, and the fused operators of the secondary recipes'
                               tails: upp_bn_rows_drop_*, upp_logsoftmax_rows_*, upp_nll_mean_*, upp_noise_loss_*, upp_linear_smallk_gelu_d_f32,
                               upp_fps_gather_bwd, upp_ln_adapter_bwd_factors / upp_adapter_wgrad_* (106 prototypes; 4 had 93).
                               4: + upp_argsort_rows, upp_group_max_fwd / _bwd.  3: split-bf16 Linear (upp_linear_sb_*); the k-parts protocol, the attention
                               `variant` entry points (upp_attn_*_ex) and the VALU / 32x32x2 attention kernels behind them are gone.
                               2: grouped weight gradients, register-tiled Linear codes; the round-1 *_set_* toggles are gone */

#define UPP_E_BADARG   (-1)  /* null pointer / non-positive size                   */
#define UPP_E_RANGE    (-2)  /* size outside what the kernels support (see below)  */
#define UPP_E_KGTN     (-3)  /* kNN: k > number of reference points                */

int         upp_abi_version(void);
const char *upp_error_string(int code);

/* ---- options: the library's only process-wide state -------------------------
 * Every knob of the library, each with the product's default (an A/B-measured choice; the other values exist for measurements and
 * tests).  Relaxed atomics: set them before launching work from several threads.  No entry point reads the environment; the Python
 * host (upp_hip/_abi.py) forwards the variables of the same names ONCE at load time so that the A/B scripts under tools/ keep working.
 *   UPP_OPT_SB_TUNED          1 | 0   upp_linear_sb_tile consults the measured tile table (csrc/linear_sb_tuned.h) before its cost
 *                                     model | the model alone                                          [env UPP_SB_TUNED]
 *   UPP_OPT_SB_XCD2D          2 | 0 | 4   column groups of the 2-D XCD tile map of one-round split-bf16 Linear launches with wide
 *                                     outputs (0: row-major XCD ranges); traffic only, same results    [env UPP_SB_XCD2D]
 *   UPP_OPT_STORE_WT          1 | 0   epilogue stores of the Linear kernels are agent-scope write-through (`sc1`) | plain
 *                                     (same results; the end-of-kernel write-back is what differs)     [env UPP_STORE_WT]
 *   UPP_OPT_EMBED_SPLIT_BF16  1 | 0   upp_patch_embed_fwd runs its two large products on the split-bf16 kernel | the exact-f32 chain
 *                                     of rounds 1-3 (read per call)                                    [env UPP_EMBED_SPLIT_BF16]
 * upp_set_option: 0, UPP_E_BADARG (unknown key) or UPP_E_RANGE (value not listed above).  upp_get_option: the value (>= 0) or UPP_E_BADARG. */
enum { UPP_OPT_SB_TUNED = 0, UPP_OPT_SB_XCD2D = 1, UPP_OPT_STORE_WT = 2, UPP_OPT_EMBED_SPLIT_BF16 = 3, UPP_OPT_COUNT = 4 };
int upp_set_option(int key, int value);
int upp_get_option(int key);

/* ---- furthest point sampling ------------------------------------------------
 * Replaces pointnet2_ops._ext.furthest_point_sampling(xyz, npoint)
 * (pointnet2_ops 3.0.0 sampling_gpu.cu furthest_point_sampling_kernel; called
 * from reference utils/misc.py:18, tools/runner_module.py:151,450).
 *   xyz     (B,N,3) f32
 *   idx     (B,M)   int32 out: idx[b,0] = 0, then the farthest-point sequence
 *   centers (B,M,3) f32 out or NULL: xyz[b, idx[b,j]] (fuses the
 *           gather_operation of utils/misc.py:19)
 * Semantics reproduced: running min-distance initialised to 1e10, points with
 * |p|^2 <= 1e-3 never sampled, ties broken exactly as the T-thread block
 * reduction of the CUDA kernel does (T = min(512, 2^floor(log2 N))).
 * Limits: 1 <= M, 1 <= N <= 32768. */
int upp_fps(const float *xyz, int32_t *idx, float *centers,
            int B, int N, int M, void *stream);
/* the same with the launch form forced: identical results.
 *   bits 0-7 of `waves`: wavefronts per cloud (1, 2, 4, 8; 0 = the library's choice = upp_fps) -- for measurements and tests;
 *   bits 8-11: clouds per workgroup (1, 2, 4; 0 = the default, one), bit 12: the launch reserves the whole LDS of the CUs it runs on.
 *       Several clouds per workgroup (4-wave launches of at most 8 points per lane, B divisible by the count) put a 32-cloud call on 16 or
 *       8 CUs instead of 32; with bit 12 no workgroup of another stream shares those CUs.  For callers that run FPS BESIDE another stream
 *       (the pipelined training step): the call itself is 11-39 % slower, the other stream's one-round GEMMs are no longer slowed by the
 *       workgroups they shared CUs with (tools/micro/fps_cpw_ab.sh).  Any other bit: UPP_E_BADARG. */
int upp_fps_ex(const float *xyz, int32_t *idx, float *centers,
               int B, int N, int M, int waves, void *stream);

/* ---- packed ("ragged") batches: clouds of different lengths --------------------
 * The clouds of a batch lie back to back in one (T,3) array; cloud b is rows offsets[b] ... offsets[b+1]-1 (offsets: B+1 int64 ON THE
 * DEVICE, non-decreasing from 0 to T; the Python layer checks them on the host).  max_len is a host promise: every length is in
 * [1, max_len].  It sizes the launch; a longer cloud is cut to its first max_len points, an empty one yields zeros -- neither reads or
 * writes outside its rows.  One launch per call, no host synchronisation, nothing is zeroed.
 *
 * upp_fps_ragged: furthest point sampling of every cloud of a packed batch in ONE launch.
 *   idx     (B,M)   int32 out: indices LOCAL to the cloud -- bit for bit what upp_fps returns for that cloud alone (B = 1, N = its length):
 *           the tie order of the reference kernel depends on N (T = min(512, 2^floor(log2 N))), so each workgroup derives it from its
 *           own cloud's length.  M > length is legal: once every distance is 0 the winner is point 0.
 *   centers (B,M,3) f32 out or NULL
 * Limits: 1 <= M, 1 <= max_len <= 32768.
 * upp_fps_ragged_slots (host function, no launch): the points one lane must hold so that EVERY length 1 ... max_len fits a launch of `waves`
 * wavefronts per cloud (1, 2, 4, 8; 0 = the library's choice for max_len) -- the maximum over the lengths, which the longest one need not
 * attain (511 points: 256 threads x 2; 512 points: 512 x 1). */
int upp_fps_ragged(const float *xyz, const int64_t *offsets, int32_t *idx, float *centers,
                   int B, int max_len, int M, void *stream);
int upp_fps_ragged_slots(int max_len, int waves);
/* upp_cloud_norm_ragged: the reference's pc_norm (datasets/RealSensorDataset.py:59-65) of every cloud of a packed batch, in float64 as
 * numpy evaluates it:  scale[b] = 2 sqrt(max_i ((x*x + y*y) + z*z)),  out = (float)(p / scale[b])  -- no contraction, IEEE sqrt and
 * division: the same bits as the numpy expression.  (Here max_len only caps the rows a workgroup touches; any positive value.)
 *   xyz   (T,3) f64 (upp_cloud_norm_ragged) or f32 (upp_cloud_norm_ragged_f32: upcast, then the same arithmetic)
 *   out   (T,3) f32 out
 *   scale (B,)  f64 out or NULL */
int upp_cloud_norm_ragged(const double *xyz, const int64_t *offsets, float *out, double *scale,
                          int B, int max_len, void *stream);
int upp_cloud_norm_ragged_f32(const float *xyz, const int64_t *offsets, float *out, double *scale,
                              int B, int max_len, void *stream);

/* ---- gather_operation ---------------------------------------------------------
 * Replaces pointnet2_ops._ext.gather_points / gather_points_grad
 * (sampling_gpu.cu gather_points_kernel / gather_points_grad_kernel; called
 * from reference utils/misc.py:19).
 *   feat (B,C,N) f32, idx (B,M) int32 -> out (B,C,M) f32
 * Backward: grad_feat (B,C,N) must be zero-filled by the caller; grad_out
 * (B,C,M) is scatter-added into it (f32 atomics, order unspecified -- as in
 * the CUDA kernel). */
int upp_gather_fwd(const float *feat, const int32_t *idx, float *out,
                   int B, int C, int N, int M, void *stream);
int upp_gather_bwd(const float *grad_out, const int32_t *idx, float *grad_feat,
                   int B, int C, int N, int M, void *stream);

/* ---- k nearest neighbours ------------------------------------------------------
 * Replaces knn_cuda.KNN(k, transpose_mode=True).forward(ref, query)
 * (KNN_CUDA 0.2 knn.cu cuComputeDistanceGlobal + cuInsertionSort +
 * cuParallelSqrt, looped over the batch in Python; constructed at reference
 * models/Point_MAE_unify.py:56, called :69).  One launch for the whole batch.
 *   ref   (B,N,3) f32, query (B,Q,3) f32
 *   dist  (B,Q,K) f32 out or NULL: Euclidean distances, ascending
 *   idx   (B,Q,K) int64 out: 0-based, ordered by (distance, index)
 *   neigh (B,Q,K,3) f32 out or NULL: ref[b, idx[b,q,j]] - query[b,q]  (fuses
 *         the gather + centre subtraction of Group.forward,
 *         models/Point_MAE_unify.py:73-88)
 * Limits: 1 <= K <= min(N, 64). */
int upp_knn(const float *ref, const float *query, float *dist, int64_t *idx, float *neigh,
            int B, int N, int Q, int K, void *stream);
/* the same with the k-th-smallest prefilter of the insertion sort switched off
 * (prefilter = 0; 1 = upp_knn): identical results, for measurements and tests. */
int upp_knn_ex(const float *ref, const float *query, float *dist, int64_t *idx, float *neigh,
               int B, int N, int Q, int K, int prefilter, void *stream);

/* ---- grouping gather (stand-alone) and its backward ----------------------------
 * Replaces the torch indexing of Group.forward (reference
 * models/Point_MAE_unify.py:73-88): out[b,g,k] = xyz[b, idx[b,g,k]] - center[b,g].
 *   xyz (B,N,3), center (B,G,3), idx (B,G,K) int64 in [0,N), out (B,G,K,3)
 * Backward: grad_xyz (B,N,3) must be zero-filled by the caller (scatter-add,
 * f32 atomics); grad_center (B,G,3) is overwritten with -sum_k grad_out.
 * Either gradient pointer may be NULL. */
int upp_group_fwd(const float *xyz, const float *center, const int64_t *idx, float *out,
                  int B, int N, int G, int K, void *stream);
int upp_group_bwd(const float *grad_out, const int64_t *idx, float *grad_xyz, float *grad_center,
                  int B, int N, int G, int K, void *stream);
/* upp_fps_gather_bwd (round 6): the backward of the centre gather that upp_fps fuses (reference utils/misc.py:19 gather_operation under
 * autograd): g_xyz (B,N,3) = zeros with g_centers[b][j] added at row idx[b][j] (int32, as upp_fps writes it) -- zero-fill, index
 * conversion and scatter in ONE launch, one workgroup per cloud. */
int upp_fps_gather_bwd(const float *g_centers, const int32_t *idx, float *g_xyz, int B, int N, int M, void *stream);

/* ---- the pointnet2_ops surface: ball_query, three_nn, three_interpolate, grouping_operation -------------
 * The rest of pointnet2_ops.pointnet2_utils (pointnet2_ops 3.0.0 ball_query_gpu.cu, interpolate_gpu.cu, group_points_gpu.cu; the
 * reference calls three_nn / three_interpolate from models/Transformer_utils.py:225-230).  The upstream CUDA sources were not at hand
 * when this was written: the rules below are RESTATED from them, as was done for FPS and kNN, and stay unpinned until they can be
 * compared with the CUDA kernels' output (tests/_pointnet2_reference.py is the same restatement in numpy).  Shapes, dtypes and tie
 * rules are upstream's; indices are int32.  Squared distances are the library's convention: with the f32 differences (x, y, z),
 * d2 = fma(z, z, fma(x, x, y * y)) (csrc/common.h sumsq3 = oracle/upp_oracle.c sumsq3).
 *
 * upp_ball_query: xyz (B,N,3), new_xyz (B,P,3) -> idx (B,P,nsample) int32.  For query j walk k = 0 ... N-1 in ascending order; k
 *   qualifies when d2 < radius * radius (the product formed in f32, the compare strict).  The FIRST qualifying k is written into all
 *   nsample slots; every qualifying k (the first included) goes into slot cnt++; the walk stops at cnt == nsample.  A query with no
 *   qualifying point yields zeros.  Every element of idx is written by the kernel: nothing to zero-fill.
 *   UPP_E_BADARG also for a radius that is not finite or <= 0 and for nsample < 1.
 * upp_three_nn: unknown (B,n,3), known (B,m,3) -> dist (B,n,3) f32, idx (B,n,3) int32: the three smallest d2 over ascending k by the
 *   strict-'<' cascade (d < best1, else d < best2, else d < best3), so equal distances keep the lower index first.  Indices start at
 *   0 and bests at +inf (f32 compares against +inf select what upstream's double 1e40 selects): with m < 3 the unfilled slots report
 *   index 0 and distance +inf.  dist is the SQUARE ROOT (one IEEE sqrt) of d2, as the upstream Python wrapper returns it.
 * upp_three_interpolate_fwd: features (B,C,m), idx (B,n,3) int32, weight (B,n,3) -> out (B,C,n):
 *   out[b][c][i] = (w0 * f[i0] + w1 * f[i1]) + w2 * f[i2] -- three products and two sums in exactly this order, each one f32 operation
 *   rounded to nearest, none contracted into an fma.  An index outside [0, m) reads 0.0f (and is skipped by the backward).
 * upp_three_interpolate_bwd: grad_out (B,C,n) -> grad_features (B,C,m), which must be zero-filled by the caller:
 *   grad_features[b][c][idx[b][i][j]] += grad_out[b][c][i] * weight[b][i][j] by f32 atomics, order unspecified (as upp_gather_bwd).
 * upp_grouping_fwd: features (B,C,N), idx (B,P,S) int32 in [0,N) -> out (B,C,P,S) = features[b][c][idx[b][p][s]].
 * upp_grouping_bwd: grad_out (B,C,P,S) scatter-added into the caller-zeroed grad_features (B,C,N), f32 atomics.
 *   (grouping_operation is gather_operation on the flattened (P S) index list: the same kernels serve both.)
 * The same two sums in a defined order: upp_three_interpolate_bwd_det / upp_grouping_bwd_det ("deterministic scatter-adds" below).
 * Every size must be positive (UPP_E_BADARG); B == 0 is a no-op.  Limits: B <= 65535 for upp_ball_query / upp_three_nn (UPP_E_RANGE
 * beyond: one grid row per cloud, as kNN / Chamfer / EMD); the other entry points loop their grid and have no batch limit;
 * P * S < 2^31. */
int upp_ball_query(const float *xyz, const float *new_xyz, float radius, int nsample, int32_t *idx,
                   int B, int N, int P, void *stream);
int upp_three_nn(const float *unknown, const float *known, float *dist, int32_t *idx,
                 int B, int n, int m, void *stream);
int upp_three_interpolate_fwd(const float *features, const int32_t *idx, const float *weight, float *out,
                              int B, int C, int m, int n, void *stream);
int upp_three_interpolate_bwd(const float *grad_out, const int32_t *idx, const float *weight, float *grad_features,
                              int B, int C, int m, int n, void *stream);
int upp_grouping_fwd(const float *features, const int32_t *idx, float *out,
                     int B, int C, int N, int P, int S, void *stream);
int upp_grouping_bwd(const float *grad_out, const int32_t *idx, float *grad_features,
                     int B, int C, int N, int P, int S, void *stream);

/* ---- the pytorch3d.ops surface: knn_points, knn_gather ---------------------------------------------------
 * The fourth third-party import of the reference's model files (`import pytorch3d.ops`; called as
 * pytorch3d.ops.knn_points(noise, partial, K=4, return_nn=True) at models/Point_MAE_pretask_dev.py:680).  The upstream sources
 * (pytorch3d/csrc/knn/knn.cu) were not at hand: the rules below are RESTATED, as for the pointnet2_ops surface above, and stay unpinned
 * until they can be compared with the CUDA kernels' output (tests/_knn_points_reference.py is the same restatement in numpy).
 *
 * upp_knn_points: p1 (N,P1,D), p2 (N,P2,D), lengths1 / lengths2 (N,) int64 ON THE DEVICE or NULL (= P1 / P2; clamped to [0, P] by the
 *   kernel, never read back) -> dists (N,P1,K) f32, idx (N,P1,K) int64, nn (N,P1,K,D) f32 or NULL.
 *   Distance of p1[n][i] and p2[n][r]:  d = 0; for j = 0 ... D-1 ascending: diff = p1[j] - p2[j]; d = fma(diff, diff, d)  (norm 2: the
 *   SQUARED distance, no root is taken) or d = d + |diff| (norm 1), one rounding per step.  At D = 3 this is ssd3 of csrc/common.h: the
 *   same query lists the same neighbours as upp_knn, and dists is the value upp_knn takes the square root of.
 *   Order: ascending (distance, index) over r < len2 = lengths2[n] -- a refinement of upstream, whose order among exactly equal
 *   distances is not defined.
 *   Padding: slots k >= min(K, len2) hold dists 0, idx 0, nn 0; rows i >= lengths1[n] are zero in all three outputs.  (Upstream gathers
 *   its zero index there, which puts p2[n][0] into nn: a deliberate deviation.)  Every element of the three outputs is written by the
 *   kernel: nothing to zero-fill.  One launch.
 *   Limits: 1 <= D <= 32, 1 <= K <= 64 (K may exceed P2), N <= 65535 -- UPP_E_RANGE beyond; norm must be 1 or 2 and every size
 *   positive (UPP_E_BADARG); N == 0 is a no-op.
 * upp_knn_points_bwd: from grad_dists (N,P1,K) and the forward's idx:  t[n][i][k][d] = (2.0f * g) * diff  (norm 2) or sign(diff) * g
 *   (norm 1; sign(0) = 0) with g = grad_dists[n][i][k], diff = p1[n][i][d] - p2[n][idx[n][i][k]][d]; 0.0f in padded slots.
 *   g_p1[n][i][d] = +0.0f, then + t[n][i][k][d] for the filled slots in ascending k (plain f32 adds).  t (N,P1,K,D) is an output: the
 *   gradient of p2 is the row scatter of -t (below).  One launch.
 * upp_knn_gather: x (N,M,U), idx (N,L,K) int64, lengths (N,) int64 or NULL -> out (N,L,K,U) = x[n][idx[n][l][k]], 0.0f in slots
 *   k >= lengths[n] (and for an index outside [0, M)).
 * upp_knn_scatter_add: src (N,L,K,U), idx (N,L,K) int64 -> out (N,M,U): out[n][idx[n][l][k]][u] += src[n][l][k][u] (-= with negate != 0)
 *   by f32 atomics in an unspecified order, over the slots with l < rows[n] and k < slots[n] (each list (N,) int64 or NULL = all) whose
 *   index lies in [0, M).  out is zeroed first BY A KERNEL of the library: the caller zero-fills nothing.  It serves the gradient of p2
 *   (src = t, negate) and the backward of upp_knn_gather.
 * upp_knn_scatter_add_det: the same sums in a defined order -- out[n][r][u] = +0.0f, then + src (or - src) of its slots in ascending
 *   l * K + k, one rounded f32 addition at a time (csrc/det_scan.h; every row is written, nothing is zeroed).
 * Limits of the last three: every size positive, L * K < 2^31, M * U < 2^31; they loop their grid and have no batch limit. */
int upp_knn_points(const float *p1, const float *p2, const int64_t *lengths1, const int64_t *lengths2,
                   float *dists, int64_t *idx, float *nn,
                   int N, int P1, int P2, int D, int K, int norm, void *stream);
int upp_knn_points_bwd(const float *p1, const float *p2, const int64_t *idx, const float *grad_dists,
                       const int64_t *lengths1, const int64_t *lengths2, float *g_p1, float *t,
                       int N, int P1, int P2, int D, int K, int norm, void *stream);
int upp_knn_gather(const float *x, const int64_t *idx, const int64_t *lengths, float *out,
                   int N, int M, int L, int K, int U, void *stream);
int upp_knn_scatter_add(const float *src, const int64_t *idx, const int64_t *rows, const int64_t *slots, float *out,
                        int N, int M, int L, int K, int U, int negate, void *stream);
int upp_knn_scatter_add_det(const float *src, const int64_t *idx, const int64_t *rows, const int64_t *slots, float *out,
                            int N, int M, int L, int K, int U, int negate, void *stream);

/* ---- edge convolution: gather, GroupNorm, LeakyReLU, max over the neighbours --------------------------------
 * One layer of the reference's DGCNN_Grouper (models/dgcnn_group.py:91-144, models/AdaPoinTr.py:559-623) and, without the norm, the local
 * branch of a PoinTr block (models/Transformer.py:176-213): max over k of act(norm(W [f_j - f_i ; f_i])).  With W = [W1 | W2] the conv is
 * W1 f_j + (W2 - W1) f_i, two per-point products the CALLER makes with upp_linear_*; these entry points take the products:
 *   A   (B,Nk,O) f32   key-side product            Bq  (B,Nq,O) f32   query-side product (+ bias)
 *   idx (B,Nq,K) int64 neighbour rows into Nk, as upp_knn returns them; they must lie in [0, Nk) (the kernels clamp: no fault)
 *   G > 0: GroupNorm(G, O) with gamma (O,), beta (O,), eps;  G == 0: no norm (gamma, beta, mean, rstd, work may be NULL)
 *   slope: LeakyReLU, 0 <= slope <= 1
 * Rules.  y[b,q,k,o] = A[b, idx[b,q,k], o] + Bq[b,q,o], one f32 addition.  Per (b, group) mean and BIASED variance over the group's
 *   O / G channels x Nq x K values of y, rstd = 1 / sqrt(var + eps), as torch.nn.GroupNorm.  The statistics are summed in a fixed order:
 *   (sum, M2) partials per slab of 8 query rows and channel (shifted by the slab's first value), combined in f64 as
 *   upp_bn_rows_fwd's finalize does (mean = sum S_i / N, M2 = sum [M2_i + n_i (S_i / n_i - mean)^2]); no atomics.
 *   z = ((y - mean) * rstd) * gamma + beta (four f32 operations, none contracted);  out = max_k lrelu(z),  lrelu(z) = z > 0 ? z : z * slope.
 *   Per channel every one of those steps is monotone in y, so the maximum is attained at the largest y when gamma * rstd > 0 and at the
 *   smallest when < 0: the kernel finds the extreme y and evaluates z ONCE -- the same bits as evaluating every z.  arg is defined ON y:
 *   the lowest k of the maximum of y when gamma * rstd > 0 (an f32 product), the lowest k of the minimum when < 0, 0 when it is zero;
 *   without a norm the lowest k of the maximum (z = y).
 *   -> out (B,Nq,O) f32, arg (B,Nq,O) uint8, mean / rstd (B,G) f32.  Every element is written by a kernel; 3 launches (1 without a norm).
 * Backward, from g_out (B,Nq,O):  g_z = g_out * (z > 0 ? 1 : slope) at k == arg, 0 elsewhere;  per group m1 = mean(gamma g_z),
 *   m2 = mean(gamma g_z xhat);  g_y = rstd * ((gamma g_z - m1) - xhat m2), dense in k (no norm: g_y = g_z);  g_Bq = sum_k g_y in ascending
 *   k;  g_A[b, idx[b,q,k]] += g_y;  g_gamma = sum g_z xhat, g_beta = sum g_z.  xhat = (y - mean) * rstd is recomputed from A, Bq, idx and
 *   the saved statistics, never stored.  m1, m2, g_gamma, g_beta are summed from per-slab partials in a fixed order (f64), g_Bq in
 *   registers: bit-identical from call to call.  g_A alone is a scatter-add:
 *     g_y == NULL: f32 atomics into g_A, which the library zeroes first WITH A KERNEL -- the order is the hardware's; no tensor of
 *                  B Nq K O elements exists in this mode.  5 launches + the zero fill (2 without a norm).
 *     g_y != NULL: (B,Nq,K,O) f32 scratch.  The kernel stores g_y there and g_A = upp_knn_scatter_add_det of it: every row's sum in
 *                  ascending q * K + k, every row written, nothing zeroed.
 *   work: upp_edge_conv_work_floats(B, Nq, O) floats (a host function; 0 for a non-positive size), for forward and backward alike.
 * Limits: 1 <= K <= 64, 1 <= O <= 512, G divides O, B <= 65535, Nq K, Nq O, Nk O < 2^31 and Nq < 2^30 -- UPP_E_RANGE beyond.  A null
 *   pointer, a non-positive size, G < 0, eps < 0 or a slope outside [0, 1] (NaN included): UPP_E_BADARG.  Both before any launch; B == 0
 *   is a no-op. */
long long upp_edge_conv_work_floats(int B, int Nq, int O);
int upp_edge_conv_fwd(const float *A, const float *Bq, const int64_t *idx, const float *gamma, const float *beta, float eps, float slope,
                      int G, float *out, uint8_t *arg, float *mean, float *rstd, float *work,
                      int B, int Nk, int Nq, int K, int O, void *stream);
int upp_edge_conv_bwd(const float *g_out, const float *A, const float *Bq, const int64_t *idx, const uint8_t *arg,
                      const float *gamma, const float *beta, const float *mean, const float *rstd, float slope, int G,
                      float *g_A, float *g_Bq, float *g_gamma, float *g_beta, float *work, float *g_y,
                      int B, int Nk, int Nq, int K, int O, void *stream);

/* ---- broadcast expand: a 1x1 conv over [u ; f repeated], BatchNorm, LeakyReLU ---------------------------------
 * Three layers of the reference's PoinTr multiply a concatenation in which one part is constant along an axis: Fold.folding1[0] and
 * folding2[0] (models/PoinTr.py:27-58, conv over [seed | fd1 ; feature repeated S times]) and PCTransformer.mlp_query[0]
 * (models/Transformer.py:324-332,413-416, conv over [global feature repeated M times ; coarse point]).  With W = [Wu | Wf] the conv is
 * (Wf f_r + b) + Wu u[r,s]: one per-ROW product the CALLER makes with upp_linear_*; these entry points take the product:
 *   P   (R,O) f32   the per-row product, bias included
 *   U   per_row != 0: (R,S,J) f32, one per row;   per_row == 0: (S,J) f32, shared by all rows
 *   Wu  (O,J) f32,  1 <= J <= 4
 *   mode 0: no norm (gamma, beta, mean, rstd, var, work may be NULL in the forward);
 *        1: an affine BatchNorm1d in training mode -- mean, var (biased), rstd (O,) are OUTPUTS of the forward;
 *        2: the same norm in eval mode -- mean and rstd (O,) are INPUTS (the caller's running mean and 1 / sqrt(running var + eps))
 *   slope: LeakyReLU, 0 <= slope <= 1 (0: ReLU)
 * Rules.  t = U[.,s,0] * Wu[o,0], then t = fma(U[.,s,j], Wu[o,j], t) for ascending j;  y[r,s,o] = P[r,o] + t, one f32 addition.  y is
 *   never stored.  Mode 1: per channel the mean and BIASED variance of y over all R S values, rstd = 1 / sqrt(var + eps), in a fixed
 *   order: (mean, M2) partials per block of rows and channel -- a block is max(1, 256 / S) whole rows; the partial is the block's sum
 *   over its count, kept as a mean so that a constant channel's mean is that constant exactly and its variance 0 -- from sums shifted by
 *   the block's first value, combined in f64 (Chan: mean = sum n_i m_i / N, M2 = sum [M2_i + n_i (m_i - mean)^2]); no atomics.
 *   z = ((y - mean) * rstd) * gamma + beta (four f32 operations, none contracted; mode 0: z = y);  h = z > 0 ? z : z * slope.
 *   -> h (R,S,O) f32.  Every element is written by a kernel; 3 launches in mode 1, 1 otherwise.
 * Backward, from g_h (R,S,O), with y and xhat = (y - mean) * rstd recomputed from P, U, Wu and the (O,) statistics:
 *   g_z = g_h * (z > 0 ? 1 : slope);   mode 1: m1 = mean(g_z), m2 = mean(g_z xhat), g_y = (rstd * gamma) * ((g_z - m1) - xhat * m2);
 *   mode 2: g_y = (rstd * gamma) * g_z;   mode 0: g_y = g_z.  g_y is never stored.
 *   g_P[r,o] = sum_s g_y;   g_U[r,s,j] = sum_o g_y Wu[o,j] (per-row U only; g_U may be NULL: not computed);
 *   g_Wu[o,j] = sum_{r,s} g_y U[.,s,j];   g_gamma[o] = sum g_z xhat,  g_beta[o] = sum g_z  (modes 1 and 2).
 *   Every sum has a fixed order and every output element is written by exactly one workgroup: sums over s in registers and across the
 *   workgroup's four wavefronts in wavefront order, sums over o by a fixed lane tree, sums over rows from per-block partials in `work`,
 *   added in f64 by a fixed tree.  No atomics, nothing is zeroed: bit-identical from call to call, in either library mode.
 *   4 launches in modes 1 and 2, 2 in mode 0.
 *   work: upp_expand_work_floats(R, S, O) floats (a host function; 0 for a non-positive size): the forward needs it in mode 1, the
 *   backward always.
 * Limits: 1 <= J <= 4, 1 <= O <= 1024, S >= 1, R >= 1, R S O < 2^31 -- UPP_E_RANGE beyond.  A null pointer, a non-positive size, an
 *   unknown mode, eps < 0, a slope outside [0, 1] (NaN included), g_U with a shared U: UPP_E_BADARG.  Both before any launch.  16-byte
 *   loads and stores are used when O is a multiple of 4 and the f32 arrays of O-sized rows are 16-byte aligned; the results do not
 *   depend on it. */
long long upp_expand_work_floats(int R, int S, int O);
int upp_expand_fwd(const float *P, const float *U, int per_row, const float *Wu, const float *gamma, const float *beta, float eps,
                   float slope, int mode, float *h, float *mean, float *var, float *rstd, float *work,
                   int R, int S, int O, int J, void *stream);
int upp_expand_bwd(const float *g_h, const float *P, const float *U, int per_row, const float *Wu, const float *gamma, const float *beta,
                   const float *mean, const float *rstd, float slope, int mode, float *g_P, float *g_U, float *g_Wu, float *g_gamma,
                   float *g_beta, float *work, int R, int S, int O, int J, void *stream);

/* ---- query selection: the Q best-ranked of M candidate points, then D extra points ----------------------------------------
 * Replaces the reference's argsort + expand + gather + cat (models/AdaPoinTr.py:855-865) and, in the backward, autograd's zero-fill
 * and scatter:
 *   score (B,M) f32, cand (B,M,3) f32, extra (B,D,3) f32 or NULL (D == 0)
 *   -> order (B,Q) int32: order[b,r] = the candidate of rank r, where the rank of i is the number of j with score_j > score_i, or
 *      score_j == score_i and j < i (descending, equal scores in ascending index order; NaN ranks as the largest and -0 equals +0: the
 *      order of upp_argsort_rows.  The reference's torch.argsort(descending=True) leaves the order of equal scores open.)
 *   -> out (B,Q+D,3) f32: out[b,r] = cand[b, order[b,r]] for r < Q, out[b,Q+d] = extra[b,d].
 *   One workgroup per cloud, its scores in the LDS; 1 launch.
 * Backward: g_out (B,Q+D,3), order (B,Q) -> g_cand (B,M,3): a selected row gets its gradient, every other row 0, each row written once
 *   (the inverse map is built in the LDS; an index outside [0, M) is ignored);  g_extra (B,D,3) = g_out[:, Q:] (NULL for D == 0).
 *   No atomics, nothing is zeroed beforehand; 1 launch.  score has no gradient.
 * Limits: 1 <= Q <= M <= 4096, D >= 0, B >= 1, 3 B (Q + D) < 2^31 -- UPP_E_RANGE for M > 4096, Q > M or a larger output; a null pointer or a non-positive B, M or Q, D < 0:
 *   UPP_E_BADARG.  Both before any launch. */
int upp_query_select_fwd(const float *score, const float *cand, const float *extra, float *out, int *order, int B, int M, int Q, int D,
                         void *stream);
int upp_query_select_bwd(const float *g_out, const int *order, float *g_cand, float *g_extra, int B, int M, int Q, int D, void *stream);

/* ---- deformable local cross-attention: the offset head and the gather-attend core (additions to ABI 5) -------------------------
 * What is left of DeformableLocalCrossAttention (reference models/Transformer_utils.py:269-491) once its three tall products are
 * taken through the gather (README "Deformable local cross-attention"): per (sample, query, neighbour slot) work with no GEMM in it.
 * C = 64 H channels, H heads of 64, G channel groups (G divides H), k neighbour slots, N queries, NK memory points.
 *
 * upp_deform_offset_fwd (forward only: nothing downstream of it is differentiable)
 *   A (B,G,NK,C), Bq (B,G,N,C) the per-point halves of the offset head's first Linear (bias in Bq); idx (B,N,k) int64 rows of the NK
 *   points (the list of upp_knn); pos (B,NK,3); gamma, beta (C) and eps of the LayerNorm; W3 (3,C)
 *   -> shift (B,G,N k,3): per row (b,g,n,s), with j = idx[b,n,s]:  y = A[b,g,j] + Bq[b,g,n] (one f32 addition per channel, never
 *      stored); LayerNorm over the C values (mean, then the BIASED variance of y - mean: two passes over the registers); exact (erf)
 *      GELU; three dot products with the rows of W3; shift = pos[b,j] + tanh(.).
 *   One wave per row, channel 64 i + lane in register i of the lane.  Every reduction (mean, variance, the three dot products) is the
 *   lane's partial over i ascending, then the fixed tree of the wave sum (xor 1, xor 2, half-row mirror, row mirror, (r0 + r1) +
 *   (r2 + r3)): the same bits on every run and for every batch size.  Each output element is written by one wave: no atomics, no
 *   scratch, nothing zeroed.  A row whose idx lies outside [0, NK) is never read through and gets NaN.  1 launch.
 *
 * upp_deform_attn_fwd
 *   q (B,N,C); PK, PV (B,G,NK,C) the per-group key / value products of the memory tokens; bk, bv (C) or NULL (= 0); idx3 int32 and
 *   w3 f32 (B,G,N k,3): the three nearest memory points of every shifted position and their interpolation weights; scale
 *   -> per (b, n, head h with channels [64 h, 64 h + 64)), for every slot s:
 *        key_s[ch] = bk[ch], then fma(w3[b,g,n k + s,j], PK[b,g,idx3[b,g,n k + s,j],ch], key_s[ch]) for ascending g, then ascending j;
 *        val_s likewise from PV and bv;  score_s = scale * sum_ch q[ch] key_s[ch] (the wave sum above);
 *        p = softmax over s with the maximum subtracted (expf, the sum by the wave sum, one division per slot);
 *        ctx[b,n,ch] = fma(p_s, val_s[ch], .) from +0 in ascending s.
 *      ctx (B,N,C) and p (B,N,H,k), which the backward reads.  The rows key_s / val_s live in registers only.  One wave per (b,n,h),
 *      lane = channel: every row read is one coalesced 256-byte segment.  Deterministic.  idx3 values are the caller's duty; one
 *      outside [0, NK) contributes nothing (never read or written through).  1 launch.
 *
 * upp_deform_attn_bwd / upp_deform_attn_bwd_det
 *   + p, d_ctx (B,N,C) -> d_q (B,N,C), d_PK, d_PV (B,G,NK,C), ds (B,N,H,k), d_krow (B,N,C) or NULL.  The rows are recomputed:
 *        dp_s = d_ctx . val_s;  ds_s = p_s (dp_s - sum_s p_s dp_s);  d_q = scale * (fma(ds_s, key_s, .) from +0 in ascending s);
 *        d_key_s = (scale * ds_s) * q, d_val_s = p_s * d_ctx (each product rounded once);  d_krow[b,n] = sum_s d_key_s in ascending s
 *        (its column sums are the gradient of bk; that of bv is the column sums of d_ctx);
 *        d_PK[b,g,idx3[..,j]] += w3[..,j] * d_key_s, d_PV likewise with d_val_s.  w3 and idx3 get no gradient.
 *      d_q, ds and d_krow have a fixed order in both forms.  upp_deform_attn_bwd: d_PK / d_PV are zeroed here by a kernel (no memset)
 *      and summed by f32 atomics, 256 contiguous bytes per wave instruction, in the order the hardware retires them: 3 launches.
 *      upp_deform_attn_bwd_det: d_PK[b,g,r,ch] = +0.0f, then + the rounded product of every source (n, s, j) with idx3 == r in ascending
 *      (n k + s) 3 + j, one rounded addition each; a job of the one `_det` kernel body (csrc/det_scan.h) whose sources are formed on
 *      the fly from w3, p, ds, q and d_ctx.  Every element is overwritten: nothing to zero.  2 launches.
 *
 * Limits: 1 <= H <= 16 (C a multiple of 64 for the offset), G divides H, 1 <= k <= 32, N, NK >= 1, B <= 65535 and every array below
 *   2^31 elements -- UPP_E_RANGE beyond.  A null pointer (bk, bv, d_krow excepted), a non-positive size, a scale or eps that is not
 *   finite and positive: UPP_E_BADARG.  Both before any launch. */
int upp_deform_offset_fwd(const float *A, const float *Bq, const int64_t *idx, const float *pos, const float *gamma, const float *beta,
                          const float *W3, float *shift, float eps, int B, int G, int N, int NK, int k, int C, void *stream);
int upp_deform_attn_fwd(const float *q, const float *PK, const float *PV, const float *bk, const float *bv, const int32_t *idx3,
                        const float *w3, float *ctx, float *p, float scale, int B, int N, int NK, int k, int H, int G, void *stream);
int upp_deform_attn_bwd(const float *q, const float *PK, const float *PV, const float *bk, const float *bv, const int32_t *idx3,
                        const float *w3, const float *p, const float *d_ctx, float *d_q, float *d_PK, float *d_PV, float *d_krow,
                        float *ds, float scale, int B, int N, int NK, int k, int H, int G, void *stream);
int upp_deform_attn_bwd_det(const float *q, const float *PK, const float *PV, const float *bk, const float *bv, const int32_t *idx3,
                            const float *w3, const float *p, const float *d_ctx, float *d_q, float *d_PK, float *d_PV, float *d_krow,
                            float *ds, float scale, int B, int N, int NK, int k, int H, int G, void *stream);

/* ---- deformable graph attention: the ball-scaled offset head and the interpolate-max (additions to ABI 5) --------------------------
 * What is left of improvedDeformableLocalGraphAttention (reference models/Transformer_utils.py:623-775) once its Linear layers are
 * taken through the gather (README "Deformable graph attention"), and the offset head of improvedDeformableLocalCrossAttention
 * (:493-621).  O channels, k neighbour slots, N queries, NK memory points.
 *
 * upp_deform_offset_ball_fwd (forward only)
 *   The operands, shapes, limits, error codes, mapping and reduction order of upp_deform_offset_fwd; only the last step differs.  With
 *   j_s = idx[b,n,s]:  r[d] = max_s pos[b,j_s,d] - min_s pos[b,j_s,d] over the k slots of (b,n), one f32 subtraction;
 *   shift = pos[b,j,d] + (tanh(.) * (0.5f * r[d])), each operation rounded once, none contracted.  A slot outside [0, NK) makes every
 *   row of its (b,n) NaN and is never read through.  k == 1 gives r = 0 and shift = pos[idx] exactly.  1 launch.
 *
 * upp_interp_max_fwd
 *   PW (B,NK,O) the key-side product of the memory points, Bq (B,N,O) the query-side product (+ bias); idx3 int32 and w3 f32
 *   (B, N k, 3): the three nearest memory points of every shifted position and their interpolation weights; slope of the LeakyReLU
 *   -> per (b,n,o), for every slot s:  y_s = Bq[b,n,o], then y_s = fma(w3[b,n k + s,j], PW[b,idx3[b,n k + s,j],o], y_s) for ascending
 *      j; an index outside [0, NK) contributes nothing (never read through).  m = max_s y_s, arg[b,n,o] = the lowest s that attains it
 *      (a NaN never wins; no y above -inf leaves m = -inf and arg 0, as the norm-free upp_edge_conv_fwd);  out = m > 0 ? m : m * slope.
 *      out (B,N,O) f32 and arg (B,N,O) uint8.  y is never stored.  One wave per (b, n, chunk of 64 channels), lane = channel: every
 *      row read is one coalesced 256-byte segment.  No atomics, nothing zeroed, deterministic.  1 launch.
 *
 * upp_interp_max_bwd / upp_interp_max_bwd_det
 *   g_out, out (B,N,O), arg, idx3, w3 -> d_Bq (B,N,O), d_PW (B,NK,O).  g = g_out * (m > 0 ? 1 : slope), where the sign of m is read
 *   off OUT (out > 0 exactly where m > 0, for every slope in [0, 1]): no row is read again.  d_Bq[b,n,o] = g, written once.
 *   d_PW[b, idx3[b, n k + arg, j], o] += w3[b, n k + arg, j] * g, the product rounded once (an arg beyond k - 1 counts as k - 1; an
 *   index outside [0, NK) is skipped).  w3 and idx3 get no gradient.
 *      upp_interp_max_bwd: d_PW is zeroed here by a kernel (no memset) and summed by f32 atomics in the order the hardware retires
 *      them: 2 launches + the zero fill.
 *      upp_interp_max_bwd_det: d_PW[b,r,o] = +0.0f, then + the rounded product of every source (n, j) with
 *      idx3[b, n k + arg[b,n,o], j] == r in ascending 3 n + j, one rounded addition each; a job of the one `_det` kernel body
 *      (csrc/det_scan.h).  The walk that was built: ALL (n k + s) 3 + j sources of the cloud in ascending order, a channel whose arg is
 *      another slot contributing +0.0f (x + 0.0f == x from a +0.0f start: the same bits), a source that none of the workgroup's
 *      channels chose taking no part.  Every element is overwritten: nothing to zero.  2 launches.
 *
 * Limits (interpolate-max): 1 <= k <= 32, 1 <= O <= 1024, N, NK >= 1, B <= 65535 and every array below 2^31 elements -- UPP_E_RANGE
 *   beyond.  A null pointer, a non-positive size, a slope outside [0, 1] or not finite: UPP_E_BADARG.  Both before any launch. */
int upp_deform_offset_ball_fwd(const float *A, const float *Bq, const int64_t *idx, const float *pos, const float *gamma, const float *beta,
                               const float *W3, float *shift, float eps, int B, int G, int N, int NK, int k, int C, void *stream);
int upp_interp_max_fwd(const float *PW, const float *Bq, const int32_t *idx3, const float *w3, float *out, uint8_t *arg, float slope,
                       int B, int N, int NK, int k, int O, void *stream);
int upp_interp_max_bwd(const float *g_out, const float *out, const uint8_t *arg, const int32_t *idx3, const float *w3, float *d_Bq,
                       float *d_PW, float slope, int B, int N, int NK, int k, int O, void *stream);
int upp_interp_max_bwd_det(const float *g_out, const float *out, const uint8_t *arg, const int32_t *idx3, const float *w3, float *d_Bq,
                           float *d_PW, float slope, int B, int N, int NK, int k, int O, void *stream);

/* ---- region-wise deformable attention: a k x k attention per token, max over its rows (additions to ABI 5) -----------------------
 * What is left of DeformableLocalAttention (reference models/Transformer_utils.py:159-266, block token `rw_deform`) once its tall
 * products are taken through the gather (README "Region-wise deformable attention"): per (sample, token, head) work with no GEMM in it.
 * C = 64 H channels, H heads of 64, G channel groups (G divides H), k neighbour slots, N tokens, NK memory points.
 *
 * upp_region_attn_fwd
 *   q (B,N,C) the projected queries; idx (B,N,k) int64 rows of q (the neighbour list); PK, PV (B,G,NK,C), bk, bv (C) or NULL (= 0),
 *   idx3 int32 and w3 f32 (B,G,N k,3), scale: what they are for upp_deform_attn_fwd
 *   -> per (b, n, head h with channels [64 h, 64 h + 64)):
 *        Q_t = q[b, idx[b,n,t]] for t < k (a zero row for an index outside [0, N));
 *        key_s[ch], val_s[ch] for s < k: the rows of upp_deform_attn_fwd, by the same statement (da_row of csrc/deform_row.h, which
 *          also holds the d_PK / d_PV atomic scatter and the size checks the two operators share): bias, then
 *          fma(w3, P[idx3], .) for ascending g, then ascending j; an idx3 outside [0, NK) contributes nothing;
 *        S[t,s] = scale * (fma(Q_t[ch], key_s[ch], .) from +0 in ascending ch), the product by scale rounded once;
 *        p[t,s] = expf(S[t,s] - max_s S[t,s]) / (the sum of the k exponentials from +0 in ascending s), one division per element;
 *        ctx_t[ch] = fma(p[t,s], val_s[ch], .) from +0 in ascending s;
 *        out[b,n,ch] = max_t ctx_t[ch], arg[b,n,ch] = the lowest t that attains it (a NaN never wins; no ctx above -inf leaves
 *          out = -inf and arg 0, as upp_interp_max_fwd).
 *      out (B,N,C) f32 and arg (B,N,C) uint8, which the backward reads.  Q_t, key_s, S and p live in the LDS, val_s and ctx_t in
 *      registers only: p is not stored (a (B,N,H,k,k) array is k / 64 of a (B,N,k,C) tensor); the backward forms it again.  One wave per (b,n,h): no atomics, nothing zeroed, deterministic.  Nothing is read or written
 *      through an index outside its range.  1 launch.
 *
 * upp_region_attn_bwd / upp_region_attn_bwd_det
 *   + arg, d_out (B,N,C) -> d_q (B,N,C), d_PK, d_PV (B,G,NK,C), d_krow, d_vrow (B,N,C) or NULL.  The rows and p are recomputed, p by
 *   the forward's own statement on the same rows (the forward's bits).  With g = d_out and a[ch] = min(arg[ch], k - 1):
 *        dp[t,s] = fma(g[ch], val_s[ch], .) from +0 over the channels of the head with a[ch] == t, in ascending ch;
 *        r_t = fma(p[t,s], dp[t,s], .) from +0 in ascending s;  ds[t,s] = p[t,s] * (dp[t,s] - r_t);
 *        d_Q_t[ch] = scale * (fma(ds[t,s], key_s[ch], .) from +0 in ascending s);
 *        d_key_s[ch] = scale * (fma(ds[t,s], Q_t[ch], .) from +0 in ascending t);  d_val_s[ch] = p[a[ch], s] * g[ch];
 *        d_krow[b,n] = sum_s d_key_s, d_vrow[b,n] = sum_s d_val_s from +0 in ascending s (their column sums are the gradients of
 *          bk and bv);
 *        d_q[b, idx[b,n,t]] += d_Q_t;  d_PK[b,g,idx3[..,j]] += w3[..,j] * d_key_s, d_PV likewise with d_val_s (each product rounded
 *          once).  An index outside its range receives nothing.  idx, w3 and idx3 get no gradient.
 *      upp_region_attn_bwd: d_q, d_PK and d_PV are zeroed here by a kernel (no memset) and summed by f32 atomics, 256 contiguous
 *      bytes per wave instruction, in the order the hardware retires them; no (B,N,k,C) array exists.  4 launches.
 *      upp_region_attn_bwd_det: the caller passes rows (3,B,N,k,C) f32, which receives d_Q, d_key and d_val (every element written);
 *      d_q is upp_knn_scatter_add_det of plane 0 over idx, in ascending n k + t; d_PK[b,g,r,ch] = +0.0f, then + the rounded product
 *      w3 * d_key_s of every source (n, s, j) with idx3 == r in ascending (n k + s) 3 + j, one rounded addition each, d_PV likewise:
 *      a job of the one `_det` kernel body (csrc/det_scan.h).  Every output element is overwritten: nothing to zero, nothing
 *      allocated.  3 launches.  d_krow and d_vrow have a fixed order in both forms.
 *
 * Limits: 1 <= H <= 16, G divides H, 1 <= k <= 32, N, NK >= 1, B <= 65535 and every array (d_PK, rows, idx3) below 2^31
 *   elements -- UPP_E_RANGE beyond.  A null pointer (bk, bv, d_krow, d_vrow excepted; rows only in the _det form), a non-positive
 *   size, a scale that is not finite and positive: UPP_E_BADARG.  Both before any launch. */
int upp_region_attn_fwd(const float *q, const int64_t *idx, const float *PK, const float *PV, const float *bk, const float *bv,
                        const int32_t *idx3, const float *w3, float *out, uint8_t *arg, float scale, int B, int N, int NK, int k, int H,
                        int G, void *stream);
int upp_region_attn_bwd(const float *q, const int64_t *idx, const float *PK, const float *PV, const float *bk, const float *bv,
                        const int32_t *idx3, const float *w3, const uint8_t *arg, const float *d_out, float *d_q,
                        float *d_PK, float *d_PV, float *d_krow, float *d_vrow, float scale, int B, int N, int NK, int k, int H, int G,
                        void *stream);
int upp_region_attn_bwd_det(const float *q, const int64_t *idx, const float *PK, const float *PV, const float *bk, const float *bv,
                            const int32_t *idx3, const float *w3, const uint8_t *arg, const float *d_out, float *d_q,
                            float *d_PK, float *d_PV, float *d_krow, float *d_vrow, float *rows, float scale, int B, int N, int NK,
                            int k, int H, int G, void *stream);

/* ---- Chamfer distance ----------------------------------------------------------
 * Replaces chamfer.forward / chamfer.backward (reference
 * extensions/chamfer_dist/chamfer_cuda.cpp:36-39, kernels chamfer.cu:15-145 and
 * :173-201).
 *   xyz1 (B,n,3), xyz2 (B,m,3)
 *   dist1 (B,n) f32, idx1 (B,n) int32: squared distance to, and index of, the
 *         nearest xyz2 point (lowest index among equal minima); dist2/idx2 the
 *         other direction.
 * Backward: g1 (B,n,3) and g2 (B,m,3) are OVERWRITTEN (no pre-zeroing: the reference's wrapper allocates zeros and its kernel adds,
 * chamfer.cu:194-199,215-222); sums by f32 atomics in an unspecified order as there -- in the LDS, one workgroup per cloud pair, when
 * both gradient arrays fit (n + m <= 5,461), in global memory otherwise.  The same sums in a defined order: upp_chamfer_bwd_det
 * ("deterministic scatter-adds" below).
 * idx1 / idx2 are TRUSTED by upp_chamfer_bwd: every idx1[b][j] must lie in [0, m) and every idx2[b][i] in [0, n), as upp_chamfer_fwd
 * writes them.  Neither the library nor its torch wrapper (which checks device, dtype, contiguity and the exact shape of every tensor
 * from metadata) can check the values without a synchronisation; an index outside the other cloud is a read and an atomic add outside
 * the caller's arrays.
 * NaN coordinates (a deviation from the reference): the comparison is `d < best`, which is false for NaN.  A query point with a NaN
 * coordinate gets dist = +inf and idx = 0 (chamfer.cu's `k == 0 ||` takes the first candidate unconditionally and returns NaN); a
 * NaN point of the other cloud is skipped by every other query.  The NaN is not lost: the point's own distance in its own direction
 * is non-finite, so both module losses (upp_chamfer_loss, L1 and L2) are non-finite; the other samples of the batch are untouched. */
int upp_chamfer_fwd(const float *xyz1, const float *xyz2,
                    float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                    int B, int n, int m, void *stream);
int upp_chamfer_bwd(const float *xyz1, const float *xyz2, const int32_t *idx1, const int32_t *idx2,
                    const float *grad_dist1, const float *grad_dist2, float *g1, float *g2,
                    int B, int n, int m, void *stream);
/* upp_chamfer_loss: the reductions of ChamferDistanceL1 / ChamferDistanceL2 (reference extensions/chamfer_dist/__init__.py:44-84) in two
 * launches: loss[0] = (mean sqrt dist1 + mean sqrt dist2) / 2 (l1 != 0) or mean dist1 + mean dist2 (l1 == 0), means over all B n resp.
 * B m entries; fac1 (B,n) / fac2 (B,m) receive d loss / d dist element-wise, so that the module's backward is upp_chamfer_bwd on
 * (upstream scalar x fac).  work: upp_chamfer_loss_work_floats() floats of scratch.  Sums in a fixed order. */
long long upp_chamfer_loss_work_floats(void);
int upp_chamfer_loss(const float *dist1, const float *dist2, int B, int n, int m, int l1, float *loss, float *fac1, float *fac2,
                     float *work, void *stream);

/* ---- approximate earth mover's distance ----------------------------------------
 * Replaces emd_cuda.approxmatch_forward / matchcost_forward / matchcost_backward
 * (reference extensions/emd/cuda/emd.cpp:23-27, kernels emd_kernel.cu:24-157,
 * :199-242, :285-354).
 *   xyz1 (B,n,3), xyz2 (B,m,3)
 *   match (B,m,n) f32 out (overwritten)
 *   work  f32 scratch of upp_emd_work_floats(B,n,m) elements
 *   cost  (B) f32 out: sum_{k,l} |xyz1[k]-xyz2[l]|^2 * match[l,k]
 *   grad1 (B,n,3), grad2 (B,m,3) out (overwritten); match is a constant.
 * Limits: n, m >= 1 (a cloud larger than the 1,024-point LDS tile is staged tile by tile).
 * After upp_emd_approxmatch, work holds the auction's state, in this order (csrc/emd.hip carve(); upp_emd_work_floats = 11 B (n + m)):
 *   remainL [B][n]      the mass each point of xyz1 still has after level 8 (the last level's own decrement is never applied:
 *                       nothing reads it)
 *   remainR [B][m]      the mass each point of xyz2 still has after all 10 levels
 *   ratioL  [10][B][n]  per level it (-4^7 ... -4^-1, then 0): remainL / (1e-9 + sum_l exp(level d) remainR[l]) at the start of the level
 *   ratioR  [10][B][m]  per level: min(remainR / (sumr + 1e-9), 1) remainR with sumr = remainR sum_k exp(level d) ratioL[it][k]
 * and match[b][l][k] = sum_it exp(level_it d[l][k]) ratioL[it][k] ratioR[it][l], accumulated in level order and stored once.  Every
 * element is written on every call (nothing to zero-fill).  tests/test_gpu_losses.py checks each level against float64 from these
 * factors.
 * NaN coordinates: as in the reference, fmaxf(0, NaN) = 0 and fminf(NaN, 1) = 1 in the remain / ratio updates, so a NaN does not
 * spread through the remains; it reaches match through the exponentials of the poisoned point's row or column, and the cost of that
 * sample is NaN.  The other samples of the batch are untouched. */
long long upp_emd_work_floats(int B, int n, int m);
int upp_emd_approxmatch(const float *xyz1, const float *xyz2, float *match, float *work,
                        int B, int n, int m, void *stream);
int upp_emd_matchcost(const float *xyz1, const float *xyz2, const float *match, float *cost,
                      int B, int n, int m, void *stream);
int upp_emd_matchcost_bwd(const float *grad_cost, const float *xyz1, const float *xyz2, const float *match,
                          float *grad1, float *grad2, int B, int n, int m, void *stream);

/* ---- deterministic scatter-adds ---------------------------------------------------
 * Per-call siblings of the seven entry points whose f32 sums the hardware orders (atomics): the arguments, shapes, limits and error
 * codes of the sibling (upp_emd_matchcost_det takes a scratch pointer besides), the same terms, a DEFINED summation order -- each
 * can be restated on the CPU and compared bit for bit (tests/_det_reference.py), and two runs give the same bits.  Every product
 * and sum below is one f32 operation rounded to nearest, none contracted into an fma.  Every output is overwritten in full on
 * every launch (nothing to zero-fill), all work is kernel launches, nothing is allocated or read back.  No process-wide switch:
 * the choice is the entry point.  Kernels: one lane per TARGET walks its cloud's sources in ascending index (csrc/det_scan.h:
 * O(targets x sources / 64) wave steps per cloud whatever the index distribution, no size limit, no scratch).
 *
 *   upp_chamfer_bwd_det     t1(j)[c] = (grad_dist1[b][j] * 2.0f) * (xyz1[b][j][c] - xyz2[b][idx1[b][j]][c]), t2(i) likewise from cloud 2.
 *                           g1[b][j][c] = +0.0f + t1(j)[c], then - t2(i)[c] for every i with idx2[b][i] == j, in ascending i;
 *                           g2 the mirror image.  (+0.0f first, as the sibling's zero-filled accumulators: where a target has at
 *                           most one foreign term the result has upp_chamfer_bwd's bits.)
 *   upp_group_bwd_det       grad_xyz[b][r][c] = +0.0f, then + grad_out[b][g][k][c] for every (g,k) with idx[b][g][k] == r, in
 *                           ascending g * K + k; grad_xyz needs NO zero-fill.  grad_center as upp_group_bwd (k ascending there too).
 *   upp_gather_bwd_det      grad_feat[b][ch][r] = +0.0f, then + grad_out[b][ch][j] for every j with idx[b][j] == r, ascending j;
 *                           grad_feat needs NO zero-fill.
 *   upp_fps_gather_bwd_det  g_xyz[b][r][c] = +0.0f, then + g_centers[b][j][c] for every j with idx[b][j] == r, ascending j; indices
 *                           outside [0, N) are skipped.
 *   upp_emd_matchcost_det   p_t = the value upp_emd_matchcost adds for the t-th tile of 64 points of xyz1 (same arithmetic);
 *                           cost[b] = ((+0.0f + p_0) + p_1) + ... in ascending t.  work: upp_emd_matchcost_det_work_bytes(B,n,m)
 *                           bytes of scratch (the p_t; a host function, 0 for a negative argument).
 *   upp_three_interpolate_bwd_det  grad_features[b][ch][r] = +0.0f, then + (grad_out[b][ch][i] * weight[b][i][j]) for every (i, j)
 *                           with idx[b][i][j] == r, in ascending i * 3 + j (the product rounded first, then the sum); indices outside
 *                           [0, m) are skipped; grad_features needs NO zero-fill.
 *   upp_grouping_bwd_det    grad_features[b][ch][r] = +0.0f, then + grad_out[b][ch][p][s] for every (p, s) with idx[b][p][s] == r,
 *                           in ascending p * S + s; grad_features needs NO zero-fill (upp_gather_bwd_det on the flattened list).
 *   upp_knn_scatter_add_det stated and declared with its sibling under "the pytorch3d.ops surface" above: ascending l * K + k.
 *   upp_deform_attn_bwd_det stated and declared with its sibling under "deformable local cross-attention" above: ascending
 *                           (n k + s) 3 + j.
 *   upp_interp_max_bwd_det  stated and declared with its sibling under "deformable graph attention" above: ascending 3 n + j.
 *   upp_region_attn_bwd_det stated and declared with its sibling under "region-wise deformable attention" above: ascending n k + t
 *                           (d_q) and (n k + s) 3 + j (d_PK, d_PV). */
int upp_chamfer_bwd_det(const float *xyz1, const float *xyz2, const int32_t *idx1, const int32_t *idx2,
                        const float *grad_dist1, const float *grad_dist2, float *g1, float *g2,
                        int B, int n, int m, void *stream);
int upp_group_bwd_det(const float *grad_out, const int64_t *idx, float *grad_xyz, float *grad_center,
                      int B, int N, int G, int K, void *stream);
int upp_gather_bwd_det(const float *grad_out, const int32_t *idx, float *grad_feat,
                       int B, int C, int N, int M, void *stream);
int upp_fps_gather_bwd_det(const float *g_centers, const int32_t *idx, float *g_xyz, int B, int N, int M, void *stream);
int upp_three_interpolate_bwd_det(const float *grad_out, const int32_t *idx, const float *weight, float *grad_features,
                                  int B, int C, int m, int n, void *stream);
int upp_grouping_bwd_det(const float *grad_out, const int32_t *idx, float *grad_features,
                         int B, int C, int N, int P, int S, void *stream);
long long upp_emd_matchcost_det_work_bytes(int B, int n, int m);
int upp_emd_matchcost_det(const float *xyz1, const float *xyz2, const float *match, float *cost, float *work,
                          int B, int n, int m, void *stream);

/* ---- patch embedding (mini-PointNet) forward --------------------------------------
 * Replaces Encoder.forward (reference models/Point_MAE_unify.py:191-222): the chain
 * Conv1d(3,128)-BN-ReLU-Conv1d(128,256) -> group max -> concat -> Conv1d(512,512)-BN-ReLU-
 * Conv1d(512,C) -> group max, as FP32-MFMA GEMMs with BatchNorm statistics, normalisation,
 * ReLU and both max-pools fused into GEMM prologues / epilogues.
 *   pts  (R,3) f32: the centred neighbourhoods, R = B*G*n rows, n = points per group (16 or 32)
 *   w1 (128,3) b1 (128) | w2 (256,128) b2 (256) | w3 (512,512) b3 (512) | w4 (C,512) b4 (C):
 *        the Conv1d weights with their trailing kernel dimension of 1 dropped
 *   bn1_* (128), bn3_* (512): BatchNorm1d weight / bias / running_mean / running_var
 *   training != 0: batch statistics (biased variance) normalise, running stats are updated
 *        in place with `momentum` and the unbiased variance, as nn.BatchNorm1d does;
 *        training == 0: running statistics normalise, nothing is written to them.
 *   work: upp_patch_embed_work_floats(R, n) floats of scratch (16-byte aligned)
 *   out  (R/n, C) f32
 * Forward only (the encoder is frozen in every UPP recipe).
 * Arithmetic (round 4): the 256 -> 512 and 512 -> C products run on the split-bf16 kernel of upp_linear_sb_f32 (both f32 operands as
 * three bf16 terms, six products, f32 accumulation: the error of an f32 GEMM) for C <= 1024, their weights split into `work` by every
 * call; option UPP_OPT_EMBED_SPLIT_BF16 = 0 (read per call) keeps the exact-f32 chain of rounds 1-3.  BatchNorm batch
 * statistics are sums of per-workgroup partial sums in a fixed order (no atomics): the call is deterministic.
 * Limits: n in {16, 32}, R % n == 0, C % 4 == 0. */
long long upp_patch_embed_work_floats(int R, int n);
int upp_patch_embed_fwd(const float *pts, int R, int n,
                        const float *w1, const float *b1, const float *bn1_gamma, const float *bn1_beta,
                        float *bn1_rmean, float *bn1_rvar,
                        const float *w2, const float *b2,
                        const float *w3, const float *b3, const float *bn3_gamma, const float *bn3_beta,
                        float *bn3_rmean, float *bn3_rvar,
                        const float *w4, const float *b4, int C,
                        float momentum, float eps, int training,
                        float *work, float *out, void *stream);

/* ---- Transformer block glue: row gather (+pos) (+scaled residual) -> LayerNorm -----------
 * Fuses the element-wise steps of Block.forward around its GEMMs (reference
 * models/Point_MAE_pretask_dev.py:245-321): `x + pos` (TransformerEncoder :348), prompt insertion
 * (:247-264) or removal (:305-310), `x + drop_path(branch)` (:266,273; timm DropPath: per-sample factor
 * floor(keep + u) / keep), and the following LayerNorm (norm1 / norm2 / Adapter.layer_norm :97).
 *   s = src(t): mode 0 identity | 1 insert P prompts after the cls row | 2 insert P prompts in front |
 *                3 strip the P prompts after the cls row | 4 strip P leading prompts
 *   out row (b,t) = x[b, s] (+ add[b, s])                  if s is a token row
 *                 = prompts[p]                             if s selects prompt p (modes 1, 2)
 *                 (+ floor(keep + u[b]) / keep * (y[b, s] + ybias))  if y (row-aligned with x; u NULL: factor 1; ybias (D)
 *                    NULL or the bias of the Linear whose bias-free GEMM produced y)
 *   xo (B,Lout,D) = those rows (optional);  h = LayerNorm(rows) * gamma + beta, mean / rstd (B,Lout) saved
 *   (gamma NULL: no LayerNorm, only xo).
 * Backward: d = g_xo + LayerNormBackward(g_h); written to g_x[b, s] (every row of g_x / g_y is written: the prompt
 * rows a strip mode drops get zeros), g_prompt (B,P,D) (caller sums over B), g_y[b, s] = factor * d.
 * ln_part (optional, upp_rowln_part_floats floats): per-workgroup partials (workgroups, 2, D) of d_gamma = sum g_h * xhat and
 * d_beta = sum g_h, produced by the same pass; the caller sums them over the workgroups (upp_batched_sum).
 * upp_ln_param_grad: the same partial sums as a stand-alone pass, part (2, chunks, D).
 * Limits: D <= 512. */
int upp_rowln_fwd(const float *x, const float *add, const float *prompts, int mode, int P, const float *y, const float *ybias,
                  const float *u, float keep, const float *gamma, const float *beta, float eps,
                  float *xo, float *h, float *mean, float *rstd, int B, int Lin, int Lout, int D, void *stream);
long long upp_rowln_part_floats(int B, int Lin, int Lout, int D, int mode);
int upp_rowln_bwd(const float *g_xo, const float *g_h, const float *xo, const float *mean, const float *rstd,
                  const float *gamma, int mode, const float *u, float keep,
                  float *g_x, float *g_prompt, float *g_y, float *ln_part,
                  int B, int Lin, int Lout, int D, int P, void *stream);
/* upp_bias_gelu_fwd / bwd: h = GELU(z + bias) (erf form) for the bias-free GEMM output z (rows, C) of Mlp.fc1, and
 * g_z = g_h * GELU'(z + bias).  C % 4 == 0. */
int upp_bias_gelu_fwd(const float *z, const float *bias, float *h, long long rows, int C, void *stream);
int upp_bias_gelu_bwd(const float *g_h, const float *z, const float *bias, float *g_z, long long rows, int C, void *stream);
/* upp_bias_gelu_fwd_d: the forward that also stores d = GELU'(z + bias) (rows, C): the backward of a training step is then
 * g_z = g_h * d, one multiply per element. */
int upp_bias_gelu_fwd_d(const float *z, const float *bias, float *h, float *d, long long rows, int C, void *stream);
int upp_ln_param_grad(const float *g_h, const float *xo, const float *mean, const float *rstd, float *part,
                      int rows, int D, int chunks, void *stream);

/* ---- multi-head attention core ------------------------------------------------------------
 * Replaces the unfused q@k^T -> *scale -> softmax -> @v of Attention.forward (reference
 * models/Point_MAE_pretask_dev.py:186-193) and its autograd.
 *   qkv (B,L,3,H,64): the qkv Linear output as the reference reshapes it (:186)
 *   ctx (B,L,H*64): softmax(q k^T * scale) v, already in the layout of (:193) `.transpose(1,2).reshape(B,N,C)`
 *   lse (B,H,L): log-sum-exp of the scaled scores (saved for backward)
 *   d_qkv (B,L,3,H,64) from d_ctx (B,L,H*64)
 * All arrays are dense (no strides) and hold exactly the element counts above.  qkv, ctx and d_ctx must be 16-byte aligned: the kernels
 * load them in 16-byte pieces (every row is a multiple of 256 bytes, so an aligned base aligns every piece).  The library does not check
 * the alignment; the torch operators (upp_hip/ops.py attn_fwd / attn_bwd) check it, and the element counts, before they launch.
 * Limits: head_dim == 64; 1 <= L <= UPP_ATTN_MAX_L, forward and backward alike; UPP_E_RANGE beyond (checked before the B == 0 return).
 * No atomics, no workspace, no memset at any L: two calls on the same inputs give the same bits. */
#define UPP_ATTN_MAX_L 2048   /* the longest sequence the attention entry points serve (the longest one the test suite covers) */
int upp_attn_fwd(const float *qkv, float *ctx, float *lse, int B, int L, int H, int head_dim, float scale, void *stream);
int upp_attn_bwd(const float *qkv, const float *ctx, const float *d_ctx, const float *lse, float *d_qkv,
                 int B, int L, int H, int head_dim, float scale, void *stream);
/* (L <= 96: the register-resident 16x16x4 MFMA kernels of attn_flash16.hip; L <= 160: attn_long.hip, K and V resident in the LDS;
 *  L <= UPP_ATTN_MAX_L: attn_stream.hip, 64-row query blocks against K / V streamed in 64-key blocks, online softmax) */
/* ---- cross-attention: queries and keys from two sequences -----------------------------------
 * softmax(q k^T * scale) v of CrossAttention.forward (reference models/Transformer.py:148-152) and its autograd; csrc/attn_stream.hip,
 * one streaming family (the structure and the summation order of attn_stream.hip) for every length in the range.
 *   q, d_q            (B, Lq, rs) arrays: head h lives in columns [64h, 64h+64) counted from the pointer
 *   k, v, d_k, d_v    (B, Lk, rs) arrays with the same head layout
 *   *_rs              the row strides in floats, one per array; the sample stride of an array is L * rs.  This admits three separate
 *                     Linear outputs (rs = H*64), a packed [k|v] product (rs = 2*H*64, v = k + H*64) and views into a packed qkv
 *                     (rs = 3*H*64).
 *   ctx, d_ctx        dense (B, Lq, H*64);  lse dense (B, H, Lq)
 * Checked before any launch -- UPP_E_BADARG: a null pointer, B < 0, a length < 1, H < 1, a stride < H*64 or not a multiple of 4;
 * UPP_E_RANGE: head_dim != 64 or a length > UPP_ATTN_MAX_L (before the B == 0 return, as upp_attn_fwd).
 * The caller's duties: every base 16-byte aligned (the kernels load 16-byte pieces), and d_q, d_k, d_v not overlapping each other or an
 * input (they may interleave, e.g. as views of one packed buffer).  The torch operators (upp_hip/ops.py xattn_fwd / xattn_bwd) check both.
 * Every output element is written by exactly one workgroup: no atomics, no workspace, no memset; two calls give the same bits.  Keys
 * >= Lk contribute exactly 0; rows >= Lq / Lk of an array are never read and never written.  With Lk <= 64 the softmax-backward row
 * sum is taken over the key block's own P dP (so a single key gives d_q = d_k = 0 exactly), otherwise it is sum_c d_ctx ctx. */
int upp_xattn_fwd(const float *q, const float *k, const float *v, float *ctx, float *lse,
                  int B, int Lq, int Lk, int H, int head_dim,
                  long long q_rs, long long k_rs, long long v_rs, float scale, void *stream);
int upp_xattn_bwd(const float *q, const float *k, const float *v, const float *ctx, const float *d_ctx, const float *lse,
                  float *d_q, float *d_k, float *d_v,
                  int B, int Lq, int Lk, int H, int head_dim,
                  long long q_rs, long long k_rs, long long v_rs,
                  long long dq_rs, long long dk_rs, long long dv_rs, float scale, void *stream);
/* ---- denoising-query attention: cross-attention under a prefix-visibility mask --------------
 * The masked self-attention of AdaPoinTr's decoder in training (reference models/AdaPoinTr.py:217-229, Attention.forward(x, mask) at
 * models/Transformer_utils.py:100-120: masked_fill(-finfo.max) before the softmax); csrc/attn_stream.hip.  Operands, strides, layouts,
 * refusals and the caller's duties are those of upp_xattn_fwd / upp_xattn_bwd ("Stride rule" above).  Two integers are added:
 *   query rows i <  split_q see the keys j < split_k;   query rows i >= split_q see all Lk keys.
 * AdaPoinTr: Lq = Lk = L, split_q = split_k = L - D for D denoising queries, q / k / v views of one packed qkv.
 * Checked before any launch, after the checks of upp_xattn_*: 0 <= split_q <= Lq and 1 <= split_k <= Lk, else UPP_E_BADARG.
 * A hidden key takes no part: its probability is the constant 0, set by a select on the indices and not by arithmetic on its score, so a
 * NaN in a hidden k row leaves ctx and lse of the rows that cannot see it untouched (in f32 the reference's masked_fill gives the same
 * exact 0, split_k >= 1 leaving every row a visible key).  lse is the log-sum-exp over the visible keys.  Nothing is promised for a
 * non-finite hidden v row or for the gradients next to one (0 * NaN, as in the reference).
 * Rows < split_q of ctx / lse carry the bits of upp_xattn_fwd on the first split_k keys, rows >= split_q those of upp_xattn_fwd on all
 * keys; with split_q == 0 or split_k == Lk forward and backward give the bits of upp_xattn_fwd / upp_xattn_bwd.
 * The mask shortens the walks: a query block wholly below split_q stops at the key block holding split_k - 1, a key block wholly at or
 * beyond split_k starts at the query block holding split_q.  The single-key-block backward form (the row sum over the block's own P dP,
 * visible keys only) is taken for every 64-row query block whose rows see one key block: Lk <= 64, or a block wholly below split_q when
 * split_k <= 64; there a row that sees one key gives d_q = d_k = 0 exactly.  One workgroup per output element: no atomics, no workspace,
 * no memset. */
int upp_xattn_prefix_fwd(const float *q, const float *k, const float *v, float *ctx, float *lse,
                         int B, int Lq, int Lk, int H, int head_dim,
                         long long q_rs, long long k_rs, long long v_rs, float scale, int split_q, int split_k, void *stream);
int upp_xattn_prefix_bwd(const float *q, const float *k, const float *v, const float *ctx, const float *d_ctx, const float *lse,
                         float *d_q, float *d_k, float *d_v,
                         int B, int Lq, int Lk, int H, int head_dim,
                         long long q_rs, long long k_rs, long long v_rs,
                         long long dq_rs, long long dk_rs, long long dv_rs, float scale, int split_q, int split_k, void *stream);
/* ---- prompt propagation (Block.forward, reference models/Point_MAE_pretask_dev.py:275-303) ----
 * X (rows, D): the block's token matrix viewed as rows = B*L' rows [cls | prompts | T centre tokens] per sample.
 * Index arguments are ABSOLUTE row numbers of X (the host converts the reference's flat / per-sample index
 * conventions, including its stride-64-into-stride-74 addressing when gather_idx is False).
 *   upp_prop_pool_fwd : pooled[g] = max_k v + mean_k v over v_k = X[i1[g*8+k]] * (1 + s_g), s_g = floor(keep+u[g])/keep
 *                       (u NULL: s = 1, i.e. eval-mode `x + drop_path(x)` = 2x); amax (groups, D) uint8 = arg max k.
 *                       (`pooling` is undefined in the reference: SURVEY D.3 assumption; BatchNorm is applied by the caller.)
 *   upp_prop_pool_bwd : g_X (rows, D), fully written (zeros where no group references a row).
 *   upp_prop_interp_fwd: out[b,t] = X[b,t] (+ 0.3 * sum_k w8[b,i,k] * (lc[b,j] + 0.3 * X[i2[b*G2+j]]), j = idx8[b,i,k])
 *                       for the last T rows (i = t - (L'-T)); `propagate(..., de_neighbors=8)` of models/Point_MAE_unify.py:22-48
 *                       with idx8 / w8 (B,T,8) precomputed once per forward from the centres.
 *   upp_prop_interp_bwd: g_c2 (B*G2, D) = gradient w.r.t. lc; g_X (rows, D) = g_out + 0.3 * g_c2 scattered to rows i2.
 * Limits: D <= 512; 8 neighbours per group / per interpolation. */
int upp_prop_pool_fwd(const float *X, const int32_t *i1, const float *u, float keep, float *pooled, uint8_t *amax,
                      int groups, int D, void *stream);
int upp_prop_pool_bwd(const float *g_pooled, const uint8_t *amax, const int32_t *i1, const float *u, float keep,
                      float *g_X, int rows, int groups, int D, void *stream);
int upp_prop_interp_fwd(const float *X, const float *lc, const int32_t *i2, const int32_t *idx8, const float *w8,
                        float *out, int B, int Lp, int T, int G2, int D, void *stream);
int upp_prop_interp_bwd(const float *g_out, const int32_t *i2, const int32_t *idx8, const float *w8, float *g_c2,
                        float *g_X, int B, int Lp, int T, int G2, int D, void *stream);

/* ---- fused propagation step: pool -> BatchNorm1d(bnorm) -> interpolate, CSR-driven backward ----
 * Same mathematics as upp_prop_pool_fwd -> BatchNorm1d over the B*G2 pooled rows (Block.bnorm, reference
 * models/Point_MAE_pretask_dev.py:275-303 + SURVEY D.3) -> upp_prop_interp_fwd, as 3 launches forward and 3 backward.
 *   upp_csr_build : stable inverse of an index list.  key(q) = (q / seg_len) * seg_rows + keys[q] (seg_rows = 0: absolute
 *                   keys); start (rows+1), perm (n): perm[start[r] .. start[r+1]) = ascending positions q with key(q) == r.
 *                   Keys outside [0, rows) are skipped.  rows <= 15360.  The three lists of a forward are inverted once:
 *                   csr1 = (i1; n = groups*8; rows = B*L'), csr2 = (i2; n = groups; rows = B*L'),
 *                   csr8 = (idx8; n = B*T*8, seg_len = T*8, seg_rows = G2; rows = groups).
 *   upp_prop_fwd  : pooled (groups, D) pre-BatchNorm rows, amax (groups, D) uint8, mean / rstd (D) batch statistics (training)
 *                   or running statistics (training == 0), out (B*L', D).  training != 0 updates running_mean / running_var
 *                   (momentum; unbiased variance) when they are non-NULL.  part: upp_prop_part_floats(groups, D) floats.
 *   upp_prop_bwd  : g_X (B*L', D) complete input gradient (identity + i2 scatter + BatchNorm/pool backward), g_gamma / g_beta (D)
 *                   BatchNorm parameter gradients; g_c2 (groups, D) and part are scratch.
 * Column partials are combined in a fixed order (Chan's update in f64 for the variance): deterministic. */
int upp_csr_build(const int32_t *keys, int n, int seg_len, int seg_rows, int rows, int32_t *start, int32_t *perm, void *stream);
/* upp_prop_index: the four index lists of upp_prop_fwd for one forward in one launch.  c1 (B,T,3) level-1 centres, c2 (B,G2,3)
 * level-2 centres; i1 (B*G2*8) / i2 (B*G2) int64 as Group hands them on (reference models/Point_MAE_unify.py:73-79: flat with
 * batch offsets when gather_idx == 0, per-sample otherwise); L' rows per sample, `off` leading rows (cls) excluded.
 * -> i1a, i2a absolute rows (the stride-T-into-stride-(L'-off) re-interpretation of Point_MAE_pretask_dev.py:291-292 when
 * gather_idx == 0); idx8 / w8 (B,T,8): 8 nearest level-2 centres by the reference's square_distance form, ascending
 * (distance, index), weights (1/(d+eps)) / sum (propagate, models/Point_MAE_unify.py:22-48).  G2 <= 64. */
int upp_prop_index(const float *c1, const float *c2, const int64_t *i1, const int64_t *i2, int gather_idx, int B, int T, int G2,
                   int Lp, int off, float eps, int32_t *i1a, int32_t *i2a, int32_t *idx8, float *w8, void *stream);
long long upp_prop_part_floats(int groups, int D);
int upp_prop_fwd(const float *X, const int32_t *i1, const float *u, float keep, const int32_t *i2, const int32_t *idx8,
                 const float *w8, const float *gamma, const float *beta, float *running_mean, float *running_var,
                 float momentum, float eps, int training, float *pooled, uint8_t *amax, float *part, float *mean,
                 float *rstd, float *out, int B, int Lp, int T, int G2, int D, void *stream);
int upp_prop_bwd(const float *g_out, const float *pooled, const uint8_t *amax, const float *mean, const float *rstd,
                 const float *gamma, const float *u, float keep, const float *w8, const int32_t *start1,
                 const int32_t *perm1, const int32_t *start2, const int32_t *perm2, const int32_t *start8,
                 const int32_t *perm8, int training, float *g_c2, float *part, float *g_gamma, float *g_beta, float *g_X,
                 int B, int Lp, int T, int G2, int D, void *stream);
/* The step of a prompted block with the MLP residual folded in: X is never stored, each of its rows is formed where it is read as
 *   x3[r] = x2[r] + dp_scale(u_dp[r / Lp]) * (m[r] + mbias)        (upp_rowln_fwd without a LayerNorm; mbias, u_dp may be NULL)
 *   upp_prop_res_pool_fwd : the first two launches of upp_prop_fwd on those rows (pooled, amax, part, mean, rstd as there); the third
 *                           is upp_ln_adapter_prop_fwd, the block's tail with the interpolation as its row phase.
 *   upp_prop_res_bwd      : upp_prop_bwd writing g_x2 = g_X and g_m = dp_scale * g_X (upp_rowln_bwd of the residual) instead of g_X.
 * Every result is bit-identical to the composition with upp_rowln_fwd / upp_rowln_bwd. */
int upp_prop_res_pool_fwd(const float *x2, const float *m, const float *mbias, const float *u_dp, float keep_dp, const int32_t *i1,
                          const float *u, float keep, float *running_mean, float *running_var, float momentum, float eps,
                          int training, float *pooled, uint8_t *amax, float *part, float *mean, float *rstd, int B, int Lp, int G2,
                          int D, void *stream);
int upp_prop_res_bwd(const float *g_out, const float *pooled, const uint8_t *amax, const float *mean, const float *rstd,
                     const float *gamma, const float *u, float keep, const float *w8, const int32_t *start1,
                     const int32_t *perm1, const int32_t *start2, const int32_t *perm2, const int32_t *start8,
                     const int32_t *perm8, int training, const float *u_dp, float keep_dp, float *g_c2, float *part,
                     float *g_gamma, float *g_beta, float *g_x2, float *g_m, int B, int Lp, int T, int G2, int D, void *stream);
/* Stage 2 of the recipe (run.sh:16, models/Point_MAE_unify.py:22-48 under autograd): the centres carry a gradient, so the
 * interpolation weights w8 do too.
 *   upp_prop_w8_grad    : g_w8 (B,T,8) = 0.3 * <g_out[token], lc[j] + 0.3 * X[i2[j]]>, j = idx8[token,k]; lc = BatchNorm(pooled) when
 *                         mean / rstd / gamma / beta are given (the tensors upp_prop_fwd saved), `pooled` itself when mean == NULL.
 *   upp_prop_weights_bwd: g_c1 (B,T,3), g_c2 (B,G2,3) from g_w8 through w = (1/(d+eps)) / sum, d = the reference's square_distance
 *                         form (models/modules.py:13-32); idx8 is a constant of the forward.  Fixed summation order, no atomics. */
int upp_prop_w8_grad(const float *g_out, const float *X, const float *pooled, const float *mean, const float *rstd,
                     const float *gamma, const float *beta, const int32_t *i2, const int32_t *idx8, float *g_w8, int B, int Lp,
                     int T, int G2, int D, void *stream);
int upp_prop_weights_bwd(const float *c1, const float *c2, const int32_t *idx8, const float *g_w8, float eps, float *g_c1,
                         float *g_c2, int B, int T, int G2, void *stream);

/* ---- row operators of the prompter branches and the per-point heads ---------------------------------
 * Replace the element-wise / reduction chains of the reference's rectify prompter
 * (models/Point_MAE_pretask_dev.py:22-52 PositionalEmbedding, :386-473 set abstraction / feature propagation):
 *   upp_bn_rows_fwd : y (R,C) = BatchNorm over the R rows of the channels-last matrix x (== BatchNorm1d/2d on the
 *                     reference's (B,C,N[,k]) layout), optional ReLU.  training != 0: batch statistics, running
 *                     statistics updated (momentum, unbiased variance) when non-NULL; training == 0: running
 *                     statistics.  gamma / beta may be NULL (1 / 0).  mean, rstd (C) are outputs; part:
 *                     upp_bn_rows_part_floats(R, C) floats of scratch.  Deterministic (fixed combination order).
 *   upp_bn_rows_bwd : backward of the training-mode form (batch statistics), for the trainable BatchNorm1d layers of the
 *                     per-point heads (models/Point_MAE_unify_segment.py seg_head / propagation_0, the patch embedding in
 *                     pre-training): x, g (R,C), mean / rstd from the forward; with xh = (x-mean)*rstd and
 *                     gm = g * [xh*gamma+beta > 0] (relu != 0; gm = g otherwise):  g_beta = sum gm, g_gamma = sum gm*xh,
 *                     g_x = gamma*rstd*(gm - (g_beta + xh*g_gamma)/R).  g_x may be NULL (parameter gradients only).
 *   upp_bn_rows_drop_fwd / _bwd (round 6): the training-mode pair with nn.Dropout(p) applied to the output in the same passes (the
 *                     segmentation head's `Conv1d, BatchNorm1d, ReLU, Dropout(0.5)`, reference models/Point_MAE_unify_segment.py:424-427):
 *                     y = dropout(relu?(bn(x))), kept values scaled by 1 / (1 - p).  The mask of element i is a counter-based hash of
 *                     (*seed + seed_add, salt, i) recomputed by the backward (no mask is stored; no uniform tensor is read): `seed` is
 *                     a DEVICE int64 whose value changes once per forward -- derived from the layer's own num_batches_tracked -- so steps
 *                     differ.  Backward and forward must be handed the same value of *seed + seed_add: the Python layer snapshots
 *                     counter + 1 (a host that bumps its counters at the end of the forward) or the counter into a tensor of its own
 *                     and passes it to both with seed_add 0, so the live counter may move any number of times in between.
 *                     0 <= p < 1 (p = 0: the plain pair).
 *                     The stream of masks is this library's (not torch's Philox).
 *   upp_sqdist_topk : dist / idx (B,N,k) = the k nearest of the S points src[b] for every query q[b,n], by the reference's
 *                     square_distance form d = |a|^2 + |b|^2 - 2 a.b (models/modules.py:13-32), ascending (d, index):
 *                     `square_distance(q, src).sort(dim=-1)` cut to k columns.  S <= 256, k <= min(S, 64).
 *   upp_interp_fwd  : out[b*N+n][col0 .. col0+C) = sum_{j<k} w_j feat[b][idx[b,n,j]],  w_j = (1/(d_j+eps)) / sum_j(1/(d_j+eps)),
 *                     where (dist, idx) (B*N rows, row stride ld_tab, idx int64) is a neighbour table sorted by distance
 *                     (torch.sort of square_distance, as the reference computes it); feat (B,S,C); k <= 16.
 *   upp_interp_affine_fwd : the same interpolation into a dense (B*N, C) matrix plus a rank-3 term,
 *                     out[row][c] = sum_j w_j feat[..][c] + x3[row][0] wt[0][c] + x3[row][1] wt[1][c] + x3[row][2] wt[2][c],
 *                     x3 (B*N,3), wt (3,C): the first 1x1 convolution of PointNetFeaturePropagation (reference
 *                     models/Point_MAE_pretask_dev.py:463-470) commuted with the interpolation -- feat then holds
 *                     W_x . points2 + b per source row and wt the xyz columns of the weight.  k <= 4, C >= 256, C % 4 == 0.
 *   upp_interp_bwd  : g_feat (B,S,C) = gradient of the above w.r.t. feat for g_out (B*N rows, row stride ld_g, columns
 *                     [col0, col0+C)); the neighbour table is a constant.  Deterministic (no atomics).  N <= 4096.
 *   upp_posenc_fwd  : out[row][col0 ..) = (x, sin(f_0 x), cos(f_0 x), ..., sin(f_{F-1} x), cos(f_{F-1} x)), x (rows,3);
 *                     freqs is a HOST array of F <= 8 frequencies.
 * interp / posenc write a column window of a row-major buffer with row stride ld_out (the reference's torch.cat). */
long long upp_bn_rows_part_floats(int R, int C);
int upp_bn_rows_fwd(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                    float momentum, float eps, int training, int relu, float *part, float *mean, float *rstd, float *y,
                    int R, int C, void *stream);
int upp_bn_rows_bwd(const float *x, const float *g, const float *mean, const float *rstd, const float *gamma, const float *beta,
                    int relu, float *part, float *g_gamma, float *g_beta, float *g_x, int R, int C, void *stream);
int upp_bn_rows_drop_fwd(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                         float momentum, float eps, int relu, float p, const long long *seed, long long seed_add, unsigned salt, float *part,
                         float *mean, float *rstd, float *y, int R, int C, void *stream);
int upp_bn_rows_drop_bwd(const float *x, const float *g, const float *mean, const float *rstd, const float *gamma, const float *beta,
                         int relu, float p, const long long *seed, long long seed_add, unsigned salt, float *part, float *g_gamma, float *g_beta,
                         float *g_x, int R, int C, void *stream);
int upp_sqdist_topk(const float *q, const float *src, float *dist, int64_t *idx, int B, int N, int S, int k, void *stream);
int upp_interp_fwd(const float *dist, const int64_t *idx, int ld_tab, const float *feat, float *out, int ld_out, int col0,
                   int B, int N, int S, int C, int k, float eps, void *stream);
int upp_interp_affine_fwd(const float *dist, const int64_t *idx, int ld_tab, const float *feat, const float *x3, const float *wt,
                          float *out, int B, int N, int S, int C, int k, float eps, void *stream);
int upp_interp_bwd(const float *dist, const int64_t *idx, int ld_tab, const float *g_out, int ld_g, int col0, float *g_feat,
                   int B, int N, int S, int C, int k, float eps, void *stream);
/* upp_interp_geo_bwd: gradient of upp_interp_fwd w.r.t. the GEOMETRY -- the queries xyz1 (B,N,3) and the sources xyz2 (B,S,3) behind the
 * squared distances of the neighbour table (d_j = |x1 - x2_j|^2, reference models/modules.py:13-32; the autograd chain of
 * models/Point_MAE_unify.py:22-48 / models/Point_MAE_pretask_dev.py:446-470 when the prompters train: stage 2, the pre-task recipe).
 * g_xyz1 (B,N,3) and / or g_xyz2 (B,S,3) are written (either may be NULL); contrib: (B*N, k, 3) floats of scratch, needed with g_xyz2
 * (the source-side terms are summed per source point in (row, j) order: deterministic).  k <= 16, k <= S. */
int upp_interp_geo_bwd(const float *dist, const int64_t *idx, int ld_tab, const float *feat, const float *g_out, int ld_g, int col0,
                       const float *xyz1, const float *xyz2, int B, int N, int S, int C, int k, float eps, float *g_xyz1,
                       float *g_xyz2, float *contrib, void *stream);
int upp_posenc_fwd(const float *x, const float *freqs, int F, float *out, int ld_out, int col0, long long rows, void *stream);

/* ---- classification tail (reference models/Point_MAE_unify.py:650-655 and get_loss_acc :499-503) ----------------
 *   upp_cls_pool_fwd : h = LayerNorm(x) (B,L,D) with gamma / beta / eps (self.norm); feat (B,2D) = [h[:,0] | max over rows 1..L-1 of h]
 *                      (first maximum); amax (B,D) int32 = the arg-max row; mean / rstd (B*L) saved.  h itself is not stored.
 *   upp_cls_pool_bwd : g_x (B,L,D) from g_feat (B,2D) (dense: every row is written).  gamma / beta gradients are not
 *                      produced (self.norm is frozen under PEFT; upp_cls_pool_bwd_ln below produces them when it trains).
 *   upp_ce_acc       : out2[0] = mean cross-entropy of logits (B,C) against labels (B) int64, out2[1] = top-1 accuracy * 100,
 *                      dlogits (B,C) = (softmax - onehot) / B.  C <= 512.  Deterministic. */
int upp_cls_pool_fwd(const float *x, const float *gamma, const float *beta, float eps, float *feat, int32_t *amax, float *mean,
                     float *rstd, int B, int L, int D, void *stream);
int upp_cls_pool_bwd(const float *g_feat, const float *x, const float *mean, const float *rstd, const float *gamma,
                     const int32_t *amax, float *g_x, int B, int L, int D, void *stream);
int upp_ce_acc(const float *logits, const int64_t *labels, float *out2, float *dlogits, int B, int C, void *stream);
/* ---- LayerNorm + token pooling with parameter gradients: the full fine-tuning models (csrc/norm_pool.hip) ---------------
 * Reference models/Point_MAE_cp.py:582-587 (PointTransformer: a trainable self.norm in front of [cls | max]) and
 * models/Point_MAE_segment.py:413-424 (PointTransformer_seg: one shared trainable self.norm on the outputs of blocks 3 / 7 / 11, their
 * concatenation, its max and mean over the tokens).  Every sum has an order fixed by the sizes; no atomics, no memset; every output
 * element is written by a kernel; arguments are checked before the first launch (UPP_E_BADARG: null pointer / size < 1, L < 2;
 * UPP_E_RANGE: outside the served range).
 *   upp_cls_pool_bwd_ln : upp_cls_pool_bwd (the same kernel: g_x has its bits) + g_gamma (D), g_beta (D).  With g_h[b][0][d] =
 *                         g_feat[b][d] and g_h[b][amax[b][d]][d] += g_feat[b][D + d]:  g_beta[d] = sum g_h,  g_gamma[d] = sum g_h * xhat
 *                         (acc = fma(g_h, xhat, acc)), xhat = (x - mean) * rstd from the saved statistics, both over (b, l) ascending and
 *                         over the 2 B rows that carry a gradient only.  Two launches.  D <= 512.
 *   upp_tap_pool_fwd    : f0, f1, f2 (B,G,C) -> x (B,G,3C) = [LN(f0) | LN(f1) | LN(f2)] (the bits of upp_rowln_fwd per row), gmax (B,3C) =
 *                         max over g of x, arg (B,3C) int32 = the LOWEST g that attains it, gmean (B,3C) = (((x[0] + x[1]) + x[2]) + ...) /
 *                         float(G) (f32, g ascending, one rounded addition at a time, one division), mean / rstd (B,G,3).  NaN: as
 *                         upp_group_max_fwd and upp_cls_pool_fwd (torch.max over a dimension) -- a NaN beats every number, the first NaN
 *                         of a column is its maximum, and it stays in its own row's tap (LayerNorm) and its own column (pooling).  One launch.
 *   upp_tap_pool_bwd    : t = (d_x + d_gmean / float(G)) + (g == arg ? d_gmax : 0) per element, then the row-LayerNorm backward of
 *                         upp_rowln_bwd per (row, tap) -> d_f0, d_f1, d_f2 (B,G,C);  d_gamma / d_beta (C): per row the three taps' terms
 *                         t * xhat / t added in tap order, rows (b, g) ascending in groups of 4 ((r0 + r1) + (r2 + r3)) into `part`,
 *                         the ceil(B G / 4) partials in 16 consecutive runs, each ascending, the run sums ascending.  `part`:
 *                         upp_tap_pool_part_floats(B, G, C) floats of scratch (0: sizes not served).  Two launches.
 *   Served: 1 <= B <= 65535, 1 <= G <= UPP_ATTN_MAX_L, C % 4 == 0, 4 <= C <= 512; exactly three taps. */
int upp_cls_pool_bwd_ln(const float *g_feat, const float *x, const float *mean, const float *rstd, const float *gamma,
                        const int32_t *amax, float *g_x, float *g_gamma, float *g_beta, int B, int L, int D, void *stream);
int upp_tap_pool_fwd(const float *f0, const float *f1, const float *f2, const float *gamma, const float *beta, float eps,
                     float *x, float *gmax, int32_t *arg, float *gmean, float *mean, float *rstd, int B, int G, int C, void *stream);
long long upp_tap_pool_part_floats(int B, int G, int C);
int upp_tap_pool_bwd(const float *d_x, const float *d_gmax, const float *d_gmean, const float *f0, const float *f1, const float *f2,
                     const float *mean, const float *rstd, const float *gamma, const int32_t *arg, float *part, float *d_f0,
                     float *d_f1, float *d_f2, float *d_gamma, float *d_beta, int B, int G, int C, void *stream);
/* ---- per-point log-softmax + NLL of the segmentation head (round 6) ---------------------------------------------------
 * Replaces `F.log_softmax(x, dim=-1)` (reference models/Point_MAE_unify_segment.py:433) and `F.nll_loss(pred, target)`
 * (:20-25 get_loss) over R = B * N point rows of C <= 64 classes, and the torch glue around them (gather, mean, neg, div, zero-fill +
 * scatter_add, zero-fill + copy of a column slice's backward):
 *   upp_logsoftmax_rows_fwd : logp (R,C) = log_softmax over c of y[r * ld_y + c] + bias[c] (bias NULL: none).  ld_y >= C: the rows may
 *                             be wider than C (the 50-class layer's GEMM writes a 52-column matrix).
 *   upp_logsoftmax_rows_bwd : g_y[r * ld_gy + c] = g_logp[r][c] - exp(logp[r][c]) * sum_c g_logp[r][c] for c < C and 0 for
 *                             C <= c < Cpad <= ld_gy: the gradient in the producing GEMM's padded layout, every element written once.
 *   upp_nll_mean_fwd        : out[0] = -(1 / R) sum_r logp[r][target[r]] (targets outside [0, C) contribute 0); `part`:
 *                             upp_nll_mean_part_floats(R) floats of scratch; two launches, sums in a fixed order (deterministic).
 *   upp_nll_mean_bwd        : g_logp (R,C) = -g_loss[0] / R at (r, target[r]), 0 elsewhere; g_loss a DEVICE scalar. */
int upp_logsoftmax_rows_fwd(const float *y, long long ld_y, const float *bias, long long R, int C, float *logp, void *stream);
int upp_logsoftmax_rows_bwd(const float *g_logp, const float *logp, long long R, int C, float *g_y, long long ld_gy, int Cpad, void *stream);
long long upp_nll_mean_part_floats(long long R);
int upp_nll_mean_fwd(const float *logp, const int64_t *target, long long R, int C, float *part, float *out, void *stream);
int upp_nll_mean_bwd(const float *g_loss, const int64_t *target, long long R, int C, float *g_logp, void *stream);
/* ---- noise-vector supervision of the pre-task recipe (round 6) -------------------------------------------------------
 * Replaces reference models/Point_MAE_pretask_dev.py:685-692 for a 3-channel rectify prompter:
 *   loss = mean_{b, noise i} |pred_noise - noise_vector|^2 + mean_{b, shape i} |pred_pure|^2,   score = |pred|
 * (`torch.mean(torch.norm(x, 2, dim=-1, keepdim=True) ** 2)` twice and `torch.norm(pred, dim=-1)`: ~30 element-wise launches with the
 * zero guards of norm's backward) where pred (B,P,3) holds pn shape points then P - pn noise points per cloud and noise_vector is
 * (B, P - pn, 3).  upp_noise_loss_fwd: loss[0], score (B,P) or NULL, `part` upp_noise_loss_part_floats(B, P) floats of scratch; two launches,
 * fixed-order sums.  upp_noise_loss_bwd: g_pred (B,P,3) = g_loss[0] * d loss / d pred (g_loss a device scalar), every element written. */
long long upp_noise_loss_part_floats(int B, int P);
int upp_noise_loss_fwd(const float *pred, const float *noise_vector, int B, int P, int pn, float *part, float *loss, float *score, void *stream);
int upp_noise_loss_bwd(const float *g_loss, const float *pred, const float *noise_vector, int B, int P, int pn, float *g_pred, void *stream);
/*   upp_bn_relu_drop_fwd / bwd : BatchNorm1d + ReLU + Dropout of a (R, C) matrix with few rows (the Linear outputs of
 *                      cls_head_finetune, R = batch size), one launch each way.  training != 0: batch statistics (mean / rstd
 *                      outputs, running statistics updated with momentum / unbiased variance when non-NULL); else running
 *                      statistics.  u (R,C) uniforms or NULL (no dropout): kept where u >= p, scaled by 1/(1-p).
 *                      Backward recomputes the ReLU / dropout masks from z and u; g_gamma / g_beta (C) are complete sums. */
int upp_bn_relu_drop_fwd(const float *z, const float *gamma, const float *beta, float *running_mean, float *running_var,
                         float momentum, float eps, int training, const float *u, float p, float *a, float *mean, float *rstd,
                         int R, int C, void *stream);
int upp_bn_relu_drop_bwd(const float *g_a, const float *z, const float *gamma, const float *beta, const float *mean,
                         const float *rstd, int training, const float *u, float p, float *g_z, float *g_gamma, float *g_beta,
                         int R, int C, void *stream);

/* ---- training step tail: gradient clipping + AdamW on flat buffers ------------------------
 * Replaces torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.AdamW.step() of the reference loop
 * (tools/runner_module.py:202-207; parameter groups of tools/builder.py:40-55) for parameters that live in one
 * flat buffer: p, g, m (exp_avg), v (exp_avg_sq) all (n) f32; elements [0, split) have weight decay 0,
 * [split, n) have `weight_decay`.  state (8 floats, zero-initialised once): [0] step count, [1] gradient L2 norm,
 * [2] clip coefficient min(max_norm / (norm + 1e-6), 1), [3] 1 - beta1^step, [4] sqrt(1 - beta2^step).
 * g is overwritten with the clipped gradient (as clip_grad_norm_ does).  max_norm <= 0 disables clipping.
 * lr < 0: the learning rate and the weight decay are read from state[5] and state[6] on the device instead of the
 * by-value arguments -- a launch captured in a HIP graph then follows a learning-rate schedule (the reference steps
 * a CosineLRScheduler per epoch, tools/builder.py:67-75 / tools/runner_module.py:217-221) without being re-captured.
 * scratch: upp_adamw_scratch_floats() floats. */
long long upp_adamw_scratch_floats(void);
/* upp_batched_sum: for `jobs` independent jobs in one launch, dst_j[c] (+)= sum_{i < n_j} src_j[i * ld_j + c], c < len_j
 * (rows added in ascending order; accumulate_j != 0 adds to dst_j, else overwrites; jobs that name the same dst are
 * applied one after the other in submission order by the same workgroups: race-free and deterministic).  src / dst / n / len / ld /
 * accumulate are HOST arrays; the pointers in src / dst are device pointers.  Used for the parameter-gradient partials of
 * a backward pass (upp_adapter_bwd partials per workgroup, upp_ln_param_grad partials per chunk, upp_rowln_bwd per-sample
 * prompt gradients), summed straight into the flat gradient buffer after the pass.
 * dst_width / dst_pitch (ABI 5; HOST arrays, both NULL = every destination flat): dst_width_j > 0 makes destination j a WINDOW of
 * (len_j / dst_width_j) rows of dst_width_j floats, dst_pitch_j floats apart -- element c lives at dst_j[(c / w) * pitch + c % w]: the
 * weight gradient of a Linear layer applied to a column range of a wider weight (the segmentation head's first layer acts on
 * [per-point 1024 | per-sample 2432] columns of one (512, 3456) weight, reference models/Point_MAE_unify_segment.py:424-433) lands in
 * that range of the weight's gradient without a zero-fill, a strided copy and an add.  len_j % dst_width_j == 0. */
int upp_batched_sum(const float *const *src, float *const *dst, const int *n, const int *len, const int *ld,
                    const int *accumulate, const int *dst_width, const int *dst_pitch, int jobs, void *stream);
/* upp_copy_batched: dst_j[0 .. bytes_j) = src_j[0 .. bytes_j) for `count` non-overlapping device buffers in one launch (host arrays of
 * device pointers and byte counts): the hand-over state a pipelined training step passes from its front-end to its back-end. */
int upp_copy_batched(const void *const *src, void *const *dst, const long long *bytes, int count, void *stream);
/* upp_colsum_partials: dst (chunks, len)[ch][c] = sum of src[r][c] over the rows r of chunk ch (ceil(n / chunks) rows each, ascending):
 * first stage of the column sum of one very tall matrix -- the bias gradient of a trainable Linear / 1x1 Conv1d over the 65,536
 * point rows of the patch embedding (reference models/Point_MAE_unify.py:191-222 under autograd) -- the second stage is
 * upp_batched_sum over the `chunks` rows. */
int upp_colsum_partials(const float *src, long long ld, int n, int len, int chunks, float *dst, void *stream);
/* upp_wcolsum_partials: dst (chunks, W, len)[ch][w][c] = sum over the rows r of chunk ch of wts[r][w] * src[r][c] (W <= 4; every fourth
 * row per wavefront, wavefronts combined in order): the weight gradient x^T . g of a rank-W update y += x (rows, W) . wt (W, len) over
 * very many rows -- the xyz columns of the first feature-propagation layer of the segmentation head over its 65,536 label points
 * (reference models/Point_MAE_unify_segment.py:420,605 under autograd).  Second stage: sum over the chunks (upp_batched_sum).
 * Limits: len % 4 == 0, ld % 4 == 0, src and dst 16-byte aligned. */
int upp_wcolsum_partials(const float *src, long long ld, const float *wts, long long ldw, int W, int n, int len, int chunks,
                         float *dst, void *stream);
int upp_adamw_flat(float *p, float *g, float *m, float *v, long long n, long long split, float *state, float *scratch,
                   float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, void *stream);

/* ---- bottleneck adapter --------------------------------------------------------------------
 * Replaces Adapter.forward after its LayerNorm and the residual that applies it (reference
 * models/Point_MAE_pretask_dev.py:96-104 and :312-320):
 *   out = x + scale * ( W2 . dropout_p(gelu(W1 . ha + b1)) + b2 )        scale = 0.7, exact (erf) GELU
 *   ha, x, out (R, D); W1 (H, D), b1 (H), W2 (D, H), b2 (D); s1 (R, H) = W1 . ha + b1 is saved for backward;
 *   u (R, H) uniforms in [0,1) select the dropout mask (kept iff u >= p, scaled by 1/(1-p)); NULL = no dropout.
 * Backward: g_ha (R, D) and, per workgroup of 32 rows, partial sums [dW1 (H,D) | dW2 (D,H) | db1 (H) | db2 (D)] in
 * `part` (upp_adapter_part_floats(R, D) floats; the caller sums the workgroups).  The gradient w.r.t. x is g_out.
 * Limits: D == 384, H == 32. */
long long upp_adapter_part_floats(int R, int D);
int upp_adapter_fwd(const float *ha, const float *x, const float *W1, const float *b1, const float *W2, const float *b2,
                    const float *u, float p, float scale, float *out, float *s1, int R, int D, int H, void *stream);
int upp_adapter_bwd(const float *g_out, const float *ha, const float *s1, const float *W1, const float *W2, const float *u,
                    float p, float scale, float *g_ha, float *part, int R, int D, int H, void *stream);
/* upp_ln_adapter_fwd: the row operator that closes a block (residual + drop path, prompt strip, the adapter's LayerNorm:
 * upp_rowln_fwd with mode 0 / 3 / 4 and no `add`) and upp_adapter_fwd in ONE launch on 16-row workgroups; the LayerNorm
 * output is never written (reference models/Point_MAE_pretask_dev.py:305-320: `x = x + drop_path(mlp(norm2(x)))`, prompt
 * removal, `x = x + adapter(x)` with Adapter.forward :96-104).
 *   xo (B, Lout, D) = x[src(t)] + dp_scale(u_b) * (y[src(t)] + ybias)     (y, ybias, u may be NULL)
 *   mean, rstd (B, Lout): LayerNorm statistics of xo;  s1 (B*Lout, H);  out (B, Lout, D) = adapter(LayerNorm(xo), xo)
 *   ud (B*Lout, H): dropout uniforms of the adapter or NULL.  Rows and statistics are bit-identical to upp_rowln_fwd's.
 * upp_ln_adapter_bwd = upp_adapter_bwd with the LayerNorm output rebuilt from (xo, mean, rstd, gamma, beta) while the tile is
 * staged; the row operator's own backward stays upp_rowln_bwd (g_xo = g_out, g_h = g_ha). */
int upp_ln_adapter_fwd(const float *x, const float *y, const float *ybias, const float *u, float keep, int mode, int P,
                       const float *gamma, const float *beta, float eps, const float *W1, const float *b1, const float *W2,
                       const float *b2, const float *ud, float p, float scale, float *xo, float *mean, float *rstd, float *s1,
                       float *out, int B, int Lin, int Lout, int D, int H, void *stream);
/* upp_ln_adapter_prop_fwd: upp_ln_adapter_fwd for a prompted block with prompt propagation, on the inputs of the MLP residual
 * (x, y, ybias, u as there; y is required) and the tensors upp_prop_res_pool_fwd wrote.  The rows it normalises are
 *   xo[t] = x3[src(t)] + (src(t) a centre row i = src(t) - (Lin - T) >= 0 ? 0.3 * sum_k w8[i][k] * (BN(pooled[j_k]) + 0.3 * x3[i2[j_k]]) : 0)
 * with x3 as above, j_k = idx8[i][k], BN = bn_gamma * (. - bn_mean) * bn_rstd + bn_beta: the rows upp_prop_fwd writes, which are
 * neither stored nor -- the prompt rows -- computed.  Outputs as upp_ln_adapter_fwd, bit-identical to
 * upp_rowln_fwd -> upp_prop_fwd -> upp_ln_adapter_fwd(y = NULL).  The backward is upp_ln_adapter_bwd_fused -> upp_prop_res_bwd. */
int upp_ln_adapter_prop_fwd(const float *x, const float *y, const float *ybias, const float *u, float keep, int mode, int P,
                            const float *pooled, const float *bn_mean, const float *bn_rstd, const float *bn_gamma,
                            const float *bn_beta, const int32_t *i2, const int32_t *idx8, const float *w8, int T, int G2,
                            const float *gamma, const float *beta, float eps, const float *W1, const float *b1, const float *W2,
                            const float *b2, const float *ud, float p, float scale, float *xo, float *mean, float *rstd, float *s1,
                            float *out, int B, int Lin, int Lout, int D, int H, void *stream);
/* upp_ln_adapter_bwd_fused: the whole backward of upp_ln_adapter_fwd in one launch on 16-row workgroups -- the adapter's backward
 * (g_ha, per-workgroup partials [dW1 (H,D) | dW2 (D,H) | db1 (H) | db2 (D)] in `part`, upp_ln_adapter_part_floats(R, D) floats, or
 * part = NULL), the LayerNorm backward with the residual (g_x / g_y (B, Lin, D): every row is written, zeros for the prompt rows
 * the strip map dropped; either may be NULL), and the LayerNorm parameter-gradient partials (`ln_part`: [workgroup][2][D], or NULL).
 * Same results as upp_ln_adapter_bwd + upp_rowln_bwd up to f32 re-association of the small products. */
long long upp_ln_adapter_part_floats(int R, int D);
int upp_ln_adapter_bwd_fused(const float *g_out, const float *xo, const float *mean, const float *rstd, const float *gamma,
                             const float *beta, const float *s1, const float *W1, const float *W2, const float *ud, float p,
                             float scale, const float *u, float keep, int mode, int P, float *g_x, float *g_y, float *part,
                             float *ln_part, int B, int Lin, int Lout, int D, int H, void *stream);
int upp_ln_adapter_bwd(const float *g_out, const float *xo, const float *mean, const float *rstd, const float *gamma,
                       const float *beta, const float *s1, const float *W1, const float *W2, const float *u, float p,
                       float scale, float *g_ha, float *part, int R, int D, int H, void *stream);
/* The adapter weight gradients from their factors (round 6; reference: autograd through Adapter.forward,
 * models/Point_MAE_pretask_dev.py:96-104, for the trainable `downstream_adapter` of every block).  upp_ln_adapter_bwd_fused writes
 * 24,992 floats of partial results per 16-row workgroup (153 MB per headline step, summed by upp_batched_sum).
 * upp_ln_adapter_bwd_factors is the same launch with `fac` (B*Lout, 2 H) = [ga | d] per row instead of `part`:
 *   ga = gradient at the hidden pre-activation, d = scale * dropout(gelu(s1)).
 * upp_adapter_wgrad_batched then forms, in ONE launch for `jobs` blocks (any number; 16 per kernel launch),
 *   dW1 = sum_rows ga^T . LayerNorm(xo),  dW2 = sum_rows g_out^T . d,  db1 = sum_rows ga,  db2 = scale sum_rows g_out
 * over `splits` row ranges per block: part[j] = (splits, 2 H D + H + D) floats in the per-workgroup layout above, to be summed over
 * its rows (upp_batched_sum).  upp_adapter_wgrad_splits(R): the split count the host side uses (128 rows per split, at most 64).
 * D = 384, H = 32; xo / g_out / fac / gamma / beta 16-byte aligned.  Deterministic; the association of the row sum differs from the
 * per-workgroup form's. */
int upp_ln_adapter_bwd_factors(const float *g_out, const float *xo, const float *mean, const float *rstd, const float *gamma,
                               const float *beta, const float *s1, const float *W1, const float *W2, const float *ud, float p,
                               float scale, const float *u, float keep, int mode, int P, float *g_x, float *g_y, float *fac,
                               float *ln_part, int B, int Lin, int Lout, int D, int H, void *stream);
int upp_adapter_wgrad_splits(int R);
int upp_adapter_wgrad_batched(const float *const *xo, const float *const *mean, const float *const *rstd, const float *const *gamma,
                              const float *const *beta, const float *const *g_out, const float *const *fac, const int *R,
                              const float *scale, float *const *part, int jobs, int splits, int D, int H, void *stream);

/* ---- tail of the denoising prompter ---------------------------------------------------------
 * Replaces RectifyPrompter.score_head (reference models/Point_MAE_pretask_dev.py:491-493,512: Linear(32,64) -> ReLU -> Dropout(0.2)
 * -> Linear(64,3), times score_factor) and the selection that follows it in the model (models/Point_MAE_unify.py:553-559):
 *   pred = head(feature) * factor;  score = ||pred||_2;  order = argsort(score, descending, stable);
 *   moved = pts + nudge * pred;     out = moved[order[N - keep :]]            (reference: nudge 0.2, keep int(0.95 point_num))
 * feature (B*N,32) 16-byte aligned, W0 (64,32), b0 (64), W1 (3,64), b1 (3), u (B*N,64) uniforms in [0,1) or NULL (no dropout;
 * with u: hidden unit kept iff u >= p and scaled by 1 / (1 - p)), pts (B,N,3).
 * Outputs: moved (B,N,3), score (B,N) (both always written: scratch of the second launch), out (B,keep,3), pred (B,N,3) or NULL,
 * order (B,N) int64 or NULL (the full descending order; ties: lower index first).  Limits: N <= 16384. */
int upp_rectify_select(const float *feature, const float *W0, const float *b0, const float *W1, const float *b1, const float *u, float p,
                       float factor, const float *pts, float nudge, int B, int N, int keep, float *pred, float *moved, float *score,
                       float *out, int64_t *order, void *stream);

/* Stable argsort of every row of key (B,N) f32 by rank counting (no library sort): order (B,N) int64 with order[b][r] = the index of the
 * r-th element of row b in ascending (descending != 0: descending) order, equal keys in index order -- what torch.argsort(...,
 * stable=True) returns, and what torch.argsort returns for distinct keys.  NaN ranks ABOVE +inf (last ascending, first descending: torch.sort's order) and -0 equals +0; always a permutation.  Replaces the reference's device sorts of
 * short rows: torch.argsort(score, descending=True) of the pre-task noise recall (models/Point_MAE_pretask_dev.py:702-704), the masking
 * orders of Point-MAE pre-training (models/Point_MAE.py:300-329: argsort of uniform draws / of distances to a random centre, and the
 * visible-first order argsort(mask)).  Limits: N <= 16384 (the row lives in the LDS). */
int upp_argsort_rows(const float *key, int B, int N, int descending, int64_t *order, void *stream);

/* Max-pool over the k rows of every group with its arg-max, and the backward that writes the whole gradient in one pass (replaces
 * `x.max(dim)[0]` under autograd at the max-pool sites whose input carries a gradient -- reference models/Point_MAE_unify.py:205,221 (the
 * patch embedding when it trains: pre-training, stage 2), models/Point_MAE_pretask_dev.py:413 (set abstraction), :294 (`pooling`) -- where
 * torch launches a reduce forward and a zero-fill + scatter backward):
 *   x (R, k, C) -> out (R, C) = max_j x[r][j][c], amax (R, C) uint8 = the first j that attains it;  g_x (R, k, C) = g[r][c] at j = amax[r][c],
 *   0 elsewhere.  k <= 255, C % 4 == 0, x / out / g / g_x 16-byte and amax 4-byte aligned. */
int upp_group_max_fwd(const float *x, int R, int k, int C, float *out, unsigned char *amax, void *stream);
int upp_group_max_bwd(const float *g, const unsigned char *amax, int R, int k, int C, float *g_x, void *stream);

/* ---- vote-batched evaluation (upp_hip/infer.py EvalStep; reference tools/runner_module.py:427-490 `test_vote`, :383-413 `validate`) ----
 * upp_vote_points: out (V*B, N, 3), vote-major (row v*B + b) = superset[b][pick[v][i]] * scale[v][b] + shift[v][b] -- the V random
 *   subsets of the FPS-ordered superset (B,S,3), one pick (V,N) int32 per vote shared by the batch, each scale/translate-augmented
 *   (misc.scale_translate) in ONE launch.  scale / shift (V,B,3) may each be NULL (no multiply / no add: a plain gather).  The multiply
 *   and the add round separately, as torch's `pc * s + t` does: bit-identical to it.  A pick outside [0,S) yields a NaN point.
 * upp_vote_reduce: pred (B) int64 = the first arg-max over c of (sum_{v=0..V-1} logits[v*B + b][c]) / V (the sum in v order, then one
 *   division; NaN ranks above everything, as torch.max), and counters (2) int64 += (number of b < n_valid with pred[b] == labels[b],
 *   n_valid).  logits (V*B, C), labels (B) int64, 0 <= n_valid <= B (rows beyond n_valid: padding, predicted but not counted).  One
 *   workgroup: deterministic, no atomics, no memset (a captured graph keeps working from its second replay on).
 * Limits: V*B < 2^31; UPP_E_RANGE for n_valid outside [0,B]. */
int upp_vote_points(const float *superset, const int32_t *pick, const float *scale, const float *shift, float *out,
                    int B, int S, int N, int V, void *stream);
int upp_vote_reduce(const float *logits, const int64_t *labels, int V, int B, int C, int n_valid, int64_t *pred,
                    int64_t *counters, void *stream);

/* ---- part-segmentation metrics (utils/evaluate.py SegMetric; reference tools/runner_unify_seg.py:301-367 `validate`) ----
 * The part table is data: part_cat (P) int32 = the category of part l; cat_range (C, 2) int32 = [lo, n) of category c's contiguous parts.
 * upp_seg_iou_counts: logp (B, N, >= P) f32 with row stride ld >= P (element (b, n, l) at (b*N + n)*ld + l), target (B, N) int64.  The
 *   category of shape b is part_cat[target[b][0]]; pred[b][n] = lo + the first arg-max of logp[b][n][lo .. lo+n) (np.argmax: equal
 *   values -> the lower index, a NaN wins, the first NaN first); -1 for a shape whose target[b][0] is outside [0, P).  pred (B, N) int64
 *   may be NULL.  Shapes b < n_valid add their integer histograms into scratch (int32, 3 B P + 2 P + 1, zero on entry): per shape and
 *   part the intersection / predicted / target counts, per part the seen / correct counts, the correct points.  Integer atomics only:
 *   deterministic.  Shapes b >= n_valid (padding) get pred only.
 * upp_seg_iou_accumulate: one workgroup, after upp_seg_iou_counts with the same (scratch, target, table, B, N, P, C, n_valid).
 *   shape_iou (B) f64 = per shape b < n_valid the mean over its category's parts of IoU_l = |T_l & P_l| / |T_l | P_l| (1.0 when the
 *   part is in neither): a sequential float64 sum in part order, then one division (np.mean of fewer than 8 values, bit for bit);
 *   shape_cat (B) int32 its category (-1, IoU NaN: an invalid shape).  cat_sum (C) f64 += the IoUs per category in shape order, cat_cnt
 *   (C) int64 += the shape counts, part_seen / part_correct (P) int64 += the part counters, counters (3) int64 += (correct points,
 *   n_valid * N, invalid shapes).  Then the scratch is zeroed by the kernel (no memset node in a captured evaluation).
 * Limits: P <= 1024, C <= 256, B <= 65535, B*N < 2^31; UPP_E_RANGE for n_valid outside [0, B]. */
int upp_seg_iou_counts(const float *logp, long long ld, const int64_t *target, const int32_t *part_cat, const int32_t *cat_range,
                       int B, int N, int P, int C, int n_valid, int64_t *pred, int32_t *scratch, void *stream);
int upp_seg_iou_accumulate(int32_t *scratch, const int64_t *target, const int32_t *part_cat, const int32_t *cat_range, int B, int N,
                           int P, int C, int n_valid, double *shape_iou, int32_t *shape_cat, double *cat_sum, int64_t *cat_cnt,
                           int64_t *part_seen, int64_t *part_correct, int64_t *counters, void *stream);

/* ---- point-completion metrics (utils/evaluate.py CompletionMetric; reference tools/runner_pretask.py:314-426 `validate`,
 * utils/metrics.py:48-111 `Metrics.get`) ----
 * upp_completion_cloud_metrics: one workgroup per cloud pair b < B of xyz1 (B, n, 3) / xyz2 (B, m, 3) f32, with dist1 / idx1 (B, n) and
 *   dist2 / idx2 (B, m) of upp_chamfer_fwd on the same pair.  stats (B, 8) f64 = (mean d1, mean d2, mean sqrt d1, mean sqrt d2, F,
 *   CDL1, CDL2, 0): float64 sums in a fixed tree (bit-identical from run to run), one division each; CDL1 = (mean sqrt d1 + mean sqrt
 *   d2) / 2 and CDL2 = mean d1 + mean d2 (upp_completion_masked_cd replaces them for a flagged pair).  counts (B, 4) int32 =
 *   (precision count, recall count, has a zero-sum point, 0).  detail = 1: a point of xyz1 counts for the precision when the float64
 *   Euclidean distance to its Chamfer partner idx1 (recomputed from the f32 coordinates) is < th, a point of xyz2 likewise for the
 *   recall; F = 2 r p / (r + p) with p = count / n, r = count / m (0 when r + p = 0); the flag is set when a point of either cloud has
 *   the f32 sum (x + y) + z == 0.  detail = 0: F, the counts and the flag are 0.  th > 0 and finite.
 * upp_completion_masked_cd: after upp_completion_cloud_metrics with the same (xyz1, xyz2, B, n, m, counts, stats).  For every pair whose
 *   flag is set, CDL1 / CDL2 of stats are recomputed with every zero-sum point removed from both clouds first (a nearest-neighbour
 *   search on upp_chamfer_fwd's f32 arithmetic; the ignore_zeros rule of the reference's Chamfer modules at batch size 1); NaN when
 *   either cloud is left without points.  A workgroup whose flag is 0 reads it on the device and returns.
 * upp_completion_accumulate: one workgroup.  sparse / dense (V B, 8) f64 are stats rows, viewpoint-major (row v B + b).  For b <
 *   n_valid, then v < V, sequentially in float64: loss_sum (4) += 1000 x (sparse CDL1-form, sparse CDL2-form, dense CDL1-form, dense
 *   CDL2-form) of the unmasked means; counters (2) int64 += (n_valid V, V x the clouds whose category is outside [0, C)).  category (B)
 *   int64 may be NULL (no detail metrics); otherwise cat_sum (C, 3) f64 += (F, 1000 CDL1, 1000 CDL2) of the dense rows of category c
 *   and cat_cnt (C) int64 += their count.  The stats rows are written whole by every cloud-metrics launch: no scratch, no memset.
 * Limits: B (V B for accumulate) <= 2^20 rows, n, m <= 2^22, V <= 64, C <= 4096; UPP_E_RANGE for n_valid outside [0, B]. */
int upp_completion_cloud_metrics(const float *xyz1, const float *xyz2, const float *dist1, const int32_t *idx1, const float *dist2,
                                 const int32_t *idx2, int B, int n, int m, double th, int detail, double *stats, int32_t *counts,
                                 void *stream);
int upp_completion_masked_cd(const float *xyz1, const float *xyz2, int B, int n, int m, const int32_t *counts, double *stats,
                             void *stream);
int upp_completion_accumulate(const double *sparse, const double *dense, const int64_t *category, int V, int B, int C, int n_valid,
                              double *loss_sum, int64_t *counters, double *cat_sum, int64_t *cat_cnt, void *stream);

/* ---- token-matrix Linear (exact f32 on the matrix cores) -------------------------------------
 * Replaces the nn.Linear layers of the Transformer blocks and their data gradients: Attention.qkv / .proj
 * (reference models/Point_MAE_pretask_dev.py:178,181 called :186,:194) and Mlp.fc1 / .fc2 (:158,:160 called
 * :164-168), i.e. torch.nn.functional.linear -> cuBLAS in the reference.
 *   C (M,N) = epilogue( A (M,K) . W (N,K)^T )       A, W, C row-major with leading dimensions lda, ldw, ldc (floats)
 * f32 in, f32 accumulate on v_mfma_f32_32x32x2_f32: every output is a k-ordered chain of fused multiply-adds
 * (one rounding per product), the order of k being a fixed permutation inside each group of 32.
 * A data gradient dX = dY . W is the same call with W^T stored row-major: (A = dY, W = W^T (K,N), N <-> K).
 *   epilogue 0: none                      1: + bias[n]
 *            2: GELU(. + bias[n])         3: GELU(. + bias[n]), and aux (M,N; ldaux) receives GELU'(. + bias[n])
 *            5: ReLU(. + bias[n])
 *            4: . * aux[m][n]   (exact erf GELU, as nn.GELU; 3 / 4 make fc1 forward / fc2 data-gradient carry the
 *               activation and its backward, reference :165 `self.act`)
 *   tile: 0 = chosen by the library for (M,N,K) (upp_linear_tile returns that choice); else 4096*BMB + 256*BNB + 16*KS + KC
 *         forces workgroups of BMB x BNB blocks of 32 x 32 (one block per wave), the contraction split KS ways over wave
 *         groups and 32*KS*KC values of k per LDS stage -- one of the compiled shapes (csrc/linear.hip UPP_LIN_CONFIGS),
 *         anything else is UPP_E_RANGE; for measurements.  Codes with bit 16 set name the register-tiled shapes of
 *         csrc/linear_rt.hip (tall matrices: thousands of tiles): 0x1000000 NST + 0x100000 (4 (RM-1) + RN-1) + 0x10000 + 4096 WM +
 *         256 WN + 16 + KC = WM x WN waves of RM x RN blocks each, NST LDS stages of 32 KC values of k, no split of the
 *         contraction (the low byte reads KS = 1, KC: the summation order).
 * Limits: K % 4 == 0 (a k-stage holds 32 KS KC values of k; the last one reads zeros beyond K: exact), lda % 4 == 0, ldw % 4 == 0,
 * A and W 16-byte aligned. */
int upp_linear_tile(int M, int N, int K);
/* Weight gradients of trainable Linear layers (AddmmBackward's second GEMM in the reference: every nn.Linear / 1x1 Conv1d under
 * autograd -- models/Point_MAE_cp.py:369-465 in pre-training, models/Point_MAE_unify_segment.py:420-433 for the segmentation head):
 * dW_p (N_p,K_p) = G_p^T . X_p with G_p = dY (M_p,N_p) and X_p (M_p,K_p) row-major (leading dimensions ldg, ldx), for `count`
 * layers in ONE launch (a weight gradient is read by nothing inside the backward pass, so a step driver issues them together when
 * the pass is over).  The rows of problem p are cut into runs of rows[p] (a multiple of 32; upp_linear_wgrad_grouped_rows plans them
 * for a group: equal work units, about six rounds of the resident workgroups); partials[p] (ceil(M_p / rows[p]), N_p, K_p) receives
 * one partial dW per run -- every entry ONE ascending-row chain of fused multiply-adds -- and the caller sums the runs in order
 * (upp_batched_sum).  All array arguments are HOST arrays; G / X / partials hold device pointers.
 * upp_linear_wgrad_f32 / upp_linear_wgrad_splits: a group of one.
 * Limits: N % 4 == 0, K % 4 == 0, ldg % 4 == 0, ldx % 4 == 0, G, X and partials 16-byte aligned. */
int upp_linear_wgrad_grouped_rows(int count, const int *M, const int *N, const int *K, int *rows);
int upp_linear_wgrad_grouped_f32(const float *const *G, const long long *ldg, const float *const *X, const long long *ldx,
                                 float *const *partials, const int *M, const int *N, const int *K, const int *rows,
                                 int count, void *stream);
/* upp_linear_wgrad_grouped_sb (round 4): the same work list, limits and partial layout on the BF16 matrix pipe -- both operands split
 * into three bf16 terms inside the kernel, six products per pair as upp_linear_sb_f32 (error of an f32 GEMM against float64; each entry a
 * fixed-order sum, not bit-comparable with the f32 chain).  csrc/wgrad_sb.hip. */
int upp_linear_wgrad_grouped_sb_rows(int count, const int *M, const int *N, const int *K, int *rows);   /* its plan of rows[] (tile classes) */
int upp_linear_wgrad_grouped_sb(const float *const *G, const long long *ldg, const float *const *X, const long long *ldx,
                                float *const *partials, const int *M, const int *N, const int *K, const int *rows,
                                int count, void *stream);
int upp_linear_wgrad_splits(int M, int N, int K);
int upp_linear_wgrad_f32(const float *G, long long ldg, const float *X, long long ldx, float *partials,
                         int M, int N, int K, void *stream);
int upp_linear_f32(const float *A, long long lda, const float *W, long long ldw, const float *bias,
                   float *C, long long ldc, float *aux, long long ldaux,
                   int M, int N, int K, int epilogue, int tile, void *stream);
/* upp_linear_group_bias_f32: C = A . W^T + bias[m >> group_shift][:], bias a (ceil(M / 2^group_shift), N) matrix -- a bias per group of
 * 2^group_shift >= 32 consecutive rows in the GEMM's epilogue: `h + per_sample.unsqueeze(1)` of the segmentation head
 * (models/Point_MAE_unify_segment.py:424-433 with the concat's broadcast half multiplied once per sample) and the per-group half of the
 * patch embedding's Conv1d(512, 512) (models/Point_MAE_unify.py:213-216).  Tall problems only (the register-tiled kernel:
 * upp_linear_tile(M, N, K) & 0x10000), UPP_E_RANGE otherwise. */
int upp_linear_group_bias_f32(const float *A, long long lda, const float *W, long long ldw, const float *bias, int group_shift,
                              float *C, long long ldc, int M, int N, int K, void *stream);
/* ---- the same Linear layers at f32 accuracy on the BF16 matrix pipe (csrc/linear_sb.hip) ------------------------------
 * Replaces the same reference calls as upp_linear_f32 (models/Point_MAE_pretask_dev.py:153-196, nn.Linear -> cuBLAS) for FROZEN
 * weights: C (M,N) = epilogue( A (M,K) . W (N,K)^T ) with every f32 operand split exactly into three bf16 terms (x = x1 + x2 + x3,
 * round-to-nearest, both residuals exact) and the six products of weight >= 2^-16 accumulated in f32 by v_mfma_f32_32x32x16_bf16;
 * the dropped terms are below 2^-25 |a w|: the error against an exact product is that of an f32 GEMM (tests/test_gpu_linear_sb.py
 * measures both against float64), at 6/16 of the matrix-pipe time of v_mfma_f32_32x32x2_f32.  Not bit-pinned (the summation order
 * inside a bf16 MFMA is not documented): the exact-f32 kernel above stays the bit-pinned one.
 *   upp_linear_sb_planes_bytes(N, K): size of the plane image of a (N,K) weight (6 bytes per element, N and K rounded up to 32).
 *   upp_linear_sb_prep(W, ldw, N, K, transposed, planes): split the (N,K) weight operand once per weight version into the kernel's LDS image
 *       [32-row block][32-wide k-stage][plane 0..2][16-byte granule of 8 k][row] (zero beyond N, K); planes 16-byte aligned.  transposed != 0:
 *       the operand is the TRANSPOSE of the row-major (K,N) matrix at W (leading dimension ldw >= N) -- the B operand of a data gradient
 *       dX = dY . W read straight from W, no f32 copy of W^T.  upp_linear_sb_prep_batched: `count` weights in one launch (HOST arrays of
 *       device pointers / sizes): the trainable weights of a step driver, re-split at the start of every step.
 *   upp_linear_sb_tile(M, N, K): the tile code the library would take (hex digits 0x4 BMB BNB RN KS NST: workgroups of
 *       BMB x BNB blocks of 32 x 32, a wave owns 1 x RN of them, the contraction cut over KS wave groups, NST LDS stages of 32 KS values
 *       of k), or 0 when the problem is not one for this kernel (K % 32, fewer k-stages than LDS stages, no tile fits).  The choice is that
 *       of a cost model fitted to a measured sweep of every tile shape over the Linear problems of the six recipes (csrc/linear_sb_model.h,
 *       tools/micro/sb_model_fit.py, profiles/r05_sb_sweep.json: within 3 % of the measured best on 95 % of the problems, also of problems
 *       held out of the fit), behind a nine-row table of the swept problems where the model is still behind (csrc/linear_sb_tuned.h, exact
 *       (M, N, K) matches); option UPP_OPT_SB_TUNED = 0 leaves the model alone.  Any
 *       compiled tile code is valid for any problem whose K its wave groups' k-stages divide (a forced code: upp_linear_sb_f32's `tile`).
 *   upp_linear_sb_f32: epilogues and aux as upp_linear_f32; tile 0 = the library's choice.  Limits: K % 32 == 0 (% 64, % 128 for KS = 2, 4 tiles),
 *       N % 4 == 0, lda % 4 == 0, ldc % 4 == 0, ldaux % 4 == 0, A / C / bias / aux 16-byte aligned; UPP_E_RANGE otherwise (the caller
 *       then takes upp_linear_f32).
 *       Value range: the split is exact for finite operands up to the largest bf16 (|x| <= 0x7F7F0000 = 3.39e38); a finite weight beyond
 *       it counts as infinite (upp_linear_sb_prep zeroes its residual terms instead of forming inf - inf).
 *       Non-finite operands: x = +-inf splits into (inf, NaN, ...) in the loop and into (inf, 0, 0) in upp_linear_sb_prep; either way the
 *       six-product sum mixes +inf and -inf terms (the residual terms of the OTHER operand carry both signs), so every output a non-finite
 *       operand reaches is non-finite -- NaN where upp_linear_f32 yields +-inf.  Overflow still surfaces, its sign does not.
 *   upp_linear_sb_group_bias_f32: C = A . W^T + bias[m >> group_shift][:] (a bias per group of 2^group_shift >= 32 rows), the split-bf16
 *       form of upp_linear_group_bias_f32 (reference models/Point_MAE_unify_segment.py:424-433, models/Point_MAE_unify.py:213-216). */
int upp_linear_sb_tile(int M, int N, int K);
long long upp_linear_sb_planes_bytes(int N, int K);
int upp_linear_sb_prep(const float *W, long long ldw, int N, int K, int transposed, void *planes, void *stream);
int upp_linear_sb_prep_batched(const float *const *W, const long long *ldw, const int *N, const int *K, const int *transposed,
                               void *const *planes, int count, void *stream);
int upp_linear_sb_f32(const float *A, long long lda, const void *planes, const float *bias, float *C, long long ldc, float *aux,
                      long long ldaux, int M, int N, int K, int epilogue, int tile, void *stream);
int upp_linear_sb_group_bias_f32(const float *A, long long lda, const void *planes, const float *bias, int group_shift, float *C,
                                 long long ldc, int M, int N, int K, void *stream);

/* upp_linear_smallk_f32: y (M,N) = act(x (M,K) . W (N,K)^T + bias) for the Linear layers upp_linear_f32 does not take (K not a
 * multiple of 4, unaligned rows): the first layer of every position MLP (K = 3; reference models/Point_MAE_unify.py pos_embed /
 * models/Point_MAE_pretask_dev.py:395-399 `nn.Linear(3, 128), nn.GELU(), nn.Linear(128, dim)`) and the first point-wise layer of
 * the rectify prompter's feature propagation (K = 59, :475-517).  act: 0 none, 1 ReLU, 2 GELU (erf).  VALU kernel, sums over k in
 * ascending order.  Limits: K <= 64, N <= 256.
 * upp_transpose_f32: dst (cols, rows; ld_dst) = src (rows, cols; ld_src)^T -- the W^T a data-gradient GEMM needs of a TRAINABLE
 * weight (frozen ones are transposed once and cached by the caller). */
int upp_linear_smallk_f32(const float *x, long long ldx, const float *W, long long ldw, const float *bias, float *y, long long ldy,
                          int M, int N, int K, int act, void *stream);
/* upp_linear_smallk_gelu_d_f32 (round 6): y = GELU(x . W^T + bias) and d = GELU'(x . W^T + bias) in the same pass (erf form, as
 * upp_linear_f32's epilogue 3): the first layer of a TRAINABLE position MLP keeps the derivative for its backward. */
int upp_linear_smallk_gelu_d_f32(const float *x, long long ldx, const float *W, long long ldw, const float *bias, float *y, long long ldy,
                                 float *d, long long ldd, int M, int N, int K, void *stream);
/* upp_linear_smallk_wgrad_f32: partials (chunks, N, K)[c][n][k] = sum over the rows m of chunk c of G[m][n] * X[m][k] -- the weight gradient of
 * a small Linear (N K <= 2048, any alignment) over many rows, rows added in ascending order; the caller sums the chunks (upp_batched_sum).
 * (The rectify prompter's point-wise layers in the pre-task recipe: 32 x 27, 64 x 3, ... over 34,432 rows.) */
int upp_linear_smallk_wgrad_f32(const float *G, long long ldg, const float *X, long long ldx, float *partials, int M, int N, int K,
                                int chunks, void *stream);
int upp_transpose_f32(const float *src, long long ld_src, float *dst, long long ld_dst, int rows, int cols, void *stream);
/* upp_transpose_batched_f32: dst_j (cols_j, rows_j) = src_j (rows_j, cols_j)^T for `count` contiguous matrices in one launch (host arrays of
 * device pointers and sizes): the W^T copies of ALL trainable weights of a recipe, refreshed once per training step. */
int upp_transpose_batched_f32(const float *const *src, float *const *dst, const int *rows, const int *cols, int count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UPP_HIP_H */
