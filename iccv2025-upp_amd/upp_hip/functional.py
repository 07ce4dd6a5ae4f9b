"""Autograd Functions over upp_hip.ops with the reference operators' contracts."""
import os
import sys

import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import _derived, ops

class FurthestPointSampling(Function):
    """pointnet2_utils.furthest_point_sample: (B,N,3) f32, npoint -> (B,npoint) int32, non-differentiable."""

    @staticmethod
    def forward(ctx, xyz, npoint):
        idx = ops.fps(xyz, npoint)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, grad_out):
        return None, None


class GatherOperation(Function):
    """pointnet2_utils.gather_operation: features (B,C,N), idx (B,M) int32 -> (B,C,M); grad w.r.t. features."""

    @staticmethod
    def forward(ctx, features, idx):
        ctx.save_for_backward(idx)
        ctx.N = features.shape[2]
        return ops.gather_fwd(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return ops.gather_bwd(grad_out.contiguous(), idx, ctx.N, deterministic=DETERMINISTIC), None


class _FpsGather(Function):
    """FPS + coordinate gather in one launch (reference utils/misc.py:13-20 fps())."""

    @staticmethod
    def forward(ctx, xyz, npoint):
        idx, centers = ops.fps(xyz, npoint, want_centers=True)
        ctx.save_for_backward(idx)
        ctx.N = xyz.shape[1]
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)          # (no zero tensor for the index output's "gradient": a fill launch per backward)
        return centers, idx

    @staticmethod
    def backward(ctx, grad_centers, _grad_idx):
        if grad_centers is None:
            return None, None
        (idx,) = ctx.saved_tensors
        return ops.fps_gather_bwd(grad_centers.contiguous(), idx, ctx.N, deterministic=DETERMINISTIC), None        # (one launch: zero-fill + int32 indices + scatter)


class _KnnGroup(Function):
    """kNN + neighbourhood gather + centre subtraction in one launch
    (reference models/Point_MAE_unify.py:69-88).  Differentiable w.r.t. xyz and center
    through the gather/subtraction, not through the neighbour selection."""

    @staticmethod
    def forward(ctx, xyz, center, k):
        _, idx, neigh = ops.knn(xyz, center, k, want_dist=False, want_neigh=True)
        ctx.save_for_backward(idx)
        ctx.N = xyz.shape[1]
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return neigh, idx

    @staticmethod
    def backward(ctx, grad_neigh, _grad_idx):
        if grad_neigh is None:
            return None, None, None
        (idx,) = ctx.saved_tensors
        gx, gc = ops.group_bwd(grad_neigh.contiguous(), idx, ctx.N,
                               need_xyz=ctx.needs_input_grad[0], need_center=ctx.needs_input_grad[1], deterministic=DETERMINISTIC)
        return gx, gc, None


class _GroupPoints(Function):
    """out[b,g,k] = xyz[b, idx[b,g,k]] - center[b,g] for given indices."""

    @staticmethod
    def forward(ctx, xyz, center, idx):
        ctx.save_for_backward(idx)
        ctx.N = xyz.shape[1]
        return ops.group_fwd(xyz, center, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        gx, gc = ops.group_bwd(grad_out.contiguous(), idx, ctx.N,
                               need_xyz=ctx.needs_input_grad[0], need_center=ctx.needs_input_grad[1], deterministic=DETERMINISTIC)
        return gx, gc, None


class ChamferFunction(Function):
    """extensions.chamfer_dist.ChamferFunction (reference extensions/chamfer_dist/__init__.py:13-25)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        dist1, dist2, idx1, idx2 = ops.chamfer_fwd(xyz1, xyz2)
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        return dist1, dist2

    @staticmethod
    def backward(ctx, grad_dist1, grad_dist2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        return ops.chamfer_bwd(xyz1, xyz2, idx1, idx2, grad_dist1.contiguous(), grad_dist2.contiguous(), deterministic=DETERMINISTIC)


class _ChamferLoss(Function):
    """ChamferDistanceL1 / L2 as one node: two direction kernels + the fused reduction forward (4 launches), a scalar x factor pair and the
    gradient kernel backward -- torch's formulation issues ~7 launches forward and ~8 backward around the same two kernels."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, l1):
        dist1, dist2, idx1, idx2 = ops.chamfer_fwd(xyz1, xyz2)
        loss, fac1, fac2 = ops.chamfer_loss(dist1, dist2, l1)
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2, fac1, fac2)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        xyz1, xyz2, idx1, idx2, fac1, fac2 = ctx.saved_tensors
        g1, g2 = ops.chamfer_bwd(xyz1, xyz2, idx1, idx2, fac1 * g, fac2 * g, deterministic=DETERMINISTIC)
        return g1, g2, None


def chamfer_loss(xyz1, xyz2, l1=True):
    """ChamferDistanceL1 (l1) / ChamferDistanceL2 of two batches of clouds (reference extensions/chamfer_dist/__init__.py:44-84)."""
    return _ChamferLoss.apply(xyz1.contiguous(), xyz2.contiguous(), bool(l1))


class EarthMoverDistanceFunction(Function):
    """extensions.emd.emd.EarthMoverDistanceFunction (reference extensions/emd/emd.py:5-21)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        xyz1 = xyz1.contiguous()
        xyz2 = xyz2.contiguous()
        assert xyz1.is_cuda and xyz2.is_cuda, "Only support cuda currently."
        match = ops.emd_approxmatch(xyz1, xyz2)
        cost = ops.emd_matchcost(xyz1, xyz2, match, deterministic=DETERMINISTIC)
        ctx.save_for_backward(xyz1, xyz2, match)
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        xyz1, xyz2, match = ctx.saved_tensors
        return ops.emd_matchcost_bwd(grad_cost.contiguous(), xyz1, xyz2, match)


class BallQuery(Function):
    """pointnet2_utils.ball_query: radius, nsample, xyz (B,N,3), new_xyz (B,P,3) -> (B,P,nsample) int32, non-differentiable."""

    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        idx = ops.ball_query(radius, nsample, xyz, new_xyz)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, grad_out):
        return None, None, None, None


class ThreeNN(Function):
    """pointnet2_utils.three_nn: unknown (B,n,3), known (B,m,3) -> (dist (B,n,3) f32 Euclidean, idx (B,n,3) int32), non-differentiable."""

    @staticmethod
    def forward(ctx, unknown, known):
        dist, idx = ops.three_nn(unknown, known)
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, grad_dist, grad_idx):
        return None, None


class ThreeInterpolate(Function):
    """pointnet2_utils.three_interpolate: features (B,C,m), idx (B,n,3) int32, weight (B,n,3) -> (B,C,n); grad w.r.t. features."""

    @staticmethod
    def forward(ctx, features, idx, weight):
        ctx.save_for_backward(idx, weight)
        ctx.m = features.shape[2]
        return ops.three_interpolate_fwd(features, idx, weight)

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        return ops.three_interpolate_bwd(grad_out.contiguous(), idx, weight, ctx.m, deterministic=DETERMINISTIC), None, None


class GroupingOperation(Function):
    """pointnet2_utils.grouping_operation: features (B,C,N), idx (B,P,S) int32 -> (B,C,P,S); grad w.r.t. features."""

    @staticmethod
    def forward(ctx, features, idx):
        ctx.save_for_backward(idx)
        ctx.N = features.shape[2]
        return ops.grouping_fwd(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return ops.grouping_bwd(grad_out.contiguous(), idx, ctx.N, deterministic=DETERMINISTIC), None


class KnnPoints(Function):
    """pytorch3d.ops.knn_points as one node: p1 (N,P1,D), p2 (N,P2,D), lengths1, lengths2 (device int64 | None), K, norm, return_nn
    -> dists (N,P1,K), idx (N,P1,K) int64 (non-differentiable), nn (N,P1,K,D) | None.  dists is differentiable w.r.t. p1 and p2, nn
    (= knn_gather(p2, idx, lengths2) on the real rows) w.r.t. p2; the neighbour selection is not differentiated."""

    @staticmethod
    def forward(ctx, p1, p2, lengths1, lengths2, K, norm, return_nn):
        dists, idx, nn = ops.knn_points(p1, p2, lengths1, lengths2, K=K, norm=norm, want_nn=return_nn)
        ctx.save_for_backward(p1, p2, idx, lengths1, lengths2)
        ctx.norm = norm
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return dists, idx, nn

    @staticmethod
    def backward(ctx, grad_dists, _grad_idx, grad_nn):
        p1, p2, idx, lengths1, lengths2 = ctx.saved_tensors
        g_p1 = g_p2 = None
        if grad_dists is not None:
            g_p1, t = ops.knn_points_bwd(p1, p2, idx, grad_dists.contiguous(), lengths1, lengths2, norm=ctx.norm)
            if ctx.needs_input_grad[1]:
                g_p2 = ops.knn_scatter_add(t, idx, p2.shape[1], rows=lengths1, slots=lengths2, negate=True, deterministic=DETERMINISTIC)
        if grad_nn is not None and ctx.needs_input_grad[1]:
            g_nn = ops.knn_scatter_add(grad_nn.contiguous(), idx, p2.shape[1], rows=lengths1, slots=lengths2, deterministic=DETERMINISTIC)
            g_p2 = g_nn if g_p2 is None else g_p2 + g_nn
        return (g_p1 if ctx.needs_input_grad[0] else None), g_p2, None, None, None, None, None


class KnnGather(Function):
    """pytorch3d.ops.knn_gather: x (N,M,U), idx (N,L,K) int64, lengths (device int64 | None) -> (N,L,K,U), zeros in slots
    k >= lengths[n]; grad w.r.t. x."""

    @staticmethod
    def forward(ctx, x, idx, lengths):
        ctx.save_for_backward(idx, lengths)
        ctx.M = x.shape[1]
        return ops.knn_gather(x, idx, lengths)

    @staticmethod
    def backward(ctx, grad_out):
        idx, lengths = ctx.saved_tensors
        return ops.knn_scatter_add(grad_out.contiguous(), idx, ctx.M, slots=lengths, deterministic=DETERMINISTIC), None, None


furthest_point_sample = FurthestPointSampling.apply
gather_operation = GatherOperation.apply


def _torch_cpu(*tensors):
    """CPU tensors and the opt-in torch formulations switched on (upp_hip.torch_cpu: BASELINE configs[0], plumbing on a GPU-less host)?
    Otherwise the operators below go to upp_hip.ops, which serves HIP tensors only and says so."""
    from . import torch_cpu
    return torch_cpu.enabled() and all(isinstance(t, torch.Tensor) and not t.is_cuda for t in tensors)


def fps_gather(xyz, npoint):
    """-> (centers (B,npoint,3), idx (B,npoint) int32)."""
    if _torch_cpu(xyz):
        from . import torch_cpu
        return torch_cpu.fps(xyz, int(npoint))
    return _FpsGather.apply(xyz, int(npoint))


def fps_gather_ragged(xyz, offsets, max_len, npoint, lengths=None):
    """FPS of every cloud of a packed batch (xyz (T,3) f32, offsets (B+1,) int64) -> (centers (B,npoint,3), idx (B,npoint) int32, local to
    each cloud): one launch, the result of fps_gather(cloud[None], npoint) per cloud.  No gradient (an input path)."""
    if _torch_cpu(xyz, offsets):
        from . import torch_cpu
        ops.ragged_layout((offsets[1:] - offsets[:-1]).tolist(), xyz.shape[0], max_len)
        return torch_cpu.fps_ragged(xyz, offsets, int(npoint))
    with torch.no_grad():
        idx, centers = ops.fps_ragged(xyz, offsets, max_len, int(npoint), want_centers=True, lengths=lengths)
    return centers, idx


def cloud_norm_ragged(xyz, offsets, max_len, want_scale=False, lengths=None):
    """pc_norm of every cloud of a packed batch (xyz (T,3) f64 or f32) -> (T,3) f32 [, scale (B,) f64]."""
    if _torch_cpu(xyz, offsets):
        from . import torch_cpu
        ops.ragged_layout((offsets[1:] - offsets[:-1]).tolist(), xyz.shape[0], max_len, fps=False)
        out, scale = torch_cpu.cloud_norm_ragged(xyz, offsets)
        return (out, scale) if want_scale else out
    with torch.no_grad():
        return ops.cloud_norm_ragged(xyz, offsets, max_len, want_scale=want_scale, lengths=lengths)


def knn_query(ref, query, k):
    """-> (dist (B,Q,k) f32, idx (B,Q,k) int64); no gradient (the reference wraps it in no_grad)."""
    if _torch_cpu(ref, query):
        from . import torch_cpu
        return torch_cpu.knn(ref, query, int(k))
    with torch.no_grad():
        dist, idx, _ = ops.knn(ref, query, k, want_dist=True, want_neigh=False)
    return dist, idx


def knn_group(xyz, center, k):
    """-> (neighborhood (B,G,k,3) centred on `center`, idx (B,G,k) int64)."""
    if _torch_cpu(xyz, center):
        from . import torch_cpu
        return torch_cpu.knn_group(xyz, center, int(k))
    return _KnnGroup.apply(xyz, center, int(k))


def group_points(xyz, center, idx):
    return _GroupPoints.apply(xyz, center, idx)


# ------------------------------------------------------------------ the pointnet2_ops surface (README "The pointnet2_ops surface")
def ball_query(radius, nsample, xyz, new_xyz):
    """pointnet2_utils.ball_query -> (B,P,nsample) int32."""
    if _torch_cpu(xyz, new_xyz):
        from . import torch_cpu
        return torch_cpu.ball_query(float(radius), int(nsample), xyz, new_xyz)
    return BallQuery.apply(float(radius), int(nsample), xyz, new_xyz)


def three_nn(unknown, known):
    """pointnet2_utils.three_nn -> (dist (B,n,3) f32, idx (B,n,3) int32)."""
    if _torch_cpu(unknown, known):
        from . import torch_cpu
        return torch_cpu.three_nn(unknown, known)
    return ThreeNN.apply(unknown, known)


def three_interpolate(features, idx, weight):
    """pointnet2_utils.three_interpolate: features (B,C,m) -> (B,C,n)."""
    if _torch_cpu(features, idx, weight):
        from . import torch_cpu
        return torch_cpu.three_interpolate(features, idx, weight)
    return ThreeInterpolate.apply(features, idx, weight)


def grouping_operation(features, idx):
    """pointnet2_utils.grouping_operation: features (B,C,N), idx (B,P,S) int32 -> (B,C,P,S)."""
    if _torch_cpu(features, idx):
        from . import torch_cpu
        return torch_cpu.grouping_operation(features, idx)
    return GroupingOperation.apply(features, idx)


# ------------------------------------------------------------------ the pytorch3d.ops surface (README "The pytorch3d.ops surface")
def _device_lengths(lengths, N, like, name):
    """lengths of a ragged batch: None | a device int64 tensor | a CPU tensor or a list, uploaded once -- never read back."""
    if lengths is None or not like.is_cuda:
        return lengths if lengths is None or isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths, dtype=torch.int64)
    return ops._lengths(lengths, N, like.device, name)


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True):
    """pytorch3d.ops.knn_points -> (dists (N,P1,K), idx (N,P1,K) int64, knn (N,P1,K,D) | None); include/upp_hip.h upp_knn_points."""
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    if p1.dim() != 3 or p2.dim() != 3:
        raise ValueError("pts1 and pts2 must be (N, P, D) tensors.")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("pts1 and pts2 must have the same batch dimension.")
    if p1.shape[2] != p2.shape[2]:
        raise ValueError("pts1 and pts2 must have the same point dimension.")
    N, K = p1.shape[0], int(K)
    lengths1, lengths2 = _device_lengths(lengths1, N, p1, "lengths1"), _device_lengths(lengths2, N, p1, "lengths2")
    if _torch_cpu(p1, p2):
        from . import torch_cpu
        return torch_cpu.knn_points(p1, p2, lengths1, lengths2, norm=norm, K=K, return_nn=return_nn)
    return KnnPoints.apply(p1.contiguous(), p2.contiguous(), lengths1, lengths2, K, int(norm), bool(return_nn))


def knn_gather(x, idx, lengths=None):
    """pytorch3d.ops.knn_gather: x (N,M,U), idx (N,L,K) int64 -> (N,L,K,U), zeros in slots k >= lengths[n]."""
    if x.dim() != 3 or idx.dim() != 3 or x.shape[0] != idx.shape[0]:
        raise ValueError("x (N, M, U) and idx (N, L, K) must have the same batch dimension.")
    lengths = _device_lengths(lengths, x.shape[0], x, "lengths")
    if _torch_cpu(x, idx):
        from . import torch_cpu
        return torch_cpu.knn_gather(x, idx, lengths)
    return KnnGather.apply(x.contiguous(), idx.contiguous(), lengths)


# ------------------------------------------------------------------ edge convolution (README "The DGCNN grouper")
class _EdgeConvMax(Function):
    """max_k lrelu(GroupNorm(A[idx] + Bq)) as one node (include/upp_hip.h "edge convolution"): saves A, Bq, idx, the arg-extreme bytes and
    the (B,G) statistics -- never a (B,Nq,K,O) tensor.  The g_A scatter-add follows the deterministic mode: `det` None reads DETERMINISTIC
    when the backward runs, True / False fixes it for this call."""

    @staticmethod
    def forward(ctx, A, Bq, idx, gamma, beta, groups, eps, slope, det):
        out, arg, mean, rstd = ops.edge_conv_fwd(A, Bq, idx, gamma, beta, groups, eps, slope)
        ctx.save_for_backward(A, Bq, idx, arg, gamma, beta, mean, rstd)
        ctx.cfg = (groups, slope, det)
        return out

    @staticmethod
    def backward(ctx, g_out):
        A, Bq, idx, arg, gamma, beta, mean, rstd = ctx.saved_tensors
        groups, slope, det = ctx.cfg
        g_A, g_Bq, g_gamma, g_beta = ops.edge_conv_bwd(g_out.contiguous(), A, Bq, idx, arg, gamma, beta, mean, rstd, groups, slope, deterministic=_det(det))
        need = ctx.needs_input_grad
        return (g_A if need[0] else None, g_Bq if need[1] else None, None, g_gamma if groups and need[3] else None,
                g_beta if groups and need[4] else None, None, None, None, None)


def _edge_norm(norm):
    """None | torch.nn.GroupNorm | (G, gamma, beta, eps) -> None | (G, gamma, beta, eps)"""
    if norm is None:
        return None
    if isinstance(norm, torch.nn.GroupNorm):
        if norm.weight is None:
            raise ValueError("edge_conv_max: the GroupNorm must be affine")
        return norm.num_groups, norm.weight, norm.bias, norm.eps
    G, gamma, beta, eps = norm
    return int(G), gamma, beta, float(eps)


def edge_conv_usable(A, Bq, idx, norm=None):
    """Do the fused kernels serve these operands (HIP f32 / int64 tensors of the served sizes)?"""
    norm = _edge_norm(norm)
    if not (A.is_cuda and Bq.is_cuda and idx.is_cuda and A.dtype == torch.float32 and Bq.dtype == torch.float32 and idx.dtype == torch.int64
            and A.dim() == 3 and Bq.dim() == 3 and idx.dim() == 3):
        return False
    if norm is not None and not (norm[1].is_cuda and norm[1].dtype == torch.float32 and norm[2].dtype == torch.float32):
        return False
    return ops.edge_conv_usable(A.shape[0], A.shape[1], idx.shape[1], idx.shape[2], A.shape[2], norm[0] if norm is not None else 0)


def edge_conv_max(A, Bq, idx, norm=None, slope=0.2, deterministic=None):
    """A (B,Nk,O) key-side product, Bq (B,Nq,O) query-side product (+ bias), idx (B,Nq,K) int64 -> (B,Nq,O) =
    max_k leaky_relu(norm(A[b, idx[b,q,k]] + Bq[b,q]), slope).  norm: None, a torch.nn.GroupNorm or (G, gamma, beta, eps).
    deterministic: None follows functional.DETERMINISTIC (read when the backward node runs), True / False per call.  HIP tensors outside
    the served range raise (upp_edge_conv_fwd: 1 <= K <= 64, 1 <= O <= 512, G | O); CPU tensors take the torch formulation when
    upp_hip.torch_cpu is enabled."""
    if not 0.0 <= float(slope) <= 1.0:
        raise ValueError("edge_conv_max: slope must be in [0, 1]")
    norm = _edge_norm(norm)
    if _torch_cpu(A, Bq, idx):
        from . import torch_cpu
        return torch_cpu.edge_conv_max(A, Bq, idx, norm, slope)
    G, gamma, beta, eps = norm if norm is not None else (0, None, None, 1e-5)
    if norm is not None and G < 1:
        raise ValueError("edge_conv_max: a norm needs at least one group")
    return _EdgeConvMax.apply(A.contiguous(), Bq.contiguous(), idx.contiguous(), None if gamma is None else gamma.contiguous(),
                              None if beta is None else beta.contiguous(), int(G), float(eps), float(slope),
                              None if deterministic is None else bool(deterministic))


# ------------------------------------------------------------------ broadcast expand (README "The PoinTr completion model")
class _ExpandAct(Function):
    """lrelu(BatchNorm(P[r] + Wu U[., s])) as one node (include/upp_hip.h "broadcast expand"): saves P, U, Wu and the (O,) statistics --
    never an (R,S,O) tensor besides the output's own gradient.  Returns (h, mean, var); mean and the biased var are the batch statistics
    in training mode (for the running buffers; not differentiable) and None otherwise."""

    @staticmethod
    def forward(ctx, P, U, Wu, gamma, beta, mean, rstd, mode, eps, slope):
        h, mean, var, rstd = ops.expand_fwd(P, U, Wu, gamma, beta, mean, rstd, mode, eps, slope)
        ctx.save_for_backward(P, U, Wu, gamma, beta, mean, rstd)
        ctx.cfg = (mode, slope)
        if mode == ops.EXPAND_TRAIN:
            ctx.mark_non_differentiable(mean, var)
            return h, mean, var
        return h, None, None

    @staticmethod
    def backward(ctx, g_h, _g_mean, _g_var):
        P, U, Wu, gamma, beta, mean, rstd = ctx.saved_tensors
        mode, slope = ctx.cfg
        need = ctx.needs_input_grad
        g_P, g_U, g_Wu, g_gamma, g_beta = ops.expand_bwd(g_h.contiguous(), P, U, Wu, gamma, beta, mean, rstd, mode, slope, want_gU=need[1])
        return (g_P if need[0] else None, g_U, g_Wu if need[2] else None, g_gamma if mode and need[3] else None,
                g_beta if mode and need[4] else None, None, None, None, None, None)


# ------------------------------------------------------------------ query selection (README "The AdaPoinTr completion model")
class _QuerySelect(Function):
    """The Q best-ranked candidates, then the extra points, as one node (include/upp_hip.h "query selection"); the backward writes
    every row of g_cand once -- no zero-fill, no scatter.  score gets no gradient."""

    @staticmethod
    def forward(ctx, score, cand, extra, Q):
        out, order = ops.query_select_fwd(score, cand, Q, extra)
        ctx.save_for_backward(order)
        ctx.M = cand.shape[1]
        ctx.mark_non_differentiable(order)
        return out, order

    @staticmethod
    def backward(ctx, g_out, _g_order):
        (order,) = ctx.saved_tensors
        g_cand, g_extra = ops.query_select_bwd(g_out.contiguous(), order, ctx.M)
        need = ctx.needs_input_grad
        return None, g_cand if need[1] else None, g_extra if need[2] else None, None


def query_select_usable(score, cand, Q, extra=None):
    ts = [score, cand] + ([extra] if extra is not None else [])
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    if score.dim() != 2 or cand.dim() != 3 or tuple(cand.shape) != (score.shape[0], score.shape[1], 3) or score.shape[0] < 1:
        return False
    if extra is not None and (extra.dim() != 3 or extra.shape[0] != score.shape[0] or extra.shape[2] != 3):
        return False
    return ops.query_select_usable(score.shape[1], int(Q))


def query_select(score, cand, Q, extra=None):
    """score (B,M), cand (B,M,3), extra (B,D,3) or None -> (out (B,Q+D,3), order (B,Q) int32): out[:, :Q] are the Q candidates of
    greatest score in descending order, equal scores by ascending index and NaN first (the reference's torch.argsort(descending=True)
    leaves the tie order open), out[:, Q:] the extra points.  cand and extra get gradients, score gets none.  1 <= Q <= M <= 4096 on
    the kernels; HIP tensors outside that take the torch formulation (note_declined records it); CPU tensors take it when
    upp_hip.torch_cpu is enabled."""
    Q = int(Q)
    if score.dim() != 2 or not 1 <= Q <= score.shape[1]:
        raise ValueError("query_select: score (B, M) and 1 <= Q <= M, got %s and Q = %d" % (tuple(score.shape), Q))
    from . import torch_cpu
    ts = [score, cand] + ([extra] if extra is not None else [])
    if _torch_cpu(*ts):
        return torch_cpu.query_select(score, cand, Q, extra)
    if score.is_cuda and not query_select_usable(score, cand, Q, extra):
        note_declined("query_select score %s, Q = %d" % (tuple(score.shape), Q), "outside the served range")
        return torch_cpu.query_select(score, cand, Q, extra)
    if extra is not None and extra.shape[1] == 0:
        extra = None
    return _QuerySelect.apply(score.detach().contiguous(), cand.contiguous(), None if extra is None else extra.contiguous(), Q)


# ------------------------------------------------------------------ deformable local cross-attention (README section of that name)
class _DeformAttention(Function):
    """softmax over the k interpolated neighbour rows of every query as one node (include/upp_hip.h "deformable local cross-attention"):
    saves its inputs, ctx's companion p (B,N,H,k) and nothing of B N k C elements -- the key / value rows are recomputed.  The d_PK / d_PV
    scatter-add follows the deterministic mode (`det`: _det).  idx3 and w3 get no gradient."""

    @staticmethod
    def forward(ctx, q, PK, PV, bk, bv, idx3, w3, num_heads, scale, det):
        out, p = ops.deform_attn_fwd(q, PK, PV, bk, bv, idx3, w3, num_heads, scale)
        ctx.save_for_backward(q, PK, PV, bk, bv, idx3, w3, p)
        ctx.cfg = (num_heads, scale, det)
        return out

    @staticmethod
    def backward(ctx, g):
        q, PK, PV, bk, bv, idx3, w3, p = ctx.saved_tensors
        num_heads, scale, det = ctx.cfg
        need = ctx.needs_input_grad
        g = g.contiguous()
        want_bk = bk is not None and need[3]
        d_q, d_PK, d_PV, _ds, d_krow = ops.deform_attn_bwd(q, PK, PV, bk, bv, idx3, w3, p, g, num_heads, scale,
                                                           deterministic=_det(det), want_krow=want_bk)
        C = g.shape[-1]
        return (d_q if need[0] else None, d_PK if need[1] else None, d_PV if need[2] else None,
                ops.sum_rows(d_krow.view(-1, C)) if want_bk else None,
                ops.sum_rows(g.view(-1, C)) if bv is not None and need[4] else None, None, None, None, None, None)


def _deform_f32(*ts):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in ts)


def _deform_operands(idx3, *f32):                      # HIP f32 tensors plus an int32 HIP idx3: what the deformable kernels take
    return _deform_f32(*f32) and isinstance(idx3, torch.Tensor) and idx3.is_cuda and idx3.dtype == torch.int32


def deform_attention_usable(q, PK, PV, idx3, w3, num_heads):
    """Do the fused kernels serve these operands (HIP f32 / int32 tensors, head_dim 64, the served sizes of include/upp_hip.h)?"""
    if not _deform_operands(idx3, q, PK, PV, w3) or q.dim() != 3 or PK.dim() != 4 or PV.shape != PK.shape or idx3.dim() != 4 or idx3.shape != w3.shape:
        return False
    B, N, C = q.shape
    G, NK = PK.shape[1], PK.shape[2]
    H = int(num_heads)
    if H < 1 or C != 64 * H or N < 1 or idx3.shape[2] % N or tuple(PK.shape) != (B, G, NK, C) or tuple(idx3.shape[:2]) != (B, G):
        return False
    return ops.deform_attn_usable(B, N, NK, idx3.shape[2] // N, H, G)


def deform_offset(A, Bq, idx, pos, gamma, beta, eps, W3, ball=False):
    """A (B,G,NK,C) and Bq (B,G,N,C) the per-point halves of the offset head's first Linear, idx (B,N,k) int64 (HF.knn_query's list),
    pos (B,NK,3), LayerNorm gamma / beta (C) and eps, W3 (3,C) -> shift (B,G,N k,3) = pos[idx] + tanh(W3 gelu(LayerNorm(A[idx] + Bq))).
    ball: the tanh is scaled by 0.5 (max_s pos[idx] - min_s pos[idx]) over the k slots of the query (upp_deform_offset_ball_fwd, the
    `improved` modules).  No autograd node: it runs under no_grad (three_nn, its only consumer, is not differentiable).  HIP tensors
    outside the served range (C = 64 H, H <= 16, k <= 32) take the torch formulation (note_declined records it); CPU tensors take it
    when upp_hip.torch_cpu is enabled."""
    from . import torch_cpu
    ball = bool(ball)
    with torch.no_grad():
        if _torch_cpu(A, Bq, idx, pos):
            return torch_cpu.deform_offset(A, Bq, idx, pos, gamma, beta, eps, W3, ball)
        if A.is_cuda and not (_deform_f32(A, Bq, pos, gamma, beta, W3) and A.dim() == 4 and A.shape[3] % 64 == 0 and idx.dim() == 3 and
                              ops.deform_attn_usable(A.shape[0], idx.shape[1], A.shape[2], idx.shape[2], A.shape[3] // 64, A.shape[1])):
            note_declined("deform_offset A %s, k = %d" % (tuple(A.shape), idx.shape[-1]), "outside the served range")
            return torch_cpu.deform_offset(A, Bq, idx, pos, gamma, beta, eps, W3, ball)
        return ops.deform_offset_fwd(A.contiguous(), Bq.contiguous(), idx.long().contiguous(), pos.contiguous(), gamma.contiguous(),
                                     beta.contiguous(), W3.contiguous(), float(eps), ball)


def deform_attention(q, PK, PV, bk, bv, idx3, w3, num_heads, scale, deterministic=None):
    """q (B,N,C), PK / PV (B,G,NK,C) the per-group key / value products of the memory tokens, bk / bv (C) or None, idx3 int32 and w3 f32
    (B,G,N k,3) (three_nn of the shifted positions and the reference's weights) -> ctx (B,N,C): per query and head the softmax over the
    k interpolated neighbour rows (include/upp_hip.h "deformable local cross-attention").  q, PK, PV, bk, bv get gradients, idx3 and w3
    none.  deterministic: None follows functional.DETERMINISTIC (read when the backward node runs), True / False per call.  HIP tensors
    outside the served range (head_dim 64, H <= 16, G | H, k <= 32) take the torch formulation (note_declined records it); CPU tensors
    take it when upp_hip.torch_cpu is enabled."""
    from . import torch_cpu
    if _torch_cpu(q, PK, PV, idx3, w3):
        return torch_cpu.deform_attention(q, PK, PV, bk, bv, idx3, w3, num_heads, scale)
    if q.is_cuda and not deform_attention_usable(q, PK, PV, idx3, w3, num_heads):
        note_declined("deform_attention q %s, %d heads, PK %s" % (tuple(q.shape), num_heads, tuple(PK.shape)), "outside the served range")
        return torch_cpu.deform_attention(q, PK, PV, bk, bv, idx3, w3, num_heads, scale)
    return _DeformAttention.apply(q.contiguous(), PK.contiguous(), PV.contiguous(), None if bk is None else bk.contiguous(),
                                  None if bv is None else bv.contiguous(), idx3.contiguous(), w3.detach().contiguous(), int(num_heads),
                                  float(scale), None if deterministic is None else bool(deterministic))


# ------------------------------------------------------------------ deformable graph attention (README section of that name)
class _InterpEdgeMax(Function):
    """lrelu(max_s (Bq + sum_j w3 PW[idx3])) as one node (include/upp_hip.h "deformable graph attention"): saves out, the arg bytes, idx3
    and w3 -- never a (B,N,k,O) tensor, and no row is read again in the backward.  The d_PW scatter-add follows the deterministic mode
    (`det`: _det).  idx3 and w3 get no gradient."""

    @staticmethod
    def forward(ctx, PW, Bq, idx3, w3, slope, det):
        out, arg = ops.interp_max_fwd(PW, Bq, idx3, w3, slope)
        ctx.save_for_backward(out, arg, idx3, w3)
        ctx.cfg = (PW.shape[1], slope, det)
        return out

    @staticmethod
    def backward(ctx, g):
        out, arg, idx3, w3 = ctx.saved_tensors
        NK, slope, det = ctx.cfg
        d_Bq, d_PW = ops.interp_max_bwd(g.contiguous(), out, arg, idx3, w3, NK, slope, deterministic=_det(det))
        need = ctx.needs_input_grad
        return d_PW if need[0] else None, d_Bq if need[1] else None, None, None, None, None


def interp_edge_max_usable(PW, Bq, idx3, w3):
    """Do the fused kernels serve these operands (HIP f32 / int32 tensors of the served sizes of include/upp_hip.h)?"""
    if not _deform_operands(idx3, PW, Bq, w3) or PW.dim() != 3 or Bq.dim() != 3 or idx3.dim() != 3 or idx3.shape != w3.shape or idx3.shape[2] != 3:
        return False
    B, N, O = Bq.shape
    if N < 1 or idx3.shape[0] != B or idx3.shape[1] % N or PW.shape[0] != B or PW.shape[2] != O:
        return False
    return ops.interp_max_usable(B, N, PW.shape[1], idx3.shape[1] // N, O)


def interp_edge_max(PW, Bq, idx3, w3, slope=0.2, deterministic=None):
    """PW (B,NK,O) the key-side product of the memory points, Bq (B,N,O) the query-side product (+ bias), idx3 int32 and w3 f32
    (B, N k, 3) (three_nn of the shifted positions and the reference's weights) -> (B,N,O) = leaky_relu(max_s (Bq[b,n] +
    sum_j w3[b,n k+s,j] PW[b, idx3[b,n k+s,j]]), slope) (include/upp_hip.h "deformable graph attention").  PW and Bq get gradients, idx3
    and w3 none.  deterministic: None follows functional.DETERMINISTIC (read when the backward node runs), True / False per call.  HIP
    tensors outside the served range (k <= 32, O <= 1024) take the torch formulation (note_declined records it); CPU tensors take it
    when upp_hip.torch_cpu is enabled."""
    if not 0.0 <= float(slope) <= 1.0:
        raise ValueError("interp_edge_max: slope must be in [0, 1]")
    from . import torch_cpu
    if _torch_cpu(PW, Bq, idx3, w3):
        return torch_cpu.interp_edge_max(PW, Bq, idx3, w3, slope)
    if PW.is_cuda and not interp_edge_max_usable(PW, Bq, idx3, w3):
        note_declined("interp_edge_max PW %s, Bq %s, idx3 %s" % (tuple(PW.shape), tuple(Bq.shape), tuple(idx3.shape)), "outside the served range")
        return torch_cpu.interp_edge_max(PW, Bq, idx3, w3, slope)
    return _InterpEdgeMax.apply(PW.contiguous(), Bq.contiguous(), idx3.contiguous(), w3.detach().contiguous(), float(slope),
                                None if deterministic is None else bool(deterministic))


# ------------------------------------------------------------------ region-wise deformable attention (README section of that name)
class _RegionAttention(Function):
    """max over the rows of a k x k attention per token and head as one node (include/upp_hip.h "region-wise deformable attention"): saves
    its inputs and the arg bytes (B,N,C) -- nothing of B N k C or B N H k k elements; the query, key and value rows and the
    probabilities are recomputed, the probabilities by the forward's own statement.  The three scatter-adds follow the deterministic
    mode (`det`: _det); the deterministic form allocates its (3,B,N,k,C) workspace for the call.  idx, idx3 and w3 get no gradient."""

    @staticmethod
    def forward(ctx, q, idx, PK, PV, bk, bv, idx3, w3, num_heads, scale, det):
        out, arg = ops.region_attn_fwd(q, idx, PK, PV, bk, bv, idx3, w3, num_heads, scale)
        ctx.save_for_backward(q, idx, PK, PV, bk, bv, idx3, w3, arg)
        ctx.cfg = (num_heads, scale, det)
        return out

    @staticmethod
    def backward(ctx, g):
        q, idx, PK, PV, bk, bv, idx3, w3, arg = ctx.saved_tensors
        num_heads, scale, det = ctx.cfg
        need = ctx.needs_input_grad
        want_bk, want_bv = bk is not None and need[4], bv is not None and need[5]
        d_q, d_PK, d_PV, d_krow, d_vrow, _rows = ops.region_attn_bwd(q, idx, PK, PV, bk, bv, idx3, w3, arg, g.contiguous(), num_heads, scale,
                                                                     deterministic=_det(det), want_krow=want_bk, want_vrow=want_bv)
        C = g.shape[-1]
        return (d_q if need[0] else None, None, d_PK if need[2] else None, d_PV if need[3] else None,
                ops.sum_rows(d_krow.view(-1, C)) if want_bk else None, ops.sum_rows(d_vrow.view(-1, C)) if want_bv else None,
                None, None, None, None, None)


def region_attention_usable(q, idx, PK, PV, idx3, w3, num_heads):
    """Do the fused kernels serve these operands (HIP f32 / int tensors, head_dim 64, the served sizes of include/upp_hip.h)?"""
    if not (_deform_operands(idx3, q, PK, PV, w3) and isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype in (torch.int64, torch.int32)):
        return False
    if q.dim() != 3 or idx.dim() != 3 or PK.dim() != 4 or PV.shape != PK.shape or idx3.dim() != 4 or idx3.shape != w3.shape:
        return False
    B, N, C = q.shape
    G, NK, k = PK.shape[1], PK.shape[2], idx.shape[2]
    H = int(num_heads)
    if H < 1 or C != 64 * H or tuple(idx.shape) != (B, N, k) or tuple(PK.shape) != (B, G, NK, C) or tuple(idx3.shape) != (B, G, N * k, 3):
        return False
    return ops.region_attn_usable(B, N, NK, k, H, G)


def region_attention(q, idx, PK, PV, bk, bv, idx3, w3, num_heads, scale, deterministic=None):
    """q (B,N,C) the projected queries, idx (B,N,k) int64 rows of q (the neighbour list), PK / PV (B,G,NK,C) the per-group key / value
    products of the memory tokens, bk / bv (C) or None, idx3 int32 and w3 f32 (B,G,N k,3) (three_nn of the shifted positions and the
    reference's weights) -> (B,N,C): per token and head a k x k softmax attention of the k gathered query rows over the k interpolated
    key / value rows, then the per-channel maximum over the k context rows (include/upp_hip.h "region-wise deformable attention").
    q, PK, PV, bk, bv get gradients, idx, idx3 and w3 none.  deterministic: None follows functional.DETERMINISTIC (read when the backward
    node runs), True / False per call.  HIP tensors outside the served range (head_dim 64, H <= 16, G | H, k <= 32) take the torch
    formulation (note_declined records it); CPU tensors take it when upp_hip.torch_cpu is enabled."""
    from . import torch_cpu
    if _torch_cpu(q, PK, PV, idx3, w3):
        return torch_cpu.region_attention(q, idx, PK, PV, bk, bv, idx3, w3, num_heads, scale)
    if q.is_cuda and not region_attention_usable(q, idx, PK, PV, idx3, w3, num_heads):
        note_declined("region_attention q %s, %d heads, PK %s, k = %d" % (tuple(q.shape), num_heads, tuple(PK.shape), idx.shape[-1]),
                      "outside the served range")
        return torch_cpu.region_attention(q, idx, PK, PV, bk, bv, idx3, w3, num_heads, scale)
    return _RegionAttention.apply(q.contiguous(), idx.long().contiguous(), PK.contiguous(), PV.contiguous(),
                                  None if bk is None else bk.contiguous(), None if bv is None else bv.contiguous(), idx3.contiguous(),
                                  w3.detach().contiguous(), int(num_heads), float(scale), None if deterministic is None else bool(deterministic))


def _expand_norm(norm):
    if norm is None:
        return None
    if not isinstance(norm, torch.nn.BatchNorm1d) or norm.weight is None:
        raise ValueError("expand_act: norm must be None or an affine torch.nn.BatchNorm1d")
    return norm


def expand_usable(P, U, Wu, norm=None):
    """Do the fused kernels serve these operands (HIP f32 tensors of the served sizes: 1 <= J <= 4, 1 <= O <= 1024, R S O < 2^31)?"""
    ts = [P, U, Wu] + ([norm.weight, norm.bias] if norm is not None else [])
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    if P.dim() != 2 or Wu.dim() != 2 or U.dim() not in (2, 3) or U.shape[-1] != Wu.shape[1] or Wu.shape[0] != P.shape[1]:
        return False
    return ops.expand_usable(P.shape[0], U.shape[-2], P.shape[1], Wu.shape[1])


def expand_act(P, U, Wu, norm=None, slope=0.0):
    """P (R,O) the per-row product (bias included), U (S,J) shared or (R,S,J) per row, Wu (O,J) -> h (R,S,O) =
    leaky_relu(norm(P[r] + Wu U[., s]), slope): a 1x1 conv over [u ; f repeated along s] with W = [Wu | Wf], P = Wf f + b, without the
    concatenation or the pre-norm tensor.  norm: None or an affine torch.nn.BatchNorm1d -- batch statistics in training mode (the running
    buffers are updated as torch does, with element-wise launches only: capturable), the running statistics in eval mode.  A shared U
    that requires a gradient raises.  HIP tensors outside the served range take the torch formulation (note_declined records it); CPU
    tensors take it when upp_hip.torch_cpu is enabled."""
    if not 0.0 <= float(slope) <= 1.0:
        raise ValueError("expand_act: slope must be in [0, 1]")
    norm = _expand_norm(norm)
    if U.dim() == 2 and U.requires_grad and torch.is_grad_enabled():
        raise ValueError("expand_act: a shared U (S, J) that requires a gradient is not served; pass it per row (R, S, J)")
    from . import torch_cpu
    if _torch_cpu(P, U, Wu):
        return torch_cpu.expand_act(P, U, Wu, norm, slope)
    if P.is_cuda and not expand_usable(P, U, Wu, norm):
        note_declined("expand_act P %s, U %s" % (tuple(P.shape), tuple(U.shape)), "outside the served range")
        return torch_cpu.expand_act(P, U, Wu, norm, slope)
    P, U, Wu = P.contiguous(), U.contiguous(), Wu.contiguous()
    if norm is None:
        return _ExpandAct.apply(P, U, Wu, None, None, None, None, ops.EXPAND_NONE, 1e-5, float(slope))[0]
    gamma, beta = norm.weight.contiguous(), norm.bias.contiguous()
    if norm.training or norm.running_mean is None:
        n = P.shape[0] * U.shape[-2]
        if n == 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % ((P.shape[0], U.shape[-2], P.shape[1]),))
        h, mean, var = _ExpandAct.apply(P, U, Wu, gamma, beta, None, None, ops.EXPAND_TRAIN, float(norm.eps), float(slope))
        if norm.training and norm.running_mean is not None:
            with torch.no_grad():
                norm.num_batches_tracked.add_(1)
                if norm.momentum is None:                                 # the cumulative average: 1 / count, formed on the device
                    f = norm.num_batches_tracked.to(torch.float32).reciprocal()
                    norm.running_mean.add_((mean - norm.running_mean) * f)
                    norm.running_var.add_((var * (n / (n - 1.0)) - norm.running_var) * f)
                else:
                    m = float(norm.momentum)
                    norm.running_mean.mul_(1.0 - m).add_(mean, alpha=m)
                    norm.running_var.mul_(1.0 - m).add_(var, alpha=m * n / (n - 1.0))
        return h
    with torch.no_grad():
        rstd = torch.rsqrt(norm.running_var + norm.eps)
    return _ExpandAct.apply(P, U, Wu, gamma, beta, norm.running_mean, rstd, ops.EXPAND_EVAL, float(norm.eps), float(slope))[0]


class QueryAndGroup(torch.nn.Module):
    """pointnet2_utils.QueryAndGroup: ball query around new_xyz, then the grouped coordinates (centre subtracted) and / or features.
    forward(xyz (B,N,3), new_xyz (B,P,3), features (B,C,N) | None) -> (B, 3+C, P, S) | (B, C, P, S) with use_xyz=False | (B, 3, P, S)
    without features."""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        grouped_xyz = None
        if self.use_xyz or features is None:
            grouped_xyz = grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is None:
            if not self.use_xyz:
                raise ValueError("QueryAndGroup: no features and use_xyz=False leave nothing to group")
            return grouped_xyz
        grouped = grouping_operation(features, idx)
        return torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped


class GroupAll(torch.nn.Module):
    """pointnet2_utils.GroupAll: the whole cloud as one group.  forward(xyz (B,N,3), new_xyz (ignored), features (B,C,N) | None)
    -> (B, 3+C, 1, N) | (B, C, 1, N) with use_xyz=False | (B, 3, 1, N) without features."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return grouped_xyz
        grouped = features.unsqueeze(2)
        return torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped


# ------------------------------------------------------------------ Transformer block glue
ROW_IDENTITY, ROW_INSERT_CLS, ROW_INSERT, ROW_STRIP_CLS, ROW_STRIP = 0, 1, 2, 3, 4


class _RowLN(Function):
    """rows = map(x (+add), prompts; mode, P) (+ dp_scale(u) * y);  returns (rows, LayerNorm(rows)).
    One kernel forward, one backward (+ one for trainable LayerNorm parameters).  See upp_rowln_fwd."""

    @staticmethod
    def forward(ctx, x, add, prompts, y, gamma, beta, mode, P, u, keep, eps, cls_add=None, ybias=None):
        x = x.contiguous()
        B, Lin, D = x.shape
        Lout = Lin + P if mode in (ROW_INSERT_CLS, ROW_INSERT) else (Lin - P if mode in (ROW_STRIP_CLS, ROW_STRIP) else Lin)
        add_c = add.contiguous() if add is not None else None
        y_c = y.contiguous() if y is not None else None
        xo, h, mean, rstd = ops.rowln_fwd(x, add_c, prompts, mode, P, y_c, u, keep, gamma, beta, eps, Lout, ybias=ybias)
        ctx.save_for_backward(xo, mean, rstd, gamma, u)
        ctx.dims = (B, Lin, Lout, D, P, mode)
        ctx.keep = keep
        ctx.has = (add is not None, prompts is not None, y is not None, gamma is not None)
        ctx.param_ptrs = tuple(t.data_ptr() if t is not None else 0 for t in (prompts, gamma, beta, cls_add))
        ctx.cls_shape = tuple(cls_add.shape) if cls_add is not None else None
        if gamma is None:
            return xo, xo.new_empty(0)
        return xo, h

    @staticmethod
    def backward(ctx, g_xo, g_h):
        xo, mean, rstd, gamma, u = ctx.saved_tensors
        B, Lin, Lout, D, P, mode = ctx.dims
        has_add, has_prompts, has_y, has_ln = ctx.has
        need = ctx.needs_input_grad
        g_xo = g_xo.contiguous() if g_xo is not None else None
        g_hc = g_h.contiguous() if (has_ln and g_h is not None) else None
        if g_xo is None and g_hc is None:
            return (None,) * 13
        strip = mode in (ROW_STRIP_CLS, ROW_STRIP) and P > 0
        need_cls = ctx.cls_shape is not None and len(need) > 11 and need[11]
        need_ln = has_ln and g_hc is not None and (need[4] or need[5])
        g_x, g_p, g_y, ln_part = ops.rowln_bwd(g_xo, g_hc, xo, mean, rstd, gamma, mode, u, ctx.keep, B, Lin, Lout, D, P,
                                               need_x=need[0] or (has_add and need[1]) or need_cls,
                                               need_prompt=has_prompts and need[2], need_y=has_y and need[3], need_ln_part=need_ln)
        g_gamma = g_beta = g_prompts = None
        p_prompts, p_gamma, p_beta, p_cls = ctx.param_ptrs
        g_cls = None
        if need_cls:     # `add` holds a trainable row 0 (the cls position) whose gradient is the batch sum of g_x[:, 0]
            _, g_cls = _DEFERRED.reduce(p_cls, g_x.view(B, Lin * D), 0, D)
            if g_cls is not None:
                g_cls = g_cls.view(ctx.cls_shape)
        if need_ln:      # per-workgroup partials [d_gamma | d_beta] written by the same backward pass
            _, g_gamma = _DEFERRED.reduce(p_gamma, ln_part, 0, D)
            _, g_beta = _DEFERRED.reduce(p_beta, ln_part, D, D)
        if g_p is not None:
            _, g_prompts = _DEFERRED.reduce(p_prompts, g_p.view(B, P * D), 0, P * D)
            if g_prompts is not None:
                g_prompts = g_prompts.view(P, D)
        return (g_x if need[0] else None, g_x if (has_add and need[1]) else None, g_prompts, g_y,
                g_gamma if need[4] else None, g_beta if need[5] else None, None, None, None, None, None, g_cls, None)


def rowln(x, add=None, prompts=None, y=None, gamma=None, beta=None, mode=ROW_IDENTITY, P=0, u=None, keep=1.0, eps=1e-5, cls_add=None,
          ybias=None):
    """-> (rows (B,Lout,D), LayerNorm(rows) or None).  mode / P: see ROW_* and upp_rowln_fwd.
    ybias: optional (D) frozen bias added to y (the Linear that produced y then runs its GEMM bias-free).
    cls_add: optional (1,1,D) parameter that `add` (passed detached) carries in its row 0 for every sample; its gradient
    (batch sum of the row-0 input gradient) is produced here instead of through a (B,L,D) gradient of `add`."""
    if cls_add is not None and (add is None or add.requires_grad or mode not in (ROW_IDENTITY, ROW_INSERT_CLS)):
        raise ValueError("cls_add needs a detached `add` and a row map that keeps source row 0 in place")
    if ybias is not None and (y is None or (torch.is_grad_enabled() and ybias.requires_grad)):
        raise ValueError("ybias is the frozen bias of the Linear that produced y")
    xo, h = _RowLN.apply(x, add, prompts, y, gamma, beta, int(mode), int(P), u, float(keep), float(eps), cls_add, ybias)
    return xo, (h if gamma is not None else None)


def layer_norm(x, ln, last=None):
    """ln(x) -- or, with `last`, ln(x[:, -last:]) -- for an nn.LayerNorm over the last dimension of a (B,L,D) / (R,D) f32 HIP tensor on
    the row kernel of csrc/block.hip (upp_rowln_fwd: identity / strip row map, the normalised rows only); the module itself for anything
    else.  The prompting front-end calls it (reference models/Point_MAE_unify.py:588 `self.norm`, models/Point_MAE_pretask_dev.py:381
    the decoder's norm over the returned tokens): no torch kernel, no copy of the row window.  `last` needs a (B,L,D) input: on (R,D)
    it would mean the last ROWS on the kernel and the last COLUMNS on the module, so it raises on both."""
    if last is not None and x.dim() != 3:
        raise ValueError("layer_norm: `last` selects token rows of a (B, L, D) input, got %s" % (tuple(x.shape),))
    ok = (isinstance(ln, torch.nn.LayerNorm) and x.is_cuda and x.dtype == torch.float32 and x.dim() in (2, 3) and len(ln.normalized_shape) == 1
          and ln.normalized_shape[0] == x.shape[-1] and x.shape[-1] <= 512 and ln.elementwise_affine and ln.bias is not None and x.numel() > 0)
    if not ok:
        return ln(x if last is None else x[:, -last:])
    x3 = x if x.dim() == 3 else x.unsqueeze(0)
    L = x3.shape[1]
    strip = 0 if last is None else L - int(last)
    if strip < 0:
        raise ValueError("layer_norm: last = %d of %d rows" % (last, L))
    mode = ROW_STRIP if strip else ROW_IDENTITY
    if torch.is_grad_enabled() and (x.requires_grad or ln.weight.requires_grad or ln.bias.requires_grad):
        _, h = rowln(x3, gamma=ln.weight, beta=ln.bias, mode=mode, P=strip, eps=ln.eps)
    else:
        _, h, _, _ = ops.rowln_fwd(x3.contiguous(), None, None, mode, strip, None, None, 1.0, ln.weight, ln.bias, float(ln.eps), L - strip, want_xo=False)
    return h if x.dim() == 3 else h.squeeze(0)


class _Attention(Function):
    """ctx = softmax(q k^T * scale) v from the packed qkv projection (B, L, 3*H*64)."""

    @staticmethod
    def forward(ctx, qkv, num_heads, scale):
        qkv = qkv.contiguous()
        B, L, _ = qkv.shape
        out, lse = ops.attn_fwd(qkv, B, L, num_heads, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.meta = (B, L, num_heads, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, out, lse = ctx.saved_tensors
        B, L, H, scale = ctx.meta
        return ops.attn_bwd(qkv, out, g.contiguous(), lse, B, L, H, scale), None, None


ATTN_MAX_L = ops.ATTN_MAX_L


def attention(qkv, num_heads, scale):
    """softmax(q k^T scale) v per head on the FP32-MFMA attention kernels, head_dim 64, three families by sequence length:
    L <= 96 attn_flash16.hip (operands in registers), L <= 160 attn_long.hip (K and V resident in the LDS), L <= ATTN_MAX_L
    attn_stream.hip (64-row query blocks, K / V streamed in 64-key blocks, online softmax; the backward runs one kernel per key
    block for dK / dV and one per query block for dQ).  Deterministic at every L; longer sequences raise."""
    return _Attention.apply(qkv, int(num_heads), float(scale))


class _CrossAttention(Function):
    """ctx = softmax(q k^T * scale) v with q (B, Lq, H*64) and k, v (B, Lk, H*64) from two sequences, under the prefix-visibility mask
    (csrc/attn_stream.hip) when `splits` is (split_q, split_k) and not None; saves q, k, v, ctx and lse -- never a (B, H, Lq, Lk) or
    (L, L) tensor, mask included.  No scatter-add: deterministic in every mode."""

    @staticmethod
    def forward(ctx, q, k, v, num_heads, scale, splits):
        B, Lq, _ = q.shape
        Lk = k.shape[1]
        ctx.masked, ctx.meta = splits is not None, (B, Lq, Lk, num_heads, scale) + (splits or ())
        out, lse = (ops.xattn_prefix_fwd if ctx.masked else ops.xattn_fwd)(q, k, v, *ctx.meta)
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, out, lse = ctx.saved_tensors
        bwd = ops.xattn_prefix_bwd if ctx.masked else ops.xattn_bwd
        return bwd(q, k, v, out, g.contiguous(), lse, *ctx.meta) + (None, None, None)


def _xattn_view(t):
    """t as upp_xattn_* can read it (ops._xattn_operand): kept when it is a 16-byte aligned row-strided view, else a contiguous copy"""
    if t.dim() != 3:
        raise ValueError("cross_attention: q, k and v must be (B, L, H * 64)")
    B, L, C = t.shape
    rs = t.stride(1) if L > 1 else (t.stride(0) if B > 1 else C)
    ok = t.stride(2) == 1 and rs >= C and rs % 4 == 0 and (B <= 1 or t.stride(0) == L * rs) and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def cross_attention(q, k, v, num_heads, scale):
    """softmax(q k^T scale) v per head with queries and keys from two sequences (reference models/Transformer.py CrossAttention):
    q (B, Lq, H*64), k and v (B, Lk, H*64) -> (B, Lq, H*64), on the streaming FP32-MFMA kernels of csrc/attn_stream.hip, head_dim 64,
    1 <= Lq, Lk <= ATTN_MAX_L (HIP tensors outside that raise).  q, k, v may be row-strided views (slices of a packed product).
    Deterministic.  CPU tensors take the torch formulation when upp_hip.torch_cpu is enabled."""
    if _torch_cpu(q, k, v):
        from . import torch_cpu
        return torch_cpu.cross_attention(q, k, v, num_heads, scale)
    return _CrossAttention.apply(_xattn_view(q), _xattn_view(k), _xattn_view(v), int(num_heads), float(scale), None)


def prefix_attention(q, k, v, num_heads, scale, split_q, split_k):
    """cross_attention in which query rows < split_q see only the keys < split_k and the other rows see every key: the masked
    self-attention of AdaPoinTr's decoder over [real queries ; D denoising queries] (reference models/AdaPoinTr.py:217-229) with q, k, v
    the three views of one packed qkv and both splits L - D.  A hidden key's probability is exactly 0.  Shapes, views, range and
    determinism as cross_attention; 0 <= split_q <= Lq, 1 <= split_k <= Lk.  CPU tensors take the torch formulation when upp_hip.torch_cpu
    is enabled."""
    if _torch_cpu(q, k, v):
        from . import torch_cpu
        return torch_cpu.prefix_attention(q, k, v, num_heads, scale, split_q, split_k)
    return _CrossAttention.apply(_xattn_view(q), _xattn_view(k), _xattn_view(v), int(num_heads), float(scale), (int(split_q), int(split_k)))


# ------------------------------------------------------------------ deferred parameter-gradient sums
class _DeferredSums:
    """Parameter gradients that are sums of partial results (adapter weights, LayerNorm gamma/beta, prompts) are not read
    by anything inside a backward pass.  Inside `with deferred_sums(targets):` (TrainStep) their reductions are queued
    and run as ONE upp_batched_sum launch when the scope exits, ACCUMULATING straight into the gradient buffers the
    caller registered (targets: {parameter data_ptr: zero-initialised f32 buffer of the parameter's shape}); autograd is
    handed None for those parameters, so nothing depends on how it would have stored a returned tensor.  Parameters
    without a registered buffer, and everything outside a scope, are summed at once and returned as usual."""

    TALL = 4096

    def __init__(self):
        self.targets = None
        self.jobs = []
        self.wgrads = []
        self.adapters = []
        self.routed = set()

    def reduce(self, ptr, part, offset, length):
        """Sum columns [offset, offset+length) of the 2-D partial matrix `part` over its rows.
        -> (routed, tensor-or-None): routed sums appear in the registered buffer at scope exit."""
        if part.is_cuda and part.shape[0] > self.TALL and part.dtype == torch.float32 and part.stride(1) == 1:
            # one very tall matrix (a bias gradient over 65,536 point rows): first stage on many workgroups (a single column
            # sum of 64-column workgroups took 0.78 ms of the pre-training step)
            part, offset = ops.colsum_partials(part, offset, length), 0
        dst = self.targets.get(ptr) if (self.targets is not None and part.is_cuda) else None
        if dst is None or dst.numel() != length:
            if part.is_cuda and part.dtype == torch.float32 and part.dim() == 2 and part.stride(1) == 1:
                return False, ops.sum_rows(part, offset, length)                  # (never a torch reduction inside a step: ops.sum_rows)
            return False, part[:, offset:offset + length].sum(dim=0)
        self.jobs.append((part, offset, part.shape[0], length, part.stride(0), dst, True))
        self.routed.add(ptr)
        return True, None

    def _queue_wgrad(self, ptr, g2, x2, numel, window=None):
        """The registered buffer of the parameter at `ptr` (numel elements) -- or its `window` -- receives the partials of g2^T . x2 at scope
        exit.  -> True when queued (autograd is handed None), False when no such buffer is registered."""
        dst = self.targets.get(ptr) if (self.targets is not None and g2.is_cuda) else None
        if dst is None or dst.numel() != numel:
            return False
        self.wgrads.append((g2, x2, dst if window is None else window(dst)))
        self.routed.add(ptr)
        return True

    def wgrad(self, ptr, g2, x2):
        """Queue dW = g2^T . x2 for a parameter whose gradient buffer is registered: every weight gradient of the backward pass
        runs in ONE grouped launch at scope exit (upp_linear_wgrad_grouped_f32; a weight gradient is read by nothing inside the
        pass) and its partials are added to the buffer by the batched sum.  -> True when queued (autograd is handed None)."""
        return self._queue_wgrad(ptr, g2, x2, g2.shape[1] * x2.shape[1])

    def wgrad_rows(self, ptr, g2, x2, n_rows):
        """dW = (g2^T . x2)[:n_rows] for a parameter whose output was computed wider than it is (g2 has n_pad >= n_rows columns whose
        pad columns are zero): the partial tiles are (n_pad, K); only their first n_rows rows are summed into the buffer."""
        return n_rows <= g2.shape[1] and self._queue_wgrad(ptr, g2, x2, n_rows * x2.shape[1])

    def wgrad_window(self, w, g2, x2):
        """The same for a weight that is a COLUMN RANGE w = P[:, a:b] of a registered 2-D parameter P (the segmentation head's first layer
        multiplies [per-point | per-sample] column ranges of one weight; the feature propagation's first layer [xyz | features]): the
        partials are added into that range of P's gradient buffer (upp_batched_sum window destination) -- autograd is handed None, so the
        slice's backward (zero-fill of P's shape, strided copy, add) never runs.  -> True when queued."""
        root = w._base
        if root is None or w.dim() != 2 or w.stride(1) != 1 or not root.is_contiguous() or root.numel() % w.shape[0]:
            return False
        N, K = w.shape
        Kt = root.numel() // N                        # P viewed as (N, Kt): trailing singleton dimensions of a Conv1d weight fold away
        off = w.storage_offset() - root.storage_offset()
        if w.stride(0) != Kt or off < 0 or off + K > Kt or (g2.shape[1], x2.shape[1]) != (N, K):
            return False
        return self._queue_wgrad(root.data_ptr(), g2, x2, root.numel(), lambda dst: dst.view(N, Kt)[:, off:off + K])

    def adapter(self, ptrs, sizes, job):
        """Queue the weight gradients of one block's adapter (ptrs / sizes of W1, b1, W2, b2; job: see ops.adapter_wgrad_batched): formed
        from the per-row factors for every block of the backward pass in ONE launch at scope exit, instead of one partial matrix per
        16-row workgroup (153 MB per headline step through upp_batched_sum).  -> True when all four buffers are registered."""
        if self.targets is None:
            return False
        dsts = [self.targets.get(p_) for p_ in ptrs]
        if any(d is None or d.numel() != n for d, n in zip(dsts, sizes)):
            return False
        self.adapters.append((job, dsts))
        self.routed.update(ptrs)
        return True

    def flush(self):
        jobs, self.jobs = self.jobs, []
        wg, self.wgrads = self.wgrads, []
        ad, self.adapters = self.adapters, []
        if ad:
            for part, (_, dsts) in zip(ops.adapter_wgrad_batched([j for j, _ in ad]), ad):
                off = 0
                for dst in dsts:                                   # [dW1 | dW2 | db1 | db2], the order of `ptrs`: W1, W2, b1, b2
                    jobs.append((part, off, part.shape[0], dst.numel(), part.stride(0), dst, True))
                    off += dst.numel()
        if wg:
            for part, (_, _, dst) in zip(ops.linear_wgrad_grouped([(g, x) for g, x, _ in wg]), wg):
                n, full = dst.numel(), part[0].numel()                # (full > n: the pad rows of a wgrad_rows problem are not summed)
                jobs.append((part.view(part.shape[0], full), 0, part.shape[0], n, full, dst, True))
        ops.batched_sum(jobs)


_DEFERRED = _DeferredSums()


class deferred_sums:
    """Scope of one backward pass whose parameter-gradient partial sums are batched (see _DeferredSums)."""

    def __init__(self, targets):
        self.targets = targets
        self.routed = set()      # after exit: data_ptrs of the parameters whose buffers received sums

    def __enter__(self):
        if _DEFERRED.targets is not None:
            raise RuntimeError("deferred_sums scopes do not nest")
        _DEFERRED.targets = self.targets
        _DEFERRED.routed = set()
        return self

    def __exit__(self, *exc):
        _DEFERRED.targets = None
        self.routed = _DEFERRED.routed
        if exc[0] is None:
            _DEFERRED.flush()
        else:
            _DEFERRED.jobs = []
            _DEFERRED.wgrads = []
            _DEFERRED.adapters = []
        return False


# ------------------------------------------------------------------ FP32-MFMA Linear (upp_linear_f32)
_declined = set()


def note_declined(what, why):
    """A fused gfx950 path was not taken: say so ONCE per (site, reason) when UPP_VERBOSE is set -- the torch / library
    path that runs instead is correct but slower, and nothing else would show it."""
    key = (what, why)
    if key in _declined:
        return
    _declined.add(key)
    if os.environ.get("UPP_VERBOSE"):
        print("[upp_hip] %s: fused path declined (%s); running the torch / library formulation" % (what, why), file=sys.stderr)


class _TransposedWeights(_derived.DerivedWeights):
    """W^T copies for the data-gradient GEMMs (dX = dY . W is upp_linear_f32(dY, W^T)): the _derived.DerivedWeights (protocol and CONTRACT
    there) of any owner's FROZEN weights, in buffers whose rows are zero-padded to a multiple of 4 (get_padded), and of a step driver's
    trainable weights -- all refreshed by ONE batched launch per step (the pre-training recipe transposed 71 weights one by one: 0.36 ms).
    A trainable entry's tag is the padded width of get_trainable_padded (False: the plain W^T)."""

    def __init__(self):
        super().__init__("W^T copy", self._make, lambda w, wt, tag: wt.copy_(w.detach().t()), _derived.any_owner, self._refill_batched)

    trainable_anchor = staticmethod(lambda w: w)       # (a step driver's copy lives as long as the tensor it was made for, window or not)

    @staticmethod
    def _make(w, n_pad):
        N, K = w.shape
        if n_pad is not None:                          # a step driver's copy, on the transpose kernel
            if not n_pad:
                return ops.transpose(w)
            full = torch.zeros((K, n_pad), dtype=w.dtype, device=w.device)
            ops.transpose(w, out=full[:, :N])
            return full
        full = torch.zeros(((K + 3) // 4 * 4, N), dtype=w.dtype, device=w.device)        # rows padded to a multiple of 4: get_padded()
        full._upp_persistent = True            # (ops.PLANES may keep the bf16 plane image of this copy: it lives as long as the entry)
        full[:K].copy_(w.detach().t())
        return full[:K]

    @staticmethod
    def _refill_batched(jobs):
        pairs = [(w, wt) for w, wt, n_pad in jobs if not n_pad and w.is_contiguous()]
        ops.transpose_batched(pairs)
        for w, wt, n_pad in jobs:              # column windows of a parameter (rows not contiguous as a whole), padded copies: one launch each
            if n_pad or not w.is_contiguous():
                ops.transpose(w, out=wt[:, :w.shape[0]])

    def get_padded(self, w):
        """W^T with zero rows up to a multiple of 4 (K, ceil4(K) x N): the B operand of a data-gradient GEMM whose output width K is
        not a multiple of 4 (K = 3: the first layer of a position MLP whose input carries a gradient); same storage as get(w)."""
        return self.get(w)._base

    def get_trainable_padded(self, w, n_pad):
        """W^T of a trainable (N,K) weight as the first N columns of a persistent zero-initialised (K, n_pad) matrix (n_pad >= N): the B
        operand of the data gradient of a Linear layer whose OUTPUT was computed n_pad columns wide (the 50-class layer of the segmentation
        head in a 52-column matrix: _LinearPadN).  Refreshed with the other copies by refresh_trainable."""
        return self.get_trainable(w, tag=int(n_pad))


TRANSPOSED = _TransposedWeights()


def managed_weights(transposes=True, planes=True, owners=None):
    """Scope of a step driver (train.TrainStep, the captured evaluation steps): inside it trainable weights are multiplied through
    persistent W^T copies / bf16 plane images, refreshed here -- transposes, then planes, one launch each -- for the parameters in
    `owners` (a set of id()s; None: all)."""
    return _derived.managed(([TRANSPOSED] if transposes else []) + ([ops.PLANES] if planes else []), owners)


def refresh_caches(model=None):
    """Bring every derived copy of FROZEN weights up to date IN PLACE after weights were loaded into a model whose training step is
    already captured in a HIP graph (load_state_dict changes contents, not addresses; the captured launches read the copies):
    the zero-padded first-conv weight of every patch-embedding Encoder, then the W^T copies of the data-gradient GEMMs (which
    include the transposes of those padded weights -- hence the order), then the bf16 plane images of both.
    Also REQUIRED after any write to a frozen weight that bypasses torch's version counter (`p.data.copy_()`, `p.data.mul_()`, an EMA
    update through `.data`, a custom kernel): the caches key their validity on that counter and cannot see such a write."""
    if model is not None:
        for m in model.modules():
            if hasattr(m, 'refresh_padded_weight'):
                m.refresh_padded_weight()
    TRANSPOSED.refresh()
    ops.PLANES.refresh()              # (after the transposes: the plane images of W^T copies are split from the refreshed copies)


def _wt(w):
    """W^T (K,N) contiguous: cached for frozen weights, a fresh upp_transpose_f32 copy for trainable ones (they change every step)."""
    if w.requires_grad:
        if not (w.is_cuda and w.stride(1) == 1):
            return w.detach().t().contiguous()
        return TRANSPOSED.get_trainable(w) if TRANSPOSED.managed else ops.transpose(w.detach())
    return TRANSPOSED.get(w)


def linear_usable(x, weight):
    """upp_linear_f32 serves f32 HIP operands with 16-byte aligned rows (contraction length a multiple of 4)."""
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.dim() == 2 and _aligned(weight)
            and x.shape[-1] == weight.shape[1] and weight.shape[1] % 4 == 0 and x.numel() > 0)


# -- what the backward passes of the Linear nodes share
_aligned = ops.aligned_rows


def _rows(g):
    """g (..., N) as a contiguous (rows, N) matrix."""
    g2 = g.reshape(-1, g.shape[-1])
    return g2 if g2.is_contiguous() else g2.contiguous()


def _smallk_dgrad(g2, w):
    """dX = g2 . W of a small-K layer: the small kernel on a fresh transpose; over more than 64 outputs (_smallk_with_grad: N % 4 == 0 and
    a frozen weight then) the contraction is too long for it -- the matrix cores, with W^T zero-padded to 4 output columns."""
    if w.shape[0] > 64:
        return ops.linear_f32(g2, TRANSPOSED.get_padded(w))[:, :w.shape[1]]
    return ops.linear_smallk(g2, ops.transpose(w.detach()) if w.requires_grad else w.detach().t().contiguous(), None, 0)


def _smallk_wgrad(ptr, g2, x, N, K):
    """dW (N,K) = g2^T . x on upp_linear_smallk_wgrad_f32 partials, summed by the deferred sums (None: into the buffer registered for ptr)."""
    x2 = x.reshape(-1, K)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    part = ops.linear_smallk_wgrad(g2, x2)
    _, gw = _DEFERRED.reduce(ptr, part.view(part.shape[0], N * K), 0, N * K)
    return None if gw is None else gw.view(N, K)


def _colsum(ptr, g2):
    """A bias gradient: the column sums of g2 through the deferred sums (None: into the buffer registered for ptr)."""
    return _DEFERRED.reduce(ptr, g2, 0, g2.shape[1])[1]


def _sum_splits(part):
    """(splits, N, K) partial weight gradients summed NOW, in split order, on ops.sum_rows (never a torch reduction inside a step)."""
    return ops.sum_rows(part.view(part.shape[0], -1)).view(part.shape[1:]) if part.shape[0] > 1 else part[0]


def _lin(a, w, bias=None, epi=None, aux=None, dgrad=False):
    """a . op(w)^T with op(w) = w (N,K) -- or, dgrad, w^T: the data gradient dX = dY . W -- on the kernel that serves the weight:
    frozen -> upp_linear_sb_f32 on the cached plane image of w / of its cached transpose (exact-f32 kernel where the split kernel does not
    take the shape); trainable inside a step driver (ops.PLANES.managed) -> upp_linear_sb_f32 on the persistent image that the driver
    re-splits once per step, the transpose read straight from w; trainable elsewhere -> the exact-f32 kernel (a fresh W^T for dgrad)."""
    epi = ops.LIN_NONE if epi is None else epi
    if not w.requires_grad:
        return ops.linear_f32(a, _wt(w) if dgrad else w, bias, epi, aux=aux, frozen=True)
    N, K = (w.shape[1], w.shape[0]) if dgrad else w.shape
    M = a.numel() // a.shape[-1]
    # (the plane image is a buffer of its own, written by upp_linear_sb_prep with scalar reads of w: a column window of a wider weight whose
    #  rows start off a 16-byte boundary -- w[:, 3:] of a (1536, 1155) weight -- is served where it lies)
    if (ops.PLANES.managed and w.is_cuda and w.dim() == 2 and w.stride(1) == 1
            and ops.linear_sb_usable(M, N, K) and (bias is None or bias.data_ptr() % 16 == 0)):
        return ops.linear_f32(a, None, bias, epi, aux=aux, planes=ops.PLANES.get_trainable(w, transposed=dgrad), wshape=(N, K))
    return ops.linear_f32(a, _wt(w) if dgrad else w, bias, epi, aux=aux)


class _LinearMFMA(Function):
    """x . W^T (+ b) on upp_linear_f32, forward and data gradient.  The weight gradient of a TRAINABLE layer is a library GEMM
    (not on the PEFT hot path: the Transformer weights are frozen there); a trainable bias takes the deferred column sum."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x if w.requires_grad else None, w)
        ctx.bias_ptr = b.data_ptr() if b is not None else 0
        return _lin(x, w, b, ops.LIN_BIAS if b is not None else ops.LIN_NONE)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2 = _rows(g)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if w.shape[0] % 4 == 0 and g2.stride(0) % 4 == 0:
                gx = _lin(g2, w, dgrad=True).view(g.shape[:-1] + (w.shape[1],))
            elif w.shape[0] <= 64 and w.shape[1] <= 256:
                # a narrow layer (the 64 -> 3 score head of the denoising prompter): the data gradient contracts over its few outputs
                gx = ops.linear_smallk(g2, _wt(w), None, 0).view(g.shape[:-1] + (w.shape[1],))
            else:
                note_declined("linear data gradient", "N = %d is not a multiple of 4" % w.shape[0])
                gx = torch.mm(g2, w).view(g.shape[:-1] + (w.shape[1],))
        if ctx.needs_input_grad[1]:
            gw = weight_grad(g2, x.reshape(-1, x.shape[-1]), w)
        if b_needed(ctx):
            gb = _colsum(ctx.bias_ptr, g2)
        return gx, gw, gb


def weight_grad(g2, x2, w):
    """dW = g2^T . x2 for the trainable weight w (N,K) on upp_linear_wgrad_grouped_f32: inside a training step the pair is queued
    and every weight gradient of the backward pass runs in one launch at the end, its partials summed in split order straight
    into w's slot of the flat gradient buffer (then None is returned); otherwise a group of one, summed at once."""
    N, K = g2.shape[1], x2.shape[1]
    if N % 4 or K % 4 or not g2.is_cuda:
        if N * K <= 2048 and N + K <= 512 and x2.stride(1) == 1 and g2.stride(1) == 1 and g2.is_cuda:
            return _smallk_wgrad(w.data_ptr(), g2, x2, N, K)
        if g2.is_cuda:
            note_declined("linear weight gradient (%d,%d)" % (N, K), "N % 4 / K % 4")
        return torch.mm(g2.t(), x2)
    if not _aligned(g2):                                                      # (a misaligned view: one copy makes it servable)
        g2 = g2.contiguous()
    if not _aligned(x2):
        x2 = x2.contiguous()
    if _DEFERRED.wgrad(w.data_ptr(), g2, x2) or _DEFERRED.wgrad_window(w, g2, x2):
        return None
    return _sum_splits(ops.linear_wgrad(g2, x2))


def b_needed(ctx):
    return len(ctx.needs_input_grad) > 2 and ctx.needs_input_grad[2]


class _LinearSmallK(Function):
    """x . W^T + b for the layers upp_linear_f32 does not take (K not a multiple of 4 or unaligned rows; K <= 64, N <= 256) WITH a
    gradient: forward upp_linear_smallk_f32, data gradient the same kernel on W^T (contraction over N <= 64), weight gradient
    upp_linear_smallk_wgrad_f32 partials, bias gradient a (two-stage) column sum -- all through the deferred sums of a step driver.
    (The rectify prompter's point-wise layers in the pre-task recipe and stage 2: K = 3, 27, 59.)"""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x if w.requires_grad else None, w)
        ctx.ptrs = (w.data_ptr(), b.data_ptr() if b is not None else 0)
        return ops.linear_smallk(x, w, b, 0)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        N, K = w.shape
        g2 = _rows(g)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _smallk_dgrad(g2, w).reshape(g.shape[:-1] + (K,))
        if ctx.needs_input_grad[1]:
            gw = _smallk_wgrad(ctx.ptrs[0], g2, x, N, K)
        if ctx.needs_input_grad[2]:
            gb = _colsum(ctx.ptrs[1], g2)
        return gx, gw, gb


class _LinearGroupBias(Function):
    """x (M,K) . W^T + gb[m // rows] with the per-group term added in the GEMM's epilogue (upp_linear_group_bias_f32).  Backward: the data
    gradient and the (deferred, grouped) weight gradient of _LinearMFMA; the group term's gradient is the sum of g over each group's rows."""

    @staticmethod
    def forward(ctx, x, w, gb, rows):
        ctx.save_for_backward(x if w.requires_grad else None, w)
        ctx.rows = rows
        if w.requires_grad and ops.PLANES.managed and ops.linear_sb_usable(x.shape[0], w.shape[0], w.shape[1]) and _aligned(w):
            return ops.linear_group_bias(x, w, gb, rows, planes=ops.PLANES.get_trainable(w))
        return ops.linear_group_bias(x, w, gb, rows, frozen=not w.requires_grad)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2 = _rows(g)
        gx = gw = ggb = None
        if ctx.needs_input_grad[0]:
            gx = _lin(g2, w, dgrad=True)
        if ctx.needs_input_grad[1]:
            gw = weight_grad(g2, x, w)
        if ctx.needs_input_grad[2]:
            groups = g2.shape[0] // ctx.rows
            if g2.is_cuda and g2.dtype == torch.float32 and groups * ctx.rows == g2.shape[0] and 1 <= groups <= 65535:
                ggb = ops.colsum_partials(g2, 0, g2.shape[1], chunks=groups)        # chunk = group: (groups, N) in one launch, wave-ordered sums
            else:
                ggb = g2.view(groups, ctx.rows, g2.shape[1]).sum(dim=1)
        return gx, gw, ggb, None


class _GroupBiasAdd(Function):
    """y (M,N) + gb[m // rows]: the broadcast add of linear_group_bias when the GEMM cannot take the term in its epilogue (few rows).
    As its own node so that the group term's gradient is upp_colsum_partials (chunk = group) and not torch's sum over the rows of a
    group -- a reduction that splits 2,048 rows over workgroups and zeroes its semaphores with a memset: inside a captured step that
    node is right in the first replay only (NOTEBOOK 12.11; the B = 4 segmentation step of tests/test_gpu_determinism.py)."""

    @staticmethod
    def forward(ctx, y, gb, rows):
        ctx.rows = rows
        M, N = y.shape
        return (y.view(M // rows, rows, N) + gb.unsqueeze(1)).view(M, N)

    @staticmethod
    def backward(ctx, g):
        g2 = g if g.is_contiguous() else g.contiguous()
        ggb = ops.colsum_partials(g2, 0, g2.shape[1], chunks=g2.shape[0] // ctx.rows) if ctx.needs_input_grad[1] else None
        return (g2 if ctx.needs_input_grad[0] else None), ggb, None


class _ExpandRows(Function):
    """token (1,1,D) or (D,) -> (B, N, D) (the mask token of the MAE decoders: `mask_token.expand(B, N, -1)`), with the backward's sum
    over the B N rows on this library's kernels (and routed into the step driver's deferred sums): torch's sum over 1,024 ... 1,216 rows
    per column splits them over workgroups behind a memset -- see _GroupBiasAdd."""

    @staticmethod
    def forward(ctx, token, B, N):
        ctx.ptr, ctx.shape = token.data_ptr(), tuple(token.shape)
        return token.reshape(1, 1, -1).expand(B, N, -1)

    @staticmethod
    def backward(ctx, g):
        D = g.shape[-1]
        g2 = g.reshape(-1, D)
        g2 = g2 if g2.is_contiguous() else g2.contiguous()
        if not (g2.is_cuda and g2.dtype == torch.float32):
            return g2.sum(dim=0).view(ctx.shape), None, None
        routed, gt = _DEFERRED.reduce(ctx.ptr, g2, 0, D)
        return (None if routed else gt.view(ctx.shape)), None, None


def expand_rows(token, B, N):
    """token.expand(B, N, -1) whose gradient is summed by this library's kernels (see _ExpandRows)."""
    if token.is_cuda and torch.is_grad_enabled() and token.requires_grad:
        return _ExpandRows.apply(token, int(B), int(N))
    return token.reshape(1, 1, -1).expand(B, N, -1)


def linear_group_bias(x, weight, group_bias, rows_per_group):
    """F.linear(x, weight) + group_bias.repeat_interleave(rows_per_group, 0) for a (M,K) matrix x whose rows come in groups of
    `rows_per_group` (a power of two >= 32) that share one bias row: in the GEMM's epilogue when the problem is tall enough for the
    register-tiled kernel, as a broadcast add otherwise."""
    M, K = x.shape
    N = weight.shape[0]
    r = int(rows_per_group)
    if (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and _aligned(x) and _aligned(weight)
            and (K % 4 == 0 and weight.shape[1] == K) and ops.linear_group_bias_usable(M, N, K, r)
            and (not (torch.is_grad_enabled() and x.requires_grad) or K % 4 == 0)):
        gb = group_bias.contiguous()
        if not torch.is_grad_enabled() or not (x.requires_grad or weight.requires_grad or gb.requires_grad):
            return ops.linear_group_bias(x, weight, gb, r, frozen=not weight.requires_grad)
        return _LinearGroupBias.apply(x, weight, gb, r)
    y = linear(x, weight)
    if y.is_cuda and y.dtype == torch.float32 and M % r == 0 and 1 <= M // r <= 65535 and torch.is_grad_enabled() and group_bias.requires_grad:
        return _GroupBiasAdd.apply(y, group_bias, r)
    return (y.view(M // r, r, N) + group_bias.unsqueeze(1)).view(M, N)


def _smallk_with_grad(x, weight):
    """(the data gradient contracts over N on the same kernel: N <= 64 unless the input needs none -- the 3 -> 128 first layer of a
    trainable position MLP reads the centres)"""
    N, K = weight.shape
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.dim() == 2 and x.shape[-1] == K
            and K <= 64 and (N <= 64 or (N <= 256 and (not x.requires_grad or (N % 4 == 0 and not weight.requires_grad))))
            and N * K <= 2048 and N + K <= 512 and x.numel() > 0
            and weight.stride(1) == 1)


_ACT_EPI = {None: (ops.LIN_BIAS, 0), 'relu': (ops.LIN_BIAS_RELU, 1), 'gelu': (ops.LIN_BIAS_GELU, 2)}


def _act_torch(y, act):
    return y if act is None else (F.relu(y) if act == 'relu' else F.gelu(y))


def linear(x, weight, bias=None, act=None):
    """act(F.linear(x, weight, bias)) on this library's kernels: upp_linear_f32 (FP32 matrix cores) for 16-byte aligned rows and
    K % 4 == 0, upp_linear_smallk_f32 (K <= 64, N <= 256, forward only) for the rest; otherwise the library GEMM (said once under
    UPP_VERBOSE).  act: None / 'relu' / 'gelu' (erf) -- fused into the epilogue when nothing needs a gradient, applied by torch
    otherwise."""
    needs_grad = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad))
    if (x.is_cuda and weight.dim() == 2 and weight.dtype == torch.float32 and weight.shape[1] % 4 == 0 and weight.shape[1] > 64
            and not _aligned(weight)):
        # a column window of a wider weight whose rows start off a 16-byte boundary (w[:, 3:] of the (1536, 1155) first layer of the
        # segmentation head's feature propagation): inside a step driver a trainable window of a parameter is multiplied through its
        # persistent bf16 plane image and its gradient lands in the parameter's gradient window (_DeferredSums.wgrad_window) -- no copy;
        # anywhere else one differentiable copy makes it servable
        rows = x.numel() // max(x.shape[-1], 1)
        window_ok = bool(needs_grad and weight.requires_grad and ops.PLANES.managed and weight.stride(1) == 1 and x.dtype == torch.float32
                         and isinstance(weight._base, torch.nn.Parameter) and x.shape[-1] == weight.shape[1] and weight.shape[0] % 4 == 0
                         and ops.linear_sb_usable(rows, weight.shape[0], weight.shape[1])
                         and (not x.requires_grad or ops.linear_sb_usable(rows, weight.shape[1], weight.shape[0])))
        if window_ok:
            return _act_torch(_LinearMFMA.apply(x, weight, bias), act)
        weight = weight.contiguous()
    if needs_grad and weight.dim() == 2 and weight.shape[0] % 4 and weight.shape[0] > 16 and linear_usable(x, weight):
        # the data gradient contracts over the N outputs and the weight gradient is (N, K): both want N % 4 == 0 (the 50 part classes of
        # the segmentation head's last layer).  Zero rows up to the next multiple of 4 -- their outputs are sliced off, their gradient
        # rows are dropped by the pad's backward -- keep forward and both gradients on our kernels.
        pad = -weight.shape[0] % 4
        y = linear(x, F.pad(weight, (0, 0, 0, pad)), None if bias is None else F.pad(bias, (0, pad)), act)
        return y[..., :weight.shape[0]]
    if not linear_usable(x, weight):
        if (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.dim() == 2 and x.shape[-1] == weight.shape[1]
                and weight.shape[1] <= 64 and weight.shape[0] <= 256 and x.numel() > 0 and not needs_grad):
            return ops.linear_smallk(x, weight, bias, _ACT_EPI[act][1])
        if needs_grad and _smallk_with_grad(x, weight):
            return _act_torch(_LinearSmallK.apply(x, weight, bias), act)
        if x.is_cuda:
            note_declined("linear %s x %s" % (tuple(x.shape), tuple(weight.shape)), "dtype / layout / K % 4" + (" with a gradient" if needs_grad else ""))
        return _act_torch(F.linear(x, weight, bias), act)
    if not needs_grad:
        if act is not None and bias is None:
            bias = _zero_bias(weight)
        return ops.linear_f32(x, weight, bias, _ACT_EPI[act][0] if bias is not None else ops.LIN_NONE, frozen=not weight.requires_grad)
    return _act_torch(_LinearMFMA.apply(x, weight, bias), act)


_ZERO_BIAS = {}


def _zero_bias(weight):
    key = (weight.device, weight.shape[0])
    z = _ZERO_BIAS.get(key)
    if z is None:
        z = _ZERO_BIAS[key] = torch.zeros(weight.shape[0], dtype=torch.float32, device=weight.device)
    return z


class _MlpGelu(Function):
    """fc2( GELU( fc1(x) + b1 ) ) (+ b2) (reference models/Point_MAE_pretask_dev.py:163-168):
    two upp_linear_f32 launches forward (the first carries bias + GELU and stores GELU'), two backward for the data gradient (the
    data gradient of fc2 is multiplied by the saved GELU' in its epilogue, i.e. it IS the gradient at the fc1 pre-activation).
    Frozen weights (the PEFT recipe): the hidden activation is not kept.  Trainable weights (Point-MAE pre-training): it is, and
    dW2 = g^T hid, dW1 = g_z^T x, db1 = column sum of g_z, db2 = column sum of g follow weight_grad / the deferred sums."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2=None):
        hid, d = _lin(x, w1, b1, ops.LIN_BIAS_GELU_D)
        train = w1.requires_grad or w2.requires_grad or b1.requires_grad
        ctx.save_for_backward(d, w1, w2, x if train else None, hid if w2.requires_grad else None)
        ctx.bias_ptrs = (b1.data_ptr(), b2.data_ptr() if b2 is not None else 0)
        return _lin(hid, w2, b2, ops.LIN_BIAS if b2 is not None else ops.LIN_NONE)

    @staticmethod
    def backward(ctx, g):
        d, w1, w2, x, hid = ctx.saved_tensors
        need = ctx.needs_input_grad
        g2 = _rows(g)
        g_z = _lin(g2, w2, None, ops.LIN_MUL, aux=d.view(-1, d.shape[-1]), dgrad=True)
        gx = None
        if need[0]:
            gx = _lin(g_z, w1, dgrad=True).view(g.shape[:-1] + (w1.shape[1],))
        gw1 = gb1 = gw2 = gb2 = None
        if need[1]:
            gw1 = weight_grad(g_z, x.reshape(-1, x.shape[-1]), w1)
        if need[2]:
            gb1 = _colsum(ctx.bias_ptrs[0], g_z)
        if need[3]:
            gw2 = weight_grad(g2, hid.reshape(-1, hid.shape[-1]), w2)
        if len(need) > 4 and need[4]:
            gb2 = _colsum(ctx.bias_ptrs[1], g2)
        return gx, gw1, gb1, gw2, gb2


# (round 5's residual + LayerNorm fold -- residual add + row-block statistics in the projection GEMM's epilogue, LayerNorm in fc1's A-prologue --
# was measured slower than the row kernel it removed (profiles/r05_fold_ab.txt: 4.63-4.66 against 4.55-4.59 ms per step) and left the library
# with ABI 5; NOTEBOOK section 11.3 keeps the account.)


class _MlpSmallKGelu(Function):
    """lin2(GELU(lin1(x))) for a first layer the small-K kernel serves (K <= 64: the 3 -> 128 layer of a position MLP, reference
    models/Point_MAE_pretask_dev.py:395-399) WITH gradients: GELU and GELU' come out of the first launch (upp_linear_smallk_gelu_d_f32), the
    data gradient of the second layer is multiplied by the saved GELU' in its epilogue -- no torch gelu / gelu_backward pair.  Weight and
    bias gradients as _LinearSmallK / _LinearMFMA (deferred sums inside a step driver)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        hid, d = ops.linear_smallk_gelu_d(x, w1, b1)
        ctx.save_for_backward(x if (w1.requires_grad or x.requires_grad) else None, w1, w2, d, hid if w2.requires_grad else None)
        ctx.ptrs = (w1.data_ptr(), b1.data_ptr() if b1 is not None else 0, b2.data_ptr() if b2 is not None else 0)
        return _lin(hid, w2, b2, ops.LIN_BIAS if b2 is not None else ops.LIN_NONE)

    @staticmethod
    def backward(ctx, g):
        x, w1, w2, d, hid = ctx.saved_tensors
        need = ctx.needs_input_grad
        H, K = w1.shape
        g2 = _rows(g)
        g_z = _lin(g2, w2, None, ops.LIN_MUL, aux=d.view(-1, H), dgrad=True)                 # (rows, H) = gradient at the pre-activation
        gx = gw1 = gb1 = gw2 = gb2 = None
        if need[0]:
            gx = _smallk_dgrad(g_z, w1).reshape(g.shape[:-1] + (K,))
        if need[1]:
            gw1 = _smallk_wgrad(ctx.ptrs[0], g_z, x, H, K)
        if need[2]:
            gb1 = _colsum(ctx.ptrs[1], g_z)
        if need[3]:
            gw2 = weight_grad(g2, hid.reshape(-1, H), w2)
        if need[4]:
            gb2 = _colsum(ctx.ptrs[2], g2)
        return gx, gw1, gb1, gw2, gb2


def mlp_smallk_gelu_usable(x, w1, b1, w2, b2):
    """Can _MlpSmallKGelu serve lin2(GELU(lin1(x)))?  The first layer is the small-K kernel's (with the gradient rules of _smallk_with_grad:
    a trainable first weight of more than 64 outputs only when x needs no gradient), its bias exists, the second layer is the matrix-core
    kernels' and the hidden width allows a small-K weight gradient."""
    H = w1.shape[0]
    return (_smallk_with_grad(x, w1) and b1 is not None and H % 4 == 0 and H * w1.shape[1] <= 2048 and w2.dim() == 2 and w2.shape[1] == H
            and w2.dtype == torch.float32 and _aligned(w2) and w2.shape[0] % 4 == 0
            and (b2 is None or b2.data_ptr() % 16 == 0))


def mlp_smallk_gelu(x, w1, b1, w2, b2):
    return _MlpSmallKGelu.apply(x, w1, b1, w2, b2)


def mlp_gelu(x, w1, b1, w2, b2=None):
    """fc2(GELU(fc1(x) + b1)) (+ b2); both GEMMs and the activation on the Linear kernels (split-bf16 for frozen / managed weights)."""
    if not torch.is_grad_enabled() or not (x.requires_grad or w1.requires_grad or w2.requires_grad or b1.requires_grad
                                           or (b2 is not None and b2.requires_grad)):
        hid = ops.linear_f32(x, w1, b1, ops.LIN_BIAS_GELU, frozen=not w1.requires_grad)
        return ops.linear_f32(hid, w2, b2, ops.LIN_BIAS if b2 is not None else ops.LIN_NONE, frozen=not w2.requires_grad)
    return _MlpGelu.apply(x, w1, b1, w2, b2)


# ------------------------------------------------------------------ prompt propagation
class _PropPool(Function):
    """X (B,L',D), absolute neighbour rows i1 (B*G2*8) -> max_k + mean_k of the (drop-path scaled) rows, (B*G2, D)."""

    @staticmethod
    def forward(ctx, X, i1, u, keep):
        X = X.contiguous()
        groups = i1.numel() // 8
        pooled, amax = ops.prop_pool_fwd(X, i1, u, keep, groups)
        ctx.save_for_backward(amax, i1, u)
        ctx.meta = (keep, X.shape)
        return pooled

    @staticmethod
    def backward(ctx, g):
        amax, i1, u = ctx.saved_tensors
        keep, shape = ctx.meta
        return ops.prop_pool_bwd(g.contiguous(), amax, i1, u, keep, shape[0] * shape[1]).view(shape), None, None, None


class _PropInterp(Function):
    """X (B,L',D), lc (B,G2,D) -> X with its last T rows += 0.3 * sum_k w8 * (lc + 0.3 * X[i2])[idx8].  w8 may carry a gradient."""

    @staticmethod
    def forward(ctx, X, lc, i2, idx8, w8):
        X, lc = X.contiguous(), lc.contiguous()
        B, Lp, D = X.shape
        T, G2 = idx8.shape[1], lc.shape[1]
        w8 = w8.contiguous()
        ctx.save_for_backward(i2, idx8, w8, *((X, lc) if ctx.needs_input_grad[4] else ()))
        ctx.meta = (B, Lp, T, G2)
        return ops.prop_interp_fwd(X, lc, i2, idx8, w8, B, Lp, T, G2)

    @staticmethod
    def backward(ctx, g):
        i2, idx8, w8 = ctx.saved_tensors[:3]
        B, Lp, T, G2 = ctx.meta
        g = g.contiguous()
        g_c2, g_X = ops.prop_interp_bwd(g, i2, idx8, w8, B, Lp, T, G2)
        g_w8 = None
        if ctx.needs_input_grad[4]:
            X, lc = ctx.saved_tensors[3:]
            g_w8 = ops.prop_w8_grad(g, X, lc, None, i2, idx8, B, Lp, T, G2)
        return g_X, g_c2.view(B, G2, -1), None, None, g_w8


def prop_pool(X, i1, u=None, keep=1.0):
    return _PropPool.apply(X, i1, u, float(keep))


def prop_interp(X, lc, i2, idx8, w8):
    return _PropInterp.apply(X, lc, i2, idx8, w8)


class PropIndex:
    """Index lists of the propagation step for one forward (they depend only on the centres): absolute neighbour rows
    i1 (groups*8), level-2 centre rows i2 (groups), interpolation neighbours idx8 / weights w8 (B,T,8), and their inverses
    (CSR) for the backward kernels.  Built once per forward and shared by every block."""

    def __init__(self, i1, i2, idx8, w8, rows, csr=None):
        B, T = idx8.shape[0], idx8.shape[1]
        groups = i2.numel()
        self.i1, self.i2, self.idx8, self.w8 = i1, i2, idx8, w8
        self.B, self.T, self.G2, self.rows = B, T, groups // B, rows
        if csr is None:
            self.csr1 = ops.csr_build(i1, rows)
            self.csr2 = ops.csr_build(i2, rows)
            self.csr8 = ops.csr_build(idx8.view(-1), groups, seg_len=T * 8, seg_rows=groups // B)
        else:
            self.csr1, self.csr2, self.csr8 = csr

    def tensors(self):
        """The ten tensors of the index (for handing it from one HIP graph to another through static buffers)."""
        return (self.i1, self.i2, self.idx8, self.w8) + self.csr1 + self.csr2 + self.csr8

    @classmethod
    def from_tensors(cls, t, rows):
        return cls(t[0], t[1], t[2], t[3], rows, csr=((t[4], t[5]), (t[6], t[7]), (t[8], t[9])))


class _PropWeights(Function):
    """The interpolation weights of a PropIndex as a differentiable function of the centres (stage 2 of the recipe: the point cloud, and so
    the centres, carry a gradient back to the prompters).  Forward: the weights the index kernel computed (the reference's sort + 1/(d+eps)
    normalisation, models/Point_MAE_unify.py:33-44); backward: upp_prop_weights_bwd.  The neighbour choice idx8 is piecewise constant."""

    @staticmethod
    def forward(ctx, c1, c2, idx8, w8, eps):
        ctx.save_for_backward(c1, c2, idx8)
        ctx.eps = eps
        return w8.clone()

    @staticmethod
    def backward(ctx, g):
        c1, c2, idx8 = ctx.saved_tensors
        g1, g2 = ops.prop_weights_bwd(c1.contiguous(), c2.contiguous(), idx8, g.contiguous(), ctx.eps)
        return g1, g2, None, None, None


def prop_weights(c1, c2, index, eps=1e-3):
    """index.w8 with the autograd edge to the centres c1 (B,T,3) / c2 (B,G2,3) it was built from."""
    return _PropWeights.apply(c1, c2, index.idx8, index.w8, float(eps))


class _Propagate(Function):
    """Fused pool -> BatchNorm1d -> interpolate of one block (upp_prop_fwd / upp_prop_bwd; upp_prop_w8_grad when w8 carries a gradient)."""

    @staticmethod
    def forward(ctx, X, gamma, beta, index, u, keep, running_mean, running_var, momentum, eps, training, w8):
        X = X.contiguous()
        B, Lp, D = X.shape
        w8 = w8.contiguous()
        out, pooled, amax, mean, rstd = ops.prop_fwd(X, index.i1, u, keep, index.i2, index.idx8, w8, gamma, beta, running_mean,
                                                     running_var, momentum, eps, training, B, Lp, index.T, index.G2)
        ctx.save_for_backward(pooled, amax, mean, rstd, gamma, u, w8, *((X, beta) if ctx.needs_input_grad[11] else ()))
        ctx.meta = (index, keep, training, B, Lp)
        return out

    @staticmethod
    def backward(ctx, g):
        pooled, amax, mean, rstd, gamma, u, w8 = ctx.saved_tensors[:7]
        index, keep, training, B, Lp = ctx.meta
        g = g.contiguous()
        g_X, g_gamma, g_beta = ops.prop_bwd(g, pooled, amax, mean, rstd, gamma, u, keep, w8, index.csr1, index.csr2,
                                            index.csr8, training, B, Lp, index.T, index.G2)
        g_w8 = None
        if ctx.needs_input_grad[11]:
            X, beta = ctx.saved_tensors[7:]
            g_w8 = ops.prop_w8_grad(g, X, pooled, (mean, rstd, gamma, beta), index.i2, index.idx8, B, Lp, index.T, index.G2)
        return (g_X, g_gamma, g_beta) + (None,) * 8 + (g_w8,)


def propagate(X, bn, index, u=None, keep=1.0, training=True, w8=None):
    """X (B,L',D) -> X with its last T rows += 0.3 * interp(bn(pool(X)) + 0.3 * X[i2]); bn: nn.BatchNorm1d (affine).
    w8: the interpolation weights when they carry a gradient (prop_weights), default index.w8 (constants of the forward).
    Limits: propagate_usable."""
    use_batch, momentum = _bn_mode(bn, training)
    return _Propagate.apply(X, bn.weight, bn.bias, index, u, float(keep), bn.running_mean, bn.running_var, momentum, bn.eps, use_batch,
                            index.w8 if w8 is None else w8)


def _bn_momentum(bn, use_batch):
    """The momentum of the running-statistics update as the row kernels take it: a number.  momentum=None asks nn.BatchNorm for the
    cumulative average 1 / num_batches_tracked, which these kernels do not form: refused where the statistics would be updated (batch
    statistics with running buffers), irrelevant elsewhere."""
    if not bn_momentum_usable(bn, use_batch):
        raise ValueError("BatchNorm with momentum=None (cumulative moving average) is not served by the row kernels")
    return 0.0 if bn.momentum is None else float(bn.momentum)


def bn_momentum_usable(bn, training):
    """Does _bn_momentum have a number for this layer?  Metadata only.  training: the layer's mode, or _bn_momentum's use_batch (training or
    no running statistics) -- the same answer, since a layer without running statistics updates none."""
    return bn.momentum is not None or not training or bn.running_mean is None


def _bn_mode(bn, training):
    """(use_batch, momentum) as the BatchNorm kernels take them: batch statistics in training and wherever there are no running ones; raises
    ValueError through _bn_momentum, before any device call."""
    use_batch = training or bn.running_mean is None
    return use_batch, _bn_momentum(bn, use_batch)


def propagate_usable(rows, bn, training, sync_bn=False):
    """Can the fused step (propagate, prop_tail) serve a token matrix of `rows` rows with this BatchNorm1d?  Metadata only.  An affine
    layer, statistics it can take (running ones in eval), a momentum the kernels form (_bn_momentum), a row count csr_build takes, and no
    synchronised BatchNorm (sync_bn: the statistics then span the ranks)."""
    return bool(bn.affine and (bn.track_running_stats or training) and bn_momentum_usable(bn, training) and rows <= ops.CSR_MAX_ROWS and not sync_bn)


# ------------------------------------------------------------------ forward-only row operators (frozen prompter branches)
def bn_rows(x, bn, training, relu=False):
    """BatchNorm(+ReLU) over the rows of a channels-last (R,C) matrix; no autograd (frozen branches only)."""
    use_batch, momentum = _bn_mode(bn, training)
    return ops.bn_rows_fwd(x.contiguous(), bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum, bn.eps, use_batch, relu)


class _BnRowsTrain(Function):
    """Training-mode BatchNorm(+ReLU)(+Dropout) over rows with its backward (upp_bn_rows_fwd / upp_bn_rows_bwd, upp_bn_rows_drop_*): the
    trainable BatchNorm1d layers of the per-point heads.  The running statistics are updated in place by the forward."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, relu, drop_p=0.0, seed=None, salt=0, bump_pending=False):
        x = x.contiguous()
        # the mask is a hash of the counter's value for THIS forward (the old value + 1 when the host bumps its counters at the end of the
        # forward, upp_layers.end_forward), taken here into a tensor of its own that forward and backward both read: the live counter
        # may move any number of times before the backward runs (another forward of the layer, reset_running_stats, load_state_dict)
        drop = snap = None
        if drop_p > 0.0:
            snap = seed + (1 if bump_pending else 0)           # one element-wise launch: capturable, no memset
            drop = (drop_p, snap, 0, salt)
        y, mean, rstd = ops.bn_rows_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, True, relu, want_stats=True, drop=drop)
        ctx.save_for_backward(x, mean, rstd, gamma, beta, snap)
        ctx.relu, ctx.drop = relu, (None if drop is None else (drop_p, salt))
        return y

    @staticmethod
    def backward(ctx, g):
        x, mean, rstd, gamma, beta, snap = ctx.saved_tensors
        drop = None if ctx.drop is None else (ctx.drop[0], snap, 0, ctx.drop[1])
        g_x, g_gamma, g_beta = ops.bn_rows_bwd(x, g.contiguous(), mean, rstd, gamma, beta, ctx.relu, want_gx=ctx.needs_input_grad[0], drop=drop)
        return (g_x, g_gamma if ctx.needs_input_grad[1] else None, g_beta if ctx.needs_input_grad[2] else None,
                None, None, None, None, None, None, None, None, None)


def bn_rows_train(x, bn, relu=False, drop_p=0.0, salt=0, bump_pending=False):
    """Differentiable training-mode BatchNorm(+ReLU) over the rows of a channels-last (R,C) matrix; drop_p > 0: nn.Dropout(drop_p) on the
    output in the same passes, its masks a hash of (bn.num_batches_tracked, salt, element) -- the caller bumps the counter once per forward
    (upp_layers.bump_counter, as nn.BatchNorm1d does); bump_pending: that bump has been queued for the end of the forward, not applied.
    The forward snapshots the counter value it hashes and the backward uses that snapshot, so any number of forwards, a reset or a
    load_state_dict may run between a forward and its backward."""
    momentum = _bn_momentum(bn, True)
    if drop_p > 0.0:
        return _BnRowsTrain.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum, bn.eps, relu, float(drop_p),
                                  bn.num_batches_tracked, int(salt), bool(bump_pending))
    return _BnRowsTrain.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum, bn.eps, relu)


class _FanOut(Function):
    """n aliases of one tensor whose gradients come back TOGETHER: autograd sums the gradients of a tensor that n consumers read with
    n - 1 element-wise launches (`pos` is added in front of every Transformer block: 11 launches of stage 2's backward); here the n
    gradients are added in branch order by one upp_batched_sum launch (n jobs of one row sharing the destination)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n = n
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        live = [g for g in gs if g is not None]
        if not live:
            return None, None
        if len(live) == 1:
            return live[0], None
        first = live[0]
        if not (first.is_cuda and first.dtype == torch.float32 and all(g.shape == first.shape and g.dtype == first.dtype for g in live)):
            total = live[0]
            for g in live[1:]:
                total = total + g
            return total, None
        out = torch.empty(first.shape, dtype=torch.float32, device=first.device)
        n = out.numel()
        ops.batched_sum([(g.contiguous().view(1, n), 0, 1, n, n, out, False) for g in live])       # (one group: dst = sum of its jobs, in order)
        return out, None


def fan_out(x, n):
    """-> n tensors equal to x (views of it); use one per consumer.  With a gradient flowing (HIP f32) the n gradients are summed in one
    launch; otherwise x itself is handed out n times."""
    if n > 1 and torch.is_grad_enabled() and x.requires_grad and x.is_cuda and x.dtype == torch.float32 and n <= 64:
        return _FanOut.apply(x, int(n))
    return (x,) * n


class _GroupMax(Function):
    """max over the k rows of every group (upp_group_max_fwd) with the one-pass backward (upp_group_max_bwd)."""

    @staticmethod
    def forward(ctx, x):
        out, amax = ops.group_max_fwd(x)
        ctx.save_for_backward(amax)
        ctx.k = x.shape[1]
        return out

    @staticmethod
    def backward(ctx, g):
        (amax,) = ctx.saved_tensors
        return ops.group_max_bwd(g.contiguous(), amax, ctx.k)


def group_max(x):
    """x (..., k, C) -> (..., C): max over the second-to-last dimension.  f32 HIP tensors with C % 4 == 0, k <= 255 and contiguous rows take
    the kernel pair (forward: max + arg-max in one read; backward: the gradient tensor written once, no zero-fill + scatter); anything else
    `x.max(dim=-2)[0]`."""
    if (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and x.is_contiguous() and x.shape[-1] % 4 == 0 and 1 <= x.shape[-2] <= 255
            and x.numel() > 0 and x.data_ptr() % 16 == 0):
        lead = tuple(x.shape[:-2])
        x3 = x.reshape(-1, x.shape[-2], x.shape[-1])
        out = _GroupMax.apply(x3) if (torch.is_grad_enabled() and x.requires_grad) else ops.group_max_fwd(x3)[0]
        return out.view(lead + (x.shape[-1],))
    return x.max(dim=-2)[0]


def argsort_rows(key, descending=False, stable=True):
    """torch.argsort(key, dim=-1, descending=..., stable=True) of short rows (N <= 16384) on the rank-counting kernel (upp_argsort_rows)
    for f32 HIP tensors; anything else (CPU tensors on a GPU-less host, other dtypes, long rows) takes torch.argsort.  Integer / bool
    keys of small magnitude (a mask) are ranked through their exact f32 image.  The kernel's order IS the stable one (ties by index, NaN
    above +inf as torch ranks it), so `stable=False` -- which only permits another tie order -- is served by the same launch."""
    if isinstance(key, torch.Tensor) and key.is_cuda and key.dim() >= 1 and 1 <= key.shape[-1] <= 16384 and key.numel() < 2 ** 31:
        if key.dtype == torch.float32:
            return ops.argsort_rows(key.detach(), descending)
        if key.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16):          # exact in f32
            return ops.argsort_rows(key.to(torch.float32), descending)
    return torch.argsort(key, dim=-1, descending=descending, stable=stable)


def sqdist_topk(xyz1, xyz2, k):
    """The k nearest xyz2 points of every xyz1 point (reference square_distance form), ascending; no autograd."""
    return ops.sqdist_topk(xyz1.contiguous(), xyz2.contiguous(), k)


def interp(dists, idx, feat, k, eps, out=None, col0=0):
    """Inverse-distance interpolation from the k nearest of a sorted neighbour table; no autograd."""
    return ops.interp_fwd(dists, idx, feat.contiguous(), k, eps, out, col0)


class _InterpTrain(Function):
    """Inverse-distance interpolation with a gradient for the features (upp_interp_fwd / upp_interp_bwd); the sorted
    neighbour table (dists, idx) is a constant of the graph."""

    @staticmethod
    def forward(ctx, dists, idx, feat, k, eps):
        feat = feat.contiguous()
        ctx.save_for_backward(dists, idx)
        ctx.S, ctx.k, ctx.eps = feat.shape[1], k, eps
        return ops.interp_fwd(dists, idx, feat, k, eps)

    @staticmethod
    def backward(ctx, g):
        dists, idx = ctx.saved_tensors
        return None, None, ops.interp_bwd(dists, idx, g.contiguous(), ctx.S, ctx.k, ctx.eps), None, None


_UNIT_DIST = {}


def gather_rows(points, idx):
    """points (B,S,C) f32, idx (B,M) int64 per-sample row indices -> (B,M,C) = points[b, idx[b, m]] with a DETERMINISTIC, sort-free
    backward: a gather is the k = 1 inverse-distance interpolation (its single weight is (1/(d+eps)) / (1/(d+eps)) = 1 exactly), so the
    forward is upp_interp_fwd and the gradient the pull kernel of upp_interp_bwd -- torch's advanced-indexing backward is an
    index_put_(accumulate=True) behind a device radix sort (reference models/Point_MAE_pretask_dev.py:409-413 set abstraction, whose
    features carry a gradient in the pre-task and stage-2 recipes).  M <= 4096; anything else takes torch.gather."""
    B, S, C = points.shape
    M = idx.shape[1]
    if not (points.is_cuda and points.dtype == torch.float32 and idx.dtype == torch.int64 and idx.dim() == 2 and 0 < M <= 4096 and S > 0):
        return torch.gather(points, 1, idx.unsqueeze(-1).expand(-1, -1, C))
    key = (B, M, str(points.device))
    d = _UNIT_DIST.get(key)
    if d is None:
        d = torch.zeros(B, M, 1, device=points.device)
        if not torch.cuda.is_current_stream_capturing():          # (memory of a graph's private pool is never cached)
            # never evicted (B M 4 bytes per shape): a HIP graph captured earlier has the address of a cached tensor baked into its interp
            # launches -- returning that memory to the allocator would let a later tensor put anything under a replayed graph's weights
            _UNIT_DIST[key] = d
    tab = idx.contiguous().view(B, M, 1)
    if torch.is_grad_enabled() and points.requires_grad:
        return _InterpTrain.apply(d, tab, points, 1, 1.0)
    return ops.interp_fwd(d, tab, points.contiguous(), 1, 1.0)


def interp_train(dists, idx, feat, k, eps):
    """Differentiable (w.r.t. feat) inverse-distance interpolation from the k nearest of a sorted neighbour table."""
    return _InterpTrain.apply(dists, idx, feat, k, eps)


class _InterpGeo(Function):
    """Inverse-distance interpolation with gradients for the features AND the geometry (queries and sources): forward upp_sqdist_topk +
    upp_interp_fwd, backward upp_interp_bwd (features) + upp_interp_geo_bwd (coordinates) -- the autograd chain of the reference's
    square_distance / sort / index / weights formulation (models/Point_MAE_unify.py:22-48) in five launches."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, feat, k, eps):
        xyz1, xyz2, feat = xyz1.contiguous(), xyz2.contiguous(), feat.contiguous()
        dists, idx = ops.sqdist_topk(xyz1, xyz2, k)
        ctx.save_for_backward(xyz1, xyz2, feat, dists, idx)
        ctx.k, ctx.eps = k, eps
        return ops.interp_fwd(dists, idx, feat, k, eps)

    @staticmethod
    def backward(ctx, g):
        xyz1, xyz2, feat, dists, idx = ctx.saved_tensors
        g = g.contiguous()
        need = ctx.needs_input_grad
        g_feat = ops.interp_bwd(dists, idx, g, feat.shape[1], ctx.k, ctx.eps) if need[2] else None
        g1 = g2 = None
        if need[0] or need[1]:
            g1, g2 = ops.interp_geo_bwd(dists, idx, feat, g, xyz1, xyz2, ctx.k, ctx.eps, need[0], need[1])
        return g1, g2, g_feat, None, None


def interp_geo(xyz1, xyz2, feat, k, eps):
    """(B,N,C) inverse-distance interpolation of feat (B,S,C) at xyz1 from its k nearest of xyz2, differentiable w.r.t. all three."""
    return _InterpGeo.apply(xyz1, xyz2, feat, int(min(k, xyz2.shape[1])), float(eps))


class _InterpAffine(Function):
    """interp(feat) + x3 . wt in one launch (upp_interp_affine_fwd); gradients for feat (upp_interp_bwd) and wt (one skinny
    GEMM); the neighbour table and x3 are constants of the graph."""

    @staticmethod
    def forward(ctx, dists, idx, feat, x3, wt, k, eps):
        feat, x3, wt = feat.contiguous(), x3.contiguous(), wt.contiguous()
        ctx.save_for_backward(dists, idx, x3)
        ctx.S, ctx.k, ctx.eps = feat.shape[1], k, eps
        return ops.interp_affine_fwd(dists, idx, feat, x3, wt, k, eps)

    @staticmethod
    def backward(ctx, g):
        dists, idx, x3 = ctx.saved_tensors
        g = g.contiguous()
        g_feat = ops.interp_bwd(dists, idx, g, ctx.S, ctx.k, ctx.eps) if ctx.needs_input_grad[2] else None
        g_wt = None
        if ctx.needs_input_grad[4]:
            g2, x2 = g.reshape(-1, g.shape[-1]), x3.reshape(-1, 3)
            if g2.shape[1] * 3 <= 2048 and g2.shape[1] + 3 <= 512:           # (3, C) = x3^T g over all points: the small-K weight-gradient kernel (transposed roles)
                g_wt = ops.linear_smallk_wgrad(g2, x2).sum(0).t()
            elif g2.shape[1] % 4 == 0 and g2.stride(0) % 4 == 0 and g2.data_ptr() % 16 == 0 and g2.is_cuda:
                # wide rows (C = 1536 over 65,536 label points): three weighted column sums of g, read once
                g_wt = ops.wcolsum_partials(g2, x2).sum(0)
            else:
                note_declined("rank-3 weight gradient (3,%d)" % g2.shape[1], "row alignment")
                g_wt = torch.mm(x2.t(), g2)
        return None, None, g_feat, None, g_wt, None, None


def interp_affine_train(dists, idx, feat, x3, wt, k, eps):
    """Differentiable (w.r.t. feat and wt) interpolation + rank-3 term: (B,N,C) = interp(feat) + x3 (B,N,3) . wt (3,C)."""
    return _InterpAffine.apply(dists, idx, feat, x3, wt, k, eps)


def posenc(x, freqs, out=None, col0=0):
    """(x, sin(f x), cos(f x))_f positional embedding of (...,3) coordinates; no autograd."""
    return ops.posenc_fwd(x.contiguous(), freqs, out, col0)


# ------------------------------------------------------------------ per-point segmentation tail
class _LinearPadN(Function):
    """y (M, Np) = x . Wp^T for Wp = the (N,K) weight W zero-padded to Np = ceil4(N) rows, WITHOUT materialising Wp (reference
    models/Point_MAE_unify_segment.py:432 the 50-class Conv1d; the GEMM kernels want N % 4 == 0): the forward multiplies through W's own
    bf16 plane image (upp_linear_sb_prep zero-fills beyond N), the data gradient through a persistent zero-padded W^T (K, Np), and the
    weight gradient's partial tiles are (Np, K) of which the first N rows are summed into W's gradient.  F.pad of weight and bias (two
    fills + two copies per step), the [:, :N] slice of the output and its backward (a zero-fill + a copy of the (M, Np) matrix) are gone."""

    @staticmethod
    def forward(ctx, x, w):
        N, K = w.shape
        Np = (N + 3) // 4 * 4
        planes = ops.PLANES.get_trainable(w) if w.requires_grad else ops.PLANES.get(w)
        ctx.save_for_backward(x if w.requires_grad else None, w)
        ctx.Np = Np
        return ops.linear_f32(x, None, None, ops.LIN_NONE, planes=planes, wshape=(Np, K))

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        N, K = w.shape
        g = _rows(g)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            wt = (TRANSPOSED.get_trainable_padded(w, ctx.Np) if w.requires_grad and TRANSPOSED.managed
                  else F.pad(w.detach().t(), (0, ctx.Np - N)).contiguous())           # (outside a step driver: a fresh padded copy)
            gx = ops.linear_f32(g, wt)
        if ctx.needs_input_grad[1]:
            if not _DEFERRED.wgrad_rows(w.data_ptr(), g, x, N):
                gw = _sum_splits(ops.linear_wgrad(g, x))[:N]
        return gx, gw


def linear_pad_n_usable(x, w):
    """Can _LinearPadN serve F.linear(x, w) for an (N,K) weight with N % 4 != 0?  HIP f32 rows, the split-bf16 kernel takes (M, ceil4(N), K),
    and the weight is frozen or managed by a step driver (persistent plane image and padded W^T, refreshed once per step)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and _aligned(x)
            and w.dim() == 2 and w.dtype == torch.float32 and w.stride(1) == 1 and x.shape[1] == w.shape[1] and w.shape[0] % 4 != 0):
        return False
    if w.requires_grad and torch.is_grad_enabled() and not (ops.PLANES.managed and TRANSPOSED.managed and isinstance(w._base if w._base is not None else w, torch.nn.Parameter)):
        return False
    if not w.requires_grad and torch.is_grad_enabled() and x.requires_grad:
        return False            # (a frozen weight under a gradient for x: the padded frozen W^T is not kept -- the padded-weight path serves it)
    return ops.linear_sb_usable(x.shape[0], (w.shape[0] + 3) // 4 * 4, w.shape[1])


class _LogSoftmaxRows(Function):
    """log_softmax(y[:, :C] + bias) over the rows of a (R, Cpad) matrix (upp_logsoftmax_rows_fwd / _bwd): the gradient comes back in the
    padded layout, pad columns zero; a trainable bias takes the deferred column sum of that gradient."""

    @staticmethod
    def forward(ctx, y, bias, C):
        logp = ops.logsoftmax_rows_fwd(y, bias, C)
        ctx.save_for_backward(logp)
        ctx.Cpad, ctx.C = y.shape[1], C
        ctx.bias_ptr = bias.data_ptr() if bias is not None else 0
        return logp

    @staticmethod
    def backward(ctx, g):
        (logp,) = ctx.saved_tensors
        g_y = ops.logsoftmax_rows_bwd(g if g.is_contiguous() else g.contiguous(), logp, ctx.Cpad)
        gb = None
        if ctx.bias_ptr and ctx.needs_input_grad[1]:
            _, gb = _DEFERRED.reduce(ctx.bias_ptr, g_y, 0, ctx.C)
        return g_y, gb, None


def log_softmax_rows(y, bias, C):
    """F.log_softmax(y[:, :C] + bias, dim=-1) for a 2-D f32 HIP matrix y (R, >= C), C <= 64."""
    return _LogSoftmaxRows.apply(y, bias, int(C))


class _NllMean(Function):
    """F.nll_loss(logp, target) (mean reduction) in two launches forward, one backward (upp_nll_mean_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, logp, target):
        ctx.save_for_backward(target)
        ctx.shape = tuple(logp.shape)
        return ops.nll_mean_fwd(logp, target).view(())

    @staticmethod
    def backward(ctx, g):
        (target,) = ctx.saved_tensors
        return ops.nll_mean_bwd(g.reshape(1).contiguous(), target, ctx.shape[0], ctx.shape[1]), None


def nll_mean(logp, target):
    """F.nll_loss(logp, target) for contiguous f32 HIP log-probabilities (R, C) and int64 targets (R); torch elsewhere."""
    if (logp.is_cuda and logp.dtype == torch.float32 and logp.dim() == 2 and logp.is_contiguous() and target.dtype == torch.int64
            and target.is_cuda and target.numel() == logp.shape[0]):
        return _NllMean.apply(logp, target.contiguous().view(-1))
    return F.nll_loss(logp, target)


class _NoiseLoss(Function):
    """(positive + negative, score) of the pre-task noise supervision in two launches forward, one backward (upp_noise_loss_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, pred, noise_vector, pn):
        pred, noise_vector = pred.contiguous(), noise_vector.contiguous()
        loss, score = ops.noise_loss_fwd(pred, noise_vector, pn)
        ctx.save_for_backward(pred, noise_vector)
        ctx.pn = pn
        ctx.mark_non_differentiable(score)
        ctx.set_materialize_grads(False)
        return loss.view(()), score

    @staticmethod
    def backward(ctx, g, _g_score):
        if g is None:
            return None, None, None
        pred, nv = ctx.saved_tensors
        return ops.noise_loss_bwd(g.reshape(1).contiguous(), pred, nv, ctx.pn), None, None


def noise_loss(pred, noise_vector, point_num):
    """mean |pred_noise - noise_vector|^2 + mean |pred_pure|^2 and score = |pred| (reference models/Point_MAE_pretask_dev.py:685-692, a
    3-channel rectify prompter): pred (B,P,3) = [point_num shape points | noise points].  -> (loss, score (B,P))."""
    return _NoiseLoss.apply(pred, noise_vector, int(point_num))


# ------------------------------------------------------------------ classification tail
class _ClsPool(Function):
    """feat = [LN(x)[:, 0] | max over rows 1.. of LN(x)]  (upp_cls_pool_fwd / bwd); LayerNorm parameters get no gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = x.contiguous()
        feat, amax, mean, rstd = ops.cls_pool_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, mean, rstd, gamma, amax)
        return feat

    @staticmethod
    def backward(ctx, g_feat):
        x, mean, rstd, gamma, amax = ctx.saved_tensors
        return ops.cls_pool_bwd(g_feat.contiguous(), x, mean, rstd, gamma, amax), None, None, None


class _ClsPoolLN(Function):
    """_ClsPool for a LayerNorm that trains: the same forward, the same g_x (upp_cls_pool_bwd's kernel) and g_gamma / g_beta from the
    rows that carry a gradient (upp_cls_pool_bwd_ln)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = x.contiguous()
        feat, amax, mean, rstd = ops.cls_pool_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, mean, rstd, gamma, amax)
        return feat

    @staticmethod
    def backward(ctx, g_feat):
        x, mean, rstd, gamma, amax = ctx.saved_tensors
        g_x, g_gamma, g_beta = ops.cls_pool_bwd_ln(g_feat.contiguous(), x, mean, rstd, gamma, amax)
        need = ctx.needs_input_grad
        return g_x if need[0] else None, g_gamma if need[1] else None, g_beta if need[2] else None, None


def cls_pool(x, norm):
    """torch.cat([norm(x)[:, 0], norm(x)[:, 1:].max(1)[0]], -1) for an nn.LayerNorm `norm`: the node of the frozen LayerNorm (and its
    bits) when neither parameter needs a gradient, the node with the parameter gradients otherwise."""
    if torch.is_grad_enabled() and (norm.weight.requires_grad or norm.bias.requires_grad):
        return _ClsPoolLN.apply(x, norm.weight, norm.bias, float(norm.eps))
    return _ClsPool.apply(x, norm.weight, norm.bias, float(norm.eps))


# ------------------------------------------------------------------ LayerNorm of three feature taps + token pooling (csrc/norm_pool.hip)
class _TapPool(Function):
    """(x, gmax, gmean) of include/upp_hip.h upp_tap_pool_fwd: one launch forward, two backward (upp_tap_pool_bwd)."""

    @staticmethod
    def forward(ctx, f0, f1, f2, gamma, beta, eps):
        f0, f1, f2 = f0.contiguous(), f1.contiguous(), f2.contiguous()
        x, gmax, arg, gmean, mean, rstd = ops.tap_pool_fwd(f0, f1, f2, gamma, beta, eps)
        ctx.save_for_backward(f0, f1, f2, mean, rstd, gamma, arg)
        return x, gmax, gmean

    @staticmethod
    def backward(ctx, d_x, d_gmax, d_gmean):
        f0, f1, f2, mean, rstd, gamma, arg = ctx.saved_tensors
        d0, d1, d2, d_gamma, d_beta = ops.tap_pool_bwd(d_x.contiguous(), d_gmax.contiguous(), d_gmean.contiguous(), f0, f1, f2, mean, rstd,
                                                       gamma, arg)
        need = ctx.needs_input_grad
        return (d0 if need[0] else None, d1 if need[1] else None, d2 if need[2] else None, d_gamma if need[3] else None,
                d_beta if need[4] else None, None)


def tap_pool_usable(f0, f1, f2, norm):
    """The served range of upp_tap_pool_fwd / bwd: three f32 HIP (B,G,C) tensors of one shape, 1 <= B <= 65535, 1 <= G <= 2048 (UPP_ATTN_MAX_L),
    C % 4 == 0, 4 <= C <= 512, and an affine nn.LayerNorm(C) with f32 parameters on the same device."""
    ts = (f0, f1, f2)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 for t in ts):
        return False
    if not (f0.shape == f1.shape == f2.shape and f0.device == f1.device == f2.device):
        return False
    B, G, C = f0.shape
    if not (isinstance(norm, torch.nn.LayerNorm) and tuple(norm.normalized_shape) == (C,) and norm.elementwise_affine and norm.bias is not None
            and norm.weight.dtype == torch.float32 and norm.weight.device == f0.device):
        return False
    return 1 <= B <= 65535 and 1 <= G <= 2048 and C % 4 == 0 and 4 <= C <= 512


def tap_pool(f0, f1, f2, norm):
    """-> (x (B,G,3C) = [norm(f0) | norm(f1) | norm(f2)], gmax (B,3C) = x.max(1)[0], gmean (B,3C) = the mean over the tokens summed in
    token order) for one shared nn.LayerNorm `norm` (reference models/Point_MAE_segment.py:413-424).  HIP tensors of the served range
    (tap_pool_usable) take the kernels; a HIP tensor outside it is recorded by note_declined and, like a CPU tensor, takes the torch
    formulation upp_hip.torch_cpu.tap_pool."""
    if tap_pool_usable(f0, f1, f2, norm):
        return _TapPool.apply(f0, f1, f2, norm.weight, norm.bias, float(norm.eps))
    from . import torch_cpu
    if isinstance(f0, torch.Tensor) and f0.is_cuda:
        note_declined("tap_pool taps %s %s" % (tuple(f0.shape), f0.dtype), "outside the served range")
    return torch_cpu.tap_pool(f0, f1, f2, norm)


class _CrossEntropyAcc(Function):
    """(mean cross-entropy, top-1 accuracy * 100) of logits (B,C) against int64 labels in one launch (upp_ce_acc)."""

    @staticmethod
    def forward(ctx, logits, labels):
        out2, dlogits = ops.ce_acc(logits.contiguous(), labels.contiguous())
        ctx.save_for_backward(dlogits)
        loss, acc = out2[0], out2[1]
        ctx.mark_non_differentiable(acc)
        ctx.set_materialize_grads(False)          # (no zero scalar for the accuracy's "gradient")
        return loss, acc

    @staticmethod
    def backward(ctx, g_loss, _g_acc):
        if g_loss is None:
            return None, None
        (dlogits,) = ctx.saved_tensors
        return dlogits * g_loss, None


class _BnReluDrop(Function):
    """Dropout(ReLU(BatchNorm1d(z))) of a few-row matrix in one launch each way (upp_bn_relu_drop_fwd / bwd)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, momentum, eps, training, u, p):
        z = z.contiguous()
        a, mean, rstd = ops.bn_relu_drop_fwd(z, gamma, beta, running_mean, running_var, momentum, eps, training, u, p)
        ctx.save_for_backward(z, gamma, beta, mean, rstd, u)
        ctx.meta = (training, p)
        return a

    @staticmethod
    def backward(ctx, g_a):
        z, gamma, beta, mean, rstd, u = ctx.saved_tensors
        training, p = ctx.meta
        g_z, g_gamma, g_beta = ops.bn_relu_drop_bwd(g_a.contiguous(), z, gamma, beta, mean, rstd, training, u, p)
        return (g_z, g_gamma, g_beta) + (None,) * 7


def bn_relu_drop(z, bn, u=None, p=0.0, training=True):
    """dropout_p(relu(bn(z))) for a (rows, C) matrix with few rows; u: uniforms (rows, C) when p > 0 in training."""
    use_batch, momentum = _bn_mode(bn, training)
    return _BnReluDrop.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum, bn.eps, use_batch, u, float(p))


def cross_entropy_acc(logits, labels):
    return _CrossEntropyAcc.apply(logits, labels)


class _BiasGelu(Function):
    """GELU(z + bias) for a frozen bias (upp_bias_gelu_fwd / bwd)."""

    @staticmethod
    def forward(ctx, z, bias):
        # (autograd only calls this forward when a gradient is wanted: the derivative is produced in the same pass and z is
        # not kept -- the backward is one multiply per element instead of a second erf + exp)
        h, d = ops.bias_gelu_fwd_d(z.contiguous(), bias)
        ctx.save_for_backward(d)
        return h

    @staticmethod
    def backward(ctx, g_h):
        d, = ctx.saved_tensors
        return g_h * d, None


def bias_gelu(z, bias):
    if not (torch.is_grad_enabled() and z.requires_grad):
        return ops.bias_gelu_fwd(z.contiguous(), bias)          # frozen front-end / evaluation: value only
    return _BiasGelu.apply(z, bias)


# ------------------------------------------------------------------ bottleneck adapter
class _Adapter(Function):
    """out = x + scale * (W2 . dropout(gelu(W1 . ha + b1)) + b2); see upp_adapter_fwd."""

    @staticmethod
    def forward(ctx, ha, x, W1, b1, W2, b2, u, p, scale):
        ha, x = ha.contiguous(), x.contiguous()
        out, s1 = ops.adapter_fwd(ha, x, W1, b1, W2, b2, u, p, scale)
        ctx.save_for_backward(ha, s1, W1, W2, u)
        ctx.meta = (p, scale)
        ctx.param_ptrs = (W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr())
        return out

    @staticmethod
    def backward(ctx, g_out):
        ha, s1, W1, W2, u = ctx.saved_tensors
        p, scale = ctx.meta
        g_out = g_out.contiguous()
        g_ha, part = ops.adapter_bwd(g_out, ha, s1, W1, W2, u, p, scale)
        need = ctx.needs_input_grad
        gW1 = gb1 = gW2 = gb2 = None
        if need[2] or need[3] or need[4] or need[5]:
            H, D = W1.shape
            pW1, pb1, pW2, pb2 = ctx.param_ptrs
            # part (workgroups, [dW1 | dW2 | db1 | db2]); rows are summed in workgroup order: deterministic
            _, gW1 = _DEFERRED.reduce(pW1, part, 0, H * D)
            _, gW2 = _DEFERRED.reduce(pW2, part, H * D, H * D)
            _, gb1 = _DEFERRED.reduce(pb1, part, 2 * H * D, H)
            _, gb2 = _DEFERRED.reduce(pb2, part, 2 * H * D + H, D)
            gW1 = gW1.view(H, D) if gW1 is not None else None
            gW2 = gW2.view(D, H) if gW2 is not None else None
        return (g_ha if need[0] else None, g_out if need[1] else None, gW1 if need[2] else None, gb1 if need[3] else None,
                gW2 if need[4] else None, gb2 if need[5] else None, None, None, None)


FUSE_TAIL_BACKWARD = True     # _LnAdapter.backward: one launch (upp_ln_adapter_bwd_fused) instead of adapter backward + row backward
ADAPTER_FACTORS = True        # ... which inside a deferred scope writes per-row factors; the weight gradients of all blocks in one launch at its exit

# Reproducible training (README "Reproducible training"): with DETERMINISTIC on, the autograd nodes whose backward (or forward: the EMD
# cost) sums with f32 atomics -- GatherOperation, _FpsGather, _KnnGroup, _GroupPoints, ChamferFunction, _ChamferLoss,
# EarthMoverDistanceFunction, ThreeInterpolate, GroupingOperation, KnnPoints, KnnGather, _EdgeConvMax, _DeformAttention -- call the library's `_det` siblings (a defined summation order: include/upp_hip.h "deterministic
# scatter-adds").  Read at CALL time, also by the backward thread; a captured step keeps the choice it was captured under, whatever the
# attribute says at replay.  UPP_DETERMINISTIC=1 sets it once, at import.
DETERMINISTIC = os.environ.get("UPP_DETERMINISTIC", "").strip() not in ("", "0")


def _det(det):                 # a node's per-call choice (True / False), or -- None -- DETERMINISTIC as it reads when the backward runs
    return DETERMINISTIC if det is None else det


class deterministic:
    """with functional.deterministic(): ... -- DETERMINISTIC set to `on` inside the block and restored after it (also on an exception)."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        global DETERMINISTIC
        self.prev = DETERMINISTIC
        DETERMINISTIC = self.on
        return self

    def __exit__(self, *exc):
        global DETERMINISTIC
        DETERMINISTIC = self.prev
        return False


def _ln_adapter_backward(saved, dims, meta, param_ptrs, g_out, need_x, need_y, need_p):
    """Backward of the block tail (ln_adapter_fwd and its PROP form write the same saved tensors) -> (g_x, g_y, g_gamma, g_beta, gW1, gb1,
    gW2, gb2).  need_p: which of (gamma, beta, W1, b1, W2, b2) want a gradient; u / keep / has_y describe the residual in front of the rows."""
    xo, mean, rstd, gamma, beta, u, s1, W1, W2, ud = saved
    B, Lin, Lout, D, P, mode = dims
    keep, pd, scale, has_y = meta
    g_out = g_out.contiguous()
    need_ln = need_p[0] or need_p[1]
    need_ad = need_p[2] or need_p[3] or need_p[4] or need_p[5]
    p_gamma, p_beta, pW1, pb1, pW2, pb2 = param_ptrs
    H = W1.shape[0]
    # inside a deferred scope (TrainStep) with all four adapter buffers registered: per-row factors now, the weight gradients of every
    # block in one launch at scope exit
    factors = (FUSE_TAIL_BACKWARD and ADAPTER_FACTORS and need_p[2] and need_p[3] and need_p[4] and need_p[5]
               and _DEFERRED.targets is not None and all(_DEFERRED.targets.get(p_) is not None for p_ in (pW1, pb1, pW2, pb2)))
    if factors:
        g_x, g_y, fac, ln_part = ops.ln_adapter_bwd_fused(g_out, xo, mean, rstd, gamma, beta, s1, W1, W2, ud, pd, scale, u, keep, mode, P, Lin,
                                                          need_x, has_y and need_y, True, need_ln, factors=True)
        R = B * Lout
        factors = _DEFERRED.adapter((pW1, pW2, pb1, pb2), (H * D, H * D, H, D),
                                    (xo.view(R, D), mean.view(R), rstd.view(R), gamma, beta, g_out.view(R, D), fac, scale))
        if not factors:
            raise RuntimeError("ln_adapter backward: the registered adapter gradient buffers do not match the adapter's shapes")
        part = None
    elif FUSE_TAIL_BACKWARD:
        g_x, g_y, part, ln_part = ops.ln_adapter_bwd_fused(g_out, xo, mean, rstd, gamma, beta, s1, W1, W2, ud, pd, scale, u, keep, mode, P, Lin,
                                                           need_x, has_y and need_y, need_ad, need_ln)
    else:       # the two kernels of the unfused path (kept: tests compare the fused launch against them)
        g_ha, part = ops.ln_adapter_bwd(g_out, xo, mean, rstd, gamma, beta, s1, W1, W2, ud, pd, scale)
        g_x, _, g_y, ln_part = ops.rowln_bwd(g_out, g_ha, xo, mean, rstd, gamma, mode, u, keep, B, Lin, Lout, D, P,
                                             need_x=need_x, need_prompt=False, need_y=has_y and need_y, need_ln_part=need_ln)
    g_gamma = g_beta = gW1 = gb1 = gW2 = gb2 = None
    if need_ln:
        _, g_gamma = _DEFERRED.reduce(p_gamma, ln_part, 0, D)
        _, g_beta = _DEFERRED.reduce(p_beta, ln_part, D, D)
    if need_ad and not factors:
        _, gW1 = _DEFERRED.reduce(pW1, part, 0, H * D)
        _, gW2 = _DEFERRED.reduce(pW2, part, H * D, H * D)
        _, gb1 = _DEFERRED.reduce(pb1, part, 2 * H * D, H)
        _, gb2 = _DEFERRED.reduce(pb2, part, 2 * H * D + H, D)
        gW1 = gW1.view(H, D) if gW1 is not None else None
        gW2 = gW2.view(D, H) if gW2 is not None else None
    return (g_x, g_y, g_gamma if need_p[0] else None, g_beta if need_p[1] else None, gW1 if need_p[2] else None, gb1 if need_p[3] else None,
            gW2 if need_p[4] else None, gb2 if need_p[5] else None)


class _LnAdapter(Function):
    """The tail of a block in one launch: rows = strip(x + dp_scale(u) (y + ybias)), out = rows + scale * adapter(LayerNorm(rows)).
    Forward: upp_ln_adapter_fwd.  Backward: upp_ln_adapter_bwd (the adapter's, rebuilding the LayerNorm output from the saved
    rows) followed by upp_rowln_bwd -- the two kernels of the unfused path, minus the stored LayerNorm output."""

    @staticmethod
    def forward(ctx, x, y, ybias, u, keep, mode, P, gamma, beta, eps, W1, b1, W2, b2, ud, pd, scale):
        x = x.contiguous()
        B, Lin, D = x.shape
        Lout = Lin - P if mode in (ROW_STRIP_CLS, ROW_STRIP) else Lin
        y_c = y.contiguous() if y is not None else None
        out, xo, mean, rstd, s1 = ops.ln_adapter_fwd(x, y_c, ybias, u, keep, mode, P, gamma, beta, eps, W1, b1, W2, b2, ud, pd, scale, Lout)
        ctx.save_for_backward(xo, mean, rstd, gamma, beta, u, s1, W1, W2, ud)
        ctx.dims = (B, Lin, Lout, D, P, mode)
        ctx.meta = (keep, pd, scale, y is not None)
        ctx.param_ptrs = (gamma.data_ptr(), beta.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr())
        return out

    @staticmethod
    def backward(ctx, g_out):
        need = ctx.needs_input_grad
        g_x, g_y, g_gamma, g_beta, gW1, gb1, gW2, gb2 = _ln_adapter_backward(ctx.saved_tensors, ctx.dims, ctx.meta, ctx.param_ptrs, g_out,
                                                                             need[0], need[1], (need[7], need[8]) + tuple(need[10:14]))
        return (g_x if need[0] else None, g_y, None, None, None, None, None, g_gamma, g_beta, None, gW1, gb1, gW2, gb2, None, None, None)


# (round 5 also let this launch compute the NEXT block's head -- upp_ln_adapter_fwd_next: bit-identical, and slower: the tail grew by what the
# head launch cost and the step went 4.57 -> 4.71 ms; it left the library with ABI 5, NOTEBOOK section 11.6.)
def ln_adapter(x, y, ybias, u, keep, mode, P, ln, W1, b1, W2, b2, ud=None, pd=0.0, scale=0.7):
    """One launch for `rowln(x, y=y, ybias=ybias, u=u, keep=keep, mode=mode, P=P, gamma, beta)` + `adapter(ha, rows, ...)`
    (mode: ROW_IDENTITY / ROW_STRIP_CLS / ROW_STRIP).  Limits: D == 384, 32 hidden units."""
    if ybias is not None and (y is None or (torch.is_grad_enabled() and ybias.requires_grad)):
        raise ValueError("ybias is the frozen bias of the Linear that produced y")
    return _LnAdapter.apply(x, y, ybias, u, float(keep), int(mode), int(P), ln.weight, ln.bias, float(ln.eps), W1, b1, W2, b2, ud,
                            float(pd), float(scale))


class _PropTail(Function):
    """A prompted block from the fc2 product to the adapter output in 3 launches forward and 4 backward:
        x3 = x2 + dp_scale(u_dp) (m + mb);  x3' = propagate(x3);  out = ln_adapter(strip(x3'))
    Forward: upp_prop_res_pool_fwd (pool + statistics on rows of x3 formed where they are gathered | BatchNorm finalize) and
    upp_ln_adapter_prop_fwd (the interpolation as the tail's row phase); neither x3 nor x3' is stored.  Backward: upp_ln_adapter_bwd_fused,
    then upp_prop_res_bwd, whose last launch writes the gradients of x2 and m.  Bit-identical to rowln -> propagate -> ln_adapter."""

    @staticmethod
    def forward(ctx, x2, m, mb, u_dp, keep_dp, mode, P, index, u_g, keep_g, bn_gamma, bn_beta, running_mean, running_var, momentum, bn_eps,
                training, ln_gamma, ln_beta, ln_eps, W1, b1, W2, b2, ud, pd, scale):
        x2, m = x2.contiguous(), m.contiguous()
        B, Lin, D = x2.shape
        Lout = Lin - P if mode in (ROW_STRIP_CLS, ROW_STRIP) else Lin
        w8 = index.w8
        pooled, amax, _, bn_mean, bn_rstd = ops.prop_res_pool_fwd(x2, m, mb, u_dp, keep_dp, index.i1, u_g, keep_g, running_mean, running_var,
                                                                  momentum, bn_eps, training, index.G2)
        out, xo, mean, rstd, s1 = ops.ln_adapter_prop_fwd(x2, m, mb, u_dp, keep_dp, mode, P, pooled, bn_mean, bn_rstd, bn_gamma, bn_beta, index.i2,
                                                          index.idx8, w8, ln_gamma, ln_beta, ln_eps, W1, b1, W2, b2, ud, pd, scale, Lout)
        ctx.save_for_backward(xo, mean, rstd, ln_gamma, ln_beta, None, s1, W1, W2, ud, pooled, amax, bn_mean, bn_rstd, bn_gamma, u_g, w8, u_dp)
        ctx.dims = (B, Lin, Lout, D, P, mode)
        ctx.meta = (index, keep_g, keep_dp, pd, scale, training)
        ctx.param_ptrs = (ln_gamma.data_ptr(), ln_beta.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr())
        return out

    @staticmethod
    def backward(ctx, g_out):
        saved = ctx.saved_tensors
        pooled, amax, bn_mean, bn_rstd, bn_gamma, u_g, w8, u_dp = saved[10:]
        index, keep_g, keep_dp, pd, scale, training = ctx.meta
        B, Lin = ctx.dims[0], ctx.dims[1]
        need = ctx.needs_input_grad
        # the tail saw x3' as its stream and no residual branch: g (B, Lin, D), zeros in the prompt rows the strip dropped
        g, _, g_gamma, g_beta, gW1, gb1, gW2, gb2 = _ln_adapter_backward(saved[:10], ctx.dims, (1.0, pd, scale, False), ctx.param_ptrs, g_out,
                                                                         True, False, (need[17], need[18], need[20], need[21], need[22], need[23]))
        g_x2, g_m, g_bn_gamma, g_bn_beta = ops.prop_res_bwd(g, pooled, amax, bn_mean, bn_rstd, bn_gamma, u_g, keep_g, w8, index.csr1, index.csr2,
                                                            index.csr8, training, u_dp, keep_dp, B, Lin, index.T, index.G2)
        return ((g_x2 if need[0] else None, g_m if need[1] else None) + (None,) * 8 + (g_bn_gamma, g_bn_beta) + (None,) * 5
                + (g_gamma, g_beta, None, gW1, gb1, gW2, gb2, None, None, None))


def prop_tail_usable(x2, bn, T, P, mode, training=True, sync_bn=False):
    """Can prop_tail serve this block (T centre rows per cloud, P prompts stripped by `mode`)?  f32 rows of D = 384 (the tail kernel), a
    strip map that keeps every centre row, and what the fused step itself asks (propagate_usable)."""
    B, Lin, D = x2.shape
    return (x2.is_cuda and x2.dtype == torch.float32 and D == 384 and P > 0 and mode in (ROW_STRIP_CLS, ROW_STRIP) and T <= Lin - P
            and propagate_usable(B * Lin, bn, training, sync_bn))


def prop_tail(x2, m, mb, u_dp, keep_dp, mode, P, bn, index, u_g, keep_g, training, ln, W1, b1, W2, b2, ud=None, pd=0.0, scale=0.7):
    """One autograd node for `rowln(x2, y=m, ybias=mb, u=u_dp, keep=keep_dp)` -> `propagate(., bn, index, u_g, keep_g, training)` ->
    `ln_adapter(., None, None, None, 1.0, mode, P, ln, W1, b1, W2, b2, ud, pd, scale)`; index.w8 are constants of the forward (no gradient
    to the centres: that is stage 2 of the recipe, which needs the stored rows).  Limits: prop_tail_usable."""
    if mb is not None and torch.is_grad_enabled() and mb.requires_grad:
        raise ValueError("mb is the frozen bias of the Linear that produced m")
    use_batch, momentum = _bn_mode(bn, training)
    return _PropTail.apply(x2, m, mb, u_dp, float(keep_dp), int(mode), int(P), index, u_g, float(keep_g), bn.weight, bn.bias, bn.running_mean,
                           bn.running_var, momentum, bn.eps, use_batch, ln.weight, ln.bias, float(ln.eps), W1, b1, W2, b2, ud, float(pd),
                           float(scale))


def adapter(ha, x, W1, b1, W2, b2, u=None, p=0.0, scale=0.7):
    return _Adapter.apply(ha, x, W1, b1, W2, b2, u, float(p), float(scale))
