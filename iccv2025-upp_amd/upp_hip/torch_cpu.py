"""Pure-torch grouping operators for CPU tensors -- BASELINE configs[0] ("Point_MAE_unify cls forward, 1 synthetic N = 1024 cloud on
torch-CPU: utils.misc.fps + torch.cdist kNN fallback -- plumbing, no GPU").  OFF by default: the product's operators have no CPU
path (`upp_hip.ops` raises on CPU tensors) and a HIP tensor never comes here.  `enable()` -- or UPP_TORCH_CPU=1 in the environment --
lets the grouping entry points of upp_hip.functional (fps_gather, knn_query, knn_group, ChamferFunction, and the packed-batch pair
fps_gather_ragged / cloud_norm_ragged, the four pointnet2_ops operators ball_query, three_nn, three_interpolate,
grouping_operation, and pytorch3d.ops' knn_points / knn_gather) serve CPU tensors with the torch formulations below, so that a reference user can run the model's forward on a
GPU-less host to check plumbing (state-dict loading, shapes, config wiring).  Nothing here touches oracle/ (test infrastructure) and nothing here is timed by bench.py.

Semantics follow the reference's own CPU-side formulations: FPS as datasets/ModelNetDataset.py:29-49 (start at index 0, arg-max of the
running minimum distance) with pointnet2_ops' rule that points with |p|^2 <= 1e-3 are never candidates; kNN as models/modules.py
knn_point (pairwise squared distances, k smallest, ties by index); Chamfer as a dense distance matrix with min / argmin.  Distances are
plain f32 torch arithmetic: on EXACT distance ties a pick can differ from the HIP kernels (which pin the CUDA kernels' fmaf order and
thread-strided tie rule: oracle/upp_oracle.c) -- bit-exact indices are a property of the HIP path, not of this fallback."""
import os

import torch

_ENABLED = os.environ.get("UPP_TORCH_CPU", "0") == "1"


def enable(on=True):
    global _ENABLED
    _ENABLED = bool(on)


def enabled():
    return _ENABLED


def fps(xyz, npoint):
    """xyz (B,N,3) f32 CPU -> (centres (B,npoint,3), idx (B,npoint) int32)."""
    B, N, _ = xyz.shape
    x = xyz.detach()
    live = (x * x).sum(-1) > 1e-3                        # pointnet2_ops: |p|^2 <= 1e-3 is skipped as a candidate
    dist = torch.full((B, N), 1e10, dtype=x.dtype)
    far = torch.zeros(B, dtype=torch.long)
    idx = torch.zeros(B, npoint, dtype=torch.long)
    rows = torch.arange(B)
    for j in range(npoint):
        idx[:, j] = far
        d = ((x - x[rows, far].unsqueeze(1)) ** 2).sum(-1)
        dist = torch.minimum(dist, d)
        far = torch.where(live, dist, torch.full_like(dist, -1.0)).argmax(-1)      # first maximum: lowest index
    centers = torch.gather(xyz, 1, idx.unsqueeze(-1).expand(-1, -1, 3))
    return centers, idx.to(torch.int32)


def fps_ragged(xyz, offsets, npoint):
    """Packed batch: xyz (T,3) f32 CPU, offsets (B+1,) int64 CPU -> (centres (B,npoint,3), idx (B,npoint) int32 local to each cloud): fps()
    above, one cloud at a time."""
    o = offsets.tolist()
    got = [fps(xyz[o[b]:o[b + 1]].unsqueeze(0), npoint) for b in range(len(o) - 1)]
    if not got:
        return torch.empty(0, npoint, 3, dtype=xyz.dtype), torch.empty(0, npoint, dtype=torch.int32)
    return torch.cat([c for c, _ in got]), torch.cat([i for _, i in got])


def cloud_norm_ragged(xyz, offsets):
    """Packed batch: the reference's pc_norm (datasets/RealSensorDataset.py:59-65) per cloud, its own numpy expression in float64
    -> ((T,3) f32, scale (B,) f64)."""
    import numpy as np
    p = xyz.detach().numpy().astype(np.float64)
    o = offsets.tolist()
    out = np.empty(p.shape, dtype=np.float32)
    scale = np.empty(len(o) - 1, dtype=np.float64)
    for b in range(len(o) - 1):
        c = p[o[b]:o[b + 1]]
        scale[b] = np.max(np.sqrt(np.sum(c ** 2, axis=1))) * 2
        out[o[b]:o[b + 1]] = c / scale[b]
    return torch.from_numpy(out), torch.from_numpy(scale)


def knn(ref, query, k):
    """ref (B,N,3), query (B,Q,3) -> (dist (B,Q,k) f32 EUCLIDEAN distances ascending, idx (B,Q,k) int64; ties by index) -- what KNN_CUDA
    (its sqrt kernel) and ops.knn (csrc/knn.hip sqrtf) return.  Ranked on the direct squared distance sum_c (q_c - r_c)^2, not on
    cdist ** 2 (whose rounding perturbs the tie order)."""
    q, r = query.detach(), ref.detach()
    d2 = ((q.unsqueeze(2) - r.unsqueeze(1)) ** 2).sum(-1)
    order = torch.argsort(d2, dim=-1, stable=True)[:, :, :k]
    return torch.gather(d2, -1, order).sqrt(), order


def knn_group(xyz, center, k):
    """-> (neighbourhood (B,G,k,3) centred on `center`, idx (B,G,k) int64); differentiable w.r.t. xyz and center."""
    _, idx = knn(xyz, center, k)
    B, G, _ = idx.shape
    nb = torch.gather(xyz.unsqueeze(1).expand(-1, G, -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, 3))
    return nb - center.unsqueeze(2), idx


def ball_query(radius, nsample, xyz, new_xyz):
    """pointnet2_utils.ball_query: xyz (B,N,3), new_xyz (B,P,3) -> (B,P,nsample) int32: the first nsample points (ascending index) with
    squared distance < radius * radius (an f32 product, strict), the first hit in every unfilled slot, zeros without a hit."""
    x, q = xyz.detach(), new_xyz.detach()
    N = x.shape[1]
    r = torch.tensor(radius, dtype=x.dtype)
    d2 = ((q.unsqueeze(2) - x.unsqueeze(1)) ** 2).sum(-1)
    key = torch.where(d2 < r * r, torch.arange(N), torch.tensor(N))                 # hits keep their index, misses sort last
    if nsample > N:
        key = torch.cat([key, key.new_full(key.shape[:2] + (nsample - N,), N)], -1)
    key = key.sort(-1)[0][:, :, :nsample]
    first = key[:, :, :1]
    key = torch.where(key == N, first, key)
    return torch.where(key == N, torch.zeros_like(key), key).to(torch.int32)


def three_nn(unknown, known):
    """pointnet2_utils.three_nn: unknown (B,n,3), known (B,m,3) -> (dist (B,n,3) Euclidean ascending, idx (B,n,3) int32; ties: lower index
    first; with m < 3 the missing neighbours are index 0 at distance +inf)."""
    u, k = unknown.detach(), known.detach()
    m = k.shape[1]
    d2 = ((u.unsqueeze(2) - k.unsqueeze(1)) ** 2).sum(-1)
    if m < 3:
        d2 = torch.cat([d2, d2.new_full(d2.shape[:2] + (3 - m,), float("inf"))], -1)
    order = torch.argsort(d2, dim=-1, stable=True)[:, :, :3]
    dist = torch.gather(d2, -1, order).sqrt()
    return dist, torch.where(order < m, order, torch.zeros_like(order)).to(torch.int32)


def three_interpolate(features, idx, weight):
    """pointnet2_utils.three_interpolate: features (B,C,m), idx (B,n,3), weight (B,n,3) -> (B,C,n) = (w0 f[i0] + w1 f[i1]) + w2 f[i2];
    differentiable w.r.t. features."""
    B, C, _ = features.shape
    n = idx.shape[1]
    f = torch.gather(features, 2, idx.long().reshape(B, 1, n * 3).expand(-1, C, -1)).reshape(B, C, n, 3)
    t = f * weight.detach().unsqueeze(1)
    return (t[..., 0] + t[..., 1]) + t[..., 2]


def grouping_operation(features, idx):
    """pointnet2_utils.grouping_operation: features (B,C,N), idx (B,P,S) -> (B,C,P,S); differentiable w.r.t. features."""
    B, C, _ = features.shape
    _, P, S = idx.shape
    return torch.gather(features, 2, idx.long().reshape(B, 1, P * S).expand(-1, C, -1)).reshape(B, C, P, S)


def _clamped(lengths, N, P):
    """lengths (None | tensor | list) -> (N,) int64 in [0, P]."""
    if lengths is None:
        return torch.full((N,), P, dtype=torch.int64)
    return torch.as_tensor(lengths, dtype=torch.int64).reshape(N).clamp(0, P)


def knn_gather(x, idx, lengths=None):
    """pytorch3d.ops.knn_gather: x (N,M,U), idx (N,L,K) -> (N,L,K,U) = x[n, idx[n,l,k]], zeros in slots k >= lengths[n]; differentiable
    w.r.t. x."""
    N, M, U = x.shape
    _, L, K = idx.shape
    out = torch.gather(x.unsqueeze(1).expand(-1, L, -1, -1), 2, idx.long().unsqueeze(-1).expand(-1, -1, -1, U))
    live = torch.arange(K).view(1, 1, K) < _clamped(lengths, N, K).view(N, 1, 1)
    return torch.where(live.unsqueeze(-1), out, torch.zeros((), dtype=x.dtype))


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, return_nn=False):
    """pytorch3d.ops.knn_points by the rules of include/upp_hip.h "the pytorch3d.ops surface": p1 (N,P1,D), p2 (N,P2,D) -> (dists (N,P1,K)
    squared L2 / L1, idx (N,P1,K) int64 in ascending (distance, index), nn (N,P1,K,D) | None); zeros in slots k >= min(K, lengths2) and
    rows i >= lengths1.  dists is differentiable w.r.t. p1 and p2, nn w.r.t. p2.  The distance is a plain f32 sum over the coordinates
    (exact on lattice inputs, where it has the kernels' bits; elsewhere a last-bit difference can reorder near-ties)."""
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    len1, len2 = _clamped(lengths1, N, P1), _clamped(lengths2, N, P2)
    diff = p1.unsqueeze(2) - p2.unsqueeze(1)                                               # (N,P1,P2,D)
    d = torch.zeros(diff.shape[:3], dtype=p1.dtype)
    for j in range(D):                                                                     # ascending j, one term at a time
        d = d + (diff[..., j] * diff[..., j] if norm == 2 else diff[..., j].abs())
    rank = torch.where(torch.arange(P2).view(1, 1, P2) < len2.view(N, 1, 1), d.detach(), torch.full((), float("inf"), dtype=d.dtype))
    if K > P2:
        rank = torch.cat([rank, rank.new_full((N, P1, K - P2), float("inf"))], -1)
    order = torch.argsort(rank, dim=-1, stable=True)[:, :, :K]
    live = (torch.arange(K).view(1, 1, K) < len2.clamp(max=K).view(N, 1, 1)) & (torch.arange(P1).view(1, P1, 1) < len1.view(N, 1, 1))
    idx = torch.where(live, order, torch.zeros_like(order))
    dists = torch.where(live, torch.gather(d, 2, idx), torch.zeros((), dtype=d.dtype))
    nn = None
    if return_nn:
        nn = torch.where(live.unsqueeze(-1), knn_gather(p2, idx), torch.zeros((), dtype=p2.dtype))
    return dists, idx, nn


def edge_conv_max(A, Bq, idx, norm=None, slope=0.2):
    """The edge convolution of include/upp_hip.h "edge convolution" as torch operators (any device; differentiable w.r.t. A, Bq, gamma,
    beta): A (B,Nk,O), Bq (B,Nq,O), idx (B,Nq,K) int64, norm None | (G, gamma, beta, eps) -> (B,Nq,O) =
    max_k leaky_relu(group_norm(A[b, idx[b,q,k]] + Bq[b,q])).  It stores the (B,Nq,K,O) tensor the kernels avoid."""
    import torch.nn.functional as F
    B, Nq, K = idx.shape
    O = A.shape[2]
    y = torch.gather(A, 1, idx.reshape(B, Nq * K, 1).expand(-1, -1, O)).view(B, Nq, K, O) + Bq.unsqueeze(2)
    if norm is not None:
        G, gamma, beta, eps = norm
        y = F.group_norm(y.permute(0, 3, 1, 2), int(G), gamma, beta, float(eps)).permute(0, 2, 3, 1)
    return F.leaky_relu(y, float(slope)).max(dim=2)[0]


def expand_act(P, U, Wu, norm=None, slope=0.0):
    """The operator of include/upp_hip.h "broadcast expand" as torch operators (any device and dtype; differentiable): P (R,O), U (S,J)
    shared or (R,S,J) per row, Wu (O,J), norm None | an affine torch.nn.BatchNorm1d (its own training flag and running buffers, updated as
    torch does) -> (R,S,O) = leaky_relu(norm(P[r] + Wu U[., s]), slope).  It stores the y (R,S,O) the kernels avoid."""
    import torch.nn.functional as F
    R, O = P.shape
    S = U.shape[-2]
    y = P.unsqueeze(1) + torch.matmul(U, Wu.t())                   # (R,1,O) + (S,O) | (R,S,O)
    if norm is not None:
        y = norm(y.reshape(R * S, O)).view(R, S, O)
    return F.leaky_relu(y, float(slope))


def query_select(score, cand, Q, extra=None):
    """The selection of include/upp_hip.h "query selection" as torch operators (any device and dtype; differentiable in cand and extra):
    score (B,M), cand (B,M,3), extra (B,D,3) | None -> (out (B,Q+D,3), order (B,Q) int32): the Q candidates of greatest score in
    descending order -- equal scores by ascending index (a stable sort), NaN first -- then the extra points."""
    order = torch.argsort(score.detach(), dim=1, descending=True, stable=True)[:, :int(Q)]
    out = torch.gather(cand, 1, order.unsqueeze(-1).expand(-1, -1, cand.shape[-1]))
    if extra is not None and extra.shape[1] > 0:
        out = torch.cat([out, extra], dim=1)
    return out, order.to(torch.int32)


def cross_attention(q, k, v, num_heads, scale):
    """The cross-attention core of include/upp_hip.h "cross-attention" as torch operators (any device, any head_dim; differentiable):
    q (B,Lq,C), k and v (B,Lk,C) -> (B,Lq,C) = softmax(q k^T scale) v per head (reference models/Transformer.py:148-152).  It keeps the
    (B,H,Lq,Lk) tensor the kernels avoid."""
    B, Lq, C = q.shape
    Lk = k.shape[1]
    H = int(num_heads)
    qh = q.reshape(B, Lq, H, C // H).permute(0, 2, 1, 3)
    kh = k.reshape(B, Lk, H, C // H).permute(0, 2, 1, 3)
    vh = v.reshape(B, Lk, H, C // H).permute(0, 2, 1, 3)
    attn = ((qh @ kh.transpose(-2, -1)) * scale).softmax(dim=-1)
    return (attn @ vh).transpose(1, 2).reshape(B, Lq, C)


def prefix_mask(Lq, Lk, split_q, split_k, device=None):
    """(Lq, Lk) bool, True = hidden: rows < split_q do not see the keys >= split_k (the reference's mask[:-D, -D:] = 1 for
    Lq = Lk = L, both splits L - D)."""
    split_q, split_k = int(split_q), int(split_k)
    if not 0 <= split_q <= Lq or not 1 <= split_k <= Lk:
        raise ValueError("prefix attention needs 0 <= split_q <= Lq and 1 <= split_k <= Lk, got %d, %d for (%d, %d)" % (split_q, split_k, Lq, Lk))
    mask = torch.zeros(Lq, Lk, dtype=torch.bool, device=device)
    mask[:split_q, split_k:] = True
    return mask


def prefix_attention(q, k, v, num_heads, scale, split_q, split_k):
    """The denoising-query attention of include/upp_hip.h as torch operators (any device, any head_dim; differentiable): cross_attention
    with the reference's masked_fill(mask, -finfo.max) before the softmax (models/Transformer_utils.py:107-112).  It keeps the (B,H,Lq,Lk)
    tensor and the (Lq,Lk) mask the kernels avoid."""
    B, Lq, C = q.shape
    Lk = k.shape[1]
    H = int(num_heads)
    qh = q.reshape(B, Lq, H, C // H).permute(0, 2, 1, 3)
    kh = k.reshape(B, Lk, H, C // H).permute(0, 2, 1, 3)
    vh = v.reshape(B, Lk, H, C // H).permute(0, 2, 1, 3)
    attn = (qh @ kh.transpose(-2, -1)) * scale
    attn = attn.masked_fill(prefix_mask(Lq, Lk, split_q, split_k, q.device), -torch.finfo(attn.dtype).max).softmax(dim=-1)
    return (attn @ vh).transpose(1, 2).reshape(B, Lq, C)


def deform_offset(A, Bq, idx, pos, gamma, beta, eps, W3, ball=False):
    """The offset head of include/upp_hip.h "deformable local cross-attention" as torch operators (any device and dtype): A (B,G,NK,C),
    Bq (B,G,N,C), idx (B,N,k) rows of the NK points, pos (B,NK,3), LayerNorm gamma / beta (C) and eps, W3 (3,C) -> shift (B,G,N k,3) =
    pos[idx] + tanh(W3 gelu(LayerNorm(A[idx] + Bq))).  ball ("deformable graph attention"): the tanh is scaled by
    0.5 (max_s pos[idx] - min_s pos[idx]) over the k slots of the query.  It keeps the (B,G,N,k,C) tensor the kernel avoids."""
    import torch.nn.functional as F
    B, G, NK, C = A.shape
    N, k = idx.shape[1], idx.shape[2]
    flat = idx.long().reshape(B, 1, N * k, 1)
    y = torch.gather(A, 2, flat.expand(-1, G, -1, C)).view(B, G, N, k, C) + Bq.unsqueeze(3)
    h = F.gelu(F.layer_norm(y, (C,), gamma, beta, float(eps)))
    off = torch.tanh(torch.matmul(h, W3.t()))                                          # (B,G,N,k,3)
    local = torch.gather(pos, 1, flat.view(B, N * k, 1).expand(-1, -1, 3)).view(B, 1, N, k, 3)
    if ball:
        off = off * ((local.max(dim=3, keepdim=True)[0] - local.min(dim=3, keepdim=True)[0]) * 0.5)
    return (local + off).reshape(B, G, N * k, 3)


def interp_edge_max(PW, Bq, idx3, w3, slope=0.2, pool=None):
    """The interpolate-max of include/upp_hip.h "deformable graph attention" as torch operators (any device and dtype; differentiable in
    PW and Bq): PW (B,NK,O), Bq (B,N,O), idx3 and w3 (B, N k, 3) -> (B,N,O) = leaky_relu(max_s (Bq + sum_j w3 PW[idx3])), j ascending; an
    index outside [0, NK) contributes nothing.  pool: None, or a callable y (B,N,k,O) -> (B,N,O) that takes the place of y.max(2)[0] (the
    modules' arg-max instrument).  It keeps the (B,N,k,O) tensor the kernels avoid."""
    import torch.nn.functional as F
    B, N, O = Bq.shape
    NK = PW.shape[1]
    k = idx3.shape[1] // N
    i = idx3.long()
    inside = ((i >= 0) & (i < NK)).unsqueeze(-1)
    rows = torch.gather(PW, 1, i.clamp(0, NK - 1).reshape(B, N * k * 3, 1).expand(-1, -1, O)).view(B, N * k, 3, O)
    t = torch.where(inside, rows * w3.detach().unsqueeze(-1), torch.zeros((), dtype=PW.dtype, device=PW.device))
    y = Bq.unsqueeze(2)
    for j in range(3):
        y = y + t[:, :, j].view(B, N, k, O)
    return F.leaky_relu(y.max(dim=2)[0] if pool is None else pool(y), float(slope))


def _deform_rows(P, bias, idx3, w3):
    """P (B,G,NK,C), bias (C) | None, idx3 and w3 (B,G,R,3) -> (B,R,C) = bias + sum_g sum_j w3 P_g[idx3] (g, then j ascending): the key /
    value rows of deform_attention and region_attention.  An index outside [0, NK) contributes nothing."""
    B, G, NK, C = P.shape
    i3 = idx3.long()
    inside = ((i3 >= 0) & (i3 < NK)).unsqueeze(-1)
    t = torch.gather(P, 2, i3.clamp(0, NK - 1).reshape(B, G, -1, 1).expand(-1, -1, -1, C)).view(B, G, -1, 3, C) * w3.detach().unsqueeze(-1)
    t = torch.where(inside, t, torch.zeros((), dtype=P.dtype, device=P.device))
    r = None
    for g in range(G):
        for j in range(3):
            r = t[:, g, :, j] if r is None else r + t[:, g, :, j]
    return r if bias is None else r + bias


def deform_attention(q, PK, PV, bk, bv, idx3, w3, num_heads, scale, drop=None):
    """The gather-attend core of include/upp_hip.h "deformable local cross-attention" as torch operators (any device, dtype and
    head_dim; differentiable in q, PK, PV, bk, bv): q (B,N,C), PK / PV (B,G,NK,C), bk / bv (C) | None, idx3 and w3 (B,G,N k,3) ->
    ctx (B,N,C); drop: the module's attention dropout or None.  key_s = bk + sum_g sum_j w3 PK_g[idx3] (g, then j ascending; an idx3
    outside [0, NK) contributes nothing), val_s likewise; softmax over the k slots per head.  It keeps the (B,N,k,C) rows the kernels avoid."""
    B, N, C = q.shape
    H = int(num_heads)
    k = idx3.shape[2] // N
    key, val = (_deform_rows(P, b, idx3, w3).view(B, N, k, H, C // H) for P, b in ((PK, bk), (PV, bv)))
    score = (q.view(B, N, 1, H, C // H) * key).sum(-1) * scale                        # (B,N,k,H)
    p = score.softmax(dim=2)
    if drop is not None:
        p = drop(p)
    return (p.unsqueeze(-1) * val).sum(2).reshape(B, N, C)


def region_attention(q, idx, PK, PV, bk, bv, idx3, w3, num_heads, scale, drop=None, pool=None):
    """The core of include/upp_hip.h "region-wise deformable attention" as torch operators (any device, dtype and head_dim;
    differentiable in q, PK, PV, bk, bv): q (B,N,C), idx (B,N,k) rows of q, PK / PV (B,G,NK,C), bk / bv (C) | None, idx3 and w3
    (B,G,N k,3) -> (B,N,C).  Q_t = q[idx[.,t]] (zero for an index outside [0, N)); key_s = bk + sum_g sum_j w3 PK_g[idx3] (g, then j
    ascending; an idx3 outside [0, NK) contributes nothing), val_s likewise; per head p = softmax_s(scale Q_t . key_s), ctx_t = sum_s
    p[t,s] val_s, out = max_t ctx_t.  drop: the module's attention dropout or None.  pool: None, or a callable ctx (B,N,k,C) -> (B,N,C)
    that takes the place of ctx.max(2)[0] (the modules' arg-max instrument).  It keeps the (B,N,k,C) tensors and the (B,N,H,k,k) scores
    the kernels avoid."""
    B, N, C = q.shape
    H = int(num_heads)
    k = idx.shape[2]
    key, val = (_deform_rows(P, b, idx3, w3).view(B, N, k, H, C // H) for P, b in ((PK, bk), (PV, bv)))
    i = idx.long()
    Q = torch.gather(q, 1, i.clamp(0, N - 1).reshape(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, C)
    Q = torch.where(((i >= 0) & (i < N)).unsqueeze(-1), Q, torch.zeros((), dtype=q.dtype, device=q.device)).view(B, N, k, H, C // H)
    p = (torch.einsum('bnthc,bnshc->bnhts', Q, key) * scale).softmax(dim=-1)
    if drop is not None:
        p = drop(p)
    ctx = torch.einsum('bnhts,bnshc->bnthc', p, val).reshape(B, N, k, C)
    return ctx.max(dim=2)[0] if pool is None else pool(ctx)


def tap_pool(f0, f1, f2, norm, pool=None):
    """include/upp_hip.h upp_tap_pool_fwd as torch operators (any device and dtype; differentiable in the taps and the LayerNorm's
    parameters): f0, f1, f2 (B,G,C), norm an nn.LayerNorm(C) -> x (B,G,3C) = [norm(f0) | norm(f1) | norm(f2)], gmax (B,3C) = x.max(1)[0],
    gmean (B,3C) = (((x[:,0] + x[:,1]) + x[:,2]) + ...) / G -- the kernel's order, one rounded addition per token, not torch.mean's.
    pool: None, or a callable x (B,G,3C) -> (B,3C) that takes the place of x.max(1)[0] (the modules' arg-max instrument)."""
    x = torch.cat([norm(f) for f in (f0, f1, f2)], dim=-1)
    gmax = x.max(dim=1)[0] if pool is None else pool(x)
    s = x[:, 0]
    for g in range(1, x.shape[1]):
        s = s + x[:, g]
    return x, gmax, s / float(x.shape[1])


def chamfer(xyz1, xyz2):
    """-> (dist1 (B,N), dist2 (B,M)) squared nearest-neighbour distances, differentiable (reference extensions/chamfer_dist)."""
    d = ((xyz1.unsqueeze(2) - xyz2.unsqueeze(1)) ** 2).sum(-1)
    return d.min(2)[0], d.min(1)[0]
