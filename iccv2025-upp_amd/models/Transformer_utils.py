"""The building blocks of AdaPoinTr's transformer (reference models/Transformer_utils.py) on the library's kernels: LayerScale, the
neighbour search, Attention with the denoising-query mask, and DynamicGraphAttention.  Class names and state-dict keys are the
reference's, so its checkpoints load with strict=True.
    Attention(x)                            upp_layers.Attention: HF.linear + HF.attention + HF.linear
    Attention(x, denoise_length=D)          the last D of the N tokens are denoising queries: the first N - D tokens see only each other,
                                            the last D see all N (reference models/AdaPoinTr.py:224-229).  HF.linear for the qkv product,
                                            HF.prefix_attention on its three views with both splits N - D, HF.linear for proj: no (N, N)
                                            mask, no (B, H, N, N) scores
    Attention(x, mask=<tensor>)             an arbitrary mask: the reference's torch formulation (masked_fill + softmax); recorded by
                                            HF.note_declined on a HIP tensor
    DynamicGraphAttention                   max_k lrelu(Linear([f_j - f_i ; f_i])) over k listed neighbours: DecoderBlock.local_branch, i.e.
                                            two per-point products and HF.edge_conv_max without a norm (no (B, N, k, 2 dim) tensor)
    knn_point                               HF.knn_query
    DeformableLocalCrossAttention           the deformable local attention (block token `deform`): the offset head and the key / value
                                            projections taken through the gather as per-point products, HF.deform_offset, HF.three_nn and
                                            HF.deform_attention -- no (B, N, k, C) tensor (README "Deformable local cross-attention")
    improvedDeformableLocalCrossAttention   the same with the offset scaled to the local ball: HF.deform_offset(ball=True)
    improvedDeformableLocalGraphAttention   the deformable graph feature (block token `deform_graph`): the ball-scaled offset head with
                                            G = 1, HF.three_nn and HF.interp_edge_max -- max over the slots of three interpolated rows
                                            plus the query half, no (B, N, k, C) tensor (README "Deformable graph attention")
    DeformableLocalAttention                the region-wise deformable self-attention (block token `rw_deform`): the same offset head,
                                            HF.three_nn and per-point products, then HF.region_attention -- a k x k attention per token
                                            and head and the max over its rows, no (B, N, k, C) tensor and no (B H N, k, k) scores (README
                                            "Region-wise deformable attention")
    DeformableAttnBlock, DeformableAttnDecoderBlock, RegionWiseBlock   the reference's fixed layouts around them
    _neighbour_list, _sample                what the modules above share: the head of every forward (defaults, checks, the neighbour
                                            list) and the deformable modules' sampling positions (offset head, three_nn, weights)
The fused attention path is taken for HIP f32 tensors with head_dim 64, N <= HF.ATTN_MAX_L and no active attention dropout; otherwise
the same module runs the torch formulation, and a HIP tensor that was declined is recorded by HF.note_declined.

Deliberate deviation (README "Denoising-query attention and the AdaPoinTr blocks"): the reference picks the k neighbours with
topk(sorted=False) of |a|^2 + |b|^2 - 2ab; here the set is the library's ascending (distance, index) on the direct squared distance.  The
sets agree wherever the k-th and (k+1)-th distances differ by more than rounding, and the order inside a set does not matter under the max.

Not ported: the other fixed-layout Block / DecoderBlock variants of the reference file, which models/AdaPoinTr.py does not use."""
import torch
import torch.nn as nn

from upp_hip import functional as HF
from upp_hip import ops, torch_cpu
from . import upp_layers as L
from .upp_layers import CrossAttention, DecoderBlock, DropPath, Mlp, index_points, square_distance  # noqa: F401  (the reference's names)


class LayerScale(nn.Module):
    def __init__(self, dim, init_values=1e-5, inplace=False):
        super().__init__()
        self.inplace = inplace
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x.mul_(self.gamma) if self.inplace else x * self.gamma


def knn_point(nsample, xyz, new_xyz):
    """xyz (B,N,3) all points, new_xyz (B,S,3) queries -> (B,S,nsample) int64 rows of xyz: the nsample nearest points of every query in the
    library's ascending (distance, index); no gradient."""
    with torch.no_grad():
        idx = HF.knn_query(xyz.detach().contiguous(), new_xyz.detach().contiguous(), int(nsample))[1].long()
    return L.trace_idx('transformer_utils.knn_point', idx)


def denoise_knn(k, pos, denoise_length):
    """The self-branch neighbour list of N = R + D tokens of which the last D are denoising queries (reference
    models/Transformer_utils.py:835-850): the first R positions search among themselves, the last D among all N -> one (B,N,k) int64 list
    over the N rows (rows < R carry the same numbers in both numberings)."""
    N, D = pos.shape[1], int(denoise_length)
    if not 1 <= D < N:
        raise ValueError("denoise_length must be in [1, N - 1] = [1, %d], got %d" % (N - 1, D))
    if N - D < k:
        raise ValueError("denoise_length %d leaves %d real tokens for %d neighbours" % (D, N - D, k))
    return torch.cat([knn_point(k, pos[:, :N - D], pos[:, :N - D]), knn_point(k, pos, pos[:, N - D:])], dim=1)


class Attention(L.Attention):
    """reference models/Transformer_utils.py:87-120.  forward(x (B,N,dim), mask=None, denoise_length=None); at most one of the two.
    State-dict keys: qkv, proj."""

    def _masked_torch(self, x, hidden):
        """the reference's formulation with `hidden` (N,N) bool, True = masked"""
        B, N, C = x.shape
        qkv = self.qkv(x).view(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn = (q @ k.transpose(-2, -1)) * self.scale
        attn = self.attn_drop(attn.masked_fill(hidden, -torch.finfo(attn.dtype).max).softmax(dim=-1))
        x = (attn @ v).transpose(1, 2).reshape(B, N, C)
        return self.proj_drop(self.proj(x))

    def forward(self, x, mask=None, denoise_length=None):
        if mask is None and denoise_length is None:
            return super().forward(x)
        if mask is not None and denoise_length is not None:
            raise ValueError("Attention takes a mask tensor or denoise_length, not both")
        B, N, C = x.shape
        if mask is not None:
            if x.is_cuda:
                HF.note_declined("Attention (%d,%d) with a mask tensor, %d heads" % (N, C, self.num_heads),
                                 "an arbitrary mask has no kernel; denoise_length does")
            return self._masked_torch(x, mask > 0)
        D = int(denoise_length)
        if not 1 <= D < N:
            raise ValueError("denoise_length must be in [1, N - 1] = [1, %d], got %d" % (N - 1, D))
        if self.fusable(x):
            qkv = HF.linear(x, self.qkv.weight, self.qkv.bias).view(B, N, 3, C)
            ctx = HF.prefix_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], self.num_heads, self.scale, N - D, N - D)
            return self.proj_drop(HF.linear(ctx, self.proj.weight, self.proj.bias))
        if x.is_cuda:
            HF.note_declined("Attention (%d,%d) with denoise_length %d, %d heads" % (N, C, D, self.num_heads),
                             "head_dim != 64 / a length beyond %d / dtype / attention dropout" % HF.ATTN_MAX_L)
        return self._masked_torch(x, torch_cpu.prefix_mask(N, N, N - D, N - D, x.device))


def _neighbour_list(m, q, q_pos, v, v_pos, idx, denoise_length, branch=False):
    """The head of every forward below, for module m (its dim and k) -> (v, v_pos, idx): v / v_pos default to q / q_pos (the self form),
    the shapes are checked, and idx (B,N,k) is searched when None -- with denoise_length by denoise_knn, which is for the self form and
    the list computed here only.  branch: DynamicGraphAttention, whose callers can supply that list and know the form as a branch."""
    if denoise_length is not None:
        if idx is not None and not branch:
            raise ValueError("denoise_length needs the list computed here, but idx is given")
        if v is not None or v_pos is not None:
            raise ValueError("denoise_length applies to the self %s only, but v / v_pos is given" % ("branch" if branch else "form"))
    v = q if v is None else v
    v_pos = q_pos if v_pos is None else v_pos
    if q_pos.dim() != 3 or q_pos.size(-1) != 3 or v_pos.dim() != 3 or v_pos.size(-1) != 3:
        raise ValueError("q_pos and v_pos must be (B, N, 3), got %s and %s" % (tuple(q_pos.shape), tuple(v_pos.shape)))
    if q.size(-1) != m.dim or v.size(-1) != m.dim:
        raise ValueError("q and v must have %d channels, got %d and %d" % (m.dim, q.size(-1), v.size(-1)))
    if idx is None:
        idx = knn_point(m.k, v_pos, q_pos) if denoise_length is None else denoise_knn(m.k, q_pos, denoise_length)
    if idx.shape != (q.shape[0], q.shape[1], m.k):
        raise ValueError("idx must be (B, N, k) = %s, got %s" % ((q.shape[0], q.shape[1], m.k), tuple(idx.shape)))
    return v, v_pos, idx


class DynamicGraphAttention(nn.Module):
    """reference models/Transformer_utils.py:777-858: the graph feature of every query token over k neighbour tokens.
    forward(q (B,N,dim), q_pos (B,N,3), v=None, v_pos=None, idx=None, denoise_length=None) -> (B,N,dim); v / v_pos default to q / q_pos
    (a self branch); idx (B,N,k) rows of v, searched here when None.  With denoise_length and no idx the list is denoise_knn's.  (The
    reference refuses idx together with denoise_length because its callers cannot supply that list; models/AdaPoinTr.py here computes it
    once per forward and passes it in.)  State-dict keys: knn_map.0."""

    def __init__(self, dim, k=10):
        super().__init__()
        self.dim = dim
        self.k = k
        self.knn_map = nn.Sequential(nn.Linear(dim * 2, dim), nn.LeakyReLU(negative_slope=0.2))

    def forward(self, q, q_pos, v=None, v_pos=None, idx=None, denoise_length=None):
        v, _, idx = _neighbour_list(self, q, q_pos, v, v_pos, idx, denoise_length, branch=True)
        return DecoderBlock.local_branch(self.knn_map, v, q, idx)


def shifted_three_nn(shift, known):
    """shift (R,n,3) the shifted neighbour positions, known (R,m,3) -> (dist (R,n,3) Euclidean ascending, idx3 (R,n,3) int32): HF.three_nn
    for HIP f32 tensors, its torch formulation elsewhere (any device and dtype); no gradient."""
    with torch.no_grad():
        if shift.is_cuda and shift.dtype == torch.float32:
            return HF.three_nn(shift.contiguous(), known.contiguous())
        return torch_cpu.three_nn(shift, known)


def _sample(m, q_off, v, v_pos, idx, fused):
    """The sampling positions of the deformable modules, for module m (proj_v_off, linear_offset, k, n_group, ball, trace_site): q_off
    (B,N,dim) the query side of the offset head, v (B,NK,dim), v_pos (B,NK,3), idx (B,N,k) -> idx3 int32, w3 (B,G,N k,3).  Per group g of
    c = dim / G channels, with linear_offset.0.weight = [Wa | Wb]: Linear([v_off_g[idx] ; q_g]) = A_g[idx] + Bq_g with A_g = v_off_g Wa^T
    over the NK points and Bq_g = q_g Wb^T + b over the N queries; deform_offset does gather, LayerNorm, GELU, the 3-row Linear, tanh and
    the shift; three_nn of the shifted positions among v_pos; weights by the reference's own r = 1 / (dist + 1e-8), r / r.sum(-1) in torch,
    so that they carry its rounding.  fused: the library's kernels (G = 1 takes A / Bq as views and v_pos as it is: no copy); otherwise
    torch operators on any device and dtype, which under upp_layers.POOL_TRACE record or replay idx3.  No gradient."""
    B, N, _ = q_off.shape
    NK, G, c, lin0, ln = v.shape[1], m.n_group, m.dim // m.n_group, m.linear_offset[0], m.linear_offset[1]
    with torch.no_grad():
        pos = v_pos.detach().contiguous()
        if not fused:
            A = torch.matmul(m.proj_v_off(v).view(B, NK, G, c).permute(0, 2, 1, 3), lin0.weight[:, :c].t())
            Bq = torch.matmul(q_off.reshape(B, N, G, c).permute(0, 2, 1, 3), lin0.weight[:, c:].t()) + lin0.bias
        else:
            v_off = HF.linear(v.detach(), m.proj_v_off.weight, m.proj_v_off.bias)
            Wa, Wb = lin0.weight[:, :c].contiguous(), lin0.weight[:, c:].contiguous()
            if G == 1:
                A, Bq = HF.linear(v_off, Wa).unsqueeze(1), HF.linear(q_off.detach(), Wb, lin0.bias).unsqueeze(1)
            else:
                vg, qg = _grouped(v_off, G), _grouped(q_off.detach(), G)
                A = torch.stack([HF.linear(vg[g], Wa) for g in range(G)], dim=1)                    # (B,G,NK,C)
                Bq = torch.stack([HF.linear(qg[g], Wb, lin0.bias) for g in range(G)], dim=1)        # (B,G,N,C)
        shift = (HF if fused else torch_cpu).deform_offset(A, Bq, idx, pos, ln.weight, ln.bias, ln.eps, m.linear_offset[3].weight, ball=m.ball)
        flat = shift.reshape(B * G, N * m.k, 3)
        known = pos if G == 1 else pos.unsqueeze(1).expand(-1, G, -1, -1).reshape(B * G, NK, 3)
        dist, idx3 = shifted_three_nn(flat, known)
        if not fused and L.POOL_TRACE is not None:
            # the recorded choice replaces this run's, and the distances follow it (slots beyond NK < 3 points stay at +inf)
            idx3 = L.trace_idx(m.trace_site, idx3)
            near = torch.gather(known, 1, idx3.long().reshape(B * G, -1, 1).expand(-1, -1, 3)).view(B * G, -1, 3, 3)
            d = (flat.unsqueeze(2) - near).pow(2).sum(-1).sqrt()
            dist = torch.where(torch.arange(3, device=d.device) < NK, d, torch.full_like(d, float('inf')))
        r = 1.0 / (dist + 1e-8)
        return idx3.view(B, G, N * m.k, 3), (r / torch.sum(r, dim=-1, keepdim=True)).view(B, G, N * m.k, 3)


def _grouped(x, G):
    """(B,M,dim) -> (G,B,M,dim / G) contiguous: the channel groups as whole matrices"""
    B, M, C = x.shape
    return x.view(B, M, G, C // G).permute(2, 0, 1, 3).contiguous()


class DeformableLocalCrossAttention(nn.Module):
    """reference models/Transformer_utils.py:269-491: every query attends over k neighbour slots whose keys and values are
    interpolated at learned, shifted positions.  forward(q (B,N,dim), q_pos (B,N,3), v=None (B,NK,dim), v_pos=None (B,NK,3), idx=None
    (B,N,k) rows of v, denoise_length=None) -> (B,N,dim); v / v_pos default to q / q_pos (the self form).  With denoise_length = D (self
    form only; v, v_pos and idx must be None, as in the reference) the list is denoise_knn's.
    State-dict keys: proj_q, proj_k, proj_v, proj_v_off, proj, linear_offset.{0,1,3}.

    Per group g of c = dim / n_group channels:
        idx3, w3        _sample with proj_q(q) on the query side: the offset head, three_nn of the shifted positions, the weights
        keys, values    proj_k(interp)[n,s] = b_k + sum_g sum_j w[g,n,s,j] PK_g[idx3[g,n,s,j]] with PK_g = v_g Wk[:, g-slice]^T over the
                        NK points, likewise proj_v; HF.deform_attention gathers, scores, normalises and sums
    three_nn is not differentiable (as upstream marks dist and idx), so the offset branch -- proj_v_off, linear_offset -- and the
    positions get no gradient: it runs under no_grad.  The fused path is taken for HIP f32 tensors in the served range (head_dim 64, at
    most 16 heads, k <= 32) with no active attention dropout and upp_layers.POOL_TRACE unset; otherwise the torch formulation
    (upp_hip.torch_cpu.deform_offset / deform_attention, which keep the (B,N,k,C) tensors) runs and a HIP tensor that was declined is
    recorded by HF.note_declined.  The neighbour set is the library's ascending (distance, index), as for the other modules."""

    ball = False        # improvedDeformableLocalCrossAttention: the offset is scaled by half the extent of the k listed positions
    trace_site = 'deformable_attention.idx3'

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., k=10, n_group=2):
        super().__init__()
        if dim % num_heads or dim % n_group or num_heads % n_group:
            raise ValueError("DeformableLocalCrossAttention: num_heads must divide dim and n_group must divide both, got dim %d, "
                             "%d heads, %d groups" % (dim, num_heads, n_group))
        self.num_heads = num_heads
        self.dim = dim
        self.head_dim = dim // num_heads
        self.scale = qk_scale or self.head_dim ** -0.5
        self.proj_q = nn.Linear(dim, dim, bias=qkv_bias)
        self.proj_k = nn.Linear(dim, dim, bias=qkv_bias)
        self.proj_v = nn.Linear(dim, dim, bias=qkv_bias)
        self.proj_v_off = nn.Linear(dim, dim, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.k = k
        self.n_group = n_group
        self.group_dims = dim // n_group
        self.linear_offset = nn.Sequential(nn.Linear(2 * self.group_dims, dim), nn.LayerNorm(dim), nn.GELU(), nn.Linear(dim, 3, bias=False))

    def fusable(self, q, v):
        """The kernels serve HIP f32 tensors, head_dim 64, <= 16 heads, k <= 32 and no active attention dropout."""
        return (q.is_cuda and v.is_cuda and q.dtype == torch.float32 and v.dtype == torch.float32 and self.dim == 64 * self.num_heads
                and not (self.training and self.attn_drop.p > 0) and L.POOL_TRACE is None
                and ops.deform_attn_usable(q.shape[0], q.shape[1], v.shape[1], self.k, self.num_heads, self.n_group))

    def _operands(self, q, v, v_pos, idx, fused):
        """-> (proj_q(q), PK, PV, idx3, w3): everything in front of the attention core, on the library's kernels (fused) or as torch
        operators, any device and dtype"""
        C, G, c = self.dim, self.n_group, self.group_dims
        qp = HF.linear(q, self.proj_q.weight, self.proj_q.bias) if fused else self.proj_q(q)
        idx3, w3 = _sample(self, qp.detach(), v, v_pos, idx, fused)
        Wk, Wv = self.proj_k.weight, self.proj_v.weight
        if fused:
            vg = _grouped(v, G)
            PK = torch.stack([HF.linear(vg[g], Wk[:, g * c:(g + 1) * c].contiguous()) for g in range(G)], dim=1)
            PV = torch.stack([HF.linear(vg[g], Wv[:, g * c:(g + 1) * c].contiguous()) for g in range(G)], dim=1)
        else:
            vg = v.view(v.shape[0], v.shape[1], G, c).permute(0, 2, 1, 3)
            PK = torch.matmul(vg, Wk.view(C, G, c).permute(1, 2, 0))
            PV = torch.matmul(vg, Wv.view(C, G, c).permute(1, 2, 0))
        return qp, PK, PV, idx3, w3

    def _fused(self, q, v, v_pos, idx):
        qp, PK, PV, idx3, w3 = self._operands(q, v, v_pos, idx, True)
        ctx = HF.deform_attention(qp, PK, PV, self.proj_k.bias, self.proj_v.bias, idx3, w3, self.num_heads, self.scale)
        return self.proj_drop(HF.linear(ctx, self.proj.weight, self.proj.bias))

    def _torch(self, q, v, v_pos, idx):
        """the same restatement as torch operators, any device and dtype"""
        qp, PK, PV, idx3, w3 = self._operands(q, v, v_pos, idx, False)
        drop = self.attn_drop if self.training and self.attn_drop.p > 0 else None
        ctx = torch_cpu.deform_attention(qp, PK, PV, self.proj_k.bias, self.proj_v.bias, idx3, w3, self.num_heads, self.scale, drop)
        return self.proj_drop(self.proj(ctx))

    def forward(self, q, q_pos, v=None, v_pos=None, idx=None, denoise_length=None):
        v, v_pos, idx = _neighbour_list(self, q, q_pos, v, v_pos, idx, denoise_length)
        idx = idx.long()
        if self.fusable(q, v):
            return self._fused(q, v, v_pos, idx)
        if q.is_cuda and L.POOL_TRACE is None:
            HF.note_declined("DeformableLocalCrossAttention (%d,%d) x (%d,%d), %d heads, k = %d"
                             % (q.shape[1], self.dim, v.shape[1], self.dim, self.num_heads, self.k),
                             "head_dim != 64 / more than 16 heads / k > 32 / dtype / attention dropout")
        return self._torch(q, v, v_pos, idx)


class improvedDeformableLocalCrossAttention(DeformableLocalCrossAttention):
    """reference models/Transformer_utils.py:493-621: DeformableLocalCrossAttention whose offsets stay within the local ball --
    shift = pos[idx] + tanh(.) * 0.5 (max_s pos[idx] - min_s pos[idx]) (HF.deform_offset(ball=True)) -- and, as in the reference, without
    a denoise_length argument.  forward(q, q_pos, v=None, v_pos=None, idx=None).  The same 15 state-dict keys."""

    ball = True

    def forward(self, q, q_pos, v=None, v_pos=None, idx=None):
        return super().forward(q, q_pos, v, v_pos, idx)


class DeformableLocalAttention(DeformableLocalCrossAttention):
    """reference models/Transformer_utils.py:159-266 (block token `rw_deform`): region-wise deformable SELF attention.  Every token
    gathers the projected query rows of its k neighbours, runs a full k x k softmax attention per head of those k rows against k keys
    and values interpolated at learned, shifted positions, and keeps the per-channel maximum over the k context rows.
    forward(x (B,N,dim), pos (B,N,3), idx=None (B,N,k) rows of x) -> (B,N,dim).  The reference's 15 state-dict keys: proj_q, proj_k,
    proj_v, proj_v_off, proj, linear_offset.{0,1,3}.

    Everything in front of the core is DeformableLocalCrossAttention's self form (v = x, q = proj_q(x), ball = False) and is shared
    with it, not copied: the offset head through the gather (HF.deform_offset), HF.three_nn with the reference's weights, and the
    commuted per-point products PK / PV.  The core is HF.region_attention: Q_t = proj_q(x)[idx[., t]], S = scale Q K^T over the k x k
    pairs, softmax over s, ctx = p V, max over t -- no (B,N,k,C) tensor and no (B H N, k, k) scores in memory.  The offset branch --
    proj_v_off, linear_offset -- and the positions get no gradient (three_nn is not differentiable): it runs under no_grad.  The fused
    path is taken for HIP f32 tensors in the served range (head_dim 64, at most 16 heads, k <= 32) with no active attention dropout
    and upp_layers.POOL_TRACE unset; otherwise the torch formulation (upp_hip.torch_cpu.region_attention, which keeps the (B,N,k,C)
    tensors) runs and a HIP tensor that was declined is recorded by HF.note_declined.  Under POOL_TRACE the torch formulation records
    and replays idx3 and the arg of the max.  The module has no denoising form (the reference's has no denoise_length argument)."""

    trace_site = 'region_attention.idx3'

    def fusable(self, q, v):
        return (super().fusable(q, v) and ops.region_attn_usable(q.shape[0], q.shape[1], v.shape[1], self.k, self.num_heads, self.n_group))

    def _fused(self, q, v, v_pos, idx):
        qp, PK, PV, idx3, w3 = self._operands(q, v, v_pos, idx, True)
        out = HF.region_attention(qp, idx, PK, PV, self.proj_k.bias, self.proj_v.bias, idx3, w3, self.num_heads, self.scale)
        return self.proj_drop(HF.linear(out, self.proj.weight, self.proj.bias))

    def _torch(self, q, v, v_pos, idx):
        qp, PK, PV, idx3, w3 = self._operands(q, v, v_pos, idx, False)
        drop = self.attn_drop if self.training and self.attn_drop.p > 0 else None
        pool = None if L.POOL_TRACE is None else (lambda y: L.max_over(y, 2, 'region_attention.max'))
        out = torch_cpu.region_attention(qp, idx, PK, PV, self.proj_k.bias, self.proj_v.bias, idx3, w3, self.num_heads, self.scale, drop, pool)
        return self.proj_drop(self.proj(out))

    def forward(self, x, pos, idx=None):
        idx = _neighbour_list(self, x, pos, None, None, idx, None)[2].long()
        if self.fusable(x, x):
            return self._fused(x, x, pos, idx)
        if x.is_cuda and L.POOL_TRACE is None:
            HF.note_declined("DeformableLocalAttention (%d,%d), %d heads, k = %d" % (x.shape[1], self.dim, self.num_heads, self.k),
                             "head_dim != 64 / more than 16 heads / k > 32 / dtype / attention dropout")
        return self._torch(x, x, pos, idx)


class improvedDeformableLocalGraphAttention(nn.Module):
    """reference models/Transformer_utils.py:623-775 (block token `deform_graph`): the graph feature of every query over k neighbour
    slots whose features are interpolated at learned positions, shifted within the local ball.  forward(q (B,N,dim), q_pos (B,N,3),
    v=None (B,NK,dim), v_pos=None (B,NK,3), idx=None (B,N,k) rows of v, denoise_length=None) -> (B,N,dim); v / v_pos default to q / q_pos
    (the self form).  With denoise_length = D (self form only; v, v_pos and idx must be None, as the reference asserts) the list is
    denoise_knn's.  State-dict keys: proj_v_off, linear_offset.{0,1,3}, knn_map.0.

    With knn_map.0.weight = [W1 | W2] (no proj_q, no heads, no channel groups: G = 1):
        idx3, w3        _sample with the RAW q on the query side and ball = True -- the tanh scaled by 0.5 (max_s pos[idx] - min_s
                        pos[idx]) -- and of its (B,1,N k,3) results the G = 1 slice
        graph feature   knn_map([f - q ; q]) = W1 f + (W2 - W1) q + b and f = sum_j w3 v[idx3], so y[n,s] = Bq'[n] + sum_j w3[n,s,j]
                        PW[idx3[n,s,j]] with PW = v W1^T over the NK points and Bq' = q (W2 - W1)^T + b over the N queries;
                        HF.interp_edge_max gathers, interpolates in registers, takes the max over the slots and applies the LeakyReLU
    three_nn is not differentiable, so the offset branch -- proj_v_off, linear_offset -- and the positions get no gradient: it runs under
    no_grad.  The fused path is taken for HIP f32 tensors in the served range (dim a multiple of 64 up to 1024, k <= 32) with
    upp_layers.POOL_TRACE unset; otherwise the torch formulation (upp_hip.torch_cpu.deform_offset / interp_edge_max, which keep the
    (B,N,k,C) tensors) runs, and a HIP tensor that was declined is recorded by HF.note_declined.  Under POOL_TRACE the torch formulation
    records and replays idx3 and the arg of the max.  The neighbour set is the library's ascending (distance, index)."""

    n_group, ball, trace_site = 1, True, 'deformable_graph.idx3'        # (what _sample reads beside proj_v_off, linear_offset and k)

    def __init__(self, dim, k=10):
        super().__init__()
        self.dim = dim
        self.proj_v_off = nn.Linear(dim, dim)
        self.k = k
        self.linear_offset = nn.Sequential(nn.Linear(2 * dim, dim), nn.LayerNorm(dim), nn.GELU(), nn.Linear(dim, 3, bias=False))
        self.knn_map = nn.Sequential(nn.Linear(dim * 2, dim), nn.LeakyReLU(negative_slope=0.2))

    def fusable(self, q, v):
        """The kernels serve HIP f32 tensors, dim = 64 H <= 1024 and k <= 32."""
        return (q.is_cuda and v.is_cuda and q.dtype == torch.float32 and v.dtype == torch.float32 and self.dim % 64 == 0
                and L.POOL_TRACE is None and ops.deform_attn_usable(q.shape[0], q.shape[1], v.shape[1], self.k, self.dim // 64, 1)
                and ops.interp_max_usable(q.shape[0], q.shape[1], v.shape[1], self.k, self.dim))

    def _fused(self, q, v, v_pos, idx):
        C, lin, act = self.dim, self.knn_map[0], self.knn_map[1]
        idx3, w3 = _sample(self, q, v, v_pos, idx, True)
        W = lin.weight
        PW = HF.linear(v, W[:, :C].contiguous())
        Bm = HF.linear(q, W[:, C:] - W[:, :C], lin.bias)
        return HF.interp_edge_max(PW, Bm, idx3[:, 0], w3[:, 0], act.negative_slope)

    def _torch(self, q, v, v_pos, idx):
        """the same restatement as torch operators, any device and dtype"""
        C, lin, act = self.dim, self.knn_map[0], self.knn_map[1]
        idx3, w3 = _sample(self, q, v, v_pos, idx, False)
        W = lin.weight
        PW = torch.matmul(v, W[:, :C].t())
        Bm = torch.matmul(q, (W[:, C:] - W[:, :C]).t()) + lin.bias
        pool = None if L.POOL_TRACE is None else (lambda y: L.max_over(y, 2, 'deformable_graph.max'))
        return torch_cpu.interp_edge_max(PW, Bm, idx3[:, 0], w3[:, 0], act.negative_slope, pool)

    def forward(self, q, q_pos, v=None, v_pos=None, idx=None, denoise_length=None):
        v, v_pos, idx = _neighbour_list(self, q, q_pos, v, v_pos, idx, denoise_length)
        idx = idx.long()
        if self.fusable(q, v):
            return self._fused(q, v, v_pos, idx)
        if q.is_cuda and L.POOL_TRACE is None:
            HF.note_declined("improvedDeformableLocalGraphAttention (%d,%d) x (%d,%d), k = %d" % (q.shape[1], self.dim, v.shape[1], self.dim, self.k),
                             "dim not a multiple of 64 / beyond 1024 / k > 32 / dtype")
        return self._torch(q, v, v_pos, idx)


class RegionWiseBlock(nn.Module):
    """reference models/Transformer_utils.py:894-915: x + region-wise deformable attention, x + MLP.  forward(x (B,N,dim), pos (B,N,3)).
    The forward is the reference's AS WRITTEN THERE: the MLP branch is normalised by norm1, not norm2.  norm2 exists (two state-dict
    keys, so the reference's checkpoints load with strict=True), is never applied, and its parameters end with grad None."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., init_values=None, drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.deformable_attn = DeformableLocalAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.ls1 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    def forward(self, x, pos):
        x = x + self.drop_path1(self.ls1(self.deformable_attn(HF.layer_norm(x, self.norm1), pos)))
        return x + self.drop_path2(self.ls2(self.mlp(HF.layer_norm(x, self.norm1))))


class DeformableAttnBlock(nn.Module):
    """reference models/Transformer_utils.py:917-935: x + deformable self-attention, x + MLP.  forward(x (B,N,dim), pos (B,N,3))."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., init_values=None, drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.deformable_attn = DeformableLocalCrossAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.ls1 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    def forward(self, x, pos):
        x = x + self.drop_path1(self.ls1(self.deformable_attn(HF.layer_norm(x, self.norm1), pos)))
        return x + self.drop_path2(self.ls2(self.mlp(HF.layer_norm(x, self.norm2))))


class DeformableAttnDecoderBlock(nn.Module):
    """reference models/Transformer_utils.py:988-1015: self-attention over the queries, deformable cross-attention over the memory
    tokens, an MLP.  forward(q (B,N,dim), v (B,NK,dim), q_pos (B,N,3), v_pos (B,NK,3))."""

    def __init__(self, dim, num_heads, dim_q=None, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., init_values=None, drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.self_attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.norm_q = norm_layer(dim_q or dim)
        self.norm_v = norm_layer(dim)
        self.attn = DeformableLocalCrossAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path1 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.drop_path3 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.ls1 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.ls3 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()

    def forward(self, q, v, q_pos, v_pos):
        q = q + self.drop_path1(self.ls1(self.self_attn(HF.layer_norm(q, self.norm1))))
        q = q + self.drop_path2(self.ls2(self.attn(q=HF.layer_norm(q, self.norm_q), v=HF.layer_norm(v, self.norm_v), q_pos=q_pos, v_pos=v_pos)))
        return q + self.drop_path3(self.ls3(self.mlp(HF.layer_norm(q, self.norm2))))
