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
The fused attention path is taken for HIP f32 tensors with head_dim 64, N <= HF.ATTN_MAX_L and no active attention dropout; otherwise
the same module runs the torch formulation, and a HIP tensor that was declined is recorded by HF.note_declined.

Deliberate deviation (README "Denoising-query attention and the AdaPoinTr blocks"): the reference picks the k neighbours with
topk(sorted=False) of |a|^2 + |b|^2 - 2ab; here the set is the library's ascending (distance, index) on the direct squared distance.  The
sets agree wherever the k-th and (k+1)-th distances differ by more than rounding, and the order inside a set does not matter under the max.

Not ported: DeformableLocalAttention, DeformableLocalCrossAttention, improvedDeformableLocalCrossAttention,
improvedDeformableLocalGraphAttention (the block tokens rw_deform, deform, deform_graph) and the fixed-layout Block / DecoderBlock
variants of the reference file, which models/AdaPoinTr.py does not use."""
import torch
import torch.nn as nn

from upp_hip import functional as HF
from upp_hip import torch_cpu
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
        if denoise_length is not None and (v is not None or v_pos is not None):
            raise ValueError("denoise_length applies to the self branch only, but v / v_pos is given")
        v = q if v is None else v
        v_pos = q_pos if v_pos is None else v_pos
        if q_pos.dim() != 3 or q_pos.size(-1) != 3 or v_pos.dim() != 3 or v_pos.size(-1) != 3:
            raise ValueError("q_pos and v_pos must be (B, N, 3), got %s and %s" % (tuple(q_pos.shape), tuple(v_pos.shape)))
        if q.size(-1) != self.dim or v.size(-1) != self.dim:
            raise ValueError("q and v must have %d channels, got %d and %d" % (self.dim, q.size(-1), v.size(-1)))
        if idx is None:
            idx = knn_point(self.k, v_pos, q_pos) if denoise_length is None else denoise_knn(self.k, q_pos, denoise_length)
        if idx.shape != (q.shape[0], q.shape[1], self.k):
            raise ValueError("idx must be (B, N, k) = %s, got %s" % ((q.shape[0], q.shape[1], self.k), tuple(idx.shape)))
        return DecoderBlock.local_branch(self.knn_map, v, q, idx)
