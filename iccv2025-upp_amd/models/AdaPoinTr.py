"""The configurable encoder / decoder blocks of AdaPoinTr and their stacks (reference models/AdaPoinTr.py:15-507) on the library's kernels.
Class names and state-dict keys are the reference's, so its checkpoints load with strict=True.

A block style is one or two tokens joined by '-'.  Served tokens: `attn` (global attention) and `graph` (DynamicGraphAttention), alone or
paired, combined by `concat` (both on one normalised input, merged by a Linear over the concatenation) or `onebyone` (one residual
branch each).  The tokens `deform` (Transformer_utils.DeformableLocalCrossAttention) and `deform_graph`
(Transformer_utils.improvedDeformableLocalGraphAttention) are served behind the keyword `deformable` of the block APIs, the stacks and
the two Point* classes, which PCTransformer and the *Entry classes read from a model config:
    token           built as                                   opted in by
    attn, graph     Attention / CrossAttention, DynamicGraphAttention          always served
    deform          DeformableLocalCrossAttention              deformable=True, or a collection that names it (`deformable: true`)
    deform_graph    improvedDeformableLocalGraphAttention      a collection that names it (`deformable: [deform, deform_graph]`)
    rw_deform       DeformableLocalAttention                   the separate keyword region_wise=True (`region_wise: true`)
True means exactly {'deform'}; a name outside ('deform', 'deform_graph') raises ValueError; with the defaults every one of the three
deformable tokens raises ValueError at construction.  `rw_deform` is a self-attention only: with region_wise=True it is built in
SelfAttnBlockApi and in CrossAttnBlockApi's self position (k, n_group from the block) and raises ValueError in the cross position, as
the reference asserts.  The module has no denoising form: in the decoder's self position a non-None denoise_length raises ValueError.
Deliberate deviation: the reference passes denoise_length to the module unconditionally there and would raise TypeError even for None;
serving denoise_length=None is this repository's.  `deformable` never opts `rw_deform` in.
    LayerNorm                      HF.layer_norm (the row kernel; eps from the module, 1e-6 in the stacks)
    self-attention                 Transformer_utils.Attention; with denoise_length the fused prefix-visibility kernel -- CrossAttnBlockApi
                                   passes denoise_length on and never builds the reference's (N, N) mask tensor
    cross-attention                upp_layers.CrossAttention (HF.cross_attention)
    graph branches                 Transformer_utils.DynamicGraphAttention (HF.edge_conv_max)
    deformable branches            Transformer_utils.DeformableLocalCrossAttention (HF.deform_offset, HF.three_nn, HF.deform_attention)
    deformable graph branches      Transformer_utils.improvedDeformableLocalGraphAttention (HF.deform_offset(ball=True), HF.three_nn,
                                   HF.interp_edge_max)
    region-wise branches           Transformer_utils.DeformableLocalAttention (HF.deform_offset, HF.three_nn, HF.region_attention)
    merge maps                     HF.linear;  MLPs: upp_layers.Mlp (HF.mlp_gelu)
TransformerEncoder / TransformerDecoder compute every neighbour list once per forward -- the denoise list included, which the reference
recomputes inside every block; positions do not change between blocks, so the lists are the same -- and only the lists some block uses.

PCTransformer and AdaPoinTr (reference models/AdaPoinTr.py:737-997) are built from those stacks and
    grouper           dgcnn_group.DGCNN_Grouper.forward(x, num); encoder_type 'pn' (SimpleEncoder) is not ported and raises ValueError
    Linear-GELU MLPs  upp_layers.mlp2 (HF.linear / HF.mlp_gelu); the global maxima: upp_layers.max_over; FPS: utils.misc.fps
    query selection   the ranking MLP under no_grad (its only use is an integer order: its parameters get no gradient), then
                      HF.query_select: the num_query best of the [predicted ; FPS] candidates and, in training mode, the 64 jittered
                      denoising points behind them -- one launch each way instead of argsort + expand + gather + cat
    three Linears over a concatenation whose largest part is constant along the token axis, each split by columns (expand_add below):
                      PCTransformer.mlp_query[0] over [global ; coarse] (GELU), AdaPoinTr.reduce_map over [global ; q ; coarse] and
                      SimpleRebuildFCLayer.layer.fc1 over [max token ; token] (GELU).  The per-sample and per-token products run on
                      HF.linear, so no (B,M,1027+C) or (B,M,2C) tensor is built and the 3-column term needs no padded copy; the
                      broadcast add, the 3-column term and the GELU are torch element-wise operators -- NOT a fused kernel yet
                      (README "The AdaPoinTr completion model": what is left out)
    loss              get_loss: HF.knn_query + HF.gather_rows for the denoise target, ChamferDistanceL1, the 0.5 weight inside
The selection's fused path is taken for HIP f32 tensors of the served sizes while upp_layers.POOL_TRACE is unset; otherwise the same module
runs the torch formulation (upp_hip.torch_cpu.query_select), and a HIP tensor that was declined is recorded by HF.note_declined.

The name AdaPoinTr is NOT in the MODELS registry (README "The AdaPoinTr completion model"): build it with from_cfg(cfg), which puts the
class itself into cfg.NAME -- utils.registry.build_from_cfg accepts a class there.

Deliberate deviations: equal ranking scores are ordered by ascending index (the reference's torch.argsort(descending=True) leaves it
open); misc.jitter_points, which the reference calls and does not define, is this repository's (utils/misc.py)."""
from functools import partial

import torch
import torch.nn as nn

from extensions.chamfer_dist import ChamferDistanceL1
from upp_hip import functional as HF
from upp_hip import torch_cpu
from utils import misc
from . import upp_layers as L
from .PoinTr import Fold  # noqa: F401  (the reference's models/AdaPoinTr.py:693-735 is the same class)
from .Transformer import conv_bn_act_conv
from .build import build_model_from_cfg
from .dgcnn_group import DGCNN_Grouper
from .Transformer_utils import (Attention, CrossAttention, DeformableLocalAttention, DeformableLocalCrossAttention, DropPath, DynamicGraphAttention, LayerScale, Mlp,
                                denoise_knn, improvedDeformableLocalGraphAttention, knn_point)

SERVED_TOKENS = ('attn', 'graph')
UNPORTED_TOKENS = ('rw_deform', 'deform', 'deform_graph')


OPT_IN_TOKENS = ('deform', 'deform_graph')


def _opted_in(deformable):
    """the keyword `deformable` -> the frozenset of opted-in tokens: False / None nothing, True exactly {'deform'}, otherwise a collection
    of names drawn from OPT_IN_TOKENS (a config's `deformable: [deform, deform_graph]`)"""
    if deformable is None or isinstance(deformable, bool):
        return frozenset(('deform',)) if deformable else frozenset()
    if isinstance(deformable, str) or not hasattr(deformable, '__iter__'):
        raise ValueError("deformable: a bool or a collection of token names drawn from %s, got %r" % (OPT_IN_TOKENS, deformable))
    names = list(deformable)
    for t in names:
        if t not in OPT_IN_TOKENS:
            raise ValueError("deformable: unexpected token %r; the opt-in tokens are %s" % (t, ', '.join(OPT_IN_TOKENS)))
    return frozenset(names)


def _tokens(style, what, deformable=False, region_wise=False, cross=False):
    """'attn-graph' -> ['attn', 'graph']: one token, or one global and one local one (`graph`, an opted-in `deform` / `deform_graph`, or
    -- region_wise, outside the cross position -- `rw_deform`)"""
    tokens = style.split('-')
    opted = _opted_in(deformable)
    for t in tokens:
        if t in opted:
            continue
        if t == 'rw_deform' and region_wise:
            if cross:
                raise ValueError("%s %r: the block token 'rw_deform' is a self-attention only and cannot serve as a cross-attention" % (what, style))
            continue
        if t in UNPORTED_TOKENS:
            raise ValueError("%s %r: the block token %r (a deformable local attention) is not ported; served tokens: %s%s"
                             % (what, style, t, ', '.join(SERVED_TOKENS), " (and `deform` with deformable=True)" if t == 'deform' else ""))
        if t not in SERVED_TOKENS:
            raise ValueError("%s %r: unexpected block token %r" % (what, style, t))
    if len(tokens) > 2 or (len(tokens) == 2 and (tokens[0] == tokens[1] or 'attn' not in tokens)):
        raise ValueError("%s %r: one token, or one `attn` and one local token" % (what, style))
    return tokens


def _local(token, dim, num_heads, qkv_bias, attn_drop, drop, k, n_group):
    """the local branch of a token: `graph`, `deform`, `deform_graph` or `rw_deform` (reference models/AdaPoinTr.py:54-60,167-173,203-206)"""
    if token == 'rw_deform':
        return DeformableLocalAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop, k=k, n_group=n_group)
    if token == 'deform_graph':
        return improvedDeformableLocalGraphAttention(dim, k=k)
    if token == 'deform':
        return DeformableLocalCrossAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop, k=k,
                                             n_group=n_group)
    return DynamicGraphAttention(dim, k=k)


def _combine_style(style, what):
    if style not in ('concat', 'onebyone'):
        raise ValueError("%s: unexpected combine style %r for local and global attention" % (what, style))
    return style


def _scale_and_path(dim, init_values, drop_path):
    return (LayerScale(dim, init_values=init_values) if init_values else nn.Identity(),
            DropPath(drop_path) if drop_path > 0. else nn.Identity())


def _merged(feats, merge_map):
    """one branch as it is; two: the merge map over their concatenation"""
    if len(feats) == 1:
        return feats[0]
    return HF.linear(torch.cat(feats, dim=-1), merge_map.weight, merge_map.bias)


class SelfAttnBlockApi(nn.Module):
    """reference models/AdaPoinTr.py:15-108.  forward(x (B,N,dim), pos (B,N,3), idx=None (B,N,k) rows of x)."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., init_values=None, drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, block_style='attn-deform', combine_style='concat', k=10, n_group=2,
                 deformable=False, region_wise=False):
        super().__init__()
        self.combine_style = _combine_style(combine_style, 'SelfAttnBlockApi')
        self.norm1 = norm_layer(dim)
        self.ls1, self.drop_path1 = _scale_and_path(dim, init_values, drop_path)
        self.norm2 = norm_layer(dim)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        tokens = _tokens(block_style, 'block_style', deformable, region_wise)
        self.block_length = len(tokens)
        self.attn = None
        self.local_attn = None
        for token in tokens:
            if token == 'attn':
                self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
            else:
                self.local_attn = _local(token, dim, num_heads, qkv_bias, attn_drop, drop, k, n_group)
        if self.block_length == 2:
            if combine_style == 'concat':
                self.merge_map = nn.Linear(dim * 2, dim)
            else:
                self.norm3 = norm_layer(dim)
                self.ls3, self.drop_path3 = _scale_and_path(dim, init_values, drop_path)

    def forward(self, x, pos, idx=None):
        if self.block_length == 2 and self.combine_style == 'onebyone':
            x = x + self.drop_path1(self.ls1(self.attn(HF.layer_norm(x, self.norm1))))
            x = x + self.drop_path3(self.ls3(self.local_attn(HF.layer_norm(x, self.norm3), pos, idx=idx)))
        else:
            norm_x = HF.layer_norm(x, self.norm1)
            feats = []
            if self.attn is not None:
                feats.append(self.attn(norm_x))
            if self.local_attn is not None:
                feats.append(self.local_attn(norm_x, pos, idx=idx))
            x = x + self.drop_path1(self.ls1(_merged(feats, getattr(self, 'merge_map', None))))
        return x + self.drop_path2(self.ls2(self.mlp(HF.layer_norm(x, self.norm2))))


class CrossAttnBlockApi(nn.Module):
    """reference models/AdaPoinTr.py:110-309.  forward(q (B,N,dim), v (B,M,dim), q_pos (B,N,3), v_pos (B,M,3), self_attn_idx=None
    (B,N,k) rows of q, cross_attn_idx=None (B,N,k) rows of v, denoise_length=None).  With denoise_length = D the last D queries are
    denoising queries: the self-attention hides them from the first N - D (Attention(x, denoise_length=D)), and a graph self branch
    without a list searches as Transformer_utils.denoise_knn does."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., init_values=None, drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, self_attn_block_style='attn-deform', self_attn_combine_style='concat',
                 cross_attn_block_style='attn-deform', cross_attn_combine_style='concat', k=10, n_group=2, deformable=False,
                 region_wise=False):
        super().__init__()
        self.norm2 = norm_layer(dim)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()

        self.norm1 = norm_layer(dim)
        self.ls1, self.drop_path1 = _scale_and_path(dim, init_values, drop_path)
        self.self_attn_combine_style = _combine_style(self_attn_combine_style, 'CrossAttnBlockApi self-attention')
        tokens = _tokens(self_attn_block_style, 'self_attn_block_style', deformable, region_wise)
        self.self_attn_block_length = len(tokens)
        self.self_attn = None
        self.local_self_attn = None
        for token in tokens:
            if token == 'attn':
                self.self_attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
            else:
                self.local_self_attn = _local(token, dim, num_heads, qkv_bias, attn_drop, drop, k, n_group)
        if self.self_attn_block_length == 2:
            if self_attn_combine_style == 'concat':
                self.self_attn_merge_map = nn.Linear(dim * 2, dim)
            else:
                self.norm3 = norm_layer(dim)
                self.ls3, self.drop_path3 = _scale_and_path(dim, init_values, drop_path)

        self.norm_q = norm_layer(dim)
        self.norm_v = norm_layer(dim)
        self.ls4, self.drop_path4 = _scale_and_path(dim, init_values, drop_path)
        self.cross_attn_combine_style = _combine_style(cross_attn_combine_style, 'CrossAttnBlockApi cross-attention')
        tokens = _tokens(cross_attn_block_style, 'cross_attn_block_style', deformable, region_wise, cross=True)
        self.cross_attn_block_length = len(tokens)
        self.cross_attn = None
        self.local_cross_attn = None
        for token in tokens:
            if token == 'attn':
                self.cross_attn = CrossAttention(dim, dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
            else:
                self.local_cross_attn = _local(token, dim, num_heads, qkv_bias, attn_drop, drop, k, n_group)
        if self.cross_attn_block_length == 2:
            if cross_attn_combine_style == 'concat':
                self.cross_attn_merge_map = nn.Linear(dim * 2, dim)
            else:
                self.norm_q_2 = norm_layer(dim)
                self.norm_v_2 = norm_layer(dim)
                self.ls5, self.drop_path5 = _scale_and_path(dim, init_values, drop_path)

    def _local_self(self, x, q_pos, idx, denoise_length):
        if isinstance(self.local_self_attn, DeformableLocalAttention):
            if denoise_length is not None:
                raise ValueError("the block token 'rw_deform' (DeformableLocalAttention) has no denoising form, got denoise_length = %r"
                                 % (denoise_length,))
            return self.local_self_attn(x, q_pos, idx=idx)
        # with a list the branch is the same in both modes (the list already is the denoise list); without one it searches
        return self.local_self_attn(x, q_pos, idx=idx, denoise_length=denoise_length if idx is None else None)

    def forward(self, q, v, q_pos, v_pos, self_attn_idx=None, cross_attn_idx=None, denoise_length=None):
        if self.self_attn_block_length == 2 and self.self_attn_combine_style == 'onebyone':
            q = q + self.drop_path1(self.ls1(self.self_attn(HF.layer_norm(q, self.norm1), denoise_length=denoise_length)))
            q = q + self.drop_path3(self.ls3(self._local_self(HF.layer_norm(q, self.norm3), q_pos, self_attn_idx, denoise_length)))
        else:
            norm_q = HF.layer_norm(q, self.norm1)
            feats = []
            if self.self_attn is not None:
                feats.append(self.self_attn(norm_q, denoise_length=denoise_length))
            if self.local_self_attn is not None:
                feats.append(self._local_self(norm_q, q_pos, self_attn_idx, denoise_length))
            q = q + self.drop_path1(self.ls1(_merged(feats, getattr(self, 'self_attn_merge_map', None))))

        if self.cross_attn_block_length == 2 and self.cross_attn_combine_style == 'onebyone':
            q = q + self.drop_path4(self.ls4(self.cross_attn(HF.layer_norm(q, self.norm_q), HF.layer_norm(v, self.norm_v))))
            q = q + self.drop_path5(self.ls5(self.local_cross_attn(q=HF.layer_norm(q, self.norm_q_2), v=HF.layer_norm(v, self.norm_v_2),
                                                                   q_pos=q_pos, v_pos=v_pos, idx=cross_attn_idx)))
        else:
            norm_q, norm_v = HF.layer_norm(q, self.norm_q), HF.layer_norm(v, self.norm_v)
            feats = []
            if self.cross_attn is not None:
                feats.append(self.cross_attn(norm_q, norm_v))
            if self.local_cross_attn is not None:
                feats.append(self.local_cross_attn(q=norm_q, v=norm_v, q_pos=q_pos, v_pos=v_pos, idx=cross_attn_idx))
            q = q + self.drop_path4(self.ls4(_merged(feats, getattr(self, 'cross_attn_merge_map', None))))
        return q + self.drop_path2(self.ls2(self.mlp(HF.layer_norm(q, self.norm2))))


def _path_rate(drop_path_rate, i):
    return drop_path_rate[i] if isinstance(drop_path_rate, list) else drop_path_rate


class TransformerEncoder(nn.Module):
    """reference models/AdaPoinTr.py:312-334.  forward(x (B,N,dim), pos (B,N,3)); one neighbour list for every block."""

    def __init__(self, embed_dim=256, depth=4, num_heads=4, mlp_ratio=4., qkv_bias=False, init_values=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, block_style_list=['attn-deform'],
                 combine_style='concat', k=10, n_group=2, deformable=False, region_wise=False):
        super().__init__()
        self.k = k
        self.blocks = nn.ModuleList([SelfAttnBlockApi(
            dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, init_values=init_values, drop=drop_rate,
            attn_drop=attn_drop_rate, drop_path=_path_rate(drop_path_rate, i), act_layer=act_layer, norm_layer=norm_layer,
            block_style=block_style_list[i], combine_style=combine_style, k=k, n_group=n_group, deformable=deformable,
            region_wise=region_wise) for i in range(depth)])

    def lists(self, pos):
        """-> idx (B,N,k) | None when no block has a graph branch"""
        return knn_point(self.k, pos, pos) if any(b.local_attn is not None for b in self.blocks) else None

    def forward(self, x, pos):
        idx = self.lists(pos)
        for block in self.blocks:
            x = block(x, pos, idx=idx)
        return x


class TransformerDecoder(nn.Module):
    """reference models/AdaPoinTr.py:336-366.  forward(q (B,N,dim), v (B,M,dim), q_pos (B,N,3), v_pos (B,M,3), denoise_length=None)."""

    def __init__(self, embed_dim=256, depth=4, num_heads=4, mlp_ratio=4., qkv_bias=False, init_values=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm,
                 self_attn_block_style_list=['attn-deform'], self_attn_combine_style='concat',
                 cross_attn_block_style_list=['attn-deform'], cross_attn_combine_style='concat', k=10, n_group=2, deformable=False,
                 region_wise=False):
        super().__init__()
        self.k = k
        self.blocks = nn.ModuleList([CrossAttnBlockApi(
            dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, init_values=init_values, drop=drop_rate,
            attn_drop=attn_drop_rate, drop_path=_path_rate(drop_path_rate, i), act_layer=act_layer, norm_layer=norm_layer,
            self_attn_block_style=self_attn_block_style_list[i], self_attn_combine_style=self_attn_combine_style,
            cross_attn_block_style=cross_attn_block_style_list[i], cross_attn_combine_style=cross_attn_combine_style,
            k=k, n_group=n_group, deformable=deformable, region_wise=region_wise) for i in range(depth)])

    def lists(self, q_pos, v_pos, denoise_length=None):
        """-> (self_attn_idx (B,N,k) rows of q, cross_attn_idx (B,N,k) rows of v), each None when no block uses it.  With denoise_length
        the self list is Transformer_utils.denoise_knn's: the reference leaves it to every block, which recomputes the same list."""
        self_idx = cross_idx = None
        if any(b.local_self_attn is not None for b in self.blocks):
            self_idx = knn_point(self.k, q_pos, q_pos) if denoise_length is None else denoise_knn(self.k, q_pos, denoise_length)
        if any(b.local_cross_attn is not None for b in self.blocks):
            cross_idx = knn_point(self.k, v_pos, q_pos)
        return self_idx, cross_idx

    def forward(self, q, v, q_pos, v_pos, denoise_length=None):
        self_attn_idx, cross_attn_idx = self.lists(q_pos, v_pos, denoise_length)
        for block in self.blocks:
            q = block(q, v, q_pos, v_pos, self_attn_idx=self_attn_idx, cross_attn_idx=cross_attn_idx, denoise_length=denoise_length)
        return q


def _init_weights(m):
    if isinstance(m, nn.Linear):
        L.trunc_normal_(m.weight, std=.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)


class PointTransformerEncoder(nn.Module):
    """reference models/AdaPoinTr.py:368-430.  forward(x, pos) -> blocks(x, pos); `norm` is constructed (a state-dict key) and, as in the
    reference, not applied."""

    def __init__(self, embed_dim=256, depth=12, num_heads=4, mlp_ratio=4., qkv_bias=True, init_values=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., norm_layer=None, act_layer=None, block_style_list=['attn-deform'],
                 combine_style='concat', k=10, n_group=2, deformable=False, region_wise=False):
        super().__init__()
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        act_layer = act_layer or nn.GELU
        self.num_features = self.embed_dim = embed_dim
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        if len(block_style_list) != depth:
            raise ValueError("block_style_list names %d blocks for depth %d" % (len(block_style_list), depth))
        self.blocks = TransformerEncoder(
            embed_dim=embed_dim, num_heads=num_heads, depth=depth, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, init_values=init_values,
            drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=dpr, norm_layer=norm_layer, act_layer=act_layer,
            block_style_list=block_style_list, combine_style=combine_style, k=k, n_group=n_group, deformable=deformable,
            region_wise=region_wise)
        self.norm = norm_layer(embed_dim)
        self.apply(_init_weights)

    def forward(self, x, pos):
        return self.blocks(x, pos)


class PointTransformerDecoder(nn.Module):
    """reference models/AdaPoinTr.py:432-499.  forward(q, v, q_pos, v_pos, denoise_length=None)."""

    def __init__(self, embed_dim=256, depth=12, num_heads=4, mlp_ratio=4., qkv_bias=True, init_values=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., norm_layer=None, act_layer=None, self_attn_block_style_list=['attn-deform'],
                 self_attn_combine_style='concat', cross_attn_block_style_list=['attn-deform'], cross_attn_combine_style='concat',
                 k=10, n_group=2, deformable=False, region_wise=False):
        super().__init__()
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        act_layer = act_layer or nn.GELU
        self.num_features = self.embed_dim = embed_dim
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        if not len(self_attn_block_style_list) == len(cross_attn_block_style_list) == depth:
            raise ValueError("the style lists name %d and %d blocks for depth %d"
                             % (len(self_attn_block_style_list), len(cross_attn_block_style_list), depth))
        self.blocks = TransformerDecoder(
            embed_dim=embed_dim, num_heads=num_heads, depth=depth, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, init_values=init_values,
            drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=dpr, norm_layer=norm_layer, act_layer=act_layer,
            self_attn_block_style_list=self_attn_block_style_list, self_attn_combine_style=self_attn_combine_style,
            cross_attn_block_style_list=cross_attn_block_style_list, cross_attn_combine_style=cross_attn_combine_style,
            k=k, n_group=n_group, deformable=deformable, region_wise=region_wise)
        self.apply(_init_weights)

    def forward(self, q, v, q_pos, v_pos, denoise_length=None):
        return self.blocks(q, v, q_pos, v_pos, denoise_length=denoise_length)


def _entry_kwargs(config, deformable, region_wise=False):
    """a stack's config section as keywords; `deformable` (a bool or a list of token names) and `region_wise` (a bool) from the section
    itself or, failing that, from the model section"""
    kw = dict(config)
    kw['deformable'] = config.get('deformable', False) or deformable
    kw['region_wise'] = bool(config.get('region_wise', False) or region_wise)
    return kw


class PointTransformerEncoderEntry(PointTransformerEncoder):
    def __init__(self, config, deformable=False, region_wise=False, **kwargs):
        super().__init__(**_entry_kwargs(config, deformable, region_wise))


class PointTransformerDecoderEntry(PointTransformerDecoder):
    def __init__(self, config, deformable=False, region_wise=False, **kwargs):
        super().__init__(**_entry_kwargs(config, deformable, region_wise))


# ---------------------------------------------------------------------------------------------- PCTransformer and AdaPoinTr
DENOISE_PICKS = 64          # reference models/AdaPoinTr.py:863,866: the number of jittered input points appended as denoising queries


def expand_add(P, T=None, U=None, Wu=None, act=None):
    """P (R,O) a per-row product (bias included), T (R,S,O) a dense addend or None, U (R,S,J) with Wu (O,J) or None -> (R,S,O) =
    act(P[r] + T[r,s] + Wu U[r,s]), act None or 'gelu' (erf form): a Linear over [f repeated along s ; x ; u] with W = [Wf | Wx | Wu],
    P = Wf f + b, T = Wx x, without the concatenation.  Torch element-wise operators on any device and dtype; the J-column term is J
    broadcast products, not a matrix product (J = 3 here: no library GEMM of K = 3, no padded copy)."""
    if T is None and U is None:
        raise ValueError("expand_add: at least one of T (R, S, O) and U (R, S, J) must be given")
    if act not in (None, 'gelu'):
        raise ValueError("expand_add: act must be None or 'gelu'")
    z = P.unsqueeze(1)
    if T is not None:
        z = z + T
    if U is not None:
        for j in range(U.shape[-1]):
            z = z + U[..., j:j + 1] * Wu[:, j]
    return nn.functional.gelu(z) if act == 'gelu' else z


def query_select(score, cand, Q, extra, site):
    """HF.query_select where the kernel serves the operands, the torch formulation elsewhere -> out (B, Q + D, 3).  With POOL_TRACE set
    the order is recorded or replayed (upp_layers.trace_idx) like every other discrete choice."""
    if L.POOL_TRACE is None and HF.query_select_usable(score, cand, Q, extra):
        return HF.query_select(score, cand, Q, extra)[0]
    if score.is_cuda and L.POOL_TRACE is None:
        HF.note_declined("%s query_select score %s, Q = %d" % (site, tuple(score.shape), Q), "outside the served range")
    if L.POOL_TRACE is None:
        return torch_cpu.query_select(score, cand, Q, extra)[0]
    order = L.trace_idx(site + '.order', torch.argsort(score.detach(), dim=1, descending=True, stable=True)[:, :Q])
    out = torch.gather(cand, 1, order.unsqueeze(-1).expand(-1, -1, 3))
    return out if extra is None else torch.cat([out, extra], dim=1)


class SimpleRebuildFCLayer(nn.Module):
    """reference models/AdaPoinTr.py:737-758.  forward(rec_feature (B,M,C)) -> (B,M,step,3): the Mlp over [max token ; token], whose
    fc1 is W1[:, :C] g + b1 per sample, W1[:, C:] tok per token, added and activated by expand_add."""

    def __init__(self, input_dims, step, hidden_dim=512):
        super().__init__()
        self.input_dims = input_dims
        self.step = step
        self.layer = Mlp(self.input_dims, hidden_dim, step * 3)

    def forward(self, rec_feature):
        B, M, C = rec_feature.shape
        if 2 * C != self.input_dims:
            raise ValueError("SimpleRebuildFCLayer(%d) takes tokens of %d channels, got %d" % (self.input_dims, self.input_dims // 2, C))
        fc1, fc2 = self.layer.fc1, self.layer.fc2
        g_feature = L.max_over(rec_feature, 1, 'rebuild_fc.global')                  # (B,C)
        P = HF.linear(g_feature, fc1.weight[:, :C], fc1.bias)
        T = HF.linear(rec_feature.reshape(B * M, C), fc1.weight[:, C:]).view(B, M, -1)
        h = expand_add(P, T, act='gelu')
        return HF.linear(h.reshape(B * M, -1), fc2.weight, fc2.bias).view(B, M, self.step, 3)


class PCTransformer(nn.Module):
    """reference models/AdaPoinTr.py:761-889.  forward(xyz (B,N,3)) -> (q (B,M,C), coarse (B,M,3), denoise_length): M = num_query in eval
    mode, num_query + 64 with denoise_length = 64 in training mode (N >= 64)."""

    def __init__(self, config):
        super().__init__()
        encoder_config = config.encoder_config
        decoder_config = config.decoder_config
        self.center_num = getattr(config, 'center_num', [512, 128])
        self.encoder_type = config.encoder_type
        if self.encoder_type == 'pn':
            raise ValueError("encoder_type 'pn' (SimpleEncoder, the PointNet grouper) is not ported; served: 'graph'")
        if self.encoder_type != 'graph':
            raise ValueError("unexpected encoder_type %r" % (self.encoder_type,))
        in_chans = 3
        self.num_query = query_num = config.num_query
        global_feature_dim = config.global_feature_dim
        self.grouper = DGCNN_Grouper(k=16)
        self.pos_embed = nn.Sequential(nn.Linear(in_chans, 128), nn.GELU(), nn.Linear(128, encoder_config.embed_dim))
        self.input_proj = nn.Sequential(nn.Linear(self.grouper.num_features, 512), nn.GELU(), nn.Linear(512, encoder_config.embed_dim))
        deformable = config.get('deformable', False)                # opt-in: true (the token `deform`) or a list of token names
        region_wise = config.get('region_wise', False)              # opt-in: true serves the token `rw_deform` in the self positions
        self.encoder = PointTransformerEncoderEntry(encoder_config, deformable=deformable, region_wise=region_wise)
        self.increase_dim = nn.Sequential(nn.Linear(encoder_config.embed_dim, 1024), nn.GELU(), nn.Linear(1024, global_feature_dim))
        self.coarse_pred = nn.Sequential(nn.Linear(global_feature_dim, 1024), nn.GELU(), nn.Linear(1024, 3 * query_num))
        self.mlp_query = nn.Sequential(nn.Linear(global_feature_dim + 3, 1024), nn.GELU(), nn.Linear(1024, 1024), nn.GELU(),
                                       nn.Linear(1024, decoder_config.embed_dim))
        if decoder_config.embed_dim == encoder_config.embed_dim:
            self.mem_link = nn.Identity()
        else:
            self.mem_link = nn.Linear(encoder_config.embed_dim, decoder_config.embed_dim)
        self.decoder = PointTransformerDecoderEntry(decoder_config, deformable=deformable, region_wise=region_wise)
        self.query_ranking = nn.Sequential(nn.Linear(3, 256), nn.GELU(), nn.Linear(256, 256), nn.GELU(), nn.Linear(256, 1), nn.Sigmoid())
        self.apply(_init_weights)

    def ranking_scores(self, cand):
        """cand (B,M,3) -> (B,M): query_ranking's sigmoid scores, under no_grad -- they only order the candidates."""
        r = self.query_ranking
        B, M, _ = cand.shape
        with torch.no_grad():
            h = HF.linear(cand.detach().reshape(B * M, 3), r[0].weight, r[0].bias, act='gelu')
            h = HF.linear(h, r[2].weight, r[2].bias, act='gelu')
            # (one output: three zero rows make the output rows 16 bytes, which upp_linear_f32 serves; no gradient passes here)
            s = HF.linear(h, nn.functional.pad(r[4].weight, (0, 0, 0, 3)), nn.functional.pad(r[4].bias, (0, 3)))[:, 0]
            return torch.sigmoid(s).view(B, M)

    def query_features(self, global_feature, coarse):
        """mlp_query over [global feature repeated M times ; coarse point]: (B,G), (B,M,3) -> (B,M,C)."""
        l0 = self.mlp_query[0]
        B, M, _ = coarse.shape
        G = global_feature.shape[1]
        P = HF.linear(global_feature, l0.weight[:, :G], l0.bias)
        h = expand_add(P, None, coarse, l0.weight[:, G:], 'gelu')
        return L.mlp2(self.mlp_query[2:5], h.reshape(B * M, -1)).view(B, M, -1)

    def forward(self, xyz):
        B, N, _ = xyz.shape
        if self.training and N < DENOISE_PICKS:
            raise ValueError("training mode picks %d denoising points from the input, which has %d" % (DENOISE_PICKS, N))
        xyz = xyz.contiguous()
        coor, f = self.grouper(xyz, self.center_num)                                 # (B,n,3), (B,n,128)
        n = coor.shape[1]
        pe = L.mlp2(self.pos_embed, coor.reshape(B * n, 3)).view(B, n, -1)
        x = L.mlp2(self.input_proj, f.reshape(B * n, -1)).view(B, n, -1)
        x = self.encoder(x + pe, coor)
        g = L.mlp2(self.increase_dim, x.reshape(B * n, -1)).view(B, n, -1)
        global_feature = L.max_over(g, 1, 'pctransformer.global')                    # (B,G)
        coarse = L.mlp2(self.coarse_pred, global_feature).reshape(B, -1, 3)
        coarse_inp = misc.fps(xyz, self.num_query // 2)[0]
        cand = torch.cat([coarse, coarse_inp], dim=1)                                # (B, num_query + num_query / 2, 3)
        mem = x if isinstance(self.mem_link, nn.Identity) else HF.linear(x, self.mem_link.weight, self.mem_link.bias)
        extra, denoise_length = None, 0
        if self.training:
            extra = misc.jitter_points(misc.fps(xyz, DENOISE_PICKS)[0])
            denoise_length = DENOISE_PICKS
        coarse = query_select(self.ranking_scores(cand), cand, self.num_query, extra, 'pctransformer.query')
        q = self.query_features(global_feature, coarse)
        q = self.decoder(q=q, v=mem, q_pos=coarse, v_pos=coor, denoise_length=denoise_length or None)
        return q, coarse, denoise_length


class AdaPoinTr(nn.Module):
    """reference models/AdaPoinTr.py:893-997.  forward(xyz (B,N,3)): eval mode -> (coarse (B,M,3), rebuild (B, M factor, 3)); training mode
    -> (pred_coarse (B,M,3), denoised_coarse (B,64,3), denoised_fine (B, 64 factor, 3), pred_fine (B, M factor, 3)).  get_loss(ret, gt) ->
    (0.5 x the denoise Chamfer-L1, coarse + fine Chamfer-L1).  Not registered in MODELS: see from_cfg."""

    def __init__(self, config, **kwargs):
        super().__init__()
        self.trans_dim = config.decoder_config.embed_dim
        self.num_query = config.num_query
        self.num_points = getattr(config, 'num_points', None)
        self.decoder_type = config.decoder_type
        if self.decoder_type not in ('fold', 'fc'):
            raise ValueError("unexpected decoder_type %r" % (self.decoder_type,))
        self.fold_step = 8
        self.base_model = PCTransformer(config)
        if self.decoder_type == 'fold':
            self.factor = self.fold_step ** 2
            self.decode_head = Fold(self.trans_dim, step=self.fold_step, hidden_dim=256)
        elif self.num_points is not None:
            if self.num_points % self.num_query:
                raise ValueError("num_points %d is no multiple of num_query %d" % (self.num_points, self.num_query))
            self.factor = self.num_points // self.num_query
            self.decode_head = SimpleRebuildFCLayer(self.trans_dim * 2, step=self.factor)
        else:
            self.factor = self.fold_step ** 2
            self.decode_head = SimpleRebuildFCLayer(self.trans_dim * 2, step=self.fold_step ** 2)
        self.increase_dim = nn.Sequential(nn.Conv1d(self.trans_dim, 1024, 1), nn.BatchNorm1d(1024), nn.LeakyReLU(negative_slope=0.2),
                                          nn.Conv1d(1024, 1024, 1))
        self.reduce_map = nn.Linear(self.trans_dim + 1027, self.trans_dim)
        self.build_loss_func()

    def build_loss_func(self):
        self.loss_func = ChamferDistanceL1()

    def get_loss(self, ret, gt, epoch=1):
        pred_coarse, denoised_coarse, denoised_fine, pred_fine = ret
        if pred_fine.size(1) != gt.size(1):
            raise ValueError("pred_fine has %d points, the ground truth %d" % (pred_fine.size(1), gt.size(1)))
        # denoise loss: every denoised coarse point is to rebuild its `factor` nearest ground-truth points
        B, D, _ = denoised_coarse.shape
        _, idx = HF.knn_query(gt.contiguous(), denoised_coarse.detach().contiguous(), self.factor)
        idx = L.trace_idx('adapointr.denoise_target', idx.long())
        denoised_target = HF.gather_rows(gt.contiguous(), idx.reshape(B, D * self.factor))
        loss_denoised = self.loss_func(denoised_fine, denoised_target) * 0.5
        loss_recon = self.loss_func(pred_coarse, gt) + self.loss_func(pred_fine, gt)
        return loss_denoised, loss_recon

    def rebuild_feature(self, global_feature, q, coarse):
        """reduce_map over [global feature repeated M times ; q ; coarse]: (B,G), (B,M,C), (B,M,3) -> (B,M,C), never concatenated."""
        B, M, C = q.shape
        G = global_feature.shape[1]
        W = self.reduce_map.weight
        P = HF.linear(global_feature, W[:, :G], self.reduce_map.bias)
        T = HF.linear(q.reshape(B * M, C), W[:, G:G + C]).view(B, M, C)
        return expand_add(P, T, coarse, W[:, G + C:])

    def forward(self, xyz):
        if L.sync_bn_active(self.training):
            raise RuntimeError("AdaPoinTr does not support synchronised BatchNorm (upp_layers.enable_sync_bn)")
        q, coarse, denoise_length = self.base_model(xyz)                             # (B,M,C), (B,M,3)
        B, M, C = q.shape
        g = conv_bn_act_conv(self.increase_dim, q.reshape(B * M, C), self.training).view(B, M, -1)
        global_feature = L.max_over(g, 1, 'adapointr.global')                        # (B,1024)
        feature = self.rebuild_feature(global_feature, q, coarse)
        if self.decoder_type == 'fold':
            relative_xyz = self.decode_head.fold_rows(feature.reshape(B * M, C)).view(B, M, -1, 3)
        else:
            relative_xyz = self.decode_head(feature)                                 # (B,M,S,3)
        rebuild_points = relative_xyz + coarse.unsqueeze(-2)
        if self.training:
            R = M - denoise_length
            pred_fine = rebuild_points[:, :R].reshape(B, -1, 3).contiguous()
            pred_coarse = coarse[:, :R].contiguous()
            denoised_fine = rebuild_points[:, R:].reshape(B, -1, 3).contiguous()
            denoised_coarse = coarse[:, R:].contiguous()
            return pred_coarse, denoised_coarse, denoised_fine, pred_fine
        return coarse, rebuild_points.reshape(B, -1, 3).contiguous()


def from_cfg(cfg):
    """cfg: the model section of a config (cfgs/AdaPoinTr.yaml) -> AdaPoinTr(cfg).  The class itself goes into cfg.NAME --
    utils.registry.build_from_cfg takes a class there -- because the name is deliberately not in the MODELS registry."""
    cfg['NAME'] = AdaPoinTr
    return build_model_from_cfg(cfg)
