"""The configurable encoder / decoder blocks of AdaPoinTr and their stacks (reference models/AdaPoinTr.py:15-507) on the library's kernels.
Class names and state-dict keys are the reference's, so its checkpoints load with strict=True.

A block style is one or two tokens joined by '-'.  Served tokens: `attn` (global attention) and `graph` (DynamicGraphAttention), alone or
paired, combined by `concat` (both on one normalised input, merged by a Linear over the concatenation) or `onebyone` (one residual
branch each).  The tokens `rw_deform`, `deform` and `deform_graph` (the deformable local attentions) are not ported and raise ValueError
at construction.
    LayerNorm                      HF.layer_norm (the row kernel; eps from the module, 1e-6 in the stacks)
    self-attention                 Transformer_utils.Attention; with denoise_length the fused prefix-visibility kernel -- CrossAttnBlockApi
                                   passes denoise_length on and never builds the reference's (N, N) mask tensor
    cross-attention                upp_layers.CrossAttention (HF.cross_attention)
    graph branches                 Transformer_utils.DynamicGraphAttention (HF.edge_conv_max)
    merge maps                     HF.linear;  MLPs: upp_layers.Mlp (HF.mlp_gelu)
TransformerEncoder / TransformerDecoder compute every neighbour list once per forward -- the denoise list included, which the reference
recomputes inside every block; positions do not change between blocks, so the lists are the same -- and only the lists some block uses.

Not ported yet: PCTransformer and AdaPoinTr themselves (query ranking, SimpleRebuildFCLayer, the denoise loss); no model is registered."""
from functools import partial

import torch
import torch.nn as nn

from upp_hip import functional as HF
from . import upp_layers as L
from .Transformer_utils import Attention, CrossAttention, DropPath, DynamicGraphAttention, LayerScale, Mlp, denoise_knn, knn_point

SERVED_TOKENS = ('attn', 'graph')
UNPORTED_TOKENS = ('rw_deform', 'deform', 'deform_graph')


def _tokens(style, what):
    """'attn-graph' -> ['attn', 'graph']: one token, or one global and one local one"""
    tokens = style.split('-')
    for t in tokens:
        if t in UNPORTED_TOKENS:
            raise ValueError("%s %r: the block token %r (a deformable local attention) is not ported; served tokens: %s"
                             % (what, style, t, ', '.join(SERVED_TOKENS)))
        if t not in SERVED_TOKENS:
            raise ValueError("%s %r: unexpected block token %r" % (what, style, t))
    if len(tokens) > 2 or (len(tokens) == 2 and tokens[0] == tokens[1]):
        raise ValueError("%s %r: one token, or one `attn` and one `graph`" % (what, style))
    return tokens


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
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, block_style='attn-deform', combine_style='concat', k=10, n_group=2):
        super().__init__()
        self.combine_style = _combine_style(combine_style, 'SelfAttnBlockApi')
        self.norm1 = norm_layer(dim)
        self.ls1, self.drop_path1 = _scale_and_path(dim, init_values, drop_path)
        self.norm2 = norm_layer(dim)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        tokens = _tokens(block_style, 'block_style')
        self.block_length = len(tokens)
        self.attn = None
        self.local_attn = None
        for token in tokens:
            if token == 'attn':
                self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
            else:
                self.local_attn = DynamicGraphAttention(dim, k=k)
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
                 cross_attn_block_style='attn-deform', cross_attn_combine_style='concat', k=10, n_group=2):
        super().__init__()
        self.norm2 = norm_layer(dim)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()

        self.norm1 = norm_layer(dim)
        self.ls1, self.drop_path1 = _scale_and_path(dim, init_values, drop_path)
        self.self_attn_combine_style = _combine_style(self_attn_combine_style, 'CrossAttnBlockApi self-attention')
        tokens = _tokens(self_attn_block_style, 'self_attn_block_style')
        self.self_attn_block_length = len(tokens)
        self.self_attn = None
        self.local_self_attn = None
        for token in tokens:
            if token == 'attn':
                self.self_attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
            else:
                self.local_self_attn = DynamicGraphAttention(dim, k=k)
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
        tokens = _tokens(cross_attn_block_style, 'cross_attn_block_style')
        self.cross_attn_block_length = len(tokens)
        self.cross_attn = None
        self.local_cross_attn = None
        for token in tokens:
            if token == 'attn':
                self.cross_attn = CrossAttention(dim, dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
            else:
                self.local_cross_attn = DynamicGraphAttention(dim, k=k)
        if self.cross_attn_block_length == 2:
            if cross_attn_combine_style == 'concat':
                self.cross_attn_merge_map = nn.Linear(dim * 2, dim)
            else:
                self.norm_q_2 = norm_layer(dim)
                self.norm_v_2 = norm_layer(dim)
                self.ls5, self.drop_path5 = _scale_and_path(dim, init_values, drop_path)

    def _local_self(self, x, q_pos, idx, denoise_length):
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
                 combine_style='concat', k=10, n_group=2):
        super().__init__()
        self.k = k
        self.blocks = nn.ModuleList([SelfAttnBlockApi(
            dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, init_values=init_values, drop=drop_rate,
            attn_drop=attn_drop_rate, drop_path=_path_rate(drop_path_rate, i), act_layer=act_layer, norm_layer=norm_layer,
            block_style=block_style_list[i], combine_style=combine_style, k=k, n_group=n_group) for i in range(depth)])

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
                 cross_attn_block_style_list=['attn-deform'], cross_attn_combine_style='concat', k=10, n_group=2):
        super().__init__()
        self.k = k
        self.blocks = nn.ModuleList([CrossAttnBlockApi(
            dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, init_values=init_values, drop=drop_rate,
            attn_drop=attn_drop_rate, drop_path=_path_rate(drop_path_rate, i), act_layer=act_layer, norm_layer=norm_layer,
            self_attn_block_style=self_attn_block_style_list[i], self_attn_combine_style=self_attn_combine_style,
            cross_attn_block_style=cross_attn_block_style_list[i], cross_attn_combine_style=cross_attn_combine_style,
            k=k, n_group=n_group) for i in range(depth)])

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
                 combine_style='concat', k=10, n_group=2):
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
            block_style_list=block_style_list, combine_style=combine_style, k=k, n_group=n_group)
        self.norm = norm_layer(embed_dim)
        self.apply(_init_weights)

    def forward(self, x, pos):
        return self.blocks(x, pos)


class PointTransformerDecoder(nn.Module):
    """reference models/AdaPoinTr.py:432-499.  forward(q, v, q_pos, v_pos, denoise_length=None)."""

    def __init__(self, embed_dim=256, depth=12, num_heads=4, mlp_ratio=4., qkv_bias=True, init_values=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., norm_layer=None, act_layer=None, self_attn_block_style_list=['attn-deform'],
                 self_attn_combine_style='concat', cross_attn_block_style_list=['attn-deform'], cross_attn_combine_style='concat',
                 k=10, n_group=2):
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
            k=k, n_group=n_group)
        self.apply(_init_weights)

    def forward(self, q, v, q_pos, v_pos, denoise_length=None):
        return self.blocks(q, v, q_pos, v_pos, denoise_length=denoise_length)


class PointTransformerEncoderEntry(PointTransformerEncoder):
    def __init__(self, config, **kwargs):
        super().__init__(**dict(config))


class PointTransformerDecoderEntry(PointTransformerDecoder):
    def __init__(self, config, **kwargs):
        super().__init__(**dict(config))
