"""The PoinTr geometry-aware transformer (reference models/Transformer.py:222-424) on the library's kernels.

`Block` is the reference's encoder block (self-attention merged with a local branch over 8 neighbours); `PCTransformer` turns a partial
cloud into M query features and a coarse cloud of M points.  Class names and state-dict keys are the reference's, so its checkpoints
load with strict=True.  Features stay channels-last inside; the reference's Conv1d weights (O, K, 1) are used as (O, K) views.
    grouper                        models/dgcnn_group.DGCNN_Grouper, channels-last
    neighbour lists                HF.knn_query(keys, queries, 8), kept as per-sample (B, Nq, 8) lists -- what DecoderBlock takes
    pos_embed, input_proj,         HF.linear + BatchNorm over rows (upp_layers._bn_rows) + LeakyReLU + HF.linear; the max over the
    increase_dim, coarse_pred      proxies is upp_layers.max_over
    mlp_query[0]                   Conv1d(1024 + 3, 1024) over [global feature repeated M times ; coarse point] as
                                   HF.expand_act(W[:, :1024] g + b  (B rows),  coarse (B,M,3),  W[:, 1024:],  None, 0.2):
                                   no (B, M, 1027) tensor
Each fused path is taken for HIP f32 tensors of the served sizes while upp_layers.POOL_TRACE is unset; otherwise the same module runs
the torch formulation (upp_hip.torch_cpu), and a HIP tensor that was declined is recorded by HF.note_declined.

Synchronised BatchNorm (upp_layers.enable_sync_bn) is NOT supported by this model: the BatchNorm inside HF.expand_act (and its torch
formulation) takes this rank's statistics only, while the layers on upp_layers._bn_rows would take all ranks' -- PoinTr.forward raises when
the switch is on during training rather than run half synchronised.

Deliberate deviation (README "The PoinTr completion model"): the reference picks the 8 neighbours with topk(sorted=False) of
|a|^2 + |b|^2 - 2ab; here the set is the library's ascending (distance, index) on the direct squared distance.  The sets agree wherever
the 8th and 9th distances differ by more than rounding, and the order inside a set does not matter under the max."""
import torch
import torch.nn as nn

from upp_hip import functional as HF
from upp_hip import torch_cpu
from . import upp_layers as L
from .dgcnn_group import DGCNN_Grouper
from .upp_layers import Attention, CrossAttention, DecoderBlock, DropPath, Mlp  # noqa: F401  (the reference's names)


def expand(P, U, Wu, norm, slope, site):
    """HF.expand_act where the kernels serve the operands, the torch formulation elsewhere (CPU tensors, the test instrument, off the
    served range -- the last is recorded)."""
    if L.POOL_TRACE is None and HF.expand_usable(P, U, Wu, norm):
        return HF.expand_act(P, U, Wu, norm, slope)
    if P.is_cuda and L.POOL_TRACE is None:
        HF.note_declined("%s expand_act P %s, U %s" % (site, tuple(P.shape), tuple(U.shape)), "outside the served range")
    return torch_cpu.expand_act(P, U, Wu, norm, slope)


def conv_rows(x, conv, act=None):
    """A 1x1 Conv1d on a channels-last (..., K) tensor: HF.linear with the (O, K, 1) weight as an (O, K) view."""
    return HF.linear(x, conv.weight.view(conv.out_channels, -1), conv.bias, act=act)


def conv_bn_act_conv(seq, x, training):
    """Sequential(Conv1d, BatchNorm1d, LeakyReLU, Conv1d) on the rows of a channels-last (R, K) matrix."""
    c0, bn, act, c1 = seq[0], seq[1], seq[2], seq[3]
    if training and bn.track_running_stats:
        L.bump_counter(bn.num_batches_tracked)
    h = L._bn_rows(conv_rows(x, c0), bn, training)
    return conv_rows(L.gate('conv_bn_act_conv', h, act.negative_slope), c1)


def knn_lists(keys, queries, k=8):
    """(B, Nq, k) int64 rows of `keys` (B,Nk,3): the k nearest keys of every query, the library's ascending (distance, index)."""
    with torch.no_grad():
        return L.trace_idx('pctransformer.knn', HF.knn_query(keys.detach().contiguous(), queries.detach().contiguous(), k)[1].long())


class Block(nn.Module):
    """The geometry-aware encoder block, reference models/Transformer.py:222-258 (not upp_layers.Block, which is UPP's).
    forward(x (B,N,dim), knn_index (B,N,8) per-sample lists | None).  State-dict keys: norm1, attn, norm2, knn_map, merge_map, mlp."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.knn_map = nn.Sequential(nn.Linear(dim * 2, dim), nn.LeakyReLU(negative_slope=0.2))
        self.merge_map = nn.Linear(dim * 2, dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def forward(self, x, knn_index=None):
        norm_x = HF.layer_norm(x, self.norm1)
        x_1 = self.attn(norm_x)
        if knn_index is not None:
            knn_f = DecoderBlock.local_branch(self.knn_map, norm_x, norm_x, knn_index)
            x_1 = HF.linear(torch.cat([x_1, knn_f], dim=-1), self.merge_map.weight, self.merge_map.bias)
        x = x + self.drop_path(x_1)
        return x + self.drop_path(self.mlp(HF.layer_norm(x, self.norm2)))


class PCTransformer(nn.Module):
    """reference models/Transformer.py:262-424.  forward(inpc (B,N,3)) -> (q (B,M,embed_dim), coarse (B,M,3))."""

    def __init__(self, in_chans=3, embed_dim=768, depth=(6, 6), num_heads=6, mlp_ratio=2., qkv_bias=False, qk_scale=None, drop_rate=0.,
                 attn_drop_rate=0., num_query=224, knn_layer=-1):
        super().__init__()
        self.num_features = self.embed_dim = embed_dim
        self.knn_layer = knn_layer
        self.grouper = DGCNN_Grouper()
        self.pos_embed = nn.Sequential(nn.Conv1d(in_chans, 128, 1), nn.BatchNorm1d(128), nn.LeakyReLU(negative_slope=0.2),
                                       nn.Conv1d(128, embed_dim, 1))
        self.input_proj = nn.Sequential(nn.Conv1d(128, embed_dim, 1), nn.BatchNorm1d(embed_dim), nn.LeakyReLU(negative_slope=0.2),
                                        nn.Conv1d(embed_dim, embed_dim, 1))
        self.encoder = nn.ModuleList([Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                            drop=drop_rate, attn_drop=attn_drop_rate) for _ in range(depth[0])])
        self.increase_dim = nn.Sequential(nn.Conv1d(embed_dim, 1024, 1), nn.BatchNorm1d(1024), nn.LeakyReLU(negative_slope=0.2),
                                          nn.Conv1d(1024, 1024, 1))
        self.num_query = num_query
        self.coarse_pred = nn.Sequential(nn.Linear(1024, 1024), nn.ReLU(inplace=True), nn.Linear(1024, 3 * num_query))
        self.mlp_query = nn.Sequential(nn.Conv1d(1024 + 3, 1024, 1), nn.LeakyReLU(negative_slope=0.2), nn.Conv1d(1024, 1024, 1),
                                       nn.LeakyReLU(negative_slope=0.2), nn.Conv1d(1024, embed_dim, 1))
        self.decoder = nn.ModuleList([DecoderBlock(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                                   qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate) for _ in range(depth[1])])
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            L.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, nn.Conv1d):
            nn.init.xavier_normal_(m.weight.data, gain=1)
        elif isinstance(m, nn.BatchNorm1d):
            nn.init.constant_(m.weight.data, 1)
            nn.init.constant_(m.bias.data, 0)

    def query_features(self, global_feature, coarse):
        """mlp_query over [global feature repeated M times ; coarse point]: global_feature (B,1024), coarse (B,M,3) -> (B,M,embed_dim)."""
        c0, a0, c1, a1, c2 = self.mlp_query
        B, M, _ = coarse.shape
        G = global_feature.shape[1]
        W = c0.weight.view(c0.out_channels, G + 3)
        P = HF.linear(global_feature, W[:, :G], c0.bias)
        h = expand(P, coarse, W[:, G:], None, a0.negative_slope, 'mlp_query')
        h = L.gate('mlp_query', conv_rows(h.view(B * M, -1), c1), a1.negative_slope)
        return conv_rows(h, c2).view(B, M, -1)

    def forward(self, inpc):
        B = inpc.size(0)
        training = self.training
        coor, f = self.grouper(inpc.contiguous(), [512, 128])                       # (B,128,3), (B,128,128)
        N = coor.shape[1]
        knn_index = knn_lists(coor, coor)
        pos = conv_bn_act_conv(self.pos_embed, coor.reshape(B * N, 3), training).view(B, N, -1)
        x = conv_bn_act_conv(self.input_proj, f.reshape(B * N, -1), training).view(B, N, -1)
        for i, blk in enumerate(self.encoder):
            x = blk(x + pos, knn_index if i < self.knn_layer else None)
        g = conv_bn_act_conv(self.increase_dim, x.reshape(B * N, -1), training).view(B, N, -1)
        global_feature = L.max_over(g, 1, 'pctransformer.global')                   # (B,1024)
        c0, _, c1 = self.coarse_pred
        coarse = HF.linear(L._relu_linear(global_feature, c0), c1.weight, c1.bias).reshape(B, -1, 3)
        new_knn_index = knn_lists(coarse, coarse)
        cross_knn_index = knn_lists(coor, coarse)
        q = self.query_features(global_feature, coarse)
        for i, blk in enumerate(self.decoder):
            if i < self.knn_layer:
                q = blk(q, x, new_knn_index, cross_knn_index)
            else:
                q = blk(q, x)
        return q, coarse
