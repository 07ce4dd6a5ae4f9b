"""PointTransformer_seg -- the full fine-tuning part-segmentation baseline (reference models/Point_MAE_segment.py:275-456,
cfgs/finetune_shapenetpart_seg.yaml): group -> trainable patch embedding -> 12 plain blocks with taps behind blocks 3 / 7 / 11 -> one shared
trainable LayerNorm on the three taps, their concatenation (1152-d), its max and mean over the tokens -> 5-NN feature propagation to the
label points and the per-point head -> log-probabilities.  Every parameter trains; no prompts, no adapters, no prompter.

Same registry name, constructor contract, forward signature and state-dict keys as the reference (cls_token / cls_pos exist there and are
unused: kept for the keys).  On HIP f32 tensors the taps' LayerNorm, concat, max and mean are one node (HF.tap_pool: one launch forward, two
backward, parameter gradients included); the label branch and the head are Point_MAE_unify_seg's (SegTail).  Under upp_layers.POOL_TRACE,
on CPU tensors and for declined tensors the torch formulation upp_hip.torch_cpu.tap_pool runs, its arg-max through upp_layers.max_over.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from upp_hip import functional as HF
from upp_hip import torch_cpu
from .build import MODELS
from . import upp_layers as L
from .upp_layers import PointNetFeaturePropagation, PositionalEmbedding, trunc_normal_
from .Point_MAE_finetune import TAPS, build_backbone, load_backbone_ckpt, no_prompter
from .Point_MAE_unify_segment import SegTail, get_loss


class FeaturePropagation(PointNetFeaturePropagation):
    """PointNetFeaturePropagation whose xyz term -- a K = 3 product with a 1536-wide output, beyond the small-K kernel, and beside a
    5-neighbour interpolation that the fused interpolate-affine launch (k <= 4) does not serve -- runs on upp_linear_f32 with both
    operands zero-padded to its 32-wide contraction granule, as the trainable patch embedding's first layer does.  Same parameters."""

    def _add_first_columns(self, y, p1, w1):
        if not (y.is_cuda and y.dtype == torch.float32):
            return super()._add_first_columns(y, p1, w1)
        pad = (0, 32 - p1.shape[1])
        return y + HF.linear(F.pad(p1, pad), F.pad(w1, pad))


@MODELS.register_module()
class PointTransformer_seg(nn.Module, SegTail):
    def __init__(self, config, **kwargs):
        super().__init__()
        build_backbone(self, config)
        if self.trans_dim != 384 or self.depth <= max(TAPS):
            raise ValueError("PointTransformer_seg: the head is built for trans_dim 384 and taps behind blocks %s" % (TAPS,))
        self.label_conv = nn.Sequential(nn.Conv1d(16, 64, kernel_size=1, bias=True), nn.BatchNorm1d(64), nn.LeakyReLU(0.2),
                                        nn.Conv1d(64, 128, kernel_size=1, bias=True), nn.BatchNorm1d(128), nn.LeakyReLU(0.2))
        self.positional_embedding = PositionalEmbedding(12)
        self.propagation_0 = FeaturePropagation(in_channel=1152 + 3, mlp=[384 * 4, 1024], interpolate_neighbors=5)
        self.seg_head = nn.Sequential(
            nn.Conv1d(1024 + 128 + 384 * 6, 512, 1), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(0.5),
            nn.Conv1d(512, 256, 1), nn.BatchNorm1d(256), nn.ReLU(),
            nn.Conv1d(256, self.cls_dim, 1))
        trunc_normal_(self.cls_token, std=.02)
        trunc_normal_(self.cls_pos, std=.02)
        self.get_loss = get_loss()

    def load_model_from_ckpt(self, bert_ckpt_path, logger=None):
        return load_backbone_ckpt(self, bert_ckpt_path)

    def forward(self, pts, cls_label, label_points=None, completion_prompt=False, denoise=False, point_num=None, **kwargs):
        no_prompter("PointTransformer_seg", completion_prompt, denoise)
        L.begin_forward(pts.device, self.training)
        try:
            return self._forward(pts, cls_label, label_points)
        finally:
            L.end_forward()

    def _forward(self, pts, cls_label, label_points=None):
        neighborhood, center = self.group_divider(pts)
        tokens = self.encoder(neighborhood)
        f0, f1, f2 = self.blocks(tokens, L.mlp2(self.pos_embed, center), taps=TAPS)
        if L.POOL_TRACE is None:
            x, x_max, x_avg = HF.tap_pool(f0, f1, f2, self.norm)             # (B,G,1152), (B,1152), (B,1152)
        else:
            x, x_max, x_avg = torch_cpu.tap_pool(f0, f1, f2, self.norm, pool=lambda y: L.max_over(y, 1, 'seg.global_max'))
        global_feat = torch.cat((x_max, x_avg, self._label_feature(cls_label)), -1)      # (B,2432)
        target = label_points if label_points is not None else pts
        return self._head(self.propagation_0(target, center, target, x), global_feat)
