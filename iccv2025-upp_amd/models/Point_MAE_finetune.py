"""PointTransformer -- the full fine-tuning classification baseline (reference models/Point_MAE_cp.py:468-596,
cfgs/finetune_modelnet_cls.yaml / finetune_scan_objonly_cls.yaml / finetune_shapenet55_cls.yaml): group -> trainable patch embedding ->
[cls | tokens] through `depth` plain blocks -> LayerNorm -> [cls | max over tokens] -> the three-layer head.  Every parameter trains: no
prompts, no adapters, no prompter.  It is the model a Point_MAE checkpoint of this library is fine-tuned with (load_model_from_ckpt maps
the `MAE_encoder.*` keys), and the yardstick the PEFT recipes are compared against.

Same registry name, constructor contract and state-dict keys as the reference.  On HIP f32 tensors the blocks run fused
(PlainBlock.forward_fused), the final LayerNorm + pooling is HF.cls_pool -- whose backward also produces the LayerNorm's parameter
gradients (upp_cls_pool_bwd_ln) -- and the head and the loss are the kernels Point_MAE_unify uses; under upp_layers.POOL_TRACE, on CPU
tensors and in other dtypes the same modules run as torch operators.
"""
import torch
import torch.nn as nn

from upp_hip import functional as HF
from .build import MODELS
from . import upp_layers as L
from .upp_layers import Encoder, Group, trunc_normal_
from .Point_MAE import _Stack, _mlp2
from .Point_MAE_unify import Point_MAE_unify

TAPS = (3, 7, 11)          # the block outputs PointTransformer_seg reads (reference models/Point_MAE_segment.py:264-272)


class TransformerEncoder(_Stack):
    """`pos` is added in front of every block (reference models/Point_MAE_cp.py:203-224); taps: block indices whose outputs are returned
    as a list instead of the last block's output (models/Point_MAE_segment.py:264-272)."""

    def forward(self, x, pos, taps=()):
        pos_i = HF.fan_out(pos, len(self.blocks))          # one launch sums the depth gradients of `pos`
        feats = []
        for i, block in enumerate(self.blocks):
            x = block.forward_fused(x, pos_i[i]) if block.fusable(x) else block(x + pos_i[i])
            if i in taps:
                feats.append(x)
        return feats if taps else x


def no_prompter(name, completion_prompt, denoise):
    """The evaluation loops pass the prompted models' switches to every model; a model without a prompter serves them switched off."""
    if completion_prompt or denoise:
        raise ValueError("%s has no prompter: completion_prompt and denoise must be False" % name)


def load_backbone_ckpt(model, path):
    """reference models/Point_MAE_cp.py:533-564: `base_model` of the checkpoint with `module.` stripped and the `MAE_encoder.` /
    `base_model.` prefixes removed, loaded non-strictly -> the (missing_keys, unexpected_keys) result of load_state_dict.  path None:
    train from scratch -- the reference's initialisation of every Linear / LayerNorm / Conv1d; -> None."""
    if path is None:
        model.apply(_init_weights)
        return None
    ckpt = torch.load(path, map_location='cpu')
    base = {k.replace("module.", ""): v for k, v in ckpt['base_model'].items()}
    for k in list(base.keys()):
        for prefix in ('MAE_encoder.', 'base_model.'):
            if k.startswith(prefix[:-1]):
                base[k[len(prefix):]] = base.pop(k)
                break
    return model.load_state_dict(base, strict=False)


def _init_weights(m):
    if isinstance(m, (nn.Linear, nn.Conv1d)):
        trunc_normal_(m.weight, std=.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)


def build_backbone(model, config):
    """The members the two fine-tuning models share (reference models/Point_MAE_cp.py:472-505, models/Point_MAE_segment.py:279-312)."""
    model.config = config
    model.trans_dim, model.depth, model.drop_path_rate = config.trans_dim, config.depth, config.drop_path_rate
    model.cls_dim, model.num_heads = config.cls_dim, config.num_heads
    model.group_size, model.num_group, model.encoder_dims = config.group_size, config.num_group, config.encoder_dims
    model.group_divider = Group(num_group=model.num_group, group_size=model.group_size)
    model.encoder = Encoder(encoder_channel=model.encoder_dims)
    model.cls_token = nn.Parameter(torch.zeros(1, 1, model.trans_dim))
    model.cls_pos = nn.Parameter(torch.randn(1, 1, model.trans_dim))
    model.pos_embed = _mlp2(3, 128, model.trans_dim)
    dpr = [x.item() for x in torch.linspace(0, model.drop_path_rate, model.depth)]
    model.blocks = TransformerEncoder(model.trans_dim, model.depth, model.num_heads, dpr)
    model.norm = nn.LayerNorm(model.trans_dim)


@MODELS.register_module()
class PointTransformer(nn.Module):
    def __init__(self, config, **kwargs):
        super().__init__()
        build_backbone(self, config)
        D = self.trans_dim
        self.cls_head_finetune = nn.Sequential(
            nn.Linear(D * 2, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(256, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(256, self.cls_dim))
        self.build_loss_func()
        trunc_normal_(self.cls_token, std=.02)
        trunc_normal_(self.cls_pos, std=.02)

    # the head and the loss are Point_MAE_unify's, kernels included: one body
    build_loss_func = Point_MAE_unify.build_loss_func
    get_loss_acc = Point_MAE_unify.get_loss_acc
    _cls_head = Point_MAE_unify._cls_head

    def load_model_from_ckpt(self, bert_ckpt_path, logger=None):
        return load_backbone_ckpt(self, bert_ckpt_path)

    def forward(self, pts, completion_prompt=False, denoise=False, point_num=None, **kwargs):
        no_prompter("PointTransformer", completion_prompt, denoise)
        L.begin_forward(pts.device, self.training)
        try:
            return self._forward(pts)
        finally:
            L.end_forward()

    def _forward(self, pts):
        neighborhood, center = self.group_divider(pts)
        tokens = self.encoder(neighborhood)
        B = tokens.shape[0]
        x = torch.cat((HF.expand_rows(self.cls_token, B, 1), tokens), dim=1)
        pos = torch.cat((HF.expand_rows(self.cls_pos, B, 1), L.mlp2(self.pos_embed, center)), dim=1)
        x = self.blocks(x, pos)
        if x.is_cuda and x.dtype == torch.float32 and x.shape[-1] <= 512 and x.shape[1] >= 2 and L.POOL_TRACE is None:
            feat = HF.cls_pool(x, self.norm)                   # LayerNorm + [cls | max over tokens], parameter gradients included
        else:
            if x.is_cuda and L.POOL_TRACE is None:
                HF.note_declined("cls_pool rows %s %s" % (tuple(x.shape), x.dtype), "outside the served range")
            x = self.norm(x)
            feat = torch.cat([x[:, 0], L.max_over(x[:, 1:], 1, 'cls.max')], dim=-1)
        return self._cls_head(feat)
