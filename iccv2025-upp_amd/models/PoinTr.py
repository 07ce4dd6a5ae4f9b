"""PoinTr, the point-cloud completion network of the reference (models/PoinTr.py), on the library's kernels.

forward(xyz (B,N,3)) -> (coarse (B, 2M, 3), rebuild (B, M S + N, 3)): the geometry-aware transformer (models/Transformer.PCTransformer)
predicts M query features and a coarse cloud, `reduce_map` mixes [global feature ; query feature ; coarse point] and the folding head
`Fold` grows S = step^2 points around every coarse point.  Class names and state-dict keys are the reference's.

Three layers multiply a concatenation in which one part is constant along an axis -- Fold.folding1[0] over [seed (2,S) ; feature repeated
S times], Fold.folding2[0] over [fd1 (3,S) ; feature repeated S times] and PCTransformer.mlp_query[0].  With W = [Wu | Wf] each is
(Wf f_r + b) + Wu u[r,s]: one product over the R rows (HF.linear) and HF.expand_act, which expands it, adds the J = 2 / 3 term,
normalises (BatchNorm1d, batch or running statistics) and activates without the (R, C + J, S) concatenation or the pre-norm tensor.  The
later layers of a folding run as (R S, .) row matrices through HF.linear and the BatchNorm-over-rows kernels; everything stays
channels-last, the only layout change is at Fold's boundary.  `reduce_map` is three products added together -- the global part per sample
and expanded, the query part and the 3-column coarse part per row -- so no (B M, 1027 + C) tensor is built.

Each fused path is taken for HIP f32 tensors of the served sizes while upp_layers.POOL_TRACE is unset; otherwise the same module runs the
torch formulation (upp_hip.torch_cpu.expand_act), and a HIP tensor that was declined is recorded by HF.note_declined."""
import torch
import torch.nn.functional as F
from torch import nn

from extensions.chamfer_dist import ChamferDistanceL1
from pointnet2_ops import pointnet2_utils
from upp_hip import functional as HF
from . import upp_layers as L
from .Transformer import PCTransformer, conv_bn_act_conv, conv_rows, expand
from .build import MODELS


def fps(pc, num):
    """pc (B,N,3) -> its `num` furthest-point samples (B,num,3), as reference models/PoinTr.py:10-13 (CPU tensors: the opt-in torch
    formulation behind HF.fps_gather, which pointnet2_utils does not serve)."""
    if not pc.is_cuda:
        return HF.fps_gather(pc.contiguous(), num)[0]
    fps_idx = pointnet2_utils.furthest_point_sample(pc, num)
    return pointnet2_utils.gather_operation(pc.transpose(1, 2).contiguous(), fps_idx).transpose(1, 2).contiguous()


class Fold(nn.Module):
    """reference models/PoinTr.py:16-58.  forward(x (R, in_channel)) -> (R, 3, step^2), the reference's layout; fold_rows(x) -> (R, step^2,
    3), what PoinTr uses.  folding_seed (2, step^2) is built on the CPU and moves with the module (failing that, with the input): not a
    buffer, no state-dict key."""

    def __init__(self, in_channel, step, hidden_dim=512):
        super().__init__()
        self.in_channel = in_channel
        self.step = step
        a = torch.linspace(-1., 1., steps=step, dtype=torch.float).view(1, step).expand(step, step).reshape(1, -1)
        b = torch.linspace(-1., 1., steps=step, dtype=torch.float).view(step, 1).expand(step, step).reshape(1, -1)
        self.folding_seed = torch.cat([a, b], dim=0)

        def folding(extra):
            return nn.Sequential(nn.Conv1d(in_channel + extra, hidden_dim, 1), nn.BatchNorm1d(hidden_dim), nn.ReLU(inplace=True),
                                 nn.Conv1d(hidden_dim, hidden_dim // 2, 1), nn.BatchNorm1d(hidden_dim // 2), nn.ReLU(inplace=True),
                                 nn.Conv1d(hidden_dim // 2, 3, 1))
        self.folding1 = folding(2)
        self.folding2 = folding(3)

    def _apply(self, fn, *args, **kwargs):
        """The seed follows the module (.cuda(), .to(), .double()) as a buffer would, without being one: a forward -- the first one
        inside a graph capture included -- then finds it on the module's device and copies nothing from the host."""
        super()._apply(fn, *args, **kwargs)
        self.folding_seed = fn(self.folding_seed)
        return self

    def seed_rows(self, like):
        """folding_seed as (step^2, 2) rows; moved with the input only where the input is not where the module is."""
        seed = self.folding_seed
        if seed.device != like.device or seed.dtype != like.dtype:
            seed = seed.to(device=like.device, dtype=like.dtype)
        return seed.t().contiguous()

    def _fold(self, seq, x, U):
        """One folding over [U ; x repeated]: x (R,C), U (S,J) shared or (R,S,J) per row -> (R,S,3)."""
        c0, bn0, _, c1, bn1, _, c2 = seq
        J = U.shape[-1]
        W = c0.weight.view(c0.out_channels, -1)
        P = HF.linear(x, W[:, J:], c0.bias)
        h = expand(P, U, W[:, :J], bn0, 0.0, 'fold')                                 # (R,S,H): conv, BatchNorm and ReLU of layer 1
        R, S, H = h.shape
        h = L._pointwise_bn_relu(h.view(R * S, H), c1, bn1, self.training)
        return conv_rows(h, c2).view(R, S, 3)

    def fold_rows(self, x):
        fd1 = self._fold(self.folding1, x, self.seed_rows(x))
        return self._fold(self.folding2, x, fd1)

    def forward(self, x):
        return self.fold_rows(x).transpose(1, 2)


@MODELS.register_module()
class PoinTr(nn.Module):
    """reference models/PoinTr.py:61-122.  config: trans_dim, knn_layer, num_pred, num_query."""

    def __init__(self, config, **kwargs):
        super().__init__()
        self.trans_dim = config.trans_dim
        self.knn_layer = config.knn_layer
        self.num_pred = config.num_pred
        self.num_query = config.num_query
        self.fold_step = int(pow(self.num_pred // self.num_query, 0.5) + 0.5)
        self.base_model = PCTransformer(in_chans=3, embed_dim=self.trans_dim, depth=[6, 8], drop_rate=0., num_query=self.num_query,
                                        knn_layer=self.knn_layer)
        self.foldingnet = Fold(self.trans_dim, step=self.fold_step, hidden_dim=256)
        self.increase_dim = nn.Sequential(nn.Conv1d(self.trans_dim, 1024, 1), nn.BatchNorm1d(1024), nn.LeakyReLU(negative_slope=0.2),
                                          nn.Conv1d(1024, 1024, 1))
        self.reduce_map = nn.Linear(self.trans_dim + 1027, self.trans_dim)
        self.build_loss_func()

    def build_loss_func(self):
        self.loss_func = ChamferDistanceL1()

    def get_loss(self, ret, gt, epoch=0):
        loss_coarse = self.loss_func(ret[0], gt)
        loss_fine = self.loss_func(ret[1], gt)
        return loss_coarse, loss_fine

    def rebuild_feature(self, global_feature, q, coarse):
        """reduce_map over [global feature repeated M times ; q ; coarse] as three products: (B,G), (B,M,C), (B,M,3) -> (B M, C)."""
        B, M, C = q.shape
        G = global_feature.shape[1]
        W = self.reduce_map.weight
        Pg = HF.linear(global_feature, W[:, :G], self.reduce_map.bias)
        Pq = HF.linear(q.reshape(B * M, C), W[:, G:G + C])
        # (K = 3 with gradients on both sides and 384 outputs: one zero column makes the rows 16 bytes, which upp_linear_f32 serves.
        #  Follow-up: the two padded copies per forward go away if this term rides in HF.expand_act -- J = 3 is what it serves -- or in
        #  a small-K kernel with both gradients.)
        Pc = HF.linear(F.pad(coarse.reshape(B * M, 3), (0, 1)), F.pad(W[:, G + C:], (0, 1)))
        return ((Pq + Pc).view(B, M, C) + Pg.unsqueeze(1)).reshape(B * M, C)

    def forward(self, xyz):
        if L.sync_bn_active(self.training):
            raise RuntimeError("PoinTr does not support synchronised BatchNorm (upp_layers.enable_sync_bn): the BatchNorm inside "
                               "HF.expand_act takes this rank's statistics only")
        q, coarse = self.base_model(xyz)                                            # (B,M,C), (B,M,3)
        B, M, C = q.shape
        g = conv_bn_act_conv(self.increase_dim, q.reshape(B * M, C), self.training).view(B, M, -1)
        global_feature = L.max_over(g, 1, 'pointr.global')                          # (B,1024)
        feature = self.rebuild_feature(global_feature, q, coarse)
        relative_xyz = self.foldingnet.fold_rows(feature)                           # (B M, S, 3)
        S = relative_xyz.shape[1]
        rebuild_points = (relative_xyz.view(B, M, S, 3) + coarse[:, :, None, :]).reshape(B, M * S, 3)
        inp_sparse = fps(xyz, self.num_query)
        coarse = torch.cat([coarse, inp_sparse], dim=1).contiguous()
        rebuild_points = torch.cat([rebuild_points, xyz], dim=1).contiguous()
        return coarse, rebuild_points
