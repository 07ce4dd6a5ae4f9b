"""DGCNN_Grouper of the PoinTr family (reference models/dgcnn_group.py:43-144 and models/AdaPoinTr.py:510-623) on the library's kernels.

Four edge-convolution layers (8 -> 32 -> 64 -> 64 -> 128 channels) with two FPS down-samplings between them.  The state dict is the
reference's (14 keys: input_trans.{weight,bias}, layer1..4.0.weight, layer1..4.1.{weight,bias}), so its checkpoints load as they are.

Inside, features stay channels-last; the only layout changes are the transposes at entry and exit.  A layer is
    neighbours  upp_knn (HF.knn_query: ascending (distance, index) on the direct squared distance)
    conv        W [f_j - f_i ; f_i] = W1 f_j + (W2 - W1) f_i: two per-point products through HF.linear (Nk and Nq rows, not Nq x k)
    the rest    HF.edge_conv_max: gather, GroupNorm, LeakyReLU and the max over the neighbours without a (B, Nq, k, O) tensor
and a down-sampling is upp_fps with the fused centre gather plus HF.gather_rows for the features.  The fused path is taken for HIP f32
tensors of the served sizes while upp_layers.POOL_TRACE is unset; otherwise the torch formulation (upp_hip.torch_cpu.edge_conv_max)
runs on the same neighbour lists, and an out-of-range size on a HIP tensor is recorded by HF.note_declined.

Deliberate deviation (README "The DGCNN grouper"): the reference picks neighbours with topk(sorted=False) of |a|^2 + |b|^2 - 2ab, whose
order among near-equal distances is undefined; here the set is the library's.  The sets agree wherever the k-th and (k+1)-th distances
differ by more than rounding, and the order inside a set does not matter under the max."""
import torch
import torch.nn as nn

from upp_hip import functional as HF
from upp_hip import torch_cpu
from . import upp_layers as L


class DGCNN_Grouper(nn.Module):
    CHANNELS = (8, 32, 64, 64, 128)

    def __init__(self, k=16):
        super().__init__()
        self.k = int(k)
        c = self.CHANNELS
        self.input_trans = nn.Conv1d(3, c[0], 1)
        for i in range(1, 5):
            setattr(self, "layer%d" % i, nn.Sequential(nn.Conv2d(2 * c[i - 1], c[i], kernel_size=1, bias=False), nn.GroupNorm(4, c[i]),
                                                       nn.LeakyReLU(negative_slope=0.2)))
        self.num_features = c[4]

    def edge_layer(self, layer, coor_q, f_q, coor_k, f_k):
        """coor_* (B,N*,3), f_* (B,N*,C) -> (B,Nq,O): max over the k nearest keys of every query of lrelu(GroupNorm(conv([f_j - f_i ; f_i])))."""
        conv, gn, act = layer[0], layer[1], layer[2]
        C = f_k.shape[-1]
        W = conv.weight.view(conv.out_channels, 2 * C)
        Wk, Wq = W[:, :C].contiguous(), W[:, C:] - W[:, :C]
        _, idx = HF.knn_query(coor_k, coor_q, self.k)
        A, Bq = HF.linear(f_k, Wk), HF.linear(f_q, Wq)
        if L.POOL_TRACE is None and HF.edge_conv_usable(A, Bq, idx, gn):
            return HF.edge_conv_max(A, Bq, idx, gn, act.negative_slope)
        if A.is_cuda and L.POOL_TRACE is None:
            HF.note_declined("edge_conv_max %s, k = %d" % (tuple(A.shape), idx.shape[2]), "outside the served range")
        return torch_cpu.edge_conv_max(A, Bq, idx, (gn.num_groups, gn.weight, gn.bias, gn.eps), act.negative_slope)

    @staticmethod
    def fps_downsample(coor, f, n):
        """coor (B,N,3), f (B,N,C) -> the n furthest-point samples' (coor, f)."""
        coor_q, idx = HF.fps_gather(coor, n)
        return coor_q, HF.gather_rows(f, idx.long())

    def forward(self, x, num=None):
        """forward(x): x (B,3,N) -> (coor (B,3,128), f (B,128,128)), FPS to 512 and then to 128 (models/dgcnn_group.py).
        forward(x, [n1, n2]): x (B,N,3) -> (coor (B,n2,3), f (B,n2,128)) (models/AdaPoinTr.py)."""
        channels_first = num is None
        n1, n2 = (512, 128) if channels_first else (int(num[0]), int(num[1]))
        coor = (x.transpose(1, 2) if channels_first else x).contiguous()
        f = HF.linear(coor, self.input_trans.weight.view(self.input_trans.out_channels, 3), self.input_trans.bias)
        f = self.edge_layer(self.layer1, coor, f, coor, f)
        coor_q, f_q = self.fps_downsample(coor, f, n1)
        f = self.edge_layer(self.layer2, coor_q, f_q, coor, f)
        coor = coor_q
        f = self.edge_layer(self.layer3, coor, f, coor, f)
        coor_q, f_q = self.fps_downsample(coor, f, n2)
        f = self.edge_layer(self.layer4, coor_q, f_q, coor, f)
        coor = coor_q
        if channels_first:
            return coor.transpose(1, 2).contiguous(), f.transpose(1, 2).contiguous()
        return coor, f
