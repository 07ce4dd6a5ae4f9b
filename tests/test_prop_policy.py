"""Which blocks the fused prompt-propagation step serves is ONE predicate on metadata (HF.propagate_usable); a BatchNorm1d with
momentum=None (the cumulative moving average) is not among them: refused by propagate / prop_tail on the host, and taken by nn.BatchNorm1d
itself in a Block."""
import itertools

import numpy as np
import pytest
import torch
from torch import nn

from models import upp_layers
from upp_hip import functional as HF, ops


@pytest.mark.parametrize("affine,track,training,sync_bn,rows,momentum",
                         list(itertools.product((True, False), (True, False), (True, False), (False, True), (15360, 15361), (0.1, None))))
def test_propagate_usable_truth_table(affine, track, training, sync_bn, rows, momentum):
    bn = nn.BatchNorm1d(8, affine=affine, track_running_stats=track, momentum=momentum)
    # served: gamma / beta to apply, statistics to take (running ones in eval), a momentum that is a number wherever the running statistics
    # are updated (training with tracked statistics), a row count csr_build takes, statistics of this rank alone
    want = (affine and (track or training) and not (momentum is None and training and track) and rows <= ops.CSR_MAX_ROWS and not sync_bn)
    assert ops.CSR_MAX_ROWS == 15360
    assert HF.propagate_usable(rows, bn, training, sync_bn) is want


def test_momentum_none_is_refused_before_any_device_call():
    bn = nn.BatchNorm1d(384, momentum=None).train()
    ln = nn.LayerNorm(384)
    x = torch.zeros(2, 19, 384)                                    # host tensors: a device call would raise RuntimeError, not ValueError
    with pytest.raises(ValueError, match="momentum=None"):
        HF.propagate(x, bn, None, training=True)
    with pytest.raises(ValueError, match="momentum=None"):
        HF.prop_tail(x, x, None, None, 1.0, HF.ROW_STRIP_CLS, 2, bn, None, None, 1.0, True, ln, None, None, None, None)


@pytest.mark.gpu
def test_a_block_with_a_cumulative_average_batchnorm_equals_the_unfused_block():
    """One prompted block whose BatchNorm has momentum=None, in training mode: forward_fused declines the fused step, equals forward within
    the bounds of tests/test_gpu_block.py (test_block_fused_equals_unfused_with_gradients), and the running statistics move as
    nn.BatchNorm1d moves them (by 1 / num_batches_tracked: after the first batch they ARE the batch statistics)."""
    def close(a, b, rtol, atol_scale):
        a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
        np.testing.assert_allclose(a, b, rtol=rtol, atol=atol_scale * max(np.abs(b).max(), 1e-30))

    B, T, G2, P, D = 2, 16, 8, 2, 384
    torch.manual_seed(0)
    blk = upp_layers.Block(D, 6, qkv_bias=False, block_idx=0, downstream_adapter=True, downstream_depth=1, downstream_prompts=True,
                           downstream_prompts_depth=1, downstream_prompts_num=P).cuda().train()
    blk.downstream_adapter.dropout.p = 0.0                          # the two paths draw their masks from different generators
    blk.bnorm = nn.BatchNorm1d(D, momentum=None).cuda().train()
    with torch.no_grad():
        nn.init.normal_(blk.downstream_adapter.ln2.weight, std=0.02)   # (zero-initialised: the adapter would contribute nothing)
    for n, p in blk.named_parameters():
        p.requires_grad_(any(k in n for k in ("adapter", "prompts", "bnorm", "norm1")))
    g = torch.Generator(device="cuda").manual_seed(1)
    c1 = torch.randn(B, T, 3, device="cuda", generator=g)
    with torch.no_grad():
        _, c2, i1, i2 = upp_layers.Group(G2, 8)(c1, require_index=True, gather_idx=False)
    kw = dict(path="downstream", downstream_adapter=True, downstream_prompts=True, classification=True, center1=c1, center1_idx=i1,
              center2=c2, center2_idx=i2, gather_idx=False, prompt_propagation_after=True)
    x = torch.randn(B, 1 + T, D, device="cuda", generator=g)
    pos = torch.randn(B, 1 + T, D, device="cuda", generator=g)
    assert blk.fusable(x)
    assert not HF.propagate_usable(B * (1 + P + T), blk.bnorm, True, False)
    params = [p for p in blk.parameters() if p.requires_grad]
    outs = []
    for fused in (True, False):
        blk.bnorm.reset_running_stats()
        xi, pi = x.clone().requires_grad_(True), pos.clone().requires_grad_(True)
        out = blk.forward_fused(xi, pi, _prop_cache={}, **kw) if fused else blk(xi + pi, **kw)
        w = torch.linspace(-1, 1, out.numel(), device="cuda").view_as(out)
        grads = torch.autograd.grad((out * w).sum(), [xi, pi] + params, allow_unused=True)
        outs.append((out.detach(), grads, blk.bnorm.running_mean.clone(), blk.bnorm.running_var.clone(), int(blk.bnorm.num_batches_tracked)))
    close(outs[0][0], outs[1][0], rtol=1e-5, atol_scale=3e-6)
    for a, b in zip(outs[0][1], outs[1][1]):
        assert (a is None) == (b is None)
        if a is not None:
            close(a, b, rtol=5e-5, atol_scale=1e-5)
    assert outs[0][4] == outs[1][4] == 1
    close(outs[0][2], outs[1][2], rtol=1e-5, atol_scale=1e-6)
    close(outs[0][3], outs[1][3], rtol=1e-5, atol_scale=1e-6)
    assert np.abs(outs[0][2].cpu().numpy()).max() > 1e-3            # they moved: the batch mean replaced the initial zeros
