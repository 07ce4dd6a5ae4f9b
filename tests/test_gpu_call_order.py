"""Training steps that do not alternate one forward with one backward: two training-mode forwards before the first backward
(`loss = model(a) + model(b)`, gradient accumulation), backwards in either order, a counter reset between a forward and its backward,
and a retained graph run twice.  Every stochastic site must hand its backward the mask its forward drew.

Op level: the fused `BatchNorm1d, ReLU, Dropout(p)` of the segmentation head (upp_bn_rows_drop_fwd / _bwd, whose mask is a hash of the
layer's num_batches_tracked and is not stored) and the three sites that take their uniforms as a tensor (bn_relu_drop, adapter, rowln's
drop path), each gradient against a float64 torch reference built from the mask that forward's own output shows.  Model level: for every
training recipe, fwd A + bwd A + fwd B + bwd B accumulates the gradient that fwd A + fwd B + one backward produces."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from models import upp_layers
from upp_hip import functional as HF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

ORDERS = ["ab_ab", "ab_ba", "ab_sum", "reset", "retain"]


def close(a, b, rtol, atol_scale):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol_scale * max(np.abs(b).max(), 1e-30))


def _interleave(order, fwd, bwd, between=None):
    """Runs forwards / backwards in `order`; fwd(k) -> forward k's output, bwd(outs, ks, retain) -> {k: gradients of forward k}.
    -> ({k: gradients}, outs).  "retain" also checks that the second backward of a retained graph repeats the first bit for bit."""
    if order == "retain":
        outs = [fwd(0)]
        g1 = bwd(outs, [0], True)[0]
        g2 = bwd(outs, [0], False)[0]
        for a, b in zip(g1, g2):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        return {0: g1}, outs
    if order == "reset":
        outs = [fwd(0)]
        between()
        return bwd(outs, [0], False), outs
    outs = [fwd(0), fwd(1)]
    if order == "ab_sum":
        return bwd(outs, [0, 1], False), outs
    ks = [0, 1] if order == "ab_ab" else [1, 0]
    got = {}
    for k in ks:
        got.update(bwd(outs, [k], False))
    return got, outs


# ------------------------------------------------------------------------------------------------ the fused BatchNorm + ReLU + Dropout
def _bn_case(R, C):
    torch.manual_seed(R + C)
    scale, shift = torch.linspace(0.5, 2.0, C, device='cuda'), torch.linspace(-1.0, 1.0, C, device='cuda')
    xs = [torch.randn(R, C, device='cuda') * scale + shift, torch.randn(R, C, device='cuda') * scale.flip(0) - 0.5 * shift]
    gs = [torch.randn(R, C, device='cuda'), torch.randn(R, C, device='cuda') * 1.5]
    bn = torch.nn.BatchNorm1d(C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(0.5, 1.5, C)); bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
    return xs, gs, bn


def _bn_forward(bn, drop, x, pending):
    """One training forward of the layer as a model forward runs it: bump the counter (queued to the end of the forward when pending)."""
    if pending:
        upp_layers.begin_forward(x.device, True)
    try:
        upp_layers.bump_counter(bn.num_batches_tracked)
        y = upp_layers._bn_rows(x, bn, True, relu=True, drop=drop)
    finally:
        if pending:
            upp_layers.end_forward()
    assert type(y.grad_fn).__name__ == '_BnRowsTrainBackward'
    return y


def _bn_reference(x0, y, bn, p, g):
    """float64 gradients (x, gamma, beta) of dropout(relu(bn(x))) with the mask read off the kernel's output y and the ReLU gate the kernel's
    own relu(bn(x)) > 0; checks y against that mask first."""
    bn_ref = torch.nn.BatchNorm1d(x0.shape[1]).cuda().train()
    with torch.no_grad():
        bn_ref.weight.copy_(bn.weight); bn_ref.bias.copy_(bn.bias)
        plain = upp_layers._bn_rows(x0, bn_ref, True, relu=True)          # relu(bn(x)) on the same kernels, no dropout
    pos = plain > 0
    kept = y.detach() != 0
    assert not (kept & ~pos).any()
    assert torch.equal(y.detach()[kept], (plain * (1.0 / (1.0 - p)))[kept])
    rate = kept[pos].float().mean().item()
    assert abs(rate - (1.0 - p)) < 4.0 * (p * (1 - p) / pos.sum().item()) ** 0.5 + 1e-3, rate
    x64 = x0.double().requires_grad_(True)
    w64 = bn.weight.detach().double().requires_grad_(True)
    b64 = bn.bias.detach().double().requires_grad_(True)
    y_lin = F.batch_norm(x64, None, None, w64, b64, True, 0.1, bn.eps)
    factor = kept.double() / (1.0 - p)                                     # (kept lies inside the gate)
    return torch.autograd.grad((y_lin * factor * g.double()).sum(), [x64, w64, b64]), kept


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("R,C,p", [(65536, 512, 0.5), (8192, 256, 0.2), (8190, 128, 0.3), (1000, 300, 0.5), (4096, 40, 0.7)])
def test_bn_relu_dropout_keeps_its_mask_across_call_orders(R, C, p, pending, order):
    """upp_bn_rows_drop_fwd / _bwd: forward A's backward uses forward A's mask whatever ran in between -- another forward of the same layer
    (which moves num_batches_tracked, the value the mask is hashed from), a counter reset, or nothing (a retained graph run twice)."""
    xs0, gs, bn = _bn_case(R, C)
    drop = torch.nn.Dropout(p).train()
    xs = [x.clone().requires_grad_(True) for x in xs0]
    params = [bn.weight, bn.bias]

    def bwd(outs, ks, retain):
        loss = sum((outs[k] * gs[k]).sum() for k in ks)
        grads = torch.autograd.grad(loss, [xs[k] for k in ks] + params, retain_graph=retain)
        if len(ks) == 1:
            return {ks[0]: grads}
        return {"sum": grads}

    got, outs = _interleave(order, lambda k: _bn_forward(bn, drop, xs[k], pending), bwd, between=bn.reset_running_stats)
    refs, masks = {}, {}
    for k in range(len(outs)):
        refs[k], masks[k] = _bn_reference(xs0[k], outs[k], bn, p, gs[k])
    if len(outs) == 2:
        differ = (masks[0] != masks[1]).float().mean().item()             # two forwards, two masks
        assert differ > 0.5 * p * (1 - p), differ
    if "sum" in got:
        g_xa, g_xb, g_gamma, g_beta = got["sum"]
        close(g_xa, refs[0][0], rtol=5e-5, atol_scale=1e-5)
        close(g_xb, refs[1][0], rtol=5e-5, atol_scale=1e-5)
        close(g_gamma, refs[0][1] + refs[1][1], rtol=2e-5, atol_scale=2e-5)
        close(g_beta, refs[0][2] + refs[1][2], rtol=2e-5, atol_scale=2e-5)
        return
    for k, (g_x, g_gamma, g_beta) in got.items():
        close(g_x, refs[k][0], rtol=5e-5, atol_scale=1e-5)
        close(g_gamma, refs[k][1], rtol=2e-5, atol_scale=2e-5)
        close(g_beta, refs[k][2], rtol=2e-5, atol_scale=2e-5)


@pytest.mark.parametrize("R,C,p", [(65536, 512, 0.5), (8190, 128, 0.3), (4096, 40, 0.7)])
def test_ranks_draw_different_dropout_masks(R, C, p, monkeypatch):
    """The layer salts the fused dropout with upp_layers._drop_salt, which mixes in the process-group rank: rank 0 draws the masks of a
    single-process run (salt = C), rank 1 at the same counter disagrees with it on 2p(1-p) of the gated elements, as two independent
    masks do."""
    import torch.distributed as dist
    xs0, _, bn = _bn_case(R, C)
    drop = torch.nn.Dropout(p).train()
    kept = []                                                                # no process group, rank 0, rank 1
    for rank in (None, 0, 1):
        if rank is not None:
            monkeypatch.setattr(dist, "is_initialized", lambda: True)
            monkeypatch.setattr(dist, "get_rank", lambda r=rank: r)
            monkeypatch.setattr(dist, "get_world_size", lambda: 2)
        try:
            with torch.no_grad():
                bn.num_batches_tracked.zero_()
            kept.append(_bn_forward(bn, drop, xs0[0].clone().requires_grad_(True), False).detach() != 0)
        finally:
            monkeypatch.undo()
    assert torch.equal(kept[0], kept[1])
    with torch.no_grad():
        bn.num_batches_tracked.fill_(1)
        y = HF.bn_rows_train(xs0[0].clone().requires_grad_(True), bn, True, drop_p=p, salt=C)
    assert torch.equal(y.detach() != 0, kept[0])                          # rank 0: the salt of one process, the channel count
    bn_ref = torch.nn.BatchNorm1d(C).cuda().train()
    with torch.no_grad():
        bn_ref.weight.copy_(bn.weight); bn_ref.bias.copy_(bn.bias)
        pos = upp_layers._bn_rows(xs0[0], bn_ref, True, relu=True) > 0
    differ = (kept[2] != kept[0])[pos].float().mean().item()
    assert abs(differ - 2 * p * (1 - p)) < 0.02, differ


# ------------------------------------------------------------------------------------- sites that take their uniforms as a tensor
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("R,C", [(32, 256), (4, 256), (7, 40), (130, 100)])
def test_bn_relu_drop_with_saved_uniforms_across_call_orders(R, C, order):
    torch.manual_seed(R * C)
    p = 0.5
    zs0 = [torch.randn(R, C, device='cuda') * 1.5 + 0.3, torch.randn(R, C, device='cuda') - 0.2]
    us = [torch.rand(R, C, device='cuda'), torch.rand(R, C, device='cuda')]
    gs = [torch.linspace(-1, 1, R * C, device='cuda').view(R, C), torch.randn(R, C, device='cuda')]
    bn = torch.nn.BatchNorm1d(C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(0.5, 1.5, C)); bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
    zs = [z.clone().requires_grad_(True) for z in zs0]
    params = [bn.weight, bn.bias]

    def bwd(outs, ks, retain):
        grads = torch.autograd.grad(sum((outs[k] * gs[k]).sum() for k in ks), [zs[k] for k in ks] + params, retain_graph=retain)
        return {ks[0]: grads} if len(ks) == 1 else {"sum": grads}

    got, outs = _interleave(order, lambda k: HF.bn_relu_drop(zs[k], bn, us[k], p, True), bwd, between=bn.reset_running_stats)
    refs = []
    for k in range(len(outs)):
        with torch.no_grad():
            plain = HF.bn_relu_drop(zs0[k], bn, None, 0.0, True)          # the kernel's own ReLU gate
        gate = (plain > 0).double()
        mask = (us[k] >= p).double() / (1.0 - p)
        z64 = zs0[k].double().requires_grad_(True)
        w64, b64 = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
        a64 = F.batch_norm(z64, None, None, w64, b64, True, 0.1, bn.eps) * gate * mask
        close(outs[k], a64, rtol=1e-5, atol_scale=2e-6)
        refs.append(torch.autograd.grad((a64 * gs[k].double()).sum(), [z64, w64, b64]))
    if "sum" in got:
        g_za, g_zb, g_gamma, g_beta = got["sum"]
        expect = [(g_za, refs[0][0]), (g_zb, refs[1][0]), (g_gamma, refs[0][1] + refs[1][1]), (g_beta, refs[0][2] + refs[1][2])]
    else:
        expect = [(a, b) for k, gk in got.items() for a, b in zip(gk, refs[k])]
    for a, b in expect:
        close(a, b, rtol=3e-5, atol_scale=1e-5)


@pytest.mark.parametrize("order", [o for o in ORDERS if o != "reset"])
@pytest.mark.parametrize("R", [2400, 1120, 45])
def test_adapter_dropout_across_call_orders(R, order):
    torch.manual_seed(R)
    D, H, p, dev = 384, 32, 0.1, 'cuda'
    has = [torch.randn(R, D, device=dev, requires_grad=True) for _ in range(2)]
    xs = [torch.randn(R, D, device=dev, requires_grad=True) for _ in range(2)]
    W1 = (torch.randn(H, D, device=dev) / D ** 0.5).requires_grad_(True)
    b1 = (0.1 * torch.randn(H, device=dev)).requires_grad_(True)
    W2 = (torch.randn(D, H, device=dev) / H ** 0.5).requires_grad_(True)
    b2 = (0.1 * torch.randn(D, device=dev)).requires_grad_(True)
    params = [W1, b1, W2, b2]
    us = [torch.rand(R, H, device=dev) for _ in range(2)]
    ws = [torch.randn(R, D, device=dev) for _ in range(2)]

    def bwd(outs, ks, retain):
        grads = torch.autograd.grad(sum((outs[k] * ws[k]).sum() for k in ks), [t for k in ks for t in (has[k], xs[k])] + params,
                                    retain_graph=retain)
        return {ks[0]: grads} if len(ks) == 1 else {"sum": grads}

    got, outs = _interleave(order, lambda k: HF.adapter(has[k], xs[k], W1, b1, W2, b2, us[k], p, 0.7), bwd)
    P64 = [t.detach().double().requires_grad_(True) for t in params]
    refs = []
    for k in range(len(outs)):
        ha64, x64 = has[k].detach().double().requires_grad_(True), xs[k].detach().double().requires_grad_(True)
        mask = (us[k] >= p).double() / (1 - p)
        ref = x64 + 0.7 * F.linear(F.gelu(F.linear(ha64, P64[0], P64[1])) * mask, P64[2], P64[3])
        close(outs[k], ref, rtol=1e-5, atol_scale=2e-6)
        refs.append(torch.autograd.grad((ref * ws[k].double()).sum(), [ha64, x64] + P64))
    if "sum" in got:
        g = got["sum"]
        expect = list(zip(g[:4], refs[0][:2] + refs[1][:2])) + [(a, r0 + r1) for a, r0, r1 in zip(g[4:], refs[0][2:], refs[1][2:])]
    else:
        expect = [(a, b) for k, gk in got.items() for a, b in zip(gk, refs[k])]
    for a, b in expect:
        close(a, b, rtol=5e-5, atol_scale=1e-5)


@pytest.mark.parametrize("order", [o for o in ORDERS if o != "reset"])
@pytest.mark.parametrize("B,L,keep", [(4, 65, 0.7), (32, 75, 0.9), (3, 33, 0.5)])
def test_rowln_drop_path_across_call_orders(B, L, keep, order):
    torch.manual_seed(B * L)
    D, dev = 384, 'cuda'
    xs = [torch.randn(B, L, D, device=dev, requires_grad=True) for _ in range(2)]
    ys = [torch.randn(B, L, D, device=dev, requires_grad=True) for _ in range(2)]
    us = [torch.rand(B, device=dev) for _ in range(2)]
    gam = (1 + 0.1 * torch.randn(D, device=dev)).requires_grad_(True)
    bet = (0.1 * torch.randn(D, device=dev)).requires_grad_(True)
    w1s = [torch.randn(B, L, D, device=dev) for _ in range(2)]
    w2s = [torch.randn(B, L, D, device=dev) for _ in range(2)]
    params = [gam, bet]

    def fwd(k):
        return HF.rowln(xs[k], y=ys[k], u=us[k], keep=keep, gamma=gam, beta=bet)

    def bwd(outs, ks, retain):
        loss = sum((outs[k][0] * w1s[k]).sum() + (outs[k][1] * w2s[k]).sum() for k in ks)
        grads = torch.autograd.grad(loss, [t for k in ks for t in (xs[k], ys[k])] + params, retain_graph=retain)
        return {ks[0]: grads} if len(ks) == 1 else {"sum": grads}

    got, outs = _interleave(order, fwd, bwd)
    P64 = [t.detach().double().requires_grad_(True) for t in params]
    refs = []
    for k in range(len(outs)):
        x64, y64 = xs[k].detach().double().requires_grad_(True), ys[k].detach().double().requires_grad_(True)
        scale = ((keep + us[k].double()).floor() / keep).view(B, 1, 1)
        rxo = x64 + scale * y64
        rh = F.layer_norm(rxo, (D,), P64[0], P64[1], 1e-5)
        close(outs[k][0], rxo, rtol=1e-5, atol_scale=2e-6)
        close(outs[k][1], rh, rtol=1e-5, atol_scale=2e-6)
        refs.append(torch.autograd.grad((rxo * w1s[k].double()).sum() + (rh * w2s[k].double()).sum(), [x64, y64] + P64))
    if "sum" in got:
        g = got["sum"]
        expect = list(zip(g[:4], refs[0][:2] + refs[1][:2])) + [(a, r0 + r1) for a, r0, r1 in zip(g[4:], refs[0][2:], refs[1][2:])]
    else:
        expect = [(a, b) for k, gk in got.items() for a, b in zip(gk, refs[k])]
    for a, b in expect:
        close(a, b, rtol=2e-5, atol_scale=5e-6)


# ------------------------------------------------------------------------------------------------------------- every training recipe
def _recipe(kind, B):
    import bench
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tr = bench.Trainer(dev, B, False, use_graph=False) if kind == "cls" else bench.RecipeTrainer(kind, dev, B, use_graph=False)
    m = tr.model
    if kind == "cls":
        inputs = list(tr.batches[0])
        kw = tr.ts.kw

        def loss_of(ins):
            return m.get_loss_acc(m(ins[0], **kw), ins[1])[0]
    else:
        inputs = list(tr.ts.inputs)

        def loss_of(ins):
            return tr.ts.loss_fn(m, *ins)[0]
    return m, list(tr.ts.trainable), loss_of, inputs, [t.roll(1, 0) for t in inputs]


def _path(order, m, params, loss_of, a, b, start):
    """From the starting state (weights, buffers, both RNGs, an empty uniform bank): two forwards and their backwards in `order`."""
    m.load_state_dict(start["model"])
    with torch.no_grad():
        for k, v in m.named_buffers():                # (non-persistent ones too)
            v.copy_(start["buffers"][k])
    torch.set_rng_state(start["cpu"])
    torch.cuda.set_rng_state(start["cuda"])
    for q in params:
        q.grad = None
    with upp_layers.use_rng(upp_layers.UniformBank()):
        if order == "serial":                     # fwd A, bwd A, fwd B, bwd B
            loss_of(a).backward()
            loss_of(b).backward()
        else:
            la = loss_of(a)
            lb = loss_of(b)
            if order == "sum":                    # fwd A, fwd B, one backward
                (la + lb).backward()
            else:                                 # fwd A, fwd B, bwd B, bwd A
                lb.backward()
                la.backward()
    torch.cuda.synchronize()
    grads = [None if q.grad is None else q.grad.detach().clone() for q in params]
    bufs = {k: v.detach().clone() for k, v in m.named_buffers()}
    return grads, bufs


@pytest.mark.parametrize("kind", ["cls", "cls_aux", "stage2", "pretask", "pretrain", "seg"])
def test_two_forwards_before_a_backward_give_the_alternating_gradient(kind):
    """fwd A, bwd A, fwd B, bwd B (what the step driver does twice) and fwd A, fwd B, backward of lossA + lossB (or bwd B, bwd A) run
    the same forwards in the same order from the same state: the buffers they leave are the same bits, and the accumulated gradients
    differ by no more than the order in which a backward adds partial sums -- a backward that read state a later forward had moved
    (a dropout mask hashed from a counter, a saved buffer the next forward overwrote) would be off by O(1)."""
    m, params, loss_of, a, b = _recipe(kind, 4)
    start = {"model": {k: v.detach().clone() for k, v in m.state_dict().items()}, "buffers": {k: v.detach().clone() for k, v in m.named_buffers()},
             "cpu": torch.get_rng_state(),
             "cuda": torch.cuda.get_rng_state()}
    g1, buf1 = _path("serial", m, params, loss_of, a, b, start)
    assert any(g is not None for g in g1)
    for order in ("sum", "reverse"):
        g2, buf2 = _path(order, m, params, loss_of, a, b, start)
        assert buf1.keys() == buf2.keys()
        for k in buf1:
            assert torch.equal(buf1[k], buf2[k]), (kind, order, k)
        norms = [0.0 if g is None else float(g.double().norm()) for g in g1]
        total, biggest = float(np.sqrt(sum(n * n for n in norms))), max(norms)
        bad, bitwise = [], True
        for q, x, y, n in zip(params, g1, g2, norms):
            assert (x is None) == (y is None), (kind, order, tuple(q.shape))
            if x is None:
                continue
            bitwise = bitwise and torch.equal(x, y)
            err = float((x.double() - y.double()).norm())
            if not err <= 1e-6 * n + 1e-7 * biggest:
                bad.append((tuple(q.shape), err, n))
        print("%s %s: gradients bit-equal to the alternating path: %s (total norm %.3e)" % (kind, order, bitwise, total))
        assert not bad, (kind, order, bad[:8], len(bad))
