"""The kernels of csrc/norm_pool.hip -- upp_tap_pool_fwd / bwd and upp_cls_pool_bwd_ln -- and their autograd nodes (HF.tap_pool, HF.cls_pool
with a LayerNorm that trains), on the GPU.

Exact checks: x against HF.layer_norm per tap, mean / rstd against upp_rowln_fwd's, gmax against x.max(1), arg (lowest token among equal
maxima: every case holds duplicated token rows) and gmean (token-order sum, one division) against tests/_norm_pool_reference.py, g_x of
upp_cls_pool_bwd_ln against upp_cls_pool_bwd, two runs against each other, a captured replay against the eager run.

Gradient checks: every other gradient against the float64 torch formulation evaluated on the SAME arg-max, within max(5e-6, 3 x err_torch) of
the tensor's maximum, err_torch being the f32 torch formulation's own error against float64, computed here (the bound of
tests/test_gpu_pointr.py: two f32 evaluations that sum in different orders land inside one rounding envelope).
"""
import ctypes

import numpy as np
import pytest
import torch

import _norm_pool_reference as R
from upp_hip import _abi, ops, torch_cpu
from upp_hip import functional as HF

pytestmark = pytest.mark.gpu

TAP_SHAPES = [(1, 1, 4), (2, 5, 8), (3, 65, 132), (2, 128, 384), (1, 257, 512)]
CLS_SHAPES = [(1, 2, 4), (3, 17, 128), (2, 65, 384), (1, 161, 512)]
E_BADARG, E_RANGE = -1, -2


def make_norm(C, seed, dtype=torch.float32, device="cuda"):
    g = torch.Generator().manual_seed(1000 + seed)
    ln = torch.nn.LayerNorm(C, eps=1e-5)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(C, generator=g))          # both signs: a negative gamma turns the row's minimum into the maximum
        ln.bias.copy_(torch.randn(C, generator=g) * 0.5)
    return ln.to(device=device, dtype=dtype)


def make_taps(B, G, C, seed):
    """Three feature maps whose token rows repeat (row j = row j // 2 * 2 for a third of the tokens): equal rows give equal LayerNorm
    rows, so every column has ties between tokens."""
    g = torch.Generator().manual_seed(seed)
    taps = []
    for k in range(3):
        f = torch.randn(B, G, C, generator=g) * (1.0 + k) + 0.25 * k
        for j in range(1, G, 3):
            f[:, j] = f[:, j - 1]
        if G >= 5:
            f[:, G - 1] = f[:, 1]
        taps.append(f.cuda())
    return taps


def scaled(a, ref):
    return ((a.double().cpu() - ref.double().cpu()).abs().max() / max(ref.double().abs().max().item(), 1e-30)).item()


def judge(name, fused, plain, exact):
    err_f, err_t = scaled(fused, exact), scaled(plain, exact)
    lim = max(5e-6, 3 * err_t)
    print("%s: fused against f64 %.3g, torch formulation against f64 %.3g, bound %.3g" % (name, err_f, err_t, lim))
    assert torch.isfinite(fused).all(), name
    assert err_f <= lim, (name, err_f, err_t, lim)


# ============================================================================================== tap pool, forward
@pytest.mark.parametrize("B,G,C", TAP_SHAPES)
def test_tap_pool_forward_bits(B, G, C):
    f = make_taps(B, G, C, seed=B * 1000 + G)
    ln = make_norm(C, seed=G)
    x, gmax, arg, gmean, mean, rstd = ops.tap_pool_fwd(f[0], f[1], f[2], ln.weight.detach(), ln.bias.detach(), ln.eps)
    with torch.no_grad():
        want = torch.cat([HF.layer_norm(t, ln) for t in f], dim=-1)
    assert torch.equal(x, want)
    for k in range(3):
        _, _, m, r = ops.rowln_fwd(f[k], None, None, HF.ROW_IDENTITY, 0, None, None, 1.0, ln.weight.detach(), ln.bias.detach(), float(ln.eps), G,
                                   want_xo=False)
        assert torch.equal(mean[:, :, k].reshape(-1), m.reshape(-1)) and torch.equal(rstd[:, :, k].reshape(-1), r.reshape(-1))
    assert torch.equal(gmax, x.max(dim=1)[0])
    r_max, r_arg, r_mean = R.pool(x.cpu().numpy())
    assert np.array_equal(gmax.cpu().numpy(), r_max)
    assert np.array_equal(arg.cpu().numpy(), r_arg)
    if G >= 2:
        assert (x.gather(1, arg.long().unsqueeze(1)).squeeze(1) == gmax).all()
        dup = (x == gmax.unsqueeze(1)).sum(1)
        assert (dup > 1).any(), "the case holds no tie"
    assert np.array_equal(gmean.cpu().numpy(), r_mean)
    # HF.tap_pool is that launch
    hx, hmax, hmean = HF.tap_pool(f[0], f[1], f[2], ln)
    assert torch.equal(hx, x) and torch.equal(hmax, gmax) and torch.equal(hmean, gmean)


# ============================================================================================== tap pool, backward
def _torch_tap_grads(f, ln, arg, cot, dtype):
    """The torch formulation in `dtype` with the arg-max TAKEN from `arg`: outputs and gradients."""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in f]
    norm = make_norm(ln.weight.numel(), 0, dtype=dtype)
    with torch.no_grad():
        norm.weight.copy_(ln.weight.to(dtype)); norm.bias.copy_(ln.bias.to(dtype))
    x, gmax, gmean = torch_cpu.tap_pool(*leaves, norm, pool=lambda y: y.gather(1, arg.long().unsqueeze(1)).squeeze(1))
    loss = sum((o * c.to(dtype)).sum() for o, c in zip((x, gmax, gmean), cot))
    loss.backward()
    return dict(x=x.detach(), gmax=gmax.detach(), gmean=gmean.detach(), d_f0=leaves[0].grad, d_f1=leaves[1].grad, d_f2=leaves[2].grad,
                d_gamma=norm.weight.grad, d_beta=norm.bias.grad)


@pytest.mark.parametrize("B,G,C", TAP_SHAPES)
def test_tap_pool_backward_against_float64_on_the_same_arg(B, G, C):
    f = make_taps(B, G, C, seed=7 + G)
    ln = make_norm(C, seed=C)
    g = torch.Generator().manual_seed(99)
    cot = [torch.randn(s, generator=g).cuda() for s in ((B, G, 3 * C), (B, 3 * C), (B, 3 * C))]
    leaves = [t.clone().requires_grad_(True) for t in f]
    x, gmax, gmean = HF.tap_pool(*leaves, ln)
    assert type(x.grad_fn).__name__ == "_TapPoolBackward"
    sum((o * c).sum() for o, c in zip((x, gmax, gmean), cot)).backward()
    fused = dict(x=x.detach(), gmax=gmax.detach(), gmean=gmean.detach(), d_f0=leaves[0].grad, d_f1=leaves[1].grad, d_f2=leaves[2].grad,
                 d_gamma=ln.weight.grad, d_beta=ln.bias.grad)
    arg = ops.tap_pool_fwd(f[0], f[1], f[2], ln.weight.detach(), ln.bias.detach(), ln.eps)[2]
    plain = _torch_tap_grads(f, ln, arg, cot, torch.float32)
    exact = _torch_tap_grads(f, ln, arg, cot, torch.float64)
    for name in fused:
        judge("tap_pool (%d,%d,%d) %s" % (B, G, C, name), fused[name], plain[name], exact[name])
    # the C entry point's sums are the node's
    d = ops.tap_pool_bwd(cot[0], cot[1], cot[2], f[0], f[1], f[2], *ops.tap_pool_fwd(f[0], f[1], f[2], ln.weight.detach(), ln.bias.detach(), ln.eps)[4:6],
                         ln.weight.detach(), arg)
    for a, b in zip(d, (leaves[0].grad, leaves[1].grad, leaves[2].grad, ln.weight.grad, ln.bias.grad)):
        assert torch.equal(a, b)


def test_tap_pool_frozen_norm_and_partial_needs():
    """A frozen LayerNorm and a tap without a gradient get None; the others keep their bits."""
    B, G, C = 2, 5, 8
    f = make_taps(B, G, C, seed=3)
    ln = make_norm(C, seed=1)
    full = [t.clone().requires_grad_(True) for t in f]
    HF.tap_pool(*full, ln)[0].sum().backward()
    ln2 = make_norm(C, seed=1).requires_grad_(False)
    part = [f[0].clone().requires_grad_(True), f[1].clone(), f[2].clone().requires_grad_(True)]
    HF.tap_pool(*part, ln2)[0].sum().backward()
    assert part[1].grad is None and ln2.weight.grad is None and ln2.bias.grad is None
    assert torch.equal(part[0].grad, full[0].grad) and torch.equal(part[2].grad, full[2].grad)


# ============================================================================================== classification tail
def _torch_cls_grads(x, ln, amax, g_feat, dtype):
    norm = make_norm(ln.weight.numel(), 0, dtype=dtype)
    with torch.no_grad():
        norm.weight.copy_(ln.weight.to(dtype)); norm.bias.copy_(ln.bias.to(dtype))
    xi = x.detach().to(dtype).requires_grad_(True)
    h = norm(xi)
    feat = torch.cat([h[:, 0], h.gather(1, amax.long().unsqueeze(1)).squeeze(1)], dim=-1)
    (feat * g_feat.to(dtype)).sum().backward()
    return dict(g_x=xi.grad, g_gamma=norm.weight.grad, g_beta=norm.bias.grad)


@pytest.mark.parametrize("B,L,D", CLS_SHAPES)
def test_cls_pool_bwd_ln(B, L, D):
    g = torch.Generator().manual_seed(B * 100 + L)
    x = (torch.randn(B, L, D, generator=g) * 2.0 + 0.5).cuda()
    if L >= 4:
        x[:, 3] = x[:, 1]                                      # ties between token rows
    g_feat = torch.randn(B, 2 * D, generator=g).cuda()
    ln = make_norm(D, seed=L)
    gamma, beta = ln.weight.detach(), ln.bias.detach()
    feat, amax, mean, rstd = ops.cls_pool_fwd(x, gamma, beta, ln.eps)
    want_gx = ops.cls_pool_bwd(g_feat, x, mean, rstd, gamma, amax)
    g_x, g_gamma, g_beta = ops.cls_pool_bwd_ln(g_feat, x, mean, rstd, gamma, amax)
    assert torch.equal(g_x, want_gx)
    plain = _torch_cls_grads(x, ln, amax, g_feat, torch.float32)
    exact = _torch_cls_grads(x, ln, amax, g_feat, torch.float64)
    judge("cls_pool_bwd_ln (%d,%d,%d) g_gamma" % (B, L, D), g_gamma, plain["g_gamma"], exact["g_gamma"])
    judge("cls_pool_bwd_ln (%d,%d,%d) g_beta" % (B, L, D), g_beta, plain["g_beta"], exact["g_beta"])
    # the restatement's order, evaluated in float64 from the SAVED statistics: the kernel's two sums themselves
    r_gg, r_gb = R.cls_param_grads(x.cpu().numpy(), mean.cpu().numpy(), rstd.cpu().numpy(), amax.cpu().numpy(), g_feat.cpu().numpy())
    assert scaled(g_gamma, torch.from_numpy(r_gg)) <= 5e-6 and scaled(g_beta, torch.from_numpy(r_gb)) <= 5e-6
    # the autograd node: trainable parameters take the new backward, frozen ones keep the node and the bits they had
    xi = x.clone().requires_grad_(True)
    f1 = HF.cls_pool(xi, ln)
    assert type(f1.grad_fn).__name__ == "_ClsPoolLNBackward" and torch.equal(f1, feat)
    (f1 * g_feat).sum().backward()
    assert torch.equal(xi.grad, want_gx) and torch.equal(ln.weight.grad, g_gamma) and torch.equal(ln.bias.grad, g_beta)
    frozen = make_norm(D, seed=L).requires_grad_(False)
    xj = x.clone().requires_grad_(True)
    f2 = HF.cls_pool(xj, frozen)
    assert type(f2.grad_fn).__name__ == "_ClsPoolBackward" and torch.equal(f2, feat)
    (f2 * g_feat).sum().backward()
    assert torch.equal(xj.grad, want_gx) and frozen.weight.grad is None


# ============================================================================================== edges
def test_constant_row_has_rstd_of_eps_and_finite_gradients():
    B, G, C = 2, 5, 8
    f = make_taps(B, G, C, seed=5)
    f[1][1, 2] = 0.5                                           # a constant token row: mean 0.5 exactly, variance 0
    ln = make_norm(C, seed=2)
    leaves = [t.clone().requires_grad_(True) for t in f]
    x, gmax, arg, gmean, mean, rstd = ops.tap_pool_fwd(f[0], f[1], f[2], ln.weight.detach(), ln.bias.detach(), ln.eps)
    assert mean[1, 2, 1].item() == 0.5
    assert rstd[1, 2, 1].item() == (np.float32(1.0) / np.sqrt(np.float32(0.0) + np.float32(ln.eps))).item()
    assert torch.equal(x[1, 2, C:2 * C], ln.bias.detach())
    out = HF.tap_pool(*leaves, ln)
    (out[0].sum() + out[1].sum() + out[2].sum()).backward()
    for t in leaves + [ln.weight, ln.bias]:
        assert torch.isfinite(t.grad).all()


def test_nan_stays_in_its_row_and_column():
    B, G, C = 2, 9, 8
    f = make_taps(B, G, C, seed=6)
    f[1][1, 4, 3] = float("nan")
    f[1][1, 6, 3] = float("nan")                               # a later NaN row: the FIRST one is the column's maximum
    ln = make_norm(C, seed=3)
    x, gmax, arg, gmean, mean, rstd = ops.tap_pool_fwd(f[0], f[1], f[2], ln.weight.detach(), ln.bias.detach(), ln.eps)
    bad = torch.zeros_like(x, dtype=torch.bool)
    bad[1, 4, C:2 * C] = True
    bad[1, 6, C:2 * C] = True
    assert torch.equal(torch.isnan(x), bad)                    # the LayerNorm row of that tap, nothing else
    badp = torch.zeros_like(gmax, dtype=torch.bool)
    badp[1, C:2 * C] = True
    assert torch.equal(torch.isnan(gmax), badp) and torch.equal(torch.isnan(gmean), badp)
    assert (arg[1, C:2 * C] == 4).all()
    r_max, r_arg, r_mean = R.pool(x.cpu().numpy())
    assert np.array_equal(arg.cpu().numpy(), r_arg) and np.array_equal(gmax.cpu().numpy(), r_max, equal_nan=True)
    assert np.array_equal(gmean.cpu().numpy(), r_mean, equal_nan=True)


def _fwd_bwd(f, ln, cot):
    o = ops.tap_pool_fwd(f[0], f[1], f[2], ln.weight.detach(), ln.bias.detach(), ln.eps)
    d = ops.tap_pool_bwd(cot[0], cot[1], cot[2], f[0], f[1], f[2], o[4], o[5], ln.weight.detach(), o[2])
    return list(o) + list(d)


def test_two_runs_and_a_captured_replay_are_bit_identical():
    B, G, C = 3, 65, 132
    f = make_taps(B, G, C, seed=8)
    ln = make_norm(C, seed=4)
    g = torch.Generator().manual_seed(5)
    cot = [torch.randn(s, generator=g).cuda() for s in ((B, G, 3 * C), (B, 3 * C), (B, 3 * C))]
    first, second = _fwd_bwd(f, ln, cot), _fwd_bwd(f, ln, cot)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fwd_bwd(f, ln, cot)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _fwd_bwd(f, ln, cot)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, captured):
        assert torch.equal(a, b)


def test_sizes_outside_the_served_range_are_refused():
    lib = _abi.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = _abi.ptr
    G_MAX = 2048                                               # include/upp_hip.h UPP_ATTN_MAX_L
    for B, G, C in ((1, G_MAX + 1, 4), (1, 2, 516)):
        f = torch.zeros(B, G, C, device="cuda")
        ga = torch.ones(C, device="cuda")
        x = torch.zeros(B, G, 3 * C, device="cuda")
        pooled = torch.zeros(B, 3 * C, device="cuda")
        arg = torch.zeros(B, 3 * C, dtype=torch.int32, device="cuda")
        stat = torch.zeros(B, G, 3, device="cuda")
        assert lib.upp_tap_pool_part_floats(B, G, C) == 0
        assert lib.upp_tap_pool_fwd(p(f), p(f), p(f), p(ga), p(ga), 1e-5, p(x), p(pooled), p(arg), p(pooled), p(stat), p(stat), B, G, C, st) == E_RANGE
        assert lib.upp_tap_pool_bwd(p(x), p(pooled), p(pooled), p(f), p(f), p(f), p(stat), p(stat), p(ga), p(arg), p(x), p(f), p(f), p(f), p(ga), p(ga),
                                    B, G, C, st) == E_RANGE
        with pytest.raises(RuntimeError, match="range"):
            ops.tap_pool_fwd(f, f, f, ga, ga, 1e-5)
        with pytest.raises(RuntimeError, match="range"):
            ops.tap_pool_bwd(x, pooled, pooled, f, f, f, stat, stat, ga, arg)
        assert not HF.tap_pool_usable(f, f, f, torch.nn.LayerNorm(C).cuda())
    assert lib.upp_tap_pool_fwd(p(f), p(f), p(f), p(ga), p(ga), 1e-5, p(x), p(pooled), p(arg), p(pooled), p(stat), p(stat), 1, 2, 6, st) == E_RANGE
    assert lib.upp_tap_pool_fwd(p(f), p(f), p(f), p(ga), p(ga), 1e-5, p(x), p(pooled), p(arg), p(pooled), p(stat), p(stat), 0, 2, 8, st) == E_BADARG
    assert lib.upp_cls_pool_bwd_ln(p(pooled), p(f), p(stat), p(stat), p(ga), p(arg), p(f), p(ga), p(ga), 1, 2, 516, st) == E_RANGE
    assert lib.upp_cls_pool_bwd_ln(p(pooled), p(f), p(stat), p(stat), p(ga), p(arg), p(f), p(ga), p(ga), 1, 1, 512, st) == E_BADARG
    # a declined HIP tensor takes the torch formulation and is recorded
    HF._declined.clear()
    f = torch.randn(1, 2, 6, device="cuda")
    ln = torch.nn.LayerNorm(6).cuda()
    x, gmax, gmean = HF.tap_pool(f, f, f, ln)
    assert torch.allclose(x, torch.cat([ln(f)] * 3, -1)) and any("tap_pool" in k[0] for k in HF._declined)
    HF._declined.clear()
