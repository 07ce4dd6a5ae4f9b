"""The broadcast-expand kernels (csrc/expand.hip, include/upp_hip.h "broadcast expand") on the GPU.

Without a norm the forward equals the numpy restatement (tests/_expand_reference.py) bit for bit.  With a norm the forward, mean and rstd
are within 1e-5 of each output's scale of a float64 evaluation, and every gradient meets close(rtol=2e-5, atol_scale=5e-6) -- the bounds
of tests/test_gpu_edge_conv.py -- against the float64 torch formulation with the activation's branch PINNED to the one the run under
test took (h > 0 <=> z > 0): an element whose z rounds across 0 may legitimately take the other branch, and the test checks that the
pinned branch differs from float64's own only where |z| is rounding-small.  Each case first holds the f32 torch formulation on the CPU
to the same bounds, so the bounds are a property of the inputs (O(1) variance per channel) and not of the kernel.  Then: the running
buffers, repeatability, capture into a graph, the memory a step allocates, and the refusals."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _expand_reference as XR
from conftest import ROOT
from upp_hip import functional as HF
from upp_hip import ops, torch_cpu

sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

pytestmark = pytest.mark.gpu

EPS = 1e-5
# (R, S, O, J, per-row U, norm, slope)
SPECIAL = (12, 10, 24, 3, True, "train-special", 0.2)
CASES = [(1, 1, 1, 1, False, "none", 0.0), (5, 9, 20, 2, False, "train", 0.0), (64, 16, 256, 2, False, "train", 0.0),
         (7, 64, 256, 3, True, "train", 0.0), (2, 224, 1024, 3, True, "none", 0.2), (2, 33, 1024, 3, True, "none", 0.2),
         (130, 4, 128, 4, True, "train", 0.2), (6, 16, 64, 3, True, "eval", 0.0), SPECIAL]
MODE = {"none": 0, "train": 1, "train-special": 1, "eval": 2}


def close(a, b, rtol=2e-5, atol_scale=5e-6):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol_scale * max(np.abs(b).max(), 1e-30))


def scaled_error(got, want):
    return ((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def inputs(case, seed=0):
    """CPU f32: P, U, Wu, gamma, beta, running_mean, running_var, g_h.  The special case: gamma holds a negative and a zero entry, and
    channel 5 is constant (a zero Wu row, a constant P column; 120 values of 0.75 sum exactly in f32): variance 0, xhat 0."""
    R, S, O, J, per_row, norm, slope = case
    g = torch.Generator().manual_seed(1000 * seed + R + 7 * S + 31 * O + J)
    P = torch.randn(R, O, generator=g) + 0.5
    U = torch.randn((R, S, J) if per_row else (S, J), generator=g)
    Wu = torch.randn(O, J, generator=g) / J ** 0.5
    gamma = 1 + 0.3 * torch.randn(O, generator=g)
    beta = 0.3 * torch.randn(O, generator=g)
    rm, rv = 0.5 + 0.1 * torch.randn(O, generator=g), 0.5 + 1.5 * torch.rand(O, generator=g)
    g_h = torch.randn(R, S, O, generator=g)
    if norm == "train-special":
        gamma[1], gamma[2] = -gamma[1].abs(), 0.0
        Wu[5], P[:, 5] = 0.0, 0.75
    return P, U, Wu, gamma, beta, rm, rv, g_h


def formulation(P, U, Wu, gamma, beta, rm, rv, norm, slope, mask=None):
    """The pinned formulation in the operands' own precision -> (h, mean, rstd, z); `mask` replaces z > 0."""
    y = P.unsqueeze(1) + torch.matmul(U, Wu.t())
    mean = rstd = None
    z = y
    if norm != "none":
        mean, var = (y.mean((0, 1)), y.var((0, 1), unbiased=False)) if norm != "eval" else (rm, rv)
        rstd = 1.0 / torch.sqrt(var + EPS)
        z = (y - mean) * rstd * gamma + beta
    return torch.where(z > 0 if mask is None else mask, z, z * slope), mean, rstd, z


def wrt_of(case, P, U, Wu, gamma, beta):
    return [P] + ([U] if case[4] else []) + [Wu] + ([gamma, beta] if case[5] != "none" else [])


@functools.lru_cache(maxsize=None)
def reference(case, which):
    """float64 on the CPU: (h, mean, rstd) free, and the gradients (g_P, [g_U,] g_Wu[, g_gamma, g_beta]) with the branch mask of the run
    `which` ("kernel" | "cpu32") pinned."""
    norm, slope = case[5], case[6]
    P, U, Wu, gamma, beta, rm, rv, g_h = (t.double() for t in inputs(case))
    with torch.no_grad():
        h, mean, rstd, z = formulation(P, U, Wu, gamma, beta, rm, rv, norm, slope)
    mask = (kernel_run(case)[0].cpu() if which == "kernel" else cpu32_run(case)[0]) > 0
    flipped = mask != (z > 0)
    assert flipped.float().mean().item() < 1e-3 and (not flipped.any() or z[flipped].abs().max().item() < 1e-5 * z.abs().max().item())
    leaves = [t.clone().requires_grad_() for t in (P, U, Wu, gamma, beta)]
    pinned = formulation(*leaves, rm, rv, norm, slope, mask)[0]
    return (h, mean, rstd) + tuple(torch.autograd.grad(pinned, wrt_of(case, *leaves), g_h))


def bn_of(case, gamma, beta, rm, rv, device):
    O, norm = case[2], case[5]
    if norm == "none":
        return None
    bn = torch.nn.BatchNorm1d(O, eps=EPS).to(device)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    return bn.train(norm != "eval")


@functools.lru_cache(maxsize=None)
def cpu32_run(case):
    """The library's torch formulation in f32 on the CPU: (h, bn after the call) + gradients."""
    P, U, Wu, gamma, beta, rm, rv, g_h = inputs(case)
    bn = bn_of(case, gamma, beta, rm, rv, "cpu")
    leaves = [t.clone().requires_grad_() for t in (P, U, Wu)]
    h = torch_cpu.expand_act(*leaves, bn, case[6])
    wrt = wrt_of(case, *leaves, *((bn.weight, bn.bias) if bn is not None else (None, None)))
    return (h.detach(), bn) + tuple(torch.autograd.grad(h, wrt, g_h))


@functools.lru_cache(maxsize=None)
def kernel_run(case):
    """One forward + backward through the library at the ops level (mean, var, rstd are outputs there)."""
    R, S, O, J, per_row, norm, slope = case
    P, U, Wu, gamma, beta, rm, rv, g_h = (t.cuda() for t in inputs(case))
    mode = MODE[norm]
    mean_in, rstd_in = (rm, torch.rsqrt(rv + EPS)) if mode == 2 else (None, None)
    h, mean, var, rstd = ops.expand_fwd(P, U, Wu, gamma, beta, mean_in, rstd_in, mode, EPS, slope)
    grads = ops.expand_bwd(g_h, P, U, Wu, gamma, beta, mean, rstd, mode, slope, want_gU=per_row)
    torch.cuda.synchronize()
    return (h, mean, var, rstd) + tuple(g for g in grads if g is not None)


@pytest.mark.parametrize("case", CASES)
def test_forward(case):
    norm, slope = case[5], case[6]
    P, U, Wu = (t.numpy() for t in inputs(case)[:3])
    h, mean, var, rstd = kernel_run(case)[:4]
    assert h.shape == case[:3] and h.dtype == torch.float32
    r_h, r_mean, r_rstd = reference(case, "kernel")[:3]
    c_h, c_bn = cpu32_run(case)[:2]
    print("%s cpu f32 formulation h: max error / scale = %.3g" % (case, scaled_error(c_h, r_h)))
    assert scaled_error(c_h, r_h) < 1e-5
    if norm == "none":
        assert mean is None and var is None and rstd is None
        assert np.array_equal(h.cpu().numpy().view(np.int32), XR.forward(P, U, Wu, slope).view(np.int32))        # bit for bit
        return
    for name, got, want in (("h", h, r_h), ("mean", mean, r_mean), ("rstd", rstd, r_rstd)):
        err = scaled_error(got, want)
        print("%s %s: max error / scale = %.3g" % (case, name, err))
        assert err < 1e-5, (name, err)
    if norm == "train-special":
        assert mean[5].item() == 0.75 and var[5].item() == 0.0                       # the constant channel: exact
        b5 = inputs(case)[4][5].item()
        assert torch.equal(h[:, :, 5].cpu(), torch.full(case[:2], b5 if b5 > 0 else np.float32(b5) * np.float32(slope)))


@pytest.mark.parametrize("case", CASES)
def test_gradients_against_the_pinned_formulation(case):
    names = ["g_P"] + (["g_U"] if case[4] else []) + ["g_Wu"] + (["g_gamma", "g_beta"] if case[5] != "none" else [])
    got, cpu = kernel_run(case)[4:], cpu32_run(case)[2:]
    assert len(got) == len(names) == len(cpu)
    for name, c, w in zip(names, cpu, reference(case, "cpu32")[3:]):
        print("%s cpu f32 formulation %s: max error / scale = %.3g" % (case, name, scaled_error(c, w)))
        close(c, w)
    for name, g, w in zip(names, got, reference(case, "kernel")[3:]):
        print("%s %s: max error / scale = %.3g" % (case, name, scaled_error(g, w)))
        assert g.shape == w.shape
        close(g, w)


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[6], CASES[7]])
@pytest.mark.parametrize("momentum", [0.1, None])
def test_node_and_running_buffers_equal_torchs(case, momentum):
    """HF.expand_act with a BatchNorm1d: the output and gradients of the ops-level run, and after one training call the running buffers
    and the counter of torch's own module fed the same y (within 1e-6); an eval call leaves them alone."""
    P, U, Wu, gamma, beta, rm, rv, g_h = inputs(case)
    bn, ref = bn_of(case, gamma, beta, rm, rv, "cuda"), bn_of(case, gamma, beta, rm, rv, "cpu")
    bn.momentum = ref.momentum = momentum
    if momentum is None:
        with torch.no_grad():
            bn.num_batches_tracked.fill_(3); ref.num_batches_tracked.fill_(3)
    leaves = [P.cuda().requires_grad_(), U.cuda().requires_grad_(case[4]), Wu.cuda().requires_grad_()]
    HF._declined.clear()
    h = HF.expand_act(*leaves, bn, case[6])
    grads = torch.autograd.grad(h, wrt_of(case, *leaves, bn.weight, bn.bias), g_h.cuda())
    assert not HF._declined, HF._declined
    want = kernel_run(case)
    assert torch.equal(h, want[0]) and all(torch.equal(a, b) for a, b in zip(grads, want[4:])) and len(grads) == len(want[4:])
    torch_cpu.expand_act(P, U, Wu, ref, case[6])
    assert bn.num_batches_tracked.item() == ref.num_batches_tracked.item() == (3 if momentum is None else 0) + (case[5] != "eval")
    for name in ("running_mean", "running_var"):
        a, b = getattr(bn, name).cpu(), getattr(ref, name)
        print("%s momentum %s %s: max difference = %.3g" % (case, momentum, name, (a - b).abs().max().item()))
        assert (a - b).abs().max().item() < 1e-6, name
        assert (case[5] == "eval") == torch.equal(b, rm if name == "running_mean" else rv)


@pytest.mark.parametrize("case", CASES)
def test_two_calls_give_equal_bits(case):
    first = kernel_run(case)
    kernel_run.cache_clear()
    again = kernel_run(case)
    assert len(first) == len(again)
    for i, (a, b) in enumerate(zip(first, again)):
        assert (a is None and b is None) or torch.equal(a, b), i


@pytest.mark.parametrize("case", [CASES[3], CASES[5]])
def test_forward_and_backward_replay_from_a_graph(case):
    from memset_census import memsets_of
    P0, U0, Wu0, gamma, beta, rm, rv, g0 = (t.cuda() for t in inputs(case))
    bn = bn_of(case, gamma, beta, rm, rv, "cuda")
    sP, sU, sW, sg = P0.clone().requires_grad_(), U0.clone().requires_grad_(), Wu0.clone().requires_grad_(), g0.clone()
    wrt = [sP, sU, sW] + ([bn.weight, bn.bias] if bn is not None else [])

    def step():
        h = HF.expand_act(sP, sU, sW, bn, case[6])
        return (h,) + torch.autograd.grad(h, wrt, sg)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not memsets_of(step)
    with HF.deterministic(True):
        assert not memsets_of(step)                 # the operator has nothing to add to the deterministic mode
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for seed in (1, 2, 3):
        P, U, Wu, _, _, _, _, g_h = inputs(case, seed)
        sP.data.copy_(P); sU.data.copy_(U); sW.data.copy_(Wu); sg.copy_(g_h)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static]
        want = step()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (seed, i)
        assert all(torch.isfinite(t).all() for t in got)


def test_a_step_stores_neither_y_nor_g_y():
    """(64, 64, 256, 3, per-row, train): one (R,S,O) f32 tensor is 4 MB.  Beyond the inputs and g_h (allocated before), forward + backward
    may allocate h, the returned gradients and less than half of one such tensor."""
    R, S, O, J = 64, 64, 256, 3
    g = torch.Generator().manual_seed(5)
    P = torch.randn(R, O, generator=g).cuda().requires_grad_()
    U = torch.randn(R, S, J, generator=g).cuda().requires_grad_()
    Wu = torch.randn(O, J, generator=g).cuda().requires_grad_()
    bn = torch.nn.BatchNorm1d(O).cuda().train()
    g_h = torch.randn(R, S, O, generator=g).cuda()

    def step():
        h = HF.expand_act(P, U, Wu, bn, 0.0)
        return (h,) + torch.autograd.grad(h, [P, U, Wu, bn.weight, bn.bias], g_h)

    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    kept = sum(t.numel() * 4 for t in out)
    one = R * S * O * 4
    print("peak rise %.2f MB, of which outputs %.2f MB; one (R,S,O) tensor %.2f MB" % (rise / 2 ** 20, kept / 2 ** 20, one / 2 ** 20))
    assert rise - kept < one // 2, (rise, kept)
    assert all(torch.isfinite(t).all() for t in out)


def test_refusals():
    dev = "cuda"
    bn1 = torch.nn.BatchNorm1d(4).to(dev).train()
    with pytest.raises(ValueError, match="more than 1 value"):
        HF.expand_act(torch.randn(1, 4, device=dev), torch.randn(1, 2, device=dev), torch.randn(4, 2, device=dev), bn1)
    with pytest.raises(ValueError, match="more than 1 value"):
        ops.expand_fwd(torch.randn(1, 4, device=dev), torch.randn(1, 2, device=dev), torch.randn(4, 2, device=dev), bn1.weight.detach(),
                       bn1.bias.detach(), mode=1)
    with pytest.raises(RuntimeError, match="1024"):
        ops.expand_fwd(torch.randn(2, 1025, device=dev), torch.randn(3, 2, device=dev), torch.randn(1025, 2, device=dev))
    with pytest.raises(RuntimeError, match="J <= 4"):
        ops.expand_fwd(torch.randn(2, 8, device=dev), torch.randn(3, 5, device=dev), torch.randn(8, 5, device=dev))
    with pytest.raises(RuntimeError, match="1024"):
        ops.expand_bwd(torch.randn(2, 3, 1025, device=dev), torch.randn(2, 1025, device=dev), torch.randn(2, 3, 2, device=dev),
                       torch.randn(1025, 2, device=dev))
    with pytest.raises(ValueError, match="shared U"):
        HF.expand_act(torch.randn(2, 8, device=dev), torch.randn(3, 2, device=dev, requires_grad=True), torch.randn(8, 2, device=dev))
    # off the served range the node declines, says so, and the torch formulation answers
    HF._declined.clear()
    P, U, Wu = torch.randn(2, 8, device=dev), torch.randn(3, 5, device=dev), torch.randn(8, 5, device=dev)
    assert not HF.expand_usable(P, U, Wu)
    out = HF.expand_act(P, U, Wu, None, 0.2)
    assert HF._declined and torch.equal(out, F.leaky_relu(P.unsqueeze(1) + U @ Wu.t(), 0.2))
    HF._declined.clear()
