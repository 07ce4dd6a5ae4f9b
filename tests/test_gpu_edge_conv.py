"""The edge-convolution kernels (csrc/edge_conv.hip) and the DGCNN grouper on the GPU.

Operator: forward against a float64 evaluation of the torch formulation (1e-5 of each output's scale); arg exactly by the rule of
include/upp_hip.h, restated in numpy on the kernel's own y (one f32 addition: numpy makes the same bits); gradients against the float64
torch formulation with arg PINNED (the inputs hold exact ties, where an unpinned max may legitimately pick another k), by the gradient
bounds of tests/test_gpu_attention_stream.py: close(rtol=2e-5, atol_scale=5e-6).  Then the deterministic mode, capture into a graph, the
memory the default mode allocates, and the module against the fixture of the reference's own class."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _seeded
from conftest import GOLDEN, ROOT
from upp_hip import functional as HF
from upp_hip import ops

sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

pytestmark = pytest.mark.gpu

# (B, Nk, Nq, K, O, G); G = 0: no norm
CASES = [(2, 96, 96, 16, 32, 4), (3, 130, 40, 16, 64, 4), (1, 20, 7, 16, 128, 4), (2, 5, 33, 16, 8, 2), (2, 70, 70, 8, 384, 0),
         (1, 64, 64, 64, 512, 8)]
SLOPE, EPS = 0.2, 1e-5


def close(a, b, rtol=2e-5, atol_scale=5e-6):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol_scale * max(np.abs(b).max(), 1e-30))


def formulation(A, Bq, idx, norm, slope, arg=None):
    """upp_hip.torch_cpu.edge_conv_max in the operands' own precision; with `arg` the max over k is replaced by the pinned pick."""
    B, Nq, K = idx.shape
    O = A.shape[2]
    y = torch.gather(A, 1, idx.reshape(B, Nq * K, 1).expand(-1, -1, O)).view(B, Nq, K, O) + Bq.unsqueeze(2)
    if norm is not None:
        G, gamma, beta, eps = norm
        y = F.group_norm(y.permute(0, 3, 1, 2), G, gamma, beta, eps).permute(0, 2, 3, 1)
    a = F.leaky_relu(y, slope)
    if arg is None:
        return a.max(dim=2)[0]
    return torch.gather(a, 2, arg.long().unsqueeze(2)).squeeze(2)


@functools.lru_cache(maxsize=None)
def inputs(case, seed=0):
    """A, Bq, idx, gamma, beta, g_out on the GPU.  gamma has positive, negative and exactly zero entries; neighbour slots 3, 6 and K - 1
    repeat slots 1, 2 and 0 of their row, so y ties exactly (at Nk = 5 every row is hit many times besides)."""
    B, Nk, Nq, K, O, G = case
    g = torch.Generator().manual_seed(1000 * seed + Nk + 7 * O)
    A = torch.randn(B, Nk, O, generator=g) + 0.5
    Bq = torch.randn(B, Nq, O, generator=g)
    idx = torch.randint(0, Nk, (B, Nq, K), generator=g)
    idx[:, :, 3], idx[:, :, 6], idx[:, :, K - 1] = idx[:, :, 1], idx[:, :, 2], idx[:, :, 0]
    gamma = 1 + 0.5 * torch.randn(O, generator=g)
    gamma[1::3] *= -1
    gamma[2::5] = 0.0
    beta = 0.3 * torch.randn(O, generator=g)
    g_out = torch.randn(B, Nq, O, generator=g)
    return tuple(t.cuda() for t in (A, Bq, idx, gamma, beta, g_out))


def norm_of(case, gamma, beta):
    return (case[5], gamma, beta, EPS) if case[5] else None


@functools.lru_cache(maxsize=None)
def kernel_run(case, deterministic=False):
    """One forward + backward through the library (ops level: arg, mean, rstd are outputs there)."""
    A, Bq, idx, gamma, beta, g_out = inputs(case)
    G = case[5]
    out, arg, mean, rstd = ops.edge_conv_fwd(A, Bq, idx, gamma, beta, G, EPS, SLOPE)
    grads = ops.edge_conv_bwd(g_out, A, Bq, idx, arg, gamma, beta, mean, rstd, G, SLOPE, deterministic=deterministic)
    torch.cuda.synchronize()
    return (out, arg, mean, rstd) + tuple(grads)


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64: out / mean / rstd of the formulation (free max), and the gradients with the kernel's arg pinned."""
    A, Bq, idx, gamma, beta, g_out = inputs(case)
    B, Nk, Nq, K, O, G = case
    arg = kernel_run(case)[1]
    Ad, Bd = A.double().requires_grad_(), Bq.double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    norm = norm_of(case, gd, bd)
    with torch.no_grad():
        out = formulation(Ad, Bd, idx, norm, SLOPE)
        mean = rstd = None
        if G:
            y = (torch.gather(Ad, 1, idx.reshape(B, Nq * K, 1).expand(-1, -1, O)).view(B, Nq, K, O) + Bd.unsqueeze(2))
            yg = y.view(B, Nq, K, G, O // G).permute(0, 3, 1, 2, 4).reshape(B, G, -1)
            mean, rstd = yg.mean(-1), 1.0 / torch.sqrt(yg.var(-1, unbiased=False) + EPS)
    pinned = formulation(Ad, Bd, idx, norm, SLOPE, arg)
    grads = torch.autograd.grad(pinned, [Ad, Bd] + ([gd, bd] if G else []), g_out.double())
    return (out, mean, rstd) + tuple(grads) + ((None, None) if not G else ())


@pytest.mark.parametrize("case", CASES)
def test_forward_against_float64(case):
    out, arg, mean, rstd = kernel_run(case)[:4]
    r_out, r_mean, r_rstd = reference(case)[:3]
    for name, got, want in (("out", out, r_out), ("mean", mean, r_mean), ("rstd", rstd, r_rstd)):
        if want is None:
            assert got is None
            continue
        err = ((got.double() - want).abs().max() / want.abs().max()).item()
        print("%s %s: max error / scale = %.3g" % (case, name, err))
        assert err < 1e-5, (name, err)
    assert arg.dtype == torch.uint8 and arg.shape == out.shape


@pytest.mark.parametrize("case", CASES)
def test_arg_follows_the_stated_rule_exactly(case):
    A, Bq, idx, gamma, beta, _ = inputs(case)
    B, Nk, Nq, K, O, G = case
    _, arg, _, rstd = kernel_run(case)[:4]
    A_, B_, i_ = A.cpu().numpy(), Bq.cpu().numpy(), idx.cpu().numpy()
    y = A_[np.arange(B)[:, None, None], i_] + B_[:, :, None, :]                     # (B,Nq,K,O), one f32 addition each
    assert y.dtype == np.float32
    hi, lo = y.argmax(axis=2), y.argmin(axis=2)                                    # numpy: the FIRST extreme, i.e. the lowest k
    if G:
        s = gamma.cpu().numpy()[None, :] * np.repeat(rstd.cpu().numpy(), O // G, axis=1)          # gamma * rstd, an f32 product, (B,O)
        assert s.dtype == np.float32 and (s > 0).any() and (s < 0).any() and (s == 0).any()
        want = np.where(s[:, None, :] > 0, hi, np.where(s[:, None, :] < 0, lo, 0))
    else:
        want = hi
    ties = (np.sort(y, axis=2)[:, :, -1] == np.sort(y, axis=2)[:, :, -2]).mean()
    print("%s: %.0f %% of the (q, o) maxima are exact ties" % (case, 100 * ties))
    assert np.array_equal(arg.cpu().numpy(), want.astype(np.uint8))


@pytest.mark.parametrize("case", CASES)
def test_gradients_against_the_pinned_formulation(case):
    got = kernel_run(case)[4:]
    want = reference(case)[3:]
    for name, g, w in zip(("g_A", "g_Bq", "g_gamma", "g_beta"), got, want):
        if w is None:
            assert g is None
            continue
        print("%s %s: max error / scale = %.3g" % (case, name, ((g.double() - w).abs().max() / w.abs().max()).item()))
        close(g, w)


@pytest.mark.parametrize("case", CASES)
def test_deterministic_mode(case):
    A, Bq, idx, gamma, beta, g_out = inputs(case)
    G = case[5]
    first = {False: kernel_run(case, False), True: kernel_run(case, True)}
    for det in (False, True):
        for _ in range(2):
            out, arg, mean, rstd = ops.edge_conv_fwd(A, Bq, idx, gamma, beta, G, EPS, SLOPE)
            again = (out, arg, mean, rstd) + tuple(ops.edge_conv_bwd(g_out, A, Bq, idx, arg, gamma, beta, mean, rstd, G, SLOPE, deterministic=det))
            for i, (a, b) in enumerate(zip(first[det], again)):
                if i == 4 and not det:
                    continue                                    # g_A by atomics: the hardware's order
                assert (a is None and b is None) or torch.equal(a, b), (det, i)
    # the two modes: the same numbers except g_A, which agrees within the gradient bounds (and with the pinned reference)
    for i, (a, b) in enumerate(zip(first[False], first[True])):
        if i == 4:
            close(b, a)
            close(b, reference(case)[3])
        else:
            assert (a is None and b is None) or torch.equal(a, b), i


def test_the_node_reads_the_mode_when_it_runs(monkeypatch):
    """HF.edge_conv_max: deterministic=None follows functional.DETERMINISTIC at BACKWARD time; True / False are per call."""
    case = CASES[0]
    A, Bq, idx, gamma, beta, g_out = inputs(case)
    seen = []
    real = ops.edge_conv_bwd
    monkeypatch.setattr(ops, "edge_conv_bwd", lambda *a, **k: (seen.append(k["deterministic"]), real(*a, **k))[1])
    for per_call, flag, want in ((None, False, False), (None, True, True), (True, False, True), (False, True, False)):
        a, b = A.clone().requires_grad_(), Bq.clone().requires_grad_()
        out = HF.edge_conv_max(a, b, idx, norm_of(case, gamma, beta), SLOPE, deterministic=per_call)
        with HF.deterministic(flag):
            out.backward(g_out)
        assert seen[-1] is want, (per_call, flag)
    close(a.grad, reference(case)[3])
    close(b.grad, reference(case)[4])


@pytest.mark.parametrize("case", [CASES[1], CASES[4]])
def test_forward_and_backward_replay_from_a_graph(case):
    from memset_census import memsets_of
    B, Nk, Nq, K, O, G = case
    A0, Bq0, idx0, gamma, beta, g0 = inputs(case)
    sA, sB, sI, sg = A0.clone().requires_grad_(), Bq0.clone().requires_grad_(), idx0.clone(), g0.clone()
    gam, bet = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    wrt = [sA, sB] + ([gam, bet] if G else [])

    def step():
        out = HF.edge_conv_max(sA, sB, sI, norm_of(case, gam, bet), SLOPE)
        return (out,) + torch.autograd.grad(out, wrt, sg)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not memsets_of(step)
    with HF.deterministic(True):
        assert not memsets_of(step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for seed in (1, 2, 3):
        A, Bq, idx, _, _, g_out = inputs(case, seed)
        sA.data.copy_(A); sB.data.copy_(Bq); sI.copy_(idx); sg.copy_(g_out)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static]
        want = step()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            if i == 1:
                close(a, b)                                     # g_A: atomics
            else:
                assert torch.equal(a, b), (seed, i)
        assert torch.isfinite(got[1]).all()


def test_default_mode_allocates_no_neighbourhood_tensor():
    """(2, 1024, 1024, 16, 32, 4): one (B,Nq,K,O) f32 tensor is 4 MB; forward + backward may rise by less than 2 MB above the inputs."""
    B, Nk, Nq, K, O, G = 2, 1024, 1024, 16, 32, 4
    g = torch.Generator().manual_seed(5)
    A = torch.randn(B, Nk, O, generator=g).cuda().requires_grad_()
    Bq = torch.randn(B, Nq, O, generator=g).cuda().requires_grad_()
    idx = torch.randint(0, Nk, (B, Nq, K), generator=g).cuda()
    gamma, beta = torch.ones(O, device="cuda", requires_grad=True), torch.zeros(O, device="cuda", requires_grad=True)
    g_out = torch.randn(B, Nq, O, generator=g).cuda()

    def step():
        out = HF.edge_conv_max(A, Bq, idx, (G, gamma, beta, EPS), SLOPE, deterministic=False)
        return torch.autograd.grad(out, [A, Bq, gamma, beta], g_out)

    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    grads = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("default mode: peak rise %.2f MB" % (rise / 2 ** 20))
    assert rise < 2 * 2 ** 20, rise
    assert all(torch.isfinite(t).all() for t in grads)


# ------------------------------------------------------------------ the module
def test_module_equals_the_reference_fixture():
    from models.dgcnn_group import DGCNN_Grouper
    g = np.load(os.path.join(GOLDEN, "dgcnn_grouper.npz"))
    model = _seeded.fill(DGCNN_Grouper()).cuda().eval()
    x = _seeded.unit_ball_clouds(2, 640, seed=0).cuda()
    HF._declined.clear()
    with torch.no_grad():
        coor, f = model(x.transpose(1, 2).contiguous())
    assert np.array_equal(coor.cpu().numpy(), g["coor"])
    err = np.abs(f.cpu().numpy() - g["f"]).max() / np.abs(g["f"]).max()
    print("f: max error / scale = %.3g" % err)
    assert err < 1e-5, err
    assert not HF._declined, HF._declined


def _module_formulation(model, x, num, lists):
    """The reference's layer in float64 -- conv of [f_j - f_i ; f_i], GroupNorm, LeakyReLU, max over k -- on the neighbour lists, FPS picks
    and arg bytes the fused run used (lists: per layer (idx, arg); picks: per down-sampling the index list)."""
    sd = {k: v.detach().double().requires_grad_() for k, v in model.state_dict(keep_vars=True).items()}
    xd = x.detach().double().requires_grad_()

    def edge(i, f_q, f_k):
        idx, arg = lists["edge"][i - 1]
        B, Nq, K = idx.shape
        C = f_k.shape[2]
        nb = torch.gather(f_k, 1, idx.reshape(B, Nq * K, 1).expand(-1, -1, C)).view(B, Nq, K, C)
        e = torch.cat([nb - f_q.unsqueeze(2), f_q.unsqueeze(2).expand(-1, -1, K, -1)], -1)
        y = e @ sd["layer%d.0.weight" % i].view(-1, 2 * C).t()
        y = F.group_norm(y.permute(0, 3, 1, 2), 4, sd["layer%d.1.weight" % i], sd["layer%d.1.bias" % i], 1e-5).permute(0, 2, 3, 1)
        return torch.gather(F.leaky_relu(y, 0.2), 2, arg.long().unsqueeze(2)).squeeze(2)

    def pick(t, j):
        return torch.gather(t, 1, lists["fps"][j].long().unsqueeze(-1).expand(-1, -1, t.shape[2]))

    f = xd @ sd["input_trans.weight"].view(8, 3).t() + sd["input_trans.bias"]
    f = edge(1, f, f)
    coor, f_q = pick(xd, 0), pick(f, 0)
    f = edge(2, f_q, f)
    f = edge(3, f, f)
    coor, f_q = pick(coor, 1), pick(f, 1)
    f = edge(4, f_q, f)
    return coor, f, xd, sd


def test_module_forward_and_backward_against_the_pinned_formulation(monkeypatch):
    from models.dgcnn_group import DGCNN_Grouper
    model = _seeded.fill(DGCNN_Grouper()).cuda().train()
    x = _seeded.unit_ball_clouds(2, 160, seed=3).cuda().requires_grad_()
    g = torch.Generator().manual_seed(11)
    g_c, g_f = torch.randn(2, 32, 3, generator=g).cuda(), torch.randn(2, 32, 128, generator=g).cuda()
    lists = {"edge": [], "fps": []}
    real_fwd, real_fps = ops.edge_conv_fwd, ops.fps

    def traced_fwd(A, Bq, idx, *a, **k):
        r = real_fwd(A, Bq, idx, *a, **k)
        lists["edge"].append((idx, r[1]))
        return r

    def traced_fps(*a, **k):
        r = real_fps(*a, **k)
        lists["fps"].append(r[0] if isinstance(r, tuple) else r)
        return r

    def run():
        coor, f = model(x, [64, 32])
        torch.autograd.backward([coor, f], [g_c, g_f])
        return coor, f

    run()                                                               # (warm-up: caches, lazy initialisation)
    model.zero_grad(); x.grad = None
    HF._declined.clear()
    monkeypatch.setattr(ops, "edge_conv_fwd", traced_fwd)
    monkeypatch.setattr(ops, "fps", traced_fps)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        coor, f = run()
        torch.cuda.synchronize()
    assert not HF._declined, HF._declined
    assert coor.shape == (2, 32, 3) and f.shape == (2, 32, 128) and len(lists["edge"]) == 4 and len(lists["fps"]) == 2

    # only the documented launches (README "The DGCNN grouper"): this library's kernels and torch's element-wise kernels (the layout
    # changes at entry and exit, the (O, 2C) weight slices and their gradients) -- no library GEMM, no top-k / sort / index kernel, no
    # GroupNorm kernel, no reduction, no memset
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    print("\n".join(names))
    ours = [n for n in names if "at::" not in n]
    for n in names:
        assert "memset" not in n.lower() and "Cijk" not in n and "gemm" not in n.lower(), n
        assert "at::" not in n or "elementwise_kernel" in n, n
    for frag in ("ec_stats_kernel", "ec_finalize_kernel", "ec_apply_kernel", "ec_bwd_reduce_kernel", "ec_bwd_group_kernel", "ec_bwd_param_kernel",
                 "ec_bwd_apply_kernel", "knn", "fps"):
        assert any(frag in n for n in ours), frag

    r_coor, r_f, xd, sd = _module_formulation(model, x, [64, 32], lists)
    torch.autograd.backward([r_coor, r_f], [g_c.double(), g_f.double()])
    assert torch.equal(coor.double(), r_coor)
    print("f: max error / scale = %.3g" % ((f.double() - r_f).abs().max() / r_f.abs().max()).item())
    close(f, r_f)
    for name, p in [("x", x)] + list(model.named_parameters()):
        want = xd.grad if name == "x" else sd[name].grad
        print("grad %s: max error / scale = %.3g" % (name, ((p.grad.double() - want).abs().max() / want.abs().max()).item()))
        close(p.grad, want)
