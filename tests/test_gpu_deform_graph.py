"""The deformable graph attention on the GPU (include/upp_hip.h "deformable graph attention", csrc/interp_max.hip and the ball form of
csrc/deform_attn.hip's offset kernel): the interpolate-max operator bit for bit against its numpy statement
(tests/_interp_max_reference.py) on lattice inputs, where every fma of the statement is exact, and against float64 on random ones; its
backward against float64 with the arg replayed; the deterministic form against the stated order; hostile inputs; the ball offset
against float64; graph capture, memory, the kernel list; the module on the fixture cases of tests/golden/deform_graph.npz with its
gradients against float64 on the same discrete choices; the opt-in wiring into AdaPoinTr.

Bounds.  Against float64: max(5e-6, 3 x err_torch) of the float64 tensor's maximum, err_torch the f32 torch formulation's own error on the
same inputs and the same discrete choices, computed here (the rule of tests/test_gpu_pointr.py).  Fixture: max(1e-5, 3 x err_ref).

Measured on MI355X: see README "Deformable graph attention"."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import _deform_graph_case as case
import _interp_max_reference as R
import _seeded
from _attention_reference import _err, _memsets
from conftest import GOLDEN
from models import AdaPoinTr, Transformer_utils
from upp_hip import _abi, functional as HF, ops, torch_cpu

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 1), (2, 5, 7, 3, 65), (1, 65, 130, 32, 384), (2, 33, 3, 8, 1024)]          # (B, N, NK, k, O)
OFFSET_BRANCH = ("proj_v_off.", "linear_offset.")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "deform_graph.npz"))


def _bound(err_torch):
    return max(5e-6, 3 * err_torch)


def _operands(B, N, NK, k, O, seed=0, lattice=False, one_row=False):
    """PW, Bq, idx3, w3, cotangent.  idx3 / w3 as three_nn and the reference's weight formula leave them: three distinct points per
    row, weights that sum to 1; with NK < 3 the missing slots are index 0 at distance +inf, so weight 0.  lattice: values on a grid on
    which every fma of the numpy statement is exact (PW, Bq multiples of 2^-6 in [-4, 4), w3 a permutation of (4, 3, 1) / 8), which
    also makes exact ties between slots common."""
    g = torch.Generator(device='cuda').manual_seed(seed + 7919 * N + 101 * NK + 13 * k + O)
    if lattice:
        rnd = lambda *s: torch.randint(-256, 256, s, device='cuda', generator=g).float() / 64
    else:
        rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)
    PW, Bq, w = rnd(B, NK, O), rnd(B, N, O), rnd(B, N, O)
    idx3 = torch.rand(B, N * k, NK, device='cuda', generator=g).argsort(-1)[..., :3]
    if lattice:
        perm = torch.rand(B, N * k, 3, device='cuda', generator=g).argsort(-1)
        w3 = torch.tensor([4.0, 3.0, 1.0], device='cuda')[perm]
    else:
        w3 = torch.rand(B, N * k, 3, device='cuda', generator=g) + 0.05
    if NK < 3:
        idx3 = torch.cat([idx3, idx3.new_zeros(B, N * k, 3 - NK)], -1)
        w3[..., NK:] = 0
    if one_row:
        idx3 = torch.full_like(idx3, NK // 2)
    return PW, Bq, idx3.int().contiguous(), (w3 / w3.sum(-1, keepdim=True)).contiguous(), w


def _np(*ts):
    return [t.detach().cpu().numpy() for t in ts]


def _replayed(PW, Bq, idx3, w3, w, slope, arg, dtype):
    """the torch formulation in `dtype` with the max taken at `arg` -> out, d_PW, d_Bq"""
    x = [t.detach().to(dtype).requires_grad_() for t in (PW, Bq)]
    pick = lambda y: y.gather(2, arg.long().unsqueeze(2)).squeeze(2)
    out = torch_cpu.interp_edge_max(x[0], x[1], idx3, w3.to(dtype), slope, pick)
    (out * w.to(dtype)).sum().backward()
    return out.detach(), x[0].grad, x[1].grad


# ---- a. the forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_forward_has_the_bits_of_the_numpy_statement(shape, slope):
    PW, Bq, idx3, w3, _ = _operands(*shape, lattice=True)
    out, arg = ops.interp_max_fwd(PW, Bq, idx3, w3, slope)
    want, want_arg, _ = R.forward(*_np(PW, Bq, idx3, w3), slope)
    assert out.shape == arg.shape == (shape[0], shape[1], shape[4]) and arg.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(arg.cpu().numpy(), want_arg)
    if shape[2] == 3:
        # eight slots over the six weightings of three points: two slots of every query are the same row, so exact ties are certain and
        # the comparison above has seen the lowest-slot rule at work
        y = (torch.gather(PW, 1, idx3.long().reshape(shape[0], -1, 1).expand(-1, -1, shape[4])).view(shape[0], -1, 3, shape[4])
             * w3.unsqueeze(-1)).sum(2).view(shape[0], shape[1], shape[3], shape[4]) + Bq.unsqueeze(2)
        assert ((y == y.max(2, keepdim=True)[0]).sum(2) > 1).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_backward_against_float64_with_the_arg_replayed(shape):
    PW, Bq, idx3, w3, w = _operands(*shape)
    NK = shape[2]
    out, arg = ops.interp_max_fwd(PW, Bq, idx3, w3, 0.2)
    f64, t32 = _replayed(PW, Bq, idx3, w3, w, 0.2, arg, torch.float64), _replayed(PW, Bq, idx3, w3, w, 0.2, arg, torch.float32)
    det =ops.interp_max_bwd(w, out, arg, idx3, w3, NK, 0.2, deterministic=True)
    atomic = ops.interp_max_bwd(w, out, arg, idx3, w3, NK, 0.2, deterministic=False)
    assert torch.equal(det[0], atomic[0])                                   # d_Bq is written once per element in both forms
    for name, got, i in (("out", out, 0), ("d_PW det", det[1], 1), ("d_PW atomic", atomic[1], 1), ("d_Bq", det[0], 2)):
        e_k, e_t = _err(got, f64[i]), _err(t32[i], f64[i])
        print("%s %s: kernel %.2e torch_f32 %.2e of max|f64|, bound %.2e" % (shape, name, e_k, e_t, _bound(e_t)))
        assert torch.isfinite(got).all() and e_k <= _bound(e_t), (name, e_k, e_t)
    e = _err(atomic[1], det[1])
    assert e <= _bound(_err(t32[1], f64[1])), e                             # the atomic form against the ordered one


# ---- b. the deterministic form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, one_row, slope", [((1, 1, 1, 1, 1), False, 0.2), ((2, 5, 7, 3, 65), False, 0.2), ((2, 5, 7, 3, 65), False, 0.0),
                                                   ((2, 5, 7, 3, 65), False, 1.0), ((2, 33, 3, 8, 1024), False, 0.2),
                                                   ((2, 40, 6, 4, 70), True, 0.2), ((1, 65, 130, 32, 384), False, 0.2)])
def test_det_scatter_has_the_bits_of_the_stated_order(shape, one_row, slope):
    PW, Bq, idx3, w3, w = _operands(*shape, seed=3, one_row=one_row)
    NK = shape[2]
    out, arg = ops.interp_max_fwd(PW, Bq, idx3, w3, slope)
    d_Bq, d_PW = ops.interp_max_bwd(w, out, arg, idx3, w3, NK, slope, deterministic=True)
    again = ops.interp_max_bwd(w, out, arg, idx3, w3, NK, slope, deterministic=True)
    assert torch.equal(d_PW, again[1]) and torch.equal(d_Bq, again[0])
    args = _np(w, out, arg, idx3, w3)
    want_Bq, want_PW = R.scatter_det(*args, slope, NK)
    assert np.array_equal(d_Bq.cpu().numpy(), want_Bq) and np.array_equal(d_PW.cpu().numpy(), want_PW)
    if one_row:
        _, rev = R.scatter_det(*args, slope, NK, reverse=True)
        assert not np.array_equal(rev, want_PW)                            # the order matters on this input, so the equality above says something
        assert not d_PW[:, :NK // 2].any() and not d_PW[:, NK // 2 + 1:].any()
    atomic = ops.interp_max_bwd(w, out, arg, idx3, w3, NK, slope, deterministic=False)
    assert torch.equal(atomic[0], d_Bq)
    np.testing.assert_allclose(atomic[1].cpu().numpy(), want_PW, rtol=0, atol=5e-6 * np.abs(want_PW).max())


def test_the_mode_is_read_when_the_backward_runs_and_the_call_overrides_it(monkeypatch):
    PW, Bq, idx3, w3, w = _operands(2, 5, 7, 3, 65)
    seen, real = [], ops.interp_max_bwd

    def spy(*a, **k):
        seen.append(k["deterministic"])
        return real(*a, **k)

    monkeypatch.setattr(ops, "interp_max_bwd", spy)
    for per_call, flag, want in [(None, False, False), (None, True, True), (True, False, True), (False, True, False)]:
        x = PW.clone().requires_grad_()
        out = HF.interp_edge_max(x, Bq, idx3, w3, deterministic=per_call)          # forward outside the block, backward inside
        with HF.deterministic(flag):
            out.backward(w)
        assert seen[-1] is want, (per_call, flag)


# ---- c. hostile inputs ---------------------------------------------------------------------------------------------------------------------
def _raw(PW, Bq, idx3, w3, w, slope, det, fill):
    """the entry points on buffers that hold stale garbage: every element must be overwritten"""
    B, N, O = Bq.shape
    NK, k = PW.shape[1], idx3.shape[1] // N
    out, d_Bq, d_PW = (torch.full(s, fill, device='cuda') for s in ((B, N, O), (B, N, O), (B, NK, O)))
    arg = torch.full((B, N, O), 0xFF, dtype=torch.uint8, device='cuda')
    ops._call(PW.device, "upp_interp_max_fwd", _abi.ptr(PW), _abi.ptr(Bq), _abi.ptr(idx3), _abi.ptr(w3), _abi.ptr(out), _abi.ptr(arg),
              slope, B, N, NK, k, O)
    ops._call(PW.device, "upp_interp_max_bwd_det" if det else "upp_interp_max_bwd", _abi.ptr(w), _abi.ptr(out), _abi.ptr(arg),
              _abi.ptr(idx3), _abi.ptr(w3), _abi.ptr(d_Bq), _abi.ptr(d_PW), slope, B, N, NK, k, O)
    return out, arg, d_Bq, d_PW


@pytest.mark.parametrize("hostile", ["negative", "foreign", "ties"])
def test_hostile_inputs_on_stale_buffers(hostile):
    shape = (2, 5, 7, 3, 65)
    PW, Bq, idx3, w3, w = _operands(*shape, seed=11, lattice=True)
    NK = shape[2]
    if hostile == "negative":
        Bq = Bq - 64.0                                                     # every y below zero: the slope branch everywhere
    elif hostile == "foreign":
        idx3 = idx3.clone()
        flat = idx3.view(-1)
        flat[0::5], flat[1::7], flat[2::11] = -1, NK, 2 ** 31 - 1
        assert ((idx3 >= 0) & (idx3 < NK)).any()
    else:
        k = shape[3]
        idx3, w3 = idx3.clone(), w3.clone()
        idx3[:, 2::k], w3[:, 2::k] = idx3[:, 1::k], w3[:, 1::k]            # slot 2 repeats slot 1: exact ties wherever either wins
    want, want_arg, m = R.forward(*_np(PW, Bq, idx3, w3), 0.2)
    want_Bq, want_PW = R.scatter_det(*_np(w), want, want_arg, *_np(idx3, w3), 0.2, NK)
    if hostile == "negative":
        assert (m < 0).all()
    if hostile == "ties":
        assert (want_arg == 1).any() and not (want_arg == 2).any()
    for fill in (float("nan"), 1e30):
        out, arg, d_Bq, d_PW = _raw(PW, Bq, idx3, w3, w, 0.2, True, fill)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(arg.cpu().numpy(), want_arg)
        assert np.array_equal(d_Bq.cpu().numpy(), want_Bq) and np.array_equal(d_PW.cpu().numpy(), want_PW)
        out, arg, d_Bq, d_PW = _raw(PW, Bq, idx3, w3, w, 0.2, False, fill)
        assert np.array_equal(d_Bq.cpu().numpy(), want_Bq)
        np.testing.assert_allclose(d_PW.cpu().numpy(), want_PW, rtol=0, atol=5e-6 * np.abs(want_PW).max())
    fused = HF.interp_edge_max(PW, Bq, idx3, w3, 0.2)
    assert np.array_equal(fused.cpu().numpy(), want)


# ---- d. the ball offset -------------------------------------------------------------------------------------------------------------------
def _offset_operands(B, G, N, NK, k, C, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed + 31 * N + NK)
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)
    A, Bq, pos, gamma, beta, W3 = rnd(B, G, NK, C), rnd(B, G, N, C), rnd(B, NK, 3), rnd(C), rnd(C), rnd(3, C) * C ** -0.5
    idx = torch.randint(0, NK, (B, N, k), device='cuda', generator=g)
    return A, Bq, idx, pos, gamma, beta, 1e-5, W3


def _f64(x):
    return tuple(t.double() if isinstance(t, torch.Tensor) and t.is_floating_point() else t for t in x)


@pytest.mark.parametrize("shape", [(1, 1, 3, 5, 1, 64), (2, 2, 9, 6, 8, 128), (1, 1, 40, 24, 32, 1024)])
def test_ball_offset_against_float64(shape):
    B, G, N, NK, k, C = shape
    x = _offset_operands(*shape)
    HF._declined.clear()
    got = HF.deform_offset(*x, ball=True)
    assert not HF._declined, HF._declined
    t32 = torch_cpu.deform_offset(*x, ball=True)
    f64 = torch_cpu.deform_offset(*_f64(x), ball=True)
    e_k, e_t = _err(got, f64), _err(t32, f64)
    print("%s ball shift: kernel %.2e torch_f32 %.2e of max|f64|, bound %.2e" % (shape, e_k, e_t, _bound(e_t)))
    assert got.shape == (B, G, N * k, 3) and torch.isfinite(got).all() and e_k <= _bound(e_t), (e_k, e_t)
    assert torch.equal(got, HF.deform_offset(*x, ball=True))
    local = torch.gather(x[3], 1, x[2].reshape(B, N * k, 1).expand(-1, -1, 3))
    if k == 1:
        assert torch.equal(got, local.unsqueeze(1).expand(-1, G, -1, -1))            # r = 0: shift == pos[idx] exactly
    else:
        half = 0.5 * (local.view(B, N, k, 3).max(2)[0] - local.view(B, N, k, 3).min(2)[0])
        assert ((got.view(B, G, N, k, 3) - local.view(B, 1, N, k, 3)).abs() <= half.view(B, 1, N, 1, 3) * (1 + 1e-6) + 1e-6).all()
    # the default keeps the bits of the existing entry point
    plain = torch.empty_like(got)
    ops._call(x[0].device, "upp_deform_offset_fwd", *(_abi.ptr(t) for t in (x[0], x[1], x[2], x[3], x[4], x[5], x[7], plain)), 1e-5,
              B, G, N, NK, k, C)
    assert torch.equal(HF.deform_offset(*x), plain) and torch.equal(HF.deform_offset(*x, ball=False), plain)
    assert not torch.equal(plain, got)


def test_ball_offset_with_a_slot_outside_the_cloud_is_nan_for_its_query_only():
    B, G, N, NK, k, C = 2, 2, 9, 6, 8, 128
    x = list(_offset_operands(B, G, N, NK, k, C))
    good = HF.deform_offset(*x, ball=True)
    x[2] = x[2].clone()
    x[2][0, 3, 5], x[2][1, 0, 0] = NK, -1
    got = HF.deform_offset(*x, ball=True).view(B, G, N, k, 3)
    bad = torch.zeros(B, N, dtype=torch.bool, device='cuda')
    bad[0, 3] = bad[1, 0] = True
    assert torch.isnan(got[bad.unsqueeze(1).expand(-1, G, -1)]).all()
    keep = ~bad.view(B, 1, N, 1, 1).expand_as(got)
    assert torch.equal(got[keep], good.view(B, G, N, k, 3)[keep])


# ---- e. graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
def test_forward_and_backward_replay_from_a_graph(deterministic):
    shape = (2, 40, 24, 8, 128)
    st = [t.clone() for t in _operands(*shape)]
    leaves = [t.requires_grad_() for t in st[:2]]

    def step():
        out = HF.interp_edge_max(*leaves, st[2], st[3], 0.2, deterministic=deterministic)
        return (out,) + torch.autograd.grad(out, leaves, st[4])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not _memsets(step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for seed in (1, 2):
        fresh = _operands(*shape, seed=seed)
        with torch.no_grad():
            for dst, src in zip(st, fresh):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static]
        want = step()
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "d_PW", "d_Bq"), got, want):
            if not deterministic and name == "d_PW":
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=5e-6 * b.abs().max().item())
            else:
                assert torch.equal(a, b), (seed, name)


# ---- f. memory ----------------------------------------------------------------------------------------------------------------------------
def test_fused_path_keeps_no_neighbourhood_tensor(monkeypatch):
    """(B,N,NK,k,O) = (2,512,512,16,128): one (B,N,k,O) f32 tensor is 8 MB.  The module's fused forward + backward rises by less than
    one of them above its operands and results; the torch formulation's figure is printed beside it."""
    B, N, NK, k, C = 2, 512, 512, 16, 128
    unit = B * N * k * C * 4
    m = _seeded.fill(Transformer_utils.improvedDeformableLocalGraphAttention(C, k=k)).cuda()
    g = torch.Generator(device='cuda').manual_seed(1)
    q, v, w = (torch.randn(B, n, C, device='cuda', generator=g) for n in (N, NK, N))
    q_pos, v_pos = _seeded.unit_ball_clouds(B, N, seed=1).cuda(), _seeded.unit_ball_clouds(B, NK, seed=2).cuda()
    q.requires_grad_(), v.requires_grad_()
    wrt = [q, v] + [p for n, p in m.named_parameters() if not any(o in n for o in OFFSET_BRANCH)]
    idx = Transformer_utils.knn_point(k, v_pos, q_pos)

    def rise():
        def step():
            out = m(q, q_pos, v=v, v_pos=v_pos, idx=idx)
            return (out,) + torch.autograd.grad(out, wrt, w)
        step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base - sum(t.numel() * 4 for t in res)

    HF._declined.clear()
    fused = rise()
    assert not HF._declined, HF._declined
    monkeypatch.setattr(m, "fusable", lambda q, v: False)
    plain = rise()
    HF._declined.clear()
    print("peak rise above operands and results: fused %.2f MB, torch formulation %.2f MB ((B,N,k,O) = %.0f MB)"
          % (fused / 2 ** 20, plain / 2 ** 20, unit / 2 ** 20))
    assert fused < unit, fused
    assert plain >= unit, plain


# ---- g. the module ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case.CASES)
def test_fused_path_meets_the_fixture_bound(fixture, name):
    m = case.module(AdaPoinTr, Transformer_utils, name).cuda()
    x = [t.cuda() for t in case.inputs(int(fixture["seed_" + name]))]
    HF._declined.clear()
    with torch.no_grad():
        got = case.run(m, name, *x)
    assert not HF._declined, HF._declined
    case.check_output(fixture, name, got, "fused path")


class Choices:
    """Record the discrete choices of one f32 forward (the neighbour lists, the three nearest points of every shifted position, the arg
    of every interpolate-max and the branch of its LeakyReLU), or replay them into another evaluation of the same module made of torch
    operators; the replayed distances are recomputed from the replayed indices in the precision of the run.  Patches the names the
    module code calls, as tests/test_gpu_pointr.py's instrument does."""

    def __init__(self, monkeypatch, items=None):
        self.m, self.items, self.replay, self.pos = monkeypatch, ([] if items is None else items), items is not None, 0

    def get(self, tag):
        got, val = self.items[self.pos]
        assert got == tag, (self.pos, got, tag)
        self.pos += 1
        return val

    def install(self):
        knn, three, fwd, plain = HF.knn_query, Transformer_utils.shifted_three_nn, ops.interp_max_fwd, torch_cpu.interp_edge_max

        def knn_query(ref, query, k):
            if not self.replay:
                r = knn(ref, query, k)
                self.items.append(("knn", r[1].clone()))
                return r
            return None, self.get("knn")

        def shifted_three_nn(shift, known):
            if not self.replay:
                r = three(shift, known)
                self.items.append(("three", r[1].clone()))
                return r
            idx3 = self.get("three")
            near = torch.gather(known, 1, idx3.long().reshape(idx3.shape[0], -1, 1).expand(-1, -1, 3)).view(*idx3.shape, 3)
            return (shift.detach().unsqueeze(2) - near.detach()).pow(2).sum(-1).sqrt(), idx3

        def interp_max_fwd(*a, **k):
            r = fwd(*a, **k)
            self.items.append(("max", (r[1].clone(), r[0] > 0)))
            return r

        def interp_edge_max(PW, Bq, idx3, w3, slope=0.2, pool=None):
            if not self.replay:
                box = []

                def pick(y):
                    val, arg = y.max(dim=2)
                    box.append(arg)
                    return val
                out = plain(PW, Bq, idx3, w3, slope, pick)
                self.items.append(("max", (box[0], out.detach() > 0)))
                return out
            arg, mask = self.get("max")
            m = plain(PW, Bq, idx3, w3, 1.0, lambda y: y.gather(2, arg.long().unsqueeze(2)).squeeze(2))        # (slope 1: no gate yet)
            return m * torch.where(mask, torch.ones((), dtype=m.dtype, device=m.device), torch.full((), slope, dtype=m.dtype, device=m.device))

        self.m.setattr(HF, "knn_query", knn_query)
        self.m.setattr(Transformer_utils, "shifted_three_nn", shifted_three_nn)
        if not self.replay:
            self.m.setattr(ops, "interp_max_fwd", interp_max_fwd)
        self.m.setattr(torch_cpu, "interp_edge_max", interp_edge_max)


@pytest.mark.parametrize("name", ["a", "c"])
def test_module_gradients_against_float64_on_the_same_choices(monkeypatch, fixture, name):
    """The fused f32 run and the torch-formulation f32 run each record their discrete choices; the module in float64 is evaluated on the
    recorded choices of each.  The output and every gradient (inputs and parameters) of the fused run must be within
    max(5e-6, 3 x err_torch) of its float64 evaluation, relative to that tensor's maximum, err_torch being the torch formulation's own
    f32-against-f64 error of the same tensor.  The offset branch and the positions have no gradient in any run."""
    model = case.module(AdaPoinTr, Transformer_utils, name).cuda()
    model64 = copy.deepcopy(model).double()
    x = [t.cuda() for t in case.inputs(int(fixture["seed_" + name]))]
    w = torch.randn(x[0].shape, generator=torch.Generator().manual_seed(3)).cuda()
    graph = [mod for mod in model.modules() if isinstance(mod, Transformer_utils.improvedDeformableLocalGraphAttention)]
    assert len(graph) == (1 if name == "a" else 2)

    def run(net, dtype):
        net.zero_grad(set_to_none=True)
        q, v, q_pos, v_pos = (t.to(dtype).clone().requires_grad_() for t in x)
        out = case.run(net, name, q, v, q_pos, v_pos)
        (out * w.to(dtype)).sum().backward()
        assert q_pos.grad is None and v_pos.grad is None
        for n, p in net.named_parameters():
            assert (p.grad is None) == any(o in n for o in OFFSET_BRANCH), n
        return [("forward", out.detach()), ("d_q", q.grad), ("d_v", v.grad)] + [(n + ".grad", p.grad.clone()) for n, p in net.named_parameters()
                                                                              if p.grad is not None]

    def with_float64(fused):
        HF._declined.clear()
        with monkeypatch.context() as m:
            if not fused:
                for mod in graph:
                    m.setattr(mod, "fusable", lambda q, v: False)
            rec = Choices(m)
            rec.install()
            f32 = run(model, torch.float32)
        assert fused == (not any(what.startswith("improvedDeformableLocalGraphAttention") for what, _ in HF._declined)), HF._declined
        with monkeypatch.context() as m:
            rep = Choices(m, rec.items)
            rep.install()
            f64 = run(model64, torch.float64)
        assert rep.pos == len(rec.items) > 0 and sum(tag == "max" for tag, _ in rec.items) == len(graph)
        HF._declined.clear()
        return f32, f64

    fused, fused64 = with_float64(True)
    plain, plain64 = with_float64(False)
    assert [n for n, _ in fused] == [n for n, _ in fused64] == [n for n, _ in plain] == [n for n, _ in plain64]
    scale, scale_t = {n: t.abs().max().item() for n, t in fused64}, {n: t.abs().max().item() for n, t in plain64}
    failures, zeros = [], []
    for (n, a), (_, a64), (_, b), (_, b64) in zip(fused, fused64, plain, plain64):
        assert torch.isfinite(a).all(), n
        unit, unit_t = scale[n], scale_t[n]
        wname = n.replace(".bias.grad", ".weight.grad")
        if n.endswith(".bias.grad") and wname in scale and unit <= 1e-9 * scale[wname] and unit_t <= 1e-9 * scale_t[wname]:
            unit, unit_t = scale[wname], scale_t[wname]                  # exactly 0 in float64: the layer's weight gradient is the scale
            zeros.append(n)
        err_f = ((a.double() - a64).abs().max() / max(unit, 1e-30)).item()
        err_t = ((b.double() - b64).abs().max() / max(unit_t, 1e-30)).item()
        lim = _bound(err_t)
        print("%s: fused against f64 %.3g, torch formulation against f64 %.3g, bound %.3g" % (n, err_f, err_t, lim))
        if not err_f <= lim:
            failures.append((n, err_f, err_t))
    print("exactly 0 in float64: %s" % zeros)
    assert all("k_map.bias" in n for n in zeros), zeros
    assert not failures, failures


def test_fused_module_launches_no_library_gemm_softmax_sort_or_gather(fixture):
    m = case.module(AdaPoinTr, Transformer_utils, "a").cuda()
    q, v, q_pos, v_pos = (t.cuda() for t in case.inputs(int(fixture["seed_a"])))
    q.requires_grad_(), v.requires_grad_()
    w = torch.randn(q.shape, device='cuda')

    def run():
        m.zero_grad(set_to_none=True)
        q.grad = v.grad = None
        (case.run(m, "a", q, v, q_pos, v_pos) * w).sum().backward()

    run()                                                               # (warm-up: caches, lazy initialisation)
    HF._declined.clear()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    assert not HF._declined, HF._declined
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    print("\n".join(names))
    for n in names:
        low = n.lower()
        assert "Cijk_" not in n and "gemm" not in low and "softmax" not in low and "topk" not in low and "sort" not in low, n
        assert not ("at::native" in n and any(t in low for t in ("index", "gather", "scatter"))), n
        assert "memset" not in low, n
    for frag in ("da_offset_kernel", "im_fwd_kernel", "im_bwd_kernel", "three_nn"):
        assert any(frag in n for n in names), frag
    for pname, prm in m.named_parameters():
        assert (prm.grad is None) == any(o in pname for o in OFFSET_BRANCH), pname


def test_dim_96_runs_the_torch_formulation_and_names_the_site():
    m = _seeded.fill(Transformer_utils.improvedDeformableLocalGraphAttention(96, k=case.K)).cuda().eval()
    g = torch.Generator().manual_seed(1)
    q, v = torch.randn(2, case.NQ, 96, generator=g).cuda(), torch.randn(2, case.NK, 96, generator=g).cuda()
    _, _, q_pos, v_pos = (t.cuda() for t in case.inputs(1))
    HF._declined.clear()
    with torch.no_grad():
        got = m(q, q_pos, v=v, v_pos=v_pos)
    sites = [what for what, why in HF._declined if what.startswith("improvedDeformableLocalGraphAttention")]
    assert len(sites) == 1 and "96" in sites[0], HF._declined
    HF._declined.clear()
    assert got.shape == q.shape and torch.isfinite(got).all()


# ---- h. the wiring ------------------------------------------------------------------------------------------------------------------------
def test_adapointr_with_deform_graph_blocks_trains_on_the_fused_path(monkeypatch):
    import _adapointr_model_case as mc
    from utils import misc
    from utils.config import EasyDict
    cfg = mc.config()
    cfg['deformable'] = ['deform', 'deform_graph']
    cfg['encoder_config']['block_style_list'] = ['attn-deform_graph', 'attn']
    cfg['decoder_config']['self_attn_block_style_list'] = ['attn-deform_graph', 'attn-deform']
    cfg['decoder_config']['cross_attn_block_style_list'] = ['attn-deform_graph', 'attn']
    monkeypatch.setattr(misc, "jitter_points", mc.jitter(0))
    model = _seeded.fill(AdaPoinTr.from_cfg(EasyDict(cfg))).cuda().train()
    model.load_state_dict({k: t.clone() for k, t in model.state_dict().items()}, strict=True)
    x, gt = (t.cuda() for t in mc.inputs(0))
    HF._declined.clear()
    ret = model(x)
    loss_denoised, loss_recon = model.get_loss(ret, gt)
    (loss_denoised + loss_recon).backward()
    assert not HF._declined, HF._declined
    assert all(torch.isfinite(t).all() for t in ret) and torch.isfinite(loss_denoised) and torch.isfinite(loss_recon)
    without = {n for n, p in model.named_parameters() if p.grad is None}
    want = {n for n, _ in model.named_parameters() if n.startswith("base_model.query_ranking.") or any(o in n for o in OFFSET_BRANCH)}
    want |= {"base_model.encoder.norm.weight", "base_model.encoder.norm.bias"}      # constructed for its keys and, as in the reference, not applied
    assert without == want, sorted(without ^ want)
    assert sum("linear_offset" in n for n in without) == 4 * 5                       # three graph modules and one deform, five offset-head tensors each
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
