"""The region-wise deformable attention on the GPU (include/upp_hip.h "region-wise deformable attention", csrc/region_attn.hip): the
operator in both backward forms against the float64 torch formulation on the same idx / idx3 / w3 with the kernel's arg replayed
(tests/_attention_reference.py's instrument, and max(5e-6, 3 x err_torch) of the float64 maximum beside it), the validity of the arg,
the softmax hazard, the deterministic form against a numpy restatement of its order (tests/_region_attn_reference.py), poisoned
outputs, the mode switch, graph capture, memory, the module on the fixture cases of tests/golden/rw_deform.npz with its gradients
against float64 on the same discrete choices, its launches, the declined list, and the opt-in wiring into AdaPoinTr.

d_bk is zero in exact arithmetic (a key bias shifts a whole score row, which the softmax does not see): its own maximum is no scale, so
its errors are taken relative to max|d_PK| under the float64 arbitration; in the module test proj_k.bias.grad is taken relative to
proj_k.weight.grad, as tests/test_gpu_deform_attention.py does.

Measured on MI355X: see README "Region-wise deformable attention"."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import _rw_deform_case as case
import _seeded
from _attention_reference import _check_against, _err, _memsets
from _region_attn_reference import scatter_det
from conftest import GOLDEN
from models import AdaPoinTr, Transformer_utils
from upp_hip import _abi, functional as HF, ops, torch_cpu

pytestmark = pytest.mark.gpu

NAMES = ("out", "d_q", "d_PK", "d_PV", "d_bk", "d_bv")
SHAPES = [(1, 1, 1, 1, 1, 1), (2, 5, 7, 3, 2, 1), (2, 40, 40, 8, 2, 2), (1, 65, 130, 32, 6, 2), (1, 3, 4, 10, 4, 4)]      # (B,N,NK,k,H,G)
OFFSET_BRANCH = ("proj_v_off.", "linear_offset.")
SCALE = 0.125


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "rw_deform.npz"))


def _bound(err_torch):
    return max(5e-6, 3 * err_torch)


def _operands(B, N, NK, k, H, G, seed=0, one_point=False):
    """q, idx, PK, PV, bk, bv, idx3, w3, cotangent.  idx: k rows of q per token, drawn with repetition (at N = 3, k = 10 every row is listed
    several times, so the d_q scatter collides).  idx3 / w3 as three_nn and the reference's weight formula leave them: three distinct
    points per row, weights that sum to 1; with NK < 3 the missing slots are index 0 with weight 0."""
    g = torch.Generator(device='cuda').manual_seed(seed + 7919 * N + 101 * NK + 13 * k + H)
    C = 64 * H
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)
    q, PK, PV, bk, bv, w = rnd(B, N, C), rnd(B, G, NK, C), rnd(B, G, NK, C), rnd(C), rnd(C), rnd(B, N, C)
    idx = torch.randint(0, N, (B, N, k), device='cuda', generator=g)
    idx3 = torch.rand(B, G, N * k, NK, device='cuda', generator=g).argsort(-1)[..., :3]
    w3 = torch.rand(B, G, N * k, 3, device='cuda', generator=g) + 0.05
    if NK < 3:
        idx3 = torch.cat([idx3, idx3.new_zeros(B, G, N * k, 3 - NK)], -1)
        w3[..., NK:] = 0
    if one_point:
        idx3 = torch.full_like(idx3, NK // 2)
    return q, idx, PK, PV, bk, bv, idx3.int().contiguous(), (w3 / w3.sum(-1, keepdim=True)).contiguous(), w


def _formulation(x, H, dtype, arg):
    """the torch formulation in `dtype` with the max taken at `arg` -> (out, d_q, d_PK, d_PV, d_bk, d_bv), ctx (B,N,k,C)"""
    q, idx, PK, PV, bk, bv, idx3, w3, w = x
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (q, PK, PV, bk, bv)]
    box = []

    def pick(ctx):
        box.append(ctx.detach())
        return ctx.gather(2, arg.long().unsqueeze(2)).squeeze(2)

    out = torch_cpu.region_attention(leaves[0], idx, leaves[1], leaves[2], leaves[3], leaves[4], idx3, w3.to(dtype), H, SCALE, None, pick)
    (out * w.to(dtype)).sum().backward()
    return (out.detach(),) + tuple(t.grad for t in leaves), box[0]


def _kernels(x, H, deterministic):
    """the operator pair -> (out, d_q, d_PK, d_PV, d_bk, d_bv), arg, rows"""
    q, idx, PK, PV, bk, bv, idx3, w3, w = x
    out, arg = ops.region_attn_fwd(q, idx, PK, PV, bk, bv, idx3, w3, H, SCALE)
    d_q, d_PK, d_PV, d_krow, d_vrow, rows = ops.region_attn_bwd(q, idx, PK, PV, bk, bv, idx3, w3, arg, w, H, SCALE,
                                                                deterministic=deterministic, want_krow=True, want_vrow=True)
    C = q.shape[-1]
    return (out, d_q, d_PK, d_PV, ops.sum_rows(d_krow.view(-1, C)), ops.sum_rows(d_vrow.view(-1, C))), arg, rows


@functools.lru_cache(maxsize=None)
def _case(shape):
    """operands, the kernels' forward (out, arg), and the f32 / f64 formulations on the kernel's arg -- computed once per shape"""
    x = _operands(*shape)
    fwd = ops.region_attn_fwd(*x[:8], shape[4], SCALE)
    t32, _ = _formulation(x, shape[4], torch.float32, fwd[1])
    f64, ctx64 = _formulation(x, shape[4], torch.float64, fwd[1])
    return x, fwd, t32, f64, ctx64


def _judge(got, t32, f64, k, pairwise=True):
    # one slot: p = 1 and ds = p (dp - p dp) = 0 exactly, whatever dp is -- and with it d_q, d_key (so d_PK) and d_bk
    exact_zero = ("d_q", "d_PK", "d_bk") if k == 1 else ()
    bad = []
    for i, name in enumerate(NAMES):
        assert torch.isfinite(got[i]).all(), name
        if name in exact_zero:
            assert not got[i].any(), name
            continue
        if name == "d_bk":
            unit = f64[2].abs().max().item()
            e_k, e_t = ((got[i].double() - f64[i]).abs().max().item() / unit, (t32[i].double() - f64[i]).abs().max().item() / unit)
            print("d_bk: kernel %.2e torch_f32 %.2e of max|d_PK f64| (float64 arbitration; max|d_bk f64| = %.1e)"
                  % (e_k, e_t, f64[i].abs().max().item()))
            if not e_k <= 2 * e_t + 2e-6:
                bad.append((name, e_k, e_t))
            continue
        e_k, e_t = _err(got[i], f64[i]), _err(t32[i], f64[i])
        print("%s: kernel %.2e torch_f32 %.2e of max|f64|, bound %.2e" % (name, e_k, e_t, _bound(e_t)))
        if pairwise:
            _check_against(name, got[i], t32[i], f64[i], 1e-5, 2e-6)
        if not e_k <= _bound(e_t):
            bad.append((name, e_k, e_t))
    assert not bad, bad


# ---- a. operator parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("deterministic", [False, True])
def test_operator_against_float64_with_the_arg_replayed(shape, deterministic):
    x, fwd, t32, f64, _ = _case(shape)
    got, arg, rows = _kernels(x, shape[4], deterministic)
    print("B, N, NK, k, H, G = %s, deterministic %s" % (shape, deterministic))
    assert torch.equal(got[0], fwd[0]) and torch.equal(arg, fwd[1])             # the forward has the same bits on every run
    assert (rows is not None) == deterministic
    _judge(got, t32, f64, shape[3])


@pytest.mark.parametrize("shape", SHAPES)
def test_the_arg_attains_the_float64_maximum(shape):
    x, (out, arg), _, _, ctx64 = _case(shape)
    B, N, NK, k, H, G = shape
    assert arg.dtype == torch.uint8 and arg.shape == out.shape == (B, N, 64 * H) and int(arg.max()) < k
    at = ctx64.gather(2, arg.long().unsqueeze(2)).squeeze(2)
    assert (at >= ctx64.max(2)[0] - 1e-5 * ctx64.abs().max()).all()


def test_scores_of_plus_minus_100_against_float64():
    """q scaled so that the largest |score| is 100.  Judged against float64 alone, by max(5e-6, 3 x err_torch): at |score| = 100 one ulp
    of a score is 7.6e-6, which moves its exponential by 7.6e-6 of itself, and the kernel and the f32 torch formulation sum the 64
    products of a score in different orders -- so two correct f32 evaluations differ from EACH OTHER by more than the pairwise
    instrument's 1e-5 of the element, while each stays as close to float64 as the other."""
    shape = (2, 40, 40, 8, 2, 2)
    B, N, NK, k, H, G = shape
    C = 64 * H
    x = list(_operands(*shape, seed=5))
    q, idx, PK, PV, bk, bv, idx3, w3, w = x
    flat = idx3.long().reshape(B, G, N * k * 3, 1).expand(-1, -1, -1, C)
    key = (torch.gather(PK.double(), 2, flat).view(B, G, N * k, 3, C) * w3.double().unsqueeze(-1)).sum((1, 3)) + bk.double()
    Q = torch.gather(q.double(), 1, idx.reshape(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, H, 64)
    s = torch.einsum('bnthc,bnshc->bnhts', Q, key.view(B, N, k, H, 64)) * SCALE
    x[0] = q * (100.0 / s.abs().max().item())
    s = s * (100.0 / s.abs().max().item())
    print("scores: min %.1f max %.1f" % (s.min().item(), s.max().item()))
    assert s.abs().max().item() >= 99.9 and s.min().item() < -50 and s.max().item() > 50
    x = tuple(x)
    for deterministic in (False, True):
        got, arg, _ = _kernels(x, H, deterministic)
        t32, _ = _formulation(x, H, torch.float32, arg)
        f64, _ = _formulation(x, H, torch.float64, arg)
        _judge(got, t32, f64, k, pairwise=False)


# ---- b. the deterministic form ------------------------------------------------------------------------------------------------------------
def _np(*ts):
    return [t.detach().cpu().numpy() for t in ts]


@pytest.mark.parametrize("shape, one_point", [((1, 1, 1, 1, 1, 1), False), ((2, 5, 7, 3, 2, 1), False), ((2, 40, 40, 8, 2, 2), False),
                                              ((1, 65, 130, 32, 6, 2), False), ((1, 3, 4, 10, 4, 4), False), ((2, 40, 6, 4, 2, 2), True)])
def test_det_scatters_have_the_bits_of_the_stated_order(shape, one_point):
    x = _operands(*shape, seed=3, one_point=one_point)
    B, N, NK, k, H, G = shape
    got, arg, rows = _kernels(x, H, True)
    again, _, rows2 = _kernels(x, H, True)
    assert all(torch.equal(a, b) for a, b in zip(got, again)) and torch.equal(rows, rows2)
    assert rows.shape == (3, B, N, k, 64 * H) and torch.isfinite(rows).all()
    want = scatter_det(*_np(rows, x[1], x[6], x[7]), NK)
    for name, a, b in zip(("d_q", "d_PK", "d_PV"), got[1:4], want):
        assert np.array_equal(a.cpu().numpy(), b), name
    if one_point:
        rev = scatter_det(*_np(rows, x[1], x[6], x[7]), NK, reverse=True)
        assert not np.array_equal(rev[2], want[2])                              # the order matters on this input, so the equality above says something
        assert not got[3][:, :, :NK // 2].any() and not got[3][:, :, NK // 2 + 1:].any()
    atomic, _, _ = _kernels(x, H, False)
    assert torch.equal(atomic[0], got[0]) and torch.equal(atomic[4], got[4]) and torch.equal(atomic[5], got[5])
    for name, a, b in zip(("d_q", "d_PK", "d_PV"), atomic[1:4], want):
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=0, atol=5e-6 * max(np.abs(b).max(), 1e-30), err_msg=name)


def test_every_sample_alone_equals_its_slice_of_the_batch():
    shape = (2, 40, 40, 8, 2, 2)
    x = _operands(*shape, seed=5)
    whole, arg, rows = _kernels(x, shape[4], True)
    for b in range(shape[0]):
        one = tuple(t[b:b + 1].contiguous() if t.dim() > 1 else t for t in x)
        got, arg1, rows1 = _kernels(one, shape[4], True)
        assert torch.equal(arg1, arg[b:b + 1]) and torch.equal(rows1, rows[:, b:b + 1])
        for name, a, w_ in zip(NAMES[:4], got[:4], whole[:4]):
            assert torch.equal(a, w_[b:b + 1]), (b, name)


def test_the_mode_is_read_when_the_backward_runs_and_the_call_overrides_it(monkeypatch):
    x = _operands(2, 5, 7, 3, 2, 1)
    seen, real = [], ops.region_attn_bwd

    def spy(*a, **k):
        seen.append(k["deterministic"])
        return real(*a, **k)

    monkeypatch.setattr(ops, "region_attn_bwd", spy)
    for per_call, flag, want in [(None, False, False), (None, True, True), (True, False, True), (False, True, False)]:
        q = x[0].clone().requires_grad_()
        out = HF.region_attention(q, *x[1:8], 2, SCALE, deterministic=per_call)      # forward outside the block, backward inside
        with HF.deterministic(flag):
            out.backward(x[8])
        assert seen[-1] is want, (per_call, flag)
        assert torch.isfinite(q.grad).all()


# ---- c. poisoned outputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 2, 1), (1, 3, 4, 10, 4, 4)])
@pytest.mark.parametrize("deterministic", [False, True])
def test_outputs_poisoned_with_nan_hold_no_poison_afterwards(shape, deterministic):
    B, N, NK, k, H, G = shape
    C = 64 * H
    q, idx, PK, PV, bk, bv, idx3, w3, w = _operands(*shape, seed=9)
    nan = lambda *s: torch.full(s, float("nan"), device='cuda')
    out, d_q, d_PK, d_PV, d_krow, d_vrow = nan(B, N, C), nan(B, N, C), nan(B, G, NK, C), nan(B, G, NK, C), nan(B, N, C), nan(B, N, C)
    rows = nan(3, B, N, k, C)
    arg = torch.full((B, N, C), 0xFF, dtype=torch.uint8, device='cuda')
    ptr = _abi.ptr
    ops._call(q.device, "upp_region_attn_fwd", ptr(q), ptr(idx), ptr(PK), ptr(PV), ptr(bk), ptr(bv), ptr(idx3), ptr(w3), ptr(out), ptr(arg),
              SCALE, B, N, NK, k, H, G)
    assert torch.isfinite(out).all() and int(arg.max()) < k
    head = (ptr(q), ptr(idx), ptr(PK), ptr(PV), ptr(bk), ptr(bv), ptr(idx3), ptr(w3), ptr(arg), ptr(w), ptr(d_q), ptr(d_PK), ptr(d_PV),
            ptr(d_krow), ptr(d_vrow))
    if deterministic:
        ops._call(q.device, "upp_region_attn_bwd_det", *head, ptr(rows), SCALE, B, N, NK, k, H, G)
        assert torch.isfinite(rows).all()
    else:
        ops._call(q.device, "upp_region_attn_bwd", *head, SCALE, B, N, NK, k, H, G)
    for name, t in (("d_q", d_q), ("d_PK", d_PK), ("d_PV", d_PV), ("d_krow", d_krow), ("d_vrow", d_vrow)):
        assert torch.isfinite(t).all(), name
    want, _, _ = _kernels((q, idx, PK, PV, bk, bv, idx3, w3, w), H, deterministic)
    assert torch.equal(out, want[0])
    for a, b in zip((d_q, d_PK, d_PV), want[1:4]):
        if deterministic:
            assert torch.equal(a, b)
        else:
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=5e-6 * b.abs().max().item())


def test_indices_outside_their_range_read_as_absent_and_get_no_gradient():
    shape = (2, 5, 7, 3, 2, 1)
    B, N, NK, k, H, G = shape
    q, idx, PK, PV, bk, bv, idx3, w3, w = _operands(*shape, seed=11)
    idx, idx3 = idx.clone(), idx3.clone()
    idx[0, 1, 2], idx[1, 0, 0], idx[1, 4, 1] = N, -1, 2 ** 40
    flat = idx3.view(-1)
    flat[0::5], flat[1::7], flat[2::11] = -1, NK, 2 ** 31 - 1
    x = (q, idx, PK, PV, bk, bv, idx3, w3, w)
    for deterministic in (False, True):
        got, arg, _ = _kernels(x, H, deterministic)
        t32, _ = _formulation(x, H, torch.float32, arg)
        f64, _ = _formulation(x, H, torch.float64, arg)
        _judge(got, t32, f64, k)


# ---- d. graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
def test_forward_and_backward_replay_from_a_graph(deterministic):
    shape = (2, 40, 40, 8, 2, 2)
    st = [t.clone() for t in _operands(*shape)]
    leaves = [st[i].requires_grad_() for i in (0, 2, 3, 4, 5)]

    def step():
        out = HF.region_attention(st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], shape[4], SCALE, deterministic=deterministic)
        return (out,) + torch.autograd.grad(out, leaves, st[8])

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
        for name, a, b in zip(NAMES, got, want):
            if not deterministic and name in ("d_q", "d_PK", "d_PV"):
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=5e-6 * b.abs().max().item(), err_msg=name)
            else:
                assert torch.equal(a, b), (seed, name)


# ---- e. memory ----------------------------------------------------------------------------------------------------------------------------
def test_fused_path_keeps_no_neighbourhood_tensor(monkeypatch):
    """(B,N,NK,k,H,G) = (2,512,512,16,2,2), default (atomic) mode: one (B,N,k,C) f32 tensor is 8 MB.  The module's fused forward +
    backward rises by less than one of them above its operands and results (arg is 1 / 64 of it); the torch formulation's
    figure is printed beside it, not gated.  The node keeps no (B,N,H,k,k) probabilities either (they would be k / 64 of it): the
    backward forms them again."""
    B, N, k, H, G = 2, 512, 16, 2, 2
    C = 64 * H
    unit = B * N * k * C * 4
    m = _seeded.fill(Transformer_utils.DeformableLocalAttention(C, num_heads=H, qkv_bias=True, k=k, n_group=G)).cuda()
    g = torch.Generator(device='cuda').manual_seed(1)
    x, w = (torch.randn(B, N, C, device='cuda', generator=g) for _ in range(2))
    pos = _seeded.unit_ball_clouds(B, N, seed=1).cuda()
    x.requires_grad_()
    wrt = [x] + [p for n, p in m.named_parameters() if not any(o in n for o in OFFSET_BRANCH)]
    idx = Transformer_utils.knn_point(k, pos, pos)

    def rise():
        def step():
            out = m(x, pos, idx=idx)
            return (out,) + torch.autograd.grad(out, wrt, w)
        step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base - sum(t.numel() * 4 for t in res)

    HF._declined.clear()
    with HF.deterministic(False):
        fused = rise()
    assert not HF._declined, HF._declined
    monkeypatch.setattr(m, "fusable", lambda q, v: False)
    plain = rise()
    HF._declined.clear()
    print("peak rise above operands and results: fused %.2f MB, torch formulation %.2f MB ((B,N,k,C) = %.0f MB)"
          % (fused / 2 ** 20, plain / 2 ** 20, unit / 2 ** 20))
    assert fused < unit, fused


# ---- f. the module ------------------------------------------------------------------------------------------------------------------------
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
    of every max over the context rows), or replay them into another evaluation of the same module made of torch operators; the
    replayed distances are recomputed from the replayed indices in the precision of the run.  Patches the names the module code calls,
    as tests/test_gpu_deform_graph.py's instrument does."""

    def __init__(self, monkeypatch, items=None):
        self.m, self.items, self.replay, self.pos = monkeypatch, ([] if items is None else items), items is not None, 0

    def get(self, tag):
        got, val = self.items[self.pos]
        assert got == tag, (self.pos, got, tag)
        self.pos += 1
        return val

    def install(self):
        knn, three, fwd, plain = HF.knn_query, Transformer_utils.shifted_three_nn, ops.region_attn_fwd, torch_cpu.region_attention

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

        def region_attn_fwd(*a, **k):
            r = fwd(*a, **k)
            self.items.append(("max", r[1].clone()))
            return r

        def region_attention(q, idx, PK, PV, bk, bv, idx3, w3, num_heads, scale, drop=None, pool=None):
            if not self.replay:
                box = []

                def pick(y):
                    val, arg = y.max(dim=2)
                    box.append(arg)
                    return val
                out = plain(q, idx, PK, PV, bk, bv, idx3, w3, num_heads, scale, drop, pick)
                self.items.append(("max", box[0]))
                return out
            arg = self.get("max")
            return plain(q, idx, PK, PV, bk, bv, idx3, w3, num_heads, scale, drop, lambda y: y.gather(2, arg.long().unsqueeze(2)).squeeze(2))

        self.m.setattr(HF, "knn_query", knn_query)
        self.m.setattr(Transformer_utils, "shifted_three_nn", shifted_three_nn)
        if not self.replay:
            self.m.setattr(ops, "region_attn_fwd", region_attn_fwd)
        self.m.setattr(torch_cpu, "region_attention", region_attention)


@pytest.mark.parametrize("name", ["a", "b"])
def test_module_gradients_against_float64_on_the_same_choices(monkeypatch, fixture, name):
    """The fused f32 run and the torch-formulation f32 run each record their discrete choices; the module in float64 is evaluated on the
    recorded choices of each.  The output and every gradient (input and parameters) of the fused run must be within
    max(5e-6, 3 x err_torch) of its float64 evaluation, relative to that tensor's maximum, err_torch being the torch formulation's own
    f32-against-f64 error of the same tensor.  The offset branch and the positions have no gradient in any run."""
    model = case.module(AdaPoinTr, Transformer_utils, name).cuda()
    model64 = copy.deepcopy(model).double()
    x = [t.cuda() for t in case.inputs(int(fixture["seed_" + name]))]
    w = torch.randn(x[0].shape, generator=torch.Generator().manual_seed(3)).cuda()
    region = [mod for mod in model.modules() if isinstance(mod, Transformer_utils.DeformableLocalAttention)]
    assert len(region) == 1

    def run(net, dtype):
        net.zero_grad(set_to_none=True)
        t, pos = (v.to(dtype).clone().requires_grad_() for v in x)
        out = case.run(net, name, t, pos)
        (out * w.to(dtype)).sum().backward()
        assert pos.grad is None
        for n, p in net.named_parameters():
            assert (p.grad is None) == any(o in n for o in OFFSET_BRANCH), n
        return [("forward", out.detach()), ("d_x", t.grad)] + [(n + ".grad", p.grad.clone()) for n, p in net.named_parameters() if p.grad is not None]

    def with_float64(fused):
        HF._declined.clear()
        with monkeypatch.context() as m:
            if not fused:
                for mod in region:
                    m.setattr(mod, "fusable", lambda q, v: False)
            rec = Choices(m)
            rec.install()
            f32 = run(model, torch.float32)
        assert fused == (not any(what.startswith("DeformableLocalAttention") for what, _ in HF._declined)), HF._declined
        with monkeypatch.context() as m:
            rep = Choices(m, rec.items)
            rep.install()
            f64 = run(model64, torch.float64)
        assert rep.pos == len(rec.items) > 0 and sum(tag == "max" for tag, _ in rec.items) == len(region)
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
    assert all("proj_k.bias" in n for n in zeros), zeros
    assert not failures, failures


def test_fused_module_launches_no_library_gemm_softmax_sort_or_gather(fixture):
    m = case.module(AdaPoinTr, Transformer_utils, "a").cuda()
    x, pos = (t.cuda() for t in case.inputs(int(fixture["seed_a"])))
    x.requires_grad_()
    w = torch.randn(x.shape, device='cuda')

    def run():
        m.zero_grad(set_to_none=True)
        x.grad = None
        (case.run(m, "a", x, pos) * w).sum().backward()

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
    for frag in ("da_offset_kernel", "ra_fwd_kernel", "ra_bwd_kernel", "three_nn"):
        assert any(frag in n for n in names), frag
    for pname, prm in m.named_parameters():
        assert (prm.grad is None) == any(o in pname for o in OFFSET_BRANCH), pname


def test_head_dim_32_runs_the_torch_formulation_and_names_the_site():
    m = _seeded.fill(Transformer_utils.DeformableLocalAttention(case.DIM, num_heads=4, qkv_bias=True, k=case.K, n_group=2)).cuda().eval()
    x, pos = (t.cuda() for t in case.inputs(1))
    HF._declined.clear()
    with torch.no_grad():
        got = m(x, pos)
    sites = [what for what, why in HF._declined if what.startswith("DeformableLocalAttention")]
    assert len(sites) == 1 and "4 heads" in sites[0], HF._declined
    HF._declined.clear()
    assert got.shape == x.shape and torch.isfinite(got).all()


# ---- g. the wiring ------------------------------------------------------------------------------------------------------------------------
def test_adapointr_with_rw_deform_blocks_trains_on_the_fused_path(monkeypatch):
    import _adapointr_model_case as mc
    from utils import misc
    from utils.config import EasyDict
    cfg = mc.config()
    cfg['region_wise'] = True
    cfg['encoder_config']['block_style_list'] = ['attn-rw_deform', 'attn']
    monkeypatch.setattr(misc, "jitter_points", mc.jitter(0))
    model = _seeded.fill(AdaPoinTr.from_cfg(EasyDict(cfg))).cuda().train()
    model.load_state_dict({k: t.clone() for k, t in model.state_dict().items()}, strict=True)
    assert isinstance(model.base_model.encoder.blocks.blocks[0].local_attn, Transformer_utils.DeformableLocalAttention)
    x, gt = (t.cuda() for t in mc.inputs(0))
    HF._declined.clear()
    ret = model(x)
    loss_denoised, loss_recon = model.get_loss(ret, gt)
    (loss_denoised + loss_recon).backward()
    assert not HF._declined, HF._declined
    assert all(torch.isfinite(t).all() for t in ret) and torch.isfinite(loss_denoised) and torch.isfinite(loss_recon)
    region = "base_model.encoder.blocks.blocks.0.local_attn."
    for n, p in model.named_parameters():
        if n.startswith(region):
            assert (p.grad is None) == any(o in n for o in OFFSET_BRANCH), n
            assert p.grad is None or torch.isfinite(p.grad).all(), n
