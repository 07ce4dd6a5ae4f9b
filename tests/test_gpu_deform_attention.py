"""The deformable local cross-attention on the GPU (include/upp_hip.h "deformable local cross-attention", csrc/deform_attn.hip): the two
operators against the float64 torch formulation on the same idx3 / w3 (tests/_attention_reference.py's instruments: the torch f32
formulation is held to the project's bound first, the kernels to 2 x e_torch + atol where it is not), the softmax hazard, bit identity,
the deterministic mode against a numpy restatement of its order (tests/_deform_attn_reference.py), graph capture, memory, the module on
the fixture cases of tests/golden/deform_attn.npz with its gradients against float64 on the same discrete choices, its launches, the
declined list, and the opt-in wiring into AdaPoinTr.

d_bk is zero in exact arithmetic (a key bias shifts a whole score row, which the softmax does not see): its own maximum is no scale, so
its errors are taken relative to max|d_PK| -- the same d_key terms, weighted by w3 -- under the float64 arbitration; in the module test
proj_k.bias.grad is taken relative to proj_k.weight.grad, as tests/test_gpu_pointr.py does for its zero-gradient biases.

Measured on MI355X.  Operators at (1,65,130,32,6,2), kernel / torch f32 of the float64 maximum: ctx 2.3e-7 / 2.2e-7, d_q 1.0e-6 / 1.3e-6,
d_PK 3.8e-7 / 3.0e-7, d_PV 2.7e-7 / 2.6e-7, d_bv 5.3e-8 / 9.9e-8, d_bk 3.1e-6 / 5.4e-6 of max|d_PK|; shift 1.2e-7 / 2.4e-7.  Scores of
+-100: ctx 8.7e-7 / 1.0e-6, d_q 3.9e-6 / 2.4e-6, d_PK 5.1e-6 / 3.2e-6 (float64 arbitration).  Fixture (bound 1e-5): a 2.5e-7, b 4.2e-7,
c 1.8e-7, d 2.1e-7.  Memory at (2,512,512,16,2,2): fused 7.1 MB, torch formulation 139.7 MB above operands and results."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import _deform_attn_case as case
import _seeded
from _attention_reference import _check_against, _err, _memsets
from _deform_attn_reference import scatter_det
from conftest import GOLDEN
from models import AdaPoinTr, Transformer_utils
from upp_hip import functional as HF, ops, torch_cpu

pytestmark = pytest.mark.gpu

NAMES = ("ctx", "d_q", "d_PK", "d_PV", "d_bk", "d_bv")
SHAPES = [(1, 1, 1, 1, 1, 1), (2, 5, 7, 3, 2, 1), (2, 40, 24, 8, 2, 2), (1, 65, 130, 32, 6, 2), (1, 3, 4, 10, 4, 4)]
OFFSET_BRANCH = ("proj_v_off.", "linear_offset.")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "deform_attn.npz"))


def _operands(B, N, NK, k, H, G, seed=0, one_point=False):
    """q, PK, PV, bk, bv, idx3, w3, cotangent.  idx3 / w3 as three_nn and the reference's weight formula leave them: three distinct points
    per row, weights that sum to 1; with NK < 3 the missing slots are index 0 with weight 0."""
    g = torch.Generator(device='cuda').manual_seed(seed + 7919 * N + 101 * NK + 13 * k + H)
    C = 64 * H
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)
    q, PK, PV, bk, bv, w = rnd(B, N, C), rnd(B, G, NK, C), rnd(B, G, NK, C), rnd(C), rnd(C), rnd(B, N, C)
    idx3 = torch.rand(B, G, N * k, NK, device='cuda', generator=g).argsort(-1)[..., :3]
    w3 = torch.rand(B, G, N * k, 3, device='cuda', generator=g) + 0.05
    if NK < 3:
        idx3 = torch.cat([idx3, idx3.new_zeros(B, G, N * k, 3 - NK)], -1)
        w3[..., NK:] = 0
    if one_point:
        idx3 = torch.full_like(idx3, NK // 2)
    return q, PK, PV, bk, bv, idx3.int().contiguous(), (w3 / w3.sum(-1, keepdim=True)).contiguous(), w


def _torch_formulation(ops_, H, dtype):
    q, PK, PV, bk, bv, idx3, w3, w = ops_
    x = [t.detach().to(dtype).requires_grad_(True) for t in (q, PK, PV, bk, bv)]
    ctx = torch_cpu.deform_attention(*x, idx3, w3.to(dtype), H, 0.125)
    (ctx * w.to(dtype)).sum().backward()
    return (ctx.detach(),) + tuple(t.grad for t in x)


def _kernels(ops_, H, deterministic=None, bias=True):
    q, PK, PV, bk, bv, idx3, w3, w = ops_
    x = [t.detach().clone().requires_grad_(True) for t in (q, PK, PV, bk, bv)]
    ctx = HF.deform_attention(x[0], x[1], x[2], x[3] if bias else None, x[4] if bias else None, idx3, w3, H, 0.125, deterministic=deterministic)
    ctx.backward(w)
    return (ctx.detach(),) + tuple(t.grad for t in x)


@functools.lru_cache(maxsize=None)
def _case(shape):
    x = _operands(*shape)
    return x, _torch_formulation(x, shape[4], torch.float32), _torch_formulation(x, shape[4], torch.float64)


def _judge(got, t32, f64):
    for i, name in enumerate(NAMES):
        assert torch.isfinite(got[i]).all(), name
        if name == "d_bk":
            unit = f64[2].abs().max().item()
            e_k, e_t = ((got[i].double() - f64[i]).abs().max().item() / unit, (t32[i].double() - f64[i]).abs().max().item() / unit)
            print("d_bk: kernel %.2e torch_f32 %.2e of max|d_PK f64| (float64 arbitration; max|d_bk f64| = %.1e)"
                  % (e_k, e_t, f64[i].abs().max().item()))
            assert e_k <= 2 * e_t + 2e-6, (name, e_k, e_t)
        else:
            _check_against(name, got[i], t32[i], f64[i], 1e-5, 2e-6)


# ---- a. operator parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("deterministic", [False, True])
def test_attention_parity_with_the_torch_formulation_and_float64(shape, deterministic):
    x, t32, f64 = _case(shape)
    got = _kernels(x, shape[4], deterministic)
    print("B, N, NK, k, H, G = %s, deterministic %s" % (shape, deterministic))
    if shape[3] == 1:
        # one slot: p = 1 and ds = p (dp - p dp) = 0 exactly, whatever dp is -- and with it d_q, d_key (so d_PK) and d_bk
        assert not got[1].any() and not got[2].any() and not got[4].any()
        got, t32, f64 = (tuple(t for i, t in enumerate(r) if i not in (1, 2, 4)) for r in (got, t32, f64))
        for i, name in enumerate(("ctx", "d_PV", "d_bv")):
            _check_against(name, got[i], t32[i], f64[i], 1e-5, 2e-6)
        return
    _judge(got, t32, f64)


def _offset_operands(B, N, NK, k, H, G, seed=0, constant=False):
    g = torch.Generator(device='cuda').manual_seed(seed + 31 * N + NK)
    C = 64 * H
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)
    A, Bq, pos, gamma, beta, W3 = rnd(B, G, NK, C), rnd(B, G, N, C), rnd(B, NK, 3), rnd(C), rnd(C), rnd(3, C) * C ** -0.5
    if constant:
        A, Bq = torch.full_like(A, 0.5), torch.full_like(Bq, -1.25)
    idx = torch.randint(0, NK, (B, N, k), device='cuda', generator=g)
    return A, Bq, idx, pos, gamma, beta, 1e-5, W3


@pytest.mark.parametrize("shape", SHAPES)
def test_offset_parity_with_float64(shape):
    x = _offset_operands(*shape)
    got = HF.deform_offset(*x)
    t32 = torch_cpu.deform_offset(*x)
    f64 = torch_cpu.deform_offset(*(t.double() if isinstance(t, torch.Tensor) and t.is_floating_point() else t for t in x))
    e_k, e_t = _err(got, f64), _err(t32, f64)
    print("%s shift: kernel %.2e torch_f32 %.2e of max|f64|" % (shape, e_k, e_t))
    assert got.shape == (shape[0], shape[5], shape[1] * shape[3], 3) and torch.isfinite(got).all()
    assert e_k <= 2e-6 + 2 * e_t, (e_k, e_t)


def test_offset_of_constant_rows_is_finite():
    """variance 0: LayerNorm gives beta, whatever 0 * rstd rounds to"""
    x = _offset_operands(2, 5, 7, 3, 2, 1, constant=True)
    got = HF.deform_offset(*x)
    f64 = torch_cpu.deform_offset(*(t.double() if isinstance(t, torch.Tensor) and t.is_floating_point() else t for t in x))
    assert torch.isfinite(got).all() and _err(got, f64) <= 2e-6 + 2 * _err(torch_cpu.deform_offset(*x), f64)


# ---- b. the softmax hazard ----------------------------------------------------------------------------------------------------------------
def test_scores_of_plus_minus_100_against_float64():
    shape = (2, 40, 24, 8, 2, 2)
    x = list(_operands(*shape, seed=5))
    H = shape[4]
    # the key rows in float64: scale q so that the largest |score| is 100
    B, N, NK, k, _, G = shape
    C = 64 * H
    flat = x[5].long().reshape(B, G, N * k * 3, 1).expand(-1, -1, -1, C)
    rows = (torch.gather(x[1].double(), 2, flat).view(B, G, N * k, 3, C) * x[6].double().unsqueeze(-1)).sum((1, 3)) + x[3].double()
    s = (x[0].double().view(B, N, 1, H, 64) * rows.view(B, N, k, H, 64)).sum(-1) * 0.125
    x[0] = x[0] * (100.0 / s.abs().max().item())
    s = s * (100.0 / s.abs().max().item())
    print("scores: min %.1f max %.1f" % (s.min().item(), s.max().item()))
    assert s.abs().max().item() >= 99.9 and s.min().item() < -50 and s.max().item() > 50
    x = tuple(x)
    _judge(_kernels(x, H), _torch_formulation(x, H, torch.float32), _torch_formulation(x, H, torch.float64))


# ---- c. bit identity ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_every_sample_alone_and_a_null_bias_give_the_same_bits():
    shape = (2, 40, 24, 8, 2, 2)
    x = _operands(*shape, seed=2)
    H = shape[4]
    a, b = _kernels(x, H), _kernels(x, H)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                        # ctx, d_q
    xo = _offset_operands(*shape, seed=2)
    s1, s2 = HF.deform_offset(*xo), HF.deform_offset(*xo)
    assert torch.equal(s1, s2)
    for i in range(shape[0]):
        one = tuple(t[i:i + 1].contiguous() if t.dim() > 1 else t for t in x)
        got = _kernels(one, H)
        assert torch.equal(got[0], a[0][i:i + 1]) and torch.equal(got[1], a[1][i:i + 1]), i
        oo = tuple(t[i:i + 1].contiguous() if isinstance(t, torch.Tensor) and t.dim() > 2 else t for t in xo)
        assert torch.equal(HF.deform_offset(*oo), s1[i:i + 1]), i
    zero = x[:3] + (torch.zeros_like(x[3]), torch.zeros_like(x[4])) + x[5:]
    with_zero, without = _kernels(zero, H, deterministic=True), _kernels(x, H, deterministic=True, bias=False)
    for i in range(4):
        assert torch.equal(with_zero[i], without[i]), NAMES[i]


# ---- d. the deterministic mode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, one_point", [((2, 5, 7, 3, 2, 1), False), ((2, 40, 24, 8, 2, 2), False), ((1, 3, 4, 10, 4, 4), False),
                                              ((2, 9, 6, 4, 2, 2), True), ((1, 1, 1, 1, 1, 1), False)])
def test_det_scatter_has_the_bits_of_the_stated_order(shape, one_point):
    q, PK, PV, bk, bv, idx3, w3, w = _operands(*shape, seed=3, one_point=one_point)
    H, NK = shape[4], shape[2]
    ctx, p = ops.deform_attn_fwd(q, PK, PV, bk, bv, idx3, w3, H, 0.125)
    d_q, d_PK, d_PV, ds, _ = ops.deform_attn_bwd(q, PK, PV, bk, bv, idx3, w3, p, w, H, 0.125, deterministic=True)
    again = ops.deform_attn_bwd(q, PK, PV, bk, bv, idx3, w3, p, w, H, 0.125, deterministic=True)
    assert torch.equal(d_PK, again[1]) and torch.equal(d_PV, again[2]) and torch.equal(d_q, again[0])
    args = [t.cpu().numpy() for t in (q, w, p, ds, idx3, w3)]
    want_K, want_V = scatter_det(*args, 0.125, NK)
    assert np.array_equal(d_PK.cpu().numpy(), want_K) and np.array_equal(d_PV.cpu().numpy(), want_V)
    if one_point:
        rev_K, _ = scatter_det(*args, 0.125, NK, reverse=True)
        assert not np.array_equal(rev_K, want_K)                    # the order matters on this input, so the equality above says something
        assert not d_PK[:, :, :NK // 2].any() and not d_PK[:, :, NK // 2 + 1:].any()
    atomic = ops.deform_attn_bwd(q, PK, PV, bk, bv, idx3, w3, p, w, H, 0.125, deterministic=False)
    assert torch.equal(atomic[0], d_q) and torch.equal(atomic[3], ds)
    np.testing.assert_allclose(atomic[1].cpu().numpy(), want_K, rtol=1e-5, atol=2e-6 * np.abs(want_K).max())


def test_the_mode_is_read_when_the_backward_runs_and_the_call_overrides_it(monkeypatch):
    x = _operands(2, 5, 7, 3, 2, 1)
    seen, real = [], ops.deform_attn_bwd

    def spy(*a, **k):
        seen.append(k["deterministic"])
        return real(*a, **k)

    monkeypatch.setattr(ops, "deform_attn_bwd", spy)
    for per_call, flag, want in [(None, False, False), (None, True, True), (True, False, True), (False, True, False)]:
        q = x[0].clone().requires_grad_()
        out = HF.deform_attention(q, *x[1:7], 2, 0.125, deterministic=per_call)       # forward outside the block, backward inside
        with HF.deterministic(flag):
            out.backward(x[7])
        assert seen[-1] is want, (per_call, flag)


# ---- e. graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
def test_forward_and_backward_replay_from_a_graph(deterministic):
    shape = (2, 40, 24, 8, 2, 2)
    H = shape[4]
    st = [t.clone() for t in _operands(*shape)]
    leaves = [t.requires_grad_() for t in st[:5]]

    def step():
        out = HF.deform_attention(*leaves, st[5], st[6], H, 0.125, deterministic=deterministic)
        return (out,) + torch.autograd.grad(out, leaves, st[7])

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
            if not deterministic and name in ("d_PK", "d_PV"):
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-5, atol=2e-6 * b.abs().max().item())
            else:
                assert torch.equal(a, b), (seed, name)


# ---- f. memory ----------------------------------------------------------------------------------------------------------------------------
def test_fused_path_keeps_no_neighbourhood_tensor_and_the_torch_formulation_does(monkeypatch):
    """(B,N,NK,k,H,G) = (2,512,512,16,2,2): one (B,N,k,C) f32 tensor is 8 MB.  The module's fused forward + backward may rise by less than
    two of them above its operands and results (its intermediates are about ten arrays of B N C G elements: 1.25 such tensors at k 16,
    G 2); the torch formulation, measured the same way, rises by at least four."""
    B, N, NK, k, H, G = 2, 512, 512, 16, 2, 2
    C, unit = 64 * H, 2 * 512 * 16 * 128 * 4
    m = _seeded.fill(Transformer_utils.DeformableLocalCrossAttention(C, num_heads=H, qkv_bias=True, k=k, n_group=G)).cuda()
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
    print("peak rise above operands and results: fused %.2f MB, torch formulation %.2f MB ((B,N,k,C) = %.0f MB)"
          % (fused / 2 ** 20, plain / 2 ** 20, unit / 2 ** 20))
    assert fused < 2 * unit, fused
    assert plain >= 4 * unit, plain


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
    """Record the discrete choices of one f32 forward (the neighbour lists and the three nearest points of every shifted position), or
    replay them into another evaluation of the same module; the replayed distances are recomputed from the replayed indices in the
    precision of the run."""

    def __init__(self, monkeypatch, items=None):
        self.m, self.items, self.replay, self.pos = monkeypatch, ([] if items is None else items), items is not None, 0

    def get(self, tag, device):
        got, val = self.items[self.pos]
        assert got == tag, (self.pos, got, tag)
        self.pos += 1
        return val.to(device)

    def install(self):
        knn, three = HF.knn_query, Transformer_utils.shifted_three_nn

        def knn_query(ref, query, k):
            if not self.replay:
                r = knn(ref, query, k)
                self.items.append(("knn", r[1].clone()))
                return r
            return None, self.get("knn", ref.device)

        def shifted_three_nn(shift, known):
            if not self.replay:
                r = three(shift, known)
                self.items.append(("three", r[1].clone()))
                return r
            idx3 = self.get("three", shift.device)
            near = torch.gather(known, 1, idx3.long().reshape(idx3.shape[0], -1, 1).expand(-1, -1, 3)).view(*idx3.shape, 3)
            return (shift.detach().unsqueeze(2) - near.detach()).pow(2).sum(-1).sqrt(), idx3

        self.m.setattr(HF, "knn_query", knn_query)
        self.m.setattr(Transformer_utils, "shifted_three_nn", shifted_three_nn)


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
    deform = [mod for mod in model.modules() if isinstance(mod, Transformer_utils.DeformableLocalCrossAttention)]

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
                for mod in deform:
                    m.setattr(mod, "fusable", lambda q, v: False)
            rec = Choices(m)
            rec.install()
            f32 = run(model, torch.float32)
        assert fused == (not any(what.startswith("DeformableLocalCrossAttention") for what, _ in HF._declined)), HF._declined
        with monkeypatch.context() as m:
            rep = Choices(m, rec.items)
            rep.install()
            f64 = run(model64, torch.float64)
        assert rep.pos == len(rec.items) > 0
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
        lim = max(5e-6, 3 * err_t)
        print("%s: fused against f64 %.3g, torch formulation against f64 %.3g, bound %.3g" % (n, err_f, err_t, lim))
        if not err_f <= lim:
            failures.append((n, err_f, err_t))
    print("exactly 0 in float64: %s" % zeros)
    assert all("proj_k.bias" in n or "k_map.bias" in n for n in zeros) and sum("proj_k.bias" in n for n in zeros) == len(deform)
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
    for frag in ("da_offset_kernel", "da_fwd_kernel", "da_bwd_kernel", "three_nn"):
        assert any(frag in n for n in names), frag


def test_head_dim_32_runs_the_torch_formulation_and_names_the_site():
    m = _seeded.fill(Transformer_utils.DeformableLocalCrossAttention(case.DIM, num_heads=4, qkv_bias=True, k=case.K, n_group=2)).cuda().eval()
    q, v, q_pos, v_pos = (t.cuda() for t in case.inputs(1))
    HF._declined.clear()
    with torch.no_grad():
        got = m(q, q_pos, v=v, v_pos=v_pos)
        f64 = copy.deepcopy(m).double()(q.double(), q_pos.double(), v=v.double(), v_pos=v_pos.double(),
                                         idx=Transformer_utils.knn_point(case.K, v_pos, q_pos))
    sites = [what for what, why in HF._declined if what.startswith("DeformableLocalCrossAttention")]
    assert len(sites) == 1 and "4 heads" in sites[0], HF._declined
    HF._declined.clear()
    assert got.shape == q.shape and _err(got, f64) <= 1e-5


# ---- h. the wiring ------------------------------------------------------------------------------------------------------------------------
def test_adapointr_with_deformable_blocks_trains_on_the_fused_path(monkeypatch):
    import _adapointr_model_case as mc
    from utils import misc
    from utils.config import EasyDict
    cfg = mc.config()
    cfg['deformable'] = True
    cfg['encoder_config']['block_style_list'] = ['attn-deform', 'attn']
    cfg['decoder_config']['self_attn_block_style_list'] = ['attn-deform', 'attn']
    cfg['decoder_config']['cross_attn_block_style_list'] = ['attn-deform', 'attn']
    monkeypatch.setattr(misc, "jitter_points", mc.jitter(0))
    model = _seeded.fill(AdaPoinTr.from_cfg(EasyDict(cfg))).cuda().train()
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
    assert sum("linear_offset" in n for n in without) == 3 * 5                       # three deformable modules, five offset-head tensors each
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
