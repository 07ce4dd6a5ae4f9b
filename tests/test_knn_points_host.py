"""The pytorch3d.ops surface, host side (no GPU): the package imports and has upstream's signature; CPU tensors are refused unless the
opt-in torch formulations are on, and those equal the numpy restatement (tests/_knn_points_reference.py) bit for bit on lattice inputs;
the five entry points validate their arguments before any launch; the `_det` restatement is right to rounding and sees order; the two
autograd nodes hand `deterministic` to upp_hip.ops exactly when the mode is on; the seeds of the random GPU cases satisfy their
precondition."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _knn_points_reference as R
from conftest import ROOT, PKG
from upp_hip import _abi, ops, torch_cpu
import upp_hip.functional as HF

P = ctypes.c_void_p(64)            # a non-NULL pointer that is never dereferenced: the checks below return before any launch
E, RANGE = -1, -2


def test_package_imports_without_a_gpu_and_has_upstreams_signature():
    out = subprocess.check_output([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import pytorch3d.ops as o; "
                                   "print(o.knn_points.__name__, o.knn_gather.__name__, 'torch.cuda' in sys.modules and "
                                   "__import__('torch').cuda.is_initialized())" % PKG],
                                  env={**os.environ, "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""}, text=True)
    assert out.split() == ["knn_points", "knn_gather", "False"]
    import pytorch3d.ops as P3
    sig = inspect.signature(P3.knn_points)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ("p1", inspect.Parameter.empty), ("p2", inspect.Parameter.empty), ("lengths1", None), ("lengths2", None), ("norm", 2), ("K", 1),
        ("version", -1), ("return_nn", False), ("return_sorted", True)]
    assert [(n, p.default) for n, p in inspect.signature(P3.knn_gather).parameters.items()] == [
        ("x", inspect.Parameter.empty), ("idx", inspect.Parameter.empty), ("lengths", None)]
    assert P3._KNN._fields == ("dists", "idx", "knn")
    assert "any order" in P3.knn_points.__doc__.lower() or "Any order" in P3.knn_points.__doc__


def test_cpu_tensors_are_refused_while_the_torch_formulations_are_off():
    import pytorch3d.ops as P3
    assert not torch_cpu.enabled()
    x, q = torch.rand(2, 16, 3), torch.rand(2, 4, 3)
    idx = torch.zeros(2, 4, 2, dtype=torch.int64)
    calls = [lambda: P3.knn_points(q, x, K=2), lambda: P3.knn_points(q, x, lengths2=[3, 4], K=2, return_nn=True),
             lambda: P3.knn_gather(x, idx), lambda: ops.knn_points(q, x, K=2), lambda: ops.knn_gather(x, idx),
             lambda: ops.knn_points_bwd(q, x, idx, torch.rand(2, 4, 2)), lambda: ops.knn_scatter_add(torch.rand(2, 4, 2, 3), idx, 16)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    # the argument errors come first, whatever the device
    with pytest.raises(ValueError):
        P3.knn_points(q, x, norm=3)
    with pytest.raises(ValueError):
        P3.knn_points(q, x[:1])
    with pytest.raises(ValueError):
        P3.knn_points(q, torch.rand(2, 16, 4))


@pytest.fixture
def cpu_on():
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    yield
    torch_cpu.enable(was)


HOST_CASES = [(3, 9, 40, 3, 4), (3, 5, 7, 5, 8), (3, 6, 65, 1, 3), (3, 4, 30, 32, 64), (3, 1, 1, 2, 1)]


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("case", HOST_CASES)
def test_torch_formulations_equal_the_restatement_on_lattice_inputs(cpu_on, case, norm):
    import pytorch3d.ops as P3
    N, P1, P2, D, K = case
    p1, p2 = R.lattice_case(N, P1, P2, D, seed=sum(case), span=3)         # 7 values per coordinate: ties and duplicates everywhere
    l1 = np.array([P1, max(P1 - 2, 0), P1 + 5], np.int64)
    l2 = np.array([0, max(1, min(K, P2) - 1), P2], np.int64)              # an empty cloud, one shorter than K
    for lengths1, lengths2 in ((None, None), (l1, l2)):
        wd, wi, wn = R.knn_points(p1, p2, lengths1, lengths2, norm, K)
        d64, i64, _ = R.knn_points(p1, p2, lengths1, lengths2, norm, K, dist=lambda q, p, n: R.distances64(q, p, n).astype(np.float32))
        assert np.array_equal(wi, i64) and np.array_equal(wd, d64)                          # lattice: every step is exact
        if P2 > 2 and K > 1 and lengths1 is None:
            kk = min(K, P2)                                                                 # (the filled slots)
            tie = np.zeros(wd[:, :, 1:].shape, bool)
            tie[:, :, :kk - 1] = wd[:, :, 1:kk] == wd[:, :, :kk - 1]
            assert tie.any()                                                                # ties are there, and broken by index
            assert (wi[:, :, 1:][tie] > wi[:, :, :-1][tie]).all()
        got = P3.knn_points(torch.from_numpy(p1), torch.from_numpy(p2), None if lengths1 is None else torch.from_numpy(lengths1),
                            None if lengths2 is None else lengths2.tolist(), norm=norm, K=K, return_nn=True)
        assert got.idx.dtype == torch.int64 and np.array_equal(got.idx.numpy(), wi)
        assert np.array_equal(got.dists.numpy().view(np.int32), wd.view(np.int32))
        assert np.array_equal(got.knn.numpy().view(np.int32), wn.view(np.int32))
        if lengths2 is not None:
            assert not wi[0].any() and not wd[0].any() and not wn[0].any()
            kk = int(min(K, l2[1]))
            assert not wd[1, :, kk:].any() and not wi[1, :, kk:].any() and not wn[1, l1[1]:].any()
        assert P3.knn_points(torch.from_numpy(p1), torch.from_numpy(p2), norm=norm, K=K).knn is None
        x = np.random.default_rng(1).standard_normal((N, P2, 6)).astype(np.float32)
        lens = None if lengths2 is None else lengths2
        assert np.array_equal(P3.knn_gather(torch.from_numpy(x), got.idx, None if lens is None else torch.from_numpy(lens)).numpy(),
                              R.knn_gather(x, wi, lens))


def test_torch_formulation_is_differentiable_where_the_header_says(cpu_on):
    import pytorch3d.ops as P3
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(2, 5, 3, generator=g, requires_grad=True), torch.rand(2, 9, 3, generator=g, requires_grad=True)
    out = P3.knn_points(a, b, lengths1=[5, 3], lengths2=[9, 2], K=4, return_nn=True)
    assert not out.idx.requires_grad
    ga, gb = torch.autograd.grad(out.dists.sum(), (a, b), retain_graph=True)
    assert ga[0].abs().sum() > 0 and not ga[1, 3:].any() and not gb[1, 2:].any()
    (gn,) = torch.autograd.grad(out.knn.sum(), b)
    assert gn[0].sum() == 5 * 4 * 3 and gn[1].sum() == 3 * 2 * 3
    x = torch.rand(2, 9, 4, requires_grad=True)
    (gx,) = torch.autograd.grad(P3.knn_gather(x, out.idx, [4, 1]).sum(), x)
    assert gx[0].sum() == 5 * 4 * 4 and gx[1].sum() == 5 * 1 * 4


def test_entry_points_validate_before_any_launch():
    lib = _abi.load()
    # upp_knn_points: (p1, p2, lengths1, lengths2, dists, idx, nn, N, P1, P2, D, K, norm, stream); lengths and nn may be NULL
    ok = (1, 8, 16, 3, 4, 2)
    assert lib.upp_knn_points(P, P, None, None, P, P, None, 0, 8, 16, 3, 4, 2, None) == 0
    for k in (0, 1, 4, 5):
        a = [None if i == k else P for i in range(7)]
        assert lib.upp_knn_points(*a, *ok, None) == E, k
    for dims in ((-1, 8, 16, 3, 4, 2), (1, 0, 16, 3, 4, 2), (1, 8, 0, 3, 4, 2), (1, 8, 16, 0, 4, 2), (1, 8, 16, 3, 0, 2), (1, 8, 16, 3, 4, 0),
                 (1, 8, 16, 3, 4, 3)):
        assert lib.upp_knn_points(*[P] * 7, *dims, None) == E, dims
    assert lib.upp_knn_points(*[P] * 7, 1, 8, 16, 33, 4, 2, None) == RANGE
    assert lib.upp_knn_points(*[P] * 7, 1, 8, 16, 3, 65, 2, None) == RANGE
    assert lib.upp_knn_points(*[P] * 7, 65536, 8, 16, 3, 4, 2, None) == RANGE
    # upp_knn_points_bwd: (p1, p2, idx, grad_dists, lengths1, lengths2, g_p1, t, N, P1, P2, D, K, norm, stream)
    assert lib.upp_knn_points_bwd(P, P, P, P, None, None, P, P, 0, 8, 16, 3, 4, 2, None) == 0
    for k in (0, 1, 2, 3, 6, 7):
        a = [None if i == k else P for i in range(8)]
        assert lib.upp_knn_points_bwd(*a, *ok, None) == E, k
    assert lib.upp_knn_points_bwd(*[P] * 8, 1, 8, 16, 3, 4, 5, None) == E
    assert lib.upp_knn_points_bwd(*[P] * 8, 1, 8, 16, 33, 4, 2, None) == RANGE
    assert lib.upp_knn_points_bwd(*[P] * 8, 1, 8, 16, 3, 65, 2, None) == RANGE
    # upp_knn_gather: (x, idx, lengths, out, N, M, L, K, U, stream)
    assert lib.upp_knn_gather(P, P, None, P, 0, 16, 8, 4, 3, None) == 0
    for k in (0, 1, 3):
        a = [None if i == k else P for i in range(4)]
        assert lib.upp_knn_gather(*a, 1, 16, 8, 4, 3, None) == E, k
    for dims in ((-1, 16, 8, 4, 3), (1, 0, 8, 4, 3), (1, 16, 0, 4, 3), (1, 16, 8, 0, 3), (1, 16, 8, 4, 0)):
        assert lib.upp_knn_gather(P, P, P, P, *dims, None) == E, dims
    assert lib.upp_knn_gather(P, P, P, P, 1, 16, 65536, 65536, 3, None) == RANGE
    # the scatter pair: (src, idx, rows, slots, out, N, M, L, K, U, negate, stream), the same argument list
    assert _abi.SIGNATURES["upp_knn_scatter_add_det"] == _abi.SIGNATURES["upp_knn_scatter_add"]
    for fn in (lib.upp_knn_scatter_add, lib.upp_knn_scatter_add_det):
        assert fn(P, P, None, None, P, 0, 16, 8, 4, 3, 0, None) == 0
        for k in (0, 1, 4):
            a = [None if i == k else P for i in range(5)]
            assert fn(*a, 1, 16, 8, 4, 3, 0, None) == E, k
        for dims in ((-1, 16, 8, 4, 3), (1, 0, 8, 4, 3), (1, 16, 0, 4, 3), (1, 16, 8, 0, 3), (1, 16, 8, 4, 0)):
            assert fn(P, P, P, P, P, *dims, 1, None) == E, dims
        assert fn(P, P, P, P, P, 1, 16, 65536, 65536, 3, 0, None) == RANGE
    # additions only
    hdr = open(os.path.join(ROOT, "include", "upp_hip.h")).read()
    assert "the pytorch3d.ops surface" in hdr and "UPP_OPT_COUNT = 4" in hdr and "#define UPP_ABI_VERSION 5" in hdr
    assert len(_abi.OPTIONS) == 4 and lib.upp_abi_version() == 5
    for name in ("upp_knn_points", "upp_knn_points_bwd", "upp_knn_gather", "upp_knn_scatter_add", "upp_knn_scatter_add_det"):
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)), name


def test_python_names_the_limit_and_does_not_fall_back(monkeypatch):
    """D = 33 / K = 65: the RuntimeError names the limit before any tensor reaches a kernel (checked on stand-ins that say they are HIP
    tensors; the GPU suite repeats it on real ones)."""
    monkeypatch.setattr(ops, "_need", lambda *a, **k: None)
    monkeypatch.setattr(ops, "_same_device", lambda *a: None)
    with pytest.raises(RuntimeError, match=r"1 <= D <= 32.*UPP_E_RANGE"):
        ops.knn_points(torch.rand(1, 4, 33), torch.rand(1, 4, 33), K=2)
    with pytest.raises(RuntimeError, match=r"1 <= K <= 64.*UPP_E_RANGE"):
        ops.knn_points(torch.rand(1, 4, 3), torch.rand(1, 4, 3), K=65)


def test_det_restatement_agrees_with_float64_and_sees_order():
    g = np.random.default_rng(5)
    src, idx = g.standard_normal((3, 20, 6, 5)).astype(np.float32), g.integers(0, 9, (3, 20, 6))
    rows, slots = np.array([20, 7, 0]), np.array([6, 2, 6])
    for r, s in ((None, None), (rows, slots)):
        total, bound = R.scatter_bound(src, idx, 11, r, s)
        for neg in (False, True):
            got = R.scatter_add_det(src, idx, 11, r, s, negate=neg)
            assert got.dtype == np.float32
            assert (np.abs(got - (-total if neg else total)) <= bound).all()       # (m + 2) 2^-24 sum |terms|, m terms per target
        assert not got[:, 9:].any() and not np.signbit(got[:, 9:]).any()           # rows nobody references: +0.0
    assert not R.scatter_add_det(src, idx, 11, rows, slots)[2].any()
    big = np.array([1e8, -1e8, 1.0], np.float32).reshape(1, 3, 1, 1)               # (1e8 - 1e8) + 1 = 1, (1 - 1e8) + 1e8 = 0
    zero = np.zeros((1, 3, 1), np.int64)
    assert R.scatter_add_det(big, zero, 2)[0, :, 0].tolist() == [1.0, 0.0]
    assert R.scatter_add_det(big, zero, 2, reverse=True)[0, :, 0].tolist() == [0.0, 0.0]
    assert R.scatter_add_det(big, zero, 2, negate=True)[0, 0, 0] == -1.0


def test_fma_emulation_rounds_once():
    """fma32 against exact rational arithmetic, including a sum that sits just off a float32 rounding midpoint -- where rounding the
    float64 sum a second time goes the wrong way."""
    from fractions import Fraction
    a = np.float32(1.0 + 2.0 ** -12)
    b = np.float32(1.0 + 2.0 ** -12)                     # a * b = 1 + 2^-11 + 2^-24: a midpoint of float32 once 2^-60-ish is added
    c = np.float32(2.0 ** -80)
    got = R.fma32(a, b, c)
    assert got == np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)                        # above the midpoint: up (a plain float64 sum says down)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(1.0 + 2.0 ** -11)
    assert R.fma32(a, b, -c) == np.float32(1.0 + 2.0 ** -11)
    g = np.random.default_rng(0)
    x, y, z = (g.standard_normal(400).astype(np.float32) for _ in range(3))
    for xi, yi, zi, ri in zip(x, y, z, R.fma32(x, y, z)):
        exact = Fraction(float(xi)) * Fraction(float(yi)) + Fraction(float(zi))
        lo, hi = np.nextafter(ri, np.float32(-np.inf)), np.nextafter(ri, np.float32(np.inf))
        assert abs(Fraction(float(ri)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))


@pytest.mark.parametrize("case", R.RANDOM_GRID)
def test_random_gpu_cases_satisfy_their_precondition(case):
    N, P1, P2, D, K, seed = case
    p1, p2 = R.random_case(N, P1, P2, D, seed)
    for norm in (1, 2):
        assert 1.0 - R.separated_queries(p1, p2, K, norm).mean() <= 0.01


def test_forward_grid_covers_what_it_must():
    grid = R.FORWARD_GRID
    assert {c[0] for c in grid} == {3} and {c[3] for c in grid} == {1, 3, 5, 32} and {c[1] for c in grid} == {1, 5, 72}
    assert {c[2] for c in grid} == {1, 63, 64, 65, 1000, 4097} and {c[4] for c in grid} == {1, 4, 64}
    assert any(c[4] > c[2] for c in grid) and (3, 5, 4097, 3, 4) in grid
    chunk32 = (12288 // 32) & ~63                        # csrc/knn_points.hip kp_chunk: points per LDS chunk at D = 32
    assert any(c[3] == 32 and c[2] % 64 and c[2] > 2 * chunk32 for c in grid)


class _Fake:
    """Stand-ins for the new upp_hip.ops entries: CPU tensors of the right shapes, and a record of the `deterministic` argument."""

    def __init__(self, monkeypatch):
        self.seen = []
        for name in ("knn_points", "knn_points_bwd", "knn_gather", "knn_scatter_add"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def knn_points(self, p1, p2, lengths1=None, lengths2=None, K=1, norm=2, want_nn=False):
        N, P1, D = p1.shape
        return torch.zeros(N, P1, K), torch.zeros(N, P1, K, dtype=torch.int64), (torch.zeros(N, P1, K, D) if want_nn else None)

    def knn_points_bwd(self, p1, p2, idx, g, lengths1=None, lengths2=None, norm=2):
        return torch.zeros_like(p1), torch.zeros(*idx.shape, p1.shape[2])

    def knn_gather(self, x, idx, lengths=None):
        return torch.zeros(*idx.shape, x.shape[2])

    def knn_scatter_add(self, src, idx, M, rows=None, slots=None, negate=False, **kw):
        self.seen.append(("knn_scatter_add", kw.get("deterministic", "absent")))
        return torch.zeros(src.shape[0], M, src.shape[3])


def _run_the_two_nodes():
    a, b = torch.rand(2, 5, 3, requires_grad=True), torch.rand(2, 9, 3, requires_grad=True)
    dists, idx, nn = HF.KnnPoints.apply(a, b, None, None, 4, 2, True)
    assert not idx.requires_grad
    (dists.sum() + nn.sum()).backward()                  # two scatters: the terms of dists, the gather of nn
    assert a.grad.shape == (2, 5, 3) and b.grad.shape == (2, 9, 3)
    x = torch.rand(2, 9, 4, requires_grad=True)
    HF.KnnGather.apply(x, idx, None).sum().backward()
    assert x.grad.shape == (2, 9, 4)


def test_the_two_new_nodes_pass_the_flag_exactly_when_the_mode_is_on(monkeypatch):
    fake = _Fake(monkeypatch)
    monkeypatch.setattr(HF, "DETERMINISTIC", False)
    _run_the_two_nodes()
    assert len(fake.seen) == 3 and all(flag is False for _, flag in fake.seen), fake.seen
    fake.seen.clear()
    with HF.deterministic():
        _run_the_two_nodes()
    assert fake.seen == [("knn_scatter_add", True)] * 3
    fake.seen.clear()
    _run_the_two_nodes()
    assert len(fake.seen) == 3 and all(flag is False for _, flag in fake.seen)
