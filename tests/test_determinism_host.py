"""The opt-in reproducible mode, host side (no GPU): the `_det` entry points are declared, bound and exported and validate their arguments
before any launch; the numpy restatements of the five defined orders (tests/_det_reference.py) are right to rounding AND sensitive to
order; functional.deterministic() / UPP_DETERMINISTIC=1 set the module attribute; each of the seven autograd nodes hands
`deterministic=True` to upp_hip.ops exactly when the mode is on."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _det_reference as R
from conftest import ROOT, PKG
from upp_hip import _abi, ops
import upp_hip.functional as HF

DET = ("upp_chamfer_bwd_det", "upp_group_bwd_det", "upp_gather_bwd_det", "upp_fps_gather_bwd_det", "upp_emd_matchcost_det",
       "upp_emd_matchcost_det_work_bytes")
P = ctypes.c_void_p(64)            # a non-NULL pointer that is never dereferenced: the checks below return before any launch


def test_det_symbols_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "upp_hip.h")).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH]).decode()
    for name in DET:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _abi.SIGNATURES, name
        assert re.search(r" T %s\b" % name, exported), name
    for name in DET[:5]:              # the same argument lists as the siblings (the EMD cost: + the scratch pointer)
        sib = _abi.SIGNATURES[name[:-4]]
        extra = 1 if name == "upp_emd_matchcost_det" else 0
        assert _abi.SIGNATURES[name][0] is sib[0] and len(_abi.SIGNATURES[name][1]) == len(sib[1]) + extra, name
    assert "UPP_OPT_COUNT = 4" in hdr and "#define UPP_ABI_VERSION 5" in hdr and len(_abi.OPTIONS) == 4


def test_det_entry_points_validate_before_any_launch():
    lib = _abi.load()
    E = -1
    # Chamfer: (xyz1, xyz2, idx1, idx2, gd1, gd2, g1, g2, B, n, m, stream)
    ok = [P] * 8
    assert lib.upp_chamfer_bwd_det(*ok, 0, 8, 8, None) == 0
    for k in range(8):
        assert lib.upp_chamfer_bwd_det(*[None if i == k else P for i in range(8)], 1, 8, 8, None) == E, k
    for dims in ((-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8)):
        assert lib.upp_chamfer_bwd_det(*ok, *dims, None) == E, dims
    # group: (grad_out, idx, grad_xyz, grad_center, B, N, G, K, stream); either gradient pointer may be NULL, as in upp_group_bwd
    assert lib.upp_group_bwd_det(P, P, P, P, 0, 8, 4, 4, None) == 0 and lib.upp_group_bwd_det(P, P, None, None, 0, 8, 4, 4, None) == 0
    assert lib.upp_group_bwd_det(None, P, P, P, 1, 8, 4, 4, None) == E and lib.upp_group_bwd_det(P, None, P, P, 1, 8, 4, 4, None) == E
    for dims in ((-1, 8, 4, 4), (1, 0, 4, 4), (1, 8, -1, 4), (1, 8, 4, -1)):
        assert lib.upp_group_bwd_det(P, P, P, P, *dims, None) == E, dims
    # gather: (grad_out, idx, grad_feat, B, C, N, M, stream)
    assert lib.upp_gather_bwd_det(P, P, P, 0, 3, 8, 4, None) == 0
    for k in range(3):
        assert lib.upp_gather_bwd_det(*[None if i == k else P for i in range(3)], 1, 3, 8, 4, None) == E, k
    for dims in ((-1, 3, 8, 4), (1, -1, 8, 4), (1, 3, 0, 4), (1, 3, 8, -1)):
        assert lib.upp_gather_bwd_det(P, P, P, *dims, None) == E, dims
    # FPS gather: (g_centers, idx, g_xyz, B, N, M, stream)
    assert lib.upp_fps_gather_bwd_det(P, P, P, 0, 8, 4, None) == 0
    for k in range(3):
        assert lib.upp_fps_gather_bwd_det(*[None if i == k else P for i in range(3)], 1, 8, 4, None) == E, k
    for dims in ((-1, 8, 4), (1, 0, 4), (1, 8, -1)):
        assert lib.upp_fps_gather_bwd_det(P, P, P, *dims, None) == E, dims
    # EMD cost: (xyz1, xyz2, match, cost, work, B, n, m, stream)
    assert lib.upp_emd_matchcost_det(*[P] * 5, 0, 8, 8, None) == 0
    for k in range(5):
        assert lib.upp_emd_matchcost_det(*[None if i == k else P for i in range(5)], 1, 8, 8, None) == E, k
    for dims in ((-1, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert lib.upp_emd_matchcost_det(*[P] * 5, *dims, None) == E, dims
    assert lib.upp_emd_matchcost_det(*[P] * 5, 65536, 8, 8, None) == -2         # the sibling's limit, not a narrower one


def test_work_bytes_is_non_negative_and_monotone():
    wb = _abi.load().upp_emd_matchcost_det_work_bytes
    sizes = (0, 1, 2, 63, 64, 65, 200, 1024, 8192, 100000)
    for a in sizes:
        for b in sizes:
            for c in (0, 1, 130, 1024):
                v = wb(a, b, c)
                assert v >= 0
                assert wb(a + 1, b, c) >= v and wb(a, b + 1, c) >= v and wb(a, b, c + 1) >= v, (a, b, c)
    assert wb(2, 200, 130) == 2 * 4 * 4 and wb(32, 1024, 1024) == 32 * 16 * 4          # one f32 per 64-point tile of xyz1
    assert wb(-1, 8, 8) == 0 and wb(1, -8, 8) == 0 and wb(1, 8, -8) == 0
    assert wb(65535, 2 ** 31 - 1, 1) > 2 ** 40                                          # no 32-bit overflow


def _chamfer_case(B, n, m, seed, grid=None):
    g = np.random.default_rng(seed)
    a, b = g.standard_normal((B, n, 3)).astype(np.float32), g.standard_normal((B, m, 3)).astype(np.float32)
    if grid:
        a, b = np.round(a * grid) / grid, np.round(b * grid) / grid
    d = ((a[:, :, None, :].astype(np.float64) - b[:, None, :, :]) ** 2).sum(-1)
    i1, i2 = d.argmin(2).astype(np.int32), d.argmin(1).astype(np.int32)
    gd1, gd2 = g.standard_normal((B, n)).astype(np.float32), g.standard_normal((B, m)).astype(np.float32)
    gd1[:, ::5] = 0.0
    return a.astype(np.float32), b.astype(np.float32), i1, i2, gd1, gd2


def test_restatements_agree_with_float64_sums():
    a, b, i1, i2, gd1, gd2 = _chamfer_case(2, 40, 96, 0, grid=4)
    g1, g2 = R.chamfer_bwd(a, b, i1, i2, gd1, gd2)
    w1, w2 = np.zeros(a.shape), np.zeros(b.shape)
    for c in range(2):
        t1 = 2.0 * gd1[c].astype(np.float64)[:, None] * (a[c].astype(np.float64) - b[c][i1[c]])
        t2 = 2.0 * gd2[c].astype(np.float64)[:, None] * (b[c].astype(np.float64) - a[c][i2[c]])
        w1[c] += t1; np.subtract.at(w1[c], i2[c], t2)
        w2[c] += t2; np.subtract.at(w2[c], i1[c], t1)
    for got, want in ((g1, w1), (g2, w2)):
        # 1e-6 relative to the largest gradient entry (entries that cancel have no relative error of their own): lists of at most 10
        # terms here, each rounding <= 6e-8 of a partial sum
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    g = np.random.default_rng(1)
    go, idx = g.standard_normal((2, 6, 5, 3)).astype(np.float32), g.integers(0, 9, (2, 6, 5))
    gx, gc = R.group_bwd(go, idx, 9)
    want = np.zeros((2, 9, 3))
    for c in range(2):
        np.add.at(want[c], idx[c].reshape(-1), go[c].reshape(-1, 3).astype(np.float64))
    assert np.allclose(gx, want, rtol=1e-6, atol=1e-6) and np.allclose(gc, -go.astype(np.float64).sum(2), rtol=1e-6, atol=1e-6)
    assert gx.dtype == np.float32 and not np.signbit(gx[want == 0]).any()             # rows nobody references: +0.0
    gf, ix = g.standard_normal((2, 4, 7)).astype(np.float32), g.integers(0, 5, (2, 7))
    want = np.zeros((2, 4, 5))
    for c in range(2):
        for j in range(7):
            want[c, :, ix[c, j]] += gf[c, :, j]
    assert np.allclose(R.gather_bwd(gf, ix, 5), want, rtol=1e-6, atol=1e-6)
    gcen, ix = g.standard_normal((2, 8, 3)).astype(np.float32), g.integers(-2, 12, (2, 8))        # some outside [0, 10): skipped
    want = np.zeros((2, 10, 3))
    for c in range(2):
        for j in range(8):
            if 0 <= ix[c, j] < 10:
                want[c, ix[c, j]] += gcen[c, j]
    assert np.allclose(R.fps_gather_bwd(gcen, ix, 10), want, rtol=1e-6, atol=1e-6)
    parts = g.standard_normal((3, 16)).astype(np.float32)
    assert np.allclose(R.ordered_sum(parts), parts.astype(np.float64).sum(1), rtol=1e-6, atol=1e-6)


def test_one_foreign_term_commutes_and_three_terms_do_not():
    """own + one foreign term is the same f32 number in either order (what makes the `_det` kernels equal to the atomic ones there);
    a crafted list of three is not -- reversing it changes the restatement, so a kernel that summed in another order would be caught."""
    a, b, i1, i2, gd1, gd2 = _chamfer_case(2, 24, 24, 3)
    i2 = np.stack([np.random.default_rng(c).permutation(24) for c in range(2)]).astype(np.int32)      # every target: exactly one foreign term
    f, r = R.chamfer_bwd(a, b, i1, i2, gd1, gd2), R.chamfer_bwd(a, b, i1, i2, gd1, gd2, reverse=True)
    assert np.array_equal(f[0].view(np.int32), r[0].view(np.int32))
    t1, t2 = R.chamfer_terms(a[0], b[0], i1[0], gd1[0]), R.chamfer_terms(b[0], a[0], i2[0], gd2[0])
    inv = np.argsort(i2[0])
    assert np.array_equal(f[0][0].view(np.int32), ((np.float32(0) - t2[inv]) + t1).astype(np.float32).view(np.int32))   # foreign first, then own
    big = np.array([[[1e8, 1e8, 3.0], [-1e8, 1.0, 5.0], [1.0, -1e8, 7.0]]], np.float32)               # vals[b][s][w]: column 0 is (1e8, -1e8, 1)
    idx = np.zeros((1, 3), np.int64)
    fwd, rev = R.rows_scatter(big, idx, 2), R.rows_scatter(big, idx, 2, reverse=True)
    assert fwd[0, 0].tolist() == [1.0, 0.0, 15.0] and rev[0, 0].tolist() == [0.0, 0.0, 15.0]          # (1e8 - 1e8) + 1 = 1, (1 - 1e8) + 1e8 = 0
    assert not np.array_equal(fwd, rev) and not fwd[0, 1].any()
    assert R.ordered_sum(big[0].T)[0] == 1.0 and R.ordered_sum(big[0].T, reverse=True)[0] == 0.0
    xyz1 = np.zeros((1, 1, 3), np.float32)
    xyz2 = np.array([[[-5e7, 0, 0], [5e7, 0, 0], [-0.5, 0, 0]]], np.float32)                           # - t2 = -2 (xyz2 - 0): the same list
    one = np.ones((1, 3), np.float32)
    z = np.zeros((1, 1), np.float32)
    gf = R.chamfer_bwd(xyz1, xyz2, np.zeros((1, 1), np.int32), np.zeros((1, 3), np.int32), z, one)[0]
    gr = R.chamfer_bwd(xyz1, xyz2, np.zeros((1, 1), np.int32), np.zeros((1, 3), np.int32), z, one, reverse=True)[0]
    assert gf[0, 0, 0] == 1.0 and gr[0, 0, 0] == 0.0


def test_context_manager_sets_and_restores_the_attribute():
    was = HF.DETERMINISTIC
    try:
        HF.DETERMINISTIC = False
        with HF.deterministic():
            assert HF.DETERMINISTIC is True
            with HF.deterministic(False):
                assert HF.DETERMINISTIC is False
            assert HF.DETERMINISTIC is True
        assert HF.DETERMINISTIC is False
        with pytest.raises(ZeroDivisionError):
            with HF.deterministic(True):
                1 / 0
        assert HF.DETERMINISTIC is False
    finally:
        HF.DETERMINISTIC = was


@pytest.mark.parametrize("value,want", [("1", True), ("0", False), (None, False)])
def test_environment_variable_is_read_once_at_import(value, want):
    env = {k: v for k, v in os.environ.items() if k != "UPP_DETERMINISTIC"}
    if value is not None:
        env["UPP_DETERMINISTIC"] = value
    out = subprocess.check_output([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import upp_hip.functional as HF; print(HF.DETERMINISTIC)" % PKG],
                                  env=env, text=True)
    assert out.strip() == str(want)


class _Fake:
    """Stand-ins for upp_hip.ops: CPU tensors of the right shapes, and a record of the `deterministic` argument each call received."""

    def __init__(self, monkeypatch):
        self.seen = []
        for name in ("gather_fwd", "gather_bwd", "fps", "fps_gather_bwd", "knn", "group_fwd", "group_bwd", "chamfer_fwd", "chamfer_bwd",
                     "chamfer_loss", "emd_approxmatch", "emd_matchcost", "emd_matchcost_bwd"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def _note(self, name, kw):
        self.seen.append((name, kw.get("deterministic", "absent")))

    def gather_fwd(self, f, idx):
        return f[:, :, :idx.shape[1]].clone()

    def gather_bwd(self, g, idx, N, **kw):
        self._note("gather_bwd", kw)
        return torch.zeros(g.shape[0], g.shape[1], N)

    def fps(self, xyz, npoint, want_centers=False, waves=0):
        return torch.zeros(xyz.shape[0], npoint, dtype=torch.int32), xyz[:, :npoint].clone()

    def fps_gather_bwd(self, g, idx, N, **kw):
        self._note("fps_gather_bwd", kw)
        return torch.zeros(g.shape[0], N, 3)

    def knn(self, xyz, center, k, want_dist=True, want_neigh=False, prefilter=True):
        B, G = center.shape[:2]
        return None, torch.zeros(B, G, k, dtype=torch.int64), torch.zeros(B, G, k, 3)

    def group_fwd(self, xyz, center, idx):
        return torch.zeros(*idx.shape, 3)

    def group_bwd(self, g, idx, N, need_xyz=True, need_center=True, **kw):
        self._note("group_bwd", kw)
        return torch.zeros(g.shape[0], N, 3), torch.zeros(g.shape[0], g.shape[1], 3)

    def chamfer_fwd(self, a, b):
        B, n, m = a.shape[0], a.shape[1], b.shape[1]
        return torch.zeros(B, n), torch.zeros(B, m), torch.zeros(B, n, dtype=torch.int32), torch.zeros(B, m, dtype=torch.int32)

    def chamfer_loss(self, d1, d2, l1):
        return torch.zeros(1), torch.ones_like(d1), torch.ones_like(d2)

    def chamfer_bwd(self, a, b, i1, i2, g1, g2, **kw):
        self._note("chamfer_bwd", kw)
        return torch.zeros_like(a), torch.zeros_like(b)

    def emd_approxmatch(self, a, b):
        return torch.zeros(a.shape[0], b.shape[1], a.shape[1])

    def emd_matchcost(self, a, b, match, **kw):
        self._note("emd_matchcost", kw)
        return torch.zeros(a.shape[0])

    def emd_matchcost_bwd(self, g, a, b, match):
        return torch.zeros_like(a), torch.zeros_like(b)


def _run_the_seven_nodes():
    x = torch.rand(2, 12, 3, requires_grad=True)
    c = torch.rand(2, 4, 3, requires_grad=True)
    feat = torch.rand(2, 3, 12, requires_grad=True)
    HF.GatherOperation.apply(feat, torch.zeros(2, 4, dtype=torch.int32)).sum().backward()
    HF._FpsGather.apply(x, 4)[0].sum().backward()
    HF._KnnGroup.apply(x, c, 3)[0].sum().backward()
    HF._GroupPoints.apply(x, c, torch.zeros(2, 4, 3, dtype=torch.int64)).sum().backward()
    d1, d2 = HF.ChamferFunction.apply(x, c)
    (d1.sum() + d2.sum()).backward()
    HF.chamfer_loss(x, c).backward()
    # the EMD node asserts HIP tensors: its forward is called directly, on stand-ins that say they are
    t = types.SimpleNamespace(is_cuda=True, shape=(2, 12, 3))
    t.contiguous = lambda: t
    HF.EarthMoverDistanceFunction.forward(types.SimpleNamespace(save_for_backward=lambda *a: None), t, t)


def test_each_autograd_node_passes_the_flag_exactly_when_the_mode_is_on(monkeypatch):
    fake = _Fake(monkeypatch)
    names = ["gather_bwd", "fps_gather_bwd", "group_bwd", "group_bwd", "chamfer_bwd", "chamfer_bwd", "emd_matchcost"]
    monkeypatch.setattr(HF, "DETERMINISTIC", False)
    _run_the_seven_nodes()
    assert [n for n, _ in fake.seen] == names
    assert all(not flag for _, flag in fake.seen), fake.seen             # off: False (or left out)
    fake.seen.clear()
    with HF.deterministic():
        _run_the_seven_nodes()
    assert fake.seen == [(n, True) for n in names]
    fake.seen.clear()
    _run_the_seven_nodes()
    assert all(not flag for _, flag in fake.seen) and len(fake.seen) == 7


def test_the_step_driver_sets_the_mode_for_its_own_passes_only():
    from upp_hip.train import TrainStep
    ts = TrainStep.__new__(TrainStep)
    seen = []
    ts._forward_backward_pass = lambda *a: seen.append(HF.DETERMINISTIC)
    was = HF.DETERMINISTIC
    try:
        for outer in (False, True):
            HF.DETERMINISTIC = outer
            for flag, want in ((True, True), (False, False), (None, outer)):
                ts.deterministic = flag
                ts._forward_backward()
                assert seen.pop() is want and HF.DETERMINISTIC is outer
    finally:
        HF.DETERMINISTIC = was
