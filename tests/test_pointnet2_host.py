"""The pointnet2_ops surface beyond FPS and gather, host side (no GPU): the shim exports upstream's names; CPU tensors are refused unless
the opt-in torch formulations are on, and those equal the numpy restatement (tests/_pointnet2_reference.py) bit for bit on lattice
clouds; the entry points validate their arguments before any launch; the two new autograd nodes hand `deterministic=True` to
upp_hip.ops exactly when the mode is on; and the seeds of the random GPU cases satisfy their preconditions."""
import ctypes

import numpy as np
import pytest
import torch

import _pointnet2_reference as R
from upp_hip import _abi, ops, torch_cpu
import upp_hip.functional as HF

P = ctypes.c_void_p(64)            # a non-NULL pointer that is never dereferenced: the checks below return before any launch
E = -1


def test_shim_exports_the_upstream_names():
    from pointnet2_ops import pointnet2_utils as p2
    names = ["furthest_point_sample", "gather_operation", "ball_query", "three_nn", "three_interpolate", "grouping_operation",
             "QueryAndGroup", "GroupAll", "FurthestPointSampling", "GatherOperation", "BallQuery", "ThreeNN", "ThreeInterpolate",
             "GroupingOperation"]
    for n in names:
        assert hasattr(p2, n), n
        assert n in p2.__all__, n
    for n in ("BallQuery", "ThreeNN", "ThreeInterpolate", "GroupingOperation"):
        assert issubclass(getattr(p2, n), torch.autograd.Function)
    assert issubclass(p2.QueryAndGroup, torch.nn.Module) and issubclass(p2.GroupAll, torch.nn.Module)


def test_cpu_tensors_are_refused_while_the_torch_formulations_are_off():
    from pointnet2_ops import pointnet2_utils as p2
    assert not torch_cpu.enabled()
    x, q = torch.rand(2, 16, 3), torch.rand(2, 4, 3)
    f = torch.rand(2, 5, 16)
    i3, w3 = torch.zeros(2, 4, 3, dtype=torch.int32), torch.rand(2, 4, 3)
    calls = [lambda: p2.ball_query(0.5, 4, x, q), lambda: p2.three_nn(q, x), lambda: p2.three_interpolate(f, i3, w3),
             lambda: p2.grouping_operation(f, i3), lambda: p2.QueryAndGroup(0.5, 4)(x, q, f),
             lambda: ops.ball_query(0.5, 4, x, q), lambda: ops.three_nn(q, x), lambda: ops.three_interpolate_fwd(f, i3, w3),
             lambda: ops.three_interpolate_bwd(torch.rand(2, 5, 4), i3, w3, 16), lambda: ops.grouping_fwd(f, i3),
             lambda: ops.grouping_bwd(torch.rand(2, 5, 4, 3), i3, 16)]
    for k, call in enumerate(calls):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


@pytest.fixture
def cpu_on():
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    yield
    torch_cpu.enable(was)


@pytest.mark.parametrize("shape", R.BALL_SHAPES)
def test_torch_ball_query_and_grouping_equal_the_restatement_on_lattice_clouds(cpu_on, shape):
    xyz, new_xyz = R.lattice_ball_case(shape)
    want, hits = R.ball_query(xyz, new_xyz, R.RADIUS, shape[3])
    assert np.array_equal(want, R.ball_query(xyz, new_xyz, R.RADIUS, shape[3], R.sqdist64)[0])       # lattice: f32 is exact
    assert any((R.sqdist64(new_xyz[b], xyz[b]) == 0.25).any() for b in range(shape[0]))              # points at exactly the radius ...
    assert all(hits[b, 0] == 0 or (want[b, 0] != 0).all() for b in range(shape[0]))                  # ... and point 0 is one: excluded
    got = HF.ball_query(R.RADIUS, shape[3], torch.from_numpy(xyz), torch.from_numpy(new_xyz))
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    feat = np.random.default_rng(1).standard_normal((shape[0], 5, shape[1])).astype(np.float32)
    f = torch.from_numpy(feat).requires_grad_(True)
    out = HF.grouping_operation(f, got)
    assert np.array_equal(out.detach().numpy(), R.grouping(feat, want))
    go = np.random.default_rng(2).random(out.shape, dtype=np.float32)
    out.backward(torch.from_numpy(go))
    np.testing.assert_allclose(f.grad.numpy(), R.grouping_bwd_det(go, want, shape[1]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape", R.NN_SHAPES)
def test_torch_three_nn_and_interpolate_equal_the_restatement_on_lattice_clouds(cpu_on, shape):
    unknown, known = R.lattice_nn_case(shape)
    wd, wi = R.three_nn(unknown, known)
    assert np.array_equal(wi, R.three_nn(unknown, known, R.sqdist64)[1])
    dist, idx = HF.three_nn(torch.from_numpy(unknown), torch.from_numpy(known))
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32
    assert np.array_equal(idx.numpy(), wi) and np.array_equal(dist.numpy().view(np.int32), wd.view(np.int32))
    if shape[2] < 3:
        assert (wi[:, :, shape[2]:] == 0).all() and np.isposinf(wd[:, :, shape[2]:]).all()
    g = np.random.default_rng(3)
    feat, w = g.standard_normal((shape[0], 5, shape[2])).astype(np.float32), g.random((shape[0], shape[1], 3), dtype=np.float32)
    f = torch.from_numpy(feat).requires_grad_(True)
    out = HF.three_interpolate(f, idx, torch.from_numpy(w))
    assert np.array_equal(out.detach().numpy().view(np.int32), R.three_interpolate(feat, wi, w).view(np.int32))
    go = g.random(out.shape, dtype=np.float32)
    out.backward(torch.from_numpy(go))
    np.testing.assert_allclose(f.grad.numpy(), R.three_interpolate_bwd_det(go, wi, w, shape[2]), rtol=1e-5, atol=1e-6)


def test_modules_equal_the_composition_of_the_operators(cpu_on):
    shape = R.BALL_SHAPES[0]
    xyz, new_xyz = (torch.from_numpy(a) for a in R.lattice_ball_case(shape))
    B, N, P_, S = shape
    feat = torch.rand(B, 6, N, generator=torch.Generator().manual_seed(4))
    idx = HF.ball_query(R.RADIUS, S, xyz, new_xyz)
    gx = HF.grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
    gf = HF.grouping_operation(feat, idx)
    out = HF.QueryAndGroup(R.RADIUS, S)(xyz, new_xyz, feat)
    assert out.shape == (B, 9, P_, S) and torch.equal(out, torch.cat([gx, gf], 1))
    out = HF.QueryAndGroup(R.RADIUS, S, use_xyz=False)(xyz, new_xyz, feat)
    assert out.shape == (B, 6, P_, S) and torch.equal(out, gf)
    out = HF.QueryAndGroup(R.RADIUS, S)(xyz, new_xyz)
    assert out.shape == (B, 3, P_, S) and torch.equal(out, gx)
    with pytest.raises(ValueError):
        HF.QueryAndGroup(R.RADIUS, S, use_xyz=False)(xyz, new_xyz)
    out = HF.GroupAll()(xyz, new_xyz, feat)
    assert out.shape == (B, 9, 1, N) and torch.equal(out[:, :3, 0], xyz.transpose(1, 2)) and torch.equal(out[:, 3:, 0], feat)
    assert HF.GroupAll(use_xyz=False)(xyz, new_xyz, feat).shape == (B, 6, 1, N)
    assert HF.GroupAll()(xyz, None).shape == (B, 3, 1, N)


def test_entry_points_validate_before_any_launch():
    lib = _abi.load()
    # ball query: (xyz, new_xyz, radius, nsample, idx, B, N, P, stream)
    assert lib.upp_ball_query(P, P, 0.5, 4, P, 0, 8, 4, None) == 0
    for k in range(3):
        a = [None if i == k else P for i in range(3)]
        assert lib.upp_ball_query(a[0], a[1], 0.5, 4, a[2], 1, 8, 4, None) == E, k
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.upp_ball_query(P, P, radius, 4, P, 1, 8, 4, None) == E, radius
    for nsample, dims in ((0, (1, 8, 4)), (-2, (1, 8, 4)), (4, (-1, 8, 4)), (4, (1, 0, 4)), (4, (1, 8, 0))):
        assert lib.upp_ball_query(P, P, 0.5, nsample, P, *dims, None) == E, (nsample, dims)
    assert lib.upp_ball_query(P, P, 0.5, 4, P, 65536, 8, 4, None) == -2                  # one grid row per cloud (INTEGRATION.md "Limits")
    # three_nn: (unknown, known, dist, idx, B, n, m, stream)
    assert lib.upp_three_nn(P, P, P, P, 0, 8, 4, None) == 0
    for k in range(4):
        assert lib.upp_three_nn(*[None if i == k else P for i in range(4)], 1, 8, 4, None) == E, k
    for dims in ((-1, 8, 4), (1, 0, 4), (1, 8, 0)):
        assert lib.upp_three_nn(P, P, P, P, *dims, None) == E, dims
    assert lib.upp_three_nn(P, P, P, P, 65536, 8, 4, None) == -2
    # three_interpolate: (dense, idx, weight, out, B, C, m, n, stream), the three entry points alike
    for fn in (lib.upp_three_interpolate_fwd, lib.upp_three_interpolate_bwd, lib.upp_three_interpolate_bwd_det):
        assert fn(P, P, P, P, 0, 5, 8, 4, None) == 0
        for k in range(4):
            assert fn(*[None if i == k else P for i in range(4)], 1, 5, 8, 4, None) == E, k
        for dims in ((-1, 5, 8, 4), (1, 0, 8, 4), (1, 5, 0, 4), (1, 5, 8, 0), (1, 5, 8, -4)):
            assert fn(P, P, P, P, *dims, None) == E, dims
    # grouping: (dense, idx, out, B, C, N, P, S, stream)
    for fn in (lib.upp_grouping_fwd, lib.upp_grouping_bwd, lib.upp_grouping_bwd_det):
        assert fn(P, P, P, 0, 5, 8, 4, 3, None) == 0
        for k in range(3):
            assert fn(*[None if i == k else P for i in range(3)], 1, 5, 8, 4, 3, None) == E, k
        for dims in ((-1, 5, 8, 4, 3), (1, 0, 8, 4, 3), (1, 5, 0, 4, 3), (1, 5, 8, 0, 3), (1, 5, 8, 4, 0)):
            assert fn(P, P, P, *dims, None) == E, dims
        assert fn(P, P, P, 1, 5, 8, 65536, 65536, None) == -2
    # the `_det` siblings take their siblings' arguments; no new process-wide option
    for name in ("upp_three_interpolate_bwd_det", "upp_grouping_bwd_det"):
        assert _abi.SIGNATURES[name] == _abi.SIGNATURES[name[:-4]]
    assert len(_abi.OPTIONS) == 4 and lib.upp_abi_version() == 5


def test_det_restatements_agree_with_float64_sums_and_see_order():
    g = np.random.default_rng(5)
    go, w, idx = g.standard_normal((2, 4, 9)).astype(np.float32), g.random((2, 9, 3), dtype=np.float32), g.integers(0, 5, (2, 9, 3))
    want = np.zeros((2, 4, 5))
    for b in range(2):
        for i in range(9):
            for j in range(3):
                want[b, :, idx[b, i, j]] += go[b, :, i].astype(np.float64) * w[b, i, j]
    got = R.three_interpolate_bwd_det(go, idx, w, 5)
    assert got.dtype == np.float32 and np.allclose(got, want, rtol=1e-5, atol=1e-6)
    go4, ix = g.standard_normal((2, 4, 3, 5)).astype(np.float32), g.integers(0, 6, (2, 3, 5))
    want = np.zeros((2, 4, 7))
    for b in range(2):
        for s in range(15):
            want[b, :, ix[b].reshape(-1)[s]] += go4[b].reshape(4, 15)[:, s]
    got = R.grouping_bwd_det(go4, ix, 7)
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6) and not got[:, :, 6].any() and not np.signbit(got[:, :, 6]).any()
    big = np.array([[[1e8, -1e8, 1.0]]], np.float32)                       # (1e8 - 1e8) + 1 = 1, (1 - 1e8) + 1e8 = 0
    zero = np.zeros((1, 1, 3), np.int64)
    assert R.grouping_bwd_det(big.reshape(1, 1, 1, 3), zero, 2)[0, 0].tolist() == [1.0, 0.0]
    assert R.grouping_bwd_det(big.reshape(1, 1, 1, 3), zero, 2, reverse=True)[0, 0].tolist() == [0.0, 0.0]
    one = np.ones((1, 1, 1), np.float32)
    assert R.three_interpolate_bwd_det(one, zero, big, 2)[0, 0].tolist() == [1.0, 0.0]
    assert R.three_interpolate_bwd_det(one, zero, big, 2, reverse=True)[0, 0].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("shape", R.BALL_SHAPES + R.BALL_SHAPES_LONG)
def test_random_ball_query_cases_satisfy_their_preconditions(shape):
    xyz, new_xyz = R.random_ball_case(shape)
    assert R.ball_preconditions(xyz, new_xyz, shape[3])
    assert np.array_equal(R.ball_query(xyz, new_xyz, R.RADIUS, shape[3])[0], R.ball_query(xyz, new_xyz, R.RADIUS, shape[3], R.sqdist64)[0])


@pytest.mark.parametrize("shape", R.NN_SHAPES + R.NN_SHAPES_LONG)
def test_random_three_nn_cases_satisfy_their_preconditions(shape):
    unknown, known = R.random_nn_case(shape)
    assert R.nn_preconditions(unknown, known)
    assert np.array_equal(R.three_nn(unknown, known)[1], R.three_nn(unknown, known, R.sqdist64)[1])


class _Fake:
    """Stand-ins for the new upp_hip.ops entries: CPU tensors of the right shapes, and a record of the `deterministic` argument."""

    def __init__(self, monkeypatch):
        self.seen = []
        for name in ("three_interpolate_fwd", "three_interpolate_bwd", "grouping_fwd", "grouping_bwd"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def three_interpolate_fwd(self, f, idx, w):
        return torch.zeros(f.shape[0], f.shape[1], idx.shape[1])

    def three_interpolate_bwd(self, g, idx, w, m, **kw):
        self.seen.append(("three_interpolate_bwd", kw.get("deterministic", "absent")))
        return torch.zeros(g.shape[0], g.shape[1], m)

    def grouping_fwd(self, f, idx):
        return torch.zeros(f.shape[0], f.shape[1], idx.shape[1], idx.shape[2])

    def grouping_bwd(self, g, idx, N, **kw):
        self.seen.append(("grouping_bwd", kw.get("deterministic", "absent")))
        return torch.zeros(g.shape[0], g.shape[1], N)


def _run_the_two_nodes():
    feat = torch.rand(2, 3, 12, requires_grad=True)
    HF.ThreeInterpolate.apply(feat, torch.zeros(2, 4, 3, dtype=torch.int32), torch.rand(2, 4, 3)).sum().backward()
    HF.GroupingOperation.apply(feat, torch.zeros(2, 4, 5, dtype=torch.int32)).sum().backward()
    assert feat.grad.shape == (2, 3, 12)


def test_the_two_new_nodes_pass_the_flag_exactly_when_the_mode_is_on(monkeypatch):
    fake = _Fake(monkeypatch)
    names = ["three_interpolate_bwd", "grouping_bwd"]
    monkeypatch.setattr(HF, "DETERMINISTIC", False)
    _run_the_two_nodes()
    assert [n for n, _ in fake.seen] == names and all(not flag for _, flag in fake.seen), fake.seen
    fake.seen.clear()
    with HF.deterministic():
        _run_the_two_nodes()
    assert fake.seen == [(n, True) for n in names]
    fake.seen.clear()
    _run_the_two_nodes()
    assert len(fake.seen) == 2 and all(not flag for _, flag in fake.seen)


def test_search_outputs_are_marked_non_differentiable(monkeypatch):
    monkeypatch.setattr(ops, "ball_query", lambda r, s, x, q: torch.zeros(x.shape[0], q.shape[1], s, dtype=torch.int32))
    monkeypatch.setattr(ops, "three_nn", lambda u, k: (torch.zeros(u.shape), torch.zeros(u.shape, dtype=torch.int32)))
    x, q = torch.rand(1, 8, 3, requires_grad=True), torch.rand(1, 2, 3, requires_grad=True)
    assert not HF.BallQuery.apply(0.5, 4, x, q).requires_grad
    dist, idx = HF.ThreeNN.apply(q, x)
    assert not dist.requires_grad and not idx.requires_grad
