"""The pointnet2_ops surface beyond FPS and gather on the GPU: ball_query, three_nn, three_interpolate, grouping_operation and the two
modules, against the numpy restatement of their rules (tests/_pointnet2_reference.py).  Indices and lattice distances are compared
bit for bit; forwards bit for bit against the stated rounding order; `_det` backward passes bit for bit against the stated summation
order; atomic backward passes against a float64 scatter-add with the tolerance tests/test_gpu_parity.py uses for gather_bwd.
Run on the GPU box with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import _det_reference as D
import _pointnet2_reference as R
import _seeded
from upp_hip import ops, functional as HF
from pointnet2_ops import pointnet2_utils as p2

pytestmark = pytest.mark.gpu

CHANNELS = [1, 5, 64, 130]
# tests/test_gpu_parity.py test_gather_operation_forward_backward: the f32-atomic scatter-add against the float64 sum, on addends in
# [0, 1) as there (no cancellation: every rounding is relative to a partial sum below the result)
BWD_RTOL, BWD_ATOL = 1e-6, 1e-7


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def ball_case(shape, kind):
    """-> xyz, new_xyz, the restated indices; computed once and shared (never modified)."""
    if kind == "lattice":
        xyz, new_xyz = R.lattice_ball_case(shape)
        want, _ = R.ball_query(xyz, new_xyz, R.RADIUS, shape[3])
        assert any((R.sqdist64(new_xyz[b], xyz[b]) == 0.25).any() for b in range(shape[0]))     # points at exactly the radius: excluded
    else:
        xyz, new_xyz = R.random_ball_case(shape)
        assert R.ball_preconditions(xyz, new_xyz, shape[3])                # on the float64 distances alone
        want, _ = R.ball_query(xyz, new_xyz, R.RADIUS, shape[3], R.sqdist64)
    return xyz, new_xyz, want


@functools.lru_cache(maxsize=None)
def nn_case(shape, kind):
    if kind == "lattice":
        unknown, known = R.lattice_nn_case(shape)
        dist, idx = R.three_nn(unknown, known)
    else:
        unknown, known = R.random_nn_case(shape)
        assert R.nn_preconditions(unknown, known)
        dist, idx = R.three_nn(unknown, known, R.sqdist64)                 # float64 distances
    return unknown, known, dist, idx


def replay_twice(fn):
    """fn() -> tensors.  One eager run, then one capture replayed twice with the outputs scribbled over in between: every replay must
    rewrite every element."""
    eager = [t.clone() for t in fn()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    for _ in range(2):
        for t in out:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
    return eager


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("shape", R.BALL_SHAPES + R.BALL_SHAPES_LONG)
def test_ball_query_indices_bit_exact_eager_and_captured(shape, kind):
    xyz, new_xyz, want = ball_case(shape, kind)
    x, q = dev(xyz), dev(new_xyz)
    (idx,) = replay_twice(lambda: (ops.ball_query(R.RADIUS, shape[3], x, q),))
    assert idx.dtype == torch.int32 and idx.shape == (shape[0], shape[2], shape[3])
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    via = p2.ball_query(R.RADIUS, shape[3], x.requires_grad_(True), q)
    assert torch.equal(via, idx) and not via.requires_grad


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("shape", R.NN_SHAPES + R.NN_SHAPES_LONG)
def test_three_nn_indices_and_distances(shape, kind):
    unknown, known, wd, wi = nn_case(shape, kind)
    u, k = dev(unknown), dev(known)
    dist, idx = replay_twice(lambda: ops.three_nn(u, k))
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32
    np.testing.assert_array_equal(idx.cpu().numpy(), wi)
    got = dist.cpu().numpy()
    m = shape[2]
    if m < 3:                                                  # the unfilled slots: index 0, +inf
        assert (idx.cpu().numpy()[:, :, m:] == 0).all() and np.isposinf(got[:, :, m:]).all()
    if kind == "lattice":
        np.testing.assert_array_equal(bits(got), bits(wd))
    else:
        # wd: sqrt of the float64 squared distance.  The f32 value: three differences (relative error u = 2^-24 each, 2u in their
        # squares), then y*y, fma, fma (u each, all terms positive) -> 5u on the squared distance, 2.5u after the square root, + u
        # for the root's own rounding = 3.5u; asserted with 4u.
        fin = np.isfinite(wd)
        assert np.array_equal(fin, np.isfinite(got))
        err = np.abs(got[fin].astype(np.float64) - wd[fin])
        print("three_nn max relative distance error / u:", float((err / wd[fin]).max() * 2 ** 24))
        assert (err <= 4 * 2.0 ** -24 * wd[fin]).all()
    d2, i2 = p2.three_nn(dev(unknown).requires_grad_(True), dev(known))
    assert torch.equal(i2, idx) and torch.equal(d2, dist) and not d2.requires_grad


def _f64_scatter(vals, keys, N):
    """vals (B,C,S), keys (B,S) -> (B,C,N) float64 scatter-add."""
    B, C, _ = vals.shape
    out = np.zeros((B, C, N))
    for b in range(B):
        np.add.at(out[b].T, keys[b], vals[b].T.astype(np.float64))
    return out


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape", R.NN_SHAPES)
def test_three_interpolate_forward_and_backward(shape, C):
    B, n, m = shape
    _, _, wd, wi = nn_case(shape, "lattice")
    g = np.random.default_rng(n * 7 + m + C)
    feat = g.standard_normal((B, C, m)).astype(np.float32)
    w = g.random((B, n, 3), dtype=np.float32)
    go = g.random((B, C, n), dtype=np.float32)
    f, idx, wt = dev(feat).requires_grad_(True), dev(wi), dev(w)
    out = p2.three_interpolate(f, idx, wt)
    np.testing.assert_array_equal(bits(out.detach().cpu().numpy()), bits(R.three_interpolate(feat, wi, w)))
    out.backward(dev(go))                                                              # atomics
    want64 = _f64_scatter(np.repeat(go, 3, axis=2).astype(np.float64) * w.reshape(B, 1, 3 * n), wi.reshape(B, 3 * n), m)
    np.testing.assert_allclose(f.grad.cpu().numpy(), want64, rtol=BWD_RTOL, atol=BWD_ATOL)
    want = R.three_interpolate_bwd_det(go, wi, w, m)
    runs = []
    for _ in range(2):
        f.grad = None
        with HF.deterministic():
            p2.three_interpolate(f, idx, wt).backward(dev(go))
        runs.append(f.grad.cpu().numpy())
    np.testing.assert_array_equal(bits(runs[0]), bits(want))
    np.testing.assert_array_equal(bits(runs[0]), bits(runs[1]))


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape", R.BALL_SHAPES)
def test_grouping_operation_forward_and_backward(shape, C):
    B, N, P, S = shape
    _, _, wi = ball_case(shape, "lattice")
    g = np.random.default_rng(N * 5 + P + C)
    feat = g.standard_normal((B, C, N)).astype(np.float32)
    go = g.random((B, C, P, S), dtype=np.float32)
    f, idx = dev(feat).requires_grad_(True), dev(wi)
    out = p2.grouping_operation(f, idx)
    assert out.shape == (B, C, P, S)
    np.testing.assert_array_equal(bits(out.detach().cpu().numpy()), bits(R.grouping(feat, wi)))
    out.backward(dev(go))
    np.testing.assert_allclose(f.grad.cpu().numpy(), _f64_scatter(go.reshape(B, C, P * S), wi.reshape(B, P * S), N), rtol=BWD_RTOL, atol=BWD_ATOL)
    want = R.grouping_bwd_det(go, wi, N)
    runs = []
    for _ in range(2):
        f.grad = None
        with HF.deterministic():
            p2.grouping_operation(f, idx).backward(dev(go))
        runs.append(f.grad.cpu().numpy())
    np.testing.assert_array_equal(bits(runs[0]), bits(want))
    np.testing.assert_array_equal(bits(runs[0]), bits(runs[1]))


@pytest.mark.parametrize("C", [1, 130])
def test_det_backward_with_one_loaded_target_and_untouched_targets(C):
    """All indices equal: one target receives every term, in the stated order (signed terms of mixed magnitude: another order gives other
    bits); every other target receives none and must be +0.0f -- in a buffer that held garbage before the call."""
    g = np.random.default_rng(C)
    B, n, m = 2, 129, 300                                            # 387 terms on one target; targets beyond one tile of 256
    go = (g.standard_normal((B, C, n)) * 10.0 ** g.integers(-3, 4, (B, C, n))).astype(np.float32)
    w = g.random((B, n, 3), dtype=np.float32)
    idx = np.full((B, n, 3), 257, np.int32)
    want = R.three_interpolate_bwd_det(go, idx, w, m)
    assert not np.array_equal(bits(want), bits(R.three_interpolate_bwd_det(go, idx, w, m, reverse=True)))       # the order is visible
    runs = [ops.three_interpolate_bwd(dev(go), dev(idx), dev(w), m, deterministic=True).cpu().numpy() for _ in range(2)]
    np.testing.assert_array_equal(bits(runs[0]), bits(want))
    np.testing.assert_array_equal(bits(runs[0]), bits(runs[1]))
    rest = np.delete(runs[0], 257, axis=2)
    assert not rest.any() and not np.signbit(rest).any()
    P, S, N = 9, 43, 300
    go4 = (g.standard_normal((B, C, P, S)) * 10.0 ** g.integers(-3, 4, (B, C, P, S))).astype(np.float32)
    ix = np.full((B, P, S), 3, np.int32)
    want = R.grouping_bwd_det(go4, ix, N)
    assert not np.array_equal(bits(want), bits(R.grouping_bwd_det(go4, ix, N, reverse=True)))
    runs = [ops.grouping_bwd(dev(go4), dev(ix), N, deterministic=True).cpu().numpy() for _ in range(2)]
    np.testing.assert_array_equal(bits(runs[0]), bits(want))
    np.testing.assert_array_equal(bits(runs[0]), bits(runs[1]))
    rest = np.delete(runs[0], 3, axis=2)
    assert not rest.any() and not np.signbit(rest).any()


def test_three_interpolate_det_backward_at_the_edges_of_the_shared_body():
    """5 channels (a second channel group with one live channel), 257 targets (a second tile with one live lane), a second chunk of fewer
    than four sources, keys of -1 and of the target count.  deterministic=True only: the atomic siblings do not range-check."""
    g = np.random.default_rng(343)
    B, C, n, m = 2, 5, 343, 257                                      # 1,029 sources: the row of source 1,024 straddles the chunk boundary
    go, w = D.mixed_upstream(g, (B, C, n)), g.random((B, n, 3), dtype=np.float32)
    idx = D.edge_indices(g, B, 3 * n, m).reshape(B, n, 3).astype(np.int32)
    want = R.three_interpolate_bwd_det(go, idx, w, m)
    assert not np.array_equal(bits(want), bits(R.three_interpolate_bwd_det(go, idx, w, m, reverse=True)))       # the order is visible
    got = ops.three_interpolate_bwd(dev(go), dev(idx), dev(w), m, deterministic=True).cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(want))


def test_grouping_det_backward_at_the_edges_of_the_shared_body():
    g = np.random.default_rng(1027)
    B, C, N, P, S = 2, 5, 257, 13, 79                                # 1,027 sources: a second chunk of three
    go4 = D.mixed_upstream(g, (B, C, P, S))
    ix = D.edge_indices(g, B, P * S, N).reshape(B, P, S).astype(np.int32)
    want = R.grouping_bwd_det(go4, ix, N)
    assert not np.array_equal(bits(want), bits(R.grouping_bwd_det(go4, ix, N, reverse=True)))
    got = ops.grouping_bwd(dev(go4), dev(ix), N, deterministic=True).cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(want))


@pytest.mark.parametrize("use_xyz,with_features", [(True, True), (False, True), (True, False)])
def test_query_and_group_through_autograd_equals_the_composition(use_xyz, with_features):
    shape = R.BALL_SHAPES[0]
    B, N, P, S = shape
    xyz_np, new_np, wi = ball_case(shape, "lattice")
    feat_np = np.random.default_rng(8).standard_normal((B, 6, N)).astype(np.float32)
    outs, grads = [], []
    for composed in (False, True):
        xyz, new_xyz = dev(xyz_np).requires_grad_(True), dev(new_np).requires_grad_(True)
        feat = dev(feat_np).requires_grad_(True) if with_features else None
        with HF.deterministic():
            if composed:
                idx = p2.ball_query(R.RADIUS, S, xyz, new_xyz)
                parts = []
                if use_xyz or feat is None:
                    parts.append(p2.grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1))
                if feat is not None:
                    parts.append(p2.grouping_operation(feat, idx))
                out = torch.cat(parts, 1)
            else:
                out = p2.QueryAndGroup(R.RADIUS, S, use_xyz=use_xyz)(xyz, new_xyz, feat)
            w = torch.rand(out.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
            (out * w).sum().backward()
        outs.append(out.detach())
        grads.append([t.grad for t in (xyz, new_xyz, feat) if t is not None])
    assert outs[0].shape == (B, (3 if use_xyz or not with_features else 0) + (6 if with_features else 0), P, S)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].cpu().numpy()
    if with_features:
        np.testing.assert_array_equal(bits(got[:, -6:]), bits(R.grouping(feat_np, wi)))
    if use_xyz or not with_features:                           # the grouped coordinates, centre subtracted (one f32 subtraction)
        np.testing.assert_array_equal(bits(got[:, :3]), bits(R.grouping(xyz_np.transpose(0, 2, 1), wi) - new_np.transpose(0, 2, 1)[:, :, :, None]))
    for a, b in zip(grads[0], grads[1]):
        if a is None or b is None:
            assert a is None and b is None                     # (use_xyz=False: the coordinates take no part)
        else:
            assert torch.equal(a, b)
    if use_xyz or not with_features:
        assert grads[0][0] is not None and grads[0][1] is not None and grads[0][0].abs().sum() > 0 and grads[0][1].abs().sum() > 0


def test_group_all_through_autograd():
    B, N = 2, 33
    xyz = dev(R.lattice_clouds(B, N, 1)).requires_grad_(True)
    feat = torch.rand(B, 5, N, device="cuda", requires_grad=True)
    out = p2.GroupAll()(xyz, None, feat)
    assert out.shape == (B, 8, 1, N) and torch.equal(out[:, :3, 0], xyz.transpose(1, 2)) and torch.equal(out[:, 3:, 0], feat)
    w = torch.rand_like(out)
    (out * w).sum().backward()
    assert torch.equal(xyz.grad, w[:, :3, 0].transpose(1, 2)) and torch.equal(feat.grad, w[:, 3:, 0])
    assert p2.GroupAll(use_xyz=False)(xyz, None, feat).shape == (B, 5, 1, N) and p2.GroupAll()(xyz, None).shape == (B, 3, 1, N)


def test_reference_call_pattern_three_nn_then_interpolate():
    """The reference's up-sampling step (models/Transformer_utils.py:225-230) through the shim at (B, N, m, C) = (2, 96, 32, 48):
    three_nn on contiguous positions, weight = 1 / (dist + 1e-8) normalised over the three, three_interpolate on the channels-first
    features.  Against the float64 evaluation of the same expression, with the tolerance of the scatter-add tests (features in [0, 1]:
    a dozen rounded operations, each relative to a positive partial result)."""
    B, N, m, C = 2, 96, 32, 48
    pos = _seeded.unit_ball_clouds(B, N, seed=21).contiguous()
    pos_known = pos[:, :m * 3:3].contiguous()
    v = ((_seeded.unit_ball_clouds(B, m * C // 3, seed=22).reshape(B, m, C) + 1.0) / 2.0).contiguous()
    assert R.nn_preconditions(pos.numpy(), pos_known.numpy())
    dist, idx = p2.three_nn(pos.cuda(), pos_known.cuda())
    recip = 1.0 / (dist + 1e-8)
    weight = recip / torch.sum(recip, dim=2, keepdim=True)
    out = p2.three_interpolate(v.cuda().transpose(-1, -2).contiguous(), idx, weight)
    assert out.shape == (B, C, N)
    d64, i64 = R.three_nn(pos.numpy(), pos_known.numpy(), R.sqdist64)
    np.testing.assert_array_equal(idx.cpu().numpy(), i64)
    r64 = 1.0 / (d64 + 1e-8)
    w64 = r64 / r64.sum(2, keepdims=True)
    f64 = v.numpy().astype(np.float64).transpose(0, 2, 1)                                  # (B, C, m)
    want = np.stack([(f64[b][:, i64[b]] * w64[b][None]).sum(-1) for b in range(B)])
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=BWD_RTOL, atol=BWD_ATOL)


def test_bad_arguments_raise_before_any_launch():
    x, q = torch.rand(2, 16, 3, device="cuda"), torch.rand(2, 4, 3, device="cuda")
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.ball_query(radius, 4, x, q)
    with pytest.raises(ValueError):
        ops.ball_query(0.5, 0, x, q)
    with pytest.raises(RuntimeError, match="int32"):
        ops.grouping_fwd(torch.rand(2, 3, 16, device="cuda"), torch.zeros(2, 4, 3, dtype=torch.int64, device="cuda"))
    assert ops.ball_query(0.5, 4, x[:0], q[:0]).shape == (0, 4, 4) and ops.three_nn(q[:0], x[:0])[1].shape == (0, 4, 3)
