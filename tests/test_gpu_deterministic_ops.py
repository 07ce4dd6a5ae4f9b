"""The deterministic siblings of the scatter-add kernels (include/upp_hip.h "deterministic scatter-adds") against the numpy restatements
of their defined orders (tests/_det_reference.py): BIT FOR BIT (np.array_equal on the int32 view) in every case -- sizes below one
workgroup's 256 targets, across several workgroups and LDS chunks of 1,024 sources, one target that owns every source, ties, zeros and
negative upstream gradients -- plus graph replays and the autograd switch."""
import os
import sys

import numpy as np
import pytest
import torch

import _det_reference as R
from upp_hip import ops
import upp_hip.functional as HF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), "%s: %d of %d elements differ" % (what, int((g != w).sum()), g.size)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _upstream(rng, shape):
    """random upstream gradients: some exactly 0, some negative"""
    g = rng.standard_normal(shape).astype(np.float32)
    g[rng.random(shape) < 0.15] = 0.0
    if not (g < 0).any():                      # (a draw of one or two numbers need not hold a negative one: make the largest negative)
        k = np.unravel_index(np.argmax(np.abs(g)), g.shape)
        g[k] = -abs(g[k]) if g[k] != 0 else np.float32(-0.75)
    assert (g < 0).any()
    return g


def _chamfer_inputs(case):
    B, n, m, kind = case
    rng = np.random.default_rng(1000 + n + 7 * m)
    a = rng.standard_normal((B, n, 3)).astype(np.float32)
    b = rng.standard_normal((B, m, 3)).astype(np.float32)
    if kind == "grid":                         # a 1/8 grid: ties in the nearest-neighbour search and long lists of points sharing a partner
        a, b = (np.round(a * 8) / 8).astype(np.float32), (np.round(b * 8) / 8).astype(np.float32)
    if kind == "same":
        b = a.copy()
    return a, b, _upstream(rng, (B, n)), _upstream(rng, (B, m))


CHAMFER = [(2, 7, 5, "plain"), (3, 160, 1024, "grid"), (2, 2048, 8192, "plain"), (1, 1, 3000, "plain"), (1, 3000, 1, "plain"), (2, 64, 64, "same")]


@pytest.mark.parametrize("case", CHAMFER, ids=lambda c: "%dx%dx%d-%s" % c)
def test_chamfer_bwd_det_has_the_restated_bits(case):
    B, n, m, kind = case
    a, b, gd1, gd2 = _chamfer_inputs(case)
    ta, tb = dev(a), dev(b)
    _, _, i1, i2 = ops.chamfer_fwd(ta, tb)
    g1, g2 = ops.chamfer_bwd(ta, tb, i1, i2, dev(gd1), dev(gd2), deterministic=True)
    n1, n2 = i1.cpu().numpy(), i2.cpu().numpy()
    w1, w2 = R.chamfer_bwd(a, b, n1, n2, gd1, gd2)
    same(g1, w1, "g1")
    same(g2, w2, "g2")
    if kind == "same":
        assert not g1.any() and not g2.any()          # every distance zero: every term is +-0, every sum +0.0
        assert not np.signbit(g1.cpu().numpy()).any()
    # where a target has at most one foreign term, the atomic kernels (LDS form up to n + m = 5,461, global form beyond) have these bits too
    h1, h2 = ops.chamfer_bwd(ta, tb, i1, i2, dev(gd1), dev(gd2))
    few1, few2 = R.foreign_counts(n2, n) <= 1, R.foreign_counts(n1, m) <= 1
    assert few1.any() or few2.any()
    assert np.array_equal(bits(h1)[few1], bits(g1)[few1]) and np.array_equal(bits(h2)[few2], bits(g2)[few2])
    if kind == "grid":
        assert R.foreign_counts(n2, n).max() >= 3     # the case does hold long lists


GROUP = [(2, 40, 8, 8, "rand"), (3, 1096, 64, 32, "rand"), (2, 2048, 128, 32, "rand"), (1, 16, 64, 32, "equal")]


@pytest.mark.parametrize("case", GROUP, ids=lambda c: "%dx%dx%dx%d-%s" % c)
def test_group_bwd_det_has_the_restated_bits(case):
    B, N, G, K, kind = case
    rng = np.random.default_rng(N + G)
    idx = np.full((B, G, K), 5, np.int64) if kind == "equal" else rng.integers(0, N // 2 + 1, (B, G, K)).astype(np.int64)   # the upper half: unreferenced
    go = _upstream(rng, (B, G, K, 3))
    wx, wc = R.group_bwd(go, idx, N)
    for need_xyz, need_center in ((True, True), (True, False), (False, True)):
        gx, gc = ops.group_bwd(dev(go), dev(idx), N, need_xyz=need_xyz, need_center=need_center, deterministic=True)
        assert (gx is None) == (not need_xyz) and (gc is None) == (not need_center)
        if need_xyz:
            same(gx, wx, "grad_xyz")
            untouched = gx.cpu().numpy()[:, N // 2 + 1:] if kind != "equal" else gx.cpu().numpy()[:, 6:]
            assert untouched.size and not untouched.any() and not np.signbit(untouched).any()         # rows nobody references: +0.0
        if need_center:
            same(gc, wc, "grad_center")
    ax, ac = ops.group_bwd(dev(go), dev(idx), N)                                      # the atomic sibling: the same sums up to order
    few = np.stack([np.bincount(r.reshape(-1), minlength=N) for r in idx]) <= 2       # (two addends commute exactly)
    assert np.array_equal(bits(ax)[few], bits(wx)[few]) and torch.equal(ac.cpu(), torch.from_numpy(wc))


@pytest.mark.parametrize("case", [(2, 3, 50, 16), (2, 384, 128, 64)], ids=lambda c: "%dx%dx%dx%d" % c)
def test_gather_bwd_det_has_the_restated_bits(case):
    B, C, N, M = case
    rng = np.random.default_rng(C + M)
    idx = rng.integers(0, max(2, M // 3), (B, M)).astype(np.int32)                    # drawn with repetition
    go = _upstream(rng, (B, C, M))
    got = ops.gather_bwd(dev(go), dev(idx), N, deterministic=True)
    same(got, R.gather_bwd(go, idx, N), "grad_feat")
    assert torch.allclose(ops.gather_bwd(dev(go), dev(idx), N), got, rtol=1e-4, atol=1e-4)


def test_fps_gather_bwd_det_has_the_restated_bits():
    B, M, N = 2, 8, 20
    rng = np.random.default_rng(5)
    idx = np.array([[3, 3, 3, -1, 25, 0, 19, 3], [7, 20, 7, 7, 1, 7, -5, 7]], np.int32)       # repeated and out-of-range indices
    g = _upstream(rng, (B, M, 3))
    same(ops.fps_gather_bwd(dev(g), dev(idx), N, deterministic=True), R.fps_gather_bwd(g, idx, N), "g_xyz")


def test_gather_bwd_det_at_the_edges_of_the_shared_body():
    """5 channels (a second channel group with one live channel), 257 targets (a second tile with one live lane), 1,027 sources (a second
    chunk of three), keys of -1 and of N.  deterministic=True only: the atomic sibling does not range-check."""
    B, C, N, M = 2, 5, 257, 1027
    rng = np.random.default_rng(C + N + M)
    idx = R.edge_indices(rng, B, M, N).astype(np.int32)
    go = R.mixed_upstream(rng, (B, C, M))
    want = R.gather_bwd(go, idx, N)
    assert not np.array_equal(bits(want), bits(R.gather_bwd(go, idx, N, reverse=True)))           # the order is visible
    same(ops.gather_bwd(dev(go), dev(idx), N, deterministic=True), want, "grad_feat")


def test_fps_gather_bwd_det_at_the_edges_of_the_shared_body():
    """the (.., 3)-row kernel with int32 indices: two tiles, two chunks, keys of -1 and of N"""
    B, N, M = 2, 257, 1027
    rng = np.random.default_rng(N + M)
    idx = R.edge_indices(rng, B, M, N).astype(np.int32)
    g = R.mixed_upstream(rng, (B, M, 3))
    want = R.fps_gather_bwd(g, idx, N)
    assert not np.array_equal(bits(want), bits(R.fps_gather_bwd(g, idx, N, reverse=True)))
    same(ops.fps_gather_bwd(dev(g), dev(idx), N, deterministic=True), want, "g_xyz")


def test_fps_gather_bwd_det_beyond_the_grid_of_16384_workgroups():
    """16,390 clouds of two points are 16,390 (cloud, tile) items: the last six are reached by the grid-stride loop alone.  With two
    sources per cloud no order can show (two addends commute exactly), so this case is not asked to: it checks that every item is
    served (the output is torch.empty: an unserved item keeps whatever was there)."""
    B, N, M = 16390, 2, 2
    rng = np.random.default_rng(B)
    idx = rng.integers(0, N, (B, M)).astype(np.int32)
    g = R.mixed_upstream(rng, (B, M, 3))
    want = R.fps_gather_bwd(g, idx, N)
    assert want[16384:].any()
    same(ops.fps_gather_bwd(dev(g), dev(idx), N, deterministic=True), want, "g_xyz")


@pytest.mark.parametrize("case", [(2, 200, 130), (2, 1024, 1024), (2, 50, 70)], ids=lambda c: "%dx%dx%d" % c)
def test_emd_matchcost_det_sums_the_tiles_in_order(case):
    B, n, m = case
    rng = np.random.default_rng(n)
    a, b = dev(rng.random((B, n, 3)).astype(np.float32)), dev(rng.random((B, m, 3)).astype(np.float32))
    match = ops.emd_approxmatch(a, b)
    got = ops.emd_matchcost(a, b, match, deterministic=True)
    # p_t: the existing operator on each 64-point slice of xyz1 with the matching slice of match (one tile, one addition to zero)
    parts = [ops.emd_matchcost(a[:, t:t + 64].contiguous(), b, match[:, :, t:t + 64].contiguous()).cpu().numpy() for t in range(0, n, 64)]
    same(got, R.ordered_sum(np.stack(parts, -1)), "cost")
    if n <= 64:
        same(got, ops.emd_matchcost(a, b, match), "cost vs the atomic sibling")
    else:
        assert torch.allclose(got, ops.emd_matchcost(a, b, match), rtol=1e-5, atol=0)


def test_det_entry_points_replay_from_a_graph_bit_for_bit_and_issue_no_memset():
    sys.path[:0] = [os.path.join(ROOT, "tools")]
    from memset_census import memsets_of
    torch.manual_seed(3)
    y1, y2 = torch.rand(2, 2048, 3, device='cuda'), torch.rand(2, 8192, 3, device='cuda')
    _, _, i1, i2 = ops.chamfer_fwd(y1, y2)
    gd1, gd2 = torch.randn(2, 2048, device='cuda'), torch.randn(2, 8192, device='cuda')
    go = torch.randn(2, 128, 32, 3, device='cuda')
    gi = torch.randint(0, 2048, (2, 128, 32), device='cuda')

    def both():
        return ops.chamfer_bwd(y1, y2, i1, i2, gd1, gd2, deterministic=True) + ops.group_bwd(go, gi, 2048, deterministic=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert not memsets_of(both)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = both()
    for k in range(3):                                   # fresh inputs copied into the static buffers before every replay
        gen = torch.Generator(device='cuda').manual_seed(10 + k)
        y1.copy_(torch.rand(y1.shape, device='cuda', generator=gen)); y2.copy_(torch.rand(y2.shape, device='cuda', generator=gen))
        n1, n2 = ops.chamfer_fwd(y1, y2)[2:]
        i1.copy_(n1); i2.copy_(n2)
        gd1.copy_(torch.randn(gd1.shape, device='cuda', generator=gen)); gd2.copy_(torch.randn(gd2.shape, device='cuda', generator=gen))
        go.copy_(torch.randn(go.shape, device='cuda', generator=gen))
        gi.copy_(torch.randint(0, 2048, gi.shape, device='cuda', generator=gen))
        g.replay()
        torch.cuda.synchronize()
        eager = both()
        for r, e in zip(out, eager):
            assert torch.equal(r.view(torch.int32), e.view(torch.int32)), k
    same(out[0], R.chamfer_bwd(y1.cpu().numpy(), y2.cpu().numpy(), i1.cpu().numpy(), i2.cpu().numpy(), gd1.cpu().numpy(), gd2.cpu().numpy())[0], "replayed g1")


def test_autograd_takes_the_det_entry_point_only_under_the_mode(monkeypatch):
    called = []
    real = ops._call

    def spy(device, name, *args):
        called.append(name)
        return real(device, name, *args)
    monkeypatch.setattr(ops, "_call", spy)
    rng = np.random.default_rng(9)
    a, b = (np.round(rng.standard_normal((2, 96, 3)) * 4) / 4).astype(np.float32), (np.round(rng.standard_normal((2, 300, 3)) * 4) / 4).astype(np.float32)
    a, b = a + np.float32(0.03), b                        # (no zero distance: the L1 factor is 1 / sqrt(d))
    with HF.deterministic():
        ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
        HF.chamfer_loss(ta, tb).backward()
    assert "upp_chamfer_bwd_det" in called and "upp_chamfer_bwd" not in called
    d1, d2, i1, i2 = ops.chamfer_fwd(dev(a), dev(b))
    _, fac1, fac2 = ops.chamfer_loss(d1, d2, True)
    w1, w2 = R.chamfer_bwd(a, b, i1.cpu().numpy(), i2.cpu().numpy(), fac1.cpu().numpy(), fac2.cpu().numpy())
    same(ta.grad, w1, "d loss / d xyz1")
    same(tb.grad, w2, "d loss / d xyz2")
    del called[:]
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    HF.chamfer_loss(ta, tb).backward()
    assert "upp_chamfer_bwd" in called and "upp_chamfer_bwd_det" not in called
