"""pytorch3d.ops.knn_points / knn_gather on the GPU (include/upp_hip.h "the pytorch3d.ops surface"): the forward bit for bit against the
numpy restatement (tests/_knn_points_reference.py) on lattice inputs, the neighbour lists of upp_knn at D = 3, random inputs against
float64, gradients inside a bound computed per element, the deterministic scatter bit for bit, and forward + backward in one captured
graph.  Run on the GPU box with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import _det_reference as D
import _knn_points_reference as R
from upp_hip import ops
import upp_hip.functional as HF
import pytorch3d.ops as P3

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def ragged(N, P1, P2, K, seed):
    """lengths1 with an entry beyond P1 (clamped), lengths2 with an empty cloud and one shorter than K."""
    l1 = R.ragged_lengths(N, P1, seed)
    l1[N - 1] = P1 + 2
    l2 = R.ragged_lengths(N, P2, seed + 1, special=(0, max(1, min(K, P2) - 1)))
    return l1, l2


@functools.lru_cache(maxsize=None)
def lattice(case):
    N, P1, P2, D, K = case
    return R.lattice_case(N, P1, P2, D, seed=sum(case))


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("case", R.FORWARD_GRID)
def test_forward_equals_the_restatement_bit_for_bit_on_lattice_inputs(case, norm):
    N, P1, P2, D, K = case
    p1, p2 = lattice(case)
    a, b = dev(p1), dev(p2)
    l1, l2 = ragged(N, P1, P2, K, seed=P1 + P2)
    for lengths1, lengths2, given1, given2 in ((None, None, None, None), (l1, l2, dev(l1), l2.tolist())):       # a device tensor, a host list
        wd, wi, wn = R.knn_points(p1, p2, lengths1, lengths2, norm, K)
        got = P3.knn_points(a, b, given1, given2, norm=norm, K=K, return_nn=True)
        assert got.idx.dtype == torch.int64 and got.dists.shape == (N, P1, K) and got.knn.shape == (N, P1, K, D)
        np.testing.assert_array_equal(got.idx.cpu().numpy(), wi)
        np.testing.assert_array_equal(bits(got.dists.cpu().numpy()), bits(wd))
        np.testing.assert_array_equal(bits(got.knn.cpu().numpy()), bits(wn))
        if lengths2 is not None:                                       # the padding really is there: an empty cloud, a short list, dead rows
            assert not wd[0].any() and not wi[0].any() and not wn[0].any()
        assert P3.knn_points(a, b, given1, given2, norm=norm, K=K).knn is None


def test_lengths_are_clamped_on_the_device():
    case = (3, 5, 65, 3, 4)
    p1, p2 = R.lattice_case(*case[:4], seed=3)
    l1, l2 = np.array([-4, 9, 2], np.int64), np.array([1000, -1, 3], np.int64)
    wd, wi, wn = R.knn_points(p1, p2, l1, l2, 2, 4)
    got = P3.knn_points(dev(p1), dev(p2), dev(l1), dev(l2), K=4, return_nn=True)
    np.testing.assert_array_equal(got.idx.cpu().numpy(), wi)
    np.testing.assert_array_equal(bits(got.dists.cpu().numpy()), bits(wd))
    np.testing.assert_array_equal(bits(got.knn.cpu().numpy()), bits(wn))
    assert not wi[0].any() and not wi[1].any() and (wi[2, :2, :3] < 3).all() and not wi[2, :, 3].any() and not wi[2, 2:].any()


@pytest.mark.parametrize("kind", ["lattice", "dup"])
@pytest.mark.parametrize("shape", [(2, 1000, 72, 4), (2, 4097, 5, 8), (2, 100, 7, 50)])
def test_at_three_dimensions_the_lists_are_upp_knns(shape, kind):
    from test_gpu_parity import clouds
    B, N, Q, K = shape
    ref = clouds(B, N, kind, seed=N + Q + K)
    qry = np.ascontiguousarray(ref[:, np.random.default_rng(1).permutation(N)[:Q]])
    r, q = dev(ref), dev(qry)
    _, idx, _ = ops.knn(r, q, K)
    got = P3.knn_points(q, r, K=K)
    assert torch.equal(got.idx, idx)
    wd, wi, _ = R.knn_points(qry, ref, None, None, 2, K)               # the sequential-fma restatement (these clouds are not exact in f32)
    np.testing.assert_array_equal(got.idx.cpu().numpy(), wi)
    np.testing.assert_array_equal(bits(got.dists.cpu().numpy()), bits(wd))


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("case", R.RANDOM_GRID)
def test_random_inputs_against_float64(case, norm):
    N, P1, P2, D, K, seed = case
    p1, p2 = R.random_case(N, P1, P2, D, seed)
    ok = R.separated_queries(p1, p2, K, norm)
    assert 1.0 - ok.mean() <= 0.01                                     # (also asserted on the host: tests/test_knn_points_host.py)
    wd, wi, _ = R.knn_points(p1.astype(np.float64), p2.astype(np.float64), None, None, norm, K,
                             dist=lambda q, p, n: R.distances64(q, p, n))
    got = P3.knn_points(dev(p1), dev(p2), norm=norm, K=K)
    gi, gd = got.idx.cpu().numpy(), got.dists.cpu().numpy().astype(np.float64)
    d64 = np.stack([np.take_along_axis(R.distances64(p1[n], p2[n], norm), wi[n], 1) for n in range(N)])
    np.testing.assert_array_equal(gi[ok], wi[ok])
    # D * 2^-24 relative: D sequential roundings on non-negative terms
    err = np.abs(gd - d64)[ok] / d64[ok]
    print("knn_points random", case, "norm", norm, "excluded", 1.0 - ok.mean(), "max rel err / 2^-24", err.max() / U24)
    assert err.max() <= D * U24


def _float64_gradients(p1, p2, idx, live, wd, wn, norm):
    """float64 autograd of the torch formulation with the indices held fixed -> (g1, g2) and, per element, the (m + 2) 2^-24 sum |terms|
    bounds (m = the number of terms that reach the element)."""
    a = torch.from_numpy(p1.astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(p2.astype(np.float64)).requires_grad_(True)
    N, P1, K = idx.shape
    D, P2 = p1.shape[2], p2.shape[1]
    ix = torch.from_numpy(idx)
    lv = torch.from_numpy(live)
    nb = torch.gather(b.unsqueeze(1).expand(-1, P1, -1, -1), 2, ix.unsqueeze(-1).expand(-1, -1, -1, D))
    diff = a.unsqueeze(2) - nb
    dist = (diff * diff).sum(-1) if norm == 2 else diff.abs().sum(-1)
    loss = (torch.from_numpy(wd.astype(np.float64)) * dist)[lv].sum()
    if wn is not None:
        loss = loss + (torch.from_numpy(wn.astype(np.float64)) * nb)[lv].sum()
    g1, g2 = torch.autograd.grad(loss, (a, b))
    d = diff.detach().numpy()
    t = (2.0 * wd[..., None] * d if norm == 2 else np.sign(d) * wd[..., None]) * live[..., None]
    b1 = (live.sum(2)[..., None] + 2.0) * U24 * np.abs(t).sum(2)
    mag, cnt = np.zeros((N, P2, D)), np.zeros((N, P2, 1))
    for n in range(N):
        np.add.at(mag[n], idx[n][live[n]], np.abs(t[n][live[n]]))
        np.add.at(cnt[n], idx[n][live[n]], 1.0)
        if wn is not None:
            np.add.at(mag[n], idx[n][live[n]], np.abs(wn[n][live[n]].astype(np.float64)))
            np.add.at(cnt[n], idx[n][live[n]], 1.0)
    return g1.numpy(), g2.numpy(), b1, (cnt + 2.0) * U24 * mag


GRAD_CASES = [((2, 72, 100, 3, 4), None, None), ((3, 65, 33, 5, 8), (65, 40, 1), (33, 5, 20))]


@pytest.mark.parametrize("return_nn", [False, True])
@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("case,l1,l2", GRAD_CASES)
def test_gradients_inside_the_rounding_bound_and_deterministic_bits(case, l1, l2, norm, return_nn):
    N, P1, P2, D, K = case
    p1, p2 = R.random_case(N, P1, P2, D, seed=21)
    g = np.random.default_rng(22)
    wd = g.standard_normal((N, P1, K)).astype(np.float32)
    wn = g.standard_normal((N, P1, K, D)).astype(np.float32) if return_nn else None
    len1 = None if l1 is None else dev(np.array(l1, np.int64))
    len2 = None if l2 is None else dev(np.array(l2, np.int64))
    live = R.live_slots(N, P1, K, P2, l1, l2)

    def run(det):
        a, b = dev(p1).requires_grad_(True), dev(p2).requires_grad_(True)
        with HF.deterministic(det):
            out = P3.knn_points(a, b, len1, len2, norm=norm, K=K, return_nn=return_nn)
            assert not out.idx.requires_grad and out.dists.requires_grad and (out.knn is None or out.knn.requires_grad)
            outs, grads = [out.dists], [dev(wd)]
            if return_nn:
                outs.append(out.knn); grads.append(dev(wn))
            ga, gb = torch.autograd.grad(outs, (a, b), grads)
        return out.idx.cpu().numpy(), ga.cpu().numpy(), gb.cpu().numpy()

    idx, ga, gb = run(False)
    w1, w2, b1, b2 = _float64_gradients(p1, p2, idx, live, wd, wn, norm)
    for name, got, want, bound in (("g_p1", ga, w1, b1), ("g_p2", gb, w2, b2)):
        over = np.abs(got - want) - bound
        print("knn_points grad", case, norm, return_nn, name, "worst |err| / bound", (np.abs(got - want) / np.maximum(bound, 1e-300)).max())
        assert (over <= 0).all(), name
    # deterministic mode: the restatement's bits, twice
    idx_d, ga_d, gb_d = run(True)
    assert np.array_equal(idx_d, idx)
    r1, t = R.knn_points_bwd(p1, p2, idx, wd, l1, l2, norm)
    want = R.scatter_add_det(t, idx, P2, l1, l2, negate=True)
    if return_nn:
        want = (want + R.scatter_add_det(wn, idx, P2, l1, l2)).astype(np.float32)
    np.testing.assert_array_equal(bits(ga_d), bits(r1))
    np.testing.assert_array_equal(bits(ga), bits(r1))                  # g_p1 has one order in either mode
    np.testing.assert_array_equal(bits(gb_d), bits(want))
    assert (np.abs(gb_d - w2) <= b2).all()
    _, ga_2, gb_2 = run(True)
    assert np.array_equal(bits(ga_2), bits(ga_d)) and np.array_equal(bits(gb_2), bits(gb_d))


@pytest.mark.parametrize("lengths", [None, (8, 3, 0)])
def test_knn_gather_and_its_gradient(lengths):
    N, L, M, K, U = 3, 65, 33, 8, 7
    g = np.random.default_rng(31)
    x = g.standard_normal((N, M, U)).astype(np.float32)
    idx = g.integers(0, M, (N, L, K))
    go = g.standard_normal((N, L, K, U)).astype(np.float32)
    lens = None if lengths is None else dev(np.array(lengths, np.int64))
    want = R.knn_gather(x, idx, lengths)
    total, bound = R.scatter_bound(go, idx, M, None, lengths)
    res = {}
    for det in (False, True, True):
        xs = dev(x).requires_grad_(True)
        with HF.deterministic(det):
            out = P3.knn_gather(xs, dev(idx), lens)
            (gx,) = torch.autograd.grad(out, xs, dev(go))
        np.testing.assert_array_equal(bits(out.detach().cpu().numpy()), bits(want))
        gx = gx.cpu().numpy()
        assert (np.abs(gx - total) <= bound).all()
        if det:
            np.testing.assert_array_equal(bits(gx), bits(R.scatter_add_det(go, idx, M, None, lengths)))
            res.setdefault("det", []).append(gx)
    assert np.array_equal(bits(res["det"][0]), bits(res["det"][1]))


@pytest.mark.parametrize("negate", [False, True])
def test_scatter_add_det_at_the_edges_of_the_shared_body(negate):
    """5 columns (a second column group with one live column), 257 target rows (a second tile with one live lane), 1,027 sources (a second
    chunk of three), keys of -1 and of M, one cloud with every slot and one with rows and slots cut short.  deterministic=True only: the
    atomic sibling's index check is not under test here."""
    N, L, K, U, M = 2, 79, 13, 5, 257
    g = np.random.default_rng(L * K)
    src = D.mixed_upstream(g, (N, L, K, U))
    idx = D.edge_indices(g, N, L * K, M).reshape(N, L, K)
    rows, slots = (79, 40), (13, 5)
    want = R.scatter_add_det(src, idx, M, rows, slots, negate=negate)
    assert not np.array_equal(bits(want), bits(R.scatter_add_det(src, idx, M, rows, slots, negate=negate, reverse=True)))   # the order is visible
    got = ops.knn_scatter_add(dev(src), dev(idx), M, dev(np.array(rows, np.int64)), dev(np.array(slots, np.int64)), negate=negate, deterministic=True)
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(want))


def test_forward_and_backward_in_one_captured_graph_replay_the_eager_bits():
    """Deterministic mode, ragged lengths on the device: nothing in the step reads the device or fills memory with a memset node (one
    would replay correctly once), so every one of three replays -- outputs scribbled over in between -- has the eager bits."""
    N, P1, P2, D, K = 3, 65, 33, 5, 8
    p1, p2 = R.random_case(N, P1, P2, D, seed=41)
    g = np.random.default_rng(42)
    a, b = dev(p1).requires_grad_(True), dev(p2).requires_grad_(True)
    wd, wn = dev(g.standard_normal((N, P1, K)).astype(np.float32)), dev(g.standard_normal((N, P1, K, D)).astype(np.float32))
    len1, len2 = dev(np.array([65, 40, 1], np.int64)), dev(np.array([33, 5, 20], np.int64))

    def step(det=True):
        with HF.deterministic(det):
            out = P3.knn_points(a, b, len1, len2, K=K, return_nn=True)
            ga, gb = torch.autograd.grad([out.dists, out.knn], (a, b), [wd, wn])
        return out.dists.detach(), out.idx, out.knn.detach(), ga, gb

    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(3):
        for t in out:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)
    # the atomic scatter zeroes its output with a kernel of the library: captured and replayed, it still starts from zero
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        out2 = step(False)
    for _ in range(3):
        for t in out2:
            t.fill_(-7)
        graph2.replay()
        torch.cuda.synchronize()
        for got, want in zip(out2[:4], eager[:4]):
            assert torch.equal(got, want)
        assert torch.allclose(out2[4], eager[4], rtol=1e-4, atol=1e-5)      # (atomics: any order; -7 left behind would show)


def test_the_references_call_shape_equals_the_fused_grouping():
    """models/Point_MAE_pretask_dev.py:680: knn_points(noise (B,72,3), partial (B,1024,3), K=4, return_nn=True); nn - noise is what
    ops.knn hands the repository's own pre-task model as `neigh`."""
    from test_gpu_parity import clouds
    partial = clouds(4, 1024, "ball", 9)
    noise = (partial[:, :72] + np.random.default_rng(5).normal(0, 0.02, (4, 72, 3))).astype(np.float32)
    a, b = dev(noise), dev(partial)
    got = P3.knn_points(a, b, K=4, return_nn=True)
    dist, idx, neigh = ops.knn(b, a, 4, want_dist=True, want_neigh=True)
    assert torch.equal(got.idx, idx)
    assert torch.equal(got.knn - a[:, :, None], neigh)
    assert torch.equal(got.dists.sqrt(), dist)


def test_limits_are_errors_that_name_the_limit():
    x = torch.rand(2, 8, 33, device="cuda")
    with pytest.raises(RuntimeError, match="D <= 32"):
        P3.knn_points(x, x, K=2)
    y = torch.rand(2, 80, 3, device="cuda")
    with pytest.raises(RuntimeError, match="K <= 64"):
        P3.knn_points(y, y, K=65)
    with pytest.raises(ValueError):
        P3.knn_points(y, y, norm=3)
    with pytest.raises(ValueError):
        P3.knn_points(y, y[:1])
    with pytest.raises(ValueError):
        P3.knn_points(y, x)
    assert P3.knn_points(y, y, K=64, version=3, return_sorted=False).idx.shape == (2, 80, 64)
