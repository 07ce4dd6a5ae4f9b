"""CPU tests of tests/_loss_reference.py, the float64 arbiter of tests/test_gpu_losses.py: the float64 auction against the C oracle at the
parity test's tolerances and against the reference's known answer, the hand-written gradients against torch autograd in float64, the
Chamfer functions against the oracle's bit-exact kernels restatement, and the one-step judge of the EMD factors on a float32
restatement of the auction for every case the GPU file runs (the judge must accept what a correct float32 kernel would leave behind).

The input generators of the GPU file live here too, with the assertions that make them what they claim: a different cloud per sample,
lattice coordinates whose squared distances are exact in float32, duplicated halves, a given match with exact zeros and one dominant
entry per row, upstream gradients of mixed sign with exact zeros."""
import numpy as np
import pytest
import torch

import _loss_reference as R
import _seeded
import oracle as O

F32, F64 = torch.float32, torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ============================================================================================== generators
KINDS = ("ball", "lattice", "dup")


def clouds(B, N, kind, seed):
    """(B, N, 3) float32, a different cloud per sample.
         ball      points of the unit ball
         lattice   coordinates on multiples of 0.25 in [-0.5, 0.75]: every difference, square and sum of three squares is exact in
                   float32 (multiples of 1/16 below 2^24 / 16), many pairs coincide (d = 0) and many distances tie
         dup       the second half of a cloud repeats the first"""
    g = _gen(seed)
    if kind == "ball":
        p = _seeded.unit_ball_clouds(B, N, seed=seed).clone() if N >= 4 else torch.rand(B, N, 3, generator=g) - 0.5
    elif kind == "lattice":
        p = torch.randint(0, 6, (B, N, 3), generator=g).float() * 0.25 - 0.5
    elif kind == "dup":
        p = torch.rand(B, N, 3, generator=g) - 0.5
        p[:, N - N // 2:] = p[:, :N // 2]
    else:
        raise ValueError(kind)
    return p.contiguous()


# the smallest shapes that reach each edge of the EMD kernels: one point, one 64-lane tile and its neighbours, B x tiles that is not /
# is a multiple of the 8 XCDs, n != m either way (multiL / multiR > 1), and the 1,024-point LDS tile crossed by one point, by a short
# second tile (6 and 76 points: three of the four waves get an empty or short segment), and twice
EMD_SHAPES = [(3, 1, 1), (2, 1, 70), (2, 70, 1), (3, 63, 65), (2, 64, 64), (2, 96, 32), (2, 40, 100), (2, 100, 40), (2, 300, 300), (8, 64, 130),
              (2, 1025, 64), (2, 64, 1025), (1, 1030, 1100), (1, 2049, 1024), (1, 1024, 2049)]
EMD_BALL_ONLY = {(1, 2049, 1024), (1, 1024, 2049)}
EMD_CASES = [(B, n, m, kind) for (B, n, m) in EMD_SHAPES for kind in KINDS if kind == "ball" or (B, n, m) not in EMD_BALL_ONLY]
# emd_grad2_kernel holds four rows of match per workgroup, emd_grad1 / the cost 64 points of xyz1 per workgroup
COST_SHAPES = EMD_SHAPES + [(2, 65, 5), (2, 63, 6), (2, 127, 7), (3, 129, 9)]


def emd_pair(B, n, m, kind, seed=0):
    return clouds(B, n, kind, 1000 * n + m + seed), clouds(B, m, kind, 1000 * m + n + 7 + seed)


# The one case whose first draw missed the one-step bound by rounding alone (tests/test_gpu_losses.py, "A case that missed"): drawn again.
EMD_RESEED = {(2, 64, 64, "ball"): 1}


def emd_case(B, n, m, kind):
    """The clouds of one entry of EMD_CASES."""
    return emd_pair(B, n, m, kind, seed=EMD_RESEED.get((B, n, m, kind), 0))


def given_match(B, n, m, seed):
    """(B, m, n) float32 >= 0: about a third exact zeros, one dominant entry (+ 8) per row l at a column that moves with l, so that a
    dropped or doubled term of any sum over it shows."""
    g = _gen(seed)
    mt = torch.rand(B, m, n, generator=g)
    mt = torch.where(torch.rand(B, m, n, generator=g) < 0.33, torch.zeros_like(mt), mt)
    col = (torch.arange(m) * 7 + 3) % n
    mt[:, torch.arange(m), col] += 8.0
    return mt.contiguous()


def grad_cost(B):
    """(B,) float32 of mixed sign with an exact zero (from B = 2 on)."""
    return torch.tensor([-1.3, 0.0, 0.7, 2.1, -0.4, 1.9, -2.2, 0.3])[torch.arange(B) % 8].contiguous()


def mixed_grads(shape, seed):
    """Upstream gradients of mixed sign over a 1e3 spread (|g| in [1e-3, 1]) with about a tenth exact zeros."""
    g = _gen(seed)
    mag = 10.0 ** (-3.0 * torch.rand(shape, generator=g))
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -torch.ones(shape), torch.ones(shape))
    v = mag * sign
    return torch.where(torch.rand(shape, generator=g) < 0.1, torch.zeros(shape), v).contiguous()


def loss_dists(B, n, m, seed, zeros=False):
    """dist1 (B, n), dist2 (B, m) float32 > 0 (squares over four decades); zeros: a few exact 0 entries in each."""
    g = _gen(seed)
    d1 = (torch.randn(B, n, generator=g) * 0.1) ** 2 + 1e-8
    d2 = (torch.randn(B, m, generator=g) * 0.1) ** 2 + 1e-8
    if zeros:
        d1.view(-1)[::3] = 0.0
        d2.view(-1)[1::5] = 0.0
        d2.view(-1)[0] = 0.0
    return d1.contiguous(), d2.contiguous()


# ============================================================================================== the generators are what they claim
@pytest.mark.parametrize("kind", KINDS)
def test_clouds(kind):
    a, b = emd_pair(3, 70, 40, kind)
    assert a.dtype == F32 and a.shape == (3, 70, 3) and b.shape == (3, 40, 3)
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2]), "a different cloud per sample"
    if kind == "lattice":
        d32, d64 = R.sqdist(a, b, F32), R.sqdist(a, b, F64)
        assert torch.equal(d32.double(), d64), "exact in float32"
        assert int((d64 == 0).sum()) > 0, "coinciding pairs"
        for lev in R.LEVELS:
            assert torch.equal((d32 * np.float32(lev)).double(), d64 * lev), "level x d is exact too"
    if kind == "dup":
        assert torch.equal(a[:, 35:], a[:, :35]) and torch.equal(b[:, 20:], b[:, :20])
    one = clouds(2, 1, kind, 5)
    assert one.shape == (2, 1, 3) and bool(torch.isfinite(one).all())


def test_given_match_and_gradients():
    mt = given_match(2, 65, 5, 1)
    assert mt.dtype == F32 and float(mt.min()) == 0.0 and 0.2 < float((mt == 0).float().mean()) < 0.45
    assert bool(((mt >= 8).sum(2) == 1).all()), "one dominant entry per row"
    gc = grad_cost(3)
    assert float(gc.min()) < 0 < float(gc.max()) and int((gc == 0).sum()) == 1
    g = mixed_grads((2, 4000), 3)
    nz = g[g != 0].abs()
    assert float(g.min()) < 0 < float(g.max()) and int((g == 0).sum()) > 0 and float(nz.max() / nz.min()) > 300
    d1, d2 = loss_dists(3, 40, 4000, 1, zeros=True)
    assert int((d1 == 0).sum()) > 0 and int((d2 == 0).sum()) > 0 and float(d1.min()) >= 0


# ============================================================================================== Chamfer
@pytest.mark.parametrize("kind", ["ball", "lattice"])
@pytest.mark.parametrize("B,n,m", [(3, 1, 1), (2, 70, 130), (2, 130, 70)])
def test_chamfer_reference_against_the_oracle(B, n, m, kind):
    """The float64 arg-min with the lowest-index rule picks the oracle's partners (exactly on lattice clouds; on random ones wherever
    float32 does not tie), the distances at those partners are the oracle's to float32 rounding, the gradient the oracle's."""
    a, b = clouds(B, n, kind, n + 1), clouds(B, m, kind, m + 2)
    w1, w2, wi1, wi2 = O.chamfer_fwd(a.numpy(), b.numpy())
    i1, i2 = R.chamfer_select(a, b)
    assert torch.equal(i1, torch.from_numpy(wi1).long()) and torch.equal(i2, torch.from_numpy(wi2).long())
    f64 = R.chamfer(a, b, i1, i2, F64)
    if kind == "lattice":
        assert torch.equal(f64["dist1"], torch.from_numpy(w1).double()) and torch.equal(f64["dist2"], torch.from_numpy(w2).double())
    else:
        np.testing.assert_allclose(f64["dist1"].numpy(), w1, rtol=1e-6, atol=1e-7)
    gd1, gd2 = mixed_grads((B, n), 1), mixed_grads((B, m), 2)
    wg1, wg2 = O.chamfer_bwd(a.numpy(), b.numpy(), wi1, wi2, gd1.numpy(), gd2.numpy())
    g = R.chamfer_bwd(a, b, i1, i2, gd1, gd2, F64)
    for got, want in ((g["g1"], wg1), (g["g2"], wg2)):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


def test_chamfer_gradient_is_autograd_of_the_min():
    a, b = clouds(2, 33, "ball", 1).double().requires_grad_(True), clouds(2, 47, "ball", 2).double().requires_grad_(True)
    gd1, gd2 = mixed_grads((2, 33), 1).double(), mixed_grads((2, 47), 2).double()
    d = R.sqdist(a, b, F64)
    ((d.min(2).values * gd1).sum() + (d.min(1).values * gd2).sum()).backward()
    i1, i2 = R.chamfer_select(a.detach(), b.detach())
    g = R.chamfer_bwd(a.detach(), b.detach(), i1, i2, gd1, gd2, F64)
    assert float((g["g1"] - a.grad).abs().max()) <= 1e-12 and float((g["g2"] - b.grad).abs().max()) <= 1e-12


@pytest.mark.parametrize("l1", [True, False])
def test_chamfer_loss_is_the_modules_formulation(l1):
    """loss and factors against torch autograd of the reference's formulation; at d = 0 the L1 factor is +inf on both sides."""
    for zeros in (False, True):
        d1, d2 = loss_dists(3, 40, 17, 4, zeros)
        x1, x2 = d1.double().requires_grad_(True), d2.double().requires_grad_(True)
        ref = (torch.mean(torch.sqrt(x1)) + torch.mean(torch.sqrt(x2))) / 2 if l1 else torch.mean(x1) + torch.mean(x2)
        ref.backward()
        got = R.chamfer_loss(d1, d2, l1, F64)
        assert abs(float(got["loss"]) - float(ref.detach())) <= 1e-14
        for f, x in ((got["fac1"], x1), (got["fac2"], x2)):
            assert torch.equal(torch.isinf(f), torch.isinf(x.grad)) and bool((f[torch.isinf(f)] > 0).all())
            fin = torch.isfinite(f)
            assert float((f[fin] - x.grad[fin]).abs().max()) <= 1e-12 * float(f[fin].abs().max())
            assert bool(torch.isinf(f).any()) == (zeros and l1)


# ============================================================================================== EMD
@pytest.fixture(autouse=True)
def _two_threads():
    """The auction is ten levels of small element-wise operations: a wide thread pool spends its time waking up (8 threads: 1.4 s for one
    2,049 x 1,024 auction, 2 threads: 0.4 s)."""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 2))
    yield
    torch.set_num_threads(n)


def test_levels():
    assert len(R.LEVELS) == 10 and R.LEVELS[0] == -16384.0 and R.LEVELS[8] == -0.25 and R.LEVELS[9] == 0.0
    assert R.emd_multi(96, 32) == (1.0, 3.0) and R.emd_multi(40, 100) == (2.0, 1.0) and R.emd_multi(64, 64) == (1.0, 1.0)


def test_float64_auction_reproduces_the_known_answer():
    """The reference's own test (test_emd_loss.py): two points against two, cost 0.71 per sample."""
    a = torch.tensor([[[1.7, -0.1, 0.1], [0.1, 1.2, 0.3]]]).repeat(3, 1, 1)
    b = torch.tensor([[[0.3, 1.8, 0.2], [1.2, -0.2, 0.3]]]).repeat(3, 1, 1)
    r = R.emd_auction(a, b, F64)
    np.testing.assert_allclose(r["cost"].numpy(), 0.71, rtol=1e-5)
    np.testing.assert_allclose(r["match"].sum(1).numpy(), 1.0, rtol=1e-6)          # every point of xyz1 is spent in full


@pytest.mark.parametrize("B,n,m", [(3, 2, 2), (4, 64, 64), (2, 96, 32), (2, 40, 100), (2, 300, 300), (1, 1024, 1024)])
def test_float64_auction_agrees_with_the_oracle(B, n, m):
    """At the tolerances, and on the clouds, of tests/test_gpu_parity.py::test_emd_against_oracle."""
    if (n, m) == (2, 2):
        a = torch.tensor([[[1.7, -0.1, 0.1], [0.1, 1.2, 0.3]]]).repeat(3, 1, 1)
        b = torch.tensor([[[0.3, 1.8, 0.2], [1.2, -0.2, 0.3]]]).repeat(3, 1, 1)
    else:
        a, b = _seeded.unit_ball_clouds(B, n, seed=n), _seeded.unit_ball_clouds(B, m, seed=m + 1)
    wm = O.emd_approxmatch(a.numpy(), b.numpy())
    wc = O.emd_matchcost(a.numpy(), b.numpy(), wm)
    r = R.emd_auction(a, b, F64)
    if n * m <= 300 * 300:
        np.testing.assert_allclose(r["match"].numpy(), wm, rtol=1e-3, atol=2e-5)
    else:
        np.testing.assert_allclose(r["match"].numpy(), wm, rtol=1e-2, atol=2e-3)
    np.testing.assert_allclose(r["cost"].numpy(), wc, rtol=2e-5)


def test_emd_cost_gradients_are_autograd_of_the_cost():
    a, b = emd_pair(2, 65, 5, "ball")
    mt, gc = given_match(2, 65, 5, 2), grad_cost(2) + 0.5
    x, y = a.double().requires_grad_(True), b.double().requires_grad_(True)
    cost = (R.sqdist(y, x, F64) * mt.double()).sum((1, 2))
    (cost * gc.double()).sum().backward()
    r = R.emd_matchcost(a, b, mt, gc, F64)
    assert float((r["cost"] - cost.detach()).abs().max()) <= 1e-12 * float(cost.detach().abs().max())
    assert float((r["grad1"] - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert float((r["grad2"] - y.grad).abs().max()) <= 1e-12 * float(y.grad.abs().max())
    wg1, wg2 = O.emd_matchcost_grad(gc.numpy(), a.numpy(), b.numpy(), mt.numpy())
    np.testing.assert_allclose(r["grad1"].numpy(), wg1, rtol=1e-4, atol=1e-5 * np.abs(wg1).max())
    np.testing.assert_allclose(r["grad2"].numpy(), wg2, rtol=1e-4, atol=1e-5 * np.abs(wg2).max())


def one_step_errors(a, b, ratioL, ratioR, match):
    """((factors', one-step float32) error pairs of ratioL, ratioR and match) as tests/test_gpu_losses.py judges them: `ratioL`, `ratioR`,
    `match` are the judged factors (the device's there, a float32 auction's here)."""
    n, m = a.shape[1], b.shape[1]
    s64, s32 = R.emd_one_step(a, b, ratioL, ratioR, F64), R.emd_one_step(a, b, ratioL, ratioR, F32)
    got, f32 = R.emd_residuals(s64, ratioL, ratioR, n, m), R.emd_residuals(s64, s32["ratioL"], s32["ratioR"], n, m)
    scale = float(s64["match"].abs().max())
    out = {k: (float(got[k].abs().max()), float(f32[k].abs().max())) for k in ("ratioL", "ratioR")}
    out["match"] = (float((match.double() - s64["match"]).abs().max()) / scale, float((s32["match"].double() - s64["match"]).abs().max()) / scale)
    return out


@pytest.mark.parametrize("B,n,m,kind", EMD_CASES)
def test_one_step_judge_accepts_a_float32_auction(B, n, m, kind):
    """A float32 restatement of the auction that is NOT the judge's own arithmetic -- the points of both clouds in reverse order (another
    order of every sum) and the exponential as 2^(x log2 e) with the product rounded (the fast intrinsic's form) -- leaves factors that
    the one-step judge accepts at the GPU file's bound, on every case the GPU file runs."""
    a, b = emd_case(B, n, m, kind)
    r = R.emd_auction(a.flip(1), b.flip(1), F32, fast_exp=True)
    ratioL, ratioR, match = r["ratioL"].flip(2), r["ratioR"].flip(2), r["match"].flip(1, 2)
    assert bool(torch.isfinite(match).all()) and float(match.min()) >= 0.0
    for k, (e, f) in one_step_errors(a, b, ratioL, ratioR, match).items():
        print("LOSSERR host | emd_step | B=%d n=%d m=%d %s | %s | %.2e | %.2e" % (B, n, m, kind, k, e, f))
        assert e <= max(2.0 * f, 2e-6), (k, e, f)
