"""The kernels of csrc/chamfer.hip and csrc/emd.hip -- chamfer_dir, chamfer_grad / chamfer_grad_cloud and the deterministic sibling,
chamfer_loss_part / final, emd_row / col / match, the cost tile (atomic and deterministic) and emd_grad1 / grad2 -- against the float64
reference of tests/_loss_reference.py, at the edges of their parameter space: clouds of one point, the 64-lane tiles and their
neighbours, B x tiles that is and is not a multiple of the 8 XCDs, n != m either way, the 1,024-point LDS tile of the EMD kernels
crossed by one point, by a short second tile and twice, the 2,048-point tile of the Chamfer forward with an odd last tile, both sides
of upp_chamfer_bwd's dispatch edge (n + m = 5,461 | 5,462) and its grid-stride loop (B (n + m) = 524,352), the 128 x 256 stride of the
loss reduction (B n = 32,767 | 32,768 | 32,769), exact d = 0, NaN coordinates, and the wrappers' argument checks.

The bound, for every judged output of every case (tests/test_gpu_head.py, whose `judge` does the judging here):
    err(x) = max|x - f64| / max|f64|,      err(kernel) <= max(2 * err(f32), 2e-6)
where f32 is the SAME formulation run by torch in float32 on the same inputs with the selections (Chamfer partners) of the float64 run.
The EMD auction amplifies last bits (two float32 runs of it differ by up to 8e-4 of max|match|), so upp_emd_approxmatch is judged ONE
LEVEL AT A TIME from the factors it leaves in `work` (include/upp_hip.h states the layout): the remains are rebuilt in float64 from the
device's own ratioL / ratioR, and per level
    ratioR   against min(remR / (sumr + 1e-9), 1) remR, relative to multiR
    ratioL   as |ratioL suml64 - remL| / (multiL + ratioL multiR sum_l e): the plain difference is ill-conditioned wherever suml is made
             of nearly exhausted columns
    match    against sum_it e_it ratioL_it ratioR_it, relative to max|match|
(the two residuals are judged against 0; the float32 column is the same one-step recipe in float32 from the same device factors).  End
to end only what amplification cannot touch: match >= 0, row sums <= multiR (1 + 1e-5), the cost within the parity test's rtol = 2e-5 of
the float64 auction's, a second call with the same bits.  `work` and `match` are NaN-filled and guarded: an element that no workgroup
served stays NaN and fails the case.  tests/test_loss_host.py checks the judge and the generators on the CPU.

Measured on MI355X: (kernel, f32) of the case nearest its bound, per family and output (number of judged outputs).  114 tests in 4.6 s;
the slowest is the first one (0.9 s, most of it loading the library), then emd_approxmatch[2-1-70-ball] (0.18 s), [1-1030-1100-ball]
(0.11 s) and test_chamfer_bwd[96-2731-2731] (0.10 s).  The nearest any output comes to its bound is 0.92 of it.
    emd_step (123)      ratioL 4.1e-6, 2.7e-6     ratioR 1.9e-6, 1.1e-6     match 3.0e-6, 1.6e-6
    emd_cost (76)       cost 1.3e-7, 5.8e-9       cost_det 1.3e-7, 5.8e-9   grad1 4.0e-7, 1.7e-7      grad2 1.2e-7, 1.3e-7
    emd_node (2)        grad1 1.2e-7, 1.3e-7      grad2 5.6e-8, 6.0e-8
    chamfer_bwd (28)    g1 1.1e-6, 1.2e-6         g2 1.5e-6, 2.4e-6         g1_det 1.2e-6, 1.2e-6     g2_det 2.4e-6, 2.4e-6
    chamfer_fwd (40)    dist1 1.3e-7, 1.3e-7      dist2 9.7e-8, 1.9e-7      idx (excess of d64[idx] over the minimum) 0, 4.9e-8
    chamfer_loss (42)   loss 8.0e-8, 8.0e-8       fac1 8.2e-8, 8.2e-8       fac2 8.9e-8, 5.9e-8
emd_step sits at 0.8 ... 0.9 of the bound where everything else is below 0.5: ratioL at B = 2, n = 70, m = 1 (ball), ratioR at 2 x 300 x
300 (dup), match at 2 x 100 x 40 (ball).  The kernels' exponential is the fast intrinsic of the reference (v_exp_f32 of x log2 e with
the product rounded: |x| 2^-24 relative on top of torch's exp), and a level's remains carry the roundings of the levels before it.  The
deterministic Chamfer gradient and the CPU's float32 index_add_ add the same terms in the same order: equal figures.

A case that missed, by rounding alone: B = 2, n = 64, m = 64, ball with the generator's first draw gave ratioR 2.02e-6 against 9.6e-7
(bound 2e-6).  Level 4, sample 0, l = 60: there sumr < remR, the consumption is min(., 1) = 1 and ratioR IS the remain -- the figure is
the device's float32 remainR (0.310009) against its float64 reconstruction (0.310011): the sumr of levels 2, 3 and 4, each within 1e-6
of multiR, added up (per level the kernel's figure grows 3.3e-7, 1.1e-6, 2.0e-6; the float32 recipe's 7.4e-7, 7.4e-7, 8.9e-7).  No term
is wrong (a wrong term shows at 1e-3 and more: the mutants below).  Measured on 5 shapes x 8 draws, this was the one miss of 40 x 3
figures; tests/test_loss_host.py EMD_RESEED draws that case's clouds again (ratioR 1.98e-6 against 1.50e-6).  The bound is untouched.

Hypotheses of the issue, decided by this file's one run of the kernels as they are -- nothing failed, csrc/emd.hip and csrc/chamfer.hip
are unchanged:
  1. the second and later LDS tiles of emd_row / col / cost / grad1 compute the same sums as the first: HOLDS.  Every case with n or m
     above 1,024 -- (2, 1025, 64), (2, 64, 1025), (1, 1030, 1100), (1, 2049, 1024), (1, 1024, 2049) -- is inside the one-step bound and
     the cost / gradient bound, short last tiles (1, 6, 76 points: empty wave segments) included.
  2. xcd_contiguous serves every (tile, cloud) exactly once when B x tiles is not a multiple of 8: HOLDS.  No NaN is left in the
     guarded, NaN-filled work / match / cost / gradient buffers -- e.g. (3, 63, 65): 3 row, 6 column and 6 match workgroups; (2, 1025,
     64): 34 row workgroups; (1, 1030, 1100): 17 and 18 -- nor at the multiples ((8, 64, 130): 8 and 24).
  3. a NaN coordinate never disappears: HOLDS, with the deviation the issue describes.  A NaN query point of Chamfer gets dist = +inf,
     idx = 0 (the reference would give NaN), every query of the other cloud skips a NaN point; the point's own distance is non-finite
     in its own direction, ChamferDistanceL1 and L2 return a non-finite loss, the other samples keep their bits
     (test_chamfer_nan_coordinate_is_never_lost).  EMD: the cost of the poisoned sample is NaN -- atomic and deterministic --, the
     match and cost of the other samples keep their bits (test_emd_nan_coordinate_is_never_lost).  include/upp_hip.h states both.
  4. the wrappers: ops.chamfer_bwd (idx1 / idx2 / grad_dist* against (B, n) / (B, m), xyz2's batch; it no longer makes its upstream
     gradients contiguous itself: the autograd node and the `chamfer` drop-in do), ops.chamfer_loss (dist2's batch), ops.emd_matchcost
     (xyz2's batch) and ops.emd_matchcost_bwd (match's shape, grad_cost's length, xyz2's batch) now check device, dtype, contiguity and
     the exact shape of every tensor from metadata alone (test_wrappers_refuse_wrong_tensors).  Not run against the old wrappers: a
     short tensor there is a read of raw memory, not a case to provoke.  Index VALUES outside the other cloud cannot be checked from
     metadata: include/upp_hip.h says so next to upp_chamfer_bwd.

Mutants (each built from a scratch copy, run once against this file and once against the old tests of the same kernels --
tests/test_gpu_parity.py -k "emd or chamfer": 33 cases).  Value changes only; the issue expected 1 to 5 to pass the old tests:
  1. emd_row_kernel resets s3 at the top of each tile: fails 7 cases here -- every level_by_level case with m > 1,024 (the row kernel
     tiles over xyz2: n > 1,024 alone does not reach it) -- through ratioL of the next level.  Old tests: 33 pass.
  2. emd_col_kernel uses level_of(it - 1) for it >= 1: fails all 41 level_by_level cases here.  Old tests: 7 of 33 fail (every
     test_emd_against_oracle shape but 2 x 2, and the module surface): the auction with a repeated level is far outside even rtol = 1e-2.
  3. emd_match_kernel skips level 8 (-0.25): fails 21 level_by_level cases here (where the clouds still hold mass at level 8; not, for one,
     at 2 x 40 x 100, 2 x 100 x 40 or 1 x 1,030 x 1,100).  Old tests: 6 of 33 fail.
  4. emd_grad1_kernel drops the factor 2 in the last wave's segment only: fails 14 of the 19 cost-and-gradient cases (every one whose
     xyz2 gives the last wave a segment with mass in it) and the autograd node's.  Old tests: 6 of 33 fail (a missing factor 2 on a
     quarter of the terms is outside rtol = 1e-4 too).
  5. chamfer_grad_kernel does not negate the partner side for e >= 2,048 x 256: fails test_chamfer_bwd[96-2731-2731] and nothing
     else.  Old tests: 33 pass -- nothing there reaches the grid-stride loop.
  6. chamfer_loss_part_kernel uses c1 for fac2: fails 12 cases here (every test_chamfer_loss shape with n != m, both zero-distance
     cases).  Old tests: 5 of 33 fail.
So 1 and 5 are seen here alone; 2, 3, 4 and 6 are large enough for the old tolerances as well.
"""
import numpy as np
import pytest
import torch

import _loss_reference as R
import test_loss_host as G
from test_gpu_head import judge, refuse_wrong_tensors
from test_gpu_step_tail import guarded
from test_gpu_tail import _bits, gin
from upp_hip import _abi, ops

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
E_BADARG = -1
TAG = "LOSSERR"


def _judge(family, label, got, f32, f64, keys):
    judge(family, label, got, f32, f64, keys, tag=TAG)


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


# ============================================================================================== 1. EMD approxmatch, one level at a time
def run_approxmatch(a, b, off):
    """upp_emd_approxmatch on guarded, NaN-filled `work` and `match` -> the buffers carved as csrc/emd.hip's carve() does, and the inputs."""
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    x1, x2 = gin(a, off), gin(b, off)
    nwork = int(lib.upp_emd_work_floats(B, n, m))
    assert nwork == 11 * B * (n + m)
    (work, ckw), (match, ckm) = guarded(nwork, F32, off), guarded(B * m * n, F32, off)
    assert lib.upp_emd_approxmatch(p(x1), p(x2), p(match), p(work), B, n, m, st) == 0
    torch.cuda.synchronize()
    ckw(); ckm()
    o1, o2, o3 = B * n, B * (n + m), B * (n + m) + 10 * B * n
    return dict(match=match.view(B, m, n), remL=work[:o1].view(B, n), remR=work[o1:o2].view(B, m),
                ratioL=work[o2:o3].view(10, B, n), ratioR=work[o3:].view(10, B, m)), x1, x2


@pytest.mark.parametrize("B,n,m,kind", G.EMD_CASES)
def test_emd_approxmatch_level_by_level(B, n, m, kind):
    """Every level's ratioL, ratioR and the match against float64 computed from the DEVICE's own earlier factors (tests/_loss_reference.py,
    emd_one_step), so that no error is carried through the auction; end to end only what amplification cannot touch."""
    a, b = G.emd_case(B, n, m, kind)
    r, x1, x2 = run_approxmatch(a, b, 1)
    assert _finite(*r.values()), "an element of work or match that no workgroup served (or a NaN the kernels made)"
    multiL, multiR = R.emd_multi(n, m)
    s64, s32 = R.emd_one_step(x1, x2, r["ratioL"], r["ratioR"], F64), R.emd_one_step(x1, x2, r["ratioL"], r["ratioR"], F32)
    got = dict(R.emd_residuals(s64, r["ratioL"], r["ratioR"], n, m), match=r["match"])
    f32 = dict(R.emd_residuals(s64, s32["ratioL"], s32["ratioR"], n, m), match=s32["match"])
    f64 = dict(ratioL=torch.zeros_like(got["ratioL"]), ratioR=torch.zeros_like(got["ratioR"]), match=s64["match"])
    _judge("emd_step", "B=%d n=%d m=%d %s" % (B, n, m, kind), got, f32, f64, ("ratioL", "ratioR", "match"))
    # what `work` holds besides: the remains, inside [0, mass]
    assert float(r["remL"].min()) >= 0.0 and float(r["remL"].max()) <= multiL and float(r["remR"].min()) >= 0.0 and float(r["remR"].max()) <= multiR
    # end to end
    assert float(r["match"].min()) >= 0.0
    assert float(r["match"].double().sum(2).max()) <= multiR * (1 + 1e-5), "a point of xyz2 hands out more than its mass"
    want = R.emd_auction(x1, x2, F64)["cost"]
    for det in (False, True):
        cost = ops.emd_matchcost(x1, x2, r["match"].contiguous(), deterministic=det)
        np.testing.assert_allclose(cost.cpu().numpy(), want.cpu().numpy(), rtol=2e-5)
    r2, _, _ = run_approxmatch(a, b, 0)
    for k in r:
        assert _bits(r[k], r2[k]), "second call (other alignment) differs: " + k


def test_emd_approxmatch_arguments():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    x = torch.zeros(2, 4, 3, device="cuda")
    o = torch.full((2 * 4 * 4 + 11 * 2 * 8,), float("nan"), device="cuda")
    assert lib.upp_emd_approxmatch(p(x), p(x), p(o), p(o), 2, 0, 4, st) == E_BADARG
    assert lib.upp_emd_approxmatch(p(x), p(x), p(o), p(o), 2, 4, 0, st) == E_BADARG
    assert lib.upp_emd_approxmatch(p(x), p(x), p(o), p(o), 0, 4, 4, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and lib.upp_emd_work_floats(-1, 4, 4) == 0


# ============================================================================================== 2. EMD cost and gradients for a given match
COST_KEYS = ("cost", "cost_det", "grad1", "grad2")


def run_cost(c, off):
    x1, x2, mt, gc = (gin(c[k], off) for k in ("a", "b", "match", "gc"))
    g1, g2 = ops.emd_matchcost_bwd(gc, x1, x2, mt)
    return dict(cost=ops.emd_matchcost(x1, x2, mt), cost_det=ops.emd_matchcost(x1, x2, mt, deterministic=True), grad1=g1, grad2=g2)


def cost_case(B, n, m, kind):
    a, b = G.emd_pair(B, n, m, kind, seed=3)
    return dict(a=a, b=b, match=G.given_match(B, n, m, n + m), gc=G.grad_cost(B))


@pytest.mark.parametrize("B,n,m", G.COST_SHAPES)
def test_emd_cost_and_gradients(B, n, m):
    """upp_emd_matchcost (atomic), upp_emd_matchcost_det and upp_emd_matchcost_bwd: plain sums over a GIVEN match -- exact zeros, one
    dominant entry per row -- and an upstream gradient of mixed sign with an exact zero."""
    kind = G.KINDS[G.COST_SHAPES.index((B, n, m)) % 3]
    c = cost_case(B, n, m, kind)
    got, again = run_cost(c, 1), run_cost(c, 0)
    for k in ("cost_det", "grad1", "grad2"):
        assert _bits(got[k], again[k]), "second call (other alignment) differs: " + k
    d = {k: v.cuda() for k, v in c.items()}
    ref = {dt: R.emd_matchcost(d["a"], d["b"], d["match"], d["gc"], dt) for dt in (F32, F64)}
    for dt in ref:
        ref[dt]["cost_det"] = ref[dt]["cost"]
    if B >= 2:
        assert float(got["grad1"][1].abs().max()) == 0.0 and float(got["grad2"][1].abs().max()) == 0.0, "grad_cost[1] is an exact 0"
    _judge("emd_cost", "B=%d n=%d m=%d %s" % (B, n, m, kind), got, ref[F32], ref[F64], COST_KEYS)


@pytest.mark.parametrize("B,n,m", [(3, 63, 65), (2, 65, 5), (1, 1030, 1100)])
def test_emd_cost_c_entry_points_with_guarded_outputs(B, n, m):
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    c = cost_case(B, n, m, "ball")
    x1, x2, mt, gc = (gin(c[k], 1) for k in ("a", "b", "match", "gc"))
    nw = int(lib.upp_emd_matchcost_det_work_bytes(B, n, m))
    assert nw == 4 * B * ((n + 63) // 64)
    outs = {k: guarded(cnt, F32, 1) for k, cnt in (("cost", B), ("cost_det", B), ("work", nw // 4), ("grad1", B * n * 3), ("grad2", B * m * 3))}
    o = {k: v[0] for k, v in outs.items()}
    assert lib.upp_emd_matchcost(p(x1), p(x2), p(mt), p(o["cost"]), B, n, m, st) == 0
    assert lib.upp_emd_matchcost_det(p(x1), p(x2), p(mt), p(o["cost_det"]), p(o["work"]), B, n, m, st) == 0
    assert lib.upp_emd_matchcost_bwd(p(gc), p(x1), p(x2), p(mt), p(o["grad1"]), p(o["grad2"]), B, n, m, st) == 0
    torch.cuda.synchronize()
    for _, check in outs.values():
        check()
    assert _finite(*o.values()), "an element no workgroup served"
    w = run_cost(c, 0)
    for k in ("cost_det", "grad1", "grad2"):
        assert _bits(o[k].view(w[k].shape), w[k]), k
    assert torch.allclose(o["cost"], w["cost"], rtol=1e-5, atol=0)


def test_emd_autograd_node_and_module_surfaces():
    """emd.emd, extensions.emd.emd.earth_mover_distance and emd_cuda.* at (2, 96, 32): the loss is mean(cost / n1), and x.grad is
    upp_emd_matchcost_bwd of the constant 1 / (B n1), bit for bit."""
    import emd
    import emd_cuda
    from extensions.emd.emd import earth_mover_distance
    B, n, m = 2, 96, 32
    a, b = G.emd_pair(B, n, m, "ball")
    x, y = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    loss = emd.emd()(x, y)
    loss.backward()
    match = emd_cuda.approxmatch_forward(x.detach(), y.detach())
    assert _bits(match, ops.emd_approxmatch(x.detach(), y.detach())) and match.shape == (B, m, n)
    cost = emd_cuda.matchcost_forward(x.detach(), y.detach(), match)
    assert _bits(loss.detach(), (cost / n).mean())
    gc = torch.full((B,), 1.0 / B, device="cuda") / n
    g1, g2 = emd_cuda.matchcost_backward(gc, x.detach(), y.detach(), match)
    w1, w2 = ops.emd_matchcost_bwd(gc, x.detach(), y.detach(), match)
    assert _bits(g1, w1) and _bits(g2, w2) and _bits(x.grad, w1) and _bits(y.grad, w2)
    x2, y2 = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    loss2 = earth_mover_distance()(x2, y2)
    loss2.backward()
    assert _bits(loss2.detach(), loss.detach()) and _bits(x2.grad, x.grad) and _bits(y2.grad, y.grad)
    ref = R.emd_matchcost(x.detach(), y.detach(), match, gc, F64)
    ref32 = R.emd_matchcost(x.detach(), y.detach(), match, gc, F32)
    _judge("emd_node", "B=2 n=96 m=32", dict(grad1=x.grad, grad2=y.grad), ref32, ref, ("grad1", "grad2"))


# ============================================================================================== 3. Chamfer
def _gd(c, off):
    return {k: gin(c[k], off) for k in ("a", "b", "gd1", "gd2")}


BWD_SHAPES = [(1, 2731, 2730), (1, 2731, 2731), (96, 2731, 2731), (2, 4000, 1), (2, 1, 4000), (3, 1, 1), (2, 70, 130)]


@pytest.mark.parametrize("B,n,m", BWD_SHAPES)
def test_chamfer_bwd(B, n, m):
    """upp_chamfer_bwd on both sides of its dispatch edge (n + m = 5,461: the LDS kernel, 5,462: global atomics), through the grid-stride
    loop of chamfer_grad_kernel (B (n + m) = 524,352 > 2,048 x 256), with every term on one target, and its deterministic sibling.
    Lattice clouds: the partners are the float64 arg-min, legal by construction; upstream gradients of mixed sign with exact zeros.
    The second cloud sits half a lattice step (0.125) off the first: still exact in float32, many equal minima, and no pair coincides --
    on one lattice nearly every point of 2,731 has a partner at distance 0 and every term of the gradient is an exact 0."""
    a, b = G.clouds(B, n, "lattice", 10 * n + m), G.clouds(B, m, "lattice", 10 * m + n + 1) + 0.125
    c = dict(a=a, b=b, gd1=G.mixed_grads((B, n), n), gd2=G.mixed_grads((B, m), m + 1))
    i1, i2 = R.chamfer_select(a.cuda(), b.cuda())
    assert 0 <= int(i1.min()) and int(i1.max()) < m and 0 <= int(i2.min()) and int(i2.max()) < n
    t = _gd(c, 1)
    j1, j2 = gin(i1.int().cpu(), 1), gin(i2.int().cpu(), 1)
    g1, g2 = ops.chamfer_bwd(t["a"], t["b"], j1, j2, t["gd1"], t["gd2"])
    h1, h2 = ops.chamfer_bwd(t["a"], t["b"], j1, j2, t["gd1"], t["gd2"], deterministic=True)
    got = dict(g1=g1, g2=g2, g1_det=h1, g2_det=h2)
    assert float(g1.abs().max()) > 0.1 and float(g2.abs().max()) > 0.1
    ref = {}
    for dt in (F32, F64):                                     # on the CPU: one order of the float32 terms on every run
        r = R.chamfer_bwd(a, b, i1.cpu(), i2.cpu(), c["gd1"], c["gd2"], dt)
        ref[dt] = dict(g1=r["g1"].cuda(), g2=r["g2"].cuda(), g1_det=r["g1"].cuda(), g2_det=r["g2"].cuda())
    _judge("chamfer_bwd", "B=%d n=%d m=%d" % (B, n, m), got, ref[F32], ref[F64], ("g1", "g2", "g1_det", "g2_det"))


def test_chamfer_bwd_c_entry_point_with_guarded_outputs():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    for B, n, m in ((2, 70, 130), (1, 2731, 2731)):
        a, b = G.clouds(B, n, "lattice", 1), G.clouds(B, m, "lattice", 2)
        i1, i2 = R.chamfer_select(a.cuda(), b.cuda())
        t = _gd(dict(a=a, b=b, gd1=G.mixed_grads((B, n), 1), gd2=G.mixed_grads((B, m), 2)), 1)
        j1, j2 = gin(i1.int().cpu(), 1), gin(i2.int().cpu(), 1)
        for name in ("upp_chamfer_bwd", "upp_chamfer_bwd_det"):
            (g1, ck1), (g2, ck2) = guarded(B * n * 3, F32, 1), guarded(B * m * 3, F32, 1)
            assert getattr(lib, name)(p(t["a"]), p(t["b"]), p(j1), p(j2), p(t["gd1"]), p(t["gd2"]), p(g1), p(g2), B, n, m, st) == 0
            torch.cuda.synchronize()
            ck1(); ck2()
            assert _finite(g1, g2)


FWD_LATTICE = [(3, 1, 1), (3, 63, 65), (2, 70, 2049), (2, 2049, 70), (1, 130, 4099), (2, 65, 2050)]


@pytest.mark.parametrize("B,n,m", FWD_LATTICE)
def test_chamfer_fwd_is_exact_on_lattice_clouds(B, n, m):
    """Every squared distance is exact in float32 there: dist and idx equal the float64 brute force, with the lowest-index rule, no
    exclusions.  m = 2,049 and 4,099: a last LDS tile of 1 and 3 points (an odd slot past the end)."""
    a, b = G.clouds(B, n, "lattice", n + 3), G.clouds(B, m, "lattice", m + 4)
    x1, x2 = gin(a, 1), gin(b, 1)
    d1, d2, i1, i2 = ops.chamfer_fwd(x1, x2)
    w1, w2 = R.chamfer_select(x1, x2)
    f64 = R.chamfer(x1, x2, w1, w2, F64)
    assert torch.equal(i1.long(), w1) and torch.equal(i2.long(), w2)
    assert torch.equal(d1.double(), f64["dist1"]) and torch.equal(d2.double(), f64["dist2"])
    assert int((f64["dist1"] == 0).sum()) > 0 or n * m < 100, "coinciding points"


@pytest.mark.parametrize("kind", ["ball", "dup"])
@pytest.mark.parametrize("B,n,m", [(3, 1, 1), (3, 63, 65), (2, 70, 2049), (1, 2049, 130), (1, 300, 4099)])
def test_chamfer_fwd_random_clouds(B, n, m, kind):
    """dist by the bound; idx by the distance it reaches: d64[idx] - min d64 <= the same bound x max d64, no exclusions."""
    a, b = G.clouds(B, n, kind, n + 5), G.clouds(B, m, kind, m + 6)
    x1, x2 = gin(a, 1), gin(b, 1)
    d1, d2, i1, i2 = ops.chamfer_fwd(x1, x2)
    assert 0 <= int(i1.min()) and int(i1.max()) < m and 0 <= int(i2.min()) and int(i2.max()) < n
    w1, w2 = R.chamfer_select(x1, x2)
    f32, f64 = R.chamfer(x1, x2, w1, w2, F32), R.chamfer(x1, x2, w1, w2, F64)
    label = "B=%d n=%d m=%d %s" % (B, n, m, kind)
    _judge("chamfer_fwd", label, dict(dist1=d1, dist2=d2), f32, f64, ("dist1", "dist2"))
    at = R.chamfer(x1, x2, i1.long(), i2.long(), F64)                           # float64 distance to the partner the kernel chose
    for k in ("dist1", "dist2"):
        scale = float(f64[k].max())
        ef = float((f32[k].double() - f64[k]).abs().max()) / (scale if scale > 0 else 1.0)
        excess = float((at[k] - f64[k]).max()) / (scale if scale > 0 else 1.0)
        print("%s | chamfer_fwd | %s | idx of %s | %.2e | %.2e" % (TAG, label, k, excess, ef))
        assert float((at[k] - f64[k]).min()) >= 0.0 and excess <= max(2.0 * ef, 2e-6), (k, excess, ef)
    e1, e2, k1, k2 = ops.chamfer_fwd(gin(a, 0), gin(b, 0))
    assert _bits(d1, e1) and _bits(d2, e2) and torch.equal(i1, k1) and torch.equal(i2, k2)


def test_chamfer_fwd_c_entry_point_with_guarded_outputs():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    for B, n, m in ((3, 63, 65), (1, 130, 4099)):
        a, b = G.clouds(B, n, "ball", 1), G.clouds(B, m, "ball", 2)
        x1, x2 = gin(a, 1), gin(b, 1)
        outs = [guarded(B * n, F32, 1), guarded(B * m, F32, 1), guarded(B * n, torch.int32, 1), guarded(B * m, torch.int32, 1)]
        d1, d2, i1, i2 = (o[0] for o in outs)
        i1.fill_(-7); i2.fill_(-7)
        assert lib.upp_chamfer_fwd(p(x1), p(x2), p(d1), p(d2), p(i1), p(i2), B, n, m, st) == 0
        torch.cuda.synchronize()
        for _, check in outs:
            check()
        w = ops.chamfer_fwd(x1, x2)
        assert _bits(d1.view(B, n), w[0]) and _bits(d2.view(B, m), w[1]) and torch.equal(i1.view(B, n), w[2]) and torch.equal(i2.view(B, m), w[3])


LOSS_SHAPES = [(1, 32767, 327), (1, 32768, 328), (1, 32769, 33), (3, 40, 4000), (7, 4681, 47), (1, 1, 1)]      # 7 x 4,681 = 32,767


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("B,n,m", LOSS_SHAPES)
def test_chamfer_loss(B, n, m, l1):
    """upp_chamfer_loss: loss, fac1 and fac2 for L1 and L2 around the 128 x 256 stride of chamfer_loss_part_kernel (B n = 32,767 / 32,768 /
    32,769), with n and m a factor of 100 apart either way."""
    d1, d2 = G.loss_dists(B, n, m, n + m)
    t1, t2 = gin(d1, 1), gin(d2, 1)
    loss, fac1, fac2 = ops.chamfer_loss(t1, t2, l1)
    l2_, f1_, f2_ = ops.chamfer_loss(gin(d1, 0), gin(d2, 0), l1)
    assert _bits(loss, l2_) and _bits(fac1, f1_) and _bits(fac2, f2_), "second call (other alignment) differs"
    ref = {dt: R.chamfer_loss(t1, t2, l1, dt) for dt in (F32, F64)}
    _judge("chamfer_loss", "B=%d n=%d m=%d %s" % (B, n, m, "L1" if l1 else "L2"), dict(loss=loss.view(()), fac1=fac1, fac2=fac2), ref[F32], ref[F64],
           ("loss", "fac1", "fac2"))


@pytest.mark.parametrize("l1", [True, False])
def test_chamfer_loss_at_exact_zero_distances(l1):
    """d = 0: under L1 d sqrt(d) / d d = +inf, as torch.sqrt's backward gives; the kernel writes the same +inf, at the same entries, and the
    finite ones stay inside the bound.  Equality with the torch formulation (autograd), non-finite entries included."""
    B, n, m = 3, 40, 4000
    d1, d2 = G.loss_dists(B, n, m, 5, zeros=True)
    t1, t2 = gin(d1, 1), gin(d2, 1)
    loss, fac1, fac2 = ops.chamfer_loss(t1, t2, l1)
    grads = {}
    for dt in (F32, F64):
        x1, x2 = t1.detach().clone().to(dt).requires_grad_(True), t2.detach().clone().to(dt).requires_grad_(True)
        out = (torch.mean(torch.sqrt(x1)) + torch.mean(torch.sqrt(x2))) / 2 if l1 else torch.mean(x1) + torch.mean(x2)
        out.backward()
        grads[dt] = dict(loss=out.detach(), fac1=x1.grad, fac2=x2.grad)
    for k, f in (("fac1", fac1), ("fac2", fac2)):
        assert torch.equal(torch.isfinite(f), torch.isfinite(grads[F64][k])) and not bool(torch.isnan(f).any())
        assert bool((~torch.isfinite(f)).any()) == l1
    _judge("chamfer_loss", "zeros %s" % ("L1" if l1 else "L2"), dict(loss=loss.view(()), fac1=fac1, fac2=fac2), grads[F32], grads[F64], ("loss", "fac1", "fac2"))
    hand = R.chamfer_loss(t1, t2, l1, F64)
    assert torch.equal(torch.isinf(hand["fac1"]), torch.isinf(fac1)) and torch.equal(torch.isinf(hand["fac2"]), torch.isinf(fac2))


def test_chamfer_loss_c_entry_point_with_guarded_outputs_and_limits():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    B, n, m = 3, 40, 4001
    d1, d2 = G.loss_dists(B, n, m, 9)
    t1, t2 = gin(d1, 1), gin(d2, 1)
    nw = int(lib.upp_chamfer_loss_work_floats())
    outs = [guarded(1, F32, 1), guarded(B * n, F32, 1), guarded(B * m, F32, 1), guarded(nw, F32, 1)]
    loss, fac1, fac2, work = (o[0] for o in outs)
    assert lib.upp_chamfer_loss(p(t1), p(t2), B, n, m, 1, p(loss), p(fac1), p(fac2), p(work), st) == 0
    torch.cuda.synchronize()
    for _, check in outs:
        check()
    w = ops.chamfer_loss(t1, t2, True)
    assert _bits(loss, w[0]) and _bits(fac1.view(B, n), w[1]) and _bits(fac2.view(B, m), w[2])
    s = torch.full((8,), float("nan"), device="cuda")
    assert lib.upp_chamfer_loss(p(t1), p(t2), 0, n, m, 1, p(s), p(s), p(s), p(s), st) == E_BADARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(s).all())


# ============================================================================================== 4. NaN coordinates
def test_chamfer_nan_coordinate_is_never_lost():
    """`d < best` is false for NaN: a NaN query point gets dist = +inf, idx = 0 (the reference's `k == 0 ||` would give NaN: a stated
    deviation, include/upp_hip.h), and every query of the other cloud skips a NaN point.  What must hold: the NaN point's own distance
    is non-finite in its own direction, both modules return a non-finite loss, the other samples keep their bits."""
    from extensions.chamfer_dist import ChamferDistanceL1, ChamferDistanceL2
    B, n, m = 3, 70, 130
    a, b = G.clouds(B, n, "ball", 1), G.clouds(B, m, "ball", 2)
    clean = ops.chamfer_fwd(a.cuda(), b.cuda())
    clean_loss = {l1: mod()(a.cuda(), b.cuda()) for l1, mod in ((True, ChamferDistanceL1), (False, ChamferDistanceL2))}
    for which, j in ((0, 0), (0, 69), (1, 5), (1, 129)):
        a2, b2 = a.clone(), b.clone()
        (a2 if which == 0 else b2)[1, j, 1] = float("nan")
        d1, d2, i1, i2 = ops.chamfer_fwd(a2.cuda(), b2.cuda())
        own = (d1 if which == 0 else d2)[1, j]
        assert not bool(torch.isfinite(own)), (which, j, float(own))
        for s in (0, 2):
            for got, want in zip((d1, d2, i1, i2), clean):
                assert _bits(got[s], want[s]), (which, j, s)
        other_i = (i2 if which == 0 else i1)[1]
        assert not bool((other_i == j).any()), "the other cloud's queries skip the NaN point"
        for l1, mod in ((True, ChamferDistanceL1), (False, ChamferDistanceL2)):
            loss = mod()(a2.cuda(), b2.cuda())
            assert not bool(torch.isfinite(loss)), (which, j, l1, float(loss))
            keep = [0, 2]
            assert _bits(mod()(a2[keep].cuda(), b2[keep].cuda()), mod()(a[keep].cuda(), b[keep].cuda()))
        assert all(bool(torch.isfinite(v)) for v in clean_loss.values())


@pytest.mark.parametrize("B,n,m", [(3, 100, 40), (3, 63, 65)])
def test_emd_nan_coordinate_is_never_lost(B, n, m):
    """The cost of the poisoned sample is NaN and the other samples keep their bits (fmaxf(0, NaN) = 0 in the remain updates, as in the
    reference: the NaN reaches the match through the exponentials of the poisoned point's column or row)."""
    a, b = G.emd_pair(B, n, m, "ball")
    clean_m = ops.emd_approxmatch(a.cuda(), b.cuda())
    clean_c = ops.emd_matchcost(a.cuda(), b.cuda(), clean_m, deterministic=True)
    for which, j in ((0, 0), (0, n - 1), (1, 7), (1, m - 1)):
        a2, b2 = a.clone(), b.clone()
        (a2 if which == 0 else b2)[1, j, 2] = float("nan")
        mt = ops.emd_approxmatch(a2.cuda(), b2.cuda())
        for det in (True, False):
            cost = ops.emd_matchcost(a2.cuda(), b2.cuda(), mt, deterministic=det)
            assert bool(torch.isnan(cost[1])), (which, j, det, float(cost[1]))
            if det:
                assert _bits(cost[0], clean_c[0]) and _bits(cost[2], clean_c[2])
        assert _bits(mt[0], clean_m[0]) and _bits(mt[2], clean_m[2])


# ============================================================================================== 5. the wrappers
def _wrapper_calls():
    B, n, m = 2, 5, 7
    a, b = G.clouds(B, n, "ball", 1).cuda(), G.clouds(B, m, "ball", 2).cuda()
    d1, d2, i1, i2 = ops.chamfer_fwd(a, b)
    gd1, gd2 = G.mixed_grads((B, n), 1).cuda(), G.mixed_grads((B, m), 2).cuda()
    match, gc = G.given_match(B, n, m, 1).cuda(), G.grad_cost(B).cuda()
    return {
        "chamfer_bwd": (lambda t: ops.chamfer_bwd(t["xyz1"], t["xyz2"], t["idx1"], t["idx2"], t["gd1"], t["gd2"]),
                        dict(xyz1=a, xyz2=b, idx1=i1, idx2=i2, gd1=gd1, gd2=gd2)),
        "chamfer_bwd_det": (lambda t: ops.chamfer_bwd(t["xyz1"], t["xyz2"], t["idx1"], t["idx2"], t["gd1"], t["gd2"], deterministic=True),
                            dict(xyz1=a, xyz2=b, idx1=i1, idx2=i2, gd1=gd1, gd2=gd2)),
        "chamfer_loss": (lambda t: ops.chamfer_loss(t["dist1"], t["dist2"], True), dict(dist1=d1, dist2=d2)),
        "emd_matchcost": (lambda t: ops.emd_matchcost(t["xyz1"], t["xyz2"], t["match"]), dict(xyz1=a, xyz2=b, match=match)),
        "emd_matchcost_det": (lambda t: ops.emd_matchcost(t["xyz1"], t["xyz2"], t["match"], deterministic=True), dict(xyz1=a, xyz2=b, match=match)),
        "emd_matchcost_bwd": (lambda t: ops.emd_matchcost_bwd(t["gc"], t["xyz1"], t["xyz2"], t["match"]), dict(gc=gc, xyz1=a, xyz2=b, match=match)),
    }


WRAPPERS = ("chamfer_bwd", "chamfer_bwd_det", "chamfer_loss", "emd_matchcost", "emd_matchcost_det", "emd_matchcost_bwd")


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrappers_refuse_wrong_tensors(name):
    """Device, dtype, contiguity and the exact shape of every tensor a wrapper passes on, from metadata alone, before any launch: a match
    of another shape, a grad_cost of another length, indices or upstream gradients that are not (B, n) / (B, m), a second cloud or a
    dist2 of another batch used to be read as raw memory of the expected shape.  (Index VALUES outside the other cloud cannot be refused
    from metadata: include/upp_hip.h.)"""
    fn, tensors = _wrapper_calls()[name]
    refuse_wrong_tensors(name, fn, tensors)
