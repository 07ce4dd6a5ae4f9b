"""The kernels of csrc/head.hip -- cls_pool_fwd / bwd, ce_acc, logsoftmax_rows_fwd / bwd, nll_mean_fwd / bwd (+ nll_final_kernel),
noise_loss_fwd / bwd, bn_relu_drop_fwd / bwd -- against the float64 reference of tests/_head_reference.py, at the edges of their
parameter space: column widths around the 64-lane slots, every residue of the 8-wave / 16-row stride of the pooling kernel and of the
16 waves of the loss kernel, the 32-row workgroups of the row kernels, more than 1,024 partials for the final sum, ties, NaN rows,
logits with a common offset, underflowing exponentials, and the limits that return a status.

The bound, for every output and every case (tests/test_gpu_prop.py, tests/test_gpu_tail.py):
    err(x) = max|x - f64| / max|f64|,      err(kernel) <= max(2 * err(f32), 2e-6)
where f32 is the SAME formulation run by torch in float32 on the GPU with the selections (arg-max rows, ReLU gates, dropout keeps) of the
float64 run.  Exact checks -- arg-max rows, the first-maximum class and the accuracy, zeros in pad columns, the [row 0] half of cls_pool
against the max half when every row is a copy of row 0, the score against float32 sqrt of the same sum, NaN propagation, determinism of
a second call, guards -- are bit equalities.  Inputs live in NaN-guarded buffers 0 and 1 float off the 16-byte alignment (every kernel
of this file loads single floats); the partial-tile cases also run the C entry points with guarded outputs.  The generators
(tests/test_head_host.py) make every selection agree between the precisions by construction, and assert so on the CPU.

Measured on MI355X: (kernel, f32) of the case nearest its bound, per family and output (number of judged outputs).  281 tests; with
tests/test_gpu_rows.py's 129 in one run, 7.9 s for the 410 (tests/test_gpu_tail.py: 5 s for 209, tests/test_gpu_prop.py: 6 s for 180); the slowest
case is the first one (1.0 s, most of it loading the library), then test_ce_labels_outside_the_classes_are_pinned (0.18 s) and the two deliberately
large ones, R = 262,145 for nll_final_kernel and B P = 262,152 for the noise loss (0.1 s each).  The nearest any output comes to its bound is 0.82 of it.
    cls_pool (72)       feat 1.7e-3, 1.7e-3    mean 1.3e-7, 1.1e-7    rstd 5.1e-6, 5.1e-6    g_x 4.5e-4, 4.5e-4
    ce_acc (78)         loss 2.0e-7, 9.5e-8    dlogits 4.3e-7, 1.3e-7
    logsoftmax (120)    logp 1.1e-7, 1.1e-7    g_y 9.8e-7, 9.1e-7
    nll_mean (10)       loss 8.4e-8, 8.4e-8    g_logp 2.8e-8, 2.8e-8
    noise_loss (8)      loss 1.6e-7, 6.1e-8    score 6.5e-8, 7.5e-8   g_pred 9.1e-8, 9.1e-8
    bn_relu_drop (255)  a 1.0e-6, 9.7e-7       mean 7.2e-7, 8.2e-7    rstd 1.4e-7, 1.1e-7    running_mean 2.2e-7, 2.2e-7    running_var 2.3e-7, 1.4e-7
                        g_z 1.6e-6, 8.9e-7     g_gamma 2.0e-6, 1.9e-6 g_beta 7.7e-7, 2.6e-7
The large figures of cls_pool are the rows of 1e3 +- 1e-2 (`offset`, L = 2, D = 65): the row, rounded to f32, keeps three digits of its
deviation from the mean, in the kernel and in torch alike.  ce_acc's f32 column is at 1e-7 because the worst RATIO is a tie case; on the
`confident` cases torch's float32 formulation itself is off by 1e-5 ... 9e-4 (its 1 + sum rounds the loss) where the kernel stays at 1e-7.
g_z of bn_relu_drop at 0.82 of the bound is R = 3, C = 64 without running statistics: three rows, 1.6e-6 against the 2e-6 floor.

Hypotheses of the issue, decided by a run of the kernels as they were (the parent's csrc/head.hip and csrc/pointwise.hip built into a scratch
library) against these two files -- 47 cases failed, no other:
  1. cls_pool_fwd_kernel hid NaN: FAILED (test_cls_pool_nan_rows_reach_the_feature: the max half stayed finite for a NaN row t >= 1).  Fixed:
     the running maximum and the cross-wave merge take the first NaN, as group_max_fwd_kernel does.
  2. ce_acc_kernel lost the loss's precision under a common offset: FAILED, 41 cases of test_ce_acc_samples_and_classes and
     test_ce_acc_every_kind_at_every_offset -- loss 6.2e-3 against 1.0e-5 of float32 torch at B = 32, C = 40, confident, offset +-1e3; 0.15
     against 2.4e-4 at B = 15, C = 2; dlogits 2e-5 against 1e-7 in EVERY kind at +-1e3 (expf(v - lse) with lse rounded to ulp(1e3)).  Fixed
     in two steps.  (max - v_y) + log(sum) and expf((v - max) - log(sum)) brought every case but one to torch's own error; B = 1, C = 63,
     confident, +30 still missed (loss 2.2e-4 against 5.0e-5: one sample, 1 + 4e-4 rounded to ulp(1) either way, torch the luckier).  So
     the accurate form leaves the first maximum's exact 1 out of the sum and takes log1p of the rest, and writes softmax - 1 at the label
     as expm1(log p): no cancellation at p -> 1.  It serves the samples where the plain form loses digits: |max logit| >= 16, or the other
     classes holding less than 1/16 of the first maximum's weight.  Everywhere else the kernel keeps the plain form -- lse = max +
     log(sum), exp(v - lse), lse - v_y -- bit for bit: there its error is below the 2e-6 floor (worst here: dlogits 4.3e-7), and last bits of
     dlogits are not free: AdamW carries them forward, and recipes that sum with atomic adds amplify them
     (tests/test_gpu_graph_safety.py::test_replays_equal_the_eager_steps compares two such trajectories).
     test_ce_acc_on_both_sides_of_the_guards_of_the_plain_form holds one batch with samples on either side of both guards to the bound.
     Three of the failing cases also missed the accuracy: a / B * 100 rounds twice (6.666667 for 1 of 15, correctly rounded 6.6666665);
     a * 100 / B rounds once.  tests/test_gpu_block.py::test_cross_entropy_acc_matches_torch now takes its reference in float64: at B = 1
     float32 torch rounds a loss of 8.7e-9 to an exact 0 and the test asked for that 0.
  3. sqdist_topk_kernel ranked a NaN point first: FAILED (tests/test_gpu_rows.py::test_sqdist_topk_ranks_a_nan_point_last, all 5 cases, for
     the NaN with the sign bit set).  Fixed: one image for NaN, above +inf and below the padding.  (torch.sort on the device ranks by the
     same sign bit: the reference ranks NaN last explicitly.)
  4. the wrappers: ops.cls_pool_fwd / cls_pool_bwd / ce_acc / nll_mean_bwd / noise_loss_bwd / bn_relu_drop_fwd / bn_relu_drop_bwd here,
     ops.bn_rows_fwd / interp_fwd (out) / group_max_bwd (amax) in tests/test_gpu_rows.py now check device, dtype, contiguity and the exact shape
     of every tensor they pass on, from metadata alone (test_wrappers_refuse_wrong_tensors).  Not run against the old wrappers: an unchecked
     float64 operand is a read of raw memory, not a case to provoke.

Mutants (each built from a scratch copy, run once against the two new files and once against the old tests of the same kernels --
tests/test_gpu_block.py -k "cls_pool or cross_entropy or bn_relu_drop" and tests/test_gpu_pointwise.py: 200 cases).  Value changes only:
  1. cls_pool's cross-wave merge without the tie rule (`v > best` alone: the first WAVE holding the maximum wins): fails 10 cases here --
     columns_and_rows[L >= 9, D = 1] (every row ties; row 8 sits in wave 0, row 1 in wave 1), edges[dup2] x 2, edges[offset, L = 9] and the
     NaN rows -- but NOT edges[dup]: rows 3, 12 and 21 sit in waves 3, 4 and 5, in the rows' own order, which is why dup2 (rows 5 and 10 in
     waves 5 and 2) exists.  Old tests: 200 pass.
  2. ce_acc's `first` with max instead of min: fails 24 cases here (every tie_first / tie_second case with C >= 2, through the accuracy);
     old tests: 200 pass.
  3. logsoftmax_rows_bwd writes gv to the pad columns: passes, here and in the old tests, and has to: EQUIVALENT -- gv is loaded under
     `lane < C` and is an exact 0 in every pad lane.  The neighbour that writes the row sum sg there (3b) fails all 40 cases of
     test_logsoftmax_rows with a pad column here and 2 of the old tests.
  4. bn_finalize_rows_kernel takes `per` for the last slab's row count: fails 14 cases of tests/test_gpu_rows.py (every training shape whose
     last slab is short, the flat non-temporal case, two option cases); old tests: 22 of 200 fail.
  5. bn_rows_bwd_apply_tall_kernel's gate with >=: fails test_bn_rows_gate_is_the_same_forward_and_backward[4096-64 | 4099-256] (the two
     tall cases) and nothing else here; old tests: 2 of 200 fail (the two largest backward cases, where a pre-activation is an exact 0 by chance).
  6. interp_bwd_kernel sums the wave segments in the order 1, 0, 2, 3: passes, here and in the old tests.  EQUIVALENT under the bound: any
     order of the same terms is a float32 sum within it; what the kernel promises beyond that is one order on every call (the second-call
     bit equality), which a permuted but fixed order keeps.
  7. sqdist_topk's selection takes the highest lane of a tie: fails 10 cases of tests/test_gpu_rows.py (lattice clouds with S >= 63, the NaN
     cases with S >= 64); old tests: 4 of 200 fail.
  8. interp_wide_kernel gathers the first source's second 256-column piece at the first piece's columns (the suggested mutant, without the
     `cb < C` store guard, would write past the row: replaced by this value-only neighbour): fails 5 cases of tests/test_gpu_rows.py
     (forward_wide[260 | 512 | 516 | 1028], the window case); old tests: 3 of 200 fail.

Behaviours torch answers with an exception and these kernels do not ("Limits of the head and per-point row kernels"; each
pinned below): a label outside [0, C) counts as a wrong prediction whose loss term is the log-sum-exp alone and whose gradient row is
softmax / B (test_ce_labels_outside_the_classes_are_pinned); an NLL target outside [0, C) adds nothing to the sum -- R still divides --
and gets a zero gradient row (test_nll_targets_outside_the_classes_are_pinned); one row of training-mode BatchNorm raises ValueError from
metadata, as torch does, and a BatchNorm with momentum=None raises ValueError where its running statistics would be updated
(test_one_row_and_cumulative_momentum_are_refused).
"""
import numpy as np
import pytest
import torch

import _head_reference as R
import test_head_host as G
from test_gpu_step_tail import guarded
from test_gpu_tail import _bits, gin
from upp_hip import _abi, ops
from upp_hip import functional as HF

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
E_BADARG, E_RANGE = -1, -2


# ---------------------------------------------------------------------------------------------- the bound
def _err(x, e):
    """max|x - e| / max|e| over the elements where e is finite (absolute where e is all zero)."""
    m = torch.isfinite(e)
    if not bool(m.any()):
        return 0.0
    scale = float(e[m].abs().max())
    d = (x.double()[m] - e[m]).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return float(d.max()) / (scale if scale > 0 else 1.0)


def judge(family, label, got, f32, f64, keys, tag="HEADERR"):
    """The bound for every key; every figure is printed before anything is asserted."""
    bad = []
    for k in keys:
        if f64[k] is None:
            assert got[k] is None, (family, label, k, "is not asked for and must be None")
            continue
        assert got[k] is not None, (family, label, k)
        e = torch.as_tensor(f64[k]).reshape(got[k].shape)
        f = torch.as_tensor(f32[k]).reshape(e.shape)
        inf_ok = torch.isinf(e)                                 # (-inf log-probabilities of -inf logits: equal on both sides, bit for bit)
        assert torch.equal(torch.isinf(got[k]) & (got[k] == e), inf_ok), (family, label, k, "infinities differ")
        if not bool(torch.isfinite(got[k])[~inf_ok].all()):
            bad.append((k, "non-finite"))
            continue
        ek, ef = _err(got[k], e), _err(f, e)
        print("%s | %s | %s | %s | %.2e | %.2e" % (tag, family, label, k, ek, ef))
        if not ek <= max(2.0 * ef, 2e-6):
            bad.append((k, ek, ef))
    assert not bad, (family, label, bad)


def _same(a, b, what):
    for k in a:
        assert _bits(a[k], b[k]), what + ": " + k


def _cuda(d, keys):
    return {k: (None if d[k] is None else d[k].cuda()) for k in keys}


def _sentinel(shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda") if dtype.is_floating_point else torch.full(shape, -77, dtype=dtype, device="cuda")


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == -77).all()) for t in ts)


# ============================================================================================== 1. cls_pool
CLS_KEYS = ("feat", "mean", "rstd", "g_x")
CLS_D = (1, 63, 64, 65, 384, 500, 512)
CLS_L = (2, 3, 8, 9, 16, 17, 25, 65, 130)        # a wave takes rows t and t + 8 and strides by 16


def run_cls(c, off):
    t = {k: gin(c[k], off) for k in ("x", "gamma", "beta", "g_feat")}
    feat, amax, mean, rstd = ops.cls_pool_fwd(t["x"], t["gamma"], t["beta"], c["eps"])
    g_x = ops.cls_pool_bwd(t["g_feat"], t["x"], mean, rstd, t["gamma"], amax)
    return dict(feat=feat, amax=amax, mean=mean, rstd=rstd, g_x=g_x)


def check_cls(c, label, off=1):
    a, b = run_cls(c, off), run_cls(c, 1 - off)
    _same(a, b, "second run (other alignment) differs")
    d = _cuda(c, ("x", "gamma", "beta", "g_feat", "amax"))
    ref = {dt: R.cls_pool(d["x"], d["gamma"], d["beta"], c["eps"], d["amax"], dt, d["g_feat"]) for dt in (F32, F64)}
    assert torch.equal(a["amax"].long(), d["amax"]), "arg-max rows"
    judge("cls_pool", label, a, ref[F32], ref[F64], CLS_KEYS)
    return a


@pytest.mark.parametrize("D", CLS_D)
@pytest.mark.parametrize("L", CLS_L)
def test_cls_pool_columns_and_rows(L, D):
    B = 1 if (CLS_D.index(D) + CLS_L.index(L)) % 2 == 0 else 3
    check_cls(G.cls_inputs(B, L, D, 100 * L + D), "B=%d L=%d D=%d" % (B, L, D), off=(L + D) % 2)


@pytest.mark.parametrize("kind,B,L,D", [("dup", 3, 25, 65), ("dup", 1, 130, 384), ("dup2", 3, 11, 65), ("dup2", 1, 25, 512), ("const", 3, 9, 64), ("const", 1, 3, 500),
                                        ("offset", 3, 2, 65), ("offset", 1, 9, 384), ("gzero", 3, 17, 63)])
def test_cls_pool_edges(kind, B, L, D):
    """Bit-identical maximal rows in three different waves, and in two waves whose order is not the rows' (the lowest row wins in feat,
    amax and the gradient), a constant row
    (rstd = eps^-1/2), rows of 1e3 +- 1e-2, a gradient that is zero in one half."""
    c = G.cls_inputs(B, L, D, L + D, kind)
    a = check_cls(c, "%s L=%d D=%d" % (kind, L, D))
    if kind == "dup":
        tied = (c["amax"] == 3).cuda()
        assert bool(tied.any()) and _bits(a["g_x"][:, 12], a["g_x"][:, 21])
        gx12 = a["g_x"][:, 12].clone()                       # rows 12 and 21 get no max gradient: LayerNorm backward of a zero row is an exact 0
        assert float(gx12.abs().max()) == 0.0 and float(a["g_x"][:, 3].abs().max()) > 0.0
    if kind == "offset":                                     # every row a copy of ... row 1; make row 0 one too: both halves, one arithmetic
        c2 = dict(c)
        c2["x"] = c["x"].clone()
        c2["x"][:, 0] = c2["x"][:, 1]
        r = run_cls(c2, 0)
        assert _bits(r["feat"][:, :D], r["feat"][:, D:]) and bool((r["amax"] == 1).all())


def test_cls_pool_nan_rows_reach_the_feature():
    """A NaN in row 0 makes the [row 0] half NaN, a NaN in a row t >= 1 the max half -- as norm(x)[:, 1:].max(1) and this library's
    group_max do (the kernel used to skip NaN rows: `h > mx` and `v > best` are false for them) -- with amax on the FIRST NaN row;
    the sample's other half and every other sample keep their bits."""
    B, L, D = 3, 25, 65
    c = G.cls_inputs(B, L, D, 7)
    clean = run_cls(c, 1)
    for rows in ((0,), (1,), (9,), (16,), (24,), (12, 5), (21, 13)):
        c2 = dict(c)
        c2["x"] = c["x"].clone()
        for t in rows:
            c2["x"][1, t, 5] = float("nan")
        r = run_cls(c2, 1)
        for s in (0, 2):
            assert _bits(r["feat"][s], clean["feat"][s]) and torch.equal(r["amax"][s], clean["amax"][s]) and _bits(r["g_x"][s], clean["g_x"][s]), rows
        if rows == (0,):
            assert bool(torch.isnan(r["feat"][1, :D]).all()) and _bits(r["feat"][1, D:], clean["feat"][1, D:]), rows
            assert torch.equal(r["amax"][1], clean["amax"][1])
        else:
            assert bool(torch.isnan(r["feat"][1, D:]).all()) and _bits(r["feat"][1, :D], clean["feat"][1, :D]), rows
            assert bool((r["amax"][1] == min(rows)).all()), (rows, r["amax"][1])
            want = R.first_max(R.layer_norm(c2["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), c["eps"], F64)[0][:, 1:], 1) + 1
            assert torch.equal(r["amax"].long(), want)


def test_cls_pool_c_entry_points_with_guarded_outputs_and_limits():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    for B, L, D in ((3, 17, 65), (1, 9, 500)):
        c = G.cls_inputs(B, L, D, 31)
        t = {k: gin(c[k], 1) for k in ("x", "gamma", "beta", "g_feat")}
        outs = {k: guarded(n, dt, 1) for k, n, dt in (("feat", B * 2 * D, F32), ("amax", B * D, torch.int32), ("mean", B * L, F32),
                                                      ("rstd", B * L, F32), ("g_x", B * L * D, F32))}
        o = {k: v[0] for k, v in outs.items()}
        assert lib.upp_cls_pool_fwd(p(t["x"]), p(t["gamma"]), p(t["beta"]), c["eps"], p(o["feat"]), p(o["amax"]), p(o["mean"]), p(o["rstd"]),
                                    B, L, D, st) == 0
        assert lib.upp_cls_pool_bwd(p(t["g_feat"]), p(t["x"]), p(o["mean"]), p(o["rstd"]), p(t["gamma"]), p(o["amax"]), p(o["g_x"]), B, L, D, st) == 0
        torch.cuda.synchronize()
        for k, (_, check) in outs.items():
            check()
        w = run_cls(c, 0)
        for k in ("feat", "amax", "mean", "rstd", "g_x"):
            assert _bits(o[k].view(w[k].shape), w[k]), k
    # D = 513: the range status; L = 1 (no row to take a maximum over): the argument status -- nothing launched, nothing written
    x, ga = torch.zeros(2, 3, 513, device="cuda"), torch.ones(513, device="cuda")
    feat, amax, stat, g_x = _sentinel((2, 1026)), _sentinel((2, 513), torch.int32), _sentinel((6,)), _sentinel((2, 3, 513))
    assert lib.upp_cls_pool_fwd(p(x), p(ga), p(ga), 1e-5, p(feat), p(amax), p(stat), p(stat), 2, 3, 513, st) == E_RANGE
    assert lib.upp_cls_pool_bwd(p(feat), p(x), p(stat), p(stat), p(ga), p(amax), p(g_x), 2, 3, 513, st) == E_RANGE
    assert lib.upp_cls_pool_fwd(p(x), p(ga), p(ga), 1e-5, p(feat), p(amax), p(stat), p(stat), 2, 1, 512, st) == E_BADARG
    assert lib.upp_cls_pool_bwd(p(feat), p(x), p(stat), p(stat), p(ga), p(amax), p(g_x), 2, 1, 512, st) == E_BADARG
    assert _untouched(feat, amax, stat, g_x)
    with pytest.raises(RuntimeError):
        ops.cls_pool_fwd(x, ga, ga, 1e-5)
    with pytest.raises(RuntimeError):
        ops.cls_pool_fwd(torch.zeros(2, 1, 64, device="cuda"), ga[:64].contiguous(), ga[:64].contiguous(), 1e-5)


# ============================================================================================== 2. ce_acc
CE_KEYS = ("loss", "dlogits")
CE_B = (1, 15, 16, 17, 33, 64)                    # 16 waves, samples strided over them
CE_C = (1, 2, 40, 63, 64, 65, 500, 512)
OFFSETS = (0.0, 30.0, -30.0, 1e3, -1e3)


def run_ce(c, off):
    out2, dlogits = ops.ce_acc(gin(c["logits"], off), gin(c["labels"], off))
    return dict(loss=out2[0], acc=out2[1], dlogits=dlogits)


def check_ce(c, label, off=1):
    a, b = run_ce(c, off), run_ce(c, 1 - off)
    _same(a, b, "second run (other alignment) differs")
    d = _cuda(c, ("logits", "labels", "first"))
    ref = {dt: R.ce_acc(d["logits"], d["labels"], d["first"], dt) for dt in (F32, F64)}
    got_acc = a["acc"].cpu().numpy()
    print("HEADERR | ce_acc | %s | acc | %r | %r" % (label, float(got_acc), float(ref[F64]["acc"])))
    assert got_acc.dtype == np.float32 and got_acc == ref[F64]["acc"], ("accuracy", float(got_acc), float(ref[F64]["acc"]))
    judge("ce_acc", label, a, ref[F32], ref[F64], CE_KEYS)


@pytest.mark.parametrize("C", CE_C)
@pytest.mark.parametrize("B", CE_B)
def test_ce_acc_samples_and_classes(B, C):
    i = CE_B.index(B) * len(CE_C) + CE_C.index(C)
    kind, offset = G.CE_KINDS[i % len(G.CE_KINDS)], OFFSETS[(i // 2) % len(OFFSETS)]
    check_ce(G.ce_inputs(B, C, 7 * B + C, kind, offset), "B=%d C=%d %s %+g" % (B, C, kind, offset), off=i % 2)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("kind", G.CE_KINDS)
def test_ce_acc_every_kind_at_every_offset(kind, offset):
    """B = 32, C = 40 -- the classification head.  `confident` is the regression case of the loss term: lse - v_y rounds every sample's
    term to ulp(max logit), (max - v_y) + log(sum exp) does not."""
    check_ce(G.ce_inputs(32, 40, 3, kind, offset), "B=32 C=40 %s %+g" % (kind, offset))


@pytest.mark.parametrize("B,C", [(32, 40), (17, 65)])
def test_ce_acc_on_both_sides_of_the_guards_of_the_plain_form(B, C):
    """The kernel keeps lse = max + log(sum) per SAMPLE while |max| < 16 and the other classes hold >= 1/16 of the first maximum's weight,
    and takes the log1p / expm1 form beyond: one batch with samples on either side of each guard, and one tie of the maximum."""
    g = torch.Generator().manual_seed(B + C)
    v = torch.randn(B, C, generator=g) * 0.3
    labels = torch.randint(0, C, (B,), generator=g)
    boost = torch.log(torch.tensor(16.0 * (C - 1)))                       # sum over the others = 1/16 at this lead of the label's logit
    lead = torch.tensor([0.0, float(boost) - 0.4, float(boost) + 0.4, 12.0])[torch.arange(B) % 4]
    v[torch.arange(B), labels] += lead
    v += torch.tensor([0.0, 15.0, 17.0, -15.0, -17.0])[torch.arange(B) % 5].view(B, 1)
    v[0, (labels[0] + 1) % C] = v[0, labels[0]] = v[0].max() + 1.0
    mx = v.max(1).values
    others = (torch.exp(v.double() - mx.double().view(B, 1)).sum(1) - 1.0)
    plain = (mx.abs() < 16) & (others >= 0.0625)
    assert 3 <= int(plain.sum()) <= B - 3 and int((mx.abs() >= 16).sum()) >= 3 and int((others < 0.0625).sum()) >= 3
    check_ce(dict(logits=v, labels=labels, first=R.ce_select(v)), "guards B=%d C=%d" % (B, C))


def test_ce_labels_outside_the_classes_are_pinned():
    """torch raises; the kernel cannot know without a synchronisation.  Such a sample is a wrong prediction, its loss term is the
    log-sum-exp alone and its gradient row softmax / B."""
    B, C = 17, 40
    c = G.ce_inputs(B, C, 5)
    labels = c["labels"].clone()
    labels[2], labels[9], labels[11] = -1, C, (1 << 32) + int(c["first"][11])      # (the last one: compared in 64 bits, no class `first`)
    a = run_ce(dict(logits=c["logits"], labels=labels), 1)
    v = c["logits"].cuda().double()
    lse = torch.logsumexp(v, 1)
    ok = torch.ones(B, dtype=torch.bool, device="cuda")
    ok[2] = ok[9] = ok[11] = False
    safe = torch.where(ok, labels.cuda(), torch.zeros_like(labels.cuda()))
    want = (lse - torch.where(ok, v.gather(1, safe.view(B, 1)).view(B), torch.zeros_like(lse))).sum() / B
    onehot = torch.zeros_like(v).scatter_(1, safe.view(B, 1), 1.0) * ok.view(B, 1)
    assert abs(float(a["loss"]) - float(want)) <= 2e-6 * float(want)
    assert float((a["dlogits"].double() - (torch.softmax(v, 1) - onehot) / B).abs().max()) <= 2e-6 / B
    count = int(((c["first"] == labels) & ok.cpu()).sum())
    assert a["acc"].cpu().numpy() == np.float32(count / B * 100)


def test_ce_acc_c_entry_point_with_guarded_outputs_and_limits():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    B, C = 17, 65
    c = G.ce_inputs(B, C, 9)
    lg, lb = gin(c["logits"], 1), gin(c["labels"], 1)
    (o2, ck2), (dl, ckd) = guarded(2, F32, 1), guarded(B * C, F32, 1)
    assert lib.upp_ce_acc(p(lg), p(lb), p(o2), p(dl), B, C, st) == 0
    torch.cuda.synchronize()
    ck2(); ckd()
    w = run_ce(c, 0)
    assert _bits(o2[0], w["loss"]) and _bits(o2[1], w["acc"]) and _bits(dl.view(B, C), w["dlogits"])
    out2, dl = _sentinel((2,)), _sentinel((2, 513))
    assert lib.upp_ce_acc(p(torch.zeros(2, 513, device="cuda")), p(torch.zeros(2, dtype=torch.int64, device="cuda")), p(out2), p(dl), 2, 513, st) == E_RANGE
    assert _untouched(out2, dl)


# ============================================================================================== 3. log-softmax rows, NLL
LS_C = (1, 2, 13, 50, 63, 64)
LS_R = (1, 7, 8, 9, 31, 32, 33, 257)             # a workgroup holds 4 waves x 8 rows


def ls_case(Rr, C, ld, bias, Cpad, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.full((Rr, ld), float("nan"))
    y[:, :C] = torch.randn(Rr, C, generator=g) * 3
    if Rr > 2:
        y[1, :C] += 40.0 * torch.arange(C) / max(C - 1, 1)         # a row whose exponentials underflow
        y[2, 0] = -float("inf") if C > 1 else y[2, 0]              # a class that cannot occur
    return dict(y=y, bias=0.5 * torch.randn(C, generator=g) if bias else None, g=torch.randn(Rr, C, generator=g), C=C, Cpad=Cpad)


def run_ls(c, off):
    y = gin(c["y"], off)
    logp = ops.logsoftmax_rows_fwd(y, gin(c["bias"], off), c["C"])
    g_y = ops.logsoftmax_rows_bwd(gin(c["g"], off), logp, c["Cpad"])
    return dict(logp=logp, g_y=g_y)


@pytest.mark.parametrize("C", LS_C)
@pytest.mark.parametrize("Rr", LS_R)
def test_logsoftmax_rows(Rr, C):
    """Row strides C, C + 2, 64 (52 for the 50 classes of the part-segmentation head), the pad columns of y NaN (never read); with and
    without bias; the backward into C and C + 2 columns, pad columns an exact 0."""
    lds = sorted({C, min(C + 2, 64), 64} | ({52} if C == 50 else set()))
    for i, ld in enumerate(lds):
        bias, Cpad = (i + Rr) % 2 == 0, (C if i % 2 == 0 else min(C + 2, 64))
        c = ls_case(Rr, C, ld, bias, Cpad, 10 * Rr + C + ld)
        a, b = run_ls(c, i % 2), run_ls(c, 1 - i % 2)
        _same(a, b, "second run (other alignment) differs")
        d = _cuda(c, ("y", "bias", "g"))
        ref = {dt: R.logsoftmax_rows(d["y"], d["bias"], C, dt, d["g"], Cpad) for dt in (F32, F64)}
        if Cpad > C:
            assert float(a["g_y"][:, C:].abs().max()) == 0.0, "pad columns"
        # the -inf class: logp = -inf on both sides, and its gradient is g itself (exp(-inf) = 0)
        judge("logsoftmax", "R=%d C=%d ld=%d bias=%d Cpad=%d" % (Rr, C, ld, bias, Cpad), a, ref[F32], ref[F64], ("logp", "g_y"))


def test_logsoftmax_c_entry_points_with_guarded_outputs_and_limits():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    for Rr, C, ld, Cpad, ldg in ((33, 50, 52, 52, 52), (9, 13, 15, 15, 20), (257, 63, 64, 64, 64)):
        c = ls_case(Rr, C, ld, True, Cpad, Rr)
        y, bias, g = gin(c["y"], 1), gin(c["bias"], 1), gin(c["g"], 1)
        (logp, ck1), (gy, ck2) = guarded(Rr * C, F32, 1), guarded(Rr * ldg, F32, 1)
        assert lib.upp_logsoftmax_rows_fwd(p(y), ld, p(bias), Rr, C, p(logp), st) == 0
        assert lib.upp_logsoftmax_rows_bwd(p(g), p(logp), Rr, C, p(gy), ldg, Cpad, st) == 0
        torch.cuda.synchronize()
        ck1(); ck2()
        w = run_ls(c, 0)
        gy = gy.view(Rr, ldg)
        assert _bits(logp.view(Rr, C), w["logp"]) and _bits(gy[:, :Cpad], w["g_y"])
        assert ldg == Cpad or bool(torch.isnan(gy[:, Cpad:]).all()), "columns beyond Cpad belong to the caller"
    y, o = torch.zeros(4, 65, device="cuda"), _sentinel((4, 65))
    assert lib.upp_logsoftmax_rows_fwd(p(y), 65, None, 4, 65, p(o), st) == E_RANGE
    assert lib.upp_logsoftmax_rows_bwd(p(y), p(y), 4, 64, p(o), 65, 65, st) == E_RANGE
    assert lib.upp_logsoftmax_rows_fwd(p(y), 63, None, 4, 64, p(o), st) == E_BADARG         # a row stride below C
    assert _untouched(o)
    with pytest.raises(RuntimeError):
        ops.logsoftmax_rows_fwd(y, None, 65)


def nll_case(Rr, C, seed):
    g = torch.Generator().manual_seed(seed)
    logp = torch.log_softmax(torch.randn(Rr, C, generator=g) * 2, -1)
    return dict(logp=logp, target=torch.randint(0, C, (Rr,), generator=g), g_loss=torch.tensor([1.7]))


def run_nll(c, off):
    target = gin(c["target"], off)
    loss = ops.nll_mean_fwd(gin(c["logp"], off), target)
    return dict(loss=loss, g_logp=ops.nll_mean_bwd(gin(c["g_loss"], off), target, *c["logp"].shape))


def check_nll(c, label, off=1):
    a, b = run_nll(c, off), run_nll(c, 1 - off)
    _same(a, b, "second run (other alignment) differs")
    d = _cuda(c, ("logp", "target", "g_loss"))
    ref = {dt: R.nll_mean(d["logp"], d["target"], dt, d["g_loss"]) for dt in (F32, F64)}
    assert torch.equal(a["g_logp"] != 0, ref[F64]["g_logp"] != 0), "one entry per row, exact zeros elsewhere"
    judge("nll_mean", label, a, ref[F32], ref[F64], ("loss", "g_logp"))


@pytest.mark.parametrize("Rr,C", [(1, 5), (63, 50), (64, 13), (65, 64), (255, 2), (256, 50), (257, 1), (1025, 50), (262145, 2)])
def test_nll_mean(Rr, C):
    """One wave per 64 rows, 256 rows per partial; R = 262,145 gives nll_final_kernel 1,025 partials (two per thread for the first 512)."""
    check_nll(nll_case(Rr, C, Rr + C), "R=%d C=%d" % (Rr, C), off=Rr % 2)


def test_nll_targets_outside_the_classes_are_pinned():
    """torch raises; here such a row adds nothing to the sum (R still divides) and gets a zero gradient row."""
    c = nll_case(257, 13, 4)
    c["target"][[0, 100, 256]] = torch.tensor([-1, 13, 1 << 40])
    check_nll(c, "targets outside")


def test_nll_backward_writes_every_element_and_the_guards_stay():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    for Rr, C in ((257, 13), (33, 50), (1, 1)):
        c = nll_case(Rr, C, 8)
        target, g_loss = gin(c["target"], 1), gin(c["g_loss"], 1)
        (g_logp, ck), (part, ckp), (out, cko) = guarded(Rr * C, F32, 1), guarded(int(lib.upp_nll_mean_part_floats(Rr)), F32, 1), guarded(1, F32, 1)
        assert lib.upp_nll_mean_bwd(p(g_loss), p(target), Rr, C, p(g_logp), st) == 0
        assert lib.upp_nll_mean_fwd(p(gin(c["logp"], 1)), p(target), Rr, C, p(part), p(out), st) == 0
        torch.cuda.synchronize()
        ck(); ckp(); cko()
        w = run_nll(c, 0)
        assert not bool(torch.isnan(g_logp).any()) and _bits(g_logp.view(Rr, C), w["g_logp"]) and _bits(out, w["loss"])


# ============================================================================================== 4. noise loss
def noise_case(B, P, pn, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(pred=torch.randn(B, P, 3, generator=g) * 0.3, nv=torch.randn(B, P - pn, 3, generator=g) * 0.3, pn=pn, g_loss=torch.tensor([0.7]))


def run_noise(c, off):
    pred, nv = gin(c["pred"], off), gin(c["nv"], off)
    loss, score = ops.noise_loss_fwd(pred, nv, c["pn"])
    return dict(loss=loss, score=score, g_pred=ops.noise_loss_bwd(gin(c["g_loss"], off), pred, nv, c["pn"]))


@pytest.mark.parametrize("B,P,pn", [(1, 2, 1), (5, 51, 1), (5, 51, 50), (4, 64, 1), (4, 64, 63), (1, 257, 1), (1, 257, 256), (8, 32769, 1000)])
def test_noise_loss(B, P, pn):
    """B P = 2, 255, 256, 257 around the 256-point partial, pn at both ends; B P = 262,152 gives the final sum 1,025 partials."""
    c = noise_case(B, P, pn, B * P + pn)
    a, b = run_noise(c, P % 2), run_noise(c, 1 - P % 2)
    _same(a, b, "second run (other alignment) differs")
    d = _cuda(c, ("pred", "nv", "g_loss"))
    ref = {dt: R.noise_loss(d["pred"], d["nv"], pn, dt, d["g_loss"]) for dt in (F32, F64)}
    assert _bits(a["score"].cpu(), R.score_f32(c["pred"])), "score = float32 sqrt of fma(z, z, fma(x, x, y y))"
    judge("noise_loss", "B=%d P=%d pn=%d" % (B, P, pn), a, ref[F32], ref[F64], ("loss", "score", "g_pred"))


def test_noise_loss_c_entry_points_with_guarded_outputs_and_limits():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    B, P, pn = 1, 257, 7
    c = noise_case(B, P, pn, 2)
    pred, nv, g_loss = gin(c["pred"], 1), gin(c["nv"], 1), gin(c["g_loss"], 1)
    outs = [guarded(n, F32, 1) for n in (int(lib.upp_noise_loss_part_floats(B, P)), 1, B * P, B * P * 3)]
    part, loss, score, g_pred = (o[0] for o in outs)
    assert lib.upp_noise_loss_fwd(p(pred), p(nv), B, P, pn, p(part), p(loss), p(score), st) == 0
    assert lib.upp_noise_loss_bwd(p(g_loss), p(pred), p(nv), B, P, pn, p(g_pred), st) == 0
    torch.cuda.synchronize()
    for _, check in outs:
        check()
    w = run_noise(c, 0)
    assert _bits(loss, w["loss"]) and _bits(score.view(B, P), w["score"]) and _bits(g_pred.view(B, P, 3), w["g_pred"])
    s = _sentinel((B * P * 3,))
    for bad_pn in (0, P):                                      # a cloud without shape points, or without noise points: a mean over nothing
        assert lib.upp_noise_loss_fwd(p(pred), p(nv), B, P, bad_pn, p(s), p(s), p(s), st) == E_BADARG
        assert lib.upp_noise_loss_bwd(p(g_loss), p(pred), p(nv), B, P, bad_pn, p(s), st) == E_BADARG
    assert _untouched(s)
    with pytest.raises(RuntimeError):
        ops.noise_loss_fwd(pred, nv[:, :0].contiguous(), P)


# ============================================================================================== 5. bn_relu_drop
BN_KEYS = ("a", "mean", "rstd", "running_mean", "running_var", "g_z", "g_gamma", "g_beta")
BRD_R = (2, 3, 4, 5, 7, 32, 130)                  # 4 waves stride the rows
BRD_C = (1, 63, 64, 65, 256, 300)
BRD_MODES = ("train", "train_u0", "train_u", "train_norun", "eval", "eval_u")


def run_brd(c, mode, u, p, off):
    training = not mode.startswith("eval")
    t = {k: gin(c[k], off) for k in ("z", "gamma", "beta", "rm", "rv", "g")}
    if mode == "train_norun":
        t["rm"] = t["rv"] = None
    ud = gin(u, off)
    a, mean, rstd = ops.bn_relu_drop_fwd(t["z"], t["gamma"], t["beta"], t["rm"], t["rv"], c["momentum"], c["eps"], training, ud, p)
    g_z, g_gamma, g_beta = ops.bn_relu_drop_bwd(t["g"], t["z"], t["gamma"], t["beta"], mean, rstd, training, ud, p)
    return dict(a=a, mean=mean, rstd=rstd, running_mean=t["rm"] if training else None, running_var=t["rv"] if training else None,
                g_z=g_z, g_gamma=g_gamma, g_beta=g_beta), t


def check_brd(Rr, C, mode, seed, kind="rand"):
    training = not mode.startswith("eval")
    c = G.bn_inputs(Rr, C, seed, training, kind)
    p = 0.5 if mode in ("train_u", "eval_u") else 0.0
    u = G.dropout_uniforms((Rr, C), p, seed + 1) if mode in ("train_u0", "train_u", "eval_u") else None
    (a, _), (b, t) = run_brd(c, mode, u, p, 1), run_brd(c, mode, u, p, 0)
    _same(a, b, "second run (other alignment) differs")
    if not training:
        assert _bits(t["rm"], c["rm"].cuda()) and _bits(t["rv"], c["rv"].cuda()), "eval leaves the running statistics alone"
    d = _cuda(c, ("z", "gamma", "beta", "rm", "rv", "g"))
    if mode == "train_norun":
        d["rm"] = d["rv"] = None
    gate = R.bn_select(d["z"], d["gamma"], d["beta"], d["rm"], d["rv"], c["eps"], training)
    keep = None if u is None else torch.from_numpy(R.dropout_select(u, p)).cuda()
    ref = {dt: R.batch_norm(d["z"], d["gamma"], d["beta"], d["rm"], d["rv"], c["momentum"], c["eps"], training, gate, keep, p, dt, d["g"])
           for dt in (F32, F64)}
    assert torch.equal(a["a"] != 0, ref[F64]["a"] != 0), "the ReLU gate and the dropout mask (the planted u == p is kept)"
    if u is not None and p > 0:
        assert float(u.view(-1)[0]) == float(np.float32(p))
    judge("bn_relu_drop", "R=%d C=%d %s %s" % (Rr, C, mode, kind), a, ref[F32], ref[F64], BN_KEYS)


@pytest.mark.parametrize("C", BRD_C)
@pytest.mark.parametrize("Rr", BRD_R)
def test_bn_relu_drop_rows_and_columns(Rr, C):
    """Every mode at every shape: training with and without uniforms (p = 0 with uniforms given, p = 0.5 with the planted u == p),
    training without running statistics, eval, eval with uniforms; forward, running update and all three gradients."""
    for i, mode in enumerate(BRD_MODES):
        check_brd(Rr, C, mode, 1000 * i + 10 * Rr + C)


@pytest.mark.parametrize("Rr,C,mode", [(130, 65, "train"), (32, 256, "train_u"), (7, 64, "eval")])
def test_bn_relu_drop_offset_columns(Rr, C, mode):
    """Columns 40 sigma off zero, a constant column, every 8th row a 30 sigma outlier: the two-pass statistics do not cancel."""
    check_brd(Rr, C, mode, 77, kind="offset")


@pytest.mark.parametrize("Rr,C", [(3, 65), (5, 300), (7, 65)])
def test_bn_relu_drop_c_entry_points_with_guarded_outputs(Rr, C):
    """Rows that do not fill the 4 waves, columns that do not fill the last 64-lane workgroup: every output between guards."""
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    c = G.bn_inputs(Rr, C, Rr + C)
    u = G.dropout_uniforms((Rr, C), 0.5, 3)
    t = {k: gin(c[k], 1) for k in ("z", "gamma", "beta", "rm", "rv", "g")}
    ud = gin(u, 1)
    outs = {k: guarded(n, F32, 1) for k, n in (("a", Rr * C), ("mean", C), ("rstd", C), ("g_z", Rr * C), ("g_gamma", C), ("g_beta", C))}
    o = {k: v[0] for k, v in outs.items()}
    assert lib.upp_bn_relu_drop_fwd(p(t["z"]), p(t["gamma"]), p(t["beta"]), p(t["rm"]), p(t["rv"]), 0.1, 1e-5, 1, p(ud), 0.5, p(o["a"]), p(o["mean"]),
                                    p(o["rstd"]), Rr, C, st) == 0
    assert lib.upp_bn_relu_drop_bwd(p(t["g"]), p(t["z"]), p(t["gamma"]), p(t["beta"]), p(o["mean"]), p(o["rstd"]), 1, p(ud), 0.5, p(o["g_z"]),
                                    p(o["g_gamma"]), p(o["g_beta"]), Rr, C, st) == 0
    torch.cuda.synchronize()
    for _, check in outs.values():
        check()
    w, _ = run_brd(c, "train_u", u, 0.5, 0)
    for k in outs:
        assert _bits(o[k].view(w[k].shape), w[k]), k


def test_one_row_and_cumulative_momentum_are_refused():
    """Training-mode statistics of ONE row: torch raises ValueError ("Expected more than 1 value per channel when training"); so do
    the wrappers, from metadata (the variance would be 0 and its unbiased form 0 / 0).  momentum=None asks for the cumulative average,
    which the kernels do not form: ValueError where the running statistics would be updated, served where they are not."""
    C = 64
    z = torch.randn(1, C, device="cuda")
    ga, rm = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    with pytest.raises(ValueError):
        ops.bn_relu_drop_fwd(z, ga, rm, rm.clone(), ga.clone(), 0.1, 1e-5, True, None, 0.0)
    with pytest.raises(ValueError):
        ops.bn_rows_fwd(z, ga, rm, rm.clone(), ga.clone(), 0.1, 1e-5, True, False)
    ops.bn_relu_drop_fwd(z, ga, rm, rm.clone(), ga.clone(), 0.1, 1e-5, False, None, 0.0)          # eval: one row is fine
    ops.bn_rows_fwd(z, ga, rm, rm.clone(), ga.clone(), 0.1, 1e-5, False, False)
    bn = torch.nn.BatchNorm1d(C, momentum=None).cuda()
    with torch.no_grad():
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 1.5)
    z = torch.randn(8, C, device="cuda")
    for fn in (lambda: HF.bn_relu_drop(z, bn, None, 0.0, True), lambda: HF.bn_rows(z, bn, True), lambda: HF.bn_rows_train(z, bn)):
        with pytest.raises(ValueError):
            fn()
    ref = torch.nn.BatchNorm1d(C, momentum=0.1).cuda()
    ref.load_state_dict(bn.state_dict())
    assert _bits(HF.bn_relu_drop(z, bn, None, 0.0, False).detach(), HF.bn_relu_drop(z, ref, None, 0.0, False).detach())
    assert _bits(HF.bn_rows(z, bn, False).detach(), HF.bn_rows(z, ref, False).detach())
    free = torch.nn.BatchNorm1d(C, momentum=None, track_running_stats=False).cuda()          # no running statistics: nothing to average
    assert bool(torch.isfinite(HF.bn_rows(z, free, True).detach()).all()) and bool(torch.isfinite(HF.bn_relu_drop(z, free, None, 0.0, True).detach()).all())


# ============================================================================================== 6. the wrappers
def _wrapper_calls():
    """name -> (function of a dict of tensors, the dict).  Every tensor argument of the wrappers of this file's families, valid."""
    c = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in G.cls_inputs(2, 5, 64, 1).items()}
    feat, amax, mean, rstd = ops.cls_pool_fwd(c["x"], c["gamma"], c["beta"], c["eps"])
    e = {k: v.cuda() for k, v in G.ce_inputs(5, 7, 1).items()}
    n = {k: v.cuda() for k, v in nll_case(9, 5, 1).items()}
    s = noise_case(2, 9, 4, 1)
    s = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
    b = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in G.bn_inputs(6, 64, 1).items()}
    u = G.dropout_uniforms((6, 64), 0.5, 1).cuda()
    _, bmean, brstd = ops.bn_relu_drop_fwd(b["z"], b["gamma"], b["beta"], b["rm"].clone(), b["rv"].clone(), 0.1, 1e-5, True, u, 0.5)
    return {
        "cls_pool_fwd": (lambda t: ops.cls_pool_fwd(t["x"], t["gamma"], t["beta"], 1e-5), dict(x=c["x"], gamma=c["gamma"], beta=c["beta"])),
        "cls_pool_bwd": (lambda t: ops.cls_pool_bwd(t["g_feat"], t["x"], t["mean"], t["rstd"], t["gamma"], t["amax"]),
                         dict(g_feat=c["g_feat"], x=c["x"], mean=mean, rstd=rstd, gamma=c["gamma"], amax=amax)),
        "ce_acc": (lambda t: ops.ce_acc(t["logits"], t["labels"]), dict(logits=e["logits"], labels=e["labels"])),
        "nll_mean_bwd": (lambda t: ops.nll_mean_bwd(t["g_loss"], t["target"], 9, 5), dict(g_loss=n["g_loss"], target=n["target"])),
        "noise_loss_bwd": (lambda t: ops.noise_loss_bwd(t["g_loss"], t["pred"], t["nv"], 4), dict(g_loss=s["g_loss"], pred=s["pred"], nv=s["nv"])),
        "bn_relu_drop_fwd": (lambda t: ops.bn_relu_drop_fwd(t["z"], t["gamma"], t["beta"], t["rm"], t["rv"], 0.1, 1e-5, True, t["u"], 0.5),
                             dict(z=b["z"], gamma=b["gamma"], beta=b["beta"], rm=b["rm"], rv=b["rv"], u=u)),
        "bn_relu_drop_bwd": (lambda t: ops.bn_relu_drop_bwd(t["g"], t["z"], t["gamma"], t["beta"], t["mean"], t["rstd"], True, t["u"], 0.5),
                             dict(g=b["g"], z=b["z"], gamma=b["gamma"], beta=b["beta"], mean=bmean, rstd=brstd, u=u)),
    }


def bad_versions(t):
    """Ways to pass the wrong thing for tensor t, each of which an unguarded launch would still read INSIDE allocated memory: another
    dtype of the same shape, a larger first / last dimension, a non-contiguous view of a larger buffer with t's shape, and (never launched)
    a CPU tensor."""
    big = torch.zeros(tuple(2 * n for n in t.shape), dtype=t.dtype, device="cuda")
    strided = big[tuple(slice(0, 2 * n, 2) for n in t.shape)]
    assert strided.shape == t.shape and (t.numel() == 1 or not strided.is_contiguous())
    other = t.double() if t.dtype.is_floating_point else (t.int() if t.dtype == torch.int64 else t.long())
    first = torch.zeros((t.shape[0] + 1,) + tuple(t.shape[1:]), dtype=t.dtype, device="cuda")
    last = torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 1,), dtype=t.dtype, device="cuda") if t.dim() > 1 else None
    return dict(dtype=other, first=first, last=last, view=strided if t.numel() > 1 else None, cpu=t.cpu())


# the tensor that DEFINES a size nothing else pins: a larger one is another valid call
DEFINES = {("cls_pool_fwd", "x", "first"), ("ce_acc", "logits", "last"), ("bn_rows_fwd", "x", "first"),
           ("interp_fwd", "out", "last"),
           ("chamfer_loss", "dist1", "last"), ("chamfer_loss", "dist2", "last")}          # (tests/test_gpu_losses.py: n and m of the two distance arrays)


def refuse_wrong_tensors(name, fn, tensors):
    fn(tensors)                                                   # the valid call passes
    n = 0
    for k, t in tensors.items():
        for kind, bad in bad_versions(t).items():
            if bad is None or (name, k, kind) in DEFINES:
                continue
            with pytest.raises((RuntimeError, TypeError)):
                fn({**tensors, k: bad})
            n += 1
        if t.dim() == 2 and t.shape[0] != t.shape[1]:             # the transposed view of a matrix (right numel, wrong shape, strided)
            with pytest.raises(RuntimeError):
                fn({**tensors, k: t.t()})
    assert n >= 4 * len(tensors) - 2


WRAPPERS = ("cls_pool_fwd", "cls_pool_bwd", "ce_acc", "nll_mean_bwd", "noise_loss_bwd", "bn_relu_drop_fwd", "bn_relu_drop_bwd")


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrappers_refuse_wrong_tensors(name):
    """Device, dtype, contiguity and the exact shape of every tensor a wrapper passes on, from metadata alone: a float64 or transposed
    operand, a label vector of another length or a CPU tensor used to be read as raw memory of the expected type and shape."""
    fn, tensors = _wrapper_calls()[name]
    refuse_wrong_tensors(name, fn, tensors)
