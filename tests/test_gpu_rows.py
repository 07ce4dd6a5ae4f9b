"""The per-point row kernels of csrc/pointwise.hip -- bn_rows_fwd / bwd and their dropout forms (partial -> f64 finalize -> flat vec4 /
flat scalar / tall / non-temporal apply), sqdist_topk<1/2/4> (bitonic and selection forms), interp_kernel<4/8/16>, interp_wide_kernel
(+ affine), interp_bwd_kernel (wide, narrow and chunked branch), interp_bwd_dense_kernel<4/8>, interp_geo_bwd + interp_geo_src,
group_max_fwd / bwd, posenc -- against the float64 reference of tests/_head_reference.py, with shapes picked to reach each dispatch
branch, slab remainder and tile edge, and the limits that return a status.

The bound, for every output and every case (tests/test_gpu_prop.py, tests/test_gpu_tail.py):
    err(x) = max|x - f64| / max|f64|,      err(kernel) <= max(2 * err(f32), 2e-6)
where f32 is the SAME formulation run by torch in float32 on the GPU with the selections (ReLU gates, neighbour lists, arg-max rows) of the
float64 run.  Exact checks -- neighbour indices and distances on lattice clouds, arg-max rows and the values they select, zeros for
unreferenced source rows, untouched columns of a wider output, the ReLU gate between forward and backward, the dropout mask between the
tall and the flat path and between forward and backward, determinism of a second call, guards -- are bit equalities.  Inputs live in
NaN-guarded buffers; one float off the 16-byte alignment wherever the kernel loads single floats (the vector paths of bn_rows, the wide
and dense interpolation kernels and group_max take 16-byte pieces: those get aligned buffers; group_max, upp_interp_affine_fwd and
bn_rows with C % 4 == 0 answer a shifted pointer with UPP_E_RANGE, interp_fwd / interp_bwd fall back to their single-float kernels -- all
pinned).  The generators (tests/test_head_host.py) make every selection agree between the precisions by construction.

Measured on MI355X: (kernel, f32) of the case nearest its bound, per family and output (number of judged outputs).  129 tests; with
tests/test_gpu_head.py's 281 in one run, 7.9 s for the 410 (tests/test_gpu_tail.py: 5 s for 209, tests/test_gpu_prop.py: 6 s for 180); the slowest
cases are the two deliberately large non-temporal ones, (104,860, 320) 0.17 s and (65,536, 512) 0.12 s, beside lattice_clouds[1] 0.17 s and
bn_rows_shapes[4096-512] 0.14 s.  The nearest any output comes to
its bound is 0.76 of it.
    bn_rows (46)        y 1.0e-6, 1.5e-7       mean 1.5e-6, 3.1e-7    rstd 1.2e-6, 1.5e-7    running_mean 1.3e-7, 6.6e-8    running_var 1.5e-6, 8.3e-8
                        g_x 2.7e-3, 2.7e-3     g_gamma 1.5e-6, 1.5e-6 g_beta 3.1e-7, 5.8e-7
    sqdist_topk (8)     dist 6.4e-8, 7.9e-8 (of max(|a|^2 + |b|^2)); lattice clouds: bit-equal
    interp_fwd (57)     out 3.0e-7, 1.3e-7
    interp_bwd (19)     g_feat 4.9e-7, 2.0e-6
    interp_geo (12)     g_xyz1 1.8e-7, 8.0e-8  g_xyz2 2.5e-7, 4.6e-7
    posenc (6)          out 1.1e-5, 1.1e-5
    group_max: a selection, bit-equal.
bn_rows' mean, rstd and y at 1e-6 are (65,536, 512): 256 float32 slab sums of 256 rows each (the finalize adds them in f64) against torch's
own tree; under the 2e-6 floor.  g_x 2.7e-3 is R = 2 (two rows: xhat = +-1 up to the rounding of eps), posenc 1.1e-5 the product f x at
f = 402 rounded to float32 before the sine, in the kernel and in torch alike.

What was found and fixed, the four hypotheses of the issue and the mutant runs are recorded in tests/test_gpu_head.py (sqdist_topk's NaN
image and the wrappers ops.bn_rows_fwd / interp_fwd / group_max_bwd are this file's share).  No other case of this file missed the bound on
the kernels as they were.
"""
import numpy as np
import pytest
import torch

import _head_reference as R
import test_head_host as G
from test_gpu_head import E_BADARG, E_RANGE, _cuda, _same, _sentinel, _untouched, judge as _judge, refuse_wrong_tensors
from test_gpu_step_tail import guarded
from test_gpu_tail import _bits, gin
from upp_hip import _abi, ops

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
EPS = 1e-8          # the interpolation's (reference models/Point_MAE_pretask_dev.py:455)


def judge(family, label, got, f32, f64, keys):
    _judge(family, label, got, f32, f64, keys, tag="ROWSERR")


# ============================================================================================== 1. bn_rows
BN_KEYS = ("y", "mean", "rstd", "running_mean", "running_var", "g_x", "g_gamma", "g_beta")


def bn_per(Rr):
    return max(8, (Rr + 255) // 256)


def bn_case(Rr, C, seed, training=True, kind="rand", tile=1):
    """tile: the (R / tile, C) block of the generator repeated `tile` times down the rows -- the same column statistics (so the same
    |o| >= 1e-3) without a float64 pass over tens of millions of elements on the host."""
    assert Rr % tile == 0
    c = G.bn_inputs(Rr // tile, C, seed, training, kind, slab=bn_per(Rr))
    if tile > 1:
        c["z"], c["g"] = c["z"].repeat(tile, 1), c["g"].repeat(tile, 1)
    return c


def run_bn(c, training, relu, affine=True, running=True, want_gx=True, off=None):
    C = c["z"].shape[1]
    off = (0 if C % 4 == 0 else 1) if off is None else off
    t = {k: gin(c[k], off) for k in ("z", "gamma", "beta", "rm", "rv", "g")}
    if not affine:
        t["gamma"] = t["beta"] = None
    if not running:
        t["rm"] = t["rv"] = None
    y, mean, rstd = ops.bn_rows_fwd(t["z"], t["gamma"], t["beta"], t["rm"], t["rv"], c["momentum"], c["eps"], training, relu, want_stats=True)
    g_x, g_gamma, g_beta = ops.bn_rows_bwd(t["z"], t["g"], mean, rstd, t["gamma"], t["beta"], relu, want_gx=want_gx) if training else (None,) * 3
    return dict(y=y, mean=mean, rstd=rstd, running_mean=t["rm"] if training else None, running_var=t["rv"] if training else None,
                g_x=g_x, g_gamma=g_gamma, g_beta=g_beta)


def check_bn(c, label, training=True, relu=True, affine=True, running=True, want_gx=True):
    a, b = run_bn(c, training, relu, affine, running, want_gx), run_bn(c, training, relu, affine, running, want_gx)
    _same(a, b, "second run differs")
    d = _cuda(c, ("z", "gamma", "beta", "rm", "rv", "g"))
    if not affine:
        d["gamma"] = d["beta"] = None
    if not running:
        d["rm"] = d["rv"] = None
    gate = R.bn_select(d["z"], d["gamma"], d["beta"], d["rm"], d["rv"], c["eps"], training) if relu else None
    ref = {dt: R.batch_norm(d["z"], d["gamma"], d["beta"], d["rm"], d["rv"], c["momentum"], c["eps"], training, gate, None, 0.0, dt,
                            d["g"] if training else None, want_gz=want_gx) for dt in (F32, F64)}
    for r in ref.values():
        r["y"], r["g_x"] = r["a"], r["g_z"]
    if relu:
        assert torch.equal(a["y"] > 0, gate > 0), "the ReLU gate"
    judge("bn_rows", label, a, ref[F32], ref[F64], BN_KEYS)


BN_SHAPES = [(7, 3), (5, 5), (1000, 300), (33, 12),                                  # flat: scalar with a ragged last thread, vec4
             (2, 12), (8, 5), (9, 12), (2047, 5), (2049, 12), (4101, 5),            # slab remainders: per = max(8, ceil(R / 256))
             (4095, 64), (4096, 64), (4099, 64), (4098, 128), (4097, 256), (4096, 512)]   # the tall path at its threshold: rpw = 4, 2, 1, grid.y = 2


@pytest.mark.parametrize("Rr,C", BN_SHAPES)
def test_bn_rows_shapes(Rr, C):
    i = BN_SHAPES.index((Rr, C))
    check_bn(bn_case(Rr, C, Rr + C), "R=%d C=%d" % (Rr, C), relu=i % 2 == 0)
    check_bn(bn_case(Rr, C, Rr + C + 1, kind="offset"), "R=%d C=%d offset" % (Rr, C), relu=i % 2 == 1)


@pytest.mark.parametrize("Rr,C,tile", [(65536, 512, 64), (104860, 320, 20)])
def test_bn_rows_non_temporal(Rr, C, tile):
    """R C >= 2^25: the tall and the flat apply kernels stream with non-temporal loads and stores.  (Deliberately large.)"""
    check_bn(bn_case(Rr, C, 5, tile=tile), "R=%d C=%d" % (Rr, C))


@pytest.mark.parametrize("Rr,C", [(33, 12), (1000, 5), (4099, 64)])
def test_bn_rows_options(Rr, C):
    """No affine parameters, no running statistics, no g_x, eval mode -- on the flat vec4, the flat scalar and the tall path."""
    c = bn_case(Rr, C, 3)
    check_bn(c, "R=%d C=%d no affine" % (Rr, C), affine=False)
    check_bn(c, "R=%d C=%d no running" % (Rr, C), running=False)
    check_bn(c, "R=%d C=%d no g_x" % (Rr, C), want_gx=False)
    check_bn(bn_case(Rr, C, 4, training=False), "R=%d C=%d eval" % (Rr, C), training=False)


def _recover_gate(c, mean, rstd, g_x, g_gamma, g_beta):
    """gm of g_x = gamma rstd (gm - (g_beta + xh g_gamma) / R), in float64 from the kernel's own outputs."""
    z, ga = c["z"].cuda().double(), c["gamma"].cuda().double()
    xh = (z - mean.double()) * rstd.double()
    return g_x.double() / (ga * rstd.double()) + (g_beta.double() + xh * g_gamma.double()) / z.shape[0]


@pytest.mark.parametrize("Rr,C", [(4096, 64), (4099, 256), (1000, 12), (1000, 5)])
def test_bn_rows_gate_is_the_same_forward_and_backward(Rr, C):
    """Pre-activations within a few ulp of 0 (many exactly 0): with g = 1, g_beta[c] is EXACTLY the number of positive outputs of column
    c, and the gate g_x was computed with is that of y -- on the tall, the flat vec4 and the flat scalar apply path.  Eval-mode forward
    (mean = running_mean, rstd from running_var), then the backward with those statistics."""
    g = torch.Generator().manual_seed(Rr + C)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 + 0.2 * torch.rand(C, generator=g)
    rm, rv = 0.2 * torch.randn(C, generator=g), 0.6 + torch.rand(C, generator=g)
    rstd = 1.0 / torch.sqrt(rv + np.float32(1e-5))
    j = torch.randint(-4, 5, (Rr, C), generator=g).float()
    z = rm + (-beta / (gamma * rstd)) * (1.0 + j * 2.0 ** -23)
    c = dict(z=z, gamma=gamma, beta=beta, rm=rm, rv=rv, g=torch.ones(Rr, C), eps=1e-5, momentum=0.1)
    off = 0 if C % 4 == 0 else 1
    t = {k: gin(c[k], off) for k in ("z", "gamma", "beta", "rm", "rv", "g")}
    y, mean, rstd_k = ops.bn_rows_fwd(t["z"], t["gamma"], t["beta"], t["rm"], t["rv"], 0.1, 1e-5, False, True, want_stats=True)
    pos = y > 0
    frac = float(pos.float().mean())
    assert 0.1 < frac < 0.9 and bool((y[~pos] == 0).all()), frac
    o = ops.bn_rows_fwd(t["z"], t["gamma"], t["beta"], t["rm"], t["rv"], 0.1, 1e-5, False, False)
    assert torch.equal(o > 0, pos) and int((o == 0).sum()) > 0 and float(o.abs().max()) < 1e-5, "pre-activations at and around an exact 0"
    g_x, g_gamma, g_beta = ops.bn_rows_bwd(t["z"], t["g"], mean, rstd_k, t["gamma"], t["beta"], True)
    assert torch.equal(g_beta, pos.sum(0).float()), "g_beta of g = 1 counts the positive outputs"
    gm = _recover_gate(c, mean, rstd_k, g_x, g_gamma, g_beta)
    assert float((gm - gm.round()).abs().max()) < 1e-3 and torch.equal(gm.round() > 0, pos), "the gate of g_x"


def test_bn_rows_dropout_mask_is_one_function_of_the_flat_index():
    """relu off, beta large: the mask is y != 0.  One seed and salt: the same mask by flat element index on the tall path (4096, 64) and
    the flat path (2048, 128), the same mask forward and backward, and g_beta of g = 1 = the kept count / (1 - p)."""
    p, salt = 0.5, 77
    seed = torch.tensor([12345], dtype=torch.int64, device="cuda")
    masks = []
    for Rr, C in ((4096, 64), (2048, 128)):
        c = bn_case(Rr, C, 9)
        c["beta"] = c["beta"] + 50.0
        c["g"] = torch.ones(Rr, C)
        t = {k: gin(c[k], 0) for k in ("z", "gamma", "beta", "rm", "rv", "g")}
        drop = (p, seed, 0, salt)
        y, mean, rstd = ops.bn_rows_fwd(t["z"], t["gamma"], t["beta"], t["rm"], t["rv"], 0.1, 1e-5, True, False, want_stats=True, drop=drop)
        y0 = ops.bn_rows_fwd(t["z"], t["gamma"], t["beta"], None, None, 0.1, 1e-5, True, False)
        keep = y != 0
        assert 0.45 < float(keep.float().mean()) < 0.55 and _bits(y[keep], (y0 * np.float32(1.0 / (1.0 - p)))[keep])
        g_x, g_gamma, g_beta = ops.bn_rows_bwd(t["z"], t["g"], mean, rstd, t["gamma"], t["beta"], False, drop=drop)
        want = keep.double().sum(0) / (1.0 - p)
        assert float((g_beta.double() - want).abs().max()) <= 2e-6 * float(want.max())
        gm = _recover_gate(c, mean, rstd, g_x, g_gamma, g_beta) * (1.0 - p)
        assert float((gm - gm.round()).abs().max()) < 1e-3 and torch.equal(gm.round() > 0, keep), "the mask of the backward"
        y2 = ops.bn_rows_fwd(t["z"], t["gamma"], t["beta"], None, None, 0.1, 1e-5, True, False, drop=(p, seed + 1, 0, salt))
        assert not torch.equal(y2 != 0, keep), "another seed, another mask"
        masks.append(keep.reshape(-1))
    assert torch.equal(masks[0], masks[1])


def test_bn_rows_c_entry_points_with_guarded_outputs():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    for Rr, C in ((4099, 64), (2049, 12), (9, 5)):
        c = bn_case(Rr, C, 6)
        off = 0 if C % 4 == 0 else 1
        t = {k: gin(c[k], off) for k in ("z", "gamma", "beta", "rm", "rv", "g")}
        nparts = int(lib.upp_bn_rows_part_floats(Rr, C))
        outs = {k: guarded(n, F32, off) for k, n in (("part", nparts), ("mean", C), ("rstd", C), ("y", Rr * C), ("part2", nparts), ("g_gamma", C),
                                                      ("g_beta", C), ("g_x", Rr * C))}
        o = {k: v[0] for k, v in outs.items()}
        assert lib.upp_bn_rows_fwd(p(t["z"]), p(t["gamma"]), p(t["beta"]), p(t["rm"]), p(t["rv"]), 0.1, 1e-5, 1, 1, p(o["part"]), p(o["mean"]),
                                   p(o["rstd"]), p(o["y"]), Rr, C, st) == 0
        assert lib.upp_bn_rows_bwd(p(t["z"]), p(t["g"]), p(o["mean"]), p(o["rstd"]), p(t["gamma"]), p(t["beta"]), 1, p(o["part2"]), p(o["g_gamma"]),
                                   p(o["g_beta"]), p(o["g_x"]), Rr, C, st) == 0
        torch.cuda.synchronize()
        for _, check in outs.values():
            check()
        w = run_bn(c, True, True)
        for k in ("y", "mean", "rstd", "g_x", "g_gamma", "g_beta"):
            assert _bits(o[k].view(w[k].shape), w[k]), k


def test_vector_paths_refuse_a_pointer_off_16_bytes():
    """The kernels that move 16-byte pieces answer a pointer one float off with UPP_E_RANGE before anything is launched: bn_rows with
    C % 4 == 0 (the matrices; on the tall path the column vectors too) and upp_interp_affine_fwd (feat, out, wt -- and k > 4, C < 256,
    C % 4 != 0).  C % 4 != 0 loads single floats (every such shape above runs one float off), and so does the backward without g_x."""
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    for Rr, C in ((33, 12), (4099, 64)):
        c = bn_case(Rr, C, 2)
        t0 = {k: gin(c[k], 0) for k in ("z", "gamma", "beta", "rm", "rv", "g")}
        t1 = {k: gin(c[k], 1) for k in ("z", "gamma", "beta", "rm", "rv", "g")}
        n = int(lib.upp_bn_rows_part_floats(Rr, C))
        part, mean, rstd, gg, gb = (torch.zeros(m, device="cuda") for m in (n, C, C, C, C))
        y, gx = _sentinel((Rr * C + 4,)), _sentinel((Rr * C + 4,))
        m1, ga1 = torch.zeros(C + 4, device="cuda")[1:C + 1], gin(c["gamma"], 1)

        def fwd(x, gamma, mean_, out):
            return lib.upp_bn_rows_fwd(p(x), p(gamma), p(t0["beta"]), p(t0["rm"]), p(t0["rv"]), 0.1, 1e-5, 1, 1, p(part), p(mean_), p(rstd), p(out), Rr, C, st)

        def bwd(x, g, gamma, g_gamma, out):
            return lib.upp_bn_rows_bwd(p(x), p(g), p(mean), p(rstd), p(gamma), p(t0["beta"]), 1, p(part), p(g_gamma), p(gb), p(out), Rr, C, st)

        assert fwd(t1["z"], t0["gamma"], mean, y) == E_RANGE and fwd(t0["z"], t0["gamma"], mean, y[1:]) == E_RANGE
        assert bwd(t1["z"], t0["g"], t0["gamma"], gg, gx) == E_RANGE and bwd(t0["z"], t1["g"], t0["gamma"], gg, gx) == E_RANGE
        assert bwd(t0["z"], t0["g"], t0["gamma"], gg, gx[1:]) == E_RANGE
        if Rr >= 4096:                                            # the tall path reads the column vectors in 16-byte pieces too
            assert fwd(t0["z"], ga1, mean, y) == E_RANGE and fwd(t0["z"], t0["gamma"], m1, y) == E_RANGE
            assert bwd(t0["z"], t0["g"], ga1, gg, gx) == E_RANGE and bwd(t0["z"], t0["g"], t0["gamma"], m1, gx) == E_RANGE
        else:                                                     # the flat path reads them float by float
            assert fwd(t0["z"], ga1, mean, y) == 0
            y[:] = float("nan")
        assert _untouched(y, gx)
        with pytest.raises(RuntimeError):
            ops.bn_rows_fwd(t1["z"], t0["gamma"], t0["beta"], t0["rm"], t0["rv"], 0.1, 1e-5, True, True)
        # without g_x nothing is read in 16-byte pieces: served, same bits
        w = run_bn(c, True, True, want_gx=False, off=0)
        mean.copy_(w["mean"]); rstd.copy_(w["rstd"])
        assert lib.upp_bn_rows_bwd(p(t1["z"]), p(t1["g"]), p(mean), p(rstd), p(ga1), p(t1["beta"]), 1, p(part), p(gg), p(gb), None, Rr, C, st) == 0
        assert _bits(gg, w["g_gamma"]) and _bits(gb, w["g_beta"])
    c = interp_case(2, 16, 9, 256, 3, 1, ld=5)
    d = _cuda(c, ("dist", "idx", "feat"))
    x3, wt, out = torch.zeros(2, 16, 3, device="cuda"), torch.zeros(3 * 260 + 4, device="cuda"), _sentinel((2 * 16 * 260 + 4,))
    feat1 = gin(c["feat"], 1)

    def affine(feat, wt_, out_, C=256, k=3):
        return lib.upp_interp_affine_fwd(p(d["dist"]), p(d["idx"]), 5, p(feat), p(x3), p(wt_), p(out_), 2, 16, 9, C, k, EPS, st)

    assert affine(d["feat"], wt, out) == 0
    out[:] = float("nan")
    assert affine(feat1, wt, out) == E_RANGE and affine(d["feat"], wt[1:], out) == E_RANGE and affine(d["feat"], wt, out[1:]) == E_RANGE
    assert affine(d["feat"], wt, out, k=5) == E_RANGE and affine(d["feat"], wt, out, C=252) == E_RANGE and affine(d["feat"], wt, out, C=258) == E_RANGE
    assert _untouched(out)


# ============================================================================================== 2. sqdist_topk
TOPK_S = (1, 5, 63, 64, 65, 128, 129, 256)
TOPK_K = (1, 4, 5, 16, 64)


def run_topk(q, src, k, off=1):
    dist, idx = ops.sqdist_topk(gin(q, off), gin(src, off), k)
    return dict(dist=dist, idx=idx)


@pytest.mark.parametrize("S", TOPK_S)
def test_sqdist_topk_on_lattice_clouds_is_exact(S):
    """Coordinates i / 64: every product is exact in float32, so indices AND distances equal the float64 sort bit for bit, ties go to the
    lowest index, and k = S lists every point once.  S <= 64 with k > 4 takes the bitonic form, the rest the selection forms with 1, 2
    and 4 candidates per lane; 2 x 7 = 14 rows leave the last workgroup half empty."""
    q, src = G.lattice_cloud(2, 7, S), G.lattice_cloud(2, S, S + 1, span=3)          # a coarse source lattice: many exact ties
    d64 = R.sqdist(q.cuda(), src.cuda(), F64)
    assert torch.equal(d64, R.sqdist(q.cuda(), src.cuda(), F32).double())
    ties = 0
    for k in sorted({k for k in TOPK_K if k <= S} | {S if S <= 64 else 64}):
        a, b = run_topk(q, src, k, 1), run_topk(q, src, k, 0)
        _same(a, b, "second run (other alignment) differs")
        wd, wi = R.topk_select(d64, k)
        assert torch.equal(a["idx"], wi) and torch.equal(a["dist"].double(), wd), (S, k)
        ties += int((wd[..., 1:] == wd[..., :-1]).sum())
        if k == S:
            assert torch.equal(a["idx"].sort(-1).values, torch.arange(S, device="cuda").expand(2, 7, S))
    assert S < 63 or ties > 0


@pytest.mark.parametrize("S,k", [(5, 4), (63, 16), (64, 5), (65, 16), (128, 64), (129, 4), (256, 16), (256, 64)])
def test_sqdist_topk_on_random_clouds_within_the_bound(S, k):
    """Every returned distance against the float64 |a - b|^2 of the returned point, relative to max(|a|^2 + |b|^2) -- the three-term form
    cancels against that scale; no returned point farther than the true k-th by more than the same margin; and, with the generator's gap
    of 1e-3 of the scale between ranks k - 1 and k, the LIST is the float64 one."""
    q, src, scale = G.random_cloud(2, 7, S, k, S + k)
    a, b = run_topk(q, src, k, 1), run_topk(q, src, k, 0)
    _same(a, b, "second run (other alignment) differs")
    qc, sc = q.cuda(), src.cuda()
    true = ((qc.double().unsqueeze(2) - sc.double().unsqueeze(1)) ** 2).sum(-1)
    ef = float((R.sqdist(qc, sc, F32).double() - true).abs().max()) / scale
    margin = max(2.0 * ef, 2e-6)
    ek = float((a["dist"].double() - true.gather(-1, a["idx"])).abs().max()) / scale
    print("ROWSERR | sqdist_topk | S=%d k=%d | dist | %.2e | %.2e" % (S, k, ek, ef))
    assert ek <= margin
    kth = true.sort(-1).values[..., k - 1:k]
    assert float((true.gather(-1, a["idx"]) - kth).max()) <= margin * scale
    assert torch.equal(a["idx"].sort(-1).values, true.sort(-1).indices[..., :k].sort(-1).values)
    assert bool((a["dist"][..., 1:] >= a["dist"][..., :-1]).all())


@pytest.mark.parametrize("S,ks", [(5, (1, 4, 5)), (64, (4, 16, 64)), (65, (5, 64)), (129, (16,)), (256, (4, 64))])
def test_sqdist_topk_ranks_a_nan_point_last(S, ks):
    """A source point with a NaN coordinate, with either sign bit: absent from every list with k < S, last with k = S -- as
    square_distance(...).sort() and argsort_rows rank it.  (The raw order-preserving image of a NaN whose sign bit is set is the smallest.)"""
    q, src = G.lattice_cloud(2, 7, S), G.lattice_cloud(2, S, S + 1)
    neg_nan = torch.tensor([float("nan")]).view(torch.int32).bitwise_or(torch.tensor([-2 ** 31], dtype=torch.int32)).view(torch.float32)
    pos_nan = torch.tensor([float("nan")]).view(torch.int32).bitwise_and(torch.tensor([2 ** 31 - 1], dtype=torch.int32)).view(torch.float32)
    for nan, where in ((neg_nan, 0), (pos_nan, S // 2), (neg_nan, S - 1)):
        s2 = src.clone()
        s2[:, where, where % 3] = nan
        d64 = R.sqdist(q.cuda(), s2.cuda(), F64)
        for k in ks:
            a = run_topk(q, s2, k)
            wd, wi = R.topk_select(d64, k)
            assert torch.equal(a["idx"], wi), (S, k, where)
            if k < S:
                assert not bool((a["idx"] == where).any()) and torch.equal(a["dist"].double(), wd)
            else:
                assert bool((a["idx"][..., -1] == where).all()) and bool(torch.isnan(a["dist"][..., -1]).all())
                assert torch.equal(a["dist"][..., :-1].double(), wd[..., :-1])


@pytest.mark.parametrize("S,k", [(65, 5), (20, 16), (256, 64)])
def test_sqdist_topk_c_entry_point_with_guarded_outputs(S, k):
    """14 rows for workgroups of four, `lane < k` stores of dist and of the int64 idx: both between guards."""
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    q, src = G.lattice_cloud(2, 7, S), G.lattice_cloud(2, S, S + 1)
    (dist, ck1), (idx, ck2) = guarded(2 * 7 * k, F32, 1), guarded(2 * 7 * k, torch.int64, 1)
    assert lib.upp_sqdist_topk(p(gin(q, 1)), p(gin(src, 1)), p(dist), p(idx), 2, 7, S, k, st) == 0
    torch.cuda.synchronize()
    ck1(); ck2()
    w = run_topk(q, src, k, 0)
    assert _bits(dist.view(2, 7, k), w["dist"]) and torch.equal(idx.view(2, 7, k), w["idx"])


def test_sqdist_topk_limits():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    q, src = torch.zeros(1, 4, 3, device="cuda"), torch.zeros(1, 257, 3, device="cuda")
    dist, idx = _sentinel((1, 4, 65)), _sentinel((1, 4, 65), torch.int64)
    assert lib.upp_sqdist_topk(p(q), p(src), p(dist), p(idx), 1, 4, 257, 4, st) == E_RANGE          # S = 257
    assert lib.upp_sqdist_topk(p(q), p(src), p(dist), p(idx), 1, 4, 256, 65, st) == E_RANGE         # k = 65
    assert lib.upp_sqdist_topk(p(q), p(src), p(dist), p(idx), 1, 4, 8, 9, st) == E_RANGE            # k > S
    assert _untouched(dist, idx)
    with pytest.raises(RuntimeError):
        ops.sqdist_topk(q, src, 4)


# ============================================================================================== 3. interpolation, forward
def interp_case(B, N, S, C, k, seed, ld=None, first=None, S_used=None, d0=False):
    g = torch.Generator().manual_seed(seed)
    dist, idx = G.neighbour_table(B, N, S if S_used is None else S_used, k, seed, ld=ld, first=first)
    if d0:
        dist[:, ::2, 0] = 0.0                                 # a query ON a source point
        dist[:, 1::4, 0] = -1e-9                              # ... and what the three-term form makes of it
        assert float(dist.min()) + np.float32(EPS) > 0
    return dict(dist=dist, idx=idx, feat=torch.randn(B, S, C, generator=g), g_out=torch.randn(B, N, C, generator=g), k=k, S=S, C=C)


def check_interp_fwd(c, label, off, col0=0, width=None, affine=False):
    B, N, C = c["g_out"].shape
    dist, idx, feat = gin(c["dist"], off), gin(c["idx"], off), gin(c["feat"], off)
    d = _cuda(c, ("dist", "idx", "feat"))
    x3 = wt = None
    if affine:
        g = torch.Generator().manual_seed(C)
        x3, wt = torch.randn(B, N, 3, generator=g), torch.randn(3, C, generator=g)
        got = ops.interp_affine_fwd(dist, idx, feat, gin(x3, off), gin(wt, 0), c["k"], EPS)
        again = ops.interp_affine_fwd(dist, idx, feat, gin(x3, off), gin(wt, 0), c["k"], EPS)
        x3, wt = x3.cuda(), wt.cuda()
    elif width is None:
        got, again = ops.interp_fwd(dist, idx, feat, c["k"], EPS), ops.interp_fwd(dist, idx, feat, c["k"], EPS)
    else:
        buf, check = guarded(B * N * width, F32, off)
        buf.copy_(torch.arange(B * N * width, device="cuda").float())
        before = buf.clone().view(B, N, width)
        out = ops.interp_fwd(dist, idx, feat, c["k"], EPS, out=buf.view(B, N, width), col0=col0)
        check()
        keep = torch.ones(width, dtype=torch.bool, device="cuda")
        keep[col0:col0 + C] = False
        assert _bits(out[..., keep], before[..., keep]), "columns outside the window"
        got = out[..., col0:col0 + C]
        again = ops.interp_fwd(dist, idx, feat, c["k"], EPS, out=before.clone(), col0=col0)[..., col0:col0 + C]
    assert _bits(got.contiguous(), again.contiguous()), "second run differs"
    ref = {dt: R.interp(d["dist"], d["idx"], d["feat"], c["k"], EPS, dt, x3, wt) for dt in (F32, F64)}
    judge("interp_fwd", label, dict(out=got), ref[F32], ref[F64], ("out",))


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 9, 16])
def test_interp_forward_narrow(k):
    """interp_kernel<4 | 8 | 16> by k, C below, at and between the powers of two its thread groups are sized by, k = S, d = 0 and d < 0."""
    for i, C in enumerate((1, 3, 12, 32, 255)):
        S = k if i == 0 else k + 3 + i
        check_interp_fwd(interp_case(2, 7, S, C, k, 10 * k + C, ld=k + i % 2, d0=i % 2 == 0), "k=%d C=%d S=%d" % (k, C, S), off=1)


def test_interp_forward_into_a_window_of_a_wider_buffer():
    """C = 300 at col0 = 5 (the narrow kernel, grid.y = 2) and the wide kernel at col0 = 4: the other columns keep their bits."""
    check_interp_fwd(interp_case(2, 7, 9, 300, 3, 1, ld=4), "C=300 col0=5", off=1, col0=5, width=309)
    check_interp_fwd(interp_case(2, 7, 9, 12, 5, 2), "C=12 col0=3", off=1, col0=3, width=16)
    check_interp_fwd(interp_case(2, 16, 9, 260, 3, 3, ld=5), "wide C=260 col0=4", off=0, col0=4, width=268)
    check_interp_fwd(interp_case(2, 16, 9, 256, 3, 4), "C=256 one float off: the single-float kernel", off=1)


@pytest.mark.parametrize("C", [256, 260, 512, 516, 1028])
def test_interp_forward_wide(C):
    """interp_wide_kernel (C >= 256, C % 4 == 0, k <= 4): one and two 256-column pieces per trip and their ragged ends, 32 rows (the
    XCD remap of the workgroup index) and 14, a table whose rows are longer than k, a query on a source point."""
    for i, (N, k) in enumerate(((16, 3), (7, 4), (16, 1))):
        check_interp_fwd(interp_case(2, N, 9, C, k, C + N, ld=k + 1 + i, d0=i == 1), "wide C=%d N=%d k=%d" % (C, N, k), off=0)
    if C in (256, 260):
        check_interp_fwd(interp_case(2, 16, 9, C, 3, C, ld=4), "affine C=%d N=16" % C, off=0, affine=True)
        check_interp_fwd(interp_case(2, 7, 9, C, 4, C + 1, d0=True), "affine C=%d N=7" % C, off=0, affine=True)


# ============================================================================================== 4. interpolation, backward
def check_interp_bwd(c, label, off, unreferenced=None):
    dist, idx, g_out = gin(c["dist"], off), gin(c["idx"], off), gin(c["g_out"], off)
    a, b = ops.interp_bwd(dist, idx, g_out, c["S"], c["k"], EPS), ops.interp_bwd(dist, idx, g_out, c["S"], c["k"], EPS)
    assert _bits(a, b), "second run differs"
    d = _cuda(c, ("dist", "idx", "feat", "g_out"))
    ref = {dt: R.interp(d["dist"], d["idx"], d["feat"], c["k"], EPS, dt, g_out=d["g_out"]) for dt in (F32, F64)}
    if unreferenced is not None:
        assert float(a[:, unreferenced].abs().max()) == 0.0 and float(ref[F64]["g_feat"][:, unreferenced].abs().max()) == 0.0
    judge("interp_bwd", label, dict(g_feat=a), ref[F32], ref[F64], ("g_feat",))


@pytest.mark.parametrize("S,N,k", [(32, 1, 16), (32, 159, 16), (32, 160, 16), (32, 161, 16), (32, 1096, 16), (64, 120, 3), (64, 121, 3), (64, 250, 16)])
def test_interp_backward_dense(S, N, k):
    """interp_bwd_dense_kernel: S = C = 32 runs eight waves on tiles of 160 rows, S = 64 four waves on tiles of 120; N around the tile.
    The last source row is never referenced: exact zeros."""
    check_interp_bwd(interp_case(2, N, S, 32, min(k, S - 1), S + N, S_used=S - 1), "dense S=%d N=%d" % (S, N), off=0, unreferenced=S - 1)


@pytest.mark.parametrize("C,S,N,k", [(1, 5, 9, 3), (3, 7, 15, 16), (36, 6, 40, 4), (129, 5, 9, 3), (256, 8, 33, 4), (300, 7, 9, 1), (2048, 5, 6, 3),
                                     (2052, 5, 6, 3)])
def test_interp_backward_pull(C, S, N, k):
    """interp_bwd_kernel: the narrow branch (C = 1, 3, 36; S % 4 != 0; N k < 256 leaves waves without entries), the wide one-pass branch
    (C = 129 ... 2048) and the chunked loop beyond it (C = 2052); B S = 10 ... 16 workgroups, with and without the XCD remap."""
    k = min(k, S - 1)
    check_interp_bwd(interp_case(2, N, S, C, k, C + S, ld=k + 1, S_used=S - 1, d0=True), "pull C=%d S=%d N=%d k=%d" % (C, S, N, k), off=1, unreferenced=S - 1)


@pytest.mark.parametrize("k,S,B", [(1, 8, 1), (16, 17, 1), (16, 20, 2)])
def test_interp_backward_fullest_hit_lists(k, S, B):
    """N = 4096, every row lists source 0 first: 1,024 hits per wave, the most the scan can produce (one per row)."""
    check_interp_bwd(interp_case(B, 4096, S, 3, k, k + S, first=0), "full N=4096 k=%d S=%d B=%d" % (k, S, B), off=1)


@pytest.mark.parametrize("C,S,N,k,off", [(32, 32, 159, 16, 0), (32, 32, 161, 16, 0), (32, 64, 121, 3, 0), (3, 7, 15, 6, 1), (256, 8, 33, 4, 1),
                                         (2052, 5, 6, 3, 1)])
def test_interp_backward_c_entry_point_with_guarded_output(C, S, N, k, off):
    """The dense tiles one row short of and past 160 / 120, the pull form with waves that own no entry, its wide branch and the chunked
    loop: g_feat between guards."""
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    c = interp_case(2, N, S, C, k, C + N, S_used=S - 1)
    dist, idx, g_out = gin(c["dist"], off), gin(c["idx"], off), gin(c["g_out"], off)
    g_feat, check = guarded(2 * S * C, F32, off)
    assert lib.upp_interp_bwd(p(dist), p(idx), k, p(g_out), C, 0, p(g_feat), 2, N, S, C, k, EPS, st) == 0
    torch.cuda.synchronize()
    check()
    assert _bits(g_feat.view(2, S, C), ops.interp_bwd(dist, idx, g_out, S, k, EPS))


@pytest.mark.parametrize("k,C", [(3, 65), (16, 1)])
def test_interp_geo_backward_c_entry_point_with_guarded_outputs(k, C):
    """g_xyz1, g_xyz2 and the (row, neighbour) contributions between guards; 18 rows and 40 / 200 sources for workgroups of four."""
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    B, N, S = 2, 9, (40 if k <= 3 else 200)
    q, src, _ = G.random_cloud(B, N, S, k, k + C)
    g = torch.Generator().manual_seed(C)
    feat, g_out = torch.randn(B, S, C, generator=g), torch.randn(B, N, C, generator=g)
    dist64, idx = R.topk_select(((q.double().unsqueeze(2) - src.double().unsqueeze(1)) ** 2).sum(-1), k)
    t = {n: gin(v, 1) for n, v in dict(dist=dist64.float(), idx=idx, feat=feat, g_out=g_out, xyz1=q, xyz2=src).items()}
    outs = [guarded(n, F32, 1) for n in (B * N * 3, B * S * 3, B * N * k * 3)]
    g1, g2, contrib = (o[0] for o in outs)
    assert lib.upp_interp_geo_bwd(p(t["dist"]), p(t["idx"]), k, p(t["feat"]), p(t["g_out"]), C, 0, p(t["xyz1"]), p(t["xyz2"]), B, N, S, C, k, EPS,
                                  p(g1), p(g2), p(contrib), st) == 0
    torch.cuda.synchronize()
    for _, check in outs:
        check()
    w1, w2 = ops.interp_geo_bwd(t["dist"], t["idx"], t["feat"], t["g_out"], t["xyz1"], t["xyz2"], k, EPS)
    assert _bits(g1.view(B, N, 3), w1) and _bits(g2.view(B, S, 3), w2) and not bool(torch.isnan(contrib).any())


def test_interp_limits():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    c = interp_case(1, 4097, 5, 4, 3, 1)
    d = _cuda(c, ("dist", "idx", "feat", "g_out"))
    out = _sentinel((1, 5, 4))
    assert lib.upp_interp_bwd(p(d["dist"]), p(d["idx"]), 3, p(d["g_out"]), 4, 0, p(out), 1, 4097, 5, 4, 3, EPS, st) == E_RANGE      # N = 4097
    o2 = _sentinel((1, 4097, 4))
    assert lib.upp_interp_fwd(p(d["dist"]), p(d["idx"]), 17, p(d["feat"]), p(o2), 4, 0, 1, 4097, 5, 4, 17, EPS, st) == E_RANGE        # k = 17
    assert lib.upp_interp_fwd(p(d["dist"]), p(d["idx"]), 3, p(d["feat"]), p(o2), 4, 1, 1, 4097, 5, 4, 3, EPS, st) == E_BADARG        # window past the row
    assert _untouched(out, o2)
    with pytest.raises(RuntimeError):
        ops.interp_bwd(d["dist"], d["idx"], d["g_out"], 5, 3, EPS)


# ============================================================================================== 5. interpolation, geometry gradients
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("C", [1, 64, 65, 300])
def test_interp_geo_backward(k, C):
    B, N, S = 2, 9, (40 if k <= 3 else 200)                   # N k < S: some sources are listed by nobody
    q, src, _ = G.random_cloud(B, N, S, k, 10 * k + C)
    g = torch.Generator().manual_seed(C + k)
    feat, g_out = torch.randn(B, S, C, generator=g), torch.randn(B, N, C, generator=g)
    true = ((q.double().unsqueeze(2) - src.double().unsqueeze(1)) ** 2).sum(-1)
    dist64, idx = R.topk_select(true, k)
    c = dict(dist=dist64.float(), idx=idx, feat=feat, g_out=g_out, xyz1=q, xyz2=src)
    t = {n: gin(v, 1) for n, v in c.items()}
    args = (t["dist"], t["idx"], t["feat"], t["g_out"], t["xyz1"], t["xyz2"], k, EPS)
    g1, g2 = ops.interp_geo_bwd(*args)
    h1, h2 = ops.interp_geo_bwd(*args)
    assert _bits(g1, h1) and _bits(g2, h2), "second run differs"
    only1, none2 = ops.interp_geo_bwd(*args, need1=True, need2=False)
    none1, only2 = ops.interp_geo_bwd(*args, need1=False, need2=True)
    assert none1 is None and none2 is None and _bits(only1, g1) and _bits(only2, g2)
    d = _cuda(c, tuple(c))
    ref = {dt: R.interp_geo(d["dist"], d["idx"], d["feat"], d["g_out"], d["xyz1"], d["xyz2"], k, EPS, dt) for dt in (F32, F64)}
    used = torch.zeros(B, S, dtype=torch.bool)
    used.scatter_(1, idx.reshape(B, -1), True)
    assert bool((~used).any()) and float(g2.cpu()[~used].abs().max()) == 0.0, "sources nobody lists"
    if k == 1:
        assert float(g1.abs().max()) == 0.0 == float(g2.abs().max()), "one neighbour: the weight is 1 whatever the geometry"
    judge("interp_geo", "k=%d C=%d" % (k, C), dict(g_xyz1=g1, g_xyz2=g2), ref[F32], ref[F64], ("g_xyz1", "g_xyz2"))


# ============================================================================================== 6. group max
@pytest.mark.parametrize("k", [1, 2, 9, 10, 255])
@pytest.mark.parametrize("C", [4, 12, 384])
def test_group_max(k, C):
    """k around the 8 rows the loop takes per trip; R C / 4 is no multiple of 256.  A selection: every output equals the selected input
    bit for bit.  Ties go to the first row (a +0 / -0 pair included: the first one's bits), an all -inf column gives row 0, the first
    NaN wins as in torch.max(dim)."""
    Rr = 7
    x, g = G.group_inputs(Rr, k, C, k + C)
    if k >= 2:
        x[0, :, 0] = x[0, :, 0].max() + 1.0                   # every row ties
        x[1, 0, 1], x[1, 1, 1] = 0.0, -0.0
        x[1, 2:, 1] = -1.0
        x[2, 0, 2], x[2, 1, 2] = -0.0, 0.0
        x[2, 2:, 2] = -1.0
        x[3, :, 3] = -float("inf")
        x[4, k - 1, 0] = float("nan")
        x[5, k // 2, 1], x[5, k - 1, 1] = float("nan"), float("nan")
    xg, gg = gin(x, 0), gin(g, 0)
    out, amax = ops.group_max_fwd(xg)
    g_x = ops.group_max_bwd(gg, amax, k)
    want = R.group_max_select(x.cuda())
    assert torch.equal(amax.long(), want)
    if k >= 2:
        assert amax[0, 0] == 0 and amax[1, 1] == 0 and amax[2, 2] == 0 and amax[3, 3] == 0 and amax[4, 0] == k - 1 and amax[5, 1] == k // 2
        assert torch.equal(amax.cpu().long(), x.max(1).indices), "as torch.max(dim)"
    ref = R.group_max(x.cuda(), want, F32, g.cuda())
    assert _bits(out, ref["out"]) and _bits(g_x, ref["g_x"])
    out2, amax2 = ops.group_max_fwd(xg)
    assert _bits(out, out2) and torch.equal(amax, amax2)


def test_group_max_c_entry_points_with_guarded_outputs_and_limits():
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    Rr, k, C = 7, 9, 12
    x, g = G.group_inputs(Rr, k, C, 3)
    xg, gg = gin(x, 0), gin(g, 0)
    (out, ck1), (amax, ck2), (g_x, ck3) = guarded(Rr * C, F32, 0), guarded(Rr * C, torch.uint8, 0), guarded(Rr * k * C, F32, 0)
    assert lib.upp_group_max_fwd(p(xg), Rr, k, C, p(out), p(amax), st) == 0
    assert lib.upp_group_max_bwd(p(gg), p(amax), Rr, k, C, p(g_x), st) == 0
    torch.cuda.synchronize()
    ck1(); ck2(); ck3()
    w_out, w_amax = ops.group_max_fwd(xg)
    assert _bits(out.view(Rr, C), w_out) and torch.equal(amax.view(Rr, C), w_amax) and _bits(g_x.view(Rr, k, C), ops.group_max_bwd(gg, w_amax, k))
    o, am, gx = _sentinel((Rr, C)), torch.full((Rr, C), 0xA5, dtype=torch.uint8, device="cuda"), _sentinel((Rr, 256, C))
    x1 = gin(x, 1)                                             # one float off the 16-byte alignment the float4 loads need
    for status, args in ((E_RANGE, (p(x1), Rr, k, C, p(o), p(am))), (E_RANGE, (p(xg), Rr, 256, C, p(o), p(am))),
                         (E_RANGE, (p(xg), Rr, k, 6, p(o), p(am)))):
        assert lib.upp_group_max_fwd(*args, st) == status
    assert lib.upp_group_max_bwd(p(gg), p(am), Rr, 256, C, p(gx), st) == E_RANGE
    assert lib.upp_group_max_bwd(p(gin(g, 1)), p(am), Rr, k, C, p(gx), st) == E_RANGE
    assert _untouched(o, gx) and bool((am == 0xA5).all())


# ============================================================================================== 7. positional encoding
@pytest.mark.parametrize("F", [0, 1, 8])
def test_posenc(F):
    """rows 3 = 87 and 771 elements (no multiple of 256), into a buffer of its own and into a window at col0 = 2 of a wider one."""
    freqs = [float(2 ** q) * 3.14159 for q in range(F)]
    width = 3 * (2 * F + 1)
    for rows in (29, 257):
        x = torch.randn(rows, 3, generator=torch.Generator().manual_seed(rows + F))
        xg = gin(x, 1)
        ref = {dt: dict(out=R.posenc(x.cuda(), freqs, dt)) for dt in (F32, F64)}
        got = ops.posenc_fwd(xg, freqs)
        assert got.shape == (rows, width) and _bits(got, ops.posenc_fwd(xg, freqs))
        assert _bits(got[:, :3], xg)
        judge("posenc", "F=%d rows=%d" % (F, rows), dict(out=got), ref[F32], ref[F64], ("out",))
        buf, check = guarded(rows * (width + 5), F32, 1)
        buf.fill_(7.0)
        out = ops.posenc_fwd(xg, freqs, out=buf.view(rows, width + 5), col0=2)
        check()
        assert _bits(out[:, 2:2 + width].contiguous(), got) and bool((out[:, :2] == 7.0).all()) and bool((out[:, 2 + width:] == 7.0).all())


def test_posenc_limits():
    import ctypes
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    x, out = torch.zeros(4, 3, device="cuda"), _sentinel((4, 57))
    arr = (ctypes.c_float * 9)(*[1.0] * 9)
    assert lib.upp_posenc_fwd(p(x), arr, 9, p(out), 57, 0, 4, st) == E_RANGE
    assert lib.upp_posenc_fwd(p(x), arr, 8, p(out), 50, 0, 4, st) == E_BADARG            # a row narrower than the embedding
    assert _untouched(out)
    with pytest.raises(RuntimeError):
        ops.posenc_fwd(x, [1.0] * 9)


# ============================================================================================== 8. the wrappers
@pytest.mark.parametrize("name", ["bn_rows_fwd", "interp_fwd", "group_max_bwd"])
def test_wrappers_refuse_wrong_tensors(name):
    """bn_rows_fwd did not check gamma, beta or the running statistics, interp_fwd not that a caller's `out` is (B, N, >= col0 + C),
    group_max_bwd not amax: device, dtype, contiguity and shape, from metadata alone."""
    if name == "bn_rows_fwd":
        c = _cuda(G.bn_inputs(6, 12, 1), ("z", "gamma", "beta", "rm", "rv"))
        fn = lambda t: ops.bn_rows_fwd(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"], 0.1, 1e-5, True, True)      # noqa: E731
        tensors = dict(x=c["z"], gamma=c["gamma"], beta=c["beta"], rm=c["rm"], rv=c["rv"])
    elif name == "interp_fwd":
        c = _cuda(interp_case(2, 7, 9, 12, 3, 1), ("dist", "idx", "feat"))
        fn = lambda t: ops.interp_fwd(c["dist"], c["idx"], c["feat"], 3, EPS, out=t["out"], col0=2)                  # noqa: E731
        tensors = dict(out=torch.zeros(2, 7, 14, device="cuda"))
        with pytest.raises(RuntimeError):
            ops.interp_fwd(c["dist"], c["idx"], c["feat"], 3, EPS, out=torch.zeros(2, 7, 13, device="cuda"), col0=2)   # one column short
        with pytest.raises(RuntimeError):
            ops.interp_fwd(c["dist"], c["idx"], c["feat"], 3, EPS, out=torch.zeros(2, 7, 14, device="cuda"), col0=-1)
    else:
        x, g = G.group_inputs(7, 3, 12, 1)
        out, amax = ops.group_max_fwd(x.cuda())
        fn = lambda t: ops.group_max_bwd(t["g"], t["amax"], 3)                                                       # noqa: E731
        tensors = dict(g=g.cuda(), amax=amax)
    refuse_wrong_tensors(name, fn, tensors)
