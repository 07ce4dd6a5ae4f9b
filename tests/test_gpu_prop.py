"""The prompt-propagation kernels of csrc/prop.hip (and bn_finalize_rows_kernel of csrc/pointwise.hip) against the float64 list-level
reference of tests/_prop_reference.py, at the edges of their parameter space: column widths around the 64-lane slots and the 4-slot
break, partial last workgroups, BatchNorm's second sweep, hit-buffer chunking, every CSR row shape, the global-memory CSR builder, the
index builder's lane masks / ties / d <= 0 image, the weight gradients, and the limits that return a status.

The bound, for every output and every case (tests/test_gpu_block.py, test_fused_propagation_gradients_reach_the_centres):
    err(x) = max|x - f64| / max|f64|,      err(kernel) <= max(2 * err(f32), 2e-6)
where f32 is the SAME formulation run by torch in float32 on the GPU with the kernel's arg-max.  Exact checks (arg-max, integer data,
guards, determinism, neighbour order on lattice clouds, row maps) are bit equalities.

Measured on MI355X: (kernel, f32) of the case nearest its bound, per family and form (number of cases); `stats` is the worst of mean, rstd
and the two running statistics.  (The f32 column moves by a few 1e-7 from run to run: torch's
index backward adds atomically.)  180 tests, 6 s.
    family / form            out             pooled          stats           g_X             g_gamma         g_beta          g_w8
    columns fused (30)       1.1e-7, 1.2e-7  9.9e-8, 9.9e-8  2.4e-7, 6.0e-8  5.3e-7, 3.5e-7  5.4e-7, 5.7e-7  1.2e-7, 1.2e-7  2.8e-7, 2.0e-7
    columns unfused (30)     1.7e-7, 8.6e-8  9.9e-8, 9.9e-8  1.1e-7, 8.4e-8  1.2e-6, 3.8e-7  1.2e-6, 5.7e-7  1.3e-7, 1.2e-7  2.5e-7, 1.8e-7
    shapes fused (63)        1.4e-7, 9.8e-8  1.1e-7, 1.1e-7  2.6e-7, 1.4e-7  5.0e-7, 4.6e-7  1.2e-6, 9.3e-7  2.5e-7, 1.3e-7  1.7e-6, 2.0e-7
    shapes unfused (18)      1.2e-7, 7.9e-8  1.1e-7, 1.1e-7  1.1e-7, 7.9e-8  1.5e-7, 1.4e-7  5.8e-7, 2.7e-7  1.2e-7, 9.1e-8  2.5e-7, 1.8e-7
    lists fused (14)         1.0e-7, 8.6e-8  1.0e-7, 9.0e-8  1.5e-7, 1.1e-7  8.5e-7, 3.8e-7  5.5e-7, 2.2e-7  4.1e-7, 3.3e-7  2.0e-7, 2.4e-7
    lists unfused (14)       1.1e-7, 8.6e-8  1.0e-7, 9.0e-8  1.5e-7, 1.2e-7  1.9e-6, 1.4e-6  6.5e-7, 3.0e-7  4.7e-7, 3.3e-7  2.9e-7, 2.2e-7
    guards fused (3)         7.4e-8, 7.9e-8  8.3e-8, 2.5e-8  1.1e-7, 1.1e-7  1.7e-7, 4.7e-8  8.9e-7, 2.6e-7  1.1e-7, 1.2e-7  1.4e-7, 2.2e-7
    offset fused             7.4e-6, 1.1e-5  8.8e-8, 6.9e-8  5.1e-3, 4.6e-3  4.9e-3, 5.8e-3  1.2e-2, 1.1e-2  1.1e-7, 9.2e-8  4.5e-5, 4.7e-5
    offset unfused           1.3e-5, 1.1e-5  8.8e-8, 6.9e-8  2.4e-7, 1.4e-7  6.9e-3, 5.8e-3  1.2e-2, 1.1e-2  9.0e-8, 9.2e-8  5.1e-5, 4.7e-5
    constant column fused    7.6e-8, 6.7e-8  6.3e-8, 5.2e-8  8.2e-8, 8.2e-8  2.3e-7, 1.4e-7  1.6e-7, 1.7e-7  1.1e-7, 8.9e-8  2.1e-7, 1.7e-7
    constant column unfused  6.4e-8, 6.7e-8  6.3e-8, 5.2e-8  1.1e-7, 8.2e-8  1.6e-7, 1.4e-7  3.1e-7, 1.7e-7  9.0e-8, 8.9e-8  1.8e-7, 1.7e-7
    identical group fused    6.6e-8, 9.6e-8  6.3e-8, 5.2e-8  8.5e-8, 8.5e-8  1.3e-7, 1.4e-7  2.1e-7, 2.7e-7  1.1e-7, 9.9e-8  1.4e-7, 1.5e-7
    identical group unfused  7.1e-8, 9.6e-8  6.3e-8, 5.2e-8  1.1e-7, 6.2e-8  1.3e-7, 1.4e-7  2.9e-7, 2.7e-7  9.0e-8, 9.9e-8  1.7e-7, 1.5e-7
    NaN, finite part fused   1.3e-7, 1.1e-7  6.1e-8, 5.6e-8  8.0e-8, 8.0e-8  1.7e-7, 1.1e-7  9.7e-8, 9.8e-8  9.5e-8, 1.1e-7  1.2e-7, 1.1e-7
    NaN, finite part unfused 1.1e-7, 1.1e-7  6.1e-8, 5.6e-8  0, 0            9.3e-8, 1.1e-7  9.7e-8, 9.8e-8  9.0e-8, 1.1e-7  1.6e-7, 1.1e-7
    T = 960, D = 1 fused     4.4e-8, 4.4e-8  4.7e-8, 4.7e-8  4.5e-8, 4.5e-8  4.7e-7, 1.3e-7  6.5e-7, 2.3e-7  9.6e-8, 9.6e-8  1.3e-7, 1.3e-7
    T = 960, D = 1 unfused   5.2e-8, 4.4e-8  4.7e-8, 4.7e-8  1.1e-7, 2.4e-8  3.1e-7, 2.0e-7  1.3e-6, 2.3e-7  1.6e-7, 9.6e-8  1.9e-7, 1.3e-7
    prop_pool_bwd, 1920 groups, D = 1: pooled 4.9e-8, 5.1e-8; g_X 7.4e-7, 1.1e-7
    prop_weights_bwd (g_c1 | g_c2): lattice 2.5e-7, 4.9e-7 | 4.2e-7, 2.0e-7; ball 2.1e-7, 2.5e-6 | 6.9e-7, 3.3e-6.  (T = 1: every level-2 centre IS the token,
    the gradient is 0 and the kernel returns an exact 0; float64 autograd leaves 1e-13 of cancellation noise there, f32 autograd 1e-5.)
The offset case is BatchNorm's variance by cancellation (tokens 1e3 +- 1e-2): both float32 evaluations lose three digits in pooled - mean, the
kernel's f64 combination of the partials does not help once `pooled` itself is rounded to f32.

Three cases missed the bound on the kernels as they were, and were fixed in csrc/prop.hip; these cases are their regression tests:
  * NaN in eval mode: prop_x_csr_kernel computed gamma * rstd * (g_c2 - 0 - xhat * 0) also in eval mode, so a NaN xhat reached g_X in column D - 1 of every
    row a NaN group lists, where the reference (and the unfused pair) has finite gradients.  Eval now takes gamma * rstd * g_c2.
  * hot320, D = 384, fused g_X: 2.55e-6 against 1.23e-6 of f32 (bound 2.47e-6).  The row's 320 terms went one by one into one accumulator.  Rows of more
    than 64 entries are now summed in chunks of 64 (one addition per chunk into the large sum); shorter rows -- every row of the models -- keep
    their order and their bits.  Now 4.5e-7 in that case, 8.5e-7 or less in every list case.
  * prop_weights_bwd on ball clouds, g_c1: 2.26e-5 against 8.2e-6 (T = 65, G2 = 33; 4.4e-5 against 2.35e-5 at T = 64).  The kernel recomputed d in the
    forward's three-term form with a FUSED dot product and unfused norms: for a coincident pair (every level-2 centre is a level-1 centre) that is
    rounding noise of ~1e-7 = 1e-4 of eps where torch's unfused f32 form cancels to an exact 0.  The backward now takes d from the differences it
    already holds: 2.1e-7 (g_c1), 6.9e-7 (g_c2) on the same clouds.
(prop_index_kernel's forward weights keep the three-term form -- it decides the neighbour ORDER, which must be the reference's; this file checks the
weights to 1e-6 only where that form is exact.)

Mutants (each built from a scratch copy, run once against this file and against the propagation tests of tests/test_gpu_block.py -- csr_build,
fused_propagation x 2, prop_index: 20 cases):
  1. collect_hits callers stop after the first pass: fails list_hazards[hot255 | hot256 | hot257 | hot320 | centre] x D (10), integer_data[hot257],
     pool_bwd_serves_1920_groups, interp_bwd_limits (T = 960); old tests: 20 pass.
  2. nw fixed at 4 in prop_pool_stats_kernel: fails the 30 training cases of shapes with groups % 4 != 0 ((1, 1, 1), (3, 9, 5), (1, 16, 9), (2, 40, 33),
     (18, 8, 57); eval takes the running statistics) and the three guard cases; old tests: 20 pass.
  3. second-sweep reload of bn_finalize_rows_kernel skipped: fails the 12 training cases of shapes with groups > 1024 ((17, 16, 64), (18, 8, 57));
     old tests: 20 pass.
  4. f1 always 0.3 in prop_x_csr_kernel: fails 115 cases here -- and 9 of the old tests: a one-entry row then counts its entry twice, which every
     test sees.  The variant that is wrong only behind the first pair (rows of 3 and more entries) fails 51 cases here (every shapes case with
     duplicates in i2, list_hazards[rows] and the other list cases) and none of the old 20.
  5. insertion sort of csr_build_kernel<false> skipped: fails csr_build[20000-2400] and [32768-2048-(1024, 64)], not the LDS case; old tests: 20 pass.
  6. prop_index_kernel takes the highest tied lane: fails all 28 lattice cases; old tests: 20 pass.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _prop_reference as R
from test_gpu_step_tail import guarded
from upp_hip import _abi, ops
from upp_hip import functional as HF

pytestmark = pytest.mark.gpu

KEEP, MOM, EPS = 0.9, 0.1, 1e-5
MODES = ("train_u", "train", "eval")
FUSED_KEYS = ("out", "pooled", "mean", "rstd", "running_mean", "running_var", "g_X", "g_gamma", "g_beta", "g_w8")
UNFUSED_KEYS = ("out", "pooled", "running_mean", "running_var", "g_X", "g_gamma", "g_beta", "g_w8")


def _bits(a, b):
    """Bit equality (NaN payloads included) of two tensors of one dtype."""
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- cases
def make_case(B, lead, T, G2, D, mode, seed):
    """Random lists within each sample (any row of the sample for i1 / i2 -- duplicates in i2 included --, any level-2 centre for idx8:
    the kernels take lists, the model's constraints are not theirs).  CPU tensors; finish() moves them to the device."""
    g = torch.Generator().manual_seed(seed)
    Lp = lead + T
    c = types.SimpleNamespace(B=B, lead=lead, T=T, G2=G2, D=D, Lp=Lp, mode=mode, rows=B * Lp, groups=B * G2, training=mode != "eval",
                              keep=KEEP if mode == "train_u" else 1.0, gen=g)
    c.X = torch.randn(B, Lp, D, generator=g) * 0.7 + 0.3
    base = (torch.arange(B) * Lp).view(B, 1)
    c.i1 = (base + torch.randint(0, Lp, (B, G2 * 8), generator=g)).reshape(-1).int()
    c.i2 = (base + torch.randint(0, Lp, (B, G2), generator=g)).reshape(-1).int()
    c.idx8 = torch.randint(0, G2, (B, T, 8), generator=g).int()
    w8 = torch.rand(B, T, 8, generator=g) + 0.05
    c.w8 = w8 / w8.sum(-1, keepdim=True)
    c.u = torch.rand(B * G2, generator=g) if mode == "train_u" else None
    c.wgt = torch.randn(B, Lp, D, generator=g)
    c.gamma, c.beta = torch.linspace(0.5, 1.5, D), torch.linspace(-0.2, 0.2, D)
    c.rm, c.rv = torch.linspace(-0.1, 0.4, D), torch.linspace(0.6, 1.7, D)
    return c


def finish(c):
    for k in ("X", "i1", "i2", "idx8", "w8", "u", "wgt", "gamma", "beta", "rm", "rv"):
        v = getattr(c, k)
        setattr(c, k, None if v is None else v.contiguous().cuda())
    assert int(c.i1.min()) >= 0 and int(c.i1.max()) < c.rows and int(c.i2.min()) >= 0 and int(c.i2.max()) < c.rows      # never a row outside X
    assert int(c.idx8.min()) >= 0 and int(c.idx8.max()) < c.G2
    un = None if c.u is None else c.u.cpu().numpy()
    c.amax = torch.from_numpy(R.amax_emulate(c.X.cpu().numpy(), c.i1.cpu().numpy(), un, c.keep)).cuda()
    c.ref = {}
    return c


def _bn(c):
    bn = torch.nn.BatchNorm1d(c.D, eps=EPS, momentum=MOM).cuda()
    with torch.no_grad():
        bn.weight.copy_(c.gamma); bn.bias.copy_(c.beta); bn.running_mean.copy_(c.rm); bn.running_var.copy_(c.rv)
    return bn


def reference(c, dtype):
    if dtype not in c.ref:
        c.ref[dtype] = R.step_with_grads(c.X, c.i1, c.i2, c.idx8, c.w8, c.u, c.keep, c.gamma, c.beta, c.rm, c.rv, MOM, EPS, c.training,
                                         c.amax, c.wgt, dtype)
    return c.ref[dtype]


def run_fused(c):
    """HF.propagate (prop_fwd / prop_bwd / prop_w8_grad) twice -- the second run must be bit-identical -- plus the saved statistics."""
    index = HF.PropIndex(c.i1, c.i2, c.idx8, c.w8, c.rows)

    def once():
        bn = _bn(c)
        xi, w = c.X.clone().requires_grad_(True), c.w8.clone().requires_grad_(True)
        out = HF.propagate(xi, bn, index, c.u, c.keep, c.training, w8=w)
        gx, gg, gb, gw = torch.autograd.grad((out * c.wgt).sum(), [xi, bn.weight, bn.bias, w])
        return dict(out=out.detach(), g_X=gx, g_gamma=gg, g_beta=gb, g_w8=gw, running_mean=bn.running_mean.detach().clone(),
                    running_var=bn.running_var.detach().clone())

    a, b = once(), once()
    for k in a:
        assert _bits(a[k], b[k]), "second fused run differs in " + k
    rm, rv = c.rm.clone(), c.rv.clone()
    out, pooled, amax, mean, rstd = ops.prop_fwd(c.X, c.i1, c.u, c.keep, c.i2, c.idx8, c.w8, c.gamma, c.beta, rm, rv, MOM, EPS, c.training,
                                                 c.B, c.Lp, c.T, c.G2)
    assert _bits(out, a["out"]) and _bits(rm, a["running_mean"]) and _bits(rv, a["running_var"])
    a.update(pooled=pooled, amax=amax, mean=mean, rstd=rstd)
    return a


def run_unfused(c):
    """HF.prop_pool + F.batch_norm + HF.prop_interp (prop_pool_fwd/bwd, prop_interp_fwd/bwd, prop_w8_grad without statistics)."""
    bn = _bn(c)
    xi, w = c.X.clone().requires_grad_(True), c.w8.clone().requires_grad_(True)
    pooled = HF.prop_pool(xi, c.i1, c.u, c.keep)
    lc = F.batch_norm(pooled, bn.running_mean, bn.running_var, bn.weight, bn.bias, c.training, MOM, EPS)
    out = HF.prop_interp(xi, lc.view(c.B, c.G2, c.D), c.i2, c.idx8, w)
    gx, gg, gb, gw = torch.autograd.grad((out * c.wgt).sum(), [xi, bn.weight, bn.bias, w])
    _, amax = ops.prop_pool_fwd(c.X, c.i1, c.u, c.keep, c.groups)
    return dict(out=out.detach(), pooled=pooled.detach(), amax=amax, g_X=gx, g_gamma=gg, g_beta=gb, g_w8=gw,
                running_mean=bn.running_mean.detach().clone(), running_var=bn.running_var.detach().clone())


def _err(x, e):
    """max|x - e| / max|e| over the elements where e is finite (absolute where e is all zero)."""
    m = torch.isfinite(e)
    if not bool(m.any()):
        return 0.0
    scale = float(e[m].abs().max())
    d = (x.double()[m] - e[m]).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return float(d.max()) / (scale if scale > 0 else 1.0)


def judge(family, label, got, f32, f64, keys):
    """The bound for every key; every figure is printed before anything is asserted."""
    bad = []
    for k in keys:
        e = f64[k].reshape(got[k].shape)
        if not torch.equal(torch.isfinite(got[k]), torch.isfinite(e)):
            bad.append((k, "non-finite set differs from the reference's"))
            continue
        assert torch.equal(torch.isfinite(f32[k].reshape(e.shape)), torch.isfinite(e)), k       # the yardstick itself must not overflow
        ek, ef = _err(got[k], e), _err(f32[k].reshape(e.shape), e)
        print("PROPERR | %s | %s | %s | %.2e | %.2e" % (family, label, k, ek, ef))
        if not ek <= max(2.0 * ef, 2e-6):
            bad.append((k, ek, ef))
    assert not bad, (family, label, bad)


def check(c, family, label, unfused=None):
    f32, f64 = reference(c, torch.float32), reference(c, torch.float64)
    fused = run_fused(c)
    assert torch.equal(fused["amax"], c.amax), "fused arg-max differs from the emulator"
    judge(family, label + " fused", fused, f32, f64, FUSED_KEYS)
    if c.G2 % 4 == 0 if unfused is None else unfused:
        un = run_unfused(c)
        assert torch.equal(un["amax"], c.amax), "unfused arg-max differs from the emulator"
        judge(family, label + " unfused", un, f32, f64, UNFUSED_KEYS)
    return fused


# ---------------------------------------------------------------------------------------------- A. parity sweep
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [1, 63, 64, 65, 200, 256, 257, 384, 500, 512])
def test_columns(D, mode):
    """Item 1: clamped column slots, the store mask c < D, the break after the first 4-slot batch (D = 256 | 257), the cap (512).
    Both forms of prop_w8_grad (statistics given: fused; None: unfused) are judged here through g_w8."""
    check(finish(make_case(2, 3, 16, 8, D, mode, seed=D)), "columns", "D=%d %s" % (D, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("extra", [0, 1, 11])
@pytest.mark.parametrize("B,T,G2", [(1, 1, 1), (3, 9, 5), (1, 16, 9), (2, 40, 33), (2, 70, 64), (17, 16, 64), (18, 8, 57)])
def test_shapes(B, T, G2, extra, mode):
    """Items 2, 3: groups % 4 != 0 (nw < 4 in prop_pool_stats / prop_c2_csr, the short last slab of bn_finalize_rows), groups > 1024
    (bn_finalize_rows' second sweep; (18, 8, 57) is the short last slab OF the second sweep), one token, one group."""
    check(finish(make_case(B, extra, T, G2, 65, mode, seed=B * 1000 + T * 10 + extra)), "shapes",
          "B=%d T=%d G2=%d Lp=T+%d %s" % (B, T, G2, extra, mode))


# ---------------------------------------------------------------------------------------------- B. list hazards
def _hazard_case(kind, D):
    if kind == "stride":
        # the reference's flat indices with batch offsets b*64, read in the (B*74)-row view of the cls-stripped tokens
        B, T, G2, off, P = 3, 64, 32, 1, 10
        c = make_case(B, off + P, T, G2, D, "train_u", seed=77)
        i1 = torch.randint(0, T, (B, G2 * 8), generator=c.gen) + torch.arange(B).view(B, 1) * T
        i2 = torch.stack([torch.randperm(T, generator=c.gen)[:G2] for _ in range(B)]) + torch.arange(B).view(B, 1) * T
        m1, m2 = R.row_maps(i1.numpy(), i2.numpy(), False, B, G2, c.Lp, off)
        c.i1, c.i2 = torch.from_numpy(m1).int(), torch.from_numpy(m2).int()
        sample_of_row, sample_of_entry = c.i1.long() // c.Lp, torch.arange(B).repeat_interleave(G2 * 8)
        foreign = set((c.i1[sample_of_row != sample_of_entry]).tolist()) - set((c.i1[sample_of_row == sample_of_entry]).tolist())
        assert len(foreign) > 0                                  # rows referenced ONLY from another sample's lists
        return c
    B, lead, T, G2 = 2, 3, 40, 32
    c = make_case(B, lead, T, G2, D, "train_u", seed=len(kind) + D)
    if kind.startswith("hot"):
        m = int(kind[3:])
        r = c.Lp + lead + 5
        c.i1[c.i1 == r] = r - 1
        c.i1[torch.randperm(c.i1.numel(), generator=c.gen)[:m]] = r          # from the lists of both samples
        assert int((c.i1 == r).sum()) == m
    elif kind == "centre":
        c.idx8[0] = 7                                            # all 320 entries of sample 0 -> centre 7; its other centres: nobody
        c.idx8[1][c.idx8[1] == 3] = 4                            # centre 3 of sample 1: selected by no token
        assert int((c.idx8[0] == 7).sum()) == 320 and int((c.idx8[1] == 3).sum()) == 0
    elif kind == "rows":
        r2, r3 = lead + 4, c.Lp + lead + 9
        unref = [c.Lp - 1, c.Lp - 2, 2 * c.Lp - 1, lead]          # token rows that no list mentions
        for v in unref + [r2, r3]:
            c.i1[c.i1 == v] = v - 3 if v != lead else lead + 1
            c.i2[c.i2 == v] = v - 3 if v != lead else lead + 1
        c.i2[1], c.i2[6] = r2, r2                                # own token of two level-2 centres (an odd CSR row tail: f1 = 0.3)
        c.i2[G2 + 0], c.i2[G2 + 2], c.i2[G2 + 31] = r3, r3, r3   # ... of three (f1 = 0 in the second pair)
        assert int((c.i2 == r2).sum()) == 2 and int((c.i2 == r3).sum()) == 3
        assert all(int((c.i1 == v).sum()) + int((c.i2 == v).sum()) == 0 for v in unref)
    return c


@pytest.mark.parametrize("D", [65, 384])
@pytest.mark.parametrize("kind", ["hot255", "hot256", "hot257", "hot320", "centre", "rows", "stride"])
def test_list_hazards(kind, D):
    """Items 4, 5: a row with 255 | 256 | 257 | 320 entries of i1 (collect_hits' second pass; CSR rows of every residue of the unroll),
    a level-2 centre listed by every idx8 entry of its sample (320), centres nobody selects (zero g_c2 that enters the BatchNorm
    partials), own token of 2 and 3 centres, rows no list mentions, rows listed only by another sample."""
    check(finish(_hazard_case(kind, D)), "lists", "%s D=%d" % (kind, D))


# ---------------------------------------------------------------------------------------------- C. exact checks
@pytest.mark.parametrize("kind", ["small", "hot257"])
def test_integer_data_is_exact(kind):
    """Small-integer X without u (f = 2, /8 exact): pooled, and the unfused g_X of prop_pool_bwd, equal float64 bit for bit."""
    c = make_case(3, 2, 9, 5, 65, "train", seed=5) if kind == "small" else _hazard_case("hot257", 65)
    c.u, c.keep, c.mode = None, 1.0, "train"
    c.X = torch.randint(-8, 9, c.X.shape, generator=c.gen).float()
    gp = torch.randint(-4, 5, (c.groups, c.D), generator=c.gen).float().cuda()
    finish(c)
    pooled, amax = ops.prop_pool_fwd(c.X, c.i1, None, 1.0, c.groups)
    pooled_f, amax_f = ops.prop_fwd(c.X, c.i1, None, 1.0, c.i2, c.idx8, c.w8, c.gamma, c.beta, c.rm.clone(), c.rv.clone(), MOM, EPS, True,
                                    c.B, c.Lp, c.T, c.G2)[1:3]
    x64 = c.X.double().requires_grad_(True)
    want = R.pool(x64, c.i1, R.factors(None, 1.0, c.groups, torch.float64, "cuda"), c.amax)
    assert torch.equal(amax, c.amax) and torch.equal(amax_f, c.amax)
    assert torch.equal(pooled.double(), want.detach()) and _bits(pooled, pooled_f)
    g64 = torch.autograd.grad((want * gp.double()).sum(), x64)[0]
    got = ops.prop_pool_bwd(gp, amax, c.i1, None, 1.0, c.rows)
    assert torch.equal(got.double(), g64.view(c.rows, c.D))


@pytest.mark.parametrize("D", [1, 65, 500])
def test_nothing_is_written_outside_the_outputs(D):
    """Every output of the fused step (and of the unfused kernels that take G2 = 5) inside sentinel-filled buffers, groups % 4 != 0."""
    c = finish(make_case(3, 2, 9, 5, D, "train_u", seed=40 + D))
    lib, p, f32 = _abi.load(), _abi.ptr, torch.float32
    nD, gD = c.rows * D, c.groups * D
    nparts = lib.upp_prop_part_floats(c.groups, D)
    assert nparts == ((c.groups + 3) // 4) * 2 * D
    outs = dict(out=guarded(nD, f32, 1), pooled=guarded(gD, f32, 3), amax=guarded(gD, torch.uint8, 5), part=guarded(nparts, f32, 2),
                mean=guarded(D, f32, 1), rstd=guarded(D, f32, 3), g_c2=guarded(gD, f32, 1), part_b=guarded(nparts, f32, 3),
                g_gamma=guarded(D, f32, 2), g_beta=guarded(D, f32, 1), g_X=guarded(nD, f32, 3), g_w8=guarded(c.B * c.T * 8, f32, 1),
                pooled_u=guarded(gD, f32, 1), amax_u=guarded(gD, torch.uint8, 1), g_X_u=guarded(nD, f32, 2), out_u=guarded(nD, f32, 3))
    v = {k: t[0] for k, t in outs.items()}
    rm, rv = c.rm.clone(), c.rv.clone()
    st = _abi.stream()
    assert lib.upp_prop_fwd(p(c.X), p(c.i1), p(c.u), c.keep, p(c.i2), p(c.idx8), p(c.w8), p(c.gamma), p(c.beta), p(rm), p(rv), MOM, EPS, 1,
                            p(v["pooled"]), p(v["amax"]), p(v["part"]), p(v["mean"]), p(v["rstd"]), p(v["out"]), c.B, c.Lp, c.T, c.G2, D, st) == 0
    index = HF.PropIndex(c.i1, c.i2, c.idx8, c.w8, c.rows)
    g = c.wgt.contiguous()
    assert lib.upp_prop_bwd(p(g), p(v["pooled"]), p(v["amax"]), p(v["mean"]), p(v["rstd"]), p(c.gamma), p(c.u), c.keep, p(c.w8),
                            p(index.csr1[0]), p(index.csr1[1]), p(index.csr2[0]), p(index.csr2[1]), p(index.csr8[0]), p(index.csr8[1]), 1,
                            p(v["g_c2"]), p(v["part_b"]), p(v["g_gamma"]), p(v["g_beta"]), p(v["g_X"]), c.B, c.Lp, c.T, c.G2, D, st) == 0
    assert lib.upp_prop_w8_grad(p(g), p(c.X), p(v["pooled"]), p(v["mean"]), p(v["rstd"]), p(c.gamma), p(c.beta), p(c.i2), p(c.idx8),
                                p(v["g_w8"]), c.B, c.Lp, c.T, c.G2, D, st) == 0
    assert lib.upp_prop_pool_fwd(p(c.X), p(c.i1), p(c.u), c.keep, p(v["pooled_u"]), p(v["amax_u"]), c.groups, D, st) == 0
    assert lib.upp_prop_pool_bwd(p(v["g_c2"]), p(v["amax_u"]), p(c.i1), p(c.u), c.keep, p(v["g_X_u"]), c.rows, c.groups, D, st) == 0
    lc = torch.randn(c.groups, D, device="cuda")
    assert lib.upp_prop_interp_fwd(p(c.X), p(lc), p(c.i2), p(c.idx8), p(c.w8), p(v["out_u"]), c.B, c.Lp, c.T, c.G2, D, st) == 0
    torch.cuda.synchronize()
    for k, (_, chk) in outs.items():
        chk()
    for k, t in v.items():
        assert bool(torch.isfinite(t.float()).all()), k + " was not written completely"
    # and the guarded run computed what the wrappers compute
    fused = run_fused(c)
    assert _bits(v["out"], fused["out"].view(-1)) and _bits(v["pooled"], fused["pooled"].view(-1)) and torch.equal(v["amax"], c.amax.view(-1))
    assert _bits(v["g_X"], fused["g_X"].view(-1)) and _bits(v["g_w8"], fused["g_w8"].view(-1)) and _bits(v["g_gamma"], fused["g_gamma"])
    assert _bits(v["pooled_u"], v["pooled"]) and torch.equal(v["amax_u"], v["amax"])
    judge("guards", "D=%d fused" % D, fused, reference(c, torch.float32), reference(c, torch.float64), FUSED_KEYS)


# ---------------------------------------------------------------------------------------------- D. numerical hazards
@pytest.mark.parametrize("kind", ["offset", "constant_column", "identical_group"])
def test_numerical_hazards(kind):
    c = make_case(4, 3, 16, 8, 65, "train", seed=90)
    if kind == "offset":
        c.X = 1e3 + 1e-2 * torch.randn(c.X.shape, generator=c.gen)          # BatchNorm variance by cancellation
    elif kind == "constant_column":
        c.X[:, :, 5] = 1.25                                                  # variance 0, rstd = 1 / sqrt(eps)
    else:
        c.i1[8:16] = c.lead + 2                                              # group 1: eight times the same row, every k ties
    finish(c)
    fused = check(c, "numerical", kind)
    if kind == "constant_column":
        assert float(fused["rstd"][5]) == pytest.approx(EPS ** -0.5, rel=1e-6)
    if kind == "identical_group":
        assert int(fused["amax"][1].max()) == 0 and int(c.amax[1].max()) == 0


@pytest.mark.parametrize("D", [65, 500])
def test_a_nan_in_the_last_column_stays_where_the_reference_has_it(D):
    """Eval mode, NaN at X[r0, D-1]: column D-1 is the one every clamped slot loads.  The set of non-finite outputs and gradients must
    equal the reference's exactly (judge() compares the sets before the errors)."""
    c = make_case(2, 3, 16, 8, D, "eval", seed=D + 1)
    r0 = c.lead + 4
    c.i1[3], c.i1[40] = r0, r0                                               # two groups of sample 0 list the row
    c.X.view(-1, D)[r0, D - 1] = float("nan")
    finish(c)
    f64 = reference(c, torch.float64)
    assert bool(torch.isnan(f64["pooled"]).any()) and bool(torch.isfinite(f64["g_X"]).all())
    assert int(torch.isnan(f64["out"]).sum()) < c.rows and not bool(torch.isnan(f64["out"][..., :D - 1]).any())
    check(c, "nan", "D=%d" % D)


# ---------------------------------------------------------------------------------------------- E. csr_build
@pytest.mark.parametrize("n,rows,seg", [(20000, 2400, None), (32768, 2048, (1024, 64)), (18000, 64, None)])
def test_csr_build_beyond_and_at_the_lds_threshold(n, rows, seg):
    """Item 6: (rows + 1024 + 2n) * 4 > 150 KiB takes csr_build_kernel<false> (global memory, per-row insertion sort): the first two;
    the third is the LDS variant next to the threshold.  Every row's multiplicity stays <= 512 (the insertion sort is quadratic)."""
    assert ((rows + 1024 + 2 * n) * 4 > 150 * 1024) == (n != 18000)
    rng = np.random.default_rng(n + rows)
    if seg is None:
        keys = rng.integers(0, rows, n).astype(np.int32)
        if rows == 2400:
            keys[rng.permutation(n)[:300]] = 1234                       # one long row, filled by many threads in arbitrary order
        keys[rng.integers(0, n, n // 50)] = rows + 7                    # out-of-range keys are skipped
        keys[0] = -1
        absolute = keys.astype(np.int64)
        start, perm = ops.csr_build(torch.from_numpy(keys).cuda(), rows)
    else:
        seg_len, seg_rows = seg
        keys = rng.integers(0, seg_rows, n).astype(np.int32)
        absolute = (np.arange(n) // seg_len) * seg_rows + keys
        start, perm = ops.csr_build(torch.from_numpy(keys).cuda(), rows, seg_len=seg_len, seg_rows=seg_rows)
    valid = np.nonzero((absolute >= 0) & (absolute < rows))[0]
    counts = np.bincount(absolute[valid], minlength=rows)
    assert counts.max() <= 512 and (rows != 2400 or counts[1234] >= 300)
    order = valid[np.argsort(absolute[valid], kind="stable")]
    assert np.array_equal(start.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
    assert np.array_equal(perm.cpu().numpy()[:len(order)], order)


# ---------------------------------------------------------------------------------------------- F. prop_index
INDEX_SHAPES = [(2, 16, 8), (3, 17, 9), (2, 66, 33), (1, 1, 8), (2, 126, 63), (2, 128, 64), (2, 4, 64)]
EPS_W = float(np.float32(1e-3))


def _index_lists(B, T, G2, gather, rng):
    if gather:
        return rng.integers(0, T, (B, G2 * 8)), rng.integers(0, T, (B, G2))
    return rng.integers(0, T, (B, G2 * 8)) + np.arange(B)[:, None] * T, rng.integers(0, T, (B, G2)) + np.arange(B)[:, None] * T


def _run_index(c1, c2, i1, i2, gather, Lp, off):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()          # noqa: E731
    got = ops.prop_index(t(c1, torch.float32), t(c2, torch.float32), t(i1.reshape(-1), torch.int64), t(i2.reshape(-1), torch.int64),
                         gather, Lp, off, 1e-3)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


def _weights64(c1, c2, idx8):
    d = np.take_along_axis(R.distances64(c1, c2), idx8.astype(np.int64), axis=-1)
    rc = 1.0 / (d + EPS_W)
    return rc / rc.sum(-1, keepdims=True)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("B,T,G2", INDEX_SHAPES)
def test_prop_index_on_lattice_clouds_is_exact(B, T, G2, gather, off):
    """Item 7: coordinates k / 4, |k| <= 4 -- the kernel's three-term distance is exact in f32, so the neighbour order (d, index) has no
    tolerance: exact ties (lowest index wins), d = 0 (level-2 centres are drawn from the level-1 ones, duplicates included), lane masks
    for G2 = 8 | 9 | 33 | 63 | 64, T = 1, T % 4 != 0, and (2, 4, 64) where the integer part needs more waves than there are tokens."""
    rng = np.random.default_rng(B * 100 + T + G2 + 7 * gather + off)
    Lp = off + 10 + T
    c1 = R.lattice((B, T, 3), rng)
    pick = rng.integers(0, T, (B, G2))
    c2 = np.take_along_axis(c1, pick[:, :, None].repeat(3, -1), axis=1)
    i1, i2 = _index_lists(B, T, G2, gather, rng)
    i1a, i2a, idx8, w8 = _run_index(c1, c2, i1, i2, gather, Lp, off)
    m1, m2 = R.row_maps(i1, i2, gather, B, G2, Lp, off)
    assert m1.max() < B * Lp and np.array_equal(i1a, m1) and np.array_equal(i2a, m2)
    want = R.neighbour_order(c1, c2)
    assert np.array_equal(idx8, want)
    d8 = np.take_along_axis(R.distances64(c1, c2), want, axis=-1)
    assert (d8[..., 0] == 0).any()                                 # coincident centres: d = 0 for every token that was picked
    assert (d8[..., 1:] == d8[..., :-1]).any()                     # and exact ties occur
    w64 = _weights64(c1, c2, want)
    assert np.all(np.abs(w8 - w64) <= 1e-6 * w64)


@pytest.mark.parametrize("shift", [0.0, 8.0])
@pytest.mark.parametrize("B,T,G2", INDEX_SHAPES)
def test_prop_index_on_ball_clouds(B, T, G2, shift):
    """Unit-ball clouds (and the same shifted by (8, 8, 8): the rounding of |a|^2 + |b|^2 - 2 a.b grows with the norms, the margin with it),
    level-2 centres a subset of the level-1 ones (d = 0 up to rounding, of either sign, for every picked token).  Nothing is left out."""
    rng = np.random.default_rng(B * 100 + T + G2 + int(shift))
    v = rng.standard_normal((B, T, 3))
    c1 = (v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.random((B, T, 1)) ** (1 / 3) + shift).astype(np.float32)
    pick = np.stack([rng.permutation(T)[:G2] if G2 <= T else rng.integers(0, T, G2) for _ in range(B)])
    c2 = np.take_along_axis(c1, pick[:, :, None].repeat(3, -1), axis=1)
    i1, i2 = _index_lists(B, T, G2, True, rng)
    Lp = 11 + T
    _, _, idx8, w8 = _run_index(c1, c2, i1, i2, True, Lp, 1)
    assert idx8.min() >= 0 and idx8.max() < G2
    s = np.sort(idx8, axis=-1)
    assert (s[..., 1:] != s[..., :-1]).all()
    d = R.distances64(c1, c2)
    kth = np.sort(d, axis=-1)[..., 7:8]
    na, nb = (c1.astype(np.float64) ** 2).sum(-1)[:, :, None], (c2.astype(np.float64) ** 2).sum(-1)[:, None, :]
    margin = 16 * 2.0 ** -24 * np.take_along_axis(na + nb, idx8.astype(np.int64), axis=-1)
    assert (np.take_along_axis(d, idx8.astype(np.int64), axis=-1) <= kth + margin).all()
    assert np.all(np.abs(w8.astype(np.float64).sum(-1) - 1.0) <= 1e-6) and (w8 >= 0).all()


# ---------------------------------------------------------------------------------------------- G. weight gradients
@pytest.mark.parametrize("cloud", ["lattice", "ball"])
@pytest.mark.parametrize("T,G2", [(1, 8), (16, 8), (65, 33), (130, 70), (64, 32), (1024, 9)])
def test_prop_weights_bwd_against_autograd(T, G2, cloud):
    """Item 8: the `+= 64` loops (T > 64, G2 > 64), T = 1, the LDS limit T = 1024, coincident centres (d = 0), a centre nobody selects."""
    B = 2
    rng = np.random.default_rng(T + G2)
    if cloud == "lattice":
        c1 = R.lattice((B, T, 3), rng)
    else:
        v = rng.standard_normal((B, T, 3))
        c1 = (v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.random((B, T, 1)) ** (1 / 3)).astype(np.float32)
    c2 = np.take_along_axis(c1, rng.integers(0, T, (B, G2))[:, :, None].repeat(3, -1), axis=1).copy()
    if G2 > 8:
        c2[:, G2 - 1] = 5.0                                         # far from every token: selected by nobody
    idx8 = R.neighbour_order(c1, c2)
    assert G2 == 8 or not (idx8 == G2 - 1).any()
    gw = rng.standard_normal((B, T, 8)).astype(np.float32)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                     # noqa: E731
    a, b, j, g = tc(c1), tc(c2), tc(idx8.astype(np.int32)), tc(gw)
    g1, g2 = ops.prop_weights_bwd(a, b, j, g, 1e-3)

    def auto(dtype):
        x, y = a.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
        gx, gy = torch.autograd.grad((R.weights(x, y, j, EPS_W) * g.to(dtype)).sum(), [x, y])
        return dict(g_c1=gx.double(), g_c2=gy.double())

    if G2 > 8:
        assert float(g2[:, G2 - 1].abs().max()) == 0.0             # an exact zero
    judge("weights_bwd", "T=%d G2=%d %s" % (T, G2, cloud), dict(g_c1=g1, g_c2=g2), auto(torch.float32), auto(torch.float64), ("g_c1", "g_c2"))


# ---------------------------------------------------------------------------------------------- H. limits
def _sentinel(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda") if dtype.is_floating_point else torch.full(shape, 0xA5, dtype=dtype, device="cuda")


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == 0xA5).all()) for t in ts)


def _refused(name, outs, *args):
    """The raw entry point returns a status (bad argument -1 or range -2) and launches nothing: no output element changes."""
    rc = getattr(_abi.load(), name)(*args, _abi.stream())
    assert rc in (-1, -2), (name, rc)
    assert _untouched(*outs), name + " wrote although it refused"
    return rc


def test_pool_bwd_serves_1920_groups_and_refuses_1921():
    """Item 9: the index list of prop_pool_bwd must fit LDS.  Block._propagate_fused takes the unfused pair under SyncBN, so this is a
    training limit (limits)."""
    rows, D, p = 50, 1, _abi.ptr
    g = torch.Generator().manual_seed(1920)
    for groups in (1920, 1921):
        X = (torch.randn(rows, D, generator=g)).cuda()
        i1 = torch.randint(0, rows, (groups * 8,), generator=g).int().cuda()
        gp = torch.randn(groups, D, generator=g).cuda()
        pooled, amax = ops.prop_pool_fwd(X, i1, None, 1.0, groups)
        if groups == 1921:
            with pytest.raises(RuntimeError):
                ops.prop_pool_bwd(gp, amax, i1, None, 1.0, rows)
            out = _sentinel((rows, D))
            assert _refused("upp_prop_pool_bwd", [out], p(gp), p(amax), p(i1), None, 1.0, p(out), rows, groups, D) == -2
            continue
        got = ops.prop_pool_bwd(gp, amax, i1, None, 1.0, rows)       # ~307 entries per row: two passes of the hit buffer as well
        em = torch.from_numpy(R.amax_emulate(X.cpu().numpy(), i1.cpu().numpy(), None, 1.0)).cuda()
        assert torch.equal(amax, em)

        def auto(dtype):
            x = X.to(dtype).requires_grad_(True)
            y = R.pool(x, i1, R.factors(None, 1.0, groups, dtype, "cuda"), em)
            return dict(pooled=y.detach().double(), g_X=torch.autograd.grad((y * gp.to(dtype)).sum(), x)[0].double())

        judge("limits", "pool_bwd groups=1920 D=1", dict(pooled=pooled, g_X=got), auto(torch.float32), auto(torch.float64), ("pooled", "g_X"))


def test_interp_bwd_limits():
    """G2 % 4 != 0 and T > 960 (idx8 / w8 of one sample must fit LDS) are refused; T = 960 runs and matches float64."""
    check(finish(make_case(1, 2, 960, 8, 1, "train", seed=960)), "limits", "interp_bwd T=960 D=1", unfused=True)
    p = _abi.ptr
    for B, T, G2 in ((2, 16, 6), (1, 961, 8)):
        c = finish(make_case(B, 2, T, G2, 4, "train", seed=T))
        with pytest.raises(RuntimeError):
            ops.prop_interp_bwd(c.wgt, c.i2, c.idx8, c.w8, c.B, c.Lp, c.T, c.G2)
        g_c2, g_X = _sentinel((c.groups, c.D)), _sentinel((c.rows, c.D))
        assert _refused("upp_prop_interp_bwd", [g_c2, g_X], p(c.wgt), p(c.i2), p(c.idx8), p(c.w8), p(g_c2), p(g_X), c.B, c.Lp, c.T, c.G2, c.D) == -2


def test_513_columns_are_refused_by_every_entry_point():
    c = finish(make_case(2, 3, 16, 8, 513, "train_u", seed=513))
    D, p = 513, _abi.ptr
    index = HF.PropIndex(c.i1, c.i2, c.idx8, c.w8, c.rows)
    pooled, lc = torch.randn(c.groups, D, device="cuda"), torch.randn(c.groups, D, device="cuda")
    amax = torch.zeros(c.groups, D, dtype=torch.uint8, device="cuda")
    stat = torch.ones(D, device="cuda")
    calls = [lambda: ops.prop_pool_fwd(c.X, c.i1, c.u, c.keep, c.groups),
             lambda: ops.prop_pool_bwd(pooled, amax, c.i1, c.u, c.keep, c.rows),
             lambda: ops.prop_interp_fwd(c.X, lc, c.i2, c.idx8, c.w8, c.B, c.Lp, c.T, c.G2),
             lambda: ops.prop_interp_bwd(c.wgt, c.i2, c.idx8, c.w8, c.B, c.Lp, c.T, c.G2),
             lambda: ops.prop_fwd(c.X, c.i1, c.u, c.keep, c.i2, c.idx8, c.w8, c.gamma, c.beta, c.rm, c.rv, MOM, EPS, True, c.B, c.Lp, c.T, c.G2),
             lambda: ops.prop_bwd(c.wgt, pooled, amax, stat, stat, c.gamma, c.u, c.keep, c.w8, index.csr1, index.csr2, index.csr8, True, c.B,
                                  c.Lp, c.T, c.G2),
             lambda: ops.prop_w8_grad(c.wgt, c.X, pooled, (stat, stat, c.gamma, c.beta), c.i2, c.idx8, c.B, c.Lp, c.T, c.G2),
             lambda: ops.prop_w8_grad(c.wgt, c.X, lc, None, c.i2, c.idx8, c.B, c.Lp, c.T, c.G2)]
    for f in calls:
        with pytest.raises(RuntimeError):
            f()
    rm, rv = c.rm.clone(), c.rv.clone()
    s = {k: _sentinel(shape) for k, shape in dict(pooled=(c.groups, D), part=(c.groups * D,), mean=(D,), rstd=(D,), out=(c.rows, D), g_c2=(c.groups, D),
                                                  g_gamma=(D,), g_beta=(D,), g_X=(c.rows, D), g_w8=(c.B, c.T, 8)).items()}
    am = _sentinel((c.groups, D), torch.uint8)
    assert _refused("upp_prop_pool_fwd", [s["pooled"], am], p(c.X), p(c.i1), p(c.u), c.keep, p(s["pooled"]), p(am), c.groups, D) == -2
    assert _refused("upp_prop_pool_bwd", [s["g_X"]], p(pooled), p(amax), p(c.i1), p(c.u), c.keep, p(s["g_X"]), c.rows, c.groups, D) == -2
    assert _refused("upp_prop_interp_fwd", [s["out"]], p(c.X), p(lc), p(c.i2), p(c.idx8), p(c.w8), p(s["out"]), c.B, c.Lp, c.T, c.G2, D) == -2
    assert _refused("upp_prop_interp_bwd", [s["g_c2"], s["g_X"]], p(c.wgt), p(c.i2), p(c.idx8), p(c.w8), p(s["g_c2"]), p(s["g_X"]), c.B, c.Lp,
                    c.T, c.G2, D) == -2
    assert _refused("upp_prop_fwd", [s["pooled"], am, s["part"], s["mean"], s["rstd"], s["out"]], p(c.X), p(c.i1), p(c.u), c.keep, p(c.i2),
                    p(c.idx8), p(c.w8), p(c.gamma), p(c.beta), p(rm), p(rv), MOM, EPS, 1, p(s["pooled"]), p(am), p(s["part"]), p(s["mean"]),
                    p(s["rstd"]), p(s["out"]), c.B, c.Lp, c.T, c.G2, D) == -2
    assert _bits(rm, c.rm) and _bits(rv, c.rv)
    assert _refused("upp_prop_bwd", [s["g_c2"], s["part"], s["g_gamma"], s["g_beta"], s["g_X"]], p(c.wgt), p(pooled), p(amax), p(stat), p(stat),
                    p(c.gamma), p(c.u), c.keep, p(c.w8), p(index.csr1[0]), p(index.csr1[1]), p(index.csr2[0]), p(index.csr2[1]),
                    p(index.csr8[0]), p(index.csr8[1]), 1, p(s["g_c2"]), p(s["part"]), p(s["g_gamma"]), p(s["g_beta"]), p(s["g_X"]), c.B, c.Lp,
                    c.T, c.G2, D) == -2
    assert _refused("upp_prop_w8_grad", [s["g_w8"]], p(c.wgt), p(c.X), p(pooled), p(stat), p(stat), p(c.gamma), p(c.beta), p(c.i2), p(c.idx8),
                    p(s["g_w8"]), c.B, c.Lp, c.T, c.G2, D) == -2


@pytest.mark.parametrize("G2,code", [(7, -1), (65, -2)])
def test_prop_index_refuses_fewer_than_8_and_more_than_64_centres(G2, code):
    B, T, p = 2, 16, _abi.ptr
    c1, c2 = torch.rand(B, T, 3, device="cuda"), torch.rand(B, G2, 3, device="cuda")
    i1, i2 = torch.zeros(B * G2 * 8, dtype=torch.int64, device="cuda"), torch.zeros(B * G2, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        ops.prop_index(c1, c2, i1, i2, True, 27, 1, 1e-3)
    i1a, i2a, idx8 = (_sentinel(s, torch.int32) for s in ((B * G2 * 8,), (B * G2,), (B, T, 8)))
    w8 = _sentinel((B, T, 8))
    assert _refused("upp_prop_index", [i1a, i2a, idx8, w8], p(c1), p(c2), p(i1), p(i2), 1, B, T, G2, 27, 1, 1e-3, p(i1a), p(i2a), p(idx8),
                    p(w8)) == code


def test_prop_weights_bwd_refuses_1025_tokens():
    T, G2, p = 1025, 8, _abi.ptr
    c1, c2 = torch.rand(1, T, 3, device="cuda"), torch.rand(1, G2, 3, device="cuda")
    idx8, g = torch.zeros(1, T, 8, dtype=torch.int32, device="cuda"), torch.ones(1, T, 8, device="cuda")
    with pytest.raises(RuntimeError):
        ops.prop_weights_bwd(c1, c2, idx8, g, 1e-3)
    g1, g2 = _sentinel((1, T, 3)), _sentinel((1, G2, 3))
    assert _refused("upp_prop_weights_bwd", [g1, g2], p(c1), p(c2), p(idx8), p(g), 1e-3, p(g1), p(g2), 1, T, G2) == -2
