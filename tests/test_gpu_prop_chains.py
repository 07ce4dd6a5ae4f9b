"""The backward and pool kernels of the fused propagation step (upp_prop_bwd, upp_prop_res_bwd, upp_prop_res_pool_fwd) against an
order-preserving restatement, bit for bit.

The kernels walk a CSR row as start -> entries (one lane-parallel load of up to 64) -> per-entry scalars -> data rows, the c2 kernel
requests the data rows of the next batch before the current one is added, and all keep 6 column slots at D <= 384 and 8 beyond; the
fused tail fetches the index lists of both rows of a wave before the first row's gathers.  None of that may change a
floating-point operation, so the oracle here is not float64 (tests/test_gpu_prop.py judges the values) but the operations themselves,
restated in NumPy with every operation rounded to float32: the batches of 8 (g_c2) and 4 (g_X) entries, the zero-weight terms that fill
the last batch with the row's last entry (they turn a -0.0 into +0.0), the pairs of the i2 list, the 64-entry chunks of a long row, the
stride-4 ownership and the (s0 + s1) + (s2 + s3) of the BatchNorm gradient, the per-workgroup (sum, M2) partials of the pool.  Every
comparison is on the raw bits, so +-0 counts; every output lies in a sentinel-filled buffer that must stay untouched around it.

The restatement was checked once against the build before the row walk changed (same files, same cases): every case equal.

Shapes are the smallest that reach each path: groups % 4 != 0 and B * Lp = 102 rows (no multiple of the 4 rows of a workgroup); one
column slot partly filled (D = 65), exactly six (384), seven (385: the first size of the 8-slot kernels), all eight (512), 500;
rows of the i1 list with 0 ... 129 entries (batch edges 3/4/5, 8/9, sweep and chunk edges 63/64/65, a third chunk at 129) and rows
of the idx8 list with 0 ... 65 (batch edges 7/8/9, 16/17, sweep edges 63/64/65).
"""
import types

import numpy as np
import pytest
import torch

from test_gpu_step_tail import guarded
from upp_hip import _abi, ops

pytestmark = pytest.mark.gpu

KEEP_G, KEEP_DP, MOM, EPS = 0.9, 0.8, 0.1, 1e-5
f32 = np.float32


# ---------------------------------------------------------------------------------------------- float32 restatement
def fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum is rounded to odd there (TwoSum gives the exact error), so the
    final rounding to float32 sees what a single rounding of a * b + c would."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward_inf = (err > 0) == (s > 0)                      # the exact value lies further from zero than s
    step = np.where(toward_inf, 1, -1).astype(np.int64)
    bits = np.where(fix, bits + step, bits)
    return bits.view(np.float64).astype(f32)


def drop_factor(u, keep, idx):
    """floorf(keep + u[idx]) / keep, or 1 without uniforms."""
    if u is None:
        return np.ones(np.shape(idx), f32)
    return np.floor(f32(keep) + u[idx]) / f32(keep)


def csr(keys, rows):
    """Ascending positions of every key: the stable CSR of upp_csr_build."""
    order = np.argsort(keys, kind="stable")
    start = np.searchsorted(keys[order], np.arange(rows + 1))
    return start, order


def ref_pool(c, res):
    """prop_pool_(res_)stats_kernel: pooled, amax and the (sum, M2) partials of every workgroup of 4 groups."""
    rows8 = c.n["i1"].reshape(c.groups, 8)
    f = (f32(1.0) + drop_factor(c.n["u_g"], KEEP_G, np.arange(c.groups))).astype(f32)[:, None]
    mx = np.full((c.groups, c.D), -np.inf, f32)
    sm = np.zeros((c.groups, c.D), f32)
    am = np.zeros((c.groups, c.D), np.uint8)
    for k in range(8):
        r = rows8[:, k]
        if res:
            mb = c.n["mb"] if c.n["mb"] is not None else f32(0.0)
            sc = drop_factor(c.n["u_dp"], KEEP_DP, r // c.Lp)[:, None]
            v = fma(c.n["m"][r] + mb, sc, c.n["x2"][r]) * f
        else:
            v = c.n["x3"][r] * f
        gt = v > mx
        mx = np.where(gt, v, mx)
        am = np.where(gt, np.uint8(k), am)
        sm = sm + v
    pooled = mx + sm * f32(0.125)
    wgs = (c.groups + 3) // 4
    part = np.zeros((wgs, 2, c.D), f32)
    for wg in range(wgs):
        blk = pooled[wg * 4:wg * 4 + 4]
        s = np.zeros(c.D, f32)
        for row in blk:
            s = s + row
        mean = s / f32(len(blk))
        m2 = np.zeros(c.D, f32)
        for row in blk:
            dv = row - mean
            m2 = fma(dv, dv, m2)
        part[wg, 0], part[wg, 1] = s, m2
    return pooled, am, part


def ref_bwd(c, pooled, amax, mean, rstd, res):
    """prop_c2_csr_kernel, prop_bn_grad_kernel and prop_x_csr(_res)_kernel."""
    D, T, Lp = c.D, c.T, c.Lp
    g_out = c.n["g_rows"].reshape(c.rows, D)
    w8 = c.n["w8"].reshape(-1)
    pos = np.arange(c.B * T * 8)
    start8, perm8 = csr((pos // (T * 8)) * c.G2 + c.n["idx8"].reshape(-1), c.groups)
    g_c2 = np.zeros((c.groups, D), f32)
    for gj in range(c.groups):
        ent = perm8[start8[gj]:start8[gj + 1]]
        acc = np.zeros(D, f32)
        for h0 in range(0, len(ent), 8):
            for t in range(8):
                live = h0 + t < len(ent)
                q = ent[h0 + t] if live else ent[-1]
                tok = q // 8
                row = (tok // T) * Lp + (Lp - T) + tok % T
                acc = acc + g_out[row] * (w8[q] if live else f32(0.0))
        g_c2[gj] = f32(0.3) * acc
    xhat = (pooled - mean) * rstd
    wgs = (c.groups + 3) // 4
    part = np.zeros((wgs, 2, D), f32)
    for wg in range(wgs):
        s0, s1 = np.zeros(D, f32), np.zeros(D, f32)
        for g in range(wg * 4, min(wg * 4 + 4, c.groups)):
            s0 = s0 + g_c2[g]
            s1 = s1 + g_c2[g] * xhat[g]
        part[wg, 0], part[wg, 1] = s0, s1
    wave = np.zeros((4, 2, D), f32)
    for w in range(wgs):
        wave[w % 4] = wave[w % 4] + part[w]
    tot = (wave[0] + wave[1]) + (wave[2] + wave[3])
    g_beta, g_gamma = tot[0], tot[1]
    # g_X
    start1, perm1 = csr(c.n["i1"], c.rows)
    start2, perm2 = csr(c.n["i2"], c.rows)
    inv_n = f32(1.0) / f32(c.groups)
    c1 = (g_beta if c.training else np.zeros(D, f32)) * inv_n
    c2 = (g_gamma if c.training else np.zeros(D, f32)) * inv_n
    gr = c.n["gamma"] * rstd
    g_X = np.zeros((c.rows, D), f32)
    for r in range(c.rows):
        acc = g_out[r].copy()
        e2 = perm2[start2[r]:start2[r + 1]]
        for h0 in range(0, len(e2), 2):
            acc = acc + f32(0.3) * g_c2[e2[h0]]
            acc = acc + (f32(0.3) if h0 + 1 < len(e2) else f32(0.0)) * g_c2[e2[min(h0 + 1, len(e2) - 1)]]
        e1 = perm1[start1[r]:start1[r + 1]]
        head = np.zeros(D, f32)
        for c0 in range(0, len(e1), 64):
            chunk = e1[c0:c0 + 64]
            if c0 > 0:
                head = head + acc
                acc = np.zeros(D, f32)
            for h0 in range(0, len(chunk), 4):
                for e_t in range(4):
                    live = h0 + e_t < len(chunk)
                    q = chunk[h0 + e_t] if live else chunk[-1]
                    g, k = q // 8, q % 8
                    f = f32(1.0) + drop_factor(c.n["u_g"], KEEP_G, g) if live else f32(0.0)
                    gp = gr * ((g_c2[g] - c1 - xhat[g] * c2) if c.training else g_c2[g])
                    acc = acc + gp * f32(f) * (f32(0.125) + (amax[g] == k).astype(f32))
        if len(e1) > 64:
            acc = acc + head
        g_X[r] = acc
    out = dict(g_c2=g_c2, part=part.reshape(-1), g_gamma=g_gamma, g_beta=g_beta, g_X=g_X)
    if res:
        out["g_m"] = g_X * drop_factor(c.n["u_dp"], KEEP_DP, np.arange(c.rows) // Lp)[:, None]
    return out


# ---------------------------------------------------------------------------------------------- cases
def make_case(B, T, G2, D, training, dp, seed, lead=11, edit=None):
    g = torch.Generator().manual_seed(seed)
    Lp = lead + T
    c = types.SimpleNamespace(B=B, T=T, G2=G2, D=D, Lp=Lp, rows=B * Lp, groups=B * G2, training=training)
    t = {}
    t["x2"] = torch.randn(B, Lp, D, generator=g) * 0.7 + 0.3
    t["m"] = torch.randn(B, Lp, D, generator=g) * 0.5
    t["mb"] = torch.randn(D, generator=g) * 0.1
    if dp:
        t["u_dp"] = torch.rand(B, generator=g)
        t["u_dp"][0], t["u_dp"][B - 1] = 0.05, 0.95                # the first sample's branch dropped, the last kept
        t["u_g"] = torch.rand(B * G2, generator=g)
    else:
        t["u_dp"], t["u_g"] = None, None
    t["i1"] = torch.randint(0, B * Lp, (B * G2 * 8,), generator=g).int()     # any row of any sample, as the flat index convention lists them
    t["i2"] = torch.randint(0, B * Lp, (B * G2,), generator=g).int()         # duplicates included: rows with several i2 entries
    t["idx8"] = torch.randint(0, G2, (B, T, 8), generator=g).int()
    w8 = torch.rand(B, T, 8, generator=g) + 0.05
    t["w8"] = w8 / w8.sum(-1, keepdim=True)
    t["gamma"], t["beta"] = torch.linspace(0.5, 1.5, D), torch.linspace(-0.2, 0.2, D)
    t["rm"], t["rv"] = torch.linspace(-0.1, 0.4, D), torch.linspace(0.6, 1.7, D)
    t["g_rows"] = torch.randn(B, Lp, D, generator=g)
    t["g_rows"][:, :, ::7] *= -0.0                                 # signed zeros among the gradients: a +0.0 padding term must show
    if edit:
        edit(t, c, g)
    # the rows x3 the plain kernels read: rowln_fwd's fmaf(m + mb, dp, x2), restated
    c.n = {k: (None if v is None else v.contiguous().numpy()) for k, v in t.items()}
    sc = drop_factor(c.n["u_dp"], KEEP_DP, np.arange(c.rows) // Lp)[:, None]
    c.n["x3"] = fma(c.n["m"].reshape(c.rows, D) + c.n["mb"], sc, c.n["x2"].reshape(c.rows, D))
    c.n["x2"], c.n["m"] = c.n["x2"].reshape(c.rows, D), c.n["m"].reshape(c.rows, D)
    c.t = {k: (None if v is None else v.contiguous().cuda()) for k, v in t.items()}
    c.t["x3"] = torch.from_numpy(c.n["x3"]).view(B, Lp, D).cuda()
    c.csr1 = ops.csr_build(c.t["i1"], c.rows)
    c.csr2 = ops.csr_build(c.t["i2"], c.rows)
    c.csr8 = ops.csr_build(c.t["idx8"].view(-1), c.groups, seg_len=T * 8, seg_rows=G2)
    return c


def bits_equal(name, got, want):
    got = got.detach().cpu().contiguous().numpy().reshape(-1)
    want = np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, name
    if got.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d" % (name, bad.size, got.size, bad[0])


def check_case(c):
    """Pool forward (residual form), then both backward entry points on its saved tensors; every output inside guard bands."""
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    D, groups, rows = c.D, c.groups, c.rows
    nparts = lib.upp_prop_part_floats(groups, D)
    checks = []

    def out(n, dtype=torch.float32):
        view, chk = guarded(n, dtype)
        checks.append(chk)
        return view

    t = c.t
    pooled, amax, part, mean, rstd = out(groups * D), out(groups * D, torch.uint8), out(nparts), out(D), out(D)
    rm, rv = t["rm"].clone(), t["rv"].clone()
    assert lib.upp_prop_res_pool_fwd(p(t["x2"]), p(t["m"]), p(t["mb"]), p(t["u_dp"]), KEEP_DP, p(t["i1"]), p(t["u_g"]), KEEP_G, p(rm), p(rv), MOM,
                                     EPS, int(c.training), p(pooled), p(amax), p(part), p(mean), p(rstd), c.B, c.Lp, c.G2, D, st) == 0
    w_pooled, w_amax, w_part = ref_pool(c, True)
    bits_equal("pooled", pooled, w_pooled)
    bits_equal("amax", amax, w_amax)
    bits_equal("part", part, w_part)
    if c.training:                                             # the statistics the partials become: against float64 of the pooled rows
        p64 = w_pooled.astype(np.float64)
        np.testing.assert_allclose(mean.cpu().numpy(), p64.mean(0), rtol=0, atol=2e-6 * np.abs(p64).max())
        np.testing.assert_allclose(rstd.cpu().numpy(), 1.0 / np.sqrt(p64.var(0) + EPS), rtol=2e-6)
    # the plain pool kernel on the stored rows x3: the same bits
    pooled3, amax3, part3, mean3, rstd3, out3 = out(groups * D), out(groups * D, torch.uint8), out(nparts), out(D), out(D), out(rows * D)
    rm3, rv3 = t["rm"].clone(), t["rv"].clone()
    assert lib.upp_prop_fwd(p(t["x3"]), p(t["i1"]), p(t["u_g"]), KEEP_G, p(t["i2"]), p(t["idx8"]), p(t["w8"]), p(t["gamma"]), p(t["beta"]), p(rm3),
                            p(rv3), MOM, EPS, int(c.training), p(pooled3), p(amax3), p(part3), p(mean3), p(rstd3), p(out3), c.B, c.Lp, c.T, c.G2,
                            D, st) == 0
    bits_equal("pooled (plain)", pooled3, w_pooled)
    bits_equal("amax (plain)", amax3, w_amax)
    bits_equal("part (plain)", part3, w_part)
    mean_n, rstd_n = mean.cpu().numpy(), rstd.cpu().numpy()
    for res in (True, False):
        want = ref_bwd(c, w_pooled, w_amax, mean_n, rstd_n, res)
        g_c2, bpart, g_gamma, g_beta, g_X, g_m = out(groups * D), out(nparts), out(D), out(D), out(rows * D), out(rows * D)
        common = (p(t["g_rows"]), p(pooled), p(amax), p(mean), p(rstd), p(t["gamma"]), p(t["u_g"]), KEEP_G, p(t["w8"]), p(c.csr1[0]), p(c.csr1[1]),
                  p(c.csr2[0]), p(c.csr2[1]), p(c.csr8[0]), p(c.csr8[1]), int(c.training))
        if res:
            assert lib.upp_prop_res_bwd(*common, p(t["u_dp"]), KEEP_DP, p(g_c2), p(bpart), p(g_gamma), p(g_beta), p(g_X), p(g_m), c.B, c.Lp, c.T,
                                        c.G2, D, st) == 0
            bits_equal("g_m", g_m, want["g_m"])
        else:
            assert lib.upp_prop_bwd(*common, p(g_c2), p(bpart), p(g_gamma), p(g_beta), p(g_X), c.B, c.Lp, c.T, c.G2, D, st) == 0
        for k in ("g_c2", "part", "g_gamma", "g_beta", "g_X"):
            bits_equal("%s (%s)" % (k, "res" if res else "plain"), dict(g_c2=g_c2, part=bpart, g_gamma=g_gamma, g_beta=g_beta, g_X=g_X)[k], want[k])
    torch.cuda.synchronize()
    for chk in checks:
        chk()


def test_restatement_of_fmaf():
    """The float32 fma of the restatement against exact rational arithmetic on values chosen to round differently when rounded twice."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(f32)
    b = rng.standard_normal(4000).astype(f32)
    cc = (rng.standard_normal(4000) * rng.choice([1e-6, 1.0, 1e5], 4000)).astype(f32)
    a[:8], b[:8], cc[:8] = f32(1 + 2 ** -12), f32(1 + 2 ** -12), f32(2 ** -30) * np.arange(-4, 4, dtype=f32)   # exact value near a float32 tie
    got = fma(a, b, cc)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(cc[i]))
        lo = f32(float(exact))                                  # float(Fraction) and f32(float) round twice: take the nearer neighbour exactly
        cands = [lo, np.nextafter(lo, f32(np.inf)), np.nextafter(lo, f32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.int32)) & 1))
        assert got[i] == best, i


@pytest.mark.parametrize("dp", [True, False], ids=["dp", "nodp"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(2, 40, 33, 65), (2, 64, 32, 384), (1, 16, 9, 500)], ids=str)
def test_bits_against_the_restatement(shape, training, dp):
    check_case(make_case(*shape, training, dp, seed=7 + shape[3]))


def _row_with(n, which):
    """List edit: exactly n entries of i1 equal one chosen centre row (which = 'i1'), or exactly n entries of sample 0's idx8 equal one
    chosen level-2 centre (which = 'idx8')."""
    def edit(t, c, g):
        if which == "i1":
            lst, target, other = t["i1"], c.Lp + 30, c.Lp + 31           # a centre row of sample 1
            span = lst.numel()
        else:
            lst, target, other = t["idx8"].view(-1), 3, 4
            span = c.T * 8                                               # sample 0
        lst[lst == target] = other
        lst[torch.randperm(span, generator=g)[:n]] = target
        assert int((lst[:span] == target).sum()) == n
    return edit


@pytest.mark.parametrize("D", [384, 65])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 8, 9, 63, 64, 65, 129])
def test_token_row_listed_by_n_groups(n, D):
    """B * Lp = 2 * 51 rows, 24 groups (192 entries of i1)."""
    check_case(make_case(2, 40, 12, D, True, True, seed=100 + n, edit=_row_with(n, "i1")))


@pytest.mark.parametrize("D", [384, 65])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 16, 17, 63, 64, 65])
def test_level2_centre_listed_by_n_tokens(n, D):
    check_case(make_case(2, 70, 8, D, True, True, seed=200 + n, lead=11, edit=_row_with(n, "idx8")))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("D", [384, 385, 512])
def test_both_slot_counts(D, training):
    """D = 384 runs the 6-slot kernels, 385 and 512 the 8-slot ones; check_case holds every output between sentinel bands."""
    check_case(make_case(2, 12, 5, D, training, True, seed=300 + D))


@pytest.mark.parametrize("lists", ["flat", "random"])
def test_tail_with_the_index_rounds_of_both_rows_first(lists):
    """upp_ln_adapter_prop_fwd at B = 2, Lin = 75 -> Lout = 65 against prop_interp + ln_adapter_fwd (the composition of
    test_gpu_prop_tail.py), torch.equal.  A wave of the tail serves two consecutive output rows and fetches the index lists of both before
    the first row's gathers; Lout is odd, so rows 64 | 65 are the last centre row of cloud 0 and the cls row of cloud 1 (a row without
    lists beside one with), and every wave of cloud 1 pairs rows the other way round."""
    from test_gpu_prop_tail import _old_forward_kernels
    from test_gpu_prop_tail import make_case as tail_case
    c = tail_case(2, True, 10, 64, 32, 384, True, "u", True, 0.1, seed=41, lists=lists)
    assert c.Lp == 75 and c.Lout == 65
    old = _old_forward_kernels(c, True)
    new = ops.ln_adapter_prop_fwd(c.x2, c.m, c.mb, c.u_dp, c.keep_dp, c.mode, c.P, old.pooled, old.mean, old.rstd, c.gamma, c.beta, c.i2, c.idx8,
                                  c.w8, c.lng, c.lnb, 1e-5, c.W1, c.b1, c.W2, c.b2, c.ud, c.pd, 0.7, c.Lout)
    for name, a, b in zip(("out", "xo", "mean", "rstd", "s1"), new, old.tail):
        assert a.shape == b.shape and torch.equal(a, b), name
