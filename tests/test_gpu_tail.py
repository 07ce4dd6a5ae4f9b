"""The block-tail kernels -- rowln_fwd / rowln_bwd / ln_param_grad of csrc/block.hip; adapter_fwd / adapter_bwd, the fused ln_adapter_fwd /
ln_adapter_bwd and adapter_wgrad_batched of csrc/adapter.hip -- against the float64 reference of tests/_tail_reference.py, at the edges of
their parameter space: column widths around the 64-lane slots, every residue of the 4-, 32- and 16-row workgroups, every row map and
optional input, GELU's tails, split boundaries and empty splits of the batched weight gradients, a second launch of more than 16 jobs, and
the limits that return a status.

The bound, for every output and every case (tests/test_gpu_prop.py):
    err(x) = max|x - f64| / max|f64|,      err(kernel) <= max(2 * err(f32), 2e-6)
where f32 is the SAME formulation run by torch in float32 on the GPU.  Exact checks (row maps, zeros for stripped rows and dropped
samples, saved rows and statistics of the fused forward against the row kernel, determinism, guards) are bit equalities.  Inputs live in
NaN-guarded buffers throughout (a read past the end shows as a NaN); the partial-tile cases also run the C entry points with guarded
outputs.  The generator asserts |keep + u - 1| >= 1e-3 and |ud - p| >= 1e-3 (but for ONE planted element ud == float32(p), which is
kept), so the float32 and float64 masks agree by construction.

Measured on MI355X: (kernel, f32) of the case nearest its bound, per family and output (number of cases).  209 tests, 5 s.  The nearest
any output comes to its bound is 0.36 of it (h of the 1e3 +- 1e-2 rows), 0.24 in every other case.
    row kernels                   xo              h               mean            rstd            g_x             g_y             g_prompt        g_gamma         g_beta
    row columns (32)              7.3e-8, 5.5e-8  1.9e-7, 1.5e-7  1.1e-7, 8.5e-8  1.2e-7, 9.1e-8  1.9e-7, 1.9e-7  1.6e-7, 8.5e-8  -               1.7e-7, 6.9e-8  7.0e-8, 1.2e-7
    row maps (18)                 7.4e-8, 8.6e-8  1.7e-7, 1.1e-7  1.3e-7, 6.2e-8  1.1e-7, 1.1e-7  1.4e-7, 1.4e-7  1.3e-7, 6.8e-8  9.8e-8, 1.5e-7  1.5e-7, 1.5e-7  7.4e-8, 7.4e-8
    row options (40)              7.9e-8, 7.9e-8  1.5e-7, 1.5e-7  1.6e-7, 9.6e-8  1.3e-7, 6.7e-8  2.0e-7, 8.6e-8  1.3e-7, 1.3e-7  1.2e-7, 1.2e-7  1.4e-7, 1.4e-7  7.3e-8, 1.3e-7
    row drop-path (8)             7.1e-8, 7.1e-8  1.4e-7, 1.1e-7  1.0e-7, 1.0e-7  1.0e-7, 1.0e-7  1.3e-7, 1.3e-7  1.2e-7, 1.2e-7  -               1.1e-7, 1.4e-7  6.4e-8, 7.7e-8
    row edges (3)                 0, 0            2.4e-3, 3.4e-3  1.8e-7, 1.3e-7  2.3e-5, 4.4e-5  5.9e-4, 1.5e-3  -               -               3.3e-3, 5.6e-3  5.4e-8, 8.9e-8
    adapter, 32 rows              out             s1              g_ha            g_W1            g_b1            g_W2            g_b2
    adapter (36)                  3.4e-7, 3.8e-7  1.2e-7, 4.6e-7  4.1e-7, 6.1e-7  4.2e-7, 5.7e-7  3.8e-7, 3.9e-7  3.8e-7, 3.9e-7  2.7e-7, 9.0e-8
    fused tail, forward           out             xo              mean            rstd            s1
    tail rows, forward (24)       1.5e-7, 2.2e-7  7.7e-8, 7.7e-8  1.5e-7, 1.0e-7  1.2e-7, 1.2e-7  2.3e-7, 2.8e-7
    tail options, forward (6)     1.6e-7, 3.1e-7  5.1e-8, 5.1e-8  1.3e-7, 1.5e-7  9.8e-8, 9.0e-8  2.5e-7, 6.0e-7
    fused tail, backward          g_x             g_y             g_gamma         g_beta          g_W1            g_b1            g_W2            g_b2
    tail rows, one-launch (24)    2.5e-7, 3.3e-7  1.5e-7, 2.3e-7  4.3e-7, 4.5e-7  3.7e-7, 2.3e-7  3.5e-7, 7.4e-7  3.5e-7, 6.7e-7  2.8e-7, 4.4e-7  1.5e-7, 1.1e-7
    tail rows, two-launch (24)    3.0e-7, 4.8e-7  1.8e-7, 2.9e-7  4.3e-7, 4.5e-7  3.0e-7, 3.0e-7  3.1e-7, 4.3e-7  3.3e-7, 9.7e-7  2.9e-7, 2.3e-7  2.6e-7, 1.1e-7
    tail rows, factors (24)       2.5e-7, 3.3e-7  1.5e-7, 2.3e-7  4.3e-7, 4.5e-7  4.5e-7, 4.2e-7  4.7e-7, 5.6e-7  3.7e-7, 5.8e-7  4.3e-7, 4.2e-7  3.7e-7, 1.2e-7
    tail options, one-launch (6)  2.4e-7, 2.6e-7  2.4e-7, 2.6e-7  2.9e-7, 4.7e-7  2.5e-7, 5.3e-7  2.4e-7, 5.2e-7  3.9e-7, 4.8e-7  2.3e-7, 4.6e-7  1.2e-7, 8.5e-8
    tail options, two-launch (6)  2.4e-7, 3.3e-7  2.2e-7, 2.6e-7  3.5e-7, 5.4e-7  2.5e-7, 4.8e-7  3.2e-7, 8.0e-7  3.6e-7, 4.8e-7  2.7e-7, 5.0e-7  1.7e-7, 1.0e-7
    tail options, factors (6)     2.4e-7, 2.6e-7  2.4e-7, 2.6e-7  3.2e-7, 5.4e-7  2.6e-7, 4.8e-7  3.0e-7, 8.0e-7  4.2e-7, 4.8e-7  2.9e-7, 6.0e-7  2.0e-7, 6.8e-8
    tail frozen, one-launch (4)   1.9e-7, 4.2e-7  2.4e-7, 2.0e-7  3.5e-7, 4.4e-7  2.4e-7, 4.8e-7  2.5e-7, 4.5e-7  3.2e-7, 7.1e-7  2.2e-7, 4.9e-7  1.2e-7, 7.1e-8
    tail frozen, two-launch (4)   1.7e-7, 4.2e-7  1.8e-7, 2.0e-7  2.3e-7, 4.4e-7  2.2e-7, 4.8e-7  3.0e-7, 4.5e-7  1.7e-7, 7.1e-7  2.3e-7, 4.9e-7  2.4e-7, 7.1e-8
    tail frozen, factors (4)      1.9e-7, 4.2e-7  2.4e-7, 2.0e-7  3.5e-7, 4.4e-7  2.3e-7, 4.8e-7  2.6e-7, 4.5e-7  3.2e-7, 7.1e-7  2.5e-7, 4.9e-7  1.9e-7, 7.1e-8
    weight gradients per job      g_W1            g_b1            g_W2            g_b2
    wgrad batched (59)            3.7e-7, 2.7e-7  4.1e-7, 2.5e-7  3.3e-7, 7.0e-7  2.5e-7, 1.5e-7
    wgrad partial (59)            3.7e-7, 2.7e-7  4.1e-7, 2.5e-7  2.3e-7, 4.8e-7  2.0e-7, 9.5e-8
    ln_param_grad (5): g_gamma 1.7e-7, 1.7e-7; g_beta 7.1e-8, 7.8e-8.  fac = [ga | d] of upp_ln_adapter_bwd_factors (4): 2.6e-7, 2.2e-7.
    HF.layer_norm, D = 512, last = 2: 1.1e-7, 1.3e-7.  g_prompt_b, the per-sample prompt gradient: 1.1e-7, 1.1e-7 (maps), 1.8e-7, 1.8e-7 (options).
The large figures of `row edges` are the rows of 1e3 +- 1e-2: the row, rounded to f32, keeps three digits of its deviation from the mean, in
the kernel and in torch alike; no case needs to be reported relative to f32 only.  No case missed the bound and no kernel was changed: the
defects found are in the wrappers (below).

Found and fixed with this file (iccv2025-upp_amd/upp_hip/ops.py, functional.py; test_wrappers_refuse_wrong_tensors and
test_layer_norm_with_last_refuses_a_2d_input hold them):
  * ops.adapter_fwd / adapter_bwd / ln_adapter_bwd / ln_adapter_bwd_fused / rowln_fwd / rowln_bwd checked none of their tensors and
    ops.ln_adapter_fwd not its y, ybias, u and ud: a float64 u, a (B, Lout) tensor for the (B Lout, 32) dropout uniforms or a transposed
    weight view was read as raw float32 memory.  Each now checks device, float32, contiguity and the exact shape of every tensor it
    passes on, from metadata alone (no synchronisation, no copy).
  * HF.layer_norm(x, ln, last=k) on a 2-D x stripped ROWS on the kernel path and COLUMNS on its fallback path: both raise ValueError.

Mutants (each built from a scratch copy, run once against this file and against the tail tests of tests/test_gpu_block.py -- rowln x 6,
adapter_kernel x 8, block_tail_in_one_launch x 6, rowln_ybias: 21 cases):
  1. gelu_grad's density constant 0.3989: fails 82 cases here (all 36 of adapter_32_row_kernels, every tail case, all 8 queues of
     batched_weight_gradients) -- and the 8 cases of the old test_adapter_kernel_forward_backward: at rtol 5e-5 the old suite did see this one.
  2. adapter_wgrad_kernel takes keepf from R instead of r_hi: passes, here and in the old tests, and has to: it is an EQUIVALENT mutant.
     `per` is rounded up to a multiple of the 16-row step, so a step never straddles r_lo + per; the only r_hi inside a step is R itself.
     The neighbour that does count a row twice at every split boundary (2b: r_hi = min(R, r_lo + per + 1)) fails 10 cases here
     (batched_weight_gradients[2080 | mixed4 | 8193 | 33mixed], tail_row_counts_and_maps[144 | 2080] x 3 maps through the factors form)
     and 3 of the old block_tail cases (B = 32).
  3. upp_adapter_wgrad_batched passes scale[j] in its second launch: fails batched_weight_gradients[17x5 | 33mixed] (g_b2 of the jobs
     behind the 16th); old tests: 21 pass.
  4. ln_adapter_bwd_kernel fills Hs without the `live ?` select: passes, here and in the old tests, and has to: EQUIVALENT.  The rows past
     R then hold ha of row R - 1 (the loads are clamped), and Hs feeds only dW1 = ga^T ha, where ga of those rows is an exact 0.  The
     neighbour on the g_out tile (4b: Zs without the select, which db2 sums over all 16 rows) fails 30 cases here (every tail case with
     B Lout % 16 != 0, batched_weight_gradients through its partial-matrix form) and 1 of the old tests (99 rows).
  5. rowln_fwd_kernel's variance without the column mask: fails 133 cases here (every row case but those of D = 512, where no
     column is masked, and every fused-tail case through the bit equality of its statistics with the row kernel's); old tests: 11 of 21 fail.
  6. the zero fill of stripped prompt rows starts at z = blockIdx.x + 1: fails 32 cases here (every strip-map tail case, the guarded
     runs, the NaN-in-stripped-rows pair); old tests: 4 of 21 fail.
"""
import ctypes
import itertools
import types

import numpy as np
import pytest
import torch

import _tail_reference as R
from test_gpu_step_tail import guarded
from upp_hip import _abi, ops
from upp_hip import functional as HF

pytestmark = pytest.mark.gpu

DA, H = 384, 32                  # the adapter's width and bottleneck
F32, F64 = torch.float32, torch.float64
INSERTS, STRIPS = (R.INSERT_CLS, R.INSERT), (R.STRIP_CLS, R.STRIP)
MODE_NAME = {R.IDENTITY: "identity", R.INSERT_CLS: "insert_cls", R.INSERT: "insert", R.STRIP_CLS: "strip_cls", R.STRIP: "strip"}
assert (HF.ROW_IDENTITY, HF.ROW_INSERT_CLS, HF.ROW_INSERT, HF.ROW_STRIP_CLS, HF.ROW_STRIP) == (0, 1, 2, 3, 4)


def _bits(a, b):
    """Bit equality (NaN payloads included) of two tensors of one dtype; None equals None."""
    if a is None or b is None:
        return a is None and b is None
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def gin(t, off=0):
    """A CPU tensor -> its copy on the device inside a NaN-guarded buffer, `off` floats off the 16-byte aligned start."""
    if t is None:
        return None
    t = t.contiguous()
    v, _ = guarded(t.numel(), t.dtype, off)
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


# ---------------------------------------------------------------------------------------------- input conditions
def drop_uniforms(B, keep, g, kind="mixed"):
    """(B,) drop-path uniforms with |keep + u - 1| >= 1e-3: the float32 floor equals the float64 one by construction."""
    k = R.f32(keep)
    u = torch.rand(B, generator=g)
    if kind == "dropped":
        u = u * (1.0 - k - 2e-3)
    elif kind == "kept":
        u = (1.0 - k + 2e-3) + u * (k - 4e-3)
    else:
        u[0] = 0.05 if k < 0.9 else 0.5
        u[-1] = 0.95
    near = (k + u.double() - 1.0).abs() < 1.5e-3
    u[near] = u[near] + 4e-3
    assert float((k + u.double() - 1.0).abs().min()) >= 1e-3 and float(u.max()) < 1.0 and float(u.min()) >= 0.0
    assert np.array_equal(R.drop_select(u.numpy(), keep), np.floor(k + u.double().numpy()))
    if kind == "dropped":
        assert float(R.drop_select(u.numpy(), keep).max()) == 0.0
    if kind == "kept":
        assert float(R.drop_select(u.numpy(), keep).min()) == 1.0
    return u


def dropout_uniforms(rows, p, g, plant=True):
    """(rows, H) dropout uniforms with |ud - p| >= 1e-3, except the planted ud[0, 0] == float32(p) (kept)."""
    p32 = np.float32(p)
    ud = torch.rand(rows, H, generator=g)
    near = (ud.double() - float(p32)).abs() < 1.5e-3
    ud[near] = ud[near] + 4e-3
    d = (ud.double() - float(p32)).abs()
    if plant and p > 0:
        ud[0, 0] = float(p32)
        d[0, 0] = 1.0
        assert R.dropout_select(ud.numpy(), p)[0, 0] == 1.0
    assert float(d.min()) >= 1e-3
    assert np.array_equal(R.dropout_select(ud.numpy(), p), (ud.double().numpy() >= float(p32)).astype(np.float32))
    return ud


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


def judge(family, label, got, f32, f64, keys):
    """The bound for every key; every figure is printed before anything is asserted."""
    bad = []
    for k in keys:
        if f64[k] is None:
            assert got[k] is None, (family, label, k, "is not asked for and must be None")
            continue
        assert got[k] is not None, (family, label, k)
        e = f64[k].reshape(got[k].shape)
        assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(f32[k]).all()), (k, "the reference itself overflows")
        if not bool(torch.isfinite(got[k]).all()):
            bad.append((k, "non-finite"))
            continue
        ek, ef = _err(got[k], e), _err(f32[k].reshape(e.shape), e)
        print("TAILERR | %s | %s | %s | %.2e | %.2e" % (family, label, k, ek, ef))
        if not ek <= max(2.0 * ef, 2e-6):
            bad.append((k, ek, ef))
    assert not bad, (family, label, bad)


def _same(a, b, what):
    for k in a:
        assert _bits(a[k], b[k]), what + ": " + k


# ============================================================================================== 1. row kernels
ROW_KEYS = ("xo", "h", "mean", "rstd", "g_x", "g_y", "g_prompt_b", "g_prompt", "g_gamma", "g_beta")


def row_case(B, Lin, Dm, mode, P, opts, seed, keep=0.7, eps=1e-5, u_kind="mixed"):
    """opts: subset of {add, y, ybias, u, ln, no_gxo}.  Every tensor sits in a guarded buffer, shifted 1 or 3 floats off alignment (the
    row kernels load single floats)."""
    g = torch.Generator().manual_seed(seed)
    Lo = R.lout(mode, Lin, P)
    assert Lo >= 1 and ("y" in opts or not ({"ybias", "u"} & set(opts)))
    c = types.SimpleNamespace(B=B, Lin=Lin, D=Dm, mode=mode, P=P, Lo=Lo, keep=keep if "u" in opts else 1.0, eps=eps, opts=set(opts), gen=g)
    c.x = _rand(g, B, Lin, Dm) * 0.8 + 0.2
    c.add = _rand(g, B, Lin, Dm) * 0.5 if "add" in opts else None
    c.prompts = _rand(g, P, Dm) if (P > 0 and mode in INSERTS) else None
    c.y = _rand(g, B, Lin, Dm) if "y" in opts else None
    c.ybias = 0.2 * _rand(g, Dm) if "ybias" in opts else None
    c.u = drop_uniforms(B, keep, g, u_kind) if "u" in opts else None
    c.gamma = 1 + 0.2 * _rand(g, Dm) if "ln" in opts else None
    c.beta = 0.2 * _rand(g, Dm) if "ln" in opts else None
    c.g_xo = None if "no_gxo" in opts else _rand(g, B, Lo, Dm)
    c.g_h = _rand(g, B, Lo, Dm) if "ln" in opts else None
    assert c.g_xo is not None or c.g_h is not None
    return c


ROW_TENSORS = ("x", "add", "prompts", "y", "ybias", "u", "gamma", "beta", "g_xo", "g_h")


def finish_row(c):
    for i, k in enumerate(ROW_TENSORS):
        setattr(c, k, gin(getattr(c, k), off=1 + 2 * (i % 2)))
    c.ref = {}
    return c


def row_reference(c, dtype):
    if dtype not in c.ref:
        c.ref[dtype] = R.rowln(c.x, c.add, c.prompts, c.y, c.ybias, c.u, c.keep, c.gamma, c.beta, c.eps, c.mode, c.P, c.g_xo, c.g_h, dtype)
    return c.ref[dtype]


def run_row(c, need_x=True, need_prompt=True, need_y=True, need_ln=True):
    """ops.rowln_fwd + ops.rowln_bwd, the parameter gradients summed from their partials by the library (ops.sum_rows)."""
    xo, h, mean, rstd = ops.rowln_fwd(c.x, c.add, c.prompts, c.mode, c.P, c.y, c.u, c.keep, c.gamma, c.beta, c.eps, c.Lo, ybias=c.ybias)
    g_x, g_p, g_y, part = ops.rowln_bwd(c.g_xo, c.g_h, xo, mean, rstd, c.gamma, c.mode, c.u, c.keep, c.B, c.Lin, c.Lo, c.D, c.P,
                                        need_x, need_prompt, need_y and c.y is not None, need_ln)
    res = dict(xo=xo, h=h, mean=mean, rstd=rstd, g_x=g_x, g_y=g_y, g_prompt_b=g_p, g_prompt=None, g_gamma=None, g_beta=None)
    if g_p is not None:
        res["g_prompt"] = ops.sum_rows(g_p.view(c.B, c.P * c.D)).view(c.P, c.D)
    if part is not None:
        res["g_gamma"], res["g_beta"] = ops.sum_rows(part, 0, c.D), ops.sum_rows(part, c.D, c.D)
    return res


def check_row(c, family, label):
    a, b = run_row(c), run_row(c)
    _same(a, b, "second run differs")
    f32, f64 = row_reference(c, F32), row_reference(c, F64)
    if c.y is None:                                            # without a residual the assembled rows are a copy (or one f32 addition)
        assert torch.equal(a["xo"].double(), f32["xo"]), "row map"
    if c.mode in STRIPS and c.P > 0:
        dropped = slice(1, 1 + c.P) if c.mode == R.STRIP_CLS else slice(0, c.P)
        assert float(a["g_x"][:, dropped].abs().max()) == 0.0 and (a["g_y"] is None or float(a["g_y"][:, dropped].abs().max()) == 0.0)
    if c.y is not None and c.u is not None:                    # dropped samples: an exact zero residual gradient
        sel = torch.from_numpy(R.drop_select(c.u.cpu().numpy(), c.keep)).cuda()
        assert float(a["g_y"][sel == 0].abs().max() if bool((sel == 0).any()) else 0.0) == 0.0
    judge(family, label, a, f32, f64, ROW_KEYS)
    return a


ROW_SHAPES = [(1, 1), (2, 13), (5, 7), (4, 17)]      # B * L = 1, 26, 35, 68: every residue of the 4 rows per workgroup; 1, 7, 9, 17 workgroups


@pytest.mark.parametrize("B,Lin", ROW_SHAPES)
@pytest.mark.parametrize("Dm", [1, 63, 64, 65, 96, 384, 500, 512])
def test_row_columns_and_row_counts(Dm, B, Lin):
    """Clamped column slots and the store mask c < D around the 64-lane slots up to the cap (512); workgroup counts below, and not a
    multiple of, the 8-way XCD remap; a last workgroup of 1, 2, 3 and 4 rows."""
    assert [(b * l) % 4 for b, l in ROW_SHAPES] == [1, 2, 3, 0] and [(b * l + 3) // 4 for b, l in ROW_SHAPES] == [1, 7, 9, 17]
    c = finish_row(row_case(B, Lin, Dm, R.IDENTITY, 0, ("add", "y", "ybias", "u", "ln"), seed=Dm * 100 + B * Lin, eps=1e-5 if Dm % 2 else 1e-6))
    check_row(c, "row columns", "D=%d rows=%d" % (Dm, B * Lin))


MAP_CASES = [(R.IDENTITY, 0, 13)] + [(m, P, 13) for m in (R.INSERT_CLS, R.INSERT, R.STRIP_CLS, R.STRIP) for P in (0, 1, 10)]
MAP_CASES += [(R.STRIP_CLS, 10, 11), (R.STRIP, 10, 11), (R.STRIP_CLS, 1, 2), (R.INSERT, 10, 1), (R.INSERT_CLS, 1, 1)]


@pytest.mark.parametrize("mode,P,Lin", MAP_CASES)
def test_row_maps(mode, P, Lin):
    """The five maps with 0, 1 and 10 prompts; STRIP_CLS / STRIP that leave ONE row (only the cls row; the last token); INSERT in front of
    one token.  Strip maps walk the backward by INPUT row: B * Lin = 39 | 33 rows, a partial last workgroup."""
    c = finish_row(row_case(3, Lin, 65, mode, P, ("add", "y", "ybias", "u", "ln"), seed=mode * 1000 + P * 10 + Lin))
    if (mode, P, Lin) in ((R.STRIP_CLS, 10, 11), (R.STRIP, 10, 11)):
        assert c.Lo == 1
    check_row(c, "row maps", "%s P=%d Lin=%d" % (MODE_NAME[mode], P, Lin))


OPTION_SETS = [o for n in range(6) for o in itertools.combinations(("add", "y", "ybias", "u", "ln"), n)
               if ("y" in o or not ({"ybias", "u"} & set(o)))]


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "+".join(o) or "plain")
def test_row_optional_inputs(opts, eps):
    """With and without each of add, y, ybias, u and the LayerNorm (20 sets), on the map that has prompt rows (no residual there)."""
    c = finish_row(row_case(3, 6, 96, R.INSERT_CLS, 3, opts, seed=len(opts) * 7 + int(eps * 1e7), eps=eps))
    check_row(c, "row options", "%s eps=%g" % ("+".join(opts) or "plain", eps))


@pytest.mark.parametrize("keep,kind", [(0.7, "mixed"), (0.7, "dropped"), (0.7, "kept"), (1.0, "kept")])
def test_row_drop_path_batches(keep, kind):
    """keep = 0.7 and 1.0; a batch whose samples are all dropped (rows = x + add exactly) and one where all are kept.  Without a
    gradient of the rows (the has_gxo = false path) on top."""
    for opts in (("add", "y", "ybias", "u", "ln"), ("y", "u", "ln", "no_gxo")):
        c = finish_row(row_case(4, 9, 65, R.STRIP_CLS, 2, opts, seed=int(keep * 10) + len(kind), keep=keep, u_kind=kind))
        a = check_row(c, "row drop-path", "keep=%g %s%s" % (keep, kind, " no g_xo" if "no_gxo" in opts else ""))
        if kind == "dropped" and "add" in opts:
            want = (c.x + c.add)[:, [0] + list(range(3, 9))]
            assert _bits(a["xo"], want) and float(a["g_y"].abs().max()) == 0.0


def test_row_backward_outputs_that_are_not_asked_for():
    """Each need_* combination _RowLN.backward can ask for: an output that is not asked for is None, the others keep their bits; and the
    autograd node returns the same bits as the wrappers."""
    c = finish_row(row_case(3, 7, 65, R.INSERT_CLS, 3, ("add", "y", "ybias", "u", "ln"), seed=77))
    full = run_row(c)
    pairs = dict(need_x=("g_x",), need_prompt=("g_prompt_b", "g_prompt"), need_y=("g_y",), need_ln=("g_gamma", "g_beta"))
    for flags in itertools.product([False, True], repeat=4):
        kw = dict(zip(pairs, flags))
        got = run_row(c, **kw)
        for name, keys in pairs.items():
            for k in keys:
                assert (got[k] is None) if not kw[name] else _bits(got[k], full[k]), (kw, k)
        assert _bits(got["xo"], full["xo"]) and _bits(got["h"], full["h"])
    leaves = [t.detach().requires_grad_(True) for t in (c.x, c.add, c.prompts, c.y, c.gamma, c.beta)]
    xo, h = HF.rowln(leaves[0], add=leaves[1], prompts=leaves[2], y=leaves[3], ybias=c.ybias, u=c.u, keep=c.keep, gamma=leaves[4],
                     beta=leaves[5], mode=c.mode, P=c.P, eps=c.eps)
    gr = torch.autograd.grad((xo * c.g_xo).sum() + (h * c.g_h).sum(), leaves)
    for g_, k in zip(gr, ("g_x", "g_x", "g_prompt", "g_y", "g_gamma", "g_beta")):
        assert _bits(g_, full[k]), k
    assert _bits(xo.detach(), full["xo"]) and _bits(h.detach(), full["h"])


@pytest.mark.parametrize("kind", ["constant_row", "offset", "one_column"])
def test_row_numerical_edges(kind):
    """A constant row (variance 0: rstd = eps^-1/2, h = beta; 1.25 * 96 sums exactly), rows of 1e3 +- 1e-2 (the variance is four
    digits below the mean: the kernel's two-pass form must hold what torch's holds), one column carrying all of a row's energy."""
    c = row_case(3, 5, 96, R.IDENTITY, 0, ("ln",), seed=len(kind))
    if kind == "constant_row":
        c.x[1, 2] = 1.25
    elif kind == "offset":
        c.x = 1e3 + 1e-2 * _rand(c.gen, 3, 5, 96)
    else:
        c.x = 1e-3 * _rand(c.gen, 3, 5, 96)
        c.x[:, :, 17] = 100.0
    finish_row(c)
    a = check_row(c, "row edges", kind)
    if kind == "constant_row":
        assert float(a["mean"][1, 2]) == 1.25 and float(a["rstd"][1, 2]) == pytest.approx(1e-5 ** -0.5, rel=1e-6)
        assert _bits(a["h"][1, 2], c.beta)


@pytest.mark.parametrize("mode,Dm,B,Lin", [(R.INSERT_CLS, 1, 1, 1), (R.STRIP_CLS, 65, 5, 7), (R.STRIP, 500, 2, 13), (R.IDENTITY, 512, 1, 3)])
def test_row_kernels_write_nothing_outside_their_outputs(mode, Dm, B, Lin):
    """The C entry points with every output inside a sentinel-filled buffer, partial last workgroups; the same bits as the wrappers."""
    P = 0 if mode == R.IDENTITY else 3
    c = finish_row(row_case(B, Lin, Dm, mode, P, ("add", "y", "ybias", "u", "ln"), seed=Dm + B))
    lib, p = _abi.load(), _abi.ptr
    nD, n = B * c.Lo * Dm, B * c.Lo
    npart = int(lib.upp_rowln_part_floats(B, Lin, c.Lo, Dm, mode))
    assert npart == ((B * (Lin if mode in STRIPS else c.Lo) + 3) // 4) * 2 * Dm
    outs = dict(xo=guarded(nD, F32, 1), h=guarded(nD, F32, 3), mean=guarded(n, F32, 1), rstd=guarded(n, F32, 2),
                g_x=guarded(B * Lin * Dm, F32, 3), g_y=guarded(B * Lin * Dm, F32, 1), g_p=guarded(B * P * Dm, F32, 2), part=guarded(npart, F32, 1))
    v = {k: t[0] for k, t in outs.items()}
    has_p = P > 0 and mode in INSERTS
    st = _abi.stream()
    assert lib.upp_rowln_fwd(p(c.x), p(c.add), p(c.prompts), mode, P, p(c.y), p(c.ybias), p(c.u), c.keep, p(c.gamma), p(c.beta), c.eps,
                             p(v["xo"]), p(v["h"]), p(v["mean"]), p(v["rstd"]), B, Lin, c.Lo, Dm, st) == 0
    assert lib.upp_rowln_bwd(p(c.g_xo), p(c.g_h), p(v["xo"]), p(v["mean"]), p(v["rstd"]), p(c.gamma), mode, p(c.u), c.keep, p(v["g_x"]),
                             p(v["g_p"]) if has_p else None, p(v["g_y"]), p(v["part"]), B, Lin, c.Lo, Dm, P, st) == 0
    torch.cuda.synchronize()
    for k, (_, chk) in outs.items():
        chk()
    for k, t in v.items():
        assert k == "g_p" and not has_p or bool(torch.isfinite(t).all()), k + " was not written completely"
    a = run_row(c)
    for k, w in (("xo", "xo"), ("h", "h"), ("mean", "mean"), ("rstd", "rstd"), ("g_x", "g_x"), ("g_y", "g_y")):
        assert _bits(v[k], a[w].reshape(-1)), k
    if has_p:
        assert _bits(v["g_p"], a["g_prompt_b"].reshape(-1))
    assert _bits(ops.sum_rows(v["part"].view(-1, 2 * Dm).clone(), 0, Dm), a["g_gamma"])


@pytest.mark.parametrize("Dm,rows,chunks", [(65, 5, 32), (65, 37, 32), (384, 5, 32), (384, 130, 32), (384, 37, 7)])
def test_ln_param_grad(Dm, rows, chunks):
    """ops.ln_param_grad: fewer rows than chunks (the empty chunks are exact zeros), rows % 4 != 0, a chunk of 1, 2, 5 and 6 rows."""
    g = torch.Generator().manual_seed(Dm + rows)
    xo, g_h = gin(_rand(g, rows, Dm) * 0.8 + 0.2, 1), gin(_rand(g, rows, Dm), 3)
    gamma, beta = gin(1 + 0.2 * _rand(g, Dm), 1), gin(0.2 * _rand(g, Dm), 3)
    _, _, mean, rstd = ops.rowln_fwd(xo.view(1, rows, Dm), None, None, 0, 0, None, None, 1.0, gamma, beta, 1e-5, rows, want_xo=False)
    mean, rstd = mean.view(rows), rstd.view(rows)
    lib, p = _abi.load(), _abi.ptr
    part, chk = guarded(2 * chunks * Dm, F32, 1)
    assert lib.upp_ln_param_grad(p(g_h), p(xo), p(mean), p(rstd), p(part), rows, Dm, chunks, _abi.stream()) == 0
    torch.cuda.synchronize()
    chk()
    part = part.view(2, chunks, Dm)
    if chunks == 32:
        assert _bits(part, ops.ln_param_grad(g_h, xo, mean, rstd))
    per = (rows + chunks - 1) // chunks
    used = (rows + per - 1) // per
    assert used < chunks or rows >= chunks
    assert float(part[:, used:].abs().max() if used < chunks else 0.0) == 0.0          # empty chunks: exact zeros
    got = dict(g_gamma=ops.sum_rows(part[0].clone()), g_beta=ops.sum_rows(part[1].clone()))

    def ref(dtype):
        x_, gh_ = xo.to(dtype), g_h.to(dtype)
        _, m_, r_ = R.ln_fwd(x_, gamma.to(dtype), beta.to(dtype), 1e-5)
        _, gg, gb = R.ln_bwd(gh_, x_, m_, r_, gamma.to(dtype))
        return dict(g_gamma=gg.double(), g_beta=gb.double())

    judge("ln_param_grad", "D=%d rows=%d chunks=%d" % (Dm, rows, chunks), got, ref(F32), ref(F64), ("g_gamma", "g_beta"))


def _sentinel(shape):
    return torch.full(shape, float("nan"), device="cuda")


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in ts)


def test_513_columns_are_refused_and_layer_norm_falls_back_to_the_module():
    """D = 513: the range status from both row entry points, nothing written; HF.layer_norm takes the module there."""
    c = finish_row(row_case(2, 5, 513, R.IDENTITY, 0, ("ln",), seed=513))
    with pytest.raises(RuntimeError):
        ops.rowln_fwd(c.x, None, None, 0, 0, None, None, 1.0, c.gamma, c.beta, 1e-5, 5)
    stat = torch.ones(2, 5, device="cuda")
    with pytest.raises(RuntimeError):
        ops.rowln_bwd(c.g_xo, c.g_h, c.x, stat, stat, c.gamma, 0, None, 1.0, 2, 5, 5, 513, 0, True, False, False, True)
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    xo, h, mean, rstd, g_x = _sentinel((2, 5, 513)), _sentinel((2, 5, 513)), _sentinel((2, 5)), _sentinel((2, 5)), _sentinel((2, 5, 513))
    assert lib.upp_rowln_fwd(p(c.x), None, None, 0, 0, None, None, None, 1.0, p(c.gamma), p(c.beta), 1e-5, p(xo), p(h), p(mean), p(rstd),
                             2, 5, 5, 513, st) == -2
    assert lib.upp_rowln_bwd(p(c.g_xo), p(c.g_h), p(c.x), p(stat), p(stat), p(c.gamma), 0, None, 1.0, p(g_x), None, None, None,
                             2, 5, 5, 513, 0, st) == -2
    assert _untouched(xo, h, mean, rstd, g_x)
    ln = torch.nn.LayerNorm(513).cuda()
    with torch.no_grad():
        ln.weight.copy_(c.gamma); ln.bias.copy_(c.beta)
    assert _bits(HF.layer_norm(c.x, ln), ln(c.x)) and _bits(HF.layer_norm(c.x, ln, last=2), ln(c.x[:, -2:]))
    # ... and at 512 it is the row kernel, which agrees with the module within the bound
    c = finish_row(row_case(2, 5, 512, R.IDENTITY, 0, ("ln",), seed=512))
    ln = torch.nn.LayerNorm(512).cuda()
    with torch.no_grad():
        ln.weight.copy_(c.gamma); ln.bias.copy_(c.beta)
    want = R.ln_fwd(c.x.double()[:, -2:], c.gamma.double(), c.beta.double(), ln.eps)[0]
    judge("layer_norm", "D=512 last=2", dict(h=HF.layer_norm(c.x, ln, last=2).detach()), dict(h=ln(c.x[:, -2:]).detach().double()), dict(h=want), ("h",))


def test_layer_norm_with_last_refuses_a_2d_input():
    """`last` on (R, D) would strip ROWS on the kernel path and COLUMNS on the module path: both raise."""
    x = torch.randn(12, 384, device="cuda")
    with pytest.raises(ValueError):
        HF.layer_norm(x, torch.nn.LayerNorm(384).cuda(), last=4)
    with pytest.raises(ValueError):
        HF.layer_norm(torch.randn(12, 513, device="cuda"), torch.nn.LayerNorm(513).cuda(), last=4)        # the fallback's side
    with pytest.raises(ValueError):
        HF.layer_norm(x.double(), torch.nn.LayerNorm(384).cuda().double(), last=4)


# ============================================================================================== 2. adapter, 32-row kernels
AD_KEYS = ("out", "s1", "g_ha", "g_W1", "g_b1", "g_W2", "g_b2")


def adapter_weights(g, w1_scale=1.0, off=0):
    return dict(W1=gin(w1_scale * _rand(g, H, DA) / DA ** 0.5, off), b1=gin(0.1 * _rand(g, H), off), W2=gin(_rand(g, DA, H) / H ** 0.5, off),
                b2=gin(0.1 * _rand(g, DA), off))


def adapter_case(Rr, p, with_ud, s, seed):
    """W1 scaled by 2.5: |s1| up to ~8 (GELU's tails); two planted rows reach s1 = +-14, where the derivative's expf(-98) underflows."""
    g = torch.Generator().manual_seed(seed)
    c = types.SimpleNamespace(R=Rr, p=p, s=s)
    W1 = 2.5 * _rand(g, H, DA) / DA ** 0.5
    ha = _rand(g, Rr, DA)
    ha[0] = 14.0 / float(W1[0].abs().sum()) * torch.sign(W1[0])
    if Rr > 1:
        ha[Rr - 1] = -14.0 / float(W1[1].abs().sum()) * torch.sign(W1[1])
    c.ha, c.x, c.g_out = gin(ha, 4), gin(_rand(g, Rr, DA), 0), gin(_rand(g, Rr, DA), 4)
    c.W1, c.b1, c.W2, c.b2 = gin(W1, 0), gin(0.1 * _rand(g, H), 4), gin(_rand(g, DA, H) / H ** 0.5, 4), gin(0.1 * _rand(g, DA), 0)
    c.ud = gin(dropout_uniforms(Rr, p, g), 4) if with_ud else None
    c.ref = {}
    return c


def adapter_reference(c, dtype):
    if dtype not in c.ref:
        c.ref[dtype] = R.adapter(c.ha, c.x, c.W1, c.b1, c.W2, c.b2, c.ud, c.p, c.s, c.g_out, dtype)
    return c.ref[dtype]


def _split_adapter_part(part, keys=("g_W1", "g_W2", "g_b1", "g_b2")):
    """[dW1 | dW2 | db1 | db2] partial rows -> the four gradients, summed by the library."""
    sizes = dict(g_W1=H * DA, g_W2=H * DA, g_b1=H, g_b2=DA)
    shapes = dict(g_W1=(H, DA), g_W2=(DA, H), g_b1=(H,), g_b2=(DA,))
    out, off = {}, 0
    for k in keys:
        out[k] = ops.sum_rows(part, off, sizes[k]).view(shapes[k])
        off += sizes[k]
    return out


def run_adapter(c):
    out, s1 = ops.adapter_fwd(c.ha, c.x, c.W1, c.b1, c.W2, c.b2, c.ud, c.p, c.s)
    g_ha, part = ops.adapter_bwd(c.g_out, c.ha, s1, c.W1, c.W2, c.ud, c.p, c.s)
    res = dict(out=out, s1=s1, g_ha=g_ha)
    res.update(_split_adapter_part(part))
    return res


@pytest.mark.parametrize("s", [0.7, 1.0])
@pytest.mark.parametrize("p,with_ud", [(0.0, False), (0.1, True), (0.0, True)])
@pytest.mark.parametrize("Rr", [1, 31, 32, 33, 45, 65])
def test_adapter_32_row_kernels(Rr, p, with_ud, s):
    """One row, one short of / exactly / one past a workgroup, two and three workgroups with a partial last one; p = 0 without and WITH
    uniforms (everything is kept), p = 0.1 with the planted ud == p; the planted s1 = +-14."""
    c = adapter_case(Rr, p, with_ud, s, seed=Rr * 10 + int(p * 10) + with_ud)
    a, b = run_adapter(c), run_adapter(c)
    _same(a, b, "second run differs")
    f64 = adapter_reference(c, F64)
    assert float(f64["s1"].abs().max()) > 13.5 and float(f64["s1"][0, 0]) > 13.5
    if with_ud and p == 0.0:
        c2 = types.SimpleNamespace(**{**vars(c), "ud": None})
        _same(a, run_adapter(c2), "p = 0 with uniforms differs from p = 0 without")
    judge("adapter", "R=%d p=%g%s s=%g" % (Rr, p, " ud" if with_ud else "", s), a, adapter_reference(c, F32), f64, AD_KEYS)


@pytest.mark.parametrize("Rr", [1, 31, 33, 45])
def test_adapter_kernels_write_nothing_outside_their_outputs(Rr):
    c = adapter_case(Rr, 0.1, True, 0.7, seed=Rr)
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    npart = int(lib.upp_adapter_part_floats(Rr, DA))
    outs = dict(out=guarded(Rr * DA, F32, 0), s1=guarded(Rr * H, F32, 4), g_ha=guarded(Rr * DA, F32, 4), part=guarded(npart, F32, 0))
    v = {k: t[0] for k, t in outs.items()}
    assert lib.upp_adapter_fwd(p(c.ha), p(c.x), p(c.W1), p(c.b1), p(c.W2), p(c.b2), p(c.ud), c.p, c.s, p(v["out"]), p(v["s1"]), Rr, DA, H, st) == 0
    assert lib.upp_adapter_bwd(p(c.g_out), p(c.ha), p(v["s1"]), p(c.W1), p(c.W2), p(c.ud), c.p, c.s, p(v["g_ha"]), p(v["part"]), Rr, DA, H, st) == 0
    torch.cuda.synchronize()
    for k, (_, chk) in outs.items():
        chk()
        assert bool(torch.isfinite(v[k]).all()), k + " was not written completely"
    a = run_adapter(c)
    assert _bits(v["out"], a["out"].view(-1)) and _bits(v["s1"], a["s1"].view(-1)) and _bits(v["g_ha"], a["g_ha"].view(-1))
    _same(_split_adapter_part(v["part"].view((Rr + 31) // 32, -1).clone()), {k: a[k] for k in ("g_W1", "g_W2", "g_b1", "g_b2")}, "guarded run")


def test_adapter_refuses_other_widths():
    """D == 384 with H == 32 only: the range status, nothing written."""
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    for Dm, Hm in ((256, 32), (384, 16)):
        ha, x = torch.randn(8, Dm, device="cuda"), torch.randn(8, Dm, device="cuda")
        W1, b1, W2, b2 = torch.randn(Hm, Dm, device="cuda"), torch.zeros(Hm, device="cuda"), torch.randn(Dm, Hm, device="cuda"), torch.zeros(Dm, device="cuda")
        with pytest.raises(RuntimeError):
            ops.adapter_fwd(ha, x, W1, b1, W2, b2, None, 0.0, 0.7)
        out, s1 = _sentinel((8, Dm)), _sentinel((8, Hm))
        assert lib.upp_adapter_fwd(p(ha), p(x), p(W1), p(b1), p(W2), p(b2), None, 0.0, 0.7, p(out), p(s1), 8, Dm, Hm, st) == -2
        xo, mean = _sentinel((1, 8, Dm)), _sentinel((1, 8))
        assert lib.upp_ln_adapter_fwd(p(x), None, None, None, 1.0, 0, 0, p(b2), p(b2), 1e-5, p(W1), p(b1), p(W2), p(b2), None, 0.0, 0.7,
                                      p(xo), p(mean), p(mean), p(s1), p(out), 1, 8, 8, Dm, Hm, st) == -2
        assert _untouched(out, s1, xo, mean)


# ============================================================================================== 3. fused tail, 16-row kernels
TAIL_FWD_KEYS = ("out", "xo", "mean", "rstd", "s1")
TAIL_GRAD_KEYS = ("g_x", "g_y", "g_gamma", "g_beta", "g_W1", "g_b1", "g_W2", "g_b2")
TAIL_SHAPES = {1: (1, 1), 15: (3, 5), 16: (2, 8), 17: (1, 17), 33: (3, 11), 7 * 16 + 3: (5, 23), 9 * 16: (9, 16), 130 * 16: (32, 65)}
assert all(b * l == n for n, (b, l) in TAIL_SHAPES.items())


def tail_case(B, Lo, mode, opts, seed, p=0.1, s=0.7, keep=0.7, eps=1e-5):
    """opts: subset of {y, ybias, u, ud}.  16-byte pieces are loaded from x, y, the weights and g_out: guarded views 0 or 4 floats off."""
    g = torch.Generator().manual_seed(seed)
    P = 0 if mode == R.IDENTITY else 10
    Lin = Lo + P
    c = types.SimpleNamespace(B=B, Lo=Lo, Lin=Lin, P=P, mode=mode, R=B * Lo, p=p if "ud" in opts else 0.0, s=s, keep=keep if "u" in opts else 1.0,
                              eps=eps, opts=set(opts), gen=g)
    c.x = gin(_rand(g, B, Lin, DA) * 0.8 + 0.2, 4)
    c.y = gin(_rand(g, B, Lin, DA), 0) if "y" in opts else None
    c.ybias = gin(0.2 * _rand(g, DA), 1) if "ybias" in opts else None
    c.u = gin(drop_uniforms(B, keep, g), 3) if "u" in opts else None
    c.gamma, c.beta = gin(1 + 0.2 * _rand(g, DA), 0), gin(0.2 * _rand(g, DA), 4)
    for k, t in adapter_weights(g, off=4).items():
        setattr(c, k, t)
    c.ud = gin(dropout_uniforms(c.R, p, g), 1) if "ud" in opts else None
    c.g_out = gin(_rand(g, B, Lo, DA), 4)
    c.ref = {}
    return c


def tail_reference(c, dtype):
    if dtype not in c.ref:
        c.ref[dtype] = R.tail(c.x, c.y, c.ybias, c.u, c.keep, c.mode, c.P, c.gamma, c.beta, c.eps, c.W1, c.b1, c.W2, c.b2, c.ud, c.p, c.s,
                              c.g_out, dtype)
    return c.ref[dtype]


TAIL_PARAMS = ("gamma", "beta", "W1", "b1", "W2", "b2")


def run_tail_forward(c):
    """ops.ln_adapter_fwd; the saved rows and statistics are the row kernel's, bit for bit."""
    out, xo, mean, rstd, s1 = ops.ln_adapter_fwd(c.x, c.y, c.ybias, c.u, c.keep, c.mode, c.P, c.gamma, c.beta, c.eps, c.W1, c.b1, c.W2, c.b2,
                                                 c.ud, c.p, c.s, c.Lo)
    xo_r, _, mean_r, rstd_r = ops.rowln_fwd(c.x, None, None, c.mode, c.P, c.y, c.u, c.keep, c.gamma, c.beta, c.eps, c.Lo, ybias=c.ybias)
    assert _bits(xo, xo_r) and _bits(mean, mean_r) and _bits(rstd, rstd_r), "the fused forward's saved rows differ from the row kernel's"
    return dict(out=out, xo=xo, mean=mean, rstd=rstd, s1=s1)


def run_tail_backward(c, form, frozen=()):
    """HF.ln_adapter + autograd in one of the three backward forms -> the TAIL_GRAD_KEYS (None where `frozen` says so)."""
    t = {k: getattr(c, k) for k in ("x", "y") + TAIL_PARAMS}
    names = [k for k in t if t[k] is not None]
    leaf = {k: t[k].detach().requires_grad_(k not in frozen) for k in names}
    ln = types.SimpleNamespace(weight=leaf["gamma"], bias=leaf["beta"], eps=c.eps)

    def fwd():
        return HF.ln_adapter(leaf["x"], leaf.get("y"), c.ybias, c.u, c.keep, c.mode, c.P, ln, leaf["W1"], leaf["b1"], leaf["W2"], leaf["b2"],
                             c.ud, c.p, c.s)

    want = [k for k in names if k not in frozen]
    res = {"g_" + k: None for k in ("x", "y") + TAIL_PARAMS}
    if form == "factors":
        targets = {leaf[k].data_ptr(): torch.zeros_like(leaf[k]) for k in TAIL_PARAMS if k not in frozen}
        data = [k for k in want if k in ("x", "y")]
        with HF.deferred_sums(targets) as scope:
            out = fwd()
            gr = torch.autograd.grad((out * c.g_out).sum(), [leaf[k] for k in data])
        assert scope.routed == set(targets)
        res.update({"g_" + k: g_ for k, g_ in zip(data, gr)})
        res.update({"g_" + k: targets[leaf[k].data_ptr()] for k in TAIL_PARAMS if k not in frozen})
    else:
        HF.FUSE_TAIL_BACKWARD = form != "two_launch"
        try:
            out = fwd()
            gr = torch.autograd.grad((out * c.g_out).sum(), [leaf[k] for k in want])
        finally:
            HF.FUSE_TAIL_BACKWARD = True
        res.update({"g_" + k: g_ for k, g_ in zip(want, gr)})
    res["out"] = out.detach()
    return res


FORMS = ("one_launch", "two_launch", "factors")


def check_tail(c, family, label, forms=FORMS):
    f32, f64 = tail_reference(c, F32), tail_reference(c, F64)
    fw = run_tail_forward(c)
    _same(fw, run_tail_forward(c), "second forward differs")
    judge(family, label + " forward", fw, f32, f64, TAIL_FWD_KEYS)
    res = {}
    for form in forms:
        a, b = run_tail_backward(c, form), run_tail_backward(c, form)
        _same(a, b, "second %s backward differs" % form)
        assert _bits(a.pop("out"), fw["out"])
        if c.mode in STRIPS:
            dropped = slice(1, 1 + c.P) if c.mode == R.STRIP_CLS else slice(0, c.P)
            assert float(a["g_x"][:, dropped].abs().max()) == 0.0 and (a["g_y"] is None or float(a["g_y"][:, dropped].abs().max()) == 0.0)
        judge(family, label + " " + form, a, f32, f64, TAIL_GRAD_KEYS)
        res[form] = a
    if "one_launch" in res and "factors" in res:                 # the data gradient does not depend on the form of the weight gradients
        assert _bits(res["one_launch"]["g_x"], res["factors"]["g_x"]) and _bits(res["one_launch"]["g_y"], res["factors"]["g_y"])
    return res


@pytest.mark.parametrize("mode", [R.IDENTITY, R.STRIP_CLS, R.STRIP])
@pytest.mark.parametrize("rows", sorted(TAIL_SHAPES))
def test_tail_row_counts_and_maps(rows, mode):
    """B * Lout = 1, 15, 16, 17, 33, 115, 144 and the models' 2080 (130 workgroups of partial sums), each of the three maps the launch
    serves, every optional input present, three backward forms."""
    B, Lo = TAIL_SHAPES[rows]
    c = tail_case(B, Lo, mode, ("y", "ybias", "u", "ud"), seed=rows * 10 + mode)
    check_tail(c, "tail rows", "rows=%d %s" % (rows, MODE_NAME[mode]))


@pytest.mark.parametrize("opts", [(), ("y",), ("y", "ybias"), ("y", "u"), ("ud",), ("y", "ybias", "u")], ids=lambda o: "+".join(o) or "plain")
def test_tail_optional_inputs(opts):
    c = tail_case(3, 11, R.STRIP_CLS, opts, seed=len(opts) + 3 * ("ud" in opts), eps=1e-6)
    check_tail(c, "tail options", "+".join(opts) or "plain")


@pytest.mark.parametrize("frozen", [("gamma", "beta"), ("W1", "b1", "W2", "b2"), ("x",), ("y",)], ids=["ln", "adapter", "x", "y"])
def test_tail_with_frozen_inputs(frozen):
    """Frozen LayerNorm, frozen adapter, x without a gradient, y without a gradient, each on its own: what is not asked for is None, the
    rest keeps the bits of the run that asks for everything (the factors form needs all four adapter buffers: it is the one-launch
    form with a frozen adapter)."""
    c = tail_case(3, 11, R.STRIP, ("y", "ybias", "u", "ud"), seed=41)
    f32, f64 = tail_reference(c, F32), tail_reference(c, F64)
    none = {"g_" + k for k in frozen}
    for form in FORMS:
        full, got = run_tail_backward(c, form), run_tail_backward(c, form, frozen)
        assert _bits(got.pop("out"), full.pop("out"))
        for k in got:
            assert (got[k] is None) if k in none else _bits(got[k], full[k]), (form, k)
        judge("tail frozen", "%s %s" % ("+".join(frozen), form), got, f32, {k: (None if k in none else v) for k, v in f64.items()}, TAIL_GRAD_KEYS)


@pytest.mark.parametrize("rows", [1, 15, 17, 33])
def test_tail_kernels_write_nothing_outside_their_outputs(rows):
    """Partial 16-row workgroups through the C entry points, every output in a guarded buffer; the same bits as the wrappers."""
    B, Lo = TAIL_SHAPES[rows]
    c = tail_case(B, Lo, R.STRIP_CLS, ("y", "ybias", "u", "ud"), seed=rows)
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream()
    nwg = (rows + 15) // 16
    npart = int(lib.upp_ln_adapter_part_floats(rows, DA))
    assert npart == nwg * (2 * H * DA + H + DA)
    outs = dict(xo=guarded(rows * DA, F32, 0), mean=guarded(rows, F32, 1), rstd=guarded(rows, F32, 3), s1=guarded(rows * H, F32, 1),
                out=guarded(rows * DA, F32, 4), g_x=guarded(B * c.Lin * DA, F32, 1), g_y=guarded(B * c.Lin * DA, F32, 3),
                part=guarded(npart, F32, 1), ln_part=guarded(nwg * 2 * DA, F32, 3), g_x2=guarded(B * c.Lin * DA, F32, 3),
                g_y2=guarded(B * c.Lin * DA, F32, 1), fac=guarded(rows * 2 * H, F32, 1), ln_part2=guarded(nwg * 2 * DA, F32, 1))
    v = {k: t[0] for k, t in outs.items()}
    assert lib.upp_ln_adapter_fwd(p(c.x), p(c.y), p(c.ybias), p(c.u), c.keep, c.mode, c.P, p(c.gamma), p(c.beta), c.eps, p(c.W1), p(c.b1),
                                  p(c.W2), p(c.b2), p(c.ud), c.p, c.s, p(v["xo"]), p(v["mean"]), p(v["rstd"]), p(v["s1"]), p(v["out"]),
                                  B, c.Lin, Lo, DA, H, st) == 0
    common = (p(c.g_out), p(v["xo"]), p(v["mean"]), p(v["rstd"]), p(c.gamma), p(c.beta), p(v["s1"]), p(c.W1), p(c.W2), p(c.ud), c.p, c.s,
              p(c.u), c.keep, c.mode, c.P)
    assert lib.upp_ln_adapter_bwd_fused(*common, p(v["g_x"]), p(v["g_y"]), p(v["part"]), p(v["ln_part"]), B, c.Lin, Lo, DA, H, st) == 0
    assert lib.upp_ln_adapter_bwd_factors(*common, p(v["g_x2"]), p(v["g_y2"]), p(v["fac"]), p(v["ln_part2"]), B, c.Lin, Lo, DA, H, st) == 0
    torch.cuda.synchronize()
    for k, (_, chk) in outs.items():
        chk()
        assert bool(torch.isfinite(v[k]).all()), k + " was not written completely"
    fw = run_tail_forward(c)
    for k in TAIL_FWD_KEYS:
        assert _bits(v[k], fw[k].reshape(-1)), k
    a = run_tail_backward(c, "one_launch")
    assert _bits(v["g_x"], a["g_x"].reshape(-1)) and _bits(v["g_y"], a["g_y"].reshape(-1))
    assert _bits(v["g_x2"], v["g_x"]) and _bits(v["g_y2"], v["g_y"]) and _bits(v["ln_part2"], v["ln_part"])
    _same(_split_adapter_part(v["part"].view(nwg, -1).clone()), {k: a[k] for k in ("g_W1", "g_W2", "g_b1", "g_b2")}, "guarded run")
    assert _bits(ops.sum_rows(v["ln_part"].view(nwg, 2 * DA).clone(), 0, DA), a["g_gamma"])
    judge("tail guards", "rows=%d" % rows, dict(fac=v["fac"].view(rows, 2 * H)), tail_reference(c, F32), tail_reference(c, F64), ("fac",))


# ============================================================================================== 4. batched weight gradients
WG_KEYS = ("g_W1", "g_b1", "g_W2", "g_b2")


def wgrad_queue(rows, seed):
    """One tail per job (identity map, its own rows, gradient and `scale`; the jobs share one adapter), run through the fused forward and
    the two backward forms -> list of (case, job tuple of ops.adapter_wgrad_batched, gradients of the partial-matrix form)."""
    g = torch.Generator().manual_seed(seed)
    w = adapter_weights(g, off=4)
    queue = []
    for j, n in enumerate(rows):
        s = 0.5 + 0.05 * (j % 11) + 0.01 * (j // 11)               # a different scale per job (33 distinct values)
        c = tail_case(1, n, R.IDENTITY, ("ud",), seed=seed * 100 + j, s=s)
        for k, t in w.items():
            setattr(c, k, t)
        fw = run_tail_forward(c)
        args = (c.g_out, fw["xo"], fw["mean"], fw["rstd"], c.gamma, c.beta, fw["s1"], c.W1, c.W2, c.ud, c.p, c.s, None, 1.0, 0, 0, n, True, False)
        _, _, fac, _ = ops.ln_adapter_bwd_fused(*args, True, False, factors=True)
        _, _, part, _ = ops.ln_adapter_bwd_fused(*args, True, False)
        job = (fw["xo"].view(n, DA), fw["mean"].view(n), fw["rstd"].view(n), c.gamma, c.beta, c.g_out.view(n, DA), fac, c.s)
        queue.append((c, job, _split_adapter_part(part)))
    return queue


WG_QUEUES = {"1": [1], "16": [16], "17": [17], "2080": [2080], "mixed4": [1, 17, 2400, 130], "8193": [8193], "17x5": [5] * 17,
             "33mixed": [1 + (7 * i * i) % 150 + (300 if i in (3, 20) else 0) for i in range(33)]}


@pytest.mark.parametrize("name", list(WG_QUEUES))
def test_batched_weight_gradients(name):
    """R below, at and past 16; jobs of different R under one `splits` taken from the largest (the small jobs' empty splits are exact
    zeros); R = 8193: 64 splits of 144 rows, more than 128 per accumulator; 17 and 33 jobs: a second and a third launch with their own
    slice of the pointer arrays; a different `scale` per job.  Each job against float64, in both forms; two runs bit-identical."""
    rows = WG_QUEUES[name]
    queue = wgrad_queue(rows, seed=len(name) + sum(rows) % 97)
    assert len({c.s for c, _, _ in queue}) == len(rows)
    jobs = [j for _, j, _ in queue]
    parts = ops.adapter_wgrad_batched(jobs)
    again = ops.adapter_wgrad_batched(jobs)
    splits = int(_abi.load().upp_adapter_wgrad_splits(max(rows)))
    assert splits == min(64, (max(rows) + 127) // 128) and (name != "8193" or (splits == 64 and -(-8193 // 64) > 128))
    for i, ((c, _, by_part), part, part2) in enumerate(zip(queue, parts, again)):
        assert part.shape == (splits, 2 * H * DA + H + DA) and _bits(part, part2), "job %d: second run differs" % i
        per = (((c.R + splits - 1) // splits + 15) // 16) * 16          # rows per split: a multiple of the 16-row step
        used = (c.R + per - 1) // per
        if used < splits:
            assert float(part[used:].abs().max()) == 0.0, "job %d: an empty split is not zero" % i
        got = _split_adapter_part(part)
        f32, f64 = tail_reference(c, F32), tail_reference(c, F64)
        judge("wgrad batched", "%s job %d R=%d" % (name, i, c.R), got, f32, f64, WG_KEYS)
        judge("wgrad partial", "%s job %d R=%d" % (name, i, c.R), by_part, f32, f64, WG_KEYS)


def test_batched_weight_gradients_refuse_a_misaligned_view():
    """A `fac` or `g_out` view shifted by one float: the range status from the host check, before any launch."""
    (c, job, _), = wgrad_queue([17], seed=5)
    lib = _abi.load()
    for which in (5, 6):
        t = job[which]
        buf = torch.zeros(t.numel() + 4, device="cuda")
        shifted = buf[1:1 + t.numel()].view(t.shape)
        shifted.copy_(t)
        assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
        bad = job[:which] + (shifted,) + job[which + 1:]
        with pytest.raises(RuntimeError):
            ops.adapter_wgrad_batched([bad])
        part = _sentinel((1, 2 * H * DA + H + DA))
        arr = lambda i: (ctypes.c_void_p * 1)(bad[i].data_ptr())          # noqa: E731
        rc = lib.upp_adapter_wgrad_batched(arr(0), arr(1), arr(2), arr(3), arr(4), arr(5), arr(6), (ctypes.c_int * 1)(17), (ctypes.c_float * 1)(c.s),
                                           (ctypes.c_void_p * 1)(part.data_ptr()), 1, 1, DA, H, _abi.stream())
        assert rc == -2 and _untouched(part)
    assert lib.upp_adapter_wgrad_batched(None, None, None, None, None, None, None, None, None, None, 0, 65, DA, H, _abi.stream()) == -2   # at most 64 splits


# ============================================================================================== 5. containment
def _other_rows_keep_their_bits(clean, dirty, row, keys):
    for k in keys:
        a, b = clean[k].reshape(clean[k].shape[0] * clean[k].shape[1], -1), dirty[k].reshape(clean[k].shape[0] * clean[k].shape[1], -1)
        keep = torch.ones(a.shape[0], dtype=torch.bool, device="cuda")
        keep[row] = False
        assert _bits(a[keep], b[keep]), k
        assert bool(torch.isnan(b[row]).any()), k + ": the poisoned row shows no NaN"


@pytest.mark.parametrize("rows", [17, 33])
def test_a_nan_row_stays_in_its_row(rows):
    """NaN in one token row of x (forward) or of g_out (backward): every other row of out, xo, g_x and g_y keeps the bits of the clean
    run, in the row kernels, the 32-row adapter and the fused tail (identity map: output row = input row)."""
    B, Lo = TAIL_SHAPES[rows]
    row = rows - 2
    c = tail_case(B, Lo, R.IDENTITY, ("y", "ybias", "u", "ud"), seed=rows + 50)
    clean_f = run_tail_forward(c)
    kw = dict(g_xo=c.g_out, g_h=c.g_out, add=None, prompts=None, D=DA, Lin=c.Lin)
    rc = types.SimpleNamespace(**{**vars(c), **kw})
    clean_r = run_row(rc)
    args = lambda f, go: (go, f["xo"], f["mean"], f["rstd"], c.gamma, c.beta, f["s1"], c.W1, c.W2, c.ud, c.p, c.s, c.u, c.keep, c.mode, c.P,   # noqa: E731
                          c.Lin, True, True, True, True)
    clean_b = dict(zip(("g_x", "g_y"), ops.ln_adapter_bwd_fused(*args(clean_f, c.g_out))[:2]))
    ha = clean_r["h"].view(rows, DA)
    clean_a = dict(zip(("out", "s1"), ops.adapter_fwd(ha, clean_r["xo"].view(rows, DA), c.W1, c.b1, c.W2, c.b2, c.ud, c.p, c.s)))
    clean_a["g_ha"] = ops.adapter_bwd(c.g_out.view(rows, DA), ha, clean_a["s1"], c.W1, c.W2, c.ud, c.p, c.s)[0]
    # forward: poison x
    x2 = gin(c.x.cpu(), 4)
    x2.view(-1, DA)[row, 5] = float("nan")
    d = types.SimpleNamespace(**{**vars(c), "x": x2})
    _other_rows_keep_their_bits(clean_f, run_tail_forward(d), row, ("out", "xo"))
    _other_rows_keep_their_bits(clean_r, run_row(types.SimpleNamespace(**{**vars(rc), "x": x2})), row, ("xo", "h"))
    ha2 = ha.clone()
    ha2[row, 5] = float("nan")
    out2, _ = ops.adapter_fwd(ha2, clean_r["xo"].view(rows, DA), c.W1, c.b1, c.W2, c.b2, c.ud, c.p, c.s)
    _other_rows_keep_their_bits(dict(out=clean_a["out"].view(1, rows, DA)), dict(out=out2.view(1, rows, DA)), row, ("out",))
    # backward: poison g_out
    go2 = gin(c.g_out.cpu(), 4)
    go2.view(-1, DA)[row, 7] = float("nan")
    dirty_b = dict(zip(("g_x", "g_y"), ops.ln_adapter_bwd_fused(*args(clean_f, go2))[:2]))
    _other_rows_keep_their_bits(clean_b, dirty_b, row, ("g_x", "g_y"))
    dirty_r = run_row(types.SimpleNamespace(**{**vars(rc), "g_xo": go2}))
    _other_rows_keep_their_bits(clean_r, dirty_r, row, ("g_x",))
    g_ha2 = ops.adapter_bwd(go2.view(rows, DA), ha, clean_a["s1"], c.W1, c.W2, c.ud, c.p, c.s)[0]
    _other_rows_keep_their_bits(dict(g=clean_a["g_ha"].view(1, rows, DA)), dict(g=g_ha2.view(1, rows, DA)), row, ("g",))


@pytest.mark.parametrize("mode", [R.STRIP_CLS, R.STRIP])
def test_nan_in_the_stripped_prompt_rows_changes_nothing(mode):
    """The rows a strip map drops are never read: NaN there leaves every output's bits unchanged (row kernels and fused tail,
    forward, backward and weight partials)."""
    c = tail_case(3, 11, mode, ("y", "ybias", "u", "ud"), seed=60 + mode)
    dropped = slice(1, 1 + c.P) if mode == R.STRIP_CLS else slice(0, c.P)
    x2, y2 = gin(c.x.cpu(), 4), gin(c.y.cpu(), 0)
    x2[:, dropped] = float("nan")
    y2[:, dropped] = float("nan")
    d = types.SimpleNamespace(**{**vars(c), "x": x2, "y": y2})
    _same(run_tail_forward(c), run_tail_forward(d), "fused forward")
    for form in FORMS:
        _same(run_tail_backward(c, form), run_tail_backward(d, form), form)
    kw = dict(g_xo=c.g_out, g_h=c.g_out, add=None, prompts=None, D=DA)
    _same(run_row(types.SimpleNamespace(**{**vars(c), **kw})), run_row(types.SimpleNamespace(**{**vars(d), **kw})), "row kernels")


def test_a_nan_row_in_one_queued_job_leaves_the_other_jobs_alone():
    queue = wgrad_queue([17, 40, 5] + [3] * 15, seed=9)            # 18 jobs: the poisoned one and job 17 sit in different launches
    jobs = [j for _, j, _ in queue]
    clean = ops.adapter_wgrad_batched(jobs)
    g2 = jobs[1][5].clone()
    g2[33, 100] = float("nan")
    dirty = ops.adapter_wgrad_batched([jobs[0], jobs[1][:5] + (g2,) + jobs[1][6:]] + jobs[2:])
    for i, (a, b) in enumerate(zip(clean, dirty)):
        assert _bits(a, b) if i != 1 else bool(torch.isnan(b).any()), i


# ============================================================================================== 6. wrapper arguments
def _wrapper_calls():
    """name -> (function of a dict of tensors, the dict).  Every tensor argument of the seven wrappers, valid."""
    c = tail_case(2, 5, R.STRIP_CLS, ("y", "ybias", "u", "ud"), seed=70)
    fw = run_tail_forward(c)
    rows = c.R
    r = finish_row(row_case(2, 5, DA, R.INSERT_CLS, 3, ("add", "y", "ybias", "u", "ln"), seed=71))
    rf = run_row(r)
    ha = rf["h"].view(-1, DA)
    udr = gin(dropout_uniforms(ha.shape[0], 0.1, c.gen), 0)
    s1r = ops.adapter_fwd(ha, rf["xo"].view(-1, DA), c.W1, c.b1, c.W2, c.b2, udr, 0.1, 0.7)[1]
    go_r = torch.randn_like(ha)
    return {
        "rowln_fwd": (lambda t: ops.rowln_fwd(t["x"], t["add"], t["prompts"], r.mode, r.P, t["y"], t["u"], r.keep, t["gamma"], t["beta"], r.eps, r.Lo,
                                              ybias=t["ybias"]),
                      dict(x=r.x, add=r.add, prompts=r.prompts, y=r.y, u=r.u, gamma=r.gamma, beta=r.beta, ybias=r.ybias)),
        "rowln_bwd": (lambda t: ops.rowln_bwd(t["g_xo"], t["g_h"], t["xo"], t["mean"], t["rstd"], t["gamma"], r.mode, t["u"], r.keep, r.B, r.Lin,
                                              r.Lo, r.D, r.P, True, True, True, True),
                      dict(g_xo=r.g_xo, g_h=r.g_h, xo=rf["xo"], mean=rf["mean"], rstd=rf["rstd"], gamma=r.gamma, u=r.u)),
        "adapter_fwd": (lambda t: ops.adapter_fwd(t["ha"], t["x"], t["W1"], t["b1"], t["W2"], t["b2"], t["u"], 0.1, 0.7),
                        dict(ha=ha, x=rf["xo"].view(-1, DA), W1=c.W1, b1=c.b1, W2=c.W2, b2=c.b2, u=udr)),
        "adapter_bwd": (lambda t: ops.adapter_bwd(t["g_out"], t["ha"], t["s1"], t["W1"], t["W2"], t["u"], 0.1, 0.7),
                        dict(g_out=go_r, ha=ha, s1=s1r, W1=c.W1, W2=c.W2, u=udr)),
        "ln_adapter_fwd": (lambda t: ops.ln_adapter_fwd(c.x, t["y"], t["ybias"], t["u"], c.keep, c.mode, c.P, c.gamma, c.beta, c.eps, c.W1, c.b1,
                                                        c.W2, c.b2, t["ud"], c.p, c.s, c.Lo),
                           dict(y=c.y, ybias=c.ybias, u=c.u, ud=c.ud)),
        "ln_adapter_bwd": (lambda t: ops.ln_adapter_bwd(t["g_out"], t["xo"], t["mean"], t["rstd"], t["gamma"], t["beta"], t["s1"], t["W1"], t["W2"],
                                                        t["u"], c.p, c.s),
                           dict(g_out=c.g_out, xo=fw["xo"], mean=fw["mean"], rstd=fw["rstd"], gamma=c.gamma, beta=c.beta, s1=fw["s1"], W1=c.W1,
                                W2=c.W2, u=c.ud)),
        "ln_adapter_bwd_fused": (lambda t: ops.ln_adapter_bwd_fused(t["g_out"], t["xo"], t["mean"], t["rstd"], t["gamma"], t["beta"], t["s1"], t["W1"],
                                                                    t["W2"], t["ud"], c.p, c.s, t["u"], c.keep, c.mode, c.P, c.Lin, True, True, True,
                                                                    True),
                                 dict(g_out=c.g_out, xo=fw["xo"], mean=fw["mean"], rstd=fw["rstd"], gamma=c.gamma, beta=c.beta, s1=fw["s1"],
                                      W1=c.W1, W2=c.W2, ud=c.ud, u=c.u)),
    }, rows


def _bad_versions(t):
    """Four ways to pass the wrong thing for tensor t, each of which an unguarded launch would still read INSIDE allocated memory: a wider
    dtype of the same shape, a larger shape, a non-contiguous view of a larger buffer with t's shape, and (never launched) a CPU tensor."""
    big = torch.zeros(tuple(2 * n for n in t.shape), device="cuda")
    strided = big[tuple(slice(0, 2 * n, 2) for n in t.shape)]
    assert strided.shape == t.shape and not strided.is_contiguous() or t.numel() == 1
    longer = torch.zeros((t.shape[0] + 1,) + tuple(t.shape[1:]), device="cuda")
    return dict(dtype=t.double(), shape=longer, view=strided if t.numel() > 1 else None, cpu=t.cpu())


@pytest.mark.parametrize("name", ["rowln_fwd", "rowln_bwd", "adapter_fwd", "adapter_bwd", "ln_adapter_fwd", "ln_adapter_bwd", "ln_adapter_bwd_fused"])
def test_wrappers_refuse_wrong_tensors(name):
    """Device, float32, contiguity and the exact shape of every tensor a wrapper passes on, optional ones included: a float64 u, a
    (B, Lout) tensor for the (B Lout, 32) uniforms or a transposed weight view used to be read as raw float32 memory."""
    calls, _ = _wrapper_calls()
    fn, tensors = calls[name]
    fn(tensors)                                                   # the valid call passes
    n = 0
    for k, t in tensors.items():
        for kind, bad in _bad_versions(t).items():
            if bad is None:
                continue
            with pytest.raises((RuntimeError, TypeError)):
                fn({**tensors, k: bad})
            n += 1
        if t.dim() == 2 and t.shape[0] != t.shape[1]:             # the transposed view of a matrix (right numel, wrong shape, strided)
            with pytest.raises(RuntimeError):
                fn({**tensors, k: t.t()})
    assert n >= 4 * len(tensors) - 2
    if name == "ln_adapter_fwd":                                  # the (B, Lout) tensor where (B Lout, 32) uniforms belong: inside a larger buffer
        with pytest.raises(RuntimeError):
            fn({**tensors, "ud": torch.zeros(2 * 5 * H, device="cuda")[:10].view(2, 5)})
