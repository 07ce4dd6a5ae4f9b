"""The attention kernels for 1 ... 160 tokens (csrc/attn_flash16.hip: L <= 96, six forward templates, five LDS-staged backward variants
and the exchanging one for 81 ... 96; csrc/attn_long.hip: 97 ... 160, forward modes 0 / 2 (129 ... 132) / 1 (133 ... 144), backward with and
without the vector-ALU tail) against float64: parity with `lse` included, the hazards of a softmax (maximum in the first / last key tile,
in the VALU-written column, elsewhere for the tail query; sharp and constant rows), independence of every (sample, head) from its
neighbours and from the grid's geometry, confinement of a non-finite operand, rows behind the last token, stale LDS contents, determinism
and graph replay, and the argument checks of ops.attn_fwd / ops.attn_bwd.

Bounds are those of tests/test_gpu_attention_stream.py: the project's bounds against the torch f32 formulation (forward rtol 1e-5, atol 2e-6
max|ref|; gradient rtol 2e-5, atol 5e-6 max|ref|) where that formulation is itself inside them against float64, else max|kernel - f64| <=
2 max|torch_f32 - f64| + 2e-6 max|f64|; `lse` rtol 2e-6, atol 2e-6 against float64 logsumexp; hazards e_kernel <= 2 e_torch_f32 + atol of
max|f64| (atol 2e-6 forward, 5e-6 gradient) and `lse` within 4e-6 of max(|lse|, 1).

Measured on MI355X, max|x - f64| / max|f64| of (kernel, torch f32), forward | gradient | lse (absolute), B, H = 3, 2:
    L      forward               gradient              lse
    1      0, 0                  3.6e-7, 0             1.3e-7, 2.5e-7
    2      9.6e-8, 9.7e-8        2.5e-7, 7.5e-8        2.5e-7, 4.9e-7
    15     2.1e-7, 1.7e-7        3.8e-7, 2.0e-7        3.3e-7, 3.1e-7
    16     3.4e-7, 4.3e-7        4.1e-7, 4.9e-7        3.2e-7, 3.4e-7
    17     2.8e-7, 3.6e-7        3.4e-7, 3.4e-7        4.6e-7, 7.0e-7
    32     4.0e-7, 3.7e-7        2.7e-7, 2.1e-7        6.4e-7, 4.8e-7
    33     5.9e-7, 5.9e-7        4.1e-7, 3.8e-7        3.8e-7, 5.2e-7
    48     3.2e-7, 2.9e-7        4.2e-7, 3.4e-7        5.4e-7, 5.4e-7
    49     3.3e-7, 3.8e-7        5.2e-7, 3.4e-7        5.3e-7, 5.2e-7
    64     4.5e-7, 5.1e-7        4.2e-7, 3.7e-7        6.1e-7, 5.8e-7
    65     4.0e-7, 8.7e-7        6.0e-7, 7.9e-7        5.2e-7, 6.0e-7
    75     3.8e-7, 3.7e-7        8.1e-7, 4.8e-7        7.3e-7, 6.0e-7
    80     6.1e-7, 6.3e-7        6.1e-7, 4.9e-7        5.9e-7, 5.9e-7
    81     4.8e-7, 6.8e-7        4.2e-7, 4.0e-7        6.0e-7, 6.0e-7
    96     5.7e-7, 7.7e-7        7.5e-7, 8.5e-7        5.7e-7, 5.8e-7
    97     5.1e-7, 5.3e-7        5.2e-7, 4.9e-7        6.6e-7, 7.7e-7
    127    4.9e-7, 4.5e-7        9.0e-7, 6.0e-7        6.2e-7, 7.2e-7
    128    5.3e-7, 6.9e-7        6.2e-7, 6.8e-7        6.8e-7, 6.5e-7
    129    7.1e-7, 6.1e-7        4.8e-7, 3.7e-7        6.5e-7, 6.7e-7
    132    5.1e-7, 6.1e-7        5.8e-7, 4.6e-7        6.0e-7, 6.7e-7
    133    7.5e-7, 7.8e-7        8.4e-7, 6.9e-7        6.9e-7, 6.7e-7
    139    4.9e-7, 4.7e-7        5.5e-7, 5.3e-7        7.5e-7, 7.5e-7
    144    7.4e-7, 7.5e-7        7.1e-7, 6.9e-7        7.0e-7, 7.2e-7
    145    5.9e-7, 5.5e-7        1.03e-6, 5.7e-7       7.0e-7, 6.5e-7
    159    4.9e-7, 4.3e-7        9.0e-7, 6.4e-7        7.0e-7, 7.4e-7
    160    7.1e-7, 8.0e-7        6.6e-7, 6.0e-7        6.7e-7, 7.1e-7
and at the other grid geometries (L, B x H):
    75, 1 x 1 3.8e-7, 3.7e-7        4.3e-7, 3.5e-7        4.7e-7, 5.3e-7
    75, 1 x 2 4.0e-7, 4.2e-7        4.0e-7, 5.6e-7        6.1e-7, 5.4e-7
    75, 7 x 1 7.8e-7, 4.5e-7        6.0e-7, 5.7e-7        6.3e-7, 6.3e-7
    75, 1 x 12 6.7e-7, 6.7e-7        5.5e-7, 4.1e-7        6.2e-7, 6.4e-7
    75, 32 x 6 5.9e-7, 7.5e-7        7.3e-7, 8.1e-7        7.1e-7, 7.9e-7
    129, 1 x 1 8.1e-7, 7.6e-7        3.9e-7, 5.7e-7        5.9e-7, 6.3e-7
    129, 1 x 2 6.3e-7, 5.1e-7        6.1e-7, 6.2e-7        5.9e-7, 6.7e-7
    129, 7 x 1 1.02e-6, 1.02e-6      8.4e-7, 5.7e-7        6.7e-7, 6.8e-7
    129, 1 x 12 7.0e-7, 4.8e-7        8.4e-7, 6.0e-7        6.9e-7, 6.6e-7
    129, 32 x 6 7.3e-7, 6.3e-7        6.7e-7, 6.1e-7        7.7e-7, 8.1e-7
The torch f32 formulation stayed inside the project's bounds against float64 in every one of these cases, so the project's bounds
against it applied everywhere and the float64 arbitration never had to.  `lse`: the kernels' worst error is 7.7e-7, torch f32 logsumexp's 8.1e-7;
at every length the kernel is inside twice the torch f32 error plus 2e-6, so the streaming kernels' bound (rtol 2e-6, atol 2e-6) holds
here unchanged.  At L = 1 the context row is the V row bit for bit and the forward error 0.

Hazard cases (kernel, torch f32), forward | gradient of max|f64|, lse relative to max(|lse|, 1):
    sharp           75   3.2e-6, 3.2e-6       3.4e-6, 3.4e-6       4.7e-7, 5.5e-7
    sharp           96   3.6e-6, 2.5e-6       3.7e-6, 4.1e-6       3.9e-7, 4.9e-7
    sharp           129  3.6e-6, 4.4e-6       3.2e-6, 2.9e-6       4.3e-7, 4.3e-7
    sharp           139  3.5e-6, 4.2e-6       5.3e-6, 4.9e-6       4.2e-7, 3.9e-7
    sharp           160  5.2e-6, 3.2e-6       3.1e-6, 4.3e-6       3.7e-7, 3.9e-7
    max_first       75   1.28e-5, 1.21e-5     6.1e-6, 6.0e-6       2.9e-7, 2.9e-7
    max_first       96   1.21e-5, 1.02e-5     4.8e-6, 5.3e-6       3.8e-7, 3.8e-7
    max_first       129  9.2e-6, 9.7e-6       8.1e-6, 7.5e-6       3.5e-7, 3.5e-7
    max_first       139  6.9e-6, 6.9e-6       5.3e-6, 5.3e-6       3.0e-7, 3.0e-7
    max_first       160  8.7e-6, 8.2e-6       5.7e-6, 5.1e-6       4.8e-7, 4.8e-7
    max_last        75   9.6e-6, 8.6e-6       9.4e-6, 5.6e-6       3.7e-7, 3.7e-7
    max_last        96   8.3e-6, 9.1e-6       7.4e-6, 8.1e-6       3.8e-7, 3.8e-7
    max_last        129  0, 0                 1.35e-6, 2.3e-7      5.6e-7, 7.6e-7
    max_last        139  1.02e-5, 1.19e-5     4.8e-6, 5.2e-6       3.6e-7, 2.8e-7
    max_last        160  1.05e-5, 1.06e-5     6.5e-6, 6.5e-6       2.0e-7, 2.0e-7
    max_tail_query  75   1.28e-5, 1.21e-5     5.8e-6, 5.7e-6       2.9e-7, 2.9e-7
    max_tail_query  96   1.21e-5, 1.02e-5     4.8e-6, 5.3e-6       3.8e-7, 3.8e-7
    max_tail_query  129  9.2e-6, 9.7e-6       8.4e-6, 7.7e-6       3.5e-7, 3.5e-7
    max_tail_query  139  6.9e-6, 6.9e-6       5.2e-6, 5.3e-6       3.0e-7, 3.0e-7
    max_tail_query  160  8.7e-6, 8.2e-6       5.2e-6, 5.0e-6       4.8e-7, 4.8e-7
    constant_row    75   4.6e-7, 4.4e-7       9.0e-7, 7.8e-7       1.2e-7, 1.2e-7
    constant_row    96   4.8e-7, 4.7e-7       7.9e-7, 5.7e-7       1.4e-7, 1.3e-7
    constant_row    129  5.3e-7, 6.0e-7       8.4e-7, 7.3e-7       1.3e-7, 1.3e-7
    constant_row    139  5.6e-7, 6.2e-7       8.9e-7, 9.2e-7       1.2e-7, 1.2e-7
    constant_row    160  6.8e-7, 6.3e-7       8.1e-7, 6.7e-7       1.2e-7, 1.2e-7
    huge_first      75   4.5e-5, 4.4e-5       2.7e-5, 2.2e-5       2.9e-7, 2.8e-7
    huge_first      96   3.5e-5, 3.1e-5       2.0e-5, 2.0e-5       2.9e-7, 2.9e-7
    huge_first      129  3.2e-5, 3.4e-5       3.8e-5, 2.7e-5       3.3e-7, 3.3e-7
    huge_first      139  3.0e-5, 3.1e-5       2.1e-5, 2.5e-5       3.3e-7, 3.0e-7
    huge_first      160  3.3e-5, 3.3e-5       3.5e-5, 3.3e-5       3.0e-7, 3.0e-7
    huge_last       75   4.2e-5, 4.1e-5       4.0e-5, 4.9e-5       3.8e-7, 3.8e-7
    huge_last       96   3.9e-5, 3.8e-5       2.4e-5, 2.4e-5       4.1e-7, 4.1e-7
    huge_last       129  0, 0                 2.7e-6, 2.3e-7       6.0e-7, 7.3e-7
    huge_last       139  4.6e-5, 4.1e-5       2.9e-5, 3.0e-5       4.4e-7, 3.4e-7
    huge_last       160  5.2e-5, 5.2e-5       3.2e-5, 3.3e-5       3.3e-7, 3.3e-7
max_last / huge_last at 129 put the whole softmax on key 128, the one column written on the vector ALU: the context is V[128] exactly in all
three computations.  The gradient there (true d_q = d_k = 0) is the rounding of dP - delta times the 16 / 32 in channel 0 of K: 1.35e-6 and
2.7e-6 against the bound 2 x 2.3e-7 + 5e-6.

Mutants, built from scratch copies and run once each (never committed): (1) attn_fwd16_kernel with its row maximum forced to 0 fails
huge_first and huge_last at 75 and 96; (2) stage_block leaving rows >= valid unwritten fails 24 of the +-32 and other cases: stale LDS at 97, 129,
132, 133, 139, 144, rows behind the last token at 97, 129, 133, parity at 97, 139, 145, 159 and at 129 with 1 x 1 and 7 x 1, seven hazards
at 129 / 139, independence and determinism at 139; (3) the mode-2 softmax taking its maximum over columns < 128 only fails huge_last at 129.  All three pass
tests/test_gpu_block.py::test_attention_core_forward_backward; (1) and (3) also pass every +-32 case here, which is why the huge kinds exist.
"""
import functools

import numpy as np
import pytest
import torch

from _attention_reference import SCALE, _check_against, _err, _kernels, _memsets, _torch_formulation
from upp_hip import ops

pytestmark = pytest.mark.gpu

# one or more per compiled template and per side of every dispatch edge: 16-row tiles up to 96 (flash16), 97 ... 160 (long: three-block walk),
# 129 ... 132 (mode 2, tail on the vector ALU), 133 ... 144 (mode 1, folded tail strip)
LENGTHS = [1, 2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 75, 80, 81, 96, 97, 127, 128, 129, 132, 133, 139, 144, 145, 159, 160]


@functools.lru_cache(maxsize=None)
def _case(L, B=3, H=2):
    g = torch.Generator(device='cuda').manual_seed(1000 * L + 10 * B + H)
    qkv = torch.randn(B, L, 3 * H * 64, device='cuda', generator=g)
    w = torch.randn(B, L, H * 64, device='cuda', generator=g)
    return qkv, w, H, _torch_formulation(qkv, w, H, torch.float32), _torch_formulation(qkv, w, H, torch.float64)


def _all_finite(ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def _parity(L, B, H):
    qkv, w, H, t32, f64 = _case(L, B, H)
    out, g, lse = _kernels(qkv, w, H)
    print("L = %d, B = %d, H = %d" % (L, B, H))
    e_lse = (lse.double() - f64[2]).abs().max().item()
    print("lse: kernel %.2e torch_f32 %.2e (absolute)" % (e_lse, (t32[2].double() - f64[2]).abs().max().item()))
    assert _all_finite((out, g, lse))
    _check_against("forward", out, t32[0], f64[0], 1e-5, 2e-6)
    _check_against("gradient", g, t32[1], f64[1], 2e-5, 5e-6)
    # lse = m + log l: a few roundings of numbers of size |lse| <= ~10 (f32 epsilon 6e-8) plus the relative error of l (~1e-6)
    np.testing.assert_allclose(lse.cpu().numpy(), f64[2].cpu().numpy(), rtol=2e-6, atol=2e-6)
    return qkv, out, lse


# ---- a. parity with float64, lse included ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_parity_with_the_torch_formulation_and_float64(L):
    qkv, out, lse = _parity(L, 3, 2)
    if L == 1:                                        # p = 1, one MFMA term: the V row itself; lse = the one scaled score
        x = qkv.view(3, 3, 2, 64)
        assert torch.equal(out[:, 0], x[:, 2].reshape(3, 128))
        s = (x[:, 0].double() * x[:, 1].double()).sum(-1) * SCALE
        assert ((lse[:, :, 0].double() - s).abs() <= 2e-6 * s.abs()).all()


# ---- b. softmax hazards ------------------------------------------------------------------------------------------------------------------
# huge_first / huge_last: max_first / max_last at +-128 instead of +-32.  exp(64) = 6e27 is finite in f32, so at +-32 a kernel WITHOUT its max
# subtraction, or with the maximum taken over the wrong columns, still passes (built and measured: both mutants did); exp(128) and exp(256)
# are not (f32 overflows above exp(88.7)), while the float64 and the torch f32 formulation stay finite (they subtract the maximum).
KINDS = ["sharp", "max_first", "max_last", "max_tail_query", "constant_row", "huge_first", "huge_last"]
HAZARD_LENGTHS = [75, 96, 129, 139, 160]             # flash16 five tiles | six tiles, the exchanging backward | long mode 2 | mode 1 | mode 0


def _last_key_tile(L):
    """the last 16-key tile of attn_flash16; the last 32-key tile of attn_long (129: the one column written on the vector ALU)"""
    return 16 * ((L - 1) // 16) if L <= 96 else 32 * ((L - 1) // 32)


def _hazard(kind, L, device='cuda'):
    B, H = 2, 2
    g = torch.Generator(device=device).manual_seed(7 + L)
    x = torch.randn(B, L, 3, H, 64, device=device, generator=g)
    if kind == "sharp":                               # q.k * 0.125 with q, k ~ N(0, 16): scores of standard deviation 16, nearly one-hot rows
        x[:, :, 0:2] *= 4.0
    elif kind != "constant_row":                      # channel 0 puts +32 (huge_*: +128) on the keys of one tile and -32 (-128) on every other key
        a = 32.0 if kind.startswith("huge") else 16.0
        x[:, :, 0, :, 0] = a
        x[:, :, 1, :, 0] = -a
        blk = slice(_last_key_tile(L), L) if kind.endswith("last") else slice(0, 16)
        x[:, blk, 1, :, 0] = a
        if kind == "max_tail_query":                  # the last query alone: -32 on keys 0-15, +32 on every other key
            x[:, L - 1, 0, :, 0] = -16.0
    else:                                             # one query row of zeros: a constant score row, uniform softmax
        x[0, 5, 0] = 0.0
        x[1, L - 1, 0] = 0.0
    return x.view(B, L, 3 * H * 64).contiguous(), torch.randn(B, L, H * 64, device=device, generator=g), H


@pytest.mark.parametrize("L", HAZARD_LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_softmax_hazards_against_float64(kind, L):
    qkv, w, H = _hazard(kind, L)
    t32, f64 = _torch_formulation(qkv, w, H, torch.float32), _torch_formulation(qkv, w, H, torch.float64)
    assert _all_finite(t32) and _all_finite(f64)       # (a condition on the inputs: checked on the CPU for every kind and length beforehand)
    out, g, lse = _kernels(qkv, w, H)
    e_lse = ((lse.double() - f64[2]).abs() / f64[2].abs().clamp_min(1.0)).max().item()
    e_lse_t = ((t32[2].double() - f64[2]).abs() / f64[2].abs().clamp_min(1.0)).max().item()
    print("%s L = %d lse: kernel %.2e torch_f32 %.2e" % (kind, L, e_lse, e_lse_t))
    errs = [(name, _err(a, f64[i]), _err(t32[i], f64[i]), atol) for name, a, i, atol in (("forward", out, 0, 2e-6), ("gradient", g, 1, 5e-6))]
    for name, e_k, e_t, atol in errs:
        print("%s L = %d %s: kernel %.2e torch_f32 %.2e of max|f64|" % (kind, L, name, e_k, e_t))
    assert _all_finite((out, g, lse))
    # the kernel may be as far from float64 as twice the torch f32 formulation on the same inputs, plus the project's absolute terms
    for name, e_k, e_t, atol in errs:
        assert e_k <= 2 * e_t + atol, (kind, L, name, e_k, e_t)
    assert e_lse <= 4e-6                               # relative to |lse| (up to ~80 in the sharp case, ~130 in the huge ones) where that exceeds 1
    if kind == "constant_row":
        v = qkv.view(2, L, 3, H, 64)[:, :, 2].double().mean(1).reshape(2, -1)        # uniform softmax: the mean of V
        for b, row in ((0, 5), (1, L - 1)):
            assert (out[b, row].double() - v[b]).abs().max().item() <= 2e-6 * f64[0].abs().max().item()
            assert (lse[b, :, row].double() - np.log(float(L))).abs().max().item() <= 2e-6


# ---- c. batch and head independence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [35, 75, 96, 129, 139, 160])
def test_every_sample_and_head_computes_alone_what_it_computes_in_a_batch(L):
    """each (sample, head) is one workgroup's private arithmetic: nothing about its result may depend on its neighbours or on H"""
    B, H = 5, 3
    qkv, w = _case(L, B, H)[:2]
    out, g, lse = _kernels(qkv, w, H)
    assert _all_finite((out, g, lse))
    for b in range(B):
        o1, g1, l1 = _kernels(qkv[b:b + 1], w[b:b + 1], H)
        assert torch.equal(o1, out[b:b + 1]) and torch.equal(l1, lse[b:b + 1]) and torch.equal(g1, g[b:b + 1]), ("sample", b)
    x5, g5 = qkv.view(B, L, 3, H, 64), g.view(B, L, 3, H, 64)
    for h in range(H):
        qh = x5[:, :, :, h:h + 1].contiguous().view(B, L, 3 * 64)
        wh = w.view(B, L, H, 64)[:, :, h].contiguous()
        o1, g1, l1 = _kernels(qh, wh, 1)
        assert torch.equal(o1, out.view(B, L, H, 64)[:, :, h]), ("head", h)
        assert torch.equal(l1[:, 0], lse[:, h]), ("head", h)
        assert torch.equal(g1.view(B, L, 3, 64), g5[:, :, :, h]), ("head", h)


# grids below 8 workgroups, grids that are no multiple of 8, and the headline 192 (32 samples x 6 heads)
@pytest.mark.parametrize("B, H", [(1, 1), (1, 2), (7, 1), (1, 12), (32, 6)])
@pytest.mark.parametrize("L", [75, 129])
def test_parity_at_other_grid_geometries(L, B, H):
    _parity(L, B, H)


# ---- d. a non-finite operand stays visible and stays put ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [75, 96, 129, 139])
def test_a_nan_operand_poisons_its_own_sample_and_head_only(L):
    B, H = 3, 2
    qkv, w = _case(L, B, H)[:2]
    clean = _kernels(qkv, w, H)

    def others_are_bit_equal(got):
        for a, c, shape, dims in zip(got, clean, ((B, L, H, 64), (B, L, 3, H, 64), (B, H, L)), ((0, 2), (0, 3), (0, 1))):
            a, c = a.view(shape).movedim(dims, (0, 1)), c.view(shape).movedim(dims, (0, 1))
            for b in range(B):
                for h in range(H):
                    if (b, h) != (1, 0):
                        assert torch.equal(a[b, h], c[b, h]), (b, h)

    bad = qkv.clone()
    bad.view(B, L, 3, H, 64)[1, 3, 2, 0, 7] = float('nan')           # V[row 3][channel 7] of (sample 1, head 0)
    got = _kernels(bad, w, H)
    assert torch.isnan(got[0].view(B, L, H, 64)[1, :, 0, 7]).all()   # p[q][3] * NaN for every query q, p = 0 included
    others_are_bit_equal(got)

    bad = qkv.clone()
    bad.view(B, L, 3, H, 64)[1, 3, 1, 0, 7] = float('nan')           # K[row 3][channel 7]: score column 3 of every query
    got = _kernels(bad, w, H)
    assert not torch.isfinite(got[0].view(B, L, H, 64)[1, :, 0]).any()
    assert not torch.isfinite(got[2][1, 0]).any()
    others_are_bit_equal(got)


# ---- e. rows behind the last token -------------------------------------------------------------------------------------------------------
# one live row in the last 16-row tile (17, 65, 81), in the last 32-row tile (97, 129, 145); one tail row in modes 2 (129) and 1 (133)
@pytest.mark.parametrize("L", [17, 65, 81, 97, 129, 133, 145])
def test_rows_behind_the_last_token_are_never_read(L):
    B, H = 2, 2
    g = torch.Generator(device='cuda').manual_seed(11 + L)
    n, nw = B * L * 3 * H * 64, B * L * H * 64
    big = torch.full((n + 64 * 3 * H * 64,), float('nan'), device='cuda')       # 64 rows: more than one full padded tile of either family
    bigw = torch.full((nw + 64 * H * 64,), float('nan'), device='cuda')
    big[:n] = torch.randn(n, device='cuda', generator=g)
    bigw[:nw] = torch.randn(nw, device='cuda', generator=g)
    qkv, w = big[:n].view(B, L, 3 * H * 64), bigw[:nw].view(B, L, H * 64)
    assert qkv.is_contiguous() and qkv.data_ptr() == big.data_ptr()
    got = _kernels(qkv, w, H)
    exact = _kernels(qkv.clone(), w.clone(), H)
    for a, b in zip(got, exact):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


# ---- f. stale LDS ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tenant():
    """fill(value) launches the library's own kernels with every operand = value over the whole chip: forward and backward at L = 160,
    H = 1, B = 1024 -- four workgroups per CU of ~140 KB of LDS each, so every CU's LDS is rewritten with what such a tenant leaves
    (value, or functions of it).  The buffers live for the module: 126 MB of qkv, 2 x 42 MB of ctx / d_ctx."""
    B, L = 1024, 160
    qkv = torch.empty(B, L, 3 * 64, device='cuda')
    ctx, d_ctx = torch.empty(B, L, 64, device='cuda'), torch.empty(B, L, 64, device='cuda')
    lse = torch.empty(B, 1, L, device='cuda')

    def fill(value):
        for t in (qkv, ctx, d_ctx, lse):
            t.fill_(value)
        ops.attn_fwd(qkv, B, L, 1, SCALE)
        ops.attn_bwd(qkv, ctx, d_ctx, lse, B, L, 1, SCALE)

    return fill


@pytest.mark.parametrize("L", [35, 75, 96, 97, 129, 132, 133, 139, 144, 160])
def test_stale_lds_does_not_leak_into_results(L, tenant):
    """Evidence, not proof.  The LDS is not cleared between workgroups, and these kernels rely on regions they fill themselves: zero rows
    [valid, R) of stage_block, zero strip columns [L, 160), every row of PT / DS, strip rows that are never written and feed only output
    rows that are not stored.  The case runs right behind a tenant that left NaN in every CU's LDS, then behind one that left zeros (and
    1 / 160): a result that depended on what was there before would be non-finite in the first run or differ between the two.  A
    workgroup's LDS base is not under the test's control, so a clean pass does not prove the absence of such a dependence.  Only NaN
    VALUES are fed, never addresses: NaN arithmetic does not fault."""
    B, H = 32, 6
    qkv, w = _case(L, B, H)[:2]
    tenant(float('nan'))
    after_nan = _kernels(qkv, w, H)                   # (same stream, nothing in between but the allocation of the outputs)
    tenant(0.0)
    after_zero = _kernels(qkv, w, H)
    for a, b in zip(after_nan, after_zero):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


# ---- g. determinism and graph replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [75, 96, 129, 139])
def test_two_runs_give_the_same_bits(L):
    qkv, w, H = _case(L)[:3]
    first = [t.clone() for t in _kernels(qkv, w, H)]
    for a, b in zip(first, _kernels(qkv, w, H)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("L", [75, 129])
def test_captured_forward_and_backward_replay_the_eager_bits_without_a_memset(L):
    qkv, w, H = _case(L)[:3]
    eager = [t.clone() for t in _kernels(qkv, w, H)]
    assert not _memsets(lambda: _kernels(qkv, w, H))       # (what a capture would turn into memset nodes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _kernels(qkv, w, H)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _kernels(qkv, w, H)
    for _ in range(3):
        for t in captured:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(a, b)


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch(monkeypatch):
    B, L, H = 2, 35, 2
    qkv, w = _case(L, B, H)[:2]
    out, lse = ops.attn_fwd(qkv, B, L, H, SCALE)
    ops.attn_bwd(qkv, out, w, lse, B, L, H, SCALE)     # the good arguments pass

    def no_launch(*a, **k):
        pytest.fail("a kernel was launched on a bad argument: %r" % (a[1],))

    monkeypatch.setattr(ops, "_call", no_launch)
    shifted = torch.zeros(qkv.numel() + 1, device='cuda')[1:].view(B, L, 3 * H * 64)      # contiguous, one float into its storage
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    shifted_w = torch.zeros(w.numel() + 1, device='cuda')[1:].view(B, L, H * 64)
    bad_bwd = {
        "lse of the wrong shape": (qkv, out, w, lse[:, :, :-1].contiguous()),
        "d_ctx of the wrong shape": (qkv, out, w[:, :-1].contiguous(), lse),
        "float64 ctx": (qkv, out.double(), w, lse),
        "transposed d_ctx": (qkv, out, w.transpose(1, 2).contiguous().transpose(1, 2), lse),
        "qkv at a one-float offset": (shifted, out, w, lse),
        "d_ctx at a one-float offset": (qkv, out, shifted_w, lse),
        "ctx at a one-float offset": (qkv, shifted_w, w, lse),
        "qkv of the wrong size": (qkv[:, :-1].contiguous(), out, w, lse),
    }
    assert not bad_bwd["transposed d_ctx"][2].is_contiguous() and bad_bwd["transposed d_ctx"][2].shape == w.shape
    for name, args in bad_bwd.items():
        with pytest.raises(RuntimeError):
            ops.attn_bwd(*args, B, L, H, SCALE)
            print("no error for", name)
    for bad in (shifted, qkv[:, :-1].contiguous(), qkv.double(), qkv.transpose(0, 1)):
        with pytest.raises(RuntimeError):
            ops.attn_fwd(bad, B, L, H, SCALE)
