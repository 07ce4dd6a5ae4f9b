"""The cross-attention kernels (csrc/attn_stream.hip: one streaming family for 1 <= Lq, Lk <= ATTN_MAX_L), their autograd node and their
first users, models.upp_layers.CrossAttention and DecoderBlock, on the GPU: parity of ctx, lse, d_q, d_k, d_v with the torch formulation
under float64 arbitration, strided operands (bit-equal to contiguous copies and, for Lq = Lk beyond 160, to ops.attn_fwd / attn_bwd on the
same packed qkv), the hazards of a softmax with the hot keys in the first and in the last 64-key block, independence of every (sample,
head, query block), confinement of a NaN, rows behind the last token, stale LDS, determinism and graph replay, and the modules against
the reference's own outputs (tests/golden/decoder_block.npz) and against their float64 torch formulation.

Bounds: ctx, lse and the three gradients rtol 1e-5, atol 2e-6 max|ref| against the torch f32 formulation where that is itself inside the
bound against float64, else max|kernel - f64| <= 2 max|torch_f32 - f64| + 2e-6 max|f64| (tests/_attention_reference._check_against);
hazards e_kernel <= 2 e_torch_f32 + atol of max|f64| (2e-6 forward, 5e-6 gradients), lse within 4e-6 of max(|lse|, 1); the fixture 1e-5 of
each output's max; module gradients the project's gradient bound (rtol 2e-5, atol 5e-6 max|ref|) through _check_against.

Measured on MI355X, max|x - f64| / max|f64| of (kernel, torch f32).  Parity, the worst of ctx | lse | d_q | d_k | d_v over the eleven shapes:
1.43e-6, 1.49e-6 | 3.9e-7, 3.2e-7 | 1.36e-6, 1.70e-6 | 1.93e-6, 1.61e-6 | 2.07e-6, 1.88e-6 (the largest at 2048 x 64 and 64 x 2048); the
torch f32 formulation stayed inside the bound against float64 everywhere, so the bound against it applied and the arbitration never had
to.  With one key (1 x 1, 193 x 1) ctx is the V row bit for bit and d_q = d_k = 0 exactly.  Hazards, ctx | the three gradients as one array:
    kind           (65, 129)                                  (129, 65)                                  (224, 128)
    sharp          3.5e-6, 2.7e-6 | 3.1e-6, 3.3e-6            4.5e-6, 4.2e-6 | 7.5e-6, 4.8e-6            4.8e-6, 3.7e-6 | 2.9e-6, 3.7e-6
    max_first      1.36e-5, 1.19e-5 | 7.9e-6, 6.0e-6          7.8e-6, 8.9e-6 | 7.1e-6, 6.7e-6            8.9e-6, 9.0e-6 | 9.4e-6, 9.1e-6
    max_last       0, 0 | 2.0e-6, 2.3e-7                      0, 0 | 1.45e-6, 2.1e-7                     6.8e-6, 7.4e-6 | 6.8e-6, 8.0e-6
    constant_row   4.8e-7, 5.2e-7 | 6.2e-7, 4.6e-7            3.9e-7, 3.5e-7 | 4.6e-7, 4.8e-7            5.2e-7, 5.5e-7 | 5.1e-7, 4.0e-7
    huge_first     6.6e-5, 5.6e-5 | 2.1e-5, 2.2e-5            3.3e-5, 2.7e-5 | 2.4e-5, 2.8e-5            3.4e-5, 3.2e-5 | 3.5e-5, 3.5e-5
    huge_last      0, 0 | 4.1e-6, 2.3e-7                      0, 0 | 2.9e-6, 2.1e-7                      4.2e-5, 4.0e-5 | 2.5e-5, 2.6e-5
max_last / huge_last with Lk = 129 or 65 put the whole softmax on the one key of the last block: ctx is that V row exactly, the true d_q and
d_k are 0 (float64: 1e-23 and below), and the kernels' are the rounding of dP - delta times the 16 / 32 in channel 0 of K -- 1.45e-6 ... 4.1e-6 of
the gradients' maximum against the bound 2 x 2.3e-7 + 5e-6.  lse: at most 7.7e-7 (torch f32: 7.8e-7) of max(|lse|, 1) in every hazard case.

Mutants, built from scratch copies and run once each (never committed): (1) stage_rows leaving rows >= valid unwritten fails parity at
1 x 1, 65 x 63, 63 x 65, 1 x 193 and 193 x 1, rows behind the last token at 65 x 1 and stale LDS at 3 x 5; (2) the single-key-block row sum
never taken (delta from ctx at every Lk) fails the exact zeros of d_q / d_k at 1 x 1 and 193 x 1 and nothing else; (3) the forward not
rescaling O when the running maximum moves fails parity at six shapes with more than one key block, both bit comparisons with
attn_stream.hip and the sharp, max_last, constant_row and huge_last hazards at all three shapes -- and passes max_first / huge_first,
where the maximum is found in the first block and never moves."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import _decoder_block_case as case
import _seeded
from _attention_reference import SCALE, _check_against, _err, _memsets
from conftest import ROOT
from models import upp_layers
from upp_hip import functional as HF, ops

pytestmark = pytest.mark.gpu

NAMES = ("ctx", "lse", "d_q", "d_k", "d_v")


def _torch_formulation(q, k, v, w, H, dtype):
    """reference models/Transformer.py:144-152 and its autograd -> (ctx, lse, d_q, d_k, d_v)"""
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    x = [t.detach().to(dtype).contiguous().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = (t.view(B, L, H, 64).permute(0, 2, 1, 3) for t, L in zip(x, (Lq, Lk, Lk)))
    s = (qh @ kh.transpose(-2, -1)) * SCALE
    out = (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, Lq, H * 64)
    (out * w.to(dtype)).sum().backward()
    return out.detach(), torch.logsumexp(s.detach(), -1), x[0].grad, x[1].grad, x[2].grad


def _kernels(q, k, v, w, H):
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    ctx, lse = ops.xattn_fwd(q, k, v, B, Lq, Lk, H, SCALE)
    return (ctx, lse) + ops.xattn_bwd(q, k, v, ctx, w, lse, B, Lq, Lk, H, SCALE)


def _operands(B, H, Lq, Lk, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed + 1000003 * Lq + 1009 * Lk + 10 * B + H)
    q, w = (torch.randn(B, Lq, H * 64, device='cuda', generator=g) for _ in range(2))
    k, v = (torch.randn(B, Lk, H * 64, device='cuda', generator=g) for _ in range(2))
    return q, k, v, w


@functools.lru_cache(maxsize=None)
def _case(B, H, Lq, Lk):
    q, k, v, w = _operands(B, H, Lq, Lk)
    return (q, k, v, w), _torch_formulation(q, k, v, w, H, torch.float32), _torch_formulation(q, k, v, w, H, torch.float64)


def _all_finite(ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def _equal(a, b, what=""):
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), (what, name)


# ---- a. parity against torch f32 with float64 arbitration ---------------------------------------------------------------------------------
SHAPES = [(2, 2, 1, 1), (1, 1, 64, 64), (2, 3, 65, 63), (2, 2, 63, 65), (1, 2, 1, 193), (1, 2, 193, 1), (2, 6, 224, 128), (1, 1, 129, 320),
          (1, 2, 2048, 64), (1, 2, 64, 2048), (7, 1, 65, 65)]


@pytest.mark.parametrize("B, H, Lq, Lk", SHAPES)
def test_parity_with_the_torch_formulation_and_float64(B, H, Lq, Lk):
    (q, k, v, w), t32, f64 = _case(B, H, Lq, Lk)
    got = _kernels(q, k, v, w, H)
    print("B = %d, H = %d, Lq = %d, Lk = %d" % (B, H, Lq, Lk))
    assert _all_finite(got)
    for i, name in enumerate(NAMES):
        if Lk == 1 and name in ("d_q", "d_k"):
            # one key: P = 1, dS = P (dP - sum_j P dP) = 0 exactly, whatever dP is
            print("%s: kernel max |x| = %.2e (true value 0)" % (name, got[i].abs().max().item()))
            assert not got[i].any(), name
            continue
        _check_against(name, got[i], t32[i], f64[i], 1e-5, 2e-6)
    if Lk == 1:
        # p = 1, one MFMA term per channel, l = 1: the context of every query is the one V row, bit for bit
        assert torch.equal(got[0], v.expand(B, Lq, H * 64))


# ---- b. strided operands ------------------------------------------------------------------------------------------------------------------
def test_views_of_a_packed_qkv_and_of_a_packed_kv_give_the_bits_of_contiguous_copies():
    B, H, L = 2, 3, 70
    g = torch.Generator(device='cuda').manual_seed(5)
    qkv = torch.randn(B, L, 3, H * 64, device='cuda', generator=g)
    w = torch.randn(B, L, H * 64, device='cuda', generator=g)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    assert not k.is_contiguous() and k.stride(1) == 3 * H * 64
    _equal(_kernels(q, k, v, w, H), _kernels(q.contiguous(), k.contiguous(), v.contiguous(), w, H), "packed qkv")
    Lq, Lk = 70, 130
    kv = torch.randn(B, Lk, 2 * H * 64, device='cuda', generator=g)
    k, v = kv[:, :, :H * 64], kv[:, :, H * 64:]
    assert v.data_ptr() == k.data_ptr() + 4 * H * 64 and v.stride(1) == 2 * H * 64
    _equal(_kernels(q, k, v, w, H), _kernels(q.contiguous(), k.contiguous(), v.contiguous(), w, H), "packed [k|v]")
    # through the autograd node the views are passed on as they are
    assert HF._xattn_view(k) is k and HF._xattn_view(q) is q


@pytest.mark.parametrize("L", [161, 257])
def test_equal_lengths_give_the_bits_of_the_self_attention_kernels(L):
    """The block walk and the accumulation order are those of attn_stream.hip (which serves L > 160): on views of one packed qkv the two
    families must agree bit for bit.  A difference here is a difference of order: the kernel is wrong, not the test."""
    B, H = 2, 3
    g = torch.Generator(device='cuda').manual_seed(L)
    qkv = torch.randn(B, L, 3 * H * 64, device='cuda', generator=g)
    w = torch.randn(B, L, H * 64, device='cuda', generator=g)
    ctx, lse = ops.attn_fwd(qkv, B, L, H, SCALE)
    d_qkv = ops.attn_bwd(qkv, ctx, w, lse, B, L, H, SCALE).view(B, L, 3, H * 64)
    x = qkv.view(B, L, 3, H * 64)
    got = _kernels(x[:, :, 0], x[:, :, 1], x[:, :, 2], w, H)
    _equal(got, (ctx, lse, d_qkv[:, :, 0], d_qkv[:, :, 1], d_qkv[:, :, 2]), L)


# ---- c. softmax hazards against float64 ---------------------------------------------------------------------------------------------------
# huge_first / huge_last: +-128 instead of +-32 -- exp(128) overflows f32, so a kernel without its max subtraction, or with the running
# maximum rescaled wrongly across key blocks, cannot pass them (tests/test_gpu_attention_short.py)
KINDS = ["sharp", "max_first", "max_last", "constant_row", "huge_first", "huge_last"]
HAZARD_SHAPES = [(65, 129), (129, 65), (224, 128)]


def _hazard(kind, Lq, Lk, device='cuda'):
    B, H = 2, 2
    g = torch.Generator(device=device).manual_seed(7 + 1000 * Lq + Lk)
    q = torch.randn(B, Lq, H, 64, device=device, generator=g)
    k = torch.randn(B, Lk, H, 64, device=device, generator=g)
    v = torch.randn(B, Lk, H, 64, device=device, generator=g)
    if kind == "sharp":                               # q.k * 0.125 with q, k ~ N(0, 16): scores of standard deviation 16, nearly one-hot rows
        q *= 4.0
        k *= 4.0
    elif kind != "constant_row":                      # channel 0 puts +32 (huge_*: +128) on the keys of one 64-key block, -32 (-128) on every other key
        a = 32.0 if kind.startswith("huge") else 16.0
        q[:, :, :, 0] = a
        k[:, :, :, 0] = -a
        blk = slice(64 * ((Lk - 1) // 64), Lk) if kind.endswith("last") else slice(0, 64)
        k[:, blk, :, 0] = a
    else:                                             # one query row of zeros: a constant score row, uniform softmax
        q[0, 5] = 0.0
        q[1, Lq - 1] = 0.0
    w = torch.randn(B, Lq, H * 64, device=device, generator=g)
    return q.view(B, Lq, H * 64), k.view(B, Lk, H * 64), v.view(B, Lk, H * 64), w, H


@pytest.mark.parametrize("Lq, Lk", HAZARD_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_softmax_hazards_against_float64(kind, Lq, Lk):
    q, k, v, w, H = _hazard(kind, Lq, Lk)
    t32, f64 = _torch_formulation(q, k, v, w, H, torch.float32), _torch_formulation(q, k, v, w, H, torch.float64)
    assert _all_finite(t32) and _all_finite(f64)       # (a condition on the inputs: checked on the CPU for every kind and shape beforehand)
    got = _kernels(q, k, v, w, H)
    e_lse = ((got[1].double() - f64[1]).abs() / f64[1].abs().clamp_min(1.0)).max().item()
    e_lse_t = ((t32[1].double() - f64[1]).abs() / f64[1].abs().clamp_min(1.0)).max().item()
    print("%s (%d, %d) lse: kernel %.2e torch_f32 %.2e" % (kind, Lq, Lk, e_lse, e_lse_t))
    # The gradients are judged as the existing test judges d_qkv: as one array (max_last / huge_last with a one-key last block put the
    # whole softmax on one key, so that the true d_q and d_k are ~0 and an error relative to their own maximum means nothing), and each
    # one alone wherever its float64 maximum is at least 1e-3 of the largest of the three -- a condition on the reference only.
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts[2:]])          # noqa: E731
    errs = [("ctx", _err(got[0], f64[0]), _err(t32[0], f64[0]), 2e-6), ("gradients", _err(flat(got), flat(f64)), _err(flat(t32), flat(f64)), 5e-6)]
    top = flat(f64).abs().max().item()
    for i in (2, 3, 4):
        if f64[i].abs().max().item() >= 1e-3 * top:
            errs.append((NAMES[i], _err(got[i], f64[i]), _err(t32[i], f64[i]), 5e-6))
        else:
            print("%s (%d, %d) %s: max|f64| %.2e of the gradients' %.2e, judged with them" % (kind, Lq, Lk, NAMES[i], f64[i].abs().max().item(), top))
    for name, e_k, e_t, atol in errs:
        print("%s (%d, %d) %s: kernel %.2e torch_f32 %.2e of max|f64|" % (kind, Lq, Lk, name, e_k, e_t))
    assert _all_finite(got)
    for name, e_k, e_t, atol in errs:
        assert e_k <= 2 * e_t + atol, (kind, Lq, Lk, name, e_k, e_t)
    assert e_lse <= 4e-6
    if kind == "constant_row":
        mean_v = v.double().mean(1)                                                   # uniform softmax: the mean of V
        for b, row in ((0, 5), (1, Lq - 1)):
            assert (got[0][b, row].double() - mean_v[b]).abs().max().item() <= 2e-6 * f64[0].abs().max().item()
            assert (got[1][b, :, row].double() - np.log(float(Lk))).abs().max().item() <= 2e-6


# ---- d. sample, head and query-block independence -----------------------------------------------------------------------------------------
def test_every_sample_head_and_query_block_computes_alone_what_it_computes_in_a_batch():
    B, H, Lq, Lk = 3, 2, 130, 70
    q, k, v, w = _operands(B, H, Lq, Lk)
    full = _kernels(q, k, v, w, H)
    assert _all_finite(full)
    heads = lambda t, L: t.view(B, L, H, 64)          # noqa: E731
    for b in range(B):
        for h in range(H):
            alone = _kernels(*(heads(t, L)[b:b + 1, :, h].contiguous() for t, L in ((q, Lq), (k, Lk), (v, Lk), (w, Lq))), 1)
            want = (heads(full[0], Lq)[b:b + 1, :, h], full[1][b:b + 1, h:h + 1], heads(full[2], Lq)[b:b + 1, :, h],
                    heads(full[3], Lk)[b:b + 1, :, h], heads(full[4], Lk)[b:b + 1, :, h])
            _equal(alone, want, (b, h))
    first = _kernels(q[:, :64].contiguous(), k, v, w[:, :64].contiguous(), H)        # the first query block alone: Lq = 64
    assert torch.equal(first[0], full[0][:, :64]) and torch.equal(first[1], full[1][:, :, :64]) and torch.equal(first[2], full[2][:, :64])


# ---- e. a NaN operand stays visible and stays put -----------------------------------------------------------------------------------------
def test_a_nan_operand_poisons_its_own_sample_and_head_only():
    B, H, Lq, Lk = 3, 2, 75, 129
    q, k, v, w = _operands(B, H, Lq, Lk)
    clean = _kernels(q, k, v, w, H)

    def others_are_bit_equal(got):
        for name, a, c in zip(NAMES, got, clean):
            if name == "lse":
                a, c = a.unsqueeze(-1), c.unsqueeze(-1)                              # (B, H, Lq, 1)
            else:
                a, c = a.view(B, -1, H, 64).transpose(1, 2), c.view(B, -1, H, 64).transpose(1, 2)
            for b in range(B):
                for h in range(H):
                    if (b, h) != (1, 0):
                        assert torch.equal(a[b, h], c[b, h]), (name, b, h)

    bad = v.clone()
    bad.view(B, Lk, H, 64)[1, 3, 0, 7] = float('nan')                # V[row 3][channel 7] of (sample 1, head 0)
    got = _kernels(q, k, bad, w, H)
    assert torch.isnan(got[0].view(B, Lq, H, 64)[1, :, 0, 7]).all()  # p[q][3] * NaN for every query q
    others_are_bit_equal(got)

    bad = k.clone()
    bad.view(B, Lk, H, 64)[1, 3, 0, 7] = float('nan')                # K[row 3][channel 7]: score column 3 of every query
    got = _kernels(q, bad, v, w, H)
    assert not torch.isfinite(got[0].view(B, Lq, H, 64)[1, :, 0]).any()
    assert not torch.isfinite(got[1][1, 0]).any()
    others_are_bit_equal(got)


# ---- f. rows behind the last token --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq, Lk", [(1, 65), (65, 1), (129, 97)])
def test_rows_behind_the_last_token_are_never_read(Lq, Lk):
    B, H = 2, 2
    g = torch.Generator(device='cuda').manual_seed(11 + 1000 * Lq + Lk)

    def carved(L):
        n = B * L * H * 64
        big = torch.full((n + 64 * H * 64,), float('nan'), device='cuda')           # 64 rows: a whole block behind the last one
        big[:n] = torch.randn(n, device='cuda', generator=g)
        t = big[:n].view(B, L, H * 64)
        assert t.data_ptr() == big.data_ptr()
        return t

    q, k, v, w = carved(Lq), carved(Lk), carved(Lk), carved(Lq)
    got = _kernels(q, k, v, w, H)
    exact = _kernels(q.clone(), k.clone(), v.clone(), w.clone(), H)
    assert _all_finite(got)
    _equal(got, exact)


# ---- g. stale LDS -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tenant():
    """fill(value) launches the cross-attention kernels with every operand = value over the whole chip: 1024 forward workgroups (66 KB of
    LDS each) and 2 x 1024 backward ones (98 KB each), so every CU's LDS is rewritten with what such a tenant leaves."""
    B, L = 1024, 64
    q, k, v, ctx, d_ctx = (torch.empty(B, L, 64, device='cuda') for _ in range(5))
    lse = torch.empty(B, 1, L, device='cuda')

    def fill(value):
        for t in (q, k, v, ctx, d_ctx, lse):
            t.fill_(value)
        ops.xattn_fwd(q, k, v, B, L, L, 1, SCALE)
        ops.xattn_bwd(q, k, v, ctx, d_ctx, lse, B, L, L, 1, SCALE)

    return fill


@pytest.mark.parametrize("Lq, Lk", [(3, 5), (70, 130)])
def test_stale_lds_does_not_leak_into_results(Lq, Lk, tenant):
    """Evidence, not proof (tests/test_gpu_attention_short.py): the kernels rely on LDS regions they fill themselves -- zero rows
    [valid, 64) of every staged block, every entry of the P / dS strips.  Only values are fed, never addresses."""
    B, H = 32, 6
    q, k, v, w = _operands(B, H, Lq, Lk)
    before = _kernels(q, k, v, w, H)
    tenant(1e30)
    after_huge = _kernels(q, k, v, w, H)
    tenant(float('nan'))
    after_nan = _kernels(q, k, v, w, H)
    assert _all_finite(before)
    _equal(after_huge, before, "behind 1e30")
    _equal(after_nan, before, "behind NaN")


# ---- h. determinism and capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq, Lk", [(224, 128), (37, 200)])
def test_two_runs_give_the_same_bits(Lq, Lk):
    q, k, v, w = _operands(2, 3, Lq, Lk)
    first = [t.clone() for t in _kernels(q, k, v, w, 3)]
    _equal(first, _kernels(q, k, v, w, 3))


def test_captured_forward_and_backward_replay_the_eager_bits_without_a_memset():
    H = 3
    q, k, v, w = _operands(2, H, 224, 128)
    eager = [t.clone() for t in _kernels(q, k, v, w, H)]
    assert not _memsets(lambda: _kernels(q, k, v, w, H))       # (what a capture would turn into memset nodes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _kernels(q, k, v, w, H)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _kernels(q, k, v, w, H)
    for _ in range(3):
        for t in captured:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        _equal(captured, eager)


# ---- i. autograd and modules --------------------------------------------------------------------------------------------------------------
def test_the_autograd_node_returns_the_kernels_gradients():
    B, H, Lq, Lk = 2, 3, 70, 130
    q, k, v, w = _operands(B, H, Lq, Lk)
    want = _kernels(q, k, v, w, H)
    x = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = HF.cross_attention(*x, H, SCALE)
    (out * w).sum().backward()
    _equal((out.detach(), want[1], x[0].grad, x[1].grad, x[2].grad), want)
    # a packed [k|v] product: the views reach the kernels as they are and the gradient comes back through the slices
    kv = torch.cat([k, v], dim=-1).requires_grad_(True)
    qx = q.clone().requires_grad_(True)
    out = HF.cross_attention(qx, kv[:, :, :H * 64], kv[:, :, H * 64:], H, SCALE)
    (out * w).sum().backward()
    assert torch.equal(out.detach(), want[0]) and torch.equal(qx.grad, want[2]) and torch.equal(kv.grad, torch.cat([want[3], want[4]], dim=-1))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "decoder_block.npz"))


def _modules(device='cuda'):
    xattn = _seeded.fill(upp_layers.CrossAttention(case.DIM, case.DIM, num_heads=case.HEADS)).eval().to(device)
    block = _seeded.fill(upp_layers.DecoderBlock(case.DIM, case.HEADS)).eval().to(device)
    return xattn, block


def test_modules_equal_the_reference_fixture(golden):
    q, v, self_idx, cross_idx = (t.cuda() for t in case.inputs())
    xattn, block = _modules()
    assert xattn.fusable(q, v)
    HF._declined.clear()
    with torch.no_grad():
        got = {"xattn": xattn(q, v), "plain": block(q, v), "knn": block(q, v, self_idx, cross_idx)}
    assert not HF._declined, HF._declined
    for name, t in got.items():
        want = torch.from_numpy(golden[name])
        e = ((t.cpu() - want).abs().max() / want.abs().max()).item()
        print("decoder-block fixture, fused path: %s %.2e of the output's max" % (name, e))
        assert e <= 1e-5, (name, e)


def _block_grads(block, q, v, self_idx, cross_idx, w):
    block.zero_grad()
    q, v = q.clone().requires_grad_(True), v.clone().requires_grad_(True)
    out = block(q, v, self_idx, cross_idx)
    (out * w).sum().backward()
    grads = {"d_q": q.grad, "d_v": v.grad}
    grads.update({n: p.grad for n, p in block.named_parameters()})
    return out.detach(), grads


def test_decoder_block_gradients_against_its_float64_torch_formulation():
    q, v, self_idx, cross_idx = case.inputs()
    w = torch.randn(q.shape, generator=torch.Generator().manual_seed(3))
    block = _modules('cpu')[1]
    out32, g32 = _block_grads(block, q, v, self_idx, cross_idx, w)
    b64 = copy.deepcopy(block).double()
    out64, g64 = _block_grads(b64, q.double(), v.double(), self_idx, cross_idx, w.double())
    fused = copy.deepcopy(block).cuda()
    HF._declined.clear()
    out, g = _block_grads(fused, q.cuda(), v.cuda(), self_idx.cuda(), cross_idx.cuda(), w.cuda())
    assert not HF._declined, HF._declined
    assert set(g) == set(g64) and len(g) == 2 + 28 and all(t is not None for t in g.values())
    _check_against("forward", out.cpu(), out32, out64, 1e-5, 2e-6)
    for name in sorted(g):
        _check_against(name, g[name].cpu(), g32[name], g64[name], 2e-5, 5e-6)


def test_fused_decoder_block_launches_no_library_gemm_softmax_or_topk():
    q, v, self_idx, cross_idx = (t.cuda() for t in case.inputs())
    w = torch.randn(q.shape, device='cuda')
    block = _modules()[1]
    _block_grads(block, q, v, self_idx, cross_idx, w)                   # (warm-up: caches, lazy initialisation)
    HF._declined.clear()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        _block_grads(block, q, v, self_idx, cross_idx, w)
        torch.cuda.synchronize()
    assert not HF._declined, HF._declined
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    print("\n".join(names))
    for n in names:
        assert "Cijk_" not in n and "gemm" not in n.lower() and "softmax" not in n.lower() and "topk" not in n.lower(), n
    for frag in ("xattn_fwd_kernel", "xattn_bwd_kv_kernel", "xattn_bwd_q_kernel", "ec_"):
        assert any(frag in n for n in names), frag


def test_declined_list_is_empty_when_fused_and_names_the_site_otherwise():
    q, v, self_idx, cross_idx = (t.cuda() for t in case.inputs())
    block = _modules()[1]
    HF._declined.clear()
    with torch.no_grad():
        block(q, v, self_idx, cross_idx)
    assert not HF._declined, HF._declined
    narrow = _seeded.fill(upp_layers.DecoderBlock(64, 2)).eval().cuda()             # head_dim 32
    with torch.no_grad():
        out = narrow(q[:, :, :64].contiguous(), v[:, :, :64].contiguous(), self_idx, cross_idx)
    assert out.shape == (case.B, case.NQ, 64) and torch.isfinite(out).all()
    sites = [what for what, why in HF._declined]
    assert any(what.startswith("CrossAttention") for what in sites), HF._declined
    HF._declined.clear()
