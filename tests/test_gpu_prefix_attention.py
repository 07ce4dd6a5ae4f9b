"""The denoising-query (prefix-visibility) attention kernels (csrc/attn_stream.hip) and their autograd node on the GPU: query rows
< split_q see the keys < split_k, the other rows see every key.  Parity of ctx, lse, d_q, d_k, d_v with the torch masked formulation
(the reference's masked_fill(-finfo.max) + softmax, models/Transformer_utils.py:100-120) under float64 arbitration; the forward's bits
against ops.xattn_fwd on the two row groups taken apart; the unmasked ends of both split ranges against ops.xattn_fwd / xattn_bwd bit
for bit; a prefix that sees one key; a NaN in a hidden key row; views of a packed qkv; determinism, graph replay without a memset; the
autograd node.

Bounds (tests/_attention_reference._check_against): rtol 1e-5, atol 2e-6 max|ref| against the torch f32 formulation where that is itself
inside the bound against float64, else max|kernel - f64| <= 2 max|torch_f32 - f64| + 2e-6 max|f64|.

Shapes are (B, H, Lq, Lk, split_q, split_k): both splits inside the first block (40), on a block edge (96 / 32, 128 / 64), just past one
(130 / 66, 193 / 129: a straddling query block and a straddling key block), unequal lengths with the splits in different blocks
(70 x 130), a prefix that sees one key (129 x 65), a prefix that sees exactly the first key block while the denoising rows straddle
nothing (65 x 129) and AdaPoinTr's own 512 + 64.

Measured on MI355X, max|x - f64| / max|f64| of (kernel, torch f32), the worst over the nine shapes: ctx 9.0e-7, 8.4e-7 | lse 1.4e-7,
1.2e-7 | d_q 8.5e-7, 7.1e-7 | d_k 1.22e-6, 1.08e-6 | d_v 8.6e-7, 8.6e-7 (the largest at 512 + 64 tokens, ctx at 193); the torch f32
formulation stayed inside the bound against float64 everywhere, so the bound against it applied and the arbitration never had to.  The
one-key prefix (129 x 65, split_k = 1): ctx of the 128 prefix rows is the V row bit for bit, their lse is 3.3e-7 of the float64 score and
their d_q is exactly 0.

Mutants, built from scratch copies and run once each (never committed): (1) the backward kernels ignoring the mask (only the shortened
walks left) fail parity at the seven shapes whose splits are not both on a block edge and the single-block one-key case, and pass
128 / 64 and 512 + 64, where the walks alone are the mask; (2) the single-key-block row sum taken only for Lk <= 64, not per query block,
fails the exact zero of d_q at 129 x 65 with split_k = 1 and the parity of that shape (the rounding of dP - delta on rows whose true
gradient is 0), and nothing else; (3) the forward deciding visibility per query block instead of per row fails parity and the
forward-bit comparison at the five shapes with a straddling query block, the single-block one-key case and the hidden NaN."""
import functools

import pytest
import torch

from _attention_reference import SCALE, _check_against, _err, _memsets
from upp_hip import functional as HF, ops

pytestmark = pytest.mark.gpu

NAMES = ("ctx", "lse", "d_q", "d_k", "d_v")
SHAPES = [(2, 2, 40, 40, 32, 32), (1, 2, 96, 96, 32, 32), (2, 1, 128, 128, 64, 64), (2, 3, 130, 130, 66, 66), (1, 2, 193, 193, 129, 129),
          (2, 2, 70, 130, 6, 65), (1, 2, 129, 65, 128, 1), (1, 1, 65, 129, 65, 64), (1, 2, 576, 576, 512, 512)]


def _torch_formulation(q, k, v, w, H, sq, sk, dtype):
    """the reference's masked attention and its autograd on separate q, k, v -> (ctx, lse over the visible keys, d_q, d_k, d_v)"""
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    x = [t.detach().to(dtype).contiguous().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = (t.view(B, L, H, 64).permute(0, 2, 1, 3) for t, L in zip(x, (Lq, Lk, Lk)))
    mask = torch.zeros(Lq, Lk, device=q.device)
    mask[:sq, sk:] = 1.
    s = (qh @ kh.transpose(-2, -1)) * SCALE
    s = s.masked_fill(mask > 0, -torch.finfo(s.dtype).max)
    out = (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, Lq, H * 64)
    (out * w.to(dtype)).sum().backward()
    lse = torch.logsumexp(s.detach().masked_fill(mask > 0, -float('inf')), -1)
    return out.detach(), lse, x[0].grad, x[1].grad, x[2].grad


def _kernels(q, k, v, w, H, sq, sk):
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    ctx, lse = ops.xattn_prefix_fwd(q, k, v, B, Lq, Lk, H, SCALE, sq, sk)
    return (ctx, lse) + ops.xattn_prefix_bwd(q, k, v, ctx, w, lse, B, Lq, Lk, H, SCALE, sq, sk)


def _unmasked(q, k, v, w, H):
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
def _case(B, H, Lq, Lk, sq, sk):
    """operands, the torch f32 and f64 results and the kernels' results of one shape: computed once, shared, never written to"""
    q, k, v, w = _operands(B, H, Lq, Lk)
    return ((q, k, v, w), _torch_formulation(q, k, v, w, H, sq, sk, torch.float32), _torch_formulation(q, k, v, w, H, sq, sk, torch.float64),
            _kernels(q, k, v, w, H, sq, sk))


def _all_finite(ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def _equal(a, b, what=""):
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), (what, name)


# ---- parity against torch f32 with float64 arbitration ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, H, Lq, Lk, sq, sk", SHAPES)
def test_parity_with_the_masked_torch_formulation_and_float64(B, H, Lq, Lk, sq, sk):
    _, t32, f64, got = _case(B, H, Lq, Lk, sq, sk)
    print("B = %d, H = %d, Lq = %d, Lk = %d, split_q = %d, split_k = %d" % (B, H, Lq, Lk, sq, sk))
    assert _all_finite(got) and _all_finite(t32) and _all_finite(f64)
    for i, name in enumerate(NAMES):
        _check_against(name, got[i], t32[i], f64[i], 1e-5, 2e-6)


# ---- the forward's bits: the two row groups taken apart -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B, H, Lq, Lk, sq, sk", [s for s in SHAPES if 0 < s[4] < s[2]])
def test_forward_rows_carry_the_bits_of_the_unmasked_kernel_on_their_own_keys(B, H, Lq, Lk, sq, sk):
    """Hidden keys add exact zeros and a row's result does not depend on the rows that share its block: rows < split_q are
    ops.xattn_fwd of those rows over the first split_k keys, rows >= split_q are ops.xattn_fwd of those rows over all keys."""
    (q, k, v, w), _, _, got = _case(B, H, Lq, Lk, sq, sk)
    ctx_p, lse_p = ops.xattn_fwd(q[:, :sq].contiguous(), k[:, :sk].contiguous(), v[:, :sk].contiguous(), B, sq, sk, H, SCALE)
    ctx_d, lse_d = ops.xattn_fwd(q[:, sq:].contiguous(), k, v, B, Lq - sq, Lk, H, SCALE)
    assert torch.equal(got[0][:, :sq], ctx_p) and torch.equal(got[1][:, :, :sq], lse_p)
    assert torch.equal(got[0][:, sq:], ctx_d) and torch.equal(got[1][:, :, sq:], lse_d)


# ---- the ends of the split ranges: no mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, H, Lq, Lk", [(2, 2, 65, 63), (1, 2, 161, 161)])
def test_split_q_zero_and_split_k_at_lk_give_the_bits_of_the_unmasked_kernels(B, H, Lq, Lk):
    q, k, v, w = _operands(B, H, Lq, Lk, seed=3)
    want = _unmasked(q, k, v, w, H)
    for sq, sk in ((0, 1), (0, Lk // 2), (0, Lk), (Lq // 2, Lk), (Lq, Lk)):
        _equal(_kernels(q, k, v, w, H, sq, sk), want, (sq, sk))


# ---- a prefix that sees one key -----------------------------------------------------------------------------------------------------------
def test_a_prefix_that_sees_one_key():
    B, H, Lq, Lk, sq, sk = 1, 2, 129, 65, 128, 1
    (q, k, v, w), _, f64, got = _case(B, H, Lq, Lk, sq, sk)
    # p = 1, one MFMA term per channel, l = 1: the context of every prefix row is the first V row of its head, bit for bit
    assert torch.equal(got[0][:, :sq], v[:, :1].expand(B, sq, H * 64))
    # lse = the one scaled score + log(1): the bits of the unmasked kernel on that key, and the float64 score within the forward bound
    _, lse_1 = ops.xattn_fwd(q[:, :sq].contiguous(), k[:, :1].contiguous(), v[:, :1].contiguous(), B, sq, 1, H, SCALE)
    assert torch.equal(got[1][:, :, :sq], lse_1)
    score = (q[:, :sq].double().view(B, sq, H, 64) * k[:, :1].double().view(B, 1, H, 64)).sum(-1).transpose(1, 2) * SCALE
    e = ((got[1][:, :, :sq].double() - score).abs() / score.abs().clamp_min(1.0)).max().item()
    print("one-key prefix lse against the float64 score: %.2e" % e)
    assert e <= 4e-6
    # every key those rows see lies in one key block: the row sum is taken over the block's own P dP, dS = P (dP - P dP) = 0 exactly
    assert not got[2][:, :sq].any()
    print("d_q of the prefix rows: max |x| = %.2e (true value 0, float64 %.2e)" % (got[2][:, :sq].abs().max().item(), f64[2][:, :sq].abs().max().item()))


def test_a_prefix_that_sees_one_key_in_the_single_block_form():
    """Lk <= 64: the single-key-block backward form under the mask.  Rows < split_q see key 0 only -- d_q of those rows is exactly zero
    and they add exactly nothing to d_k -- and the gradients still meet the parity bound."""
    B, H, Lq, Lk, sq, sk = 2, 2, 70, 40, 66, 1
    _, t32, f64, got = _case(B, H, Lq, Lk, sq, sk)
    assert not got[2][:, :sq].any()
    for i, name in enumerate(NAMES):
        _check_against(name, got[i], t32[i], f64[i], 1e-5, 2e-6)
    # d_k of key 0 is what the four rows that see every key give it: the prefix rows' share is an exact zero
    (q, k, v, w), _, _, _ = _case(B, H, Lq, Lk, sq, sk)
    ctx_d, lse_d = ops.xattn_fwd(q[:, sq:].contiguous(), k, v, B, Lq - sq, Lk, H, SCALE)
    _, d_k, _ = ops.xattn_bwd(q[:, sq:].contiguous(), k, v, ctx_d, w[:, sq:].contiguous(), lse_d, B, Lq - sq, Lk, H, SCALE)
    assert _err(got[3], d_k) <= 2e-6


# ---- a NaN in a hidden key row ------------------------------------------------------------------------------------------------------------
def test_a_nan_in_a_hidden_key_row_leaves_the_rows_that_cannot_see_it_untouched():
    B, H, Lq, Lk, sq, sk = 1, 2, 130, 130, 66, 66
    (q, k, v, w), _, _, clean = _case(B, H, Lq, Lk, sq, sk)
    for row in (sk, Lk - 1):                              # the first hidden key (inside the straddling key block) and the last one
        bad = k.clone()
        bad[:, row] = float('nan')
        ctx, lse = ops.xattn_prefix_fwd(q, bad, v, B, Lq, Lk, H, SCALE, sq, sk)
        assert torch.equal(ctx[:, :sq], clean[0][:, :sq]) and torch.equal(lse[:, :, :sq], clean[1][:, :, :sq]), row
        assert not torch.isfinite(ctx[:, sq:]).any() and not torch.isfinite(lse[:, :, sq:]).any(), row      # the rows that see it show it


# ---- views --------------------------------------------------------------------------------------------------------------------------------
def test_views_of_a_packed_qkv_give_the_bits_of_contiguous_copies():
    B, H, L, D = 2, 3, 130, 64
    g = torch.Generator(device='cuda').manual_seed(5)
    qkv = torch.randn(B, L, 3, H * 64, device='cuda', generator=g)
    w = torch.randn(B, L, H * 64, device='cuda', generator=g)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    assert not k.is_contiguous() and k.stride(1) == 3 * H * 64
    _equal(_kernels(q, k, v, w, H, L - D, L - D), _kernels(q.contiguous(), k.contiguous(), v.contiguous(), w, H, L - D, L - D), "packed qkv")
    assert HF._xattn_view(k) is k and HF._xattn_view(q) is q           # through the autograd node the views are passed on as they are


# ---- determinism and capture --------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    B, H, Lq, Lk, sq, sk = 2, 3, 130, 130, 66, 66
    (q, k, v, w), _, _, first = _case(B, H, Lq, Lk, sq, sk)
    _equal(_kernels(q, k, v, w, H, sq, sk), first)


def test_captured_forward_and_backward_replay_the_eager_bits_without_a_memset():
    B, H, Lq, Lk, sq, sk = 2, 3, 130, 130, 66, 66
    (q, k, v, w), _, _, eager = _case(B, H, Lq, Lk, sq, sk)
    assert not _memsets(lambda: _kernels(q, k, v, w, H, sq, sk))       # (what a capture would turn into memset nodes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _kernels(q, k, v, w, H, sq, sk)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _kernels(q, k, v, w, H, sq, sk)
    for _ in range(2):
        for t in captured:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        _equal(captured, eager)


# ---- autograd -----------------------------------------------------------------------------------------------------------------------------
def test_the_autograd_node_returns_the_kernels_gradients():
    B, H, L, D = 2, 3, 130, 64
    (q, k, v, w), _, _, want = _case(B, H, L, L, L - D, L - D)
    x = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = HF.prefix_attention(*x, H, SCALE, L - D, L - D)
    assert [tuple(t.shape) for t in out.grad_fn.saved_tensors] == [(B, L, H * 64)] * 4 + [(B, H, L)]      # q, k, v, ctx, lse: nothing L x L
    (out * w).sum().backward()
    _equal((out.detach(), want[1], x[0].grad, x[1].grad, x[2].grad), want)
    # a packed qkv: the three views reach the kernels as they are and the gradient comes back through the slices
    qkv = torch.stack([q, k, v], dim=2).requires_grad_(True)
    out = HF.prefix_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], H, SCALE, L - D, L - D)
    (out * w).sum().backward()
    assert torch.equal(out.detach(), want[0]) and torch.equal(qkv.grad, torch.stack(want[2:], dim=2))
    for bad in ((-1, 1), (L + 1, 1), (0, 0), (0, L + 1)):
        with pytest.raises(RuntimeError, match="split_"):
            HF.prefix_attention(q, k, v, H, SCALE, *bad)
