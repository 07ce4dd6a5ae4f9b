"""Denoising-query (prefix-visibility) attention and the AdaPoinTr blocks, host side (no GPU): the argument checks of the two C-ABI entry
points and of ops.xattn_prefix_fwd / xattn_prefix_bwd that return before the first launch, upp_hip.torch_cpu.prefix_attention against the
reference's mask formula in float64, and the modules of models.AdaPoinTr / models.Transformer_utils on the CPU (torch formulation)
against the reference's own outputs (tests/golden/adapointr_blocks.npz, tools/gen_golden_adapointr_blocks.py) and its state-dict schema.

The fixture bound is the PoinTr fixture's: every output is compared with the reference's FLOAT64 run; its error over the output's
maximum is at most max(1e-5, 3 x err_ref), err_ref being the reference's own f32-against-f64 error of that output, computed here from
the two stored arrays.  Measured for the torch formulation on the CPU: a 3.7e-7, b 3.8e-7, c 3.2e-7, d 3.1e-7 (err_ref 4.8e-7, 4.4e-7,
3.3e-7, 5.2e-7: the bound is 1e-5 for all four)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _adapointr_case as case
from conftest import GOLDEN
from upp_hip import _abi, functional as HF, ops, torch_cpu

BADARG, RANGE = -1, -2
P = ctypes.c_void_p(64)            # non-NULL, 16-byte aligned, never dereferenced
MAX_L = ops.ATTN_MAX_L


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "adapointr_blocks.npz"))


@pytest.fixture()
def cpu_formulations():
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    yield
    torch_cpu.enable(was)


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def _fwd(lib, B=2, Lq=40, Lk=40, H=2, hd=64, rs=None, sq=32, sk=32):
    rs = rs or (H * 64,) * 3
    return lib.upp_xattn_prefix_fwd(*(P,) * 5, B, Lq, Lk, H, hd, *rs, 0.125, sq, sk, None)


def _bwd(lib, B=2, Lq=40, Lk=40, H=2, hd=64, rs=None, sq=32, sk=32):
    rs = rs or (H * 64,) * 6
    return lib.upp_xattn_prefix_bwd(*(P,) * 9, B, Lq, Lk, H, hd, *rs, 0.125, sq, sk, None)


def test_entry_points_refuse_bad_splits_before_any_launch(lib):
    for kw in (dict(sq=-1), dict(sq=41), dict(sk=0), dict(sk=41), dict(sk=-5), dict(Lq=70, Lk=130, sq=71, sk=1), dict(Lq=70, Lk=130, sq=0, sk=131)):
        for B in (0, 2):                                   # the split check precedes the B == 0 return
            assert _fwd(lib, B=B, **kw) == BADARG and _bwd(lib, B=B, **kw) == BADARG, (B, kw)
    # the checks of upp_xattn_* come first and keep their codes
    assert _fwd(lib, B=0, hd=32) == RANGE and _bwd(lib, B=0, hd=32) == RANGE
    for kw in (dict(Lq=MAX_L + 1, sq=0), dict(Lk=MAX_L + 1, sk=1)):
        assert _fwd(lib, B=0, **kw) == RANGE and _bwd(lib, B=0, **kw) == RANGE, kw
    assert _fwd(lib, rs=(124, 128, 128)) == BADARG and _bwd(lib, rs=(128,) * 5 + (130,)) == BADARG
    assert _fwd(lib, Lq=0, sq=0) == BADARG and _bwd(lib, Lk=0) == BADARG


def test_entry_points_accept_every_split_in_range(lib):
    # B == 0 returns 0 after every check and before any launch
    for Lq, Lk, sq, sk in ((40, 40, 0, 1), (40, 40, 40, 40), (40, 40, 0, 40), (40, 40, 40, 1), (1, 1, 0, 1), (1, 1, 1, 1), (576, 576, 512, 512),
                           (MAX_L, MAX_L, MAX_L - 64, MAX_L - 64), (70, 130, 6, 65)):
        assert _fwd(lib, B=0, Lq=Lq, Lk=Lk, sq=sq, sk=sk) == 0 and _bwd(lib, B=0, Lq=Lq, Lk=Lk, sq=sq, sk=sk) == 0, (Lq, Lk, sq, sk)
    assert _fwd(lib, B=0, rs=(384,) * 3) == 0 and _bwd(lib, B=0, rs=(384,) * 6) == 0              # views of a packed qkv


# ---- the torch operators ------------------------------------------------------------------------------------------------------------------
def _operands(B=2, Lq=5, Lk=3, H=2):
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B, L, H * 64, generator=g) for L in (Lq, Lk, Lk))
    ctx, lse = torch.randn(B, Lq, H * 64, generator=g), torch.randn(B, H, Lq, generator=g)
    return q, k, v, ctx, lse


def test_operators_raise_before_any_launch(monkeypatch):
    """Every rule but the device is checked first, so that a host without a GPU can see each of them: the good arguments get as far as
    "must be a HIP tensor", each bad one stops at its own message -- and nothing reaches the launcher."""
    B, Lq, Lk, H = 2, 5, 3, 2
    q, k, v, ctx, lse = _operands(B, Lq, Lk, H)

    def no_launch(*a, **kw):
        pytest.fail("a kernel was launched on a bad argument: %r" % (a[1],))

    monkeypatch.setattr(ops, "_call", no_launch)
    fwd = lambda q=q, k=k, v=v, Lq=Lq, Lk=Lk, sq=2, sk=2: ops.xattn_prefix_fwd(q, k, v, B, Lq, Lk, H, 0.125, sq, sk)          # noqa: E731
    bwd = lambda q=q, k=k, v=v, ctx=ctx, d=ctx, lse=lse, sq=2, sk=2: ops.xattn_prefix_bwd(q, k, v, ctx, d, lse, B, Lq, Lk, H, 0.125, sq, sk)  # noqa: E731
    for call in (fwd, bwd):
        with pytest.raises(RuntimeError, match="must be a HIP"):
            call()
        for sq in (-1, Lq + 1):
            with pytest.raises(RuntimeError, match="split_q"):
                call(sq=sq)
        for sk in (0, -1, Lk + 1):
            with pytest.raises(RuntimeError, match="split_k"):
                call(sk=sk)
        for sq, sk in ((0, 1), (Lq, Lk), (0, Lk), (Lq, 1)):                   # the ends of both ranges are served
            with pytest.raises(RuntimeError, match="must be a HIP"):
                call(sq=sq, sk=sk)
        with pytest.raises(RuntimeError, match="float32"):
            call(k=k.double())
        with pytest.raises(RuntimeError, match="float32"):
            call(q=q.half())
        with pytest.raises(RuntimeError, match="row stride"):
            call(v=torch.randn(B, Lk, H * 64 + 2)[:, :, :H * 64])
        with pytest.raises(RuntimeError, match="last dimension must be contiguous"):
            call(q=torch.randn(B, H * 64, Lq).transpose(1, 2))
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(k=torch.randn(B * Lk * H * 64 + 4)[1:1 + B * Lk * H * 64].view(B, Lk, H * 64))
    with pytest.raises(RuntimeError, match="ATTN_MAX_L"):
        ops.xattn_prefix_fwd(torch.randn(1, MAX_L + 1, 64), k[:1, :, :64], v[:1, :, :64], 1, MAX_L + 1, Lk, 1, 0.125, 0, 1)
    with pytest.raises(RuntimeError, match="ATTN_MAX_L"):
        ops.xattn_prefix_bwd(q, k, v, ctx, ctx, lse, B, Lq, MAX_L + 1, H, 0.125, 2, 2)
    with pytest.raises(RuntimeError, match="dense float32"):
        bwd(d=ctx.transpose(0, 1))
    # a packed qkv's views pass the layout rules
    qkv = torch.randn(B, Lq, 3, H * 64)
    with pytest.raises(RuntimeError, match="must be a HIP"):
        ops.xattn_prefix_fwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], B, Lq, Lq, H, 0.125, 3, 3)


def _reference_masked(x_q, x_k, x_v, H, scale, mask):
    """reference models/Transformer_utils.py:105-117 on separate q, k, v (B, L, H * hd): masked_fill(mask > 0, -finfo.max), softmax"""
    B, Lq, C = x_q.shape
    Lk = x_k.shape[1]
    q, k, v = (t.view(B, L, H, C // H).permute(0, 2, 1, 3) for t, L in ((x_q, Lq), (x_k, Lk), (x_v, Lk)))
    attn = (q @ k.transpose(-2, -1)) * scale
    attn = attn.masked_fill(mask > 0, -torch.finfo(attn.dtype).max).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, Lq, C), attn


@pytest.mark.parametrize("Lq, Lk, sq, sk", [(40, 40, 32, 32), (7, 9, 3, 1), (5, 3, 0, 2), (5, 3, 5, 3), (6, 6, 6, 2)])
def test_torch_formulation_is_the_references_mask_formula(Lq, Lk, sq, sk):
    B, H = 2, 2
    g = torch.Generator().manual_seed(Lq * 100 + Lk)
    q, k, v = (torch.randn(B, L, H * 16, generator=g, dtype=torch.float64) for L in (Lq, Lk, Lk))
    mask = torch.zeros(Lq, Lk, dtype=torch.float64)
    mask[:sq, sk:] = 1.                                                       # the reference's mask[:-D, -D:] = 1 for Lq = Lk, both splits L - D
    if Lq == Lk and sq == sk and 0 < sq < Lq:
        ref_mask = torch.zeros(Lq, Lq)
        ref_mask[:-(Lq - sq), -(Lq - sq):] = 1.
        assert torch.equal(mask, ref_mask.double())
    want, attn = _reference_masked(q, k, v, H, 0.25, mask)
    got = torch_cpu.prefix_attention(q, k, v, H, 0.25, sq, sk)
    assert torch.equal(got, want)
    assert not attn[:, :, :sq, sk:].any() and (attn.sum(-1) - 1).abs().max() < 1e-12          # hidden keys: probability exactly 0
    # differentiable, and the hidden keys get no gradient from the rows that cannot see them
    x = [t.clone().requires_grad_(True) for t in (q, k, v)]
    torch_cpu.prefix_attention(*x, H, 0.25, sq, sk)[:, :sq].sum().backward()
    assert not x[1].grad[:, sk:].any() and not x[2].grad[:, sk:].any()
    for bad in ((-1, 1), (Lq + 1, 1), (0, 0), (0, Lk + 1)):
        with pytest.raises(ValueError):
            torch_cpu.prefix_attention(q, k, v, H, 0.25, *bad)


def test_functional_entry_serves_cpu_tensors_only_when_enabled(cpu_formulations):
    q, k, v, _, _ = _operands(2, 6, 6, 2)
    got = HF.prefix_attention(q, k, v, 2, 0.125, 4, 4)
    assert torch.equal(got, torch_cpu.prefix_attention(q, k, v, 2, 0.125, 4, 4))
    torch_cpu.enable(False)
    with pytest.raises(RuntimeError, match="must be a HIP"):
        HF.prefix_attention(q, k, v, 2, 0.125, 4, 4)


# ---- the modules on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case.CASES)
def test_torch_formulation_on_cpu_meets_the_fixture_bound(fixture, cpu_formulations, name):
    from models import AdaPoinTr
    assert int(fixture["seed"]) == 0
    with torch.no_grad():
        got = case.run(case.module(AdaPoinTr, name), name, *case.inputs(int(fixture["seed"])))
    case.check_output(fixture, name, got, "cpu torch formulation")


def test_state_dicts_are_the_references_and_round_trip():
    from models import AdaPoinTr
    want = {}
    for line in open(os.path.join(GOLDEN, "adapointr_blocks_keys.txt")):
        name, key, *shape = line.split()
        want.setdefault(name, []).append((key, tuple(int(s) for s in shape)))
    assert sorted(want) == ["a", "c", "d"] and sum(len(v) for v in want.values()) == 116
    for name in want:
        m = case.module(AdaPoinTr, name)
        sd = m.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == want[name], name
        fresh = case.module(AdaPoinTr, name)
        changed = {k: v + 1 for k, v in sd.items()}
        fresh.load_state_dict(changed, strict=True)
        assert all(torch.equal(v, changed[k]) for k, v in fresh.state_dict().items())


def test_entry_classes_and_reexports():
    from models import AdaPoinTr, MODELS, Transformer_utils, upp_layers
    assert (Transformer_utils.Mlp, Transformer_utils.CrossAttention, Transformer_utils.index_points) == (
        upp_layers.Mlp, upp_layers.CrossAttention, upp_layers.index_points)
    assert issubclass(Transformer_utils.Attention, upp_layers.Attention)
    cfg = dict(embed_dim=128, depth=2, num_heads=2, block_style_list=case.STYLES, combine_style='onebyone', k=case.K)
    enc = AdaPoinTr.PointTransformerEncoderEntry(cfg)
    assert isinstance(enc.blocks, AdaPoinTr.TransformerEncoder) and enc.blocks.blocks[0].norm1.eps == 1e-6 and hasattr(enc.blocks.blocks[0], "norm3")
    dec = AdaPoinTr.PointTransformerDecoderEntry(dict(embed_dim=128, depth=1, num_heads=2, self_attn_block_style_list=['graph'],
                                                      cross_attn_block_style_list=['graph-attn'], k=case.K))
    blk = dec.blocks.blocks[0]
    assert blk.self_attn is None and blk.local_self_attn is not None and blk.cross_attn is not None and hasattr(blk, "cross_attn_merge_map")
    assert MODELS.get("AdaPoinTr") is None                                                       # no model is registered yet


@pytest.mark.parametrize("token", ["rw_deform", "deform", "deform_graph"])
def test_unported_block_tokens_raise_and_name_the_token(token):
    from models import AdaPoinTr
    with pytest.raises(ValueError, match="%r" % token):
        AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-' + token)
    with pytest.raises(ValueError, match="%r" % token):
        AdaPoinTr.CrossAttnBlockApi(128, 2, self_attn_block_style=token, cross_attn_block_style='attn')
    with pytest.raises(ValueError, match="%r" % token):
        AdaPoinTr.CrossAttnBlockApi(128, 2, self_attn_block_style='attn', cross_attn_block_style='attn-' + token)
    with pytest.raises(ValueError, match="%r" % token):
        AdaPoinTr.PointTransformerEncoder(embed_dim=128, depth=1, num_heads=2, block_style_list=[token])


def test_denoise_length_that_leaves_fewer_real_tokens_than_neighbours_raises(cpu_formulations):
    from models import AdaPoinTr, Transformer_utils
    q, v, q_pos, v_pos = case.inputs(0)
    graph = Transformer_utils.DynamicGraphAttention(case.DIM, k=case.K)
    with pytest.raises(ValueError, match="real tokens"):
        graph(q, q_pos, denoise_length=case.NQ - case.K + 1)                 # 7 real tokens for 8 neighbours
    assert graph(q, q_pos, denoise_length=case.NQ - case.K).shape == q.shape  # 8 real tokens: served
    with pytest.raises(ValueError, match="self branch"):
        graph(q, q_pos, v=v, v_pos=v_pos, denoise_length=8)
    dec = case.module(AdaPoinTr, "a")
    with pytest.raises(ValueError, match="real tokens"):
        dec(q, v, q_pos, v_pos, denoise_length=case.NQ - case.K + 1)
    attn = Transformer_utils.Attention(case.DIM, num_heads=case.HEADS)
    for bad in (0, case.NQ, -1):
        with pytest.raises(ValueError, match="denoise_length"):
            attn(q, denoise_length=bad)
    with pytest.raises(ValueError, match="not both"):
        attn(q, mask=torch.zeros(case.NQ, case.NQ), denoise_length=8)


def test_denoise_lists_are_the_two_searches_of_the_reference(cpu_formulations):
    from models import Transformer_utils as TU
    _, _, q_pos, _ = case.inputs(0)
    idx = TU.denoise_knn(case.K, q_pos, case.D)
    R = case.NQ - case.D
    assert idx.shape == (case.B, case.NQ, case.K) and idx.dtype == torch.int64
    assert int(idx[:, :R].max()) < R                                                              # the real queries never list a denoising one
    assert torch.equal(idx[:, :R], TU.knn_point(case.K, q_pos[:, :R], q_pos[:, :R]))
    assert torch.equal(idx[:, R:], TU.knn_point(case.K, q_pos, q_pos[:, R:]))


def test_attention_with_denoise_length_equals_the_references_mask(cpu_formulations):
    from models import Transformer_utils as TU
    import _seeded
    q = case.inputs(0)[0]
    attn = _seeded.fill(TU.Attention(case.DIM, num_heads=case.HEADS)).eval()
    mask = torch.zeros(case.NQ, case.NQ)
    mask[:-case.D, -case.D:] = 1.
    with torch.no_grad():
        assert torch.equal(attn(q, denoise_length=case.D), attn(q, mask=mask))
        assert not torch.equal(attn(q, denoise_length=case.D), attn(q))
