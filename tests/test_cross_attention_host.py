"""Cross-attention and the PoinTr decoder block, host side (no GPU): the two new C-ABI entry points (header = ctypes table = nm -D, the
argument checks that return before the first launch), the operand rules of ops.xattn_fwd / xattn_bwd, the torch formulations of
upp_hip.torch_cpu.cross_attention, models.upp_layers.CrossAttention and DecoderBlock against the reference's own outputs
(tests/golden/decoder_block.npz, tools/gen_golden_decoder_block.py) and the reference's state-dict schema."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _decoder_block_case as case
import _seeded
from conftest import ROOT
from models import upp_layers
from upp_hip import _abi, functional as HF, ops, torch_cpu

BADARG, RANGE = -1, -2
P = ctypes.c_void_p(64)            # non-NULL, 16-byte aligned, never dereferenced
MAX_L = ops.ATTN_MAX_L
NAMES = ("upp_xattn_fwd", "upp_xattn_bwd")
FIXTURE_BOUND = 1e-5               # of each output's max: the project's fixture bound


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "decoder_block.npz"))


def test_header_ctypes_table_and_library_agree_on_the_new_names(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "upp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(upp_[a-z0-9_]+)\s*\(", text))
    exported = {l.split()[-1] for l in subprocess.check_output(["nm", "-D", _abi.LIB_PATH]).decode().splitlines() if " T upp_" in l}
    for n in NAMES:
        assert n in declared and n in exported and n in _abi.SIGNATURES, n
    assert declared == exported == set(_abi.SIGNATURES)
    # the header's argument lists and the ctypes rows have the same lengths and the same kinds
    for n in NAMES:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, text, flags=re.S).group(1).split(",")
        kinds = [ctypes.c_void_p if "*" in a else ctypes.c_longlong if "long long" in a else ctypes.c_float if "float" in a else ctypes.c_int
                 for a in args]
        assert kinds == _abi.SIGNATURES[n][1], n
    assert lib.upp_abi_version() == 5 == _abi.ABI_VERSION
    assert "UPP_OPT_COUNT = 4" in text and len(_abi.OPTIONS) == 4
    assert int(re.search(r"#define\s+UPP_ABI_VERSION\s+(\d+)", text).group(1)) == 5


def _fwd(lib, B=2, Lq=224, Lk=128, H=6, hd=64, rs=None, ptrs=(P,) * 5):
    rs = rs or (H * 64,) * 3
    return lib.upp_xattn_fwd(*ptrs, B, Lq, Lk, H, hd, *rs, 0.125, None)


def _bwd(lib, B=2, Lq=224, Lk=128, H=6, hd=64, rs=None, ptrs=(P,) * 9):
    rs = rs or (H * 64,) * 6
    return lib.upp_xattn_bwd(*ptrs, B, Lq, Lk, H, hd, *rs, 0.125, None)


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    for k in range(5):
        assert _fwd(lib, ptrs=tuple(None if i == k else P for i in range(5))) == BADARG, k
    for k in range(9):
        assert _bwd(lib, ptrs=tuple(None if i == k else P for i in range(9))) == BADARG, k
    for kw in (dict(B=-1), dict(Lq=0), dict(Lk=0), dict(H=0), dict(Lq=-3)):
        assert _fwd(lib, **kw) == BADARG and _bwd(lib, **kw) == BADARG, kw
    for k in range(3):
        for bad in (6 * 64 - 4, 6 * 64 + 2, 0, -384):
            assert _fwd(lib, rs=tuple(bad if i == k else 384 for i in range(3))) == BADARG, (k, bad)
    for k in range(6):
        for bad in (6 * 64 - 4, 6 * 64 + 2, 0):
            assert _bwd(lib, rs=tuple(bad if i == k else 384 for i in range(6))) == BADARG, (k, bad)
    for hd in (32, 128):
        assert _fwd(lib, B=0, hd=hd) == RANGE and _bwd(lib, B=0, hd=hd) == RANGE, hd
    for kw in (dict(Lq=MAX_L + 1), dict(Lk=MAX_L + 1), dict(Lq=2 ** 30, Lk=1)):
        for B in (0, 2):                                   # the range check precedes the B == 0 return
            assert _fwd(lib, B=B, **kw) == RANGE and _bwd(lib, B=B, **kw) == RANGE, (B, kw)


def test_entry_points_accept_the_whole_range_and_the_three_operand_forms(lib):
    # B == 0 returns 0 after every check and before any launch
    for Lq, Lk in ((1, 1), (1, MAX_L), (MAX_L, 1), (224, 128), (576, 256), (MAX_L, MAX_L)):
        assert _fwd(lib, B=0, Lq=Lq, Lk=Lk) == 0 and _bwd(lib, B=0, Lq=Lq, Lk=Lk) == 0, (Lq, Lk)
    for rs in (384, 2 * 384, 3 * 384, 388):
        assert _fwd(lib, B=0, rs=(rs,) * 3) == 0 and _bwd(lib, B=0, rs=(rs,) * 6) == 0, rs


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

    def both(match, q=q, k=k, v=v, Lq=Lq, Lk=Lk, H=H):
        with pytest.raises(RuntimeError, match=match):
            ops.xattn_fwd(q, k, v, B, Lq, Lk, H, 0.125)
        with pytest.raises(RuntimeError, match=match):
            ops.xattn_bwd(q, k, v, ctx, ctx.clone(), lse, B, Lq, Lk, H, 0.125)

    both("must be a HIP")                                                     # the good arguments, on a host tensor
    both("must be torch.float32", q=q.double())
    both("must be torch.float32", v=v.half())
    shifted = torch.zeros(k.numel() + 1)[1:].view(B, Lk, H * 64)              # contiguous, one float into its storage
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    both("16-byte aligned", k=shifted)
    packed = torch.zeros(B, Lk, 2 * H * 64 + 2)                               # a row stride that is no multiple of 4
    both("row stride", k=packed[:, :, :H * 64])
    both("last dimension must be contiguous", k=torch.zeros(B, Lk, 2 * H * 64)[:, :, ::2])
    both("sample stride", v=torch.zeros(B, Lk + 1, H * 64)[:, :Lk])           # rows behind every sample: not L * rs
    both("head_dim 64", q=torch.zeros(B, Lq, H * 32), k=torch.zeros(B, Lk, H * 32), v=torch.zeros(B, Lk, H * 32))
    both("lengths >= 1", q=torch.zeros(B, 0, H * 64), Lq=0)
    both("lengths >= 1", k=torch.zeros(B, 0, H * 64), v=torch.zeros(B, 0, H * 64), Lk=0)
    both("up to ATTN_MAX_L", q=torch.zeros(1, MAX_L + 1, H * 64).expand(B, -1, -1), Lq=MAX_L + 1)
    both("up to ATTN_MAX_L", k=torch.zeros(1, MAX_L + 1, H * 64).expand(B, -1, -1), v=torch.zeros(1, MAX_L + 1, H * 64).expand(B, -1, -1),
         Lk=MAX_L + 1)
    both(r"must be \(B, L, H \* 64\)", k=k[:, :-1])
    assert MAX_L + 1 == 2049
    # the backward's dense operands
    for bad in (dict(ctx=ctx[:, :-1]), dict(d_ctx=ctx.double()), dict(lse=lse[:, :, :-1]), dict(d_ctx=ctx.transpose(1, 2).contiguous().transpose(1, 2))):
        args = dict(ctx=ctx, d_ctx=ctx.clone(), lse=lse)
        args.update(bad)
        with pytest.raises(RuntimeError, match="dense float32"):
            ops.xattn_bwd(q, k, v, args["ctx"], args["d_ctx"], args["lse"], B, Lq, Lk, H, 0.125)


def test_strided_views_pass_the_operand_rule():
    """the three forms of include/upp_hip.h: separate products, a packed [k|v], views of a packed qkv -- each reaches the device check"""
    B, L, H = 2, 7, 3
    qkv = torch.zeros(B, L, 3, H, 64)
    kv = torch.zeros(B, L, 2 * H * 64)
    for q, k, v, rs in ((qkv[:, :, 0].reshape(B, L, H * 64), qkv[:, :, 1].reshape(B, L, H * 64), qkv[:, :, 2].reshape(B, L, H * 64), H * 64),
                        (qkv.view(B, L, 3, H * 64)[:, :, 0], kv[:, :, :H * 64], kv[:, :, H * 64:], None)):
        with pytest.raises(RuntimeError, match="must be a HIP"):
            ops.xattn_fwd(q, k, v, B, L, L, H, 0.125)
    view = qkv.view(B, L, 3, H * 64)[:, :, 1]
    assert not view.is_contiguous() and HF._xattn_view(view) is view
    assert HF._xattn_view(torch.zeros(B, H * 64, L).transpose(1, 2)).is_contiguous()


def _rel(got, want):
    want = torch.as_tensor(want)
    return ((got.detach() - want).abs().max() / want.abs().max()).item()


def test_cpu_formulations_equal_the_reference_fixture(golden):
    q, v, self_idx, cross_idx = case.inputs()
    xattn = _seeded.fill(upp_layers.CrossAttention(case.DIM, case.DIM, num_heads=case.HEADS)).eval()
    block = _seeded.fill(upp_layers.DecoderBlock(case.DIM, case.HEADS)).eval()
    with torch.no_grad():
        core = torch_cpu.cross_attention(xattn.q_map(q), xattn.k_map(v), xattn.v_map(v), case.HEADS, xattn.scale)
        got = {"core": xattn.proj(core), "xattn": xattn(q, v), "plain": block(q, v), "knn": block(q, v, self_idx, cross_idx),
               "knn64": block(q, v, self_idx.long(), cross_idx.long())}
    errs = {name: _rel(t, golden[name if name in golden.files else {"core": "xattn", "knn64": "knn"}[name]]) for name, t in got.items()}
    print("decoder-block fixture, CPU torch formulation: " + ", ".join("%s %.2e" % kv for kv in errs.items()) + " of the output's max")
    assert set(golden.files) == {"xattn", "plain", "knn"}
    for name, e in errs.items():
        assert e <= FIXTURE_BOUND, (name, e)
    assert _rel(got["knn"], golden["plain"]) > 1e-2                            # the local branches do change the output


def test_reference_state_dicts_load_strictly():
    dim = 384
    lin = lambda o, i, bias=True: {"weight": (o, i), **({"bias": (o,)} if bias else {})}          # noqa: E731
    ln = {"weight": (dim,), "bias": (dim,)}
    xattn = {"q_map": lin(dim, dim, False), "k_map": lin(dim, dim, False), "v_map": lin(dim, dim, False), "proj": lin(dim, dim)}
    block = {"norm1": ln, "self_attn.qkv": lin(3 * dim, dim, False), "self_attn.proj": lin(dim, dim), "norm_q": ln, "norm_v": ln,
             "norm2": ln, "mlp.fc1": lin(4 * dim, dim), "mlp.fc2": lin(dim, 4 * dim), "knn_map.0": lin(dim, 2 * dim),
             "merge_map": lin(dim, 2 * dim), "knn_map_cross.0": lin(dim, 2 * dim), "merge_map_cross": lin(dim, 2 * dim)}
    block.update({"attn." + k: v for k, v in xattn.items()})

    def state(schema):
        return {"%s.%s" % (mod, leaf): torch.zeros(shape) for mod, leaves in schema.items() for leaf, shape in leaves.items()}

    upp_layers.CrossAttention(dim, dim, num_heads=6).load_state_dict(state(xattn), strict=True)
    upp_layers.DecoderBlock(dim, 6).load_state_dict(state(block), strict=True)
    assert len(state(block)) == 28
    with_bias = upp_layers.CrossAttention(dim, dim, num_heads=6, qkv_bias=True)
    assert {k for k in with_bias.state_dict() if k.endswith("bias")} == {"q_map.bias", "k_map.bias", "v_map.bias", "proj.bias"}


class _Shape:
    """What the `fusable` predicates read of a tensor (a CUDA f32 tensor of this shape), without a GPU."""

    def __init__(self, *shape):
        self.shape, self.is_cuda, self.dtype = torch.Size(shape), True, torch.float32


def test_fusable_follows_head_dim_lengths_and_dropout():
    m = upp_layers.CrossAttention(384, 384, num_heads=6)
    for Lq, Lk in ((224, 128), (576, 256), (1, 1), (MAX_L, MAX_L)):
        assert m.fusable(_Shape(2, Lq, 384), _Shape(2, Lk, 384)), (Lq, Lk)
    assert not m.fusable(_Shape(2, MAX_L + 1, 384), _Shape(2, 128, 384))
    assert not m.fusable(_Shape(2, 224, 384), _Shape(2, MAX_L + 1, 384))
    assert not upp_layers.CrossAttention(384, 384, num_heads=12).fusable(_Shape(2, 224, 384), _Shape(2, 128, 384))      # head_dim 32
    drop = upp_layers.CrossAttention(384, 384, num_heads=6, attn_drop=0.1)
    assert not drop.fusable(_Shape(2, 224, 384), _Shape(2, 128, 384)) and drop.eval().fusable(_Shape(2, 224, 384), _Shape(2, 128, 384))
    assert not m.fusable(torch.zeros(2, 224, 384), torch.zeros(2, 128, 384))                                            # a host tensor
