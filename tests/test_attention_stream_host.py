"""The attention entry points beyond 160 tokens, host side (no GPU): the argument checks of upp_attn_fwd / upp_attn_bwd that return before
the first launch, the lifted range (L = 161 ... ATTN_MAX_L is accepted: the range check precedes the B == 0 return, so a library that still
stops at 160 answers UPP_E_RANGE here), and the one constant that the models' `fusable` predicates and the library share.  The pointers
are fake non-NULL values that are never dereferenced."""
import ctypes
import os
import re

import pytest
import torch

from models import upp_layers
from upp_hip import _abi, functional as HF, ops

BADARG, RANGE = -1, -2
P = ctypes.c_void_p(64)            # non-NULL, 16-byte aligned, never dereferenced
MAX_L = ops.ATTN_MAX_L


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


def _fwd(lib, B, L, H=6, hd=64, ptrs=(P, P, P)):
    return lib.upp_attn_fwd(*ptrs, B, L, H, hd, 0.125, None)


def _bwd(lib, B, L, H=6, hd=64, ptrs=(P, P, P, P, P)):
    return lib.upp_attn_bwd(*ptrs, B, L, H, hd, 0.125, None)


def test_attention_refuses_bad_arguments(lib):
    for k in range(3):
        assert _fwd(lib, 2, 257, ptrs=tuple(None if i == k else P for i in range(3))) == BADARG, k
    for k in range(5):
        assert _bwd(lib, 2, 257, ptrs=tuple(None if i == k else P for i in range(5))) == BADARG, k
    for B, L, H in ((-1, 257, 6), (2, 0, 6), (2, 257, 0)):
        assert _fwd(lib, B, L, H) == BADARG and _bwd(lib, B, L, H) == BADARG, (B, L, H)
    for hd in (32, 128):
        assert _fwd(lib, 0, 257, hd=hd) == RANGE and _bwd(lib, 0, 257, hd=hd) == RANGE, hd
    for L in (MAX_L + 1, 2 * MAX_L, 2 ** 30):
        assert _fwd(lib, 0, L) == RANGE and _bwd(lib, 0, L) == RANGE, L
        assert _fwd(lib, 2, L) == RANGE and _bwd(lib, 2, L) == RANGE, L


def test_attention_accepts_every_length_up_to_the_maximum(lib):
    # B == 0 returns 0 after the range check and before any launch
    assert MAX_L >= 2048
    for L in (1, 96, 97, 160, 161, 257, MAX_L - 1, MAX_L):
        assert _fwd(lib, 0, L) == 0, L
        assert _bwd(lib, 0, L) == 0, L


def test_the_header_states_the_same_maximum():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "upp_hip.h")
    m = re.search(r"#define\s+UPP_ATTN_MAX_L\s+(\d+)", open(header).read())
    assert m and int(m.group(1)) == MAX_L


class _Shape:
    """What the `fusable` predicates read of a tensor (a CUDA f32 tensor of this shape), without a GPU."""

    def __init__(self, *shape):
        self.shape, self.is_cuda, self.dtype = torch.Size(shape), True, torch.float32


def test_fusable_predicates_follow_the_library_maximum():
    assert HF.ATTN_MAX_L == MAX_L
    attn = upp_layers.Attention(384, num_heads=6)
    blk = upp_layers.Block(384, 6)
    for L in (144, 145, 161, 257, MAX_L):
        assert attn.fusable(_Shape(2, L, 384)), L
    assert not attn.fusable(_Shape(2, MAX_L + 1, 384))
    assert not attn.fusable(_Shape(2, 257, 768))                     # head_dim 128
    # a block may insert up to 16 prompt rows in front of the attention
    for L in (128, 129, 257, MAX_L - 16):
        assert blk.fusable(_Shape(2, L, 384)), L
    assert not blk.fusable(_Shape(2, MAX_L - 15, 384))
