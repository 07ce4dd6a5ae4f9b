"""What tests/test_gpu_attention_family_bits.py and tools/gen_golden_attn_family_bits.py share: the cases of the streaming attention family
(csrc/attn_stream.hip: self-attention beyond 160 tokens, cross-attention, prefix-visibility attention), their inputs and the calls that
produce the arrays of tests/golden/attn_stream_family_bits.npz.

The inputs are a closed form of the element index in 32-bit integer arithmetic (numpy, no random-number library): a multiplicative hash
with the murmur3 finaliser, whose top 24 bits map to the multiples of 2^-23 in [-1, 1) -- every value is exact in float32.  The cases are
the smallest shapes that reach every path of the three kernel bodies, H * 64 channels, scale 0.125:
    self_161          (B, H, L) = (1, 1, 161): three blocks with a 33-row tail, the dispatch edge of the family
    cross_65x63       (1, 2, 65, 63): the single-key-block delta form, a 1-row query tail, a second head
    cross_70x130      (1, 1, 70, 130): more than one block in both directions
    prefix_130_66     (1, 2, 130, 130, 66, 66): a straddling query block, shortened walks, a key block whose query walk starts late
    prefix_96_32      (1, 1, 96, 96, 32, 32): a query block wholly below split_q with split_k <= 64 -- the single-block form inside a
                      multi-block call"""
import numpy as np
import torch

from upp_hip import ops

SCALE = 0.125
CASES = {
    "self_161": ("self", 1, 1, 161),
    "cross_65x63": ("cross", 1, 2, 65, 63),
    "cross_70x130": ("cross", 1, 1, 70, 130),
    "prefix_130_66": ("prefix", 1, 2, 130, 130, 66, 66),
    "prefix_96_32": ("prefix", 1, 1, 96, 96, 32, 32),
}
ARRAYS = {"self": ("ctx", "lse", "d_qkv"), "cross": ("ctx", "lse", "d_q", "d_k", "d_v"), "prefix": ("ctx", "lse", "d_q", "d_k", "d_v")}


def pattern(shape, salt):
    """float32 array of `shape` in [-1, 1): element i is hash32(i * 2654435761 + salt * 0x9E3779B9) >> 8, as a multiple of 2^-23, minus 1"""
    n = int(np.prod(shape))
    h = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32((salt * 0x9E3779B9) & 0xFFFFFFFF)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return ((h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)).reshape(shape)


def _dev(shape, salt):
    return torch.from_numpy(pattern(shape, salt)).cuda()


def run(name):
    """the kernels' forward and backward of one case -> {array name: tensor}, in the order of ARRAYS"""
    kind, B, H = CASES[name][:3]
    salt = 16 * list(CASES).index(name)
    if kind == "self":
        L = CASES[name][3]
        qkv, w = _dev((B, L, 3 * H * 64), salt), _dev((B, L, H * 64), salt + 1)
        ctx, lse = ops.attn_fwd(qkv, B, L, H, SCALE)
        got = (ctx, lse, ops.attn_bwd(qkv, ctx, w, lse, B, L, H, SCALE))
    else:
        Lq, Lk = CASES[name][3:5]
        q, w = _dev((B, Lq, H * 64), salt), _dev((B, Lq, H * 64), salt + 1)
        k, v = _dev((B, Lk, H * 64), salt + 2), _dev((B, Lk, H * 64), salt + 3)
        if kind == "cross":
            ctx, lse = ops.xattn_fwd(q, k, v, B, Lq, Lk, H, SCALE)
            got = (ctx, lse) + ops.xattn_bwd(q, k, v, ctx, w, lse, B, Lq, Lk, H, SCALE)
        else:
            sq, sk = CASES[name][5:]
            ctx, lse = ops.xattn_prefix_fwd(q, k, v, B, Lq, Lk, H, SCALE, sq, sk)
            got = (ctx, lse) + ops.xattn_prefix_bwd(q, k, v, ctx, w, lse, B, Lq, Lk, H, SCALE, sq, sk)
    return dict(zip(ARRAYS[kind], got))
