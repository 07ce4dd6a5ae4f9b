"""The one case of tests/golden/decoder_block.npz, shared by its generator (tools/gen_golden_decoder_block.py: the reference's
CrossAttention and DecoderBlock) and by the tests of this repository's classes: dim 128, 2 heads (head_dim 64), B = 2, 40 queries over 24
proxies, everything from one seeded CPU generator.  The neighbour lists are random: the block consumes whatever lists it is given, so
random ones avoid every tie question of a neighbour search."""
import torch

DIM, HEADS, B, NQ, NK, K = 128, 2, 2, 40, 24, 8


def inputs(seed=0):
    """-> q (B,NQ,DIM), v (B,NK,DIM) f32, self_idx (B,NQ,K) int32 rows of q, cross_idx (B,NQ,K) int32 rows of v"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, NQ, DIM, generator=g)
    v = torch.randn(B, NK, DIM, generator=g)
    self_idx = torch.randint(0, NQ, (B, NQ, K), generator=g).to(torch.int32)
    cross_idx = torch.randint(0, NK, (B, NQ, K), generator=g).to(torch.int32)
    return q, v, self_idx, cross_idx
