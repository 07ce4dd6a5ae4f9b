"""The cases of tests/golden/adapointr_blocks.npz, shared by their generator (tools/gen_golden_adapointr_blocks.py: the reference's own
classes) and by the tests of this repository's classes (`ns` is the module that holds the classes: the reference's models.AdaPoinTr or
ours).  dim 128, 2 heads (head_dim 64), k = 8, B = 2, eval mode, weights from tests/_seeded.fill:
    a   PointTransformerDecoder, depth 2, styles ['attn-graph', 'attn'] for both lists, concat, 32 + 8 queries over 24 memory tokens,
        denoise_length = 8
    b   the same decoder, denoise_length = None
    c   PointTransformerEncoder, depth 2, ['attn-graph', 'attn'], concat, on the 24 tokens
    d   one CrossAttnBlockApi, 'attn-graph' with onebyone on both sides, denoise_length = 8
Features come from one seeded CPU generator, positions from unit_ball_clouds (40 query positions, 24 memory positions)."""
import numpy as np
import torch

import _seeded

DIM, HEADS, K, B, NQ, NK, D = 128, 2, 8, 2, 40, 24, 8
STYLES = ['attn-graph', 'attn']
CASES = ("a", "b", "c", "d")


def inputs(seed):
    """-> q (B,NQ,DIM), v (B,NK,DIM), q_pos (B,NQ,3), v_pos (B,NK,3), all f32 CPU"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, NQ, DIM, generator=g)
    v = torch.randn(B, NK, DIM, generator=g)
    return q, v, _seeded.unit_ball_clouds(B, NQ, seed=seed), _seeded.unit_ball_clouds(B, NK, seed=seed + 1000)


def module(ns, case):
    """the seeded eval-mode module of a case"""
    if case in ("a", "b"):
        m = ns.PointTransformerDecoder(embed_dim=DIM, depth=2, num_heads=HEADS, self_attn_block_style_list=STYLES,
                                       self_attn_combine_style='concat', cross_attn_block_style_list=STYLES,
                                       cross_attn_combine_style='concat', k=K)
    elif case == "c":
        m = ns.PointTransformerEncoder(embed_dim=DIM, depth=2, num_heads=HEADS, block_style_list=STYLES, combine_style='concat', k=K)
    else:
        m = ns.CrossAttnBlockApi(DIM, HEADS, self_attn_block_style='attn-graph', self_attn_combine_style='onebyone',
                                 cross_attn_block_style='attn-graph', cross_attn_combine_style='onebyone', k=K)
    return _seeded.fill(m).eval()


def run(m, case, q, v, q_pos, v_pos):
    if case == "c":
        return m(v, v_pos)
    return m(q, v, q_pos, v_pos, denoise_length=None if case == "b" else D)


def bound(fixture, name):
    """the fixture rule: (max(1e-5, 3 x err_ref), err_ref), err_ref the reference's own f32-against-f64 error over the output's maximum"""
    r32, r64 = fixture[name + "_f32"], fixture[name + "_f64"]
    err_ref = np.abs(r32 - r64).max() / np.abs(r64).max()
    return max(1e-5, 3 * err_ref), err_ref


def check_output(fixture, name, got, who):
    r64 = fixture[name + "_f64"]
    lim, err_ref = bound(fixture, name)
    err = np.abs(got.detach().double().cpu().numpy() - r64).max() / np.abs(r64).max()
    print("%s case %s: error / maximum = %.3g (reference f32: %.3g, bound %.3g)" % (who, name, err, err_ref, lim))
    assert got.shape == r64.shape and err <= lim, (name, err, lim)
    return err
