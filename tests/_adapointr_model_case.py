"""The case of tests/golden/adapointr.npz, shared by its generator (tools/gen_golden_adapointr.py: the reference's own AdaPoinTr) and by
the tests of this repository's class.  Encoder and decoder: dim 128, depth 2, 2 heads, k = 8, styles ['attn-graph', 'attn'], concat;
32 queries rebuilt into 256 points (8 per query), centres [64, 32], a 256-wide global feature, the graph encoder; weights from
tests/_seeded.fill; input unit_ball_clouds(2, 128, seed), ground truth unit_ball_clouds(2, 256, seed + 1000).

Training mode jitters its 64 denoising picks with misc.jitter_points, which the reference tree calls and does not define: both sides
take `jitter(seed)` below for it -- normal noise, std 0.01, clipped at 0.05, from a seeded CPU generator in float32 whatever the run's
precision, so that the reference's f32 and f64 runs and ours all add the same numbers."""
import numpy as np
import torch

import _seeded

DIM, DEPTH, HEADS, K, B, N, NGT = 128, 2, 2, 8, 2, 128, 256
NUM_QUERY, NUM_POINTS, CENTERS, GLOBAL_DIM, DENOISE = 32, 256, [64, 32], 256, 64
STYLES = ['attn-graph', 'attn']
EVAL_OUTPUTS = ("coarse", "rebuild")
TRAIN_OUTPUTS = ("pred_coarse", "denoised_coarse", "denoised_fine", "pred_fine")


def config(decoder_type='fc'):
    """the model section as plain dicts (wrap it in the EasyDict of whichever tree builds the class)"""
    return dict(NAME='AdaPoinTr', num_query=NUM_QUERY, num_points=NUM_POINTS, center_num=list(CENTERS), global_feature_dim=GLOBAL_DIM,
                encoder_type='graph', decoder_type=decoder_type,
                encoder_config=dict(embed_dim=DIM, depth=DEPTH, num_heads=HEADS, k=K, block_style_list=list(STYLES), combine_style='concat'),
                decoder_config=dict(embed_dim=DIM, depth=DEPTH, num_heads=HEADS, k=K, self_attn_block_style_list=list(STYLES),
                                    self_attn_combine_style='concat', cross_attn_block_style_list=list(STYLES),
                                    cross_attn_combine_style='concat'))


def inputs(seed):
    """-> xyz (B,N,3), gt (B,NGT,3), f32 CPU"""
    return _seeded.unit_ball_clouds(B, N, seed=seed), _seeded.unit_ball_clouds(B, NGT, seed=seed + 1000)


def jitter(seed, std=0.01, clip=0.05):
    """-> the jitter_points both sides use: pc + the same seeded noise on every call, in pc's precision and on pc's device"""
    def jitter_points(pc, *args, **kwargs):
        g = torch.Generator().manual_seed(int(seed) + 77)
        noise = (torch.randn(tuple(pc.shape), generator=g) * std).clamp_(-clip, clip)
        return pc + noise.to(device=pc.device, dtype=pc.dtype)
    return jitter_points


def bound(fixture, name):
    """the fixture rule: (max(1e-5, 3 x err_ref), err_ref), err_ref the reference's own f32-against-f64 error over the output's maximum"""
    r32, r64 = fixture[name + "_f32"], fixture[name + "_f64"]
    err_ref = np.abs(r32.astype(np.float64) - r64).max() / np.abs(r64).max()
    return max(1e-5, 3 * err_ref), err_ref


def check_output(fixture, name, got, who):
    r64 = fixture[name + "_f64"]
    lim, err_ref = bound(fixture, name)
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    err = np.abs(got - r64).max() / np.abs(r64).max()
    print("%s %s: error / maximum = %.3g (reference f32: %.3g, bound %.3g)" % (who, name, err, err_ref, lim))
    assert got.shape == r64.shape and err <= lim, (name, err, lim)
    return err
