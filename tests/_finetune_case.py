"""The cases of tests/golden/finetune_cls.npz and finetune_seg.npz (tools/gen_golden_finetune.py), shared by tests/test_finetune_models.py
and tests/test_gpu_finetune_models.py: configurations, inputs regenerated from the stored seed, and the fixture bound."""
import os

import numpy as np
import torch

import _seeded
from conftest import GOLDEN

CFG = {
    "cls": dict(trans_dim=128, depth=4, drop_path_rate=0.1, cls_dim=40, num_heads=2, group_size=16, num_group=16, encoder_dims=128),
    "seg": dict(trans_dim=384, depth=12, drop_path_rate=0.1, cls_dim=50, num_heads=6, group_size=16, num_group=32, encoder_dims=384),
}
SHAPE = {"cls": (2, 128), "seg": (2, 256)}
SEED = {"cls": 0, "seg": 1}
NAME = {"cls": "PointTransformer", "seg": "PointTransformer_seg"}
KEYS = {"cls": "pointtransformer_keys.txt", "seg": "pointtransformer_seg_keys.txt"}
LABELS = (3, 11)


def config(kind, **over):
    from utils.config import EasyDict
    return EasyDict(dict(CFG[kind], NAME=NAME[kind], **over))


def build(kind, **over):
    from models import build_model_from_cfg
    return build_model_from_cfg(config(kind, **over))


def fixture(kind):
    return np.load(os.path.join(GOLDEN, "finetune_%s.npz" % kind))


def inputs(kind, seed=None):
    B, N = SHAPE[kind]
    return _seeded.unit_ball_clouds(B, N, seed=SEED[kind] if seed is None else seed)


def one_hot(labels=LABELS, device="cpu", dtype=torch.float32):
    return torch.nn.functional.one_hot(torch.tensor(labels), 16).to(device=device, dtype=dtype)


def forward(model, kind, pts):
    if kind == "cls":
        return model(pts)
    return model(pts, one_hot(device=pts.device, dtype=pts.dtype))


def check_output(fx, got, who):
    """|got - reference f64| / max|reference f64| <= max(1e-5, 3 x err_ref): the bound of tests/test_adapointr_model.py, err_ref the
    reference's own f32-against-f64 error computed from the two stored arrays."""
    r64 = fx["out_f64"]
    scale = np.abs(r64).max()
    err_ref = np.abs(fx["out_f32"].astype(np.float64) - r64).max() / scale
    assert abs(err_ref - float(fx["err_ref"])) <= 1e-12
    got = got.detach().double().cpu().numpy()
    assert got.shape == r64.shape and np.isfinite(got).all()
    err = np.abs(got - r64).max() / scale
    lim = max(1e-5, 3 * err_ref)
    print("%s: error %.3g of the maximum, reference's own %.3g, bound %.3g" % (who, err, err_ref, lim))
    assert err <= lim, (who, err, err_ref, lim)
    return err
