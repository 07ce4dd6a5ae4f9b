"""models.PoinTr on a GPU-less host: the reference's state dict, the registry, the shipped config, and the module's torch formulation
against the fixture of the reference's own class (tests/golden/pointr.npz and pointr_keys.txt, written by tools/gen_golden_pointr.py).

The bound (README "The PoinTr completion model"): every output is compared with the reference's FLOAT64 run; its error, over the
output's maximum, is at most max(1e-5, 3 x err_ref), err_ref being the reference's own f32-against-f64 error of that output, computed
here from the two stored arrays -- two f32 evaluations that sum in different orders each land anywhere inside the same rounding
envelope.  Measured for the torch formulation on the CPU: eval 4.3e-7 (coarse), 5.6e-7 (rebuild); train 6.2e-7 (coarse), 1.8e-5 (rebuild, bound
3.9e-5); the fused path on an MI355X (tests/test_gpu_pointr.py): 4.4e-7, 5.7e-7, 5.7e-7 and 1.4e-5."""
import os

import numpy as np
import pytest
import torch

import _seeded
from conftest import GOLDEN
from upp_hip import torch_cpu

CONFIG = dict(NAME="PoinTr", trans_dim=384, knn_layer=1, num_pred=512, num_query=32)


def bound(fixture, mode, name):
    r32, r64 = fixture["%s_%s_f32" % (mode, name)], fixture["%s_%s_f64" % (mode, name)]
    err_ref = np.abs(r32 - r64).max() / np.abs(r64).max()
    return max(1e-5, 3 * err_ref), err_ref


def check_outputs(fixture, mode, coarse, rebuild, who):
    for name, got in (("coarse", coarse), ("rebuild", rebuild)):
        r64 = fixture["%s_%s_f64" % (mode, name)]
        lim, err_ref = bound(fixture, mode, name)
        err = np.abs(got.detach().double().cpu().numpy() - r64).max() / np.abs(r64).max()
        print("%s %s %s: error / maximum = %.3g (reference f32: %.3g, bound %.3g)" % (who, mode, name, err, err_ref, lim))
        assert got.shape == r64.shape and err <= lim, (mode, name, err, lim)


def build():
    from utils.config import EasyDict
    from models import build_model_from_cfg
    return build_model_from_cfg(EasyDict(CONFIG))


def test_state_dict_is_the_references():
    want = [(line.split()[0], tuple(int(s) for s in line.split()[1:])) for line in open(os.path.join(GOLDEN, "pointr_keys.txt"))]
    sd = build().state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want and len(want) == 408


def test_registry_and_config():
    from models import MODELS, build_model_from_cfg
    from models.PoinTr import Fold, PoinTr
    from models.Transformer import Attention, Block, CrossAttention, DecoderBlock, Mlp, PCTransformer
    from models import upp_layers
    from utils.config import cfg_from_yaml_file
    from conftest import PKG
    assert MODELS.get("PoinTr") is PoinTr
    assert (CrossAttention, DecoderBlock, Attention, Mlp) == (upp_layers.CrossAttention, upp_layers.DecoderBlock, upp_layers.Attention,
                                                              upp_layers.Mlp) and Block is not upp_layers.Block
    cfg = cfg_from_yaml_file(os.path.join(PKG, "cfgs", "PoinTr.yaml"))
    assert dict(cfg.model) == dict(NAME="PoinTr", trans_dim=384, knn_layer=1, num_pred=14336, num_query=224)
    model = build_model_from_cfg(cfg.model)
    assert isinstance(model, PoinTr) and isinstance(model.base_model, PCTransformer) and isinstance(model.foldingnet, Fold)
    assert model.fold_step == 8 and model.foldingnet.folding_seed.shape == (2, 64) and not list(model.foldingnet.buffers(recurse=False))
    assert [k for k, _ in model.base_model.encoder[0].named_children()] == ["norm1", "attn", "drop_path", "norm2", "knn_map", "merge_map", "mlp"]


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "pointr.npz"))


@pytest.fixture(scope="module")
def cpu_runs(fixture):
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    try:
        x = _seeded.unit_ball_clouds(2, 640, seed=int(fixture["seed"]))
        out = {}
        for mode in ("eval", "train"):
            model = _seeded.fill(build()).train(mode == "train")
            with torch.no_grad():
                ret = model(x)
                out[mode] = ret + (tuple(model.get_loss(ret, x)) if mode == "train" else ())
    finally:
        torch_cpu.enable(was)
    return out


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_torch_formulation_on_cpu_meets_the_fixture_bound(fixture, cpu_runs, mode):
    assert int(fixture["seed"]) == 4
    check_outputs(fixture, mode, cpu_runs[mode][0], cpu_runs[mode][1], "cpu torch formulation")


def test_train_mode_losses(fixture, cpu_runs):
    """Chamfer-L1 of the two train-mode outputs against the input: a mean over thousands of distances of outputs that meet the bound
    above -> 1e-5 relative, the project's bound for a model output."""
    got = np.array([float(v) for v in cpu_runs["train"][2:]])
    print("losses %s, reference f64 %s, f32 %s" % (got, fixture["train_loss_f64"], fixture["train_loss_f32"]))
    assert np.abs(got - fixture["train_loss_f64"]).max() <= 1e-5 * np.abs(fixture["train_loss_f64"]).max()


def test_fold_keeps_the_references_layout():
    from models.PoinTr import Fold
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    try:
        fold = _seeded.fill(Fold(24, step=3, hidden_dim=16)).eval()
        x = torch.randn(5, 24, generator=torch.Generator().manual_seed(0))
        with torch.no_grad():
            got = fold(x)
            seed = fold.folding_seed.view(1, 2, 9).expand(5, 2, 9)
            feat = x.view(5, 24, 1).expand(5, 24, 9)
            fd1 = fold.folding1(torch.cat([seed, feat], 1))
            want = fold.folding2(torch.cat([fd1, feat], 1))
        assert got.shape == (5, 3, 9) and torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    finally:
        torch_cpu.enable(was)
