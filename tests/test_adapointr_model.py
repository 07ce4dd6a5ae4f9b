"""models.AdaPoinTr (PCTransformer, SimpleRebuildFCLayer, AdaPoinTr) on a GPU-less host: the reference's state dicts, from_cfg and the
shipped config, what is not ported, misc.jitter_points, and the module's torch formulation against the fixture of the reference's own
class (tests/golden/adapointr.npz and the two key lists, written by tools/gen_golden_adapointr.py on the case of
tests/_adapointr_model_case.py).

The bound (README "The AdaPoinTr completion model"): every output and both losses are compared with the reference's FLOAT64 run; the
error, over the tensor's maximum, is at most max(1e-5, 3 x err_ref), err_ref being the reference's own f32-against-f64 error of that
tensor, computed here from the two stored arrays."""
import os

import numpy as np
import pytest
import torch

import _adapointr_model_case as case
import _seeded
from conftest import GOLDEN, PKG
from upp_hip import torch_cpu


def build(decoder_type='fc'):
    from models import AdaPoinTr
    from utils.config import EasyDict
    return AdaPoinTr.from_cfg(EasyDict(case.config(decoder_type)))


def run_modes(model_of, x, gt, seed, monkeypatch_ctx):
    """eval and train forward (+ losses) of a freshly seeded model with the fixture's jitter -> {mode: tuple of tensors}"""
    from utils import misc
    out = {}
    with monkeypatch_ctx as m:
        m.setattr(misc, "jitter_points", case.jitter(seed))
        for mode in ("eval", "train"):
            model = model_of().train(mode == "train")
            with torch.no_grad():
                ret = model(x)
                out[mode] = tuple(ret) + (tuple(model.get_loss(ret, gt)) if mode == "train" else ())
    return out


def check_runs(fixture, runs, who):
    errs = {}
    for name, got in zip(case.EVAL_OUTPUTS, runs["eval"]):
        errs["eval_" + name] = case.check_output(fixture, "eval_" + name, got, who)
    for name, got in zip(case.TRAIN_OUTPUTS, runs["train"]):
        errs["train_" + name] = case.check_output(fixture, "train_" + name, got, who)
    losses = np.array([float(v) for v in runs["train"][4:]])
    errs["train_loss"] = case.check_output(fixture, "train_loss", losses, who)
    return errs


@pytest.mark.parametrize("decoder_type, fname, count", [("fc", "adapointr_keys.txt", 143), ("fold", "adapointr_fold_keys.txt", 171)])
def test_state_dict_is_the_references_and_loads_strictly(decoder_type, fname, count):
    want = [(line.split()[0], tuple(int(s) for s in line.split()[1:])) for line in open(os.path.join(GOLDEN, fname))]
    model = build(decoder_type)
    sd = model.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want and len(want) == count
    changed = {k: torch.full(shape, 0.5).to(sd[k].dtype) for k, shape in want}          # a checkpoint made from the key list alone
    build(decoder_type).load_state_dict(changed, strict=True)


def test_from_cfg_builds_the_class_and_the_name_stays_unregistered():
    from models import AdaPoinTr, MODELS, PoinTr
    from utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file(os.path.join(PKG, "cfgs", "AdaPoinTr.yaml"))
    assert cfg.model.num_query == 512 and cfg.model.num_points == 8192 and cfg.model.decoder_type == 'fc'
    assert cfg.model.encoder_config.depth == len(cfg.model.encoder_config.block_style_list) == 6
    assert cfg.model.decoder_config.depth == len(cfg.model.decoder_config.cross_attn_block_style_list) == 8
    model = build()
    assert type(model) is AdaPoinTr.AdaPoinTr and isinstance(model.base_model, AdaPoinTr.PCTransformer)
    assert isinstance(model.decode_head, AdaPoinTr.SimpleRebuildFCLayer) and model.factor == 8
    fold = build('fold')
    assert AdaPoinTr.Fold is PoinTr.Fold and isinstance(fold.decode_head, PoinTr.Fold) and fold.factor == 64
    assert MODELS.get("AdaPoinTr") is None


def test_what_is_not_ported_raises_and_names_it():
    from models import AdaPoinTr
    from utils.config import EasyDict
    cfg = case.config()
    cfg["encoder_type"] = "pn"
    with pytest.raises(ValueError, match="'pn'"):
        AdaPoinTr.PCTransformer(EasyDict(cfg))
    with pytest.raises(ValueError, match="'pn'"):
        AdaPoinTr.from_cfg(EasyDict(cfg))
    cfg = case.config()
    cfg["decoder_type"] = "mlp"
    with pytest.raises(ValueError, match="decoder_type"):
        AdaPoinTr.AdaPoinTr(EasyDict(cfg))
    cfg = case.config()
    cfg["num_points"] = 250
    with pytest.raises(ValueError, match="num_points"):
        AdaPoinTr.AdaPoinTr(EasyDict(cfg))


def test_jitter_points():
    from utils import misc
    pc = _seeded.unit_ball_clouds(2, 64, seed=1)
    keep = pc.clone()
    a = misc.jitter_points(pc, generator=torch.Generator().manual_seed(5))
    b = misc.jitter_points(pc, generator=torch.Generator().manual_seed(5))
    assert torch.equal(pc, keep) and a is not pc and torch.equal(a, b) and a.shape == pc.shape and a.dtype == pc.dtype
    d = a - pc
    assert 0 < d.abs().max() <= 0.05 + 1e-7 and 0.005 < d.std() < 0.015
    wide = misc.jitter_points(pc, std=1.0, clip=0.05, generator=torch.Generator().manual_seed(5)) - pc
    assert wide.abs().max() <= 0.05 + 1e-7 and (wide.abs() > 0.0499).float().mean() > 0.5
    assert torch.equal(misc.jitter_points(pc, std=0.0), pc)
    with pytest.raises(ValueError):
        misc.jitter_points(pc, std=-1.0)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "adapointr.npz"))


@pytest.fixture(scope="module")
def cpu_runs(fixture):
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    try:
        seed = int(fixture["seed"])
        x, gt = case.inputs(seed)
        return run_modes(lambda: _seeded.fill(build()), x, gt, seed, pytest.MonkeyPatch.context())
    finally:
        torch_cpu.enable(was)


def test_torch_formulation_on_cpu_meets_the_fixture_bound(fixture, cpu_runs):
    assert int(fixture["seed"]) == 14
    assert [tuple(t.shape) for t in cpu_runs["eval"]] == [(2, 32, 3), (2, 256, 3)]
    assert [tuple(t.shape) for t in cpu_runs["train"][:4]] == [(2, 32, 3), (2, 64, 3), (2, 512, 3), (2, 256, 3)]
    check_runs(fixture, cpu_runs, "cpu torch formulation")


def test_training_mode_needs_64_input_points():
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    try:
        model = build().train()
        with pytest.raises(ValueError, match="64"):
            model(_seeded.unit_ball_clouds(1, 63, seed=0))
    finally:
        torch_cpu.enable(was)


@pytest.mark.parametrize("with_t, with_u", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("act", [None, 'gelu'])
def test_expand_add_is_the_linear_over_the_concatenation(with_t, with_u, act):
    """models.AdaPoinTr.expand_add against a float64 evaluation that builds [f repeated ; x ; u] and multiplies it by W = [Wf | Wx | Wu]"""
    import torch.nn.functional as F
    from models.AdaPoinTr import expand_add
    R, S, G, C, J, O = 3, 5, 16, (8 if with_t else 0), (3 if with_u else 0), 24
    g = torch.Generator().manual_seed(1)
    f, x, u = torch.randn(R, G, generator=g), torch.randn(R, S, C, generator=g), torch.randn(R, S, J, generator=g)
    W, b = torch.randn(O, G + C + J, generator=g) / (G + C + J) ** 0.5, torch.randn(O, generator=g)
    want = F.linear(torch.cat([f.unsqueeze(1).expand(-1, S, -1), x, u], dim=-1).double(), W.double(), b.double())
    want = F.gelu(want) if act else want
    for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 1e-5)):
        Wd = W.to(dtype)
        P = F.linear(f.to(dtype), Wd[:, :G], b.to(dtype))
        T = F.linear(x.to(dtype), Wd[:, G:G + C]) if with_t else None
        got = expand_add(P, T, u.to(dtype) if with_u else None, Wd[:, G + C:] if with_u else None, act)
        assert got.shape == (R, S, O) and got.dtype == dtype
        assert (got.double() - want).abs().max().item() <= tol * want.abs().max().item()
    with pytest.raises(ValueError, match="at least one"):
        expand_add(P)
    with pytest.raises(ValueError, match="act"):
        expand_add(P, T if with_t else P.unsqueeze(1), act='relu')


def test_simple_rebuild_fc_layer_is_the_mlp_over_the_concatenation():
    from models.AdaPoinTr import SimpleRebuildFCLayer
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    try:
        head = _seeded.fill(SimpleRebuildFCLayer(48, step=5, hidden_dim=20)).double()
        x = torch.randn(3, 7, 24, generator=torch.Generator().manual_seed(0), dtype=torch.float64, requires_grad=True)
        got = head(x)
        cat = torch.cat([x.max(1)[0].unsqueeze(1).expand(-1, 7, -1), x], dim=-1)
        want = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(cat, head.layer.fc1.weight, head.layer.fc1.bias)),
                                          head.layer.fc2.weight, head.layer.fc2.bias).reshape(3, 7, 5, 3)
        assert got.shape == (3, 7, 5, 3) and torch.allclose(got, want, rtol=1e-12, atol=1e-13)
        with pytest.raises(ValueError, match="channels"):
            head(x[..., :20])
    finally:
        torch_cpu.enable(was)
