"""models.PointTransformer / PointTransformer_seg (the full fine-tuning baselines) on a GPU-less host: registry names, the reference's
state dicts, the shipped recipes, the torch formulation against the fixtures of the reference's own classes (tests/golden/finetune_cls.npz,
finetune_seg.npz and the two key lists, written by tools/gen_golden_finetune.py), fine-tuning from a Point_MAE checkpoint of this
repository, the evaluation loops' keyword rule, upp_hip.torch_cpu.tap_pool against tests/_norm_pool_reference.py, and the argument checks
of the new entry points (no device needed: they answer before any launch).

Fixture bound (README "The full fine-tuning baselines"): max(1e-5, 3 x err_ref) of the float64 output's maximum."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _finetune_case as case
import _norm_pool_reference as R
import _seeded
from conftest import GOLDEN, PKG
from upp_hip import _abi, torch_cpu


@pytest.fixture()
def cpu_ops(oracle_ops):
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    yield
    torch_cpu.enable(was)


def test_both_names_are_registered():
    from models import MODELS, Point_MAE_finetune, Point_MAE_segment
    assert MODELS.get("PointTransformer") is Point_MAE_finetune.PointTransformer
    assert MODELS.get("PointTransformer_seg") is Point_MAE_segment.PointTransformer_seg
    assert type(case.build("cls")) is Point_MAE_finetune.PointTransformer and type(case.build("seg")) is Point_MAE_segment.PointTransformer_seg
    assert isinstance(case.build("seg").get_loss, torch.nn.Module)


@pytest.mark.parametrize("kind, count", [("cls", 86), ("seg", 202)])
def test_state_dict_is_the_references_and_loads_strictly(kind, count):
    want = [(line.split()[0], tuple(int(s) for s in line.split()[1:])) for line in open(os.path.join(GOLDEN, case.KEYS[kind]))]
    sd = case.build(kind).state_dict()
    assert sorted((k, tuple(v.shape)) for k, v in sd.items()) == sorted(want) and len(want) == count
    changed = {k: torch.full(shape, 0.5).to(sd[k].dtype) for k, shape in want}          # a checkpoint made from the key list alone
    case.build(kind).load_state_dict(changed, strict=True)


@pytest.mark.parametrize("fname, name, cls_dim, groups, npoints", [
    ("finetune_modelnet_cls", "PointTransformer", 40, 64, 1024), ("finetune_scan_objonly_cls", "PointTransformer", 15, 128, 2048),
    ("finetune_shapenet55_cls", "PointTransformer", 55, 128, 1024), ("finetune_shapenetpart_seg", "PointTransformer_seg", 50, 128, 2048)])
def test_shipped_recipes_build_their_models(fname, name, cls_dim, groups, npoints):
    from models import build_model_from_cfg
    from utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file(os.path.join(PKG, "cfgs", fname + ".yaml"))
    assert cfg.model.NAME == name and cfg.npoints == npoints
    model = build_model_from_cfg(cfg.model)
    assert type(model).__name__ == name and model.cls_dim == cls_dim and model.num_group == groups and model.group_size == 32
    assert len(model.blocks.blocks) == 12 and model.trans_dim == 384 and all(p.requires_grad for p in model.parameters())
    last = model.cls_head_finetune[-1] if name == "PointTransformer" else model.seg_head[-1]
    assert last.weight.shape[0] == cls_dim


def test_segmentation_model_is_built_for_384_channels():
    with pytest.raises(ValueError, match="384"):
        case.build("seg", trans_dim=128, encoder_dims=128, num_heads=2)


@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_torch_formulation_on_cpu_meets_the_fixture_bound(kind, cpu_ops):
    fx = case.fixture(kind)
    assert int(fx["seed"]) == case.SEED[kind] and float(fx["gap"]) >= 1e-5
    model = _seeded.fill(case.build(kind)).eval()
    with torch.no_grad():
        out = case.forward(model, kind, case.inputs(kind))
    assert tuple(out.shape) == ((2, 40) if kind == "cls" else (2, 256, 50))
    case.check_output(fx, out, "cpu torch formulation, " + kind)
    if kind == "seg":
        assert torch.allclose(out.exp().sum(-1), torch.ones(2, 256), atol=1e-5)       # log-probabilities


@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_fine_tuning_starts_from_a_point_mae_checkpoint(kind, tmp_path):
    from models import build_model_from_cfg
    from utils.checkpoint import save_checkpoint
    from utils.config import EasyDict
    c = case.CFG[kind]
    tc = dict(mask_ratio=0.6, mask_type='rand', trans_dim=c["trans_dim"], encoder_dims=c["encoder_dims"], depth=c["depth"], drop_path_rate=0.1,
              num_heads=c["num_heads"], decoder_depth=2, decoder_num_heads=c["num_heads"])
    mae = _seeded.fill(build_model_from_cfg(EasyDict(dict(NAME="Point_MAE", group_size=c["group_size"], num_group=c["num_group"], loss="cdl2",
                                                         transformer_config=tc))))
    path = save_checkpoint(torch.nn.DataParallel(mae) if kind == "cls" else mae, None, 3, str(tmp_path / "ckpt" / "pretrain.pth"))
    model = case.build(kind)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    res = model.load_model_from_ckpt(path)
    sd, src = model.state_dict(), mae.state_dict()
    taken = [k for k in src if k.startswith("MAE_encoder.")]
    assert len(taken) > 40
    for k in taken:                                                  # encoder, blocks, pos_embed, norm
        assert torch.equal(sd[k[len("MAE_encoder."):]], src[k]), k
    for part in ("encoder.first_conv.0.weight", "blocks.blocks.0.attn.qkv.weight", "pos_embed.0.weight", "norm.weight"):
        assert "MAE_encoder." + part in taken
    head = "cls_head_finetune." if kind == "cls" else "seg_head."
    missing, unexpected = list(res.missing_keys), list(res.unexpected_keys)
    assert any(k.startswith(head) for k in missing) and "cls_token" in missing and "cls_pos" in missing
    assert not any(k.startswith(("encoder.", "blocks.", "pos_embed.", "norm.")) for k in missing)
    assert any(k.startswith("MAE_decoder.") for k in unexpected) and "mask_token" in unexpected and all(not k.startswith("MAE_encoder") for k in unexpected)
    for k in missing:
        assert torch.equal(sd[k], before[k]), k                       # what the checkpoint does not hold keeps its initialisation
    # from scratch: the reference's initialisation of every Linear / LayerNorm / Conv1d
    fresh = case.build(kind)
    assert fresh.load_model_from_ckpt(None) is None
    assert float(fresh.norm.weight.detach().min()) == 1.0 and float(fresh.norm.bias.detach().abs().max()) == 0.0
    assert float(fresh.pos_embed[0].bias.detach().abs().max()) == 0.0 and 0.005 < float(fresh.pos_embed[0].weight.detach().std()) < 0.04


@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_prompter_switches_are_accepted_off_and_refused_on(kind, cpu_ops):
    model = _seeded.fill(case.build(kind)).eval()
    pts = case.inputs(kind)
    with torch.no_grad():
        plain = case.forward(model, kind, pts)
        extra = (pts,) if kind == "cls" else (pts, case.one_hot())
        same = model(*extra, completion_prompt=False, denoise=False, point_num=pts.shape[1])
        assert torch.equal(plain, same)
        for kw in (dict(completion_prompt=True), dict(denoise=True), dict(completion_prompt=True, denoise=True, point_num=128)):
            with pytest.raises(ValueError, match="no prompter"):
                model(*extra, **kw)
        if kind == "seg":
            moved = model(pts, case.one_hot(), label_points=pts[:, :100].contiguous())
            assert tuple(moved.shape) == (2, 100, 50) and torch.allclose(moved, plain[:, :100], atol=1e-5)


def test_losses(cpu_ops):
    g = torch.Generator().manual_seed(0)
    logits, gt = torch.randn(6, 40, generator=g), torch.randint(0, 40, (6,), generator=g)
    loss, acc = case.build("cls").get_loss_acc(logits, gt)
    assert torch.allclose(loss, torch.nn.functional.cross_entropy(logits, gt)) and float(acc) == float((logits.argmax(-1) == gt).sum()) / 6 * 100
    logp = torch.log_softmax(torch.randn(30, 50, generator=g), -1)
    target = torch.randint(0, 50, (30,), generator=g)
    assert torch.allclose(case.build("seg").get_loss(logp, target), torch.nn.functional.nll_loss(logp, target))


# ============================================================================================== torch_cpu.tap_pool
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_tap_pool_torch_formulation_against_the_restatement(dtype):
    B, G, C = 2, 37, 12
    g = torch.Generator().manual_seed(4)
    f = [torch.randn(B, G, C, generator=g).to(dtype) * (k + 1) for k in range(3)]
    for t in f:
        t[:, 5] = t[:, 2]                                             # equal token rows: ties in every column
        t[:, 30] = t[:, 2]
    ln = torch.nn.LayerNorm(C).to(dtype)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(C, generator=g)); ln.bias.copy_(torch.randn(C, generator=g))
        x, gmax, gmean = torch_cpu.tap_pool(f[0], f[1], f[2], ln)
    npd = np.float32 if dtype == torch.float32 else np.float64
    rx, rmax, rarg, rmean, _, _ = R.tap_pool(*(t.numpy() for t in f), ln.weight.detach().numpy(), ln.bias.detach().numpy(), ln.eps, npd)
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    assert x.shape == (B, G, 3 * C) and np.abs(x.numpy() - rx).max() <= tol
    # the pooling of torch's own x, exactly: the token-order sum (not torch.mean's pairwise one) and the lowest index among equal maxima
    pmax, parg, pmean = R.pool(x.numpy())
    assert np.array_equal(gmax.numpy(), pmax) and np.array_equal(gmean.numpy(), pmean)
    assert not np.array_equal(gmean.numpy(), x.mean(1).numpy()) or dtype == torch.float64
    assert (parg[:, :] != 5).all() and (parg != 30).all() and (parg == 2).any()
    picked = torch.from_numpy(parg).long()
    assert torch.equal(x.gather(1, picked.unsqueeze(1)).squeeze(1), gmax)
    # the arg-max instrument takes the place of the max
    with torch.no_grad():
        _, forced, _ = torch_cpu.tap_pool(f[0], f[1], f[2], ln, pool=lambda y: y[:, 0])
    assert torch.equal(forced, x[:, 0])


def test_tap_pool_dispatch_on_cpu_tensors():
    from upp_hip import functional as HF
    f = torch.randn(2, 5, 8)
    ln = torch.nn.LayerNorm(8)
    assert not HF.tap_pool_usable(f, f, f, ln)
    HF._declined.clear()
    a, b = HF.tap_pool(f, f, f, ln), torch_cpu.tap_pool(f, f, f, ln)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and not HF._declined           # (a CPU tensor is not a DECLINED HIP tensor)


# ============================================================================================== argument checks, no device
def test_new_entry_points_check_their_arguments_before_any_launch():
    lib = _abi.load()
    E_BADARG, E_RANGE = -1, -2
    buf = (ctypes.c_float * 16)()                                    # a non-null host address: never dereferenced, the sizes are refused first
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda B, G, C, f0=p, arg=p: lib.upp_tap_pool_fwd(f0, p, p, p, p, 1e-5, p, p, arg, p, p, p, B, G, C, None)
    bwd = lambda B, G, C, part=p: lib.upp_tap_pool_bwd(p, p, p, p, p, p, p, p, p, p, part, p, p, p, p, p, B, G, C, None)
    assert fwd(2, 5, 8, f0=None) == E_BADARG and fwd(2, 5, 8, arg=None) == E_BADARG and bwd(2, 5, 8, part=None) == E_BADARG
    for B, G, C in ((0, 5, 8), (2, 0, 8), (2, 5, 0), (-1, 5, 8)):
        assert fwd(B, G, C) == E_BADARG and bwd(B, G, C) == E_BADARG and lib.upp_tap_pool_part_floats(B, G, C) == 0
    for B, G, C in ((65536, 5, 8), (2, 2049, 8), (2, 5, 516), (2, 5, 6), (2, 5, 2), (2, 5, 1024)):
        assert fwd(B, G, C) == E_RANGE and bwd(B, G, C) == E_RANGE and lib.upp_tap_pool_part_floats(B, G, C) == 0
    assert lib.upp_tap_pool_part_floats(2, 5, 8) == 3 * 2 * 8 and lib.upp_tap_pool_part_floats(32, 128, 384) == 1024 * 2 * 384
    assert lib.upp_tap_pool_part_floats(65535, 2048, 512) == (65535 * 2048 // 4) * 2 * 512
    cls = lambda B, L, D, gg=p: lib.upp_cls_pool_bwd_ln(p, p, p, p, p, p, p, gg, p, B, L, D, None)
    assert cls(2, 3, 8, gg=None) == E_BADARG and cls(0, 3, 8) == E_BADARG and cls(2, 1, 8) == E_BADARG and cls(2, 3, 0) == E_BADARG
    assert cls(2, 3, 513) == E_RANGE
    assert _abi.ABI_VERSION == 5 and lib.upp_abi_version() == 5
