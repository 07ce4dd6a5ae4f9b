"""models.PointTransformer / PointTransformer_seg on the GPU, fused path: the fixtures of the reference's own classes (the bound of
tests/test_finetune_models.py), one eval forward at each recipe's size, one training pass (launch list, gradients), the gradients against
the model's own float64 torch formulation on replayed choices, the recipes of upp_hip.recipes under upp_hip.train.TrainStep (captured
replays against eager steps, no memset), and the captured evaluation loops.

The float64 comparison uses the repository's instruments: upp_layers.POOL_TRACE records every discrete choice of an instrumented HIP run
(FPS picks, neighbour lists, the arg of every max, ReLU / LeakyReLU gates) and upp_layers.use_rng hands that run a uniform bank whose
draws are logged; the CPU evaluations of the torch formulation, in float32 and float64, replay the choices and are given the logged
uniforms at their DropPath and Dropout sites.  Under POOL_TRACE the pooled nodes (HF.cls_pool, HF.tap_pool) decline in favour of torch
operators whose arg-max goes through upp_layers.max_over -- their kernels are held to float64 on the same arg in
tests/test_gpu_norm_pool.py; everything else of the instrumented run (Linear layers, attention, the block row kernels, BatchNorm rows,
interpolation, losses) is the fused path.  Bound: max(5e-6, 3 x err_torch) of each gradient's float64 maximum, err_torch the CPU float32
evaluation's own error (tests/test_gpu_pointr.py)."""
import os
import sys

import pytest
import torch

import _finetune_case as case
import _seeded
from conftest import PKG, ROOT
from upp_hip import functional as HF

pytestmark = pytest.mark.gpu

RECIPE = {"cls": ("finetune_modelnet_cls", 1024), "seg": ("finetune_shapenetpart_seg", 2048)}


def recipe_model(kind):
    from models import build_model_from_cfg
    from utils.config import cfg_from_yaml_file
    cfg = cfg_from_yaml_file(os.path.join(PKG, "cfgs", RECIPE[kind][0] + ".yaml"))
    return _seeded.fill(build_model_from_cfg(cfg.model))


def recipe_inputs(kind, B, seed=2):
    N = RECIPE[kind][1]
    g = torch.Generator().manual_seed(seed)
    pts = _seeded.unit_ball_clouds(B, N, seed=seed).cuda()
    if kind == "cls":
        return [pts, torch.randint(0, 40, (B,), generator=g).cuda()]
    onehot = torch.nn.functional.one_hot(torch.randint(0, 16, (B,), generator=g), 16).float().cuda()
    return [pts, onehot, torch.randint(0, 50, (B * N,), generator=g).cuda()]


def loss_of(model, kind, inputs):
    """The model's pass without the recipe's metric: (loss, loss)"""
    if kind == "cls":
        return model.get_loss_acc(model(inputs[0]), inputs[1])
    logp = model(inputs[0], inputs[1])
    loss = model.get_loss(logp.reshape(-1, logp.shape[-1]), inputs[2])
    return loss, loss.detach()


def no_random_draws(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    return model


# ============================================================================================== fixtures, eval forwards
@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_fused_model_meets_the_fixture_bound(kind):
    fx = case.fixture(kind)
    model = _seeded.fill(case.build(kind)).cuda().eval()
    HF._declined.clear()
    with torch.no_grad():
        out = case.forward(model, kind, case.inputs(kind).cuda())
    assert not HF._declined, HF._declined
    case.check_output(fx, out, "gpu fused, " + kind)


@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_eval_forward_at_the_recipes_size(kind):
    model = recipe_model(kind).cuda().eval()
    inputs = recipe_inputs(kind, 2)
    HF._declined.clear()
    with torch.no_grad():
        out = model(inputs[0]) if kind == "cls" else model(inputs[0], inputs[1])
        again = model(inputs[0]) if kind == "cls" else model(inputs[0], inputs[1], completion_prompt=False, denoise=False, point_num=2048)
    assert not HF._declined, HF._declined
    assert tuple(out.shape) == ((2, 40) if kind == "cls" else (2, 2048, 50)) and torch.isfinite(out).all() and torch.equal(out, again)
    if kind == "seg":
        assert torch.allclose(out.exp().sum(-1), torch.ones(2, 2048, device="cuda"), atol=1e-5)


# ============================================================================================== one training pass
@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_one_training_pass(kind):
    """Forward + loss + backward of the shipped recipe in training mode (dropout and stochastic depth on) through the step driver's eager
    pass: the launches (no library GEMM, no sort, no torch reduction but the per-row arg-max of the segmentation recipe's point
    accuracy), the nodes of this pull request among them, an empty declined list, and a finite gradient
    on every parameter the forward reads (the segmentation model's cls_token / cls_pos are, as in the reference, constructed and unused)."""
    from upp_hip.train import TrainStep
    model = _seeded.fill(case.build(kind, group_size=32)).cuda().train()      # (groups of 32, the recipes' size: with 16 the patch embedding's per-group term is a broadcast add)
    inputs = [case.inputs(kind).cuda()] + ([torch.tensor([3, 17]).cuda()] if kind == "cls" else
                                           [case.one_hot(device="cuda"), torch.randint(0, 50, (2 * 256,), generator=torch.Generator().manual_seed(1)).cuda()])
    from upp_hip import recipes
    ts = TrainStep(model, tuple(inputs[0].shape), use_graph=False, loss_fn=recipes.finetune_cls if kind == "cls" else recipes.finetune_seg, inputs=inputs)
    ts._forward_backward()                                              # (warm-up: caches, the uniform bank's demand)
    HF._declined.clear()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        ts._forward_backward()
        torch.cuda.synchronize()
    assert not HF._declined, HF._declined
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    print("\n".join(names))
    argmax = [n for n in names if "reduce_kernel" in n and "ArgMaxOps" in n]       # the per-row arg-max of recipes.point_accuracy: the one torch reduction
    assert len(argmax) == (0 if kind == "cls" else 1), argmax
    for n in names:
        low = n.lower()
        assert "Cijk_" not in n and "gemm" not in low and "sort" not in low and ("reduce_kernel" not in n or n in argmax) and "memset" not in low, n
    want = ("cls_pool_fwd_kernel", "cls_pool_bwd_kernel", "cls_pool_param_grad_kernel") if kind == "cls" else \
        ("tap_pool_fwd_kernel", "tap_pool_bwd_kernel", "part_sum_kernel")
    for frag in want + ("rowln_fwd_kernel", "attn_"):
        assert any(frag in n for n in names), frag
    # (the step driver hands every parameter its window of the flat gradient buffer: one the pass never wrote is zero)
    without = sorted(n for n, p in model.named_parameters() if p.grad is None or float(p.grad.abs().max()) == 0.0)
    assert without == ([] if kind == "cls" else ["cls_pos", "cls_token"]), without
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())


class Draws:
    """The uniforms of one instrumented run, logged (a upp_layers.UniformBank under upp_layers.use_rng, and nn.Dropout modules), or handed
    to the torch formulation's DropPath and Dropout sites in the same order."""

    def __init__(self, monkeypatch, log=None):
        self.m, self.log, self.replay, self.pos = monkeypatch, ([] if log is None else log), log is not None, 0

    def next(self):
        item = self.log[self.pos]
        self.pos += 1
        return item

    def install(self):
        from models import upp_layers as L
        draws = self

        class Bank(L.UniformBank):
            def begin(self, device, training):
                self.buf = None

            def take(self, shape, device):
                u = torch.rand(shape, device=device)
                draws.log.append(u.detach().cpu())
                return u

        def dropout(mod, x):
            if not mod.training or mod.p == 0.0:
                return x
            if draws.replay:
                u = draws.next().to(device=x.device).reshape(x.shape)
            else:
                u = torch.rand(x.shape, device=x.device)
                draws.log.append(u.detach().cpu())
            return x * ((u >= mod.p).to(x.dtype) / (1.0 - mod.p))

        state = {}

        def sample_scale(mod, x):
            """Block.forward_fused draws one (2, B) tensor per block: row 0 scales the attention branch, row 1 the MLP branch"""
            if mod.drop_prob == 0. or not mod.training:
                return None
            if "u" not in state:
                state["u"] = draws.next()
                u = state["u"][0]
            else:
                u = state.pop("u")[1]
            keep = 1.0 - mod.drop_prob
            return ((u.to(device=x.device, dtype=torch.float32) + keep).floor() / keep).to(x.dtype).view((x.shape[0],) + (1,) * (x.dim() - 1))

        self.m.setattr(torch.nn.Dropout, "forward", dropout)
        if self.replay:
            self.m.setattr(L.DropPath, "sample_scale", sample_scale)
            return None
        return L.use_rng(Bank())


@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_training_gradients_against_float64_on_the_same_choices(kind, monkeypatch, oracle_ops):
    from models import upp_layers as L
    from upp_hip import torch_cpu
    # six clouds: a training-mode BatchNorm over the TWO rows of the fixture's batch (the heads, the label branch) maps every channel to
    # +-1 whatever the data and divides by the two samples' difference -- every f32 evaluation is then ill-conditioned there
    B = 6
    pts = _seeded.unit_ball_clouds(B, case.SHAPE[kind][1], seed=case.SEED[kind])
    g = torch.Generator().manual_seed(3)
    extra = [torch.tensor([3, 17, 0, 39, 21, 8])] if kind == "cls" else [case.one_hot((3, 11, 0, 15, 7, 3)), torch.randint(0, 50, (B * 256,), generator=g)]

    def grads(model, dtype, dev):
        model.zero_grad(set_to_none=True)
        a = [pts.to(dtype).to(dev)] + [t.to(dev) if t.dtype == torch.int64 else t.to(dtype).to(dev) for t in extra]
        loss, _ = loss_of(model, kind, a)
        loss.backward()
        return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}, float(loss)

    saved = dict(L.OPS)
    L.OPS.update(fps_gather=HF.fps_gather, knn_group=HF.knn_group)        # (the HIP grouping primitives, whatever a fixture put into the table)
    trace = {'mode': 'record', 'items': []}
    HF._declined.clear()
    try:
        with monkeypatch.context() as m:
            rec = Draws(m)
            with rec.install():
                L.POOL_TRACE = trace
                hip, loss_h = grads(_seeded.fill(case.build(kind)).cuda().train(), torch.float32, "cuda")
    finally:
        L.POOL_TRACE = None
        L.OPS.clear(); L.OPS.update(saved)
    sites = {k[0] for k, _ in trace['items']}
    assert {'group.fps', 'group.knn', 'encoder.pool1', 'encoder.pool2', 'cls.max' if kind == "cls" else 'seg.global_max'} <= sites, sites
    assert len(rec.log) >= (3 + 2 if kind == "cls" else 11 + 1), len(rec.log)      # (block 0 has no stochastic depth) + the head's dropout

    def cpu(dtype):
        was = torch_cpu.enabled()
        torch_cpu.enable(True)
        L.POOL_TRACE = {'mode': 'replay', 'items': trace['items']}
        try:
            with monkeypatch.context() as m:
                rep = Draws(m, rec.log)
                rep.install()
                out = grads(_seeded.fill(case.build(kind)).to(dtype).train(), dtype, "cpu")
            assert L.POOL_TRACE['pos'] == len(trace['items']) and rep.pos == len(rec.log)      # same sites, same order
        finally:
            L.POOL_TRACE = None
            torch_cpu.enable(was)
        return out
    (c32, loss32), (c64, loss64) = cpu(torch.float32), cpu(torch.float64)
    assert sorted(hip) == sorted(c32) == sorted(c64)
    assert abs(loss_h - loss64) <= max(5e-6, 3 * abs(loss32 - loss64) / abs(loss64)) * abs(loss64), (loss_h, loss32, loss64)
    scale = {n: t.abs().max().item() for n, t in c64.items()}
    worst, failures, zeros = ("", 0.0, 0.0), [], []
    for name in sorted(c64):
        unit = scale[name]
        wname = name[:-len("bias")] + "weight"
        if name.endswith(".bias") and wname in scale and unit <= 1e-9 * scale[wname]:
            # float64 evaluates this gradient to 0 (a bias in front of a training-mode BatchNorm): its own maximum is no scale, so the
            # errors are taken relative to the same layer's weight gradient (tests/test_gpu_pointr.py)
            unit = scale[wname]
            zeros.append(name)
        err_f = ((hip[name] - c64[name]).abs().max() / max(unit, 1e-30)).item()
        err_t = ((c32[name] - c64[name]).abs().max() / max(unit, 1e-30)).item()
        lim = max(5e-6, 3 * err_t)
        print("%s: hip against f64 %.3g, torch formulation against f64 %.3g, bound %.3g" % (name, err_f, err_t, lim))
        if err_f > worst[1]:
            worst = (name, err_f, err_t)
        if not err_f <= lim:
            failures.append((name, err_f, err_t))
    print("exactly 0 in float64: %s" % zeros)
    print("largest: %s hip %.3g (torch formulation %.3g)" % worst)
    assert not failures, failures


# ============================================================================================== the recipes under the step driver
@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_recipe_steps_replay_as_the_eager_steps_and_issue_no_memset(kind):
    """TrainStep with upp_hip.recipes at B = 4 and the recipe's size.  Three captured steps: finite losses; with every random draw
    switched off a step is a function of the weights and the batch, so the replays walk the eager driver's trajectory (the tolerance of
    tests/test_gpu_graph_safety.py: 2e-6 of the loss, 2e-5 of the gradient buffer's maximum); and the eager step issues no memset -- what
    a capture would turn into a memset node (that file's instrument, tools/memset_census.py)."""
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tools")) if p not in sys.path]
    from memset_census import memsets_of
    from upp_hip import recipes
    from upp_hip.train import TrainStep
    loss_fn = recipes.finetune_cls if kind == "cls" else recipes.finetune_seg
    inputs = recipe_inputs(kind, 4)
    runs = {}
    for use_graph in (False, True):
        model = no_random_draws(recipe_model(kind)).cuda().train()
        ts = TrainStep(model, tuple(inputs[0].shape), use_graph=use_graph, loss_fn=loss_fn, inputs=inputs)
        out = []
        for _ in range(3):
            loss = ts.step_inputs(*inputs)
            torch.cuda.synchronize()
            out.append((float(loss), ts.flat.flat.clone(), float(ts.flat.scalars[1])))
            assert torch.isfinite(ts.flat.flat).all() and float(ts.flat.flat.abs().max()) > 0.0
        runs[use_graph] = out
        if not use_graph:
            def step():
                ts._forward_backward()
                ts._update()
            found = memsets_of(step)
            assert not found, "memsets in the %s fine-tuning step:\n%s" % (kind, "\n".join("  %s %s | %s" % f for f in found))
    for k, ((le, ge, ae), (lg, gg, ag)) in enumerate(zip(runs[False], runs[True])):
        assert le == le and abs(le) < 1e6 and 0.0 <= ag <= 100.0
        assert abs(le - lg) <= 2e-6 * abs(le), (k, le, lg)
        scale = float(ge.abs().max())
        assert float((ge - gg).abs().max()) <= 2e-5 * scale, (k, float((ge - gg).abs().max()), scale)
        assert abs(ae - ag) <= 1e-3, (k, ae, ag)


def test_point_accuracy_is_the_share_of_hits():
    from upp_hip import recipes
    g = torch.Generator().manual_seed(0)
    logp = torch.log_softmax(torch.randn(70001, 50, generator=g), -1).cuda()
    target = torch.randint(0, 50, (70001,), generator=g).cuda()
    target[:30000] = logp[:30000].argmax(-1)
    want = float((logp.argmax(-1) == target).double().mean()) * 100.0
    got = recipes.point_accuracy(logp, target)
    assert got.shape == () and abs(float(got) - want) <= 1e-4 * want and want > 42.0


# ============================================================================================== captured evaluation loops
def test_captured_evaluation_loops_serve_the_new_models():
    from utils import evaluate
    g = torch.Generator().manual_seed(5)
    model = recipe_model("cls").cuda()
    batches = [(_seeded.unit_ball_clouds(3, 1200, seed=s).cuda(), torch.randint(0, 40, (3,), generator=g).cuda()) for s in (1, 2)]
    acc_e, pred_e = evaluate.validate(model, batches, 1024), None
    acc_c, pred_c = evaluate.validate_captured(model, batches, 1024, return_predictions=True)
    assert pred_c.shape == (6,) and abs(float(acc_e) - float(acc_c)) <= 1e-4
    seg = recipe_model("seg").cuda()
    label = torch.randint(0, 16, (2, 2), generator=g)
    batches = [(_seeded.unit_ball_clouds(2, 2048, seed=s).cuda(), label[i].cuda(), torch.randint(0, 50, (2, 2048), generator=g).cuda())
               for i, s in enumerate((3, 4))]
    out_e = evaluate.validate_seg(seg, batches)
    out_c = evaluate.validate_seg_captured(seg, batches)
    flat = lambda d: {k: v for k, v in d.items() if k != 'category_iou'} | {"iou " + k: v for k, v in d['category_iou'].items()}
    out_e, out_c = flat(out_e), flat(out_c)
    assert sorted(out_e) == sorted(out_c) and 0.0 <= out_c['accuracy'] <= 1.0
    for k in out_e:
        a, b = torch.tensor(out_e[k]).double(), torch.tensor(out_c[k]).double()
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-9, equal_nan=True), (k, out_e[k], out_c[k])
