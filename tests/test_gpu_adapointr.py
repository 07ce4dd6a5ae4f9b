"""models.AdaPoinTr on the GPU, fused path: the model against the fixture of the reference's own class (tests/golden/adapointr.npz; the
bound of tests/test_adapointr_model.py), the launches and the gradients of one training step, and every output and parameter gradient
against the module's own float64 torch formulation with the discrete choices replayed (the instrument and the bound
max(5e-6, 3 x err_torch) of tests/test_gpu_pointr.py).

The torch formulation on the device is the SAME module with HF.query_select_usable switched off: the selection then runs torch
operators (upp_hip.torch_cpu.query_select) and says so through HF.note_declined."""
import copy
import os

import numpy as np
import pytest
import torch

import _adapointr_model_case as case
import _seeded
from conftest import GOLDEN
from test_adapointr_model import build, check_runs, run_modes
from test_gpu_pointr import Choices
from upp_hip import functional as HF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "adapointr.npz"))


def test_fused_model_meets_the_fixture_bound(fixture):
    seed = int(fixture["seed"])
    x, gt = (t.cuda() for t in case.inputs(seed))
    HF._declined.clear()
    runs = run_modes(lambda: _seeded.fill(build()).cuda(), x, gt, seed, pytest.MonkeyPatch.context())
    assert not HF._declined, HF._declined                                # the declined-path list is empty for the fixture configuration
    check_runs(fixture, runs, "gpu fused")


def test_fold_head_runs_fused():
    model = _seeded.fill(build('fold')).cuda().eval()
    x = case.inputs(3)[0].cuda()
    HF._declined.clear()
    with torch.no_grad():
        coarse, rebuild = model(x)
    assert not HF._declined, HF._declined
    assert coarse.shape == (2, 32, 3) and rebuild.shape == (2, 32 * 64, 3) and torch.isfinite(rebuild).all()


def test_one_training_step(monkeypatch, fixture):
    """Forward + both losses + backward at the fixture size, in training mode: the launches (no library GEMM, no sort, no scatter), the
    declined list, finite gradients everywhere but on query_ranking, whose only use is an integer order."""
    from utils import misc
    seed = int(fixture["seed"])
    monkeypatch.setattr(misc, "jitter_points", case.jitter(seed))
    model = _seeded.fill(build()).cuda().train()
    x, gt = (t.cuda() for t in case.inputs(seed))

    def run():
        model.zero_grad(set_to_none=True)
        ret = model(x)
        loss_denoised, loss_recon = model.get_loss(ret, gt)
        (loss_denoised + loss_recon).backward()

    run()                                                               # (warm-up: caches, lazy initialisation)
    HF._declined.clear()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    assert not HF._declined, HF._declined
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    print("\n".join(names))
    for n in names:
        low = n.lower()
        assert "Cijk_" not in n and "gemm" not in low and "sort" not in low and "scatter" not in low and "topk" not in low, n
    for frag in ("qs_fwd_kernel", "qs_bwd_kernel", "xattn_prefix_fwd_kernel", "ec_", "knn", "fps"):
        assert any(frag in n for n in names), frag
    without = sorted(n for n, p in model.named_parameters() if p.grad is None)
    ranking = sorted(n for n, _ in model.named_parameters() if n.startswith("base_model.query_ranking."))
    assert len(ranking) == 6 and set(ranking) <= set(without)
    # besides the ranking MLP only the encoder's final norm has none: constructed for its state-dict keys and, as in the reference, not applied
    assert set(without) - set(ranking) == {"base_model.encoder.norm.weight", "base_model.encoder.norm.bias"}, without
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


class ModelChoices(Choices):
    """test_gpu_pointr.Choices plus the one discrete choice AdaPoinTr adds: the order of the query selection."""

    def install(self):
        super().install()
        from models import AdaPoinTr as MA
        from upp_hip import torch_cpu
        rec = not self.replay

        def query_select(score, cand, Q, extra, site):
            if rec:
                fn = HF.query_select if HF.query_select_usable(score, cand, Q, extra) else torch_cpu.query_select
                if fn is torch_cpu.query_select:
                    HF.note_declined("%s query_select" % site, "switched off")
                out, order = fn(score, cand, Q, extra)
                self.put("order", order.clone())
                return out
            out = torch.gather(cand, 1, self.get("order").long().unsqueeze(-1).expand(-1, -1, 3))
            return out if extra is None else torch.cat([out, extra], dim=1)

        self.m.setattr(MA, "query_select", query_select)


def test_training_outputs_and_gradients_against_float64_on_the_same_choices(monkeypatch, fixture):
    """Training mode, the whole model at the fixture size, fixed cotangents on the four outputs.  The fused f32 run and the
    torch-formulation f32 run each record their discrete choices (neighbour lists, FPS picks, the arg of every max, the branch of every
    LeakyReLU, the selection's order); the module in float64 -- torch operators only -- is evaluated on the recorded choices of each.
    Every output and parameter gradient of the fused run must be within max(5e-6, 3 x err_torch) of its float64 evaluation, relative to
    that tensor's maximum, err_torch being the torch formulation's own f32-against-f64 error of the same tensor."""
    from utils import misc
    seed = int(fixture["seed"])
    monkeypatch.setattr(misc, "jitter_points", case.jitter(seed))
    model = _seeded.fill(build()).cuda().train()
    x = case.inputs(seed)[0].cuda()
    g = torch.Generator().manual_seed(12)
    cot = [torch.randn(2, n, 3, generator=g).cuda() for n in (32, 64, 512, 256)]
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model64 = copy.deepcopy(model).double()

    def run(net, dtype):
        net.zero_grad(set_to_none=True)
        ret = net(x.to(dtype))
        torch.autograd.backward(list(ret), [c.to(dtype) for c in cot])
        return [(n, t.detach()) for n, t in zip(case.TRAIN_OUTPUTS, ret)] + [(n + ".grad", p.grad.clone()) for n, p in net.named_parameters()
                                                                            if p.grad is not None]

    def with_float64(fused):
        model.load_state_dict(state)
        HF._declined.clear()
        with monkeypatch.context() as m:
            if not fused:
                m.setattr(HF, "query_select_usable", lambda *a, **k: False)
            rec = ModelChoices(m)
            rec.install()
            f32 = run(model, torch.float32)
        assert bool(HF._declined) != fused, HF._declined
        with monkeypatch.context() as m:
            rep = ModelChoices(m, rec.items)
            rep.install()
            f64 = run(model64, torch.float64)
        assert rep.pos == len(rec.items)
        HF._declined.clear()
        return f32, f64

    run(model, torch.float32)                                           # (warm-up)
    fused, fused64 = with_float64(True)
    plain, plain64 = with_float64(False)
    model.zero_grad(set_to_none=True)
    assert [n for n, _ in fused] == [n for n, _ in fused64] == [n for n, _ in plain] == [n for n, _ in plain64]
    assert not any(n.startswith("base_model.query_ranking.") for n, _ in fused)
    scale = {n: t.abs().max().item() for n, t in fused64}
    scale_t = {n: t.abs().max().item() for n, t in plain64}
    worst, failures, zeros = ("", 0.0, 0.0), [], []
    for (name, a), (_, a64), (_, b), (_, b64) in zip(fused, fused64, plain, plain64):
        assert torch.isfinite(a).all(), name
        unit, unit_t = scale[name], scale_t[name]
        wname = name.replace(".bias.grad", ".weight.grad")
        if name.endswith(".bias.grad") and wname in scale and unit <= 1e-9 * scale[wname] and unit_t <= 1e-9 * scale_t[wname]:
            # float64 evaluates this gradient to 0 (a constant per channel in front of a training-mode BatchNorm, or a key bias in front
            # of a softmax): its own maximum is no scale, so the errors are taken relative to the same layer's weight gradient
            unit, unit_t = scale[wname], scale_t[wname]
            zeros.append(name)
        err_f = ((a.double() - a64).abs().max() / max(unit, 1e-30)).item()
        err_t = ((b.double() - b64).abs().max() / max(unit_t, 1e-30)).item()
        lim = max(5e-6, 3 * err_t)
        print("%s: fused against f64 %.3g, torch formulation against f64 %.3g, bound %.3g" % (name, err_f, err_t, lim))
        if err_f > worst[1]:
            worst = (name, err_f, err_t)
        if not err_f <= lim:
            failures.append((name, err_f, err_t))
    print("exactly 0 in float64: %s" % zeros)
    print("largest: %s fused %.3g (torch formulation %.3g)" % worst)
    assert not failures, failures
