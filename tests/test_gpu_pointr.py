"""models.PoinTr on the GPU: the fused model against the fixture of the reference's own class (tests/golden/pointr.npz; the bound of
tests/test_pointr_model.py), the fused expand sites against the torch formulation on the same device (the gradient bounds of
tests/test_gpu_edge_conv.py), and the launches of one training step.

The torch formulation on the device is the SAME module with HF.expand_usable switched off: the three expand sites then build y with
torch operators (upp_hip.torch_cpu.expand_act) and say so through HF.note_declined.  Nothing in front of the first expand site
(mlp_query) depends on one, so the three neighbour searches, the FPS picks and the grouper's lists are the same in both runs without
being replayed."""
import os
import re

import numpy as np
import pytest
import torch

import _seeded
from conftest import GOLDEN
from test_pointr_model import CONFIG, build, check_outputs
from upp_hip import functional as HF

pytestmark = pytest.mark.gpu


def close(a, b, rtol=2e-5, atol_scale=5e-6):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol_scale * max(np.abs(b).max(), 1e-30))


def scaled_error(got, want):
    return ((got.detach().double() - want.detach().double()).abs().max() / want.detach().double().abs().max().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "pointr.npz"))


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_fused_model_meets_the_fixture_bound(fixture, mode):
    model = _seeded.fill(build()).cuda().train(mode == "train")
    x = _seeded.unit_ball_clouds(2, 640, seed=int(fixture["seed"])).cuda()
    HF._declined.clear()
    with torch.no_grad():
        coarse, rebuild = model(x)
        losses = model.get_loss((coarse, rebuild), x)
    assert not HF._declined, HF._declined
    check_outputs(fixture, mode, coarse, rebuild, "gpu fused")
    if mode == "train":
        got = np.array([float(v) for v in losses])
        print("losses %s, reference f64 %s" % (got, fixture["train_loss_f64"]))
        assert np.abs(got - fixture["train_loss_f64"]).max() <= 1e-5 * np.abs(fixture["train_loss_f64"]).max()


def both_ways(monkeypatch, module, run):
    """run() on the fused path and on the torch formulation (same module, same device) -> two lists of (name, tensor)."""
    HF._declined.clear()
    fused = run()
    assert not HF._declined, HF._declined
    module.zero_grad(set_to_none=True)
    with monkeypatch.context() as m:
        m.setattr(HF, "expand_usable", lambda *a, **k: False)
        plain = run()
    assert HF._declined                                     # the torch formulation did run, and said so
    HF._declined.clear()
    module.zero_grad(set_to_none=True)
    return fused, plain


def zero_gradient_biases(module):
    """Names of the conv biases that feed a training-mode BatchNorm: the norm subtracts the batch mean, so their exact gradient is
    sum g_y = 0 and what an f32 run returns is the rounding of that sum -- there is no value to be relatively close to.  g_y is the sum's
    term in the same layer's weight gradient too (times an O(1) input), so that gradient's scale is the yardstick: compare() holds such
    a bias gradient to the absolute part of the bound, 5e-6 of the weight gradient's maximum."""
    names = set()
    for prefix, seq in module.named_modules():
        if isinstance(seq, torch.nn.Sequential):
            for i in range(len(seq) - 1):
                if isinstance(seq[i], torch.nn.Conv1d) and isinstance(seq[i + 1], torch.nn.BatchNorm1d) and seq[i + 1].training:
                    names.add("%s%d.bias.grad" % (prefix + "." if prefix else "", i))
    for prefix, fold in module.named_modules():
        # Fold returns fd2 alone, and fd1 reaches it only as the U of folding2's first layer: a constant added to fd1 shifts every y of a
        # channel alike, which that layer's training-mode BatchNorm removes -- the last bias of folding1 has gradient 0 in the same way
        if type(fold).__name__ == "Fold" and fold.folding2[1].training:
            names.add("%sfolding1.6.bias.grad" % (prefix + "." if prefix else ""))
    return names


def compare(fused, plain, zero=()):
    assert [n for n, _ in fused] == [n for n, _ in plain]
    scale = {n: t.abs().max().item() for n, t in plain}
    for (name, a), (_, b) in zip(fused, plain):
        assert torch.isfinite(a).all(), name
        if name in zero:
            lim = 5e-6 * scale[name.replace(".bias.grad", ".weight.grad")]
            print("%s: |fused| %.3g, |torch| %.3g (exactly 0 in exact arithmetic; bound %.3g)" % (name, a.abs().max(), b.abs().max(), lim))
            assert a.abs().max().item() <= lim and b.abs().max().item() <= lim, name
            continue
        print("%s: max difference / scale = %.3g" % (name, scaled_error(a, b)))
        close(a, b)


@pytest.mark.parametrize("training", [True, False])
def test_fused_fold_against_the_torch_formulation(monkeypatch, training):
    from models.PoinTr import Fold
    fold = _seeded.fill(Fold(384, step=4, hidden_dim=256)).cuda().train(training)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(14, 384, generator=g).cuda().requires_grad_()
    g_out = torch.randn(14, 3, 16, generator=g).cuda()
    state = {k: v.clone() for k, v in fold.state_dict().items()}

    def run():
        fold.load_state_dict(state)                          # (the running buffers move in training mode)
        x.grad = None
        out = fold(x)
        out.backward(g_out)
        return [("out", out.detach()), ("x.grad", x.grad.clone())] + [(n + ".grad", p.grad.clone()) for n, p in fold.named_parameters()] + \
            [(n, b.clone().float()) for n, b in fold.named_buffers()]

    compare(*both_ways(monkeypatch, fold, run), zero=zero_gradient_biases(fold))


def test_fused_mlp_query_against_the_torch_formulation(monkeypatch):
    from models.Transformer import PCTransformer
    model = _seeded.fill(PCTransformer(embed_dim=384, depth=[1, 1], num_query=32, knn_layer=1)).cuda().train()
    g = torch.Generator().manual_seed(4)
    gf = torch.randn(2, 1024, generator=g).cuda().requires_grad_()
    coarse = (0.5 * torch.randn(2, 32, 3, generator=g)).cuda().requires_grad_()
    g_out = torch.randn(2, 32, 384, generator=g).cuda()

    def run():
        gf.grad = coarse.grad = None
        out = model.query_features(gf, coarse)
        out.backward(g_out)
        return [("out", out.detach()), ("global.grad", gf.grad.clone()), ("coarse.grad", coarse.grad.clone())] + \
            [(n + ".grad", p.grad.clone()) for n, p in model.mlp_query.named_parameters()]

    compare(*both_ways(monkeypatch, model, run))


def test_one_training_step(monkeypatch, fixture):
    """Forward + loss + backward of the model at the fixture size, in training mode: the launches (no library GEMM, no top-k, no softmax
    kernel) and finite gradients.  Then, in eval mode, every parameter gradient against the torch formulation's by
    close(rtol=2e-5, atol_scale=5e-6).  Training mode is held to float64 by test_training_gradients_against_float64_on_the_same_choices."""
    model = _seeded.fill(build()).cuda().train()
    x = _seeded.unit_ball_clouds(2, 640, seed=int(fixture["seed"])).cuda()
    gt = _seeded.unit_ball_clouds(2, 512, seed=11).cuda()
    state = {k: v.clone() for k, v in model.state_dict().items()}

    def run():
        model.load_state_dict(state)
        ret = model(x)
        loss_coarse, loss_fine = model.get_loss(ret, gt)
        (loss_coarse + loss_fine).backward()
        return [("loss", (loss_coarse + loss_fine).detach())] + [(n + ".grad", p.grad.clone()) for n, p in model.named_parameters()
                                                                 if p.grad is not None]

    run()                                                               # (warm-up: caches, lazy initialisation)
    model.zero_grad(set_to_none=True)
    HF._declined.clear()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    assert not HF._declined, HF._declined
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    print("\n".join(names))
    for n in names:
        assert "Cijk_" not in n and "topk" not in n.lower() and "softmax" not in n.lower(), n
    for frag in ("ex_stats_kernel", "ex_finalize_kernel", "ex_apply_kernel", "ex_bwd_reduce_kernel", "ex_bwd_param_kernel", "ex_bwd_apply_kernel",
                 "ex_bwd_wu_kernel", "ec_apply_kernel", "knn", "fps"):
        assert any(frag in n for n in names), frag
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    model.zero_grad(set_to_none=True)
    model.eval()
    fused, plain = both_ways(monkeypatch, model, run)
    # every parameter has a gradient but the local branches of the blocks past knn_layer, which the forward does not run (as the reference)
    unused = [n for n, _ in model.named_parameters() if n + ".grad" not in dict(fused)]
    assert unused and all(re.match(r"base_model\.(encoder|decoder)\.[1-9]\d*\.(knn_map|merge_map)", n) for n in unused), unused
    assert len(fused) + len(unused) == 1 + len(list(model.parameters()))
    compare(fused, plain, zero=zero_gradient_biases(model))


# ------------------------------------------------------------------ training mode against float64, discrete choices replayed
class Choices:
    """Record the discrete choices of one f32 forward (neighbour lists, FPS picks, the arg of every max, the branch of every ReLU /
    LeakyReLU), or replay them into a float64 evaluation of the same module made of torch operators only.  Patches the names the model
    code calls: HF.knn_query, HF.fps_gather, models.PoinTr.fps, ops.edge_conv_fwd (record) / torch_cpu.edge_conv_max (replay),
    upp_layers.max_over / gate / _relu_linear / _pointwise_bn_relu, and models.{Transformer,PoinTr}.expand."""

    def __init__(self, monkeypatch, items=None):
        self.m, self.items, self.replay, self.pos = monkeypatch, ([] if items is None else items), items is not None, 0

    def put(self, tag, *vals):
        self.items.append((tag, vals))

    def get(self, tag):
        got, vals = self.items[self.pos]
        assert got == tag, (self.pos, got, tag)
        self.pos += 1
        return vals if len(vals) > 1 else vals[0]

    @staticmethod
    def gated(z, mask, slope):
        return z * torch.where(mask, torch.ones((), dtype=z.dtype, device=z.device), torch.full((), slope, dtype=z.dtype, device=z.device))

    def install(self):
        import torch.nn.functional as F
        from models import PoinTr as MP, Transformer as MT, upp_layers as L
        from upp_hip import ops, torch_cpu
        m, rec = self.m, not self.replay
        real = dict(knn=HF.knn_query, fps=HF.fps_gather, fps_final=MP.fps, ec=ops.edge_conv_fwd, max=L.max_over, gate=L.gate,
                    relu_lin=L._relu_linear, bn_relu=L._pointwise_bn_relu, expand=MT.expand)

        def knn(ref, query, k):
            if rec:
                r = real["knn"](ref, query, k)
                self.put("knn", r[1].clone())
                return r
            return None, self.get("knn")

        def fps_gather(xyz, n):
            if rec:
                r = real["fps"](xyz, n)
                self.put("fps", r[1].clone())
                return r
            idx = self.get("fps")
            return torch.gather(xyz, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)), idx

        def fps_final(pc, num):
            if rec:
                r = real["fps_final"](pc, num)
                self.put("fps_final", r.clone())
                return r
            return self.get("fps_final").to(pc.dtype)

        def edge_conv_fwd(*a, **k):
            r = real["ec"](*a, **k)
            self.put("ec", r[1].clone(), r[0] > 0)
            return r

        def edge_conv_max(A, Bq, idx, norm=None, slope=0.2):
            arg, mask = self.get("ec")
            B, Nq, K = idx.shape
            O = A.shape[2]
            y = torch.gather(A, 1, idx.reshape(B, Nq * K, 1).expand(-1, -1, O)).view(B, Nq, K, O) + Bq.unsqueeze(2)
            if norm is not None:
                G, gamma, beta, eps = norm
                y = F.group_norm(y.permute(0, 3, 1, 2), int(G), gamma, beta, float(eps)).permute(0, 2, 3, 1)
            return self.gated(torch.gather(y, 2, arg.long().unsqueeze(2)).squeeze(2), mask, slope)

        def max_over(x, dim, site=""):
            if rec:
                self.put("max", x.detach().max(dim=dim)[1])
                return real["max"](x, dim, site)
            return x.gather(dim, self.get("max").unsqueeze(dim)).squeeze(dim)

        def gate(site, z, slope=0.0):
            if rec:
                self.put("gate", z.detach() > 0)
                return real["gate"](site, z, slope)
            return self.gated(z, self.get("gate"), slope)

        def relu_linear(x, lin):
            if rec:
                out = real["relu_lin"](x, lin)
                self.put("relu_lin", out.detach() > 0)
                return out
            return self.gated(F.linear(x, lin.weight, lin.bias), self.get("relu_lin"), 0.0)

        def pointwise_bn_relu(x, conv, bn, training):
            if rec:
                out = real["bn_relu"](x, conv, bn, training)
                self.put("bn_relu", out.detach() > 0)
                return out
            y = F.linear(x, conv.weight.view(conv.weight.shape[0], -1), conv.bias)
            y = F.batch_norm(y, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)
            return self.gated(y, self.get("bn_relu"), 0.0)

        def expand(P, U, Wu, norm, slope, site):
            if rec:
                out = real["expand"](P, U, Wu, norm, slope, site)
                self.put("expand", out.detach() > 0)
                return out
            y = P.unsqueeze(1) + torch.matmul(U, Wu.t())
            if norm is not None:
                y = F.batch_norm(y.reshape(-1, y.shape[-1]), None, None, norm.weight, norm.bias, True, 0.0, norm.eps).view_as(y)
            return self.gated(y, self.get("expand"), slope)

        m.setattr(HF, "knn_query", knn)
        m.setattr(HF, "fps_gather", fps_gather)
        m.setattr(MP, "fps", fps_final)
        if rec:
            m.setattr(ops, "edge_conv_fwd", edge_conv_fwd)
        else:
            m.setattr(torch_cpu, "edge_conv_max", edge_conv_max)
        m.setattr(L, "max_over", max_over)
        m.setattr(L, "gate", gate)
        m.setattr(L, "_relu_linear", relu_linear)
        m.setattr(L, "_pointwise_bn_relu", pointwise_bn_relu)
        m.setattr(MT, "expand", expand)
        m.setattr(MP, "expand", expand)


def test_training_gradients_against_float64_on_the_same_choices(monkeypatch, fixture):
    """Training mode (batch statistics in every BatchNorm, the expand sites' included), the whole model at the fixture size, fixed
    cotangents on both outputs.  The fused f32 run and the torch-formulation f32 run (HF.expand_usable off) each record their discrete
    choices; the module in float64 -- torch operators only -- is evaluated on the recorded choices of each.  Every output and parameter
    gradient of the fused run must then be within max(5e-6, 3 x err_torch) of its float64 evaluation, relative to that tensor's maximum:
    5e-6 is the absolute part of close(), err_torch the torch formulation's own f32-against-f64 error of the same tensor, computed here,
    and 3 the fixture bound's factor -- two f32 evaluations that sum in different orders land anywhere inside one rounding envelope.
    A bias whose gradient float64 evaluates to 0 (those of zero_gradient_biases, and those that add one vector to every query feature,
    which the folding head's first BatchNorm removes) has no scale of its own: its errors are taken relative to its layer's weight
    gradient, under the same rule."""
    import copy
    model = _seeded.fill(build()).cuda().train()
    x = _seeded.unit_ball_clouds(2, 640, seed=int(fixture["seed"])).cuda()
    g = torch.Generator().manual_seed(12)
    g_coarse, g_rebuild = torch.randn(2, 64, 3, generator=g).cuda(), torch.randn(2, 1152, 3, generator=g).cuda()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model64 = copy.deepcopy(model).double()

    def run(net, dtype):
        net.zero_grad(set_to_none=True)
        coarse, rebuild = net(x.to(dtype))
        torch.autograd.backward([coarse, rebuild], [g_coarse.to(dtype), g_rebuild.to(dtype)])
        return [("coarse", coarse.detach()), ("rebuild", rebuild.detach())] + [(n + ".grad", p.grad.clone()) for n, p in net.named_parameters()
                                                                               if p.grad is not None]

    def with_float64(fused):
        model.load_state_dict(state)
        HF._declined.clear()
        with monkeypatch.context() as m:
            if not fused:
                m.setattr(HF, "expand_usable", lambda *a, **k: False)
            rec = Choices(m)
            rec.install()
            f32 = run(model, torch.float32)
        assert bool(HF._declined) != fused, HF._declined
        with monkeypatch.context() as m:
            rep = Choices(m, rec.items)
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
    scale = {n: t.abs().max().item() for n, t in fused64}
    scale_t = {n: t.abs().max().item() for n, t in plain64}
    worst = ("", 0.0, 0.0)
    failures, zeros = [], []
    for (name, a), (_, a64), (_, b), (_, b64) in zip(fused, fused64, plain, plain64):
        assert torch.isfinite(a).all(), name
        unit, unit_t = scale[name], scale_t[name]
        wname = name.replace(".bias.grad", ".weight.grad")
        if name.endswith(".bias.grad") and wname in scale and unit <= 1e-9 * scale[wname] and unit_t <= 1e-9 * scale_t[wname]:
            # float64 evaluates this gradient to 0 (a constant per channel in front of a training-mode BatchNorm: the biases of
            # zero_gradient_biases and those that shift the query features by one vector): its own maximum is no scale, so the errors
            # are taken relative to the same layer's weight gradient -- the same sum with each term weighted by the layer's input
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
    assert zero_gradient_biases(model) <= set(zeros), sorted(zero_gradient_biases(model) - set(zeros))
    print("largest: %s fused %.3g (torch formulation %.3g)" % worst)
    assert not failures, failures
