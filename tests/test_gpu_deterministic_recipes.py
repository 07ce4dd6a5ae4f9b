"""Reproducible training (README "Reproducible training"): with TrainStep(..., deterministic=True) two independent constructions of a
recipe from the same seed walk the same trajectory BIT FOR BIT -- six losses and the final flat parameter buffer -- eager against eager
and captured against captured.  The four recipes whose steps differentiate through the library's scatter-adds (Chamfer gradients, the
grouping / gather / FPS-gather backward, the EMD cost): pretask, stage2, cls_aux, pretrain; six steps is three past the point where two
eager runs of stage 2 and of the pre-task recipe used to part company (NOTEBOOK 12.11).  The captured run is NOT compared with the
eager one here (tests/test_gpu_graph_safety.py does that, to a tolerance)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

pytestmark = pytest.mark.gpu
STEPS, BATCH = 6, 4


def _run(kind, use_graph, monkeypatch):
    import bench
    from models import upp_layers
    import upp_hip.train as T
    import upp_hip.functional as HF
    real = T.TrainStep
    modes = []

    class Step(real):                                  # the recipe as bench.RecipeTrainer builds it, its driver in the reproducible mode
        def __init__(self, *a, **kw):
            super().__init__(*a, deterministic=True, **kw)

        def _forward_backward_pass(self, *a):
            modes.append(HF.DETERMINISTIC)
            return super()._forward_backward_pass(*a)
    monkeypatch.setattr(T, "TrainStep", Step)
    torch.manual_seed(1234)
    bank = upp_layers.UNIFORMS                          # every run starts from an empty uniform bank (tests/test_gpu_determinism.py)
    bank.buf, bank.pos, bank.asked, bank.need = None, 0, 0, 0
    tr = bench.RecipeTrainer(kind, torch.device("cuda", 0), BATCH, use_graph=use_graph, pipeline=False)
    monkeypatch.setattr(T, "TrainStep", real)
    assert isinstance(tr.ts, Step) and tr.ts.deterministic is True
    torch.manual_seed(4321)                             # (the construction's draws are done: the steps' draws start from here)
    losses = []
    for _ in range(STEPS):
        loss = tr.step()
        torch.cuda.synchronize()
        losses.append(loss.detach().clone())
    assert modes and all(modes) and HF.DETERMINISTIC is False          # every pass of the driver ran in the mode, and it is restored
    return torch.stack(losses), tr.ts.flat.flat.detach().clone(), tr.ts.opt.p.detach().clone()      # (losses, flat gradients, flat parameters)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("kind", ["pretask", "stage2", "cls_aux", "pretrain"])
def test_two_runs_of_a_recipe_are_bit_identical(kind, use_graph, monkeypatch):
    la, ga, pa = _run(kind, use_graph, monkeypatch)
    lb, gb, pb = _run(kind, use_graph, monkeypatch)
    assert torch.isfinite(la).all() and float(pa.abs().max()) > 0.0
    first = [k for k in range(STEPS) if la[k].view(torch.int32) != lb[k].view(torch.int32)]
    assert not first, "%s: the losses part at step %d: %s vs %s" % (kind, first[0], la.tolist(), lb.tolist())
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)), "%s: %d gradient entries differ after %d steps" % (
        kind, int((ga != gb).sum()), STEPS)
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), "%s: %d of %d parameters differ after %d steps" % (
        kind, int((pa != pb).sum()), pa.numel(), STEPS)
