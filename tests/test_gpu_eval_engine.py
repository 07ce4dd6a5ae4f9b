"""Captured, vote-batched evaluation (upp_hip/infer.py, csrc/eval.hip): the two kernels against torch, the captured protocols against
the eager `validate` / `test_vote`, graph against eager driver, staleness after training and after load_state_dict, graph safety."""
import os
import sys

import pytest
import torch

import _seeded
from conftest import ROOT
from models import build_model_from_cfg
from utils import evaluate
from utils.config import builtin_cfg
from upp_hip import functional as HF
from upp_hip import infer, ops
from upp_hip.train import TrainStep, freeze_for_peft

pytestmark = pytest.mark.gpu

N_RAW = 1400          # superset: min(1200, N_RAW) = 1200 points


def _model(peft=True):
    m = _seeded.fill(build_model_from_cfg(builtin_cfg('unify_modelnet_cls').model)).cuda()
    if peft:
        freeze_for_peft(m)
    return m.train()


def _batches(sizes, n_raw=N_RAW, seed=0):
    out = []
    for i, b in enumerate(sizes):
        pts = _seeded.noisy_clouds(b, n_raw - 72, seed=seed + i).cuda()            # (+ 48 lidar and 24 shell outliers)
        lab = torch.randint(0, 40, (b,), generator=torch.Generator().manual_seed(100 + i)).cuda()
        out.append((pts, lab))
    return out


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("V", [1, 3, 10])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("S", [1100, 1200])
def test_vote_points_is_scale_translate_of_the_gather(V, B, S):
    g = torch.Generator(device='cuda').manual_seed(V * 100 + B * 10 + S)
    sup = torch.randn(B, S, 3, device='cuda', generator=g)
    pick = torch.stack([torch.randperm(S, device='cuda', generator=g)[:1024] for _ in range(V)]).to(torch.int32)
    s = torch.empty(V, B, 3, device='cuda').uniform_(2. / 3., 3. / 2., generator=g)
    t = torch.empty(V, B, 3, device='cuda').uniform_(-0.2, 0.2, generator=g)
    got = ops.vote_points(sup, pick, s, t).view(V, B, 1024, 3)
    plain = ops.vote_points(sup, pick).view(V, B, 1024, 3)
    for v in range(V):
        pc = sup[:, pick[v].long()]
        assert torch.equal(plain[v], pc)
        assert torch.equal(got[v], pc * s[v].unsqueeze(1) + t[v].unsqueeze(1))       # misc.scale_translate's expression


def _reduce_reference(logits, V, B):
    m = logits.double().cpu().view(V, B, -1).mean(0)
    return m, m.argmax(-1)


@pytest.mark.parametrize("V", [1, 3, 10])
def test_vote_reduce_matches_a_float64_mean_and_argmax(V):
    B, C = 8, 40
    g = torch.Generator(device='cuda').manual_seed(V)
    logits = torch.randn(V * B, C, device='cuda', generator=g) * 3
    L = logits.view(V, B, C)
    L[:, 1, 7] = L[:, 1, 30] = L[:, 1].max() + 1.0                  # planted exact tie: the first index wins
    L[:, 2, :] = 0.25                                               # all equal: class 0
    L[V - 1, 3, 12] = float('nan')                                  # a NaN vote: its class is the arg-max
    L[0, 4, 5] = L[0, 4, 9] = float('nan')                          # two NaN classes: the first
    labels = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(V)).cuda()
    m, want = _reduce_reference(logits, V, B)
    want[3], want[4] = 12, 5
    labels[1:3] = want[1:3].cuda()                                  # two certain hits
    pred = torch.full((B,), -1, dtype=torch.long, device='cuda')
    counters = torch.zeros(2, dtype=torch.long, device='cuda')
    top2 = m.nan_to_num(1e30).topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-5
    clear[1] = clear[2] = clear[3] = clear[4] = True
    n_valid, expect = [B, 5, 3], [0, 0]
    for nv in n_valid:                                              # counters accumulate over calls; rows >= n_valid are not counted
        ops.vote_reduce(logits, labels, V, nv, pred, counters)
        p = pred.cpu()
        assert torch.equal(p[clear], want[clear]), (p, want)
        expect[0] += int((p[:nv] == labels[:nv].cpu()).sum())
        expect[1] += nv
    assert counters.cpu().tolist() == expect
    assert expect[0] >= 2 * len(n_valid)


def test_vote_reduce_rejects_bad_arguments_before_any_launch():
    lib = ops._abi.load()
    x = torch.zeros(4, 10, device='cuda')
    lab = torch.zeros(4, dtype=torch.long, device='cuda')
    pred = torch.zeros(4, dtype=torch.long, device='cuda')
    c = torch.zeros(2, dtype=torch.long, device='cuda')
    with pytest.raises(RuntimeError, match="range"):
        ops.vote_reduce(x, lab, 1, 5, pred, c)
    assert lib.upp_vote_reduce(None, None, 1, 4, 10, 4, None, None, None) == -1
    assert c.tolist() == [0, 0]


# ------------------------------------------------------------------ the protocols
def _eager_logits(model, fn):
    got = []
    h = model.register_forward_hook(lambda mod, inp, out: got.append(out.detach().clone()))
    seen = []
    real = evaluate._accuracy

    def spy(pred, label, distributed):
        seen.append(torch.cat(pred))
        return real(pred, label, distributed)
    evaluate._accuracy = spy
    try:
        acc = fn()
    finally:
        evaluate._accuracy = real
        h.remove()
    return acc, got, seen[0]


def _captured_logits(model, batches, fn):
    """fn(generator of batches) -> result; the vote-major logits of every batch (the step's static buffer, read after each one)."""
    got = []

    def gen():
        for b in batches:
            yield b
            steps = list(infer._STEPS[model].values())
            got.append(steps[-1].logits.clone())
    return fn(gen()), got


def test_test_vote_captured_matches_test_vote():
    model = _model()
    assert infer.mixes_samples(model)          # (the recipe's propagation indexing: one vote per forward keeps test_vote's logits)
    batches = _batches([4, 4, 3])
    V = 10
    torch.manual_seed(7)
    gen = torch.Generator(device='cuda').manual_seed(11)
    acc_e, eager, pred_e = _eager_logits(model, lambda: evaluate.test_vote(model, batches, 1024, times=V, generator=gen))
    rng_e = torch.cuda.get_rng_state()
    model.train()
    torch.manual_seed(7)
    gen = torch.Generator(device='cuda').manual_seed(11)
    (acc_c, pred_c), cap = _captured_logits(model, batches, lambda it: evaluate.test_vote_captured(
        model, it, 1024, times=V, generator=gen, return_predictions=True))
    assert torch.equal(torch.cuda.get_rng_state(), rng_e), "test_vote_captured must advance the RNG exactly as test_vote"
    assert model.training
    k = 0
    margins = []
    for (pts, _), lg in zip(batches, cap):
        n = pts.shape[0]
        votes = eager[k:k + V]
        k += V
        ref = torch.stack(votes)                                    # (V, n, C)
        scale = ref.abs().max()
        assert (lg.view(V, -1, lg.shape[-1])[:, :n] - ref).abs().max() <= 2e-5 * scale
        m = ref.double().mean(0)
        top2 = m.topk(2, -1).values
        margins.append(top2[:, 0] - top2[:, 1])
    margins = torch.cat(margins)
    clear = margins > 1e-4
    assert torch.equal(pred_c[clear], pred_e[clear])
    assert torch.equal(pred_c, pred_e), "seeded case: every prediction agrees"
    assert torch.equal(acc_c, acc_e) and acc_c.dtype == acc_e.dtype


@pytest.mark.parametrize("noisy", [False, True])
def test_validate_captured_matches_validate(noisy):
    model = _model()
    batches = _batches([4, 4, 3], n_raw=2048, seed=20)
    rng = torch.cuda.get_rng_state()
    acc_e, eager, pred_e = _eager_logits(model, lambda: evaluate.validate(model, batches, 1024, noisy=noisy))
    model.train()
    (acc_c, pred_c), cap = _captured_logits(model, batches, lambda it: evaluate.validate_captured(
        model, it, 1024, noisy=noisy, return_predictions=True))
    assert model.training, "the training flag is restored"
    assert torch.equal(torch.cuda.get_rng_state(), rng), "validate_captured draws nothing"
    for (pts, _), lg, ref in zip(batches, cap, eager):
        n = pts.shape[0]
        assert (lg[:n] - ref).abs().max() <= 2e-5 * ref.abs().max()
    assert torch.equal(pred_c, pred_e)
    assert torch.equal(acc_c, acc_e)


# ------------------------------------------------------------------ driver
def _run_step(step, batches, seed=3):
    torch.manual_seed(seed)
    gen = torch.Generator(device='cuda').manual_seed(seed)
    step.prepare()
    step.counters.zero_()
    out = []
    for pts, lab in batches:
        p = step.run(pts, lab, generator=gen)
        out.append((step.logits.clone(), p.clone()))
    return out, step.counters.clone()


@pytest.mark.parametrize("votes", [1, 10])
def test_replay_equals_the_eager_driver(votes):
    model = _model()
    batches = _batches([4, 4, 2], seed=30)
    # votes = 1: the validate form; 10: the test_vote form in forwards of 4 + 4 + 2 votes (max_clouds = 16 at B = 4)
    kw = dict(votes=1) if votes == 1 else dict(votes=votes, superset=1200, max_clouds=16)
    g, cg = _run_step(infer.EvalStep(model, (4, N_RAW, 3), 1024, use_graph=True, **kw), batches)
    e, ce = _run_step(infer.EvalStep(model, (4, N_RAW, 3), 1024, use_graph=False, **kw), batches)
    for (lg, pg), (le, pe) in zip(g, e):
        assert torch.equal(lg, le) and torch.equal(pg, pe)
    assert torch.equal(cg, ce) and int(cg[1]) == 10


def test_captured_evaluation_follows_training_and_loaded_weights():
    model = _model()
    batches = _batches([4, 3], seed=40)
    step = infer.EvalStep(model, (4, N_RAW, 3), 1024, votes=3, superset=1200)
    before, _ = _run_step(step, batches)
    # (a) a TrainStep re-points the trainable parameters into its flat buffer and trains
    ts = TrainStep(model, (4, 1096, 3))
    x = _seeded.noisy_clouds(4, 1024, seed=41).cuda()
    y = torch.tensor([1, 2, 3, 4], device='cuda')
    for _ in range(3):
        ts.step(x, y)
    torch.cuda.synchronize()
    after, _ = _run_step(step, batches)
    fresh, _ = _run_step(infer.EvalStep(model, (4, N_RAW, 3), 1024, votes=3, superset=1200, use_graph=False), batches)
    for (la, pa), (lf, pf), (lb, _) in zip(after, fresh, before):
        assert torch.equal(la, lf) and torch.equal(pa, pf)
        assert not torch.equal(la, lb)
    # (b) new frozen weights through load_state_dict (contents change, addresses stay)
    sd = model.state_dict()
    g = torch.Generator().manual_seed(5)
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    new = {k: (v + 0.05 * torch.randn(v.shape, generator=g).to(v.device) * v.abs().mean() if k in frozen else v) for k, v in sd.items()}
    model.load_state_dict(new)
    loaded, _ = _run_step(step, batches)
    fresh, _ = _run_step(infer.EvalStep(model, (4, N_RAW, 3), 1024, votes=3, superset=1200, use_graph=False), batches)
    for (la, pa), (lf, pf), (lb, _) in zip(loaded, fresh, after):
        assert torch.equal(la, lf) and torch.equal(pa, pf)
        assert not torch.equal(la, lb)


def test_an_evaluation_is_graph_safe():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from memset_census import memsets_of
    model = _model()
    batches = _batches([4], seed=50)
    for votes, noisy in ((10, False), (1, True)):
        kw = dict(votes=votes, noisy=noisy) if votes == 1 else dict(votes=votes, superset=1200)
        step = infer.EvalStep(model, (4, N_RAW, 3), 1024, use_graph=False, **kw)
        _run_step(step, batches)                                # warm-up: lazy caches
        HF._declined.clear()
        model.eval()
        try:
            assert memsets_of(step._evaluate) == []
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
                step._evaluate()
                torch.cuda.synchronize()
        finally:
            model.train()
        names = [e.key for e in prof.key_averages()]
        assert not [k for k in names if k.startswith('Cijk') or 'rocprim' in k.lower() or 'radixsort' in k.lower()], names
        assert HF._declined == set()
    assert model.training
