"""Part-segmentation evaluation on the device (csrc/seg_eval.hip, utils/evaluate.py SegMetric / validate_seg /
validate_seg_captured, upp_hip/infer.py SegEvalStep): the metric kernels against the numpy restatement of the reference's `validate`
(tests/_seg_reference.py), the eager and captured protocols on a seeded Point_MAE_unify_seg, graph against eager driver, staleness
after training and after load_state_dict, graph safety."""
import os
import sys

import numpy as np
import pytest
import torch

import _seeded
from _seg_reference import SEG_CLASSES, assert_metrics_match, planted_batch, reference_metrics
from conftest import ROOT
from models import build_model_from_cfg
from utils import evaluate
from utils.config import builtin_cfg
from upp_hip import functional as HF
from upp_hip import infer, ops
from upp_hip.train import TrainStep, freeze_for_peft

pytestmark = pytest.mark.gpu

SEG_PEFT = ['downstream_adapter', 'downstream_prompts', 'label_conv', 'propagation_0', 'seg_head', 'propagation_1']   # reference tools/runner_unify_seg.py:143-146
N_PTS = 2048


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _device_metric(batches, strided=False, n_valid=None):
    """SegMetric on the device over numpy batches; strided: logp as a [..., :50] view of a (B, N, 56) buffer."""
    m = evaluate.SegMetric()
    preds, ious = [], []
    for i, (logp, target) in enumerate(batches):
        x = torch.from_numpy(logp).cuda()
        if strided:
            wide = torch.full(x.shape[:2] + (56,), 7.0, device='cuda')             # the padding columns would win every arg-max
            wide[..., :50] = x
            x = wide[..., :50]
        pred = torch.full(logp.shape[:2], -7, dtype=torch.long, device='cuda')
        nv = None if n_valid is None else n_valid[i]
        ious.append(m.update(x, torch.from_numpy(target).cuda(), n_valid=nv, pred=pred).cpu().clone())
        preds.append(pred.cpu())
    return m, preds, torch.cat(ious)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("N", [1, 100, 2048, 2500])
@pytest.mark.parametrize("B", [1, 3, 32])
def test_the_metric_kernels_match_the_reference_arithmetic(B, N):
    batches = [planted_batch(B, N, seed=B * 1000 + N), planted_batch(B, N, seed=B * 1000 + N + 1, ties=False)]
    want = reference_metrics(batches)
    for strided in (False, True):
        m, preds, ious = _device_metric(batches, strided=strided)
        for p, w in zip(preds, want['pred']):
            assert np.array_equal(p.numpy(), w)
        assert np.array_equal(_bits(ious.numpy()), _bits(want['shape_iou'])), "per-shape IoU is bit-identical in float64"
        s = m.sums
        assert s.counters.cpu().tolist() == [want['correct'], want['seen'], 0]
        assert np.array_equal(s.part_seen.cpu().numpy(), want['part_seen'])
        assert np.array_equal(s.part_correct.cpu().numpy(), want['part_correct'])
        assert_metrics_match(m.compute(), want)
    host = evaluate.SegMetric()
    for logp, target in batches:
        host.update(torch.from_numpy(logp), torch.from_numpy(target))
    assert np.array_equal(_bits(host.sums.cat_sum.numpy()), _bits(m.sums.cat_sum.cpu().numpy())), "the CPU path is the same arithmetic"
    assert torch.equal(host.sums.cat_cnt, m.sums.cat_cnt.cpu())


def test_a_ragged_batch_and_an_invalid_shape_on_the_device():
    a, b = planted_batch(5, 300, seed=1), planted_batch(5, 300, seed=2)
    b[1][4, 0] = 77                                                          # a padding row: never a shape
    m, preds, ious = _device_metric([a, b], n_valid=[5, 3])
    want = reference_metrics([a, (b[0][:3], b[1][:3])])
    assert np.array_equal(_bits(ious.numpy()), _bits(want['shape_iou']))
    assert m.sums.counters.cpu().tolist() == [want['correct'], want['seen'], 0]
    assert_metrics_match(m.compute(), want)
    logp, target = planted_batch(3, 64, seed=3)
    target[2, 0] = -1
    m, preds, _ = _device_metric([(logp, target)])
    assert m.sums.counters.cpu().tolist()[2] == 1 and (preds[0][2] == -1).all()
    with pytest.raises(ValueError, match="1 shape"):
        m.compute()


def test_two_evaluations_in_a_row_are_identical():
    batches = [planted_batch(32, N_PTS, seed=60 + i) for i in range(2)]
    runs = []
    for _ in range(2):
        m, preds, ious = _device_metric(batches)
        s = m.sums
        runs.append((s.counters.cpu(), s.part_seen.cpu(), s.part_correct.cpu(), s.cat_sum.cpu(), s.cat_cnt.cpu(), ious))
        assert not s.scratch.any(), "the accumulate launch leaves the scratch zeroed"
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_bad_arguments_are_refused_before_any_launch():
    _, pc, cr = evaluate.seg_tables()
    pc, cr = pc.cuda(), cr.cuda()
    acc = ops.SegAccumulator(50, 16, 'cuda')
    logp = torch.zeros(2, 8, 50, device='cuda')
    tgt = torch.zeros(2, 8, dtype=torch.long, device='cuda')
    with pytest.raises(RuntimeError, match="row stride"):
        ops.seg_iou_update(torch.zeros(2, 50, 8, device='cuda').transpose(1, 2), tgt, pc, cr, acc)
    with pytest.raises(RuntimeError, match="target"):
        ops.seg_iou_update(logp, tgt.int(), pc, cr, acc)
    with pytest.raises(RuntimeError, match="table"):
        ops.seg_iou_update(torch.zeros(2, 8, 40, device='cuda'), tgt, pc[:40], cr, acc)
    with pytest.raises(RuntimeError, match="n_valid"):
        ops.seg_iou_update(logp, tgt, pc, cr, acc, n_valid=3)
    assert acc.counters.tolist() == [0, 0, 0] and acc.scratch is None


# ------------------------------------------------------------------ the protocols on the model
def _model(peft=True):
    m = _seeded.fill(build_model_from_cfg(builtin_cfg('unify_shapenetpart_seg').model)).cuda()
    if peft:
        freeze_for_peft(m, SEG_PEFT)
    return m.train()


def _batches(sizes, seed=0):
    cats = list(SEG_CLASSES.values())
    names = sorted(SEG_CLASSES)
    out = []
    for i, b in enumerate(sizes):
        rng = np.random.default_rng(seed + i)
        pts = _seeded.unit_ball_clouds(b, N_PTS, seed=seed + i).cuda()
        label, target = np.zeros((b, 1), dtype=np.int64), np.zeros((b, N_PTS), dtype=np.int64)
        for j in range(b):
            parts = cats[(seed + i * 5 + j) % len(cats)]
            label[j, 0] = names.index(next(k for k, v in SEG_CLASSES.items() if v == parts))
            target[j] = rng.choice(parts, N_PTS)
        out.append((pts, torch.from_numpy(label).cuda(), torch.from_numpy(target).cuda()))
    return out


def _with_logp(model, fn):
    got = []
    h = model.register_forward_hook(lambda mod, inp, out: got.append(out.detach().clone()))
    try:
        return fn(), got
    finally:
        h.remove()


def test_validate_seg_is_the_reference_protocol():
    model = _model()
    batches = _batches([4, 4, 3], seed=10)
    (out, pred), logps = _with_logp(model, lambda: evaluate.validate_seg(model, batches, return_predictions=True))
    assert model.training
    assert [tuple(x.shape) for x in logps] == [(4, N_PTS, 50), (4, N_PTS, 50), (3, N_PTS, 50)]
    want = reference_metrics([(lp.cpu().numpy(), t.cpu().numpy()) for lp, (_, _, t) in zip(logps, batches)])
    assert_metrics_match(out, want)
    assert np.array_equal(pred.cpu().numpy(), np.concatenate(want['pred']))
    assert 0.0 < out['inctance_avg_iou'] < 1.0


def _in_category_margin(logp, target):
    names, part_cat, cat_range = evaluate.seg_tables()
    out = []
    for i in range(logp.shape[0]):
        c = int(part_cat[int(target[i, 0])])
        lo, n = int(cat_range[c, 0]), int(cat_range[c, 1])
        top = logp[i, :, lo:lo + n].double().topk(min(2, n), -1).values
        out.append(top[:, 0] - top[:, 1] if n > 1 else torch.full_like(top[:, 0], float('inf')))
    return torch.stack(out)


def test_validate_seg_captured_matches_validate_seg():
    model = _model()
    batches = _batches([4, 4, 3], seed=20)
    rng = torch.cuda.get_rng_state(), torch.get_rng_state()
    (out_e, pred_e), eager = _with_logp(model, lambda: evaluate.validate_seg(model, batches, return_predictions=True))
    out_c, pred_c = evaluate.validate_seg_captured(model, batches, return_predictions=True)
    assert model.training, "the training flag is restored"
    assert torch.equal(torch.cuda.get_rng_state(), rng[0]) and torch.equal(torch.get_rng_state(), rng[1]), "nothing is drawn"
    step = [s for s in infer._STEPS[model].values() if isinstance(s, infer.SegEvalStep)][-1]
    assert step.B == 4
    # the last batch's log-probabilities are still in the step's static output: padded 3 -> 4
    ref = eager[-1]
    assert (step.logp[:3] - ref).abs().max() <= 2e-5 * ref.abs().max()
    margins = torch.cat([_in_category_margin(lp, t) for lp, (_, _, t) in zip(eager, batches)])
    clear = margins > 1e-4
    assert torch.equal(pred_c[clear], pred_e[clear])
    assert torch.equal(pred_c, pred_e), "seeded case: every prediction agrees"
    for key in ('accuracy', 'class_avg_accuracy', 'class_avg_iou', 'inctance_avg_iou'):
        assert out_c[key] == out_e[key] or (out_c[key] != out_c[key] and out_e[key] != out_e[key]), key
    assert out_c['category_iou'] == out_e['category_iou'] or all(
        a == b or (a != a and b != b) for a, b in zip(out_c['category_iou'].values(), out_e['category_iou'].values()))


def test_a_full_size_batch():
    model = _model()
    batches = _batches([32], seed=30)
    (out_e, pred_e), eager = _with_logp(model, lambda: evaluate.validate_seg(model, batches, return_predictions=True))
    out_c, pred_c = evaluate.validate_seg_captured(model, batches, return_predictions=True)
    want = reference_metrics([(eager[0].cpu().numpy(), batches[0][2].cpu().numpy())])
    assert_metrics_match(out_e, want)
    clear = _in_category_margin(eager[0], batches[0][2]) > 1e-4
    assert torch.equal(pred_c[clear], pred_e[clear])
    assert_metrics_match(out_c, out_e, rel=1e-3)


# ------------------------------------------------------------------ driver
def _run_step(step, batches):
    step.prepare()
    m = evaluate.SegMetric()
    out = []
    for pts, lab, tgt in batches:
        p = step.run(pts, lab, tgt, m)
        out.append((step.logp.clone(), p.clone()))
    return out, m


def test_replay_equals_the_eager_driver():
    model = _model()
    batches = _batches([4, 4, 2], seed=40)
    model.eval()
    g, mg = _run_step(infer.SegEvalStep(model, (4, N_PTS, 3), use_graph=True), batches)
    e, me = _run_step(infer.SegEvalStep(model, (4, N_PTS, 3), use_graph=False), batches)
    model.train()
    for (lg, pg), (le, pe) in zip(g, e):
        assert torch.equal(lg, le) and torch.equal(pg, pe)
    for name in ('counters', 'part_seen', 'part_correct', 'cat_sum', 'cat_cnt'):
        assert torch.equal(getattr(mg.sums, name), getattr(me.sums, name)), name
    assert int(mg.sums.counters[1]) == 10 * N_PTS


def test_a_model_that_reads_across_samples_is_refused():
    cfg = builtin_cfg('unify_shapenetpart_seg').model
    cfg.prompt_propagation_after, cfg.gather_idx = True, False
    m = build_model_from_cfg(cfg).cuda()
    with pytest.raises(ValueError, match="per sample"):
        infer.SegEvalStep(m, (4, N_PTS, 3))


def _seg_train_step(model, B=4):
    g = torch.Generator(device='cuda').manual_seed(0)
    pts = _seeded.unit_ball_clouds(B, N_PTS, seed=41).cuda()
    onehot = torch.zeros(B, 16, device='cuda')
    onehot[torch.arange(B), torch.arange(B) % 16] = 1
    target = torch.randint(0, 50, (B * N_PTS,), device='cuda', generator=g)

    def loss_fn(m, pts, onehot, target):
        logp = m(pts, onehot, completion_prompt=False, denoise=False, point_num=N_PTS)
        loss = m.get_loss(logp.reshape(-1, 50), target)
        return loss, loss.detach()
    return TrainStep(model, (B, N_PTS, 3), loss_fn=loss_fn, inputs=[pts, onehot, target])


def test_captured_evaluation_follows_training_and_loaded_weights():
    model = _model()
    batches = _batches([4, 3], seed=50)
    step = infer.SegEvalStep(model, (4, N_PTS, 3))
    before, _ = _run_step(step, batches)
    # (a) a TrainStep re-points the trainable parameters into its flat buffer and trains
    ts = _seg_train_step(model)
    for _ in range(3):
        ts.step()
    torch.cuda.synchronize()
    after, m_after = _run_step(step, batches)
    fresh, m_fresh = _run_step(infer.SegEvalStep(model, (4, N_PTS, 3), use_graph=False), batches)
    for (la, pa), (lf, pf), (lb, _) in zip(after, fresh, before):
        assert torch.equal(la, lf) and torch.equal(pa, pf)
        assert not torch.equal(la, lb)
    assert torch.equal(m_after.sums.cat_sum, m_fresh.sums.cat_sum)
    # (b) new frozen weights through load_state_dict (contents change, addresses stay)
    sd = model.state_dict()
    g = torch.Generator().manual_seed(5)
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    new = {k: (v + 0.05 * torch.randn(v.shape, generator=g).to(v.device) * v.abs().mean() if k in frozen else v) for k, v in sd.items()}
    model.load_state_dict(new)
    loaded, _ = _run_step(step, batches)
    fresh, _ = _run_step(infer.SegEvalStep(model, (4, N_PTS, 3), use_graph=False), batches)
    for (la, pa), (lf, pf), (lb, _) in zip(loaded, fresh, after):
        assert torch.equal(la, lf) and torch.equal(pa, pf)
        assert not torch.equal(la, lb)


def test_a_seg_evaluation_is_graph_safe():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from memset_census import memsets_of
    model = _model()
    batches = _batches([4], seed=60)
    step = infer.SegEvalStep(model, (4, N_PTS, 3), use_graph=False)
    _run_step(step, batches)                                    # warm-up: lazy caches
    HF._declined.clear()
    model.eval()
    try:
        assert memsets_of(step._evaluate) == []
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            step._evaluate()
            m = evaluate.SegMetric()
            m.update(step.logp, batches[0][2])
            torch.cuda.synchronize()
        assert memsets_of(lambda: m.update(step.logp, batches[0][2])) == []
    finally:
        model.train()
    names = [e.key for e in prof.key_averages()]
    assert not [k for k in names if k.startswith('Cijk') or 'rocprim' in k.lower() or 'radixsort' in k.lower()], names
    assert HF._declined == set()
