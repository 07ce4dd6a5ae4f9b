"""Point-completion evaluation on the device (csrc/completion_eval.hip, utils/evaluate.py CompletionMetric / validate_completion /
validate_completion_captured, upp_hip/infer.py CompletionEvalStep): the metric kernels against the numpy restatement of the reference
(tests/_completion_reference.py), the ignore_zeros pass, determinism, the eager and captured protocols on a seeded
Point_MAE_pretask_dev, staleness after an optimizer step and after load_state_dict, graph safety, one full-size batch."""
import os
import sys

import numpy as np
import pytest
import torch

import _seeded
from _completion_reference import assert_completion_match, nearest, nonzero_rows, records_of, reference_metrics
from conftest import ROOT
from models import build_model_from_cfg
from utils import evaluate, misc
from utils.config import builtin_cfg
from upp_hip import functional as HF
from upp_hip import infer, ops

pytestmark = pytest.mark.gpu

TH = 0.01


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _pair(B, n, m, seed):
    """gt (B, m, 3) in the unit ball; x (B, n, 3): points of gt moved by 0.002 / 0.0099 / 0.0101 / 0.03 (both sides of TH)."""
    rng = np.random.default_rng(seed)
    gt = _seeded.unit_ball_clouds(B, m, seed=seed).numpy()
    x = np.empty((B, n, 3), np.float32)
    for b in range(B):
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        x[b] = gt[b][rng.integers(0, m, n)] + u * rng.choice([0.002, 0.0099, 0.0101, 0.03], n)[:, None]
    return x, gt


def _dist64(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def _count_with_tie_allowance(x, y, idx):
    """The F-Score count of x against y by the kernel's rule (exact), and a check that the float64 nearest neighbour disagrees with it
    only where the two candidates tie within f32 rounding on opposite sides of TH."""
    dk = _dist64(x, y[idx])
    exact = int((dk < TH).sum())
    dmin = np.sqrt(nearest(x, y)[0])
    differ = (dk < TH) != (dmin < TH)
    assert np.all(dk[differ] ** 2 - dmin[differ] ** 2 <= 4e-7 * dmin[differ] ** 2 + 1e-12), "only f32 ties may disagree"
    return exact


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n,m", [(2048, 8192), (160, 8192), (157, 1001), (1, 5)])
def test_the_cloud_kernels_match_the_reference(n, m):
    B = 3
    x, gt = _pair(B, n, m, seed=n + m)
    X, G = torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda()
    acc = ops.CompletionAccumulator(1, 'cuda')
    ops.completion_cloud_metrics(X, X, G, acc, True, TH)
    d1, d2, i1, i2 = (t.cpu().numpy() for t in ops.chamfer_fwd(X, G))
    stats, counts = acc.dense.cpu().numpy(), acc.dense_counts.cpu().numpy()
    assert np.array_equal(np.delete(stats, 4, 1), np.delete(acc.sparse.cpu().numpy(), 4, 1)), "the same pair: the same means"
    for b in range(B):
        own = [d1[b].astype(np.float64), d2[b].astype(np.float64)]
        want = [own[0].mean(), own[1].mean(), np.sqrt(own[0]).mean(), np.sqrt(own[1]).mean()]
        np.testing.assert_allclose(stats[b, :4], want, rtol=1e-12, atol=0)
        bf = [nearest(x[b], gt[b])[0], nearest(gt[b], x[b])[0]]
        np.testing.assert_allclose(stats[b, :4], [bf[0].mean(), bf[1].mean(), np.sqrt(bf[0]).mean(), np.sqrt(bf[1]).mean()],
                                   rtol=1e-5)
        p = _count_with_tie_allowance(x[b], gt[b], i1[b])
        r = _count_with_tie_allowance(gt[b], x[b], i2[b])
        assert counts[b, :2].tolist() == [p, r]
        prec, rec = float(p) / n, float(r) / m
        f = 2 * rec * prec / (rec + prec) if rec + prec else 0.
        assert _bits(stats[b, 4]) == _bits(f)
        assert counts[b, 2] == 0 and stats[b, 5] == (stats[b, 2] + stats[b, 3]) / 2 and stats[b, 6] == stats[b, 0] + stats[b, 1]
    assert acc.sparse_counts.cpu().numpy().tolist() == [[0, 0, 0, 0]] * B, "no detail on the sparse pair"


def test_the_ignore_zeros_pass_runs_only_on_clouds_with_zero_sum_points():
    B, n, m = 4, 300, 1000
    x, gt = _pair(B, n, m, seed=11)
    x[1, :3] = [[0.5, -0.25, -0.25], [0, 0, 0], [0.25, 0.25, -0.5]]
    gt[2, 7] = [-1.0, 0.5, 0.5]
    x[3] = [0.5, -0.25, -0.25]                                          # every point zero-sum: NaN
    X, G = torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda()
    acc = ops.CompletionAccumulator(1, 'cuda')
    ops.completion_cloud_metrics(X, X, G, acc, True, TH)
    stats, counts = acc.dense.cpu().numpy(), acc.dense_counts.cpu().numpy()
    assert counts[:, 2].tolist() == [0, 1, 1, 1]
    assert _bits(stats[0, 5]) == _bits((stats[0, 2] + stats[0, 3]) / 2) and _bits(stats[0, 6]) == _bits(stats[0, 0] + stats[0, 1])
    for b in (1, 2):
        a, g = x[b][nonzero_rows(x[b])], gt[b][nonzero_rows(gt[b])]
        e1, e2 = nearest(a, g)[0], nearest(g, a)[0]
        np.testing.assert_allclose(stats[b, 5:7], [(np.sqrt(e1).mean() + np.sqrt(e2).mean()) / 2, e1.mean() + e2.mean()], rtol=1e-5)
        assert stats[b, 6] != stats[b, 0] + stats[b, 1]
    assert np.isnan(stats[3, 5]) and np.isnan(stats[3, 6]) and not np.isnan(stats[3, 0])


def _device_metric(batches, C=3, detail=True):
    m = evaluate.CompletionMetric(C)
    for gt, coarse, dense, cat in batches:
        m.update(torch.from_numpy(coarse).cuda(), torch.from_numpy(dense).cuda(), torch.from_numpy(gt).cuda(),
                 torch.tensor(cat).cuda() if detail else None)
    return m


def _metric_batches():
    out = []
    for i in range(2):
        dense, gt = _pair(6, 500, 1200, seed=20 + i)                      # V = 2 viewpoints of B = 3 clouds
        gt = gt[:3]
        coarse = _pair(6, 40, 1200, seed=30 + i)[0]
        out.append((gt, coarse, dense, [i, 2, 0]))
    return out


def test_the_device_metric_matches_the_reference_and_repeats_bit_for_bit():
    batches = _metric_batches()
    a, b = _device_metric(batches), _device_metric(batches)
    for name in ('loss_sum', 'counters', 'cat_sum', 'cat_cnt'):
        assert torch.equal(getattr(a.sums, name), getattr(b.sums, name)), name
    want = reference_metrics(sum((records_of(c, d, g, k, 2) for g, c, d, k in batches), []), True)
    assert_completion_match(a.compute(), want, rel=1e-5, f_abs=1e-3)
    assert int(a.sums.counters[0]) == 12 and a.sums.cat_cnt.tolist() == [6, 2, 4]
    host = evaluate.CompletionMetric(3)
    for gt, coarse, dense, cat in batches:
        host.update(torch.from_numpy(coarse), torch.from_numpy(dense), torch.from_numpy(gt), torch.tensor(cat))
    assert_completion_match(host.compute(), a.compute(), rel=1e-5, f_abs=1e-3)
    losses = _device_metric(batches, detail=False).compute()
    assert losses['category_metrics'] == {} and losses['dense_cd_l2'] == a.compute()['dense_cd_l2']


def test_bad_tensors_are_refused_before_any_launch():
    acc = ops.CompletionAccumulator(2, 'cuda')
    x = torch.zeros(4, 8, 3, device='cuda')
    g = torch.zeros(2, 8, 3, device='cuda')
    with pytest.raises(RuntimeError, match="float32"):
        ops.completion_update(x.double(), x, g, acc)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.completion_update(x.transpose(0, 1), x, g, acc)
    with pytest.raises(RuntimeError, match="last dim"):
        ops.completion_update(x[..., :2].contiguous(), x, g, acc)
    with pytest.raises(RuntimeError, match="V x 2"):
        ops.completion_update(x[:3].contiguous(), x[:3].contiguous(), g, acc)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.completion_update(x, x, g.cpu(), acc)
    with pytest.raises(RuntimeError, match="category"):
        ops.completion_update(x, x, g, acc, category=torch.zeros(3, dtype=torch.long, device='cuda'))
    with pytest.raises(RuntimeError, match="n_valid"):
        ops.completion_update(x, x, g, acc, n_valid=3)
    with pytest.raises(RuntimeError, match="th"):
        ops.completion_update(x, x, g, acc, th=0.0)
    assert acc.counters.tolist() == [0, 0]


# ------------------------------------------------------------------ protocols on a seeded model
N_PTS = 2048


def _model():
    return _seeded.fill(build_model_from_cfg(builtin_cfg('pretask').model)).cuda().train()


def _batches(sizes, seed=0, N=N_PTS):
    return [(_seeded.unit_ball_clouds(b, N, seed=seed + i).cuda(), torch.arange(b, device='cuda') % 3) for i, b in enumerate(sizes)]


def _same(a, b):
    for k, v in a.items():
        if k == 'category_metrics':
            assert list(v) == list(b[k])
            for c in v:
                _same(v[c], b[k][c])
        else:
            assert v == b[k] or (v != v and b[k] != b[k]), (k, v, b[k])


def _reference_of_the_batched_outputs(model, batches, mode, in_detail):
    model.eval()
    records = []
    try:
        with torch.no_grad():
            for gt, cat in batches:
                centers = torch.tensor(evaluate.viewpoints(in_detail), device='cuda')
                coarse, dense = evaluate.completion_outputs(model, gt, centers, evaluate.crop_count(gt.shape[1], mode))
                records += records_of(coarse.cpu().numpy(), dense.cpu().numpy(), gt.cpu().numpy(), cat.tolist(), len(centers))
    finally:
        model.train()
    return reference_metrics(records, in_detail)


def _reference_loop(model, batches, mode, in_detail):
    """The reference's loop verbatim: batch size 1, one crop, two FPS and one forward per (cloud, viewpoint)."""
    model.eval()
    records = []
    try:
        with torch.no_grad():
            for gt_b, cat in batches:
                for b in range(gt_b.shape[0]):
                    gt = gt_b[b:b + 1]
                    npoints = gt.shape[1]
                    for item in evaluate.viewpoints(in_detail):
                        partial, _ = misc.seprate_point_cloud(gt, npoints, int(npoints * evaluate.CROP_RATIO[mode]),
                                                              fixed_points=torch.tensor(item))
                        partial, _ = misc.fps(partial, 1024)
                        partial_center, _ = misc.fps(partial, 128)
                        pred_center, rebuild = model(partial, train_with_gaussian=False, predict_center_num=16)
                        coarse = torch.cat([partial_center, pred_center], dim=1)
                        dense = torch.cat([partial, rebuild], dim=1)
                        records.append((coarse[0].cpu().numpy(), dense[0].cpu().numpy(), gt[0].cpu().numpy(), int(cat[b])))
    finally:
        model.train()
    return reference_metrics(records, in_detail)


@pytest.mark.parametrize("mode,in_detail", [('easy', False), ('median', True)])
def test_validate_completion_is_the_reference_protocol(mode, in_detail):
    model = _model()
    batches = _batches([3, 2], seed=10)
    out = evaluate.validate_completion(model, batches, mode=mode, in_detail=in_detail, num_categories=3)
    assert model.training, "the training flag is restored"
    want = _reference_of_the_batched_outputs(model, batches, mode, in_detail)
    # the same batched forward: only the device's f32 Chamfer distances (and F-Score ties) separate the two
    assert_completion_match(out, want, rel=1e-5, f_abs=1e-3)
    assert out['dense_cd_l2'] > 0 and (not in_detail or len(out['category_metrics']) == 3)
    # the reference's batch-1 loop: other forwards (batch 1 against 2-3 clouds x V) and an unstable argsort in the crop
    loop = _reference_loop(model, batches, mode, in_detail)
    assert_completion_match(out, loop, rel=1e-3, f_abs=2e-2)


def test_validate_completion_captured_matches_eager_bit_for_bit():
    model = _model()
    batches = _batches([3, 3, 2], seed=20)                                # ragged last batch: padded 2 -> 3
    rng = torch.cuda.get_rng_state(), torch.get_rng_state()
    for in_detail in (True, False):
        eager = evaluate.validate_completion(model, batches, mode='easy', in_detail=in_detail, num_categories=3)
        captured = evaluate.validate_completion_captured(model, batches, mode='easy', in_detail=in_detail, num_categories=3)
        _same(captured, eager)
    assert model.training
    assert torch.equal(torch.cuda.get_rng_state(), rng[0]) and torch.equal(torch.get_rng_state(), rng[1]), "nothing is drawn"
    steps = [s for s in infer._STEPS[model].values() if isinstance(s, infer.CompletionEvalStep)]
    assert sorted({s.B for s in steps}) == [2, 3], "the ragged last batch runs a graph of its own size"
    # a step also takes a smaller batch padded with its last cloud: equal to the eager metric up to the forward's f32 rounding
    step = infer.CompletionEvalStep(model, (3, N_PTS, 3), in_detail=True)
    step.prepare()
    padded = evaluate.CompletionMetric(3)
    model.eval()
    try:
        step.run(batches[2][0], batches[2][1], padded)
    finally:
        model.train()
    assert int(padded.sums.counters[0]) == 2 * 8
    want = evaluate.validate_completion(model, batches[2:], mode='easy', in_detail=True, num_categories=3)
    assert_completion_match(padded.compute(), want, rel=1e-6, f_abs=1e-3)


def test_captured_evaluation_follows_an_optimizer_step_and_loaded_weights():
    model = _model()
    batches = _batches([3, 2], seed=30)
    kw = dict(mode='easy', in_detail=True, num_categories=3)
    before = evaluate.validate_completion_captured(model, batches, **kw)
    # (a) an optimizer step: contents change in place, addresses stay
    opt = torch.optim.SGD(model.parameters(), lr=1.0)
    g = torch.Generator(device='cuda').manual_seed(3)
    for p in model.parameters():
        p.grad = 1e-3 * torch.randn(p.shape, device='cuda', generator=g) * p.detach().abs().mean()
    opt.step()
    after = evaluate.validate_completion_captured(model, batches, **kw)
    _same(after, evaluate.validate_completion(model, batches, **kw))
    assert after['dense_cd_l2'] != before['dense_cd_l2']
    # (b) load_state_dict
    sd = model.state_dict()
    gen = torch.Generator().manual_seed(5)
    new = {k: (v + 0.05 * torch.randn(v.shape, generator=gen).to(v.device) * v.abs().mean() if v.is_floating_point() else v)
           for k, v in sd.items()}
    model.load_state_dict(new)
    loaded = evaluate.validate_completion_captured(model, batches, **kw)
    _same(loaded, evaluate.validate_completion(model, batches, **kw))
    assert loaded['dense_cd_l2'] != after['dense_cd_l2']


def test_a_model_that_reads_across_samples_is_refused():
    cfg = builtin_cfg('pretask').model
    cfg.gather_idx = False
    m = build_model_from_cfg(cfg).cuda()
    with pytest.raises(ValueError, match="per sample"):
        infer.CompletionEvalStep(m, (4, N_PTS, 3))


def test_a_completion_evaluation_is_graph_safe():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from memset_census import memsets_of
    model = _model()
    (gt, cat), = _batches([3], seed=40)
    step = infer.CompletionEvalStep(model, (3, N_PTS, 3), in_detail=True, use_graph=False)
    m = evaluate.CompletionMetric(3)
    step.prepare()
    step.run(gt, cat, m)                                        # warm-up: lazy caches
    HF._declined.clear()
    model.eval()
    try:
        assert memsets_of(step._evaluate) == []
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            step._evaluate()
            torch.cuda.synchronize()
        assert memsets_of(lambda: ops.completion_accumulate(m.sums, step.V, step.B, step.category, 3, rows=step.rows)) == []
    finally:
        model.train()
    names = [e.key for e in prof.key_averages()]
    assert not [k for k in names if k.startswith('Cijk') or 'rocprim' in k.lower() or 'radixsort' in k.lower()], names
    assert HF._declined == set()


def test_a_full_size_batch():
    model = _model()
    N = 8192
    batches = [(_seeded.unit_ball_clouds(32, N, seed=50).cuda(), torch.arange(32, device='cuda') % 5)]
    kw = dict(mode='easy', in_detail=True, num_categories=5)
    eager = evaluate.validate_completion(model, batches, **kw)
    captured = evaluate.validate_completion_captured(model, batches, **kw)
    _same(captured, eager)
    step = [s for s in infer._STEPS[model].values() if isinstance(s, infer.CompletionEvalStep)][-1]
    assert (step.B, step.N, step.V) == (32, N, 8)
    assert sum(v['count'] for v in eager['category_metrics'].values()) == 256
    coarse, dense = step.coarse.cpu().numpy(), step.dense.cpu().numpy()
    assert coarse.shape == (256, 160, 3) and dense.shape == (256, 2048, 3)
    gt = batches[0][0].cpu().numpy()
    rows = step.rows.dense.cpu().numpy()
    for r in (0, 37, 255):                                      # spot rows against float64 brute force
        d1, d2 = nearest(dense[r], gt[r % 32])[0], nearest(gt[r % 32], dense[r])[0]
        np.testing.assert_allclose(rows[r, :4], [d1.mean(), d2.mean(), np.sqrt(d1).mean(), np.sqrt(d2).mean()], rtol=1e-5)
    for k in ('sparse_cd_l1', 'dense_cd_l1', 'f_score', 'cd_l1'):
        assert np.isfinite(eager[k]), k
