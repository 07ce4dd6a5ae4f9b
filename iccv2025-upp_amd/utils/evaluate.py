"""Evaluation loops of the reference classification runner (tools/runner_module.py:370-490), on device:
`validate` = one pass, arg-max accuracy; `test_vote` = the 10x voting protocol (FPS to a 1200-point superset once,
then `times` random 1024-subsets, each scale/translate-augmented; logits averaged before the arg-max)."""
import torch

from utils import dist_utils, misc
from upp_hip import functional as HF


def _accuracy(pred, label, distributed):
    pred, label = torch.cat(pred), torch.cat(label)
    if distributed:
        pred, label = dist_utils.gather_tensor(pred), dist_utils.gather_tensor(label)
    return (pred == label).sum() / float(label.size(0)) * 100.


@torch.no_grad()
def validate(model, batches, npoints, noisy=False, distributed=False):
    """batches: iterable of (points (B,N,3), label (B,)).  runner_module.py:383-413."""
    model.eval()
    preds, labels = [], []
    for points, label in batches:
        points = misc.fps(points.contiguous(), npoints)[0]
        logits = model(points, completion_prompt=noisy, denoise=noisy, point_num=npoints)
        preds.append(logits.argmax(-1).view(-1))
        labels.append(label.view(-1))
    return _accuracy(preds, labels, distributed)


@torch.no_grad()
def test_vote(model, batches, npoints, times=10, transform=misc.scale_translate, distributed=False, generator=None):
    """runner_module.py:427-490.  The random subsets are drawn on the device (torch.randperm) instead of
    np.random.choice on the host: same distribution, no host round trip per vote."""
    superset = {1024: 1200, 4096: 4800, 8192: 8192}
    if npoints not in superset:
        raise NotImplementedError()
    model.eval()
    preds, labels = [], []
    for points_raw, label in batches:
        point_all = min(superset[npoints], points_raw.size(1))
        raw, _ = HF.fps_gather(points_raw.contiguous(), point_all)                # (B, point_all, 3) FPS-ordered superset
        votes = []
        for _ in range(times):
            pick = torch.randperm(point_all, device=raw.device, generator=generator)[:npoints]
            points = raw[:, pick].contiguous()
            if transform is not None:
                points = transform(points)
            votes.append(model(points).unsqueeze(0))
        preds.append(torch.cat(votes, dim=0).mean(0).argmax(-1))
        labels.append(label.view(-1))
    return _accuracy(preds, labels, distributed)


# ------------------------------------------------------------------ the same protocols, captured (upp_hip.infer.EvalStep)
def _run_captured(model, batches, npoints, kw, generator, distributed, return_predictions):
    """One EvalStep per (B, N_raw) of the batches (a batch smaller than the step in use is padded into it); the accuracy is
    `_accuracy`'s expression over the device counters (correct, total), all-reduced outside the graph when distributed."""
    from upp_hip.infer import EvalStep
    was = model.training
    model.eval()
    steps, step, preds = [], None, []
    try:
        for points, label in batches:
            n, n_raw = points.shape[0], points.shape[1]
            if step is None or step.B < n or step.n_raw != n_raw:
                step = EvalStep.cached(model, (n, n_raw, 3), npoints, **kw)
                if step not in steps:
                    step.prepare()
                    step.counters.zero_()
                    steps.append(step)
            pred = step.run(points.contiguous(), label.view(-1), generator=generator)
            if return_predictions:
                preds.append(pred.clone())
    finally:
        model.train(was)
    if not steps:
        return _accuracy([], [], distributed)
    counters = steps[0].counters.clone()
    for s in steps[1:]:
        counters += s.counters
    if distributed:
        torch.distributed.all_reduce(counters)
    acc = counters[0] / float(int(counters[1])) * 100.
    return (acc, torch.cat(preds)) if return_predictions else acc


@torch.no_grad()
def validate_captured(model, batches, npoints, noisy=False, distributed=False, return_predictions=False):
    """`validate` as one HIP-graph replay per batch (FPS, the eval forward) plus one reduction launch.  return_predictions: also
    this rank's arg-max predictions (n,) int64 of the real clouds, in batch order."""
    return _run_captured(model, batches, npoints, dict(votes=1, noisy=bool(noisy), transform=False), None, distributed,
                         return_predictions)


@torch.no_grad()
def test_vote_captured(model, batches, npoints, times=10, transform=misc.scale_translate, distributed=False, generator=None,
                       max_clouds=None, return_predictions=False):
    """`test_vote` with the `times` votes of a batch inside ONE HIP graph: FPS to the superset, the random subsets and their
    scale/translate (upp_vote_points) as one vote-major batch, the forwards in chunks of at most `max_clouds` clouds, then the vote mean
    and arg-max (upp_vote_reduce).  The random draws are test_vote's, in its order (same seeds: same subsets and transforms).
    max_clouds None: all votes in one forward -- or, for a model whose forward reads across the samples of its batch
    (upp_hip.infer.mixes_samples: the reference's propagation indexing with gather_idx = false), one vote per forward, which is what
    keeps the logits those of test_vote; a larger max_clouds then batches votes at the price of that equality.
    `transform`: misc.scale_translate (with its default ranges) or None; another callable cannot run inside the kernel."""
    superset = {1024: 1200, 4096: 4800, 8192: 8192}
    if npoints not in superset:
        raise NotImplementedError()
    if transform is not None and transform is not misc.scale_translate:
        raise NotImplementedError("test_vote_captured applies misc.scale_translate (or no transform) on the device")
    kw = dict(votes=int(times), transform=transform is not None, superset=superset[npoints], max_clouds=max_clouds)
    return _run_captured(model, batches, npoints, kw, generator, distributed, return_predictions)
