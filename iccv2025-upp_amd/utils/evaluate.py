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


# ------------------------------------------------------------------ part segmentation (reference tools/runner_unify_seg.py:301-367)
# ShapeNetPart: 16 categories in the dataset's category order, each owning a contiguous range of the 50 part labels
# (reference tools/runner_unify_seg.py:79-82, datasets/PartNormalDataset.py).
SHAPENET_PART = (('Airplane', (0, 1, 2, 3)), ('Bag', (4, 5)), ('Cap', (6, 7)), ('Car', (8, 9, 10, 11)), ('Chair', (12, 13, 14, 15)),
                 ('Earphone', (16, 17, 18)), ('Guitar', (19, 20, 21)), ('Knife', (22, 23)), ('Lamp', (24, 25, 26, 27)),
                 ('Laptop', (28, 29)), ('Motorbike', (30, 31, 32, 33, 34, 35)), ('Mug', (36, 37)), ('Pistol', (38, 39, 40)),
                 ('Rocket', (41, 42, 43)), ('Skateboard', (44, 45, 46)), ('Table', (47, 48, 49)))


def seg_tables(classes=SHAPENET_PART):
    """(names, part_cat (P,) int32, cat_range (C, 2) int32 = [lo, n)) of a part table; every part belongs to exactly one category and
    every category's parts are one contiguous, non-empty range."""
    names = [name for name, _ in classes]
    P = sum(len(parts) for _, parts in classes)
    part_cat = torch.full((P,), -1, dtype=torch.int32)
    cat_range = torch.zeros((len(classes), 2), dtype=torch.int32)
    for c, (_, parts) in enumerate(classes):
        parts = list(parts)
        if not parts or parts != list(range(parts[0], parts[0] + len(parts))) or parts[0] < 0 or parts[-1] >= P:
            raise ValueError("category %d: parts %s are not a contiguous range inside [0, %d)" % (c, parts, P))
        if bool((part_cat[parts[0]:parts[-1] + 1] >= 0).any()):
            raise ValueError("category %d: a part of %s belongs to another category" % (c, parts))
        part_cat[parts[0]:parts[-1] + 1] = c
        cat_range[c, 0], cat_range[c, 1] = parts[0], len(parts)
    return names, part_cat, cat_range


def one_hot(label, num_classes):
    """(B,) or (B, 1) int -> (B, num_classes) f32: the reference's to_categorical (a label outside the range gives a zero row)."""
    label = label.reshape(-1, 1)
    return (label == torch.arange(num_classes, device=label.device)).float()


class _HostSums:
    """SegMetric's sums on the CPU: the fields of upp_hip.ops.SegAccumulator."""

    def __init__(self, P, C):
        self.counters = torch.zeros(3, dtype=torch.int64)
        self.part_seen = torch.zeros(P, dtype=torch.int64)
        self.part_correct = torch.zeros(P, dtype=torch.int64)
        self.cat_sum = torch.zeros(C, dtype=torch.float64)
        self.cat_cnt = torch.zeros(C, dtype=torch.int64)


def _seg_update_host(logp, target, part_cat, cat_range, sums, n_valid, pred=None):
    """The arithmetic of upp_seg_iou_counts + upp_seg_iou_accumulate in torch on the CPU (the same integers, the same float64
    operations in the same order) -> the per-shape IoUs of shapes [0, n_valid)."""
    B, N, P = logp.shape
    C = cat_range.shape[0]
    part_cat, cat_range = part_cat.long(), cat_range.long()
    t0 = target[:, 0]
    in0 = (t0 >= 0) & (t0 < P)
    cat = torch.where(in0, part_cat[t0.clamp(0, P - 1)], torch.full_like(t0, -1))
    ok = (cat >= 0) & (cat < C)
    lo = torch.where(ok, cat_range[cat.clamp(0, C - 1), 0], torch.zeros_like(cat))
    cnt = torch.where(ok, cat_range[cat.clamp(0, C - 1), 1], torch.zeros_like(cat))
    ok = ok & (lo >= 0) & (cnt >= 1) & (lo + cnt <= P)
    cnt = torch.where(ok, cnt, torch.zeros_like(cnt))
    K = int(cnt.max()) if B else 0

    def column(k):
        return logp.gather(2, (lo + k).clamp(0, P - 1).view(B, 1, 1).expand(B, N, 1)).squeeze(2)
    best, bk = column(0), torch.zeros((B, N), dtype=torch.long)
    for k in range(1, K):                       # np.argmax: a NaN best stays, a NaN replaces a number, else only a larger value
        v = column(k)
        rep = (k < cnt).view(B, 1) & ~torch.isnan(best) & (torch.isnan(v) | (v > best))
        best, bk = torch.where(rep, v, best), torch.where(rep, torch.full_like(bk, k), bk)
    p = torch.where(ok.view(B, 1), lo.view(B, 1) + bk, torch.full_like(bk, -1))
    if pred is not None:
        pred.copy_(p)

    rows = (torch.arange(B) < n_valid) & ok
    m = rows.view(B, 1).expand(B, N)
    hit = (p == target) & m
    t_in = m & (target >= 0) & (target < P)
    sums.counters += torch.stack([hit.sum(), torch.tensor(n_valid * N), (~ok[:n_valid]).sum()])
    sums.part_seen += torch.bincount(target[t_in], minlength=P)
    sums.part_correct += torch.bincount(target[t_in & hit], minlength=P)
    base = (torch.arange(B) * P).view(B, 1)
    in_cat = m & (target >= lo.view(B, 1)) & (target < (lo + cnt).view(B, 1))
    predc = torch.bincount((base + p - lo.view(B, 1))[m], minlength=B * P).view(B, P)
    tgtc = torch.bincount((base + target - lo.view(B, 1))[in_cat], minlength=B * P).view(B, P)
    inter = torch.bincount((base + target - lo.view(B, 1))[in_cat & hit], minlength=B * P).view(B, P)
    union = tgtc + predc - inter
    part_iou = torch.where(union == 0, torch.ones((), dtype=torch.float64), inter.double() / union.double())
    s = torch.zeros(B, dtype=torch.float64)
    for k in range(K):                          # sequential in part order, then one division
        s = torch.where(k < cnt, s + part_iou[:, k], s)
    iou = torch.where(ok, s / cnt.double(), torch.full_like(s, float('nan')))[:n_valid]
    cs, cc = sums.cat_sum.tolist(), sums.cat_cnt.tolist()
    for b, (c, v) in enumerate(zip(cat[:n_valid].tolist(), iou.tolist())):      # per category, in shape order
        if ok[b]:
            cs[c] += v
            cc[c] += 1
    sums.cat_sum.copy_(torch.tensor(cs, dtype=torch.float64))
    sums.cat_cnt.copy_(torch.tensor(cc, dtype=torch.int64))
    return iou


class SegMetric:
    """The part-segmentation metrics of the reference's `validate` (tools/runner_unify_seg.py:301-367), accumulated batch by batch.

    update(logp (B, N, P) log-probabilities, target (B, N) part labels, n_valid=None, pred=None): shapes [0, n_valid) count.  The category
    of shape i is the one that owns target[i, 0] (not its object label); its prediction is the first arg-max of the log-probabilities
    restricted to that category's parts (np.argmax: a NaN wins).  HIP tensors run the metric kernels (upp_hip.ops.seg_iou_update: no
    log-probability leaves the device); CPU tensors the same arithmetic in torch.  pred: a (B, N) int64 tensor the predictions are
    written to.  Returns the per-shape IoUs (n_valid,) f64.

    compute(distributed=False) -> {'accuracy', 'class_avg_accuracy', 'class_avg_iou', 'inctance_avg_iou' (the reference's key),
    'category_iou': {name: mean shape IoU}}.  A part never seen makes class_avg_accuracy NaN and a category without shapes makes
    class_avg_iou NaN, as in the reference.  distributed: the integer and float64 sums are all-reduced before the divisions.  A shape
    whose target[i, 0] is no part label raises here (the reference fails on it with a KeyError)."""

    def __init__(self, num_part=50, num_classes=16, classes=SHAPENET_PART):
        self.names, self.part_cat, self.cat_range = seg_tables(classes)
        if len(self.part_cat) != num_part or len(self.names) != num_classes:
            raise ValueError("the part table has %d parts in %d categories, not %d in %d" % (len(self.part_cat), len(self.names),
                                                                                           num_part, num_classes))
        self.num_part, self.num_classes = int(num_part), int(num_classes)
        self.sums = None
        self._tables = None

    def update(self, logp, target, n_valid=None, pred=None):
        B, N = logp.shape[0], logp.shape[1]
        if logp.dim() != 3 or logp.shape[2] != self.num_part:
            raise ValueError("logp must be (B, N, %d), got %s" % (self.num_part, tuple(logp.shape)))
        target = target.reshape(B, N).to(logp.device, torch.long).contiguous()
        n_valid = B if n_valid is None else int(n_valid)
        if not 0 <= n_valid <= B:
            raise ValueError("n_valid %d outside [0, %d]" % (n_valid, B))
        if logp.is_cuda:
            from upp_hip import ops
            if self.sums is None:
                self.sums = ops.SegAccumulator(self.num_part, self.num_classes, logp.device)
                self._tables = (self.part_cat.to(logp.device), self.cat_range.to(logp.device))
            elif not isinstance(self.sums, ops.SegAccumulator) or self.sums.device != logp.device:
                raise RuntimeError("SegMetric: all updates must come from one device")
            return ops.seg_iou_update(logp, target, self._tables[0], self._tables[1], self.sums, n_valid, pred)
        if self.sums is None:
            self.sums = _HostSums(self.num_part, self.num_classes)
        elif not isinstance(self.sums, _HostSums):
            raise RuntimeError("SegMetric: all updates must come from one device")
        return _seg_update_host(logp.detach().float(), target, self.part_cat, self.cat_range, self.sums, n_valid, pred)

    def compute(self, distributed=False):
        import numpy as np
        s = self.sums if self.sums is not None else _HostSums(self.num_part, self.num_classes)
        ints = torch.cat([s.counters, s.part_seen, s.part_correct, s.cat_cnt])
        cat_sum = s.cat_sum.clone()
        if distributed:
            torch.distributed.all_reduce(ints)
            torch.distributed.all_reduce(cat_sum)
        ints, cat_sum = ints.cpu().numpy(), cat_sum.cpu().numpy()
        P = self.num_part
        (correct, seen, invalid), part_seen, part_correct, cat_cnt = ints[:3], ints[3:3 + P], ints[3 + P:3 + 2 * P], ints[3 + 2 * P:]
        if invalid:
            raise ValueError("%d shape(s) have a first target outside the %d part labels: their category is unknown" % (invalid, P))
        with np.errstate(divide='ignore', invalid='ignore'):
            cat_iou = cat_sum / cat_cnt.astype(np.float64)
            return {'accuracy': float(np.float64(correct) / np.float64(seen)),
                    'class_avg_accuracy': float(np.mean(part_correct / part_seen.astype(np.float64))),
                    'class_avg_iou': float(np.mean(cat_iou)),
                    'inctance_avg_iou': float(cat_sum.sum() / np.float64(cat_cnt.sum())),
                    'category_iou': {name: float(v) for name, v in zip(self.names, cat_iou)}}


def _seg_batch(points, label, target):
    B, N = points.shape[0], points.shape[1]
    return points.contiguous(), label.reshape(-1), target.reshape(B, N)


@torch.no_grad()
def validate_seg(model, batches, num_part=50, num_classes=16, distributed=False, return_predictions=False, classes=SHAPENET_PART):
    """batches: iterable of (points (B, N, 3), label (B,) or (B, 1), target (B, N)).  The reference's `validate` of the part-segmentation
    runner (tools/runner_unify_seg.py:301-367) with an eager forward: log-probabilities of model(points, one_hot(label),
    completion_prompt=False, denoise=False, point_num=N) into a SegMetric -> its compute(distributed) dict; with return_predictions also
    this rank's predictions (n, N) int64, in batch order.  The model's training flag is restored afterwards."""
    metric = SegMetric(num_part, num_classes, classes)
    was = model.training
    model.eval()
    preds = []
    try:
        for points, label, target in batches:
            points, label, target = _seg_batch(points, label, target)
            logp = model(points, one_hot(label.to(points.device), num_classes), completion_prompt=False, denoise=False,
                         point_num=points.shape[1])
            pred = torch.empty(target.shape, dtype=torch.long, device=logp.device) if return_predictions else None
            metric.update(logp, target, pred=pred)
            if return_predictions:
                preds.append(pred)
    finally:
        model.train(was)
    out = metric.compute(distributed)
    return (out, torch.cat(preds) if preds else torch.empty((0, 0), dtype=torch.long)) if return_predictions else out


@torch.no_grad()
def validate_seg_captured(model, batches, num_part=50, num_classes=16, distributed=False, return_predictions=False,
                          classes=SHAPENET_PART):
    """`validate_seg` with each batch's forward one HIP-graph replay (upp_hip.infer.SegEvalStep, one per (B, N); a smaller batch is
    padded into the step in use) and the metric on the device.  Same arguments and results."""
    from upp_hip.infer import SegEvalStep
    metric = SegMetric(num_part, num_classes, classes)
    was = model.training
    model.eval()
    steps, step, preds = [], None, []
    try:
        for points, label, target in batches:
            points, label, target = _seg_batch(points, label, target)
            n, N = points.shape[0], points.shape[1]
            if step is None or step.B < n or step.N != N:
                step = SegEvalStep.cached(model, (n, N, 3), num_classes)
                if step not in steps:
                    step.prepare()
                    steps.append(step)
            pred = step.run(points, label.to(step.device), target.to(step.device), metric)
            if return_predictions:
                preds.append(pred.clone())
    finally:
        model.train(was)
    out = metric.compute(distributed)
    return (out, torch.cat(preds) if preds else torch.empty((0, 0), dtype=torch.long)) if return_predictions else out
