"""Evaluation loops of the reference classification runner (tools/runner_module.py:370-490), on device:
`validate` = one pass, arg-max accuracy; `test_vote` = the 10x voting protocol (FPS to a 1200-point superset once,
then `times` random 1024-subsets, each scale/translate-augmented; logits averaged before the arg-max)."""
import contextlib

import torch

from utils import dist_utils, misc
from upp_hip import functional as HF, infer


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
    if npoints not in infer.SUPERSET:
        raise NotImplementedError()
    model.eval()
    preds, labels = [], []
    for points_raw, label in batches:
        point_all = min(infer.SUPERSET[npoints], points_raw.size(1))
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


# ------------------------------------------------------------------ the same protocols, captured (upp_hip.infer)
@contextlib.contextmanager
def _evaluating(model):
    """model.eval() inside (every sub-module, whatever the top-level flag was), the model's training flag again after."""
    was = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was)


def _run_steps(model, batches, make, fits, run, first=None):
    """The loop of the captured protocols, the model in eval mode meanwhile.  Per batch, whose first member holds n clouds of N points:
    the step in use while fits(step, n, N), else make(n, N) (the cached step of that shape); a step met for the first time in this call
    is brought up to date with the model's weights (prepare()) and passed to `first`; then run(step, batch).  -> the steps used, in
    the order they were first met."""
    steps, step = [], None
    with _evaluating(model):
        for batch in batches:
            n, N = batch[0].shape[0], batch[0].shape[1]
            if step is None or not fits(step, n, N):
                step = make(n, N)
                if step not in steps:
                    step.prepare()
                    if first is not None:
                        first(step)
                    steps.append(step)
            run(step, batch)
    return steps


def _run_captured(model, batches, npoints, kw, generator, distributed, return_predictions):
    """One EvalStep per (B, N_raw) of the batches (a batch smaller than the step in use is padded into it); the accuracy is
    `_accuracy`'s expression over the device counters (correct, total), all-reduced outside the graph when distributed."""
    preds = []

    def run(step, batch):
        pred = step.run(batch[0].contiguous(), batch[1].view(-1), generator=generator)
        if return_predictions:
            preds.append(pred.clone())
    steps = _run_steps(model, batches, lambda n, N: infer.EvalStep.cached(model, (n, N, 3), npoints, **kw),
                       lambda s, n, N: s.B >= n and s.n_raw == N, run, first=lambda s: s.counters.zero_())
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
    if npoints not in infer.SUPERSET:
        raise NotImplementedError()
    if transform is not None and transform is not misc.scale_translate:
        raise NotImplementedError("test_vote_captured applies misc.scale_translate (or no transform) on the device")
    kw = dict(votes=int(times), transform=transform is not None, superset=infer.SUPERSET[npoints], max_clouds=max_clouds)
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
    preds = []
    with _evaluating(model):
        for points, label, target in batches:
            points, label, target = _seg_batch(points, label, target)
            logp = model(points, one_hot(label.to(points.device), num_classes), completion_prompt=False, denoise=False,
                         point_num=points.shape[1])
            pred = torch.empty(target.shape, dtype=torch.long, device=logp.device) if return_predictions else None
            metric.update(logp, target, pred=pred)
            if return_predictions:
                preds.append(pred)
    out = metric.compute(distributed)
    return (out, torch.cat(preds) if preds else torch.empty((0, 0), dtype=torch.long)) if return_predictions else out


@torch.no_grad()
def validate_seg_captured(model, batches, num_part=50, num_classes=16, distributed=False, return_predictions=False,
                          classes=SHAPENET_PART):
    """`validate_seg` with each batch's forward one HIP-graph replay (upp_hip.infer.SegEvalStep, one per (B, N); a smaller batch is
    padded into the step in use) and the metric on the device.  Same arguments and results."""
    metric = SegMetric(num_part, num_classes, classes)
    preds = []

    def run(step, batch):
        points, label, target = _seg_batch(*batch)
        pred = step.run(points, label.to(step.device), target.to(step.device), metric)
        if return_predictions:
            preds.append(pred.clone())
    _run_steps(model, batches, lambda n, N: infer.SegEvalStep.cached(model, (n, N, 3), num_classes),
               lambda s, n, N: s.B >= n and s.N == N, run)
    out = metric.compute(distributed)
    return (out, torch.cat(preds) if preds else torch.empty((0, 0), dtype=torch.long)) if return_predictions else out


# ------------------------------------------------------------------ point completion (reference tools/runner_pretask.py:314-426)
# The viewpoints of the reference's `validate` (not normalised), in its order; in_detail=False uses the first one only.
VIEWPOINTS = ((1., 1., 1.), (1., 1., -1.), (1., -1., 1.), (-1., 1., 1.), (-1., -1., 1.), (-1., 1., -1.), (1., -1., -1.), (-1., -1., -1.))
CROP_RATIO = {'easy': 1 / 4, 'median': 1 / 2, 'hard': 3 / 4}        # (the reference spells the middle mode 'median')
CENTERS = 128                                                       # misc.fps(partial, 128): the visible half of the coarse output


def crop_count(num_points, mode):
    """The points removed from a cloud of num_points in `mode`: int(N * ratio), as the reference computes num_crop."""
    if mode not in CROP_RATIO:
        raise ValueError("mode must be one of %s, got %r" % (sorted(CROP_RATIO), mode))
    return int(num_points * CROP_RATIO[mode])


def viewpoints(in_detail):
    return VIEWPOINTS if in_detail else VIEWPOINTS[:1]


class _CompletionHostSums:
    """CompletionMetric's sums on the CPU: the fields of upp_hip.ops.CompletionAccumulator."""

    def __init__(self, C):
        self.loss_sum = torch.zeros(4, dtype=torch.float64)
        self.counters = torch.zeros(2, dtype=torch.int64)
        self.cat_sum = torch.zeros((C, 3), dtype=torch.float64)
        self.cat_cnt = torch.zeros(C, dtype=torch.int64)


def _nn64(a, b, chunk=512):
    """a (n, 3), b (m, 3) float64 -> (squared distance to the nearest point of b, its index: the first among equal minima)."""
    d_out, i_out = [], []
    for s in range(0, a.shape[0], chunk):
        q = a[s:s + chunk]
        dx, dy, dz = (q[:, None, k] - b[None, :, k] for k in range(3))
        d, i = ((dx * dx + dy * dy) + dz * dz).min(1)
        d_out.append(d)
        i_out.append(i)
    return torch.cat(d_out), torch.cat(i_out)


def _zero_sum(p):
    """(n, 3) f32 -> (n,) bool: the f32 coordinate sum (x + y) + z is exactly 0 (the reference's torch.sum(xyz, dim=2).ne(0))."""
    p = p.float()
    return (p[:, 0] + p[:, 1]) + p[:, 2] == 0


def _completion_row_host(x1, x2, detail, th):
    """One cloud pair on the CPU, in float64: the 8 values of a upp_completion_cloud_metrics row (with the masked CDs)."""
    a, b = x1.double(), x2.double()
    d1, _ = _nn64(a, b)
    d2, _ = _nn64(b, a)
    md1, md2 = float(d1.mean()), float(d2.mean())
    mq1, mq2 = float(d1.sqrt().mean()), float(d2.sqrt().mean())
    f, cdl1, cdl2 = 0.0, (mq1 + mq2) / 2.0, md1 + md2
    if detail:
        precision = float(int((d1.sqrt() < th).sum())) / float(a.shape[0])
        recall = float(int((d2.sqrt() < th).sum())) / float(b.shape[0])
        f = 2 * recall * precision / (recall + precision) if recall + precision else 0.
        z1, z2 = _zero_sum(x1), _zero_sum(x2)
        if bool(z1.any()) or bool(z2.any()):
            a, b = a[~z1], b[~z2]
            if a.shape[0] == 0 or b.shape[0] == 0:
                cdl1 = cdl2 = float('nan')
            else:
                e1, _ = _nn64(a, b)
                e2, _ = _nn64(b, a)
                cdl1 = (float(e1.sqrt().mean()) + float(e2.sqrt().mean())) / 2.0
                cdl2 = float(e1.mean()) + float(e2.mean())
    return md1, md2, mq1, mq2, f, cdl1, cdl2


def _completion_update_host(coarse, dense, gt, sums, category, n_valid, th):
    """upp_completion_cloud_metrics + upp_completion_accumulate in float64 on the CPU, in the same order (cloud, then viewpoint)."""
    B = gt.shape[0]
    V = coarse.shape[0] // B
    loss = sums.loss_sum.tolist()
    counters = sums.counters.tolist()
    cs, cc = sums.cat_sum.tolist(), sums.cat_cnt.tolist()
    C = len(cc)
    cats = None if category is None else category.tolist()
    for b in range(n_valid):
        for v in range(V):
            r = v * B + b
            sp = _completion_row_host(coarse[r], gt[b], False, th)
            de = _completion_row_host(dense[r], gt[b], cats is not None, th)
            for k, (row, l1) in enumerate(((sp, True), (sp, False), (de, True), (de, False))):
                loss[k] += ((row[2] + row[3]) / 2.0 if l1 else row[0] + row[1]) * 1000.0
            counters[0] += 1
            if cats is None:
                continue
            c = cats[b]
            if not 0 <= c < C:
                counters[1] += 1
                continue
            cs[c] = [cs[c][0] + de[4], cs[c][1] + de[5] * 1000.0, cs[c][2] + de[6] * 1000.0]
            cc[c] += 1
    sums.loss_sum.copy_(torch.tensor(loss, dtype=torch.float64))
    sums.counters.copy_(torch.tensor(counters, dtype=torch.int64))
    sums.cat_sum.copy_(torch.tensor(cs, dtype=torch.float64).view(C, 3))
    sums.cat_cnt.copy_(torch.tensor(cc, dtype=torch.int64))


class CompletionMetric:
    """The point-completion metrics of the reference's pre-task `validate` (tools/runner_pretask.py:314-426; utils/metrics.py:48-111),
    accumulated batch by batch.

    update(coarse (V B, nc, 3), dense (V B, nd, 3), gt (B, N, 3), category=None, n_valid=None): viewpoint-expanded batches, row v B + b
    being cloud b seen from viewpoint v; clouds [0, n_valid) count.  For every (cloud, viewpoint) pair: the losses ChamferDistanceL1 /
    L2 (ignore_zeros=False) of (coarse, gt) and (dense, gt), x 1000; with a category (B,) int also the detail metrics of (dense, gt)
    under that category: F-Score@threshold, CDL1 and CDL2 (x 1000, ignore_zeros: every point whose f32 coordinate sum (x + y) + z is 0
    is removed from both clouds first; a cloud left empty gives NaN).  category=None: losses only (the reference's in_detail=False).
    HIP tensors run the metric kernels (upp_hip.ops.completion_update: no per-point value leaves the device); CPU tensors the same rules
    in float64 torch.

    compute(distributed=False) -> {'sparse_cd_l1', 'sparse_cd_l2', 'dense_cd_l1', 'dense_cd_l2' (means over the pairs; dense_cd_l2 is
    the reference's CD_Metric), 'f_score', 'cd_l1', 'cd_l2' (the unweighted mean over the seen categories of their per-category means:
    test_metrics.update(v.avg())), 'category_metrics': {name or id: {'f_score', 'cd_l1', 'cd_l2', 'count'}} of the seen categories}.
    distributed: the sums and counts are all-reduced before any division.

    Deliberate deviations from the reference:
      * the sums are float64, added in the reference's order (batch by batch, cloud-major, then viewpoint); the reference sums f32 CDs
        and Python floats (about 1e-7 relative apart);
      * the F-Score distance: the reference's comes from open3d (a float64 KD-tree over the f32 coordinates).  Here a point's partner
        is its Chamfer nearest neighbour as upp_chamfer_fwd picks it (the lowest index among equal f32 minima), the distance to it is
        recomputed in float64 from the f32 coordinates, and the point counts when sqrt(d64) < threshold.  This differs from a float64
        nearest-neighbour search only where two candidates tie within f32 rounding and lie on opposite sides of the threshold.  (The
        CPU path searches in float64 directly.)"""

    def __init__(self, num_categories=1, threshold=0.01, names=None):
        self.num_categories, self.threshold = int(num_categories), float(threshold)
        if self.num_categories < 1:
            raise ValueError("num_categories must be positive")
        if not (self.threshold > 0.0 and self.threshold != float('inf')):
            raise ValueError("threshold must be positive and finite, got %r" % (threshold,))
        self.names = None if names is None else list(names)
        if self.names is not None and len(self.names) != self.num_categories:
            raise ValueError("%d names for %d categories" % (len(self.names), self.num_categories))
        self.sums = None

    def _check(self, coarse, dense, gt, category, n_valid):
        for name, t in (('coarse', coarse), ('dense', dense), ('gt', gt)):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 3 or t.shape[1] < 1:
                raise ValueError("%s must be a (rows, points, 3) tensor, got %s" % (name, getattr(t, 'shape', type(t))))
        B, R = gt.shape[0], coarse.shape[0]
        if B < 1 or R < B or R % B or dense.shape[0] != R:
            raise ValueError("coarse %s and dense %s must hold V x %d clouds for gt %s" % (tuple(coarse.shape), tuple(dense.shape), B,
                                                                                     tuple(gt.shape)))
        if not (coarse.device == dense.device == gt.device):
            raise ValueError("coarse, dense and gt must be on one device")
        n_valid = B if n_valid is None else int(n_valid)
        if not 0 <= n_valid <= B:
            raise ValueError("n_valid %d outside [0, %d]" % (n_valid, B))
        if category is not None:
            category = torch.as_tensor(category).reshape(-1)
            if category.shape[0] != B or category.dtype.is_floating_point or category.dtype == torch.bool:
                raise ValueError("category must be (%d,) integers, got %s %s" % (B, category.dtype, tuple(category.shape)))
            category = category.to(gt.device, torch.long).contiguous()
        return category, n_valid

    def device_sums(self, device):
        """The upp_hip.ops.CompletionAccumulator the updates of a HIP device add into (made on first use)."""
        from upp_hip import ops
        if self.sums is None:
            self.sums = ops.CompletionAccumulator(self.num_categories, device)
        elif not isinstance(self.sums, ops.CompletionAccumulator) or self.sums.device != torch.device(device):
            raise RuntimeError("CompletionMetric: all updates must come from one device")
        return self.sums

    def update(self, coarse, dense, gt, category=None, n_valid=None):
        category, n_valid = self._check(coarse, dense, gt, category, n_valid)
        coarse, dense, gt = (t.detach().contiguous() for t in (coarse, dense, gt))
        if gt.is_cuda:
            from upp_hip import ops
            ops.completion_update(coarse, dense, gt, self.device_sums(gt.device), category, n_valid, self.threshold)
            return self
        if self.sums is None:
            self.sums = _CompletionHostSums(self.num_categories)
        elif not isinstance(self.sums, _CompletionHostSums):
            raise RuntimeError("CompletionMetric: all updates must come from one device")
        _completion_update_host(coarse.float(), dense.float(), gt.float(), self.sums, category, n_valid, self.threshold)
        return self

    def compute(self, distributed=False):
        import numpy as np
        s = self.sums if self.sums is not None else _CompletionHostSums(self.num_categories)
        ints = torch.cat([s.counters, s.cat_cnt])
        reals = torch.cat([s.loss_sum, s.cat_sum.reshape(-1)])
        if distributed:
            torch.distributed.all_reduce(ints)
            torch.distributed.all_reduce(reals)
        ints, reals = ints.cpu().numpy(), reals.cpu().numpy()
        (pairs, invalid), cat_cnt = ints[:2], ints[2:]
        loss_sum, cat_sum = reals[:4], reals[4:].reshape(-1, 3)
        if invalid:
            raise ValueError("%d (cloud, viewpoint) pair(s) have a category outside [0, %d)" % (invalid, self.num_categories))
        seen = np.flatnonzero(cat_cnt)
        with np.errstate(divide='ignore', invalid='ignore'):
            losses = loss_sum / np.float64(pairs)
            means = cat_sum[seen] / cat_cnt[seen, None].astype(np.float64)
        overall = means.sum(0) / np.float64(len(seen)) if len(seen) else np.full(3, np.nan)
        out = {k: float(v) for k, v in zip(('sparse_cd_l1', 'sparse_cd_l2', 'dense_cd_l1', 'dense_cd_l2'), losses)}
        out.update(f_score=float(overall[0]), cd_l1=float(overall[1]), cd_l2=float(overall[2]))
        out['category_metrics'] = {(self.names[c] if self.names is not None else int(c)):
                                   {'f_score': float(m[0]), 'cd_l1': float(m[1]), 'cd_l2': float(m[2]), 'count': int(cat_cnt[c])}
                                   for c, m in zip(seen, means)}
        return out


def completion_outputs(model, gt, centers, num_crop, npoints=1024, max_clouds=None):
    """The completion of every (cloud, viewpoint) pair of one batch as ONE viewpoint-major V B batch (row v B + b): gt (B, N, 3),
    centers (V, 3) -> (coarse (V B, 128 + n_pred, 3), dense (V B, npoints + n_rebuild, 3)).  The reference's steps 1-5 per pair
    (tools/runner_pretask.py:366-373): crop num_crop points nearest the viewpoint and FPS the kept part to npoints, FPS it again
    (npoints of npoints: a re-ordering from index 0 that the model's grouping sees), FPS 128 centres, the eval forward, the two
    concatenations.  The forwards take at most max_clouds clouds each (whole viewpoints, infer.plan_chunks)."""
    B, N = gt.shape[0], gt.shape[1]
    V = centers.shape[0]
    rep = gt if V == 1 else gt.repeat(V, 1, 1)
    ctr = centers.view(V, 1, 1, 3).expand(V, B, 1, 3).reshape(V * B, 1, 3)
    partial, _ = misc.seprate_point_cloud(rep, N, num_crop, sample_points=npoints, centers=ctr, keep_crop=False)
    partial = misc.fps(partial, npoints)[0]
    partial_center = misc.fps(partial, CENTERS)[0]
    preds, rebuilds = [], []
    for v0, v1 in infer.plan_chunks(V, B, max_clouds):
        pred_center, rebuild = model(partial[v0 * B:v1 * B], train_with_gaussian=False, predict_center_num=16)
        preds.append(pred_center)
        rebuilds.append(rebuild)
    pred_center = preds[0] if len(preds) == 1 else torch.cat(preds)
    rebuild = rebuilds[0] if len(rebuilds) == 1 else torch.cat(rebuilds)
    return torch.cat([partial_center, pred_center], dim=1), torch.cat([partial, rebuild], dim=1)


def _num_crop(N, mode, npoints):
    """crop_count(N, mode), refusing a mode that leaves fewer points than the model takes."""
    num_crop = crop_count(N, mode)
    if N - num_crop < npoints:
        raise ValueError("%s mode keeps %d of %d points, fewer than the %d the model takes" % (mode, N - num_crop, N, npoints))
    return num_crop


@torch.no_grad()
def validate_completion(model, batches, mode='easy', in_detail=False, npoints=1024, distributed=False, threshold=0.01, num_categories=None,
                        names=None, max_clouds=None):
    """batches: iterable of (gt (B, N, 3), category (B,) int).  The reference's pre-task `validate` (tools/runner_pretask.py:314-426)
    with every viewpoint of a batch cropped and completed as one viewpoint-major batch (completion_outputs) and the metrics on the device
    (CompletionMetric; in_detail adds the per-category F-Score / CDL1 / CDL2 over the eight viewpoints).  num_categories: default the
    largest category seen + 1 -- which needs the categories on the host -- or len(names).  The model's training flag is restored.
    -> CompletionMetric.compute(distributed)."""
    batches = list(batches)
    metric = CompletionMetric(_num_categories(batches, num_categories, names, in_detail), threshold, names)
    with _evaluating(model):
        for gt, category in batches:
            gt = gt.contiguous()
            centers = torch.tensor(viewpoints(in_detail), dtype=torch.float32, device=gt.device)
            coarse, dense = completion_outputs(model, gt, centers, _num_crop(gt.shape[1], mode, npoints), npoints, max_clouds)
            metric.update(coarse, dense, gt, category if in_detail else None)
    return metric.compute(distributed)


def _num_categories(batches, num_categories, names, in_detail):
    if num_categories is not None:
        return int(num_categories)
    if names is not None:
        return len(names)
    if not in_detail or not batches:
        return 1
    return max(int(torch.as_tensor(c).max()) for _, c in batches) + 1


@torch.no_grad()
def validate_completion_captured(model, batches, mode='easy', in_detail=False, npoints=1024, distributed=False, threshold=0.01,
                                 num_categories=None, names=None, max_clouds=None):
    """`validate_completion` with each batch one HIP-graph replay (upp_hip.infer.CompletionEvalStep, one per (B, N, V)) and the
    accumulation launch after it.  Same arguments and results, bit for bit: a ragged last batch runs a graph of its own size rather than
    a padded one, because the forward's GEMM tiling follows the row count (a padded forward equals it only to f32 rounding)."""
    batches = list(batches)
    metric = CompletionMetric(_num_categories(batches, num_categories, names, in_detail), threshold, names)
    kw = dict(mode=mode, in_detail=bool(in_detail), npoints=int(npoints), threshold=float(threshold), max_clouds=max_clouds)
    _run_steps(model, batches, lambda n, N: infer.CompletionEvalStep.cached(model, (n, N, 3), **kw),
               lambda s, n, N: s.B == n and s.N == N,            # (never padded: see above)
               lambda s, b: s.run(b[0].contiguous(), b[1] if in_detail else None, metric))
    return metric.compute(distributed)
