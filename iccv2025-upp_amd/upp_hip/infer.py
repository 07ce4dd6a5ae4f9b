"""Captured, vote-batched evaluation of the classification models (the `validate` / `test_vote` loops of the reference runner,
tools/runner_module.py:383-413, 427-490; eager form: utils/evaluate.py).

EvalStep captures one evaluation of a fixed (B, N_raw, 3) raw batch into one HIP graph:

  1. FPS to the superset (upp_fps; to `npoints` in the validate form),
  2. upp_vote_points: the V random subsets, scale/translate-augmented, as ONE vote-major (V*B, npoints, 3) batch,
  3. the eval-mode forward over the V*B clouds, in vote chunks of at most `max_clouds` clouds (default: all votes in one forward, or
     one vote per forward for a model whose forward reads across samples -- mixes_samples(): the classification recipe),

and after the replay upp_vote_reduce turns the logits into predictions and accumulates the (correct, total) counters.  The
reduction is a launch of its own, outside the graph, because its row count n_valid changes with the ragged last batch.

The random draws stay on the host side of the graph, in the reference's order: per vote a randperm from `generator`, then the scale
and the shift from the default generator (evaluate.test_vote calls its transform without one), into static buffers.

SegEvalStep does the same for the eval forward of a part-segmentation model (the reference's tools/runner_unify_seg.py:301-367): one
graph per (B, N), the metric kernels (ops.seg_iou_update) after each replay.

CompletionEvalStep does it for the pre-task `validate` of a completion model (the reference's tools/runner_pretask.py:314-426): one
graph per (B, N, V) holds the crop, the FPS launches, the forward, both Chamfer searches and the per-cloud metric kernels; the
accumulation (ops.completion_accumulate) follows each replay.

The three share _CapturedStep: the capture, the replay and the tracking of the model's weights between evaluations."""
import weakref

import torch

from . import functional as HF
from . import ops

SUPERSET = {1024: 1200, 4096: 4800, 8192: 8192}        # evaluate.test_vote (reference tools/runner_module.py:440)
SCALE = (2. / 3., 3. / 2.)                              # misc.scale_translate's defaults
TRANSLATE = 0.2


def plan_chunks(votes, batch, max_clouds=None):
    """Vote ranges [(v0, v1), ...] of the forwards of one evaluation: as many votes per forward as fit in `max_clouds` clouds (at
    least one vote), all of them in one forward when max_clouds is None."""
    votes, batch = int(votes), int(batch)
    if votes < 1 or batch < 1:
        raise ValueError("votes and batch must be positive")
    per = votes if max_clouds is None else max(1, min(votes, int(max_clouds) // batch))
    return [(v, min(v + per, votes)) for v in range(0, votes, per)]


def mixes_samples(model):
    """Does the model's eval forward read across the samples of its batch?  Point_MAE_unify with prompt propagation and
    gather_idx = false indexes its level-2 propagation as the reference does: flat indices of a (B*G)-row matrix mapped onto
    (B*Lp) token rows with G = Lp - 1, so that sample b reads rows of samples <= b.  A row then depends on the rows BEFORE it (padding
    at the end changes nothing), but a forward over several votes is not the votes' forwards: such a model runs one vote per forward."""
    cfg = getattr(model, 'config', None)
    return bool(getattr(cfg, 'prompt_propagation_after', False)) and not bool(getattr(cfg, 'gather_idx', True))


def pad_batch(points, batch, out=None):
    """(n, ...) -> (batch, ...): the n rows, then the last one repeated (every eval-mode operator works per sample, so the padding
    cannot change the real rows).  out: the static buffer to fill in place."""
    n = points.shape[0]
    if not 0 < n <= batch:
        raise ValueError("a batch of %d rows does not fit a step of %d" % (n, batch))
    if out is None:
        out = points.new_empty((batch,) + tuple(points.shape[1:]))
    out[:n].copy_(points)
    if n < batch:
        out[n:].copy_(points[n - 1:n].expand((batch - n,) + tuple(points.shape[1:])))
    return out


class _eval_mode:
    """The model in eval mode inside, its own mode again after (a top-level model already in eval mode is left alone)."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.was = self.model.training
        if self.was:
            self.model.eval()

    def __exit__(self, *exc):
        if self.was:
            self.model.train()
        return False


_STEPS = weakref.WeakKeyDictionary()         # model -> {(class, batch shape, arguments): step}


class _CapturedStep:
    """One evaluation of a fixed (B, N, 3) batch as one HIP graph.  A concrete step owns its static buffers, `_body()` (the launches
    of the captured region after the first) and `run()` (fill the static inputs, `_replay()`, the launch whose row count follows the
    batch).  use_graph=False runs the same launches eagerly.

    Weights change between evaluations (training, load_state_dict, FlatAdamW re-pointing parameters into its flat buffer).  prepare()
    compares every parameter's and buffer's address, version and requires_grad with the capture-time snapshot: a moved version refreshes
    the derived weight caches in place (functional.refresh_caches: same buffers, the graph stays valid), a moved address or a changed
    requires_grad recaptures.  The bf16 plane images of the model's trainable weights are re-split by the graph's first launch."""

    def __init__(self, model, batch_shape, use_graph, per_sample=False):
        """per_sample: the step pads a ragged batch into its forward, so a model whose forward reads across samples is refused."""
        self._model = weakref.ref(model)            # (the step is cached per model: it must not keep the model alive)
        self.device = next(model.parameters()).device
        name = type(self).__name__
        if self.device.type != 'cuda':
            raise RuntimeError("%s runs the HIP kernels: the model must live on a HIP device" % name)
        if per_sample and mixes_samples(model):
            raise ValueError("%s pads a ragged batch, which needs a forward that works per sample; this model's reads across the "
                             "samples of its batch (gather_idx = false)" % name)
        B, N, c = (int(x) for x in batch_shape)
        if c != 3:
            raise ValueError("batch_shape must be (B, N, 3)")
        self.B, self.N = B, N
        self.use_graph = bool(use_graph)
        self._graph = None
        self._snap = None
        self._owners = self._trainable()
        HF.refresh_caches(model)

    @property
    def model(self):
        return self._model()

    def _trainable(self):
        return {id(p) for p in self.model.parameters() if p.requires_grad}

    def _evaluate(self):
        """The captured region."""
        with torch.no_grad(), HF.managed_weights(transposes=False, owners=self._owners):   # (the graph's first launch: the model's
            self._body()                                                                   #  trainable weights, split)

    def _params(self):
        return list(self.model.parameters()) + list(self.model.buffers())

    def _snapshot(self):
        return [(t.data_ptr(), t._version, t.requires_grad) for t in self._params()]

    def _capture(self):
        self._graph = None
        HF.refresh_caches(self.model)
        self._owners = self._trainable()
        cur = torch.cuda.current_stream(self.device)
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(cur)
        with torch.cuda.stream(s):               # warm-up on a side stream, as graph capture requires (plane images, lazy caches)
            for _ in range(2):
                self._evaluate()
        cur.wait_stream(s)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._evaluate()
        torch.cuda.synchronize(self.device)
        self._graph = g
        self._snap = self._snapshot()

    def prepare(self):
        """Before an evaluation: bring the captured graph up to date with the model's weights (see the class docstring)."""
        if not self.use_graph:
            self._owners = self._trainable()
            return
        now = self._snapshot() if self._graph is not None else None
        if now is None or len(now) != len(self._snap) or any(a[0] != b[0] or a[2] != b[2] for a, b in zip(now, self._snap)):
            with _eval_mode(self.model):
                self._capture()
        elif any(a[1] != b[1] for a, b in zip(now, self._snap)):
            HF.refresh_caches(self.model)        # contents changed, addresses kept: the images are re-split in place
            self._snap = now

    def _replay(self):
        with _eval_mode(self.model):
            if self.use_graph:
                if self._graph is None:
                    self._capture()
                self._graph.replay()
            else:
                self._evaluate()

    @classmethod
    def cached(cls, model, batch_shape, **kw):
        """One step per model, class, batch shape and arguments: the same arguments give the same step object."""
        steps = _STEPS.setdefault(model, {})
        key = (cls, tuple(int(x) for x in batch_shape)) + tuple(sorted(kw.items()))
        step = steps.get(key)
        if step is None:
            step = steps[key] = cls(model, batch_shape, **kw)
        return step


class EvalStep(_CapturedStep):
    """run(points, labels) -> pred (n,) int64 (a view of the static `pred`); the counters (2,) int64 accumulate (correct, total).

    votes == 1 and superset None: the validate form (FPS to npoints, no draws).  Otherwise the test_vote form: FPS to `superset`
    (default SUPERSET[npoints], at most N_raw), per vote a random npoints-subset, scale/translate when `transform`.
    Static outputs: `logits` (votes*B, C) vote-major, `pred` (B,)."""

    def __init__(self, model, batch_shape, npoints, votes=1, noisy=False, transform=True, use_graph=True, superset=None,
                 max_clouds=None):
        super().__init__(model, batch_shape, use_graph)
        B, n_raw = self.B, self.N
        self.n_raw, self.npoints, self.votes = n_raw, int(npoints), int(votes)
        self.noisy = bool(noisy)
        self.subsets = not (self.votes == 1 and superset is None)
        if self.subsets:
            if superset is None:
                if self.npoints not in SUPERSET:
                    raise NotImplementedError()
                superset = SUPERSET[self.npoints]
            self.S = min(int(superset), n_raw)
        else:
            self.S = self.npoints
        if self.npoints > self.S:
            raise ValueError("npoints %d exceeds the superset of %d points" % (self.npoints, self.S))
        self.transform = bool(transform) and self.subsets
        if max_clouds is None and mixes_samples(model):
            max_clouds = B                         # one vote per forward: the reference's per-vote batches (see mixes_samples)
        self.chunks = plan_chunks(self.votes, B, max_clouds)
        dev = self.device
        self.raw = torch.zeros((B, n_raw, 3), device=dev)
        self.labels = torch.zeros(B, dtype=torch.long, device=dev)
        self.pick = torch.arange(self.npoints, dtype=torch.int32, device=dev).repeat(self.votes, 1).contiguous()
        self.scale = torch.ones((self.votes, B, 3), device=dev) if self.transform else None
        self.shift = torch.zeros((self.votes, B, 3), device=dev) if self.transform else None
        self.pts = torch.empty((self.votes * B, self.npoints, 3), device=dev)
        self.logits = None
        self.pred = torch.zeros(B, dtype=torch.long, device=dev)
        self.counters = torch.zeros(2, dtype=torch.long, device=dev)

    def _body(self):
        sup, _ = HF.fps_gather(self.raw, self.S)
        ops.vote_points(sup, self.pick, self.scale, self.shift, out=self.pts)
        B, outs = self.B, []
        for v0, v1 in self.chunks:
            outs.append(self.model(self.pts[v0 * B:v1 * B], completion_prompt=self.noisy, denoise=self.noisy,
                                   point_num=self.npoints))
        if self.logits is None:
            self.logits = torch.empty((self.votes * B, outs[0].shape[-1]), device=self.device)
        ops.copy_batched([self.logits[v0 * B:v1 * B] for v0, v1 in self.chunks], [o.contiguous() for o in outs])

    def draw(self, n, generator=None):
        """The host-side draws of one batch of n real clouds, in evaluate.test_vote's order: per vote randperm(S) from `generator`,
        then scale and shift of the n clouds from the default generator."""
        if not self.subsets:
            return
        for v in range(self.votes):
            perm = torch.randperm(self.S, device=self.device, generator=generator)
            self.pick[v].copy_(perm[:self.npoints])
            if self.transform:
                self.scale[v, :n].uniform_(*SCALE)
                self.shift[v, :n].uniform_(-TRANSLATE, TRANSLATE)

    def run(self, points, labels=None, generator=None):
        n = points.shape[0]
        if tuple(points.shape[1:]) != (self.n_raw, 3):
            raise ValueError("points %s do not fit a step of (%d, %d, 3)" % (tuple(points.shape), self.B, self.n_raw))
        pad_batch(points, self.B, out=self.raw)
        if labels is not None:
            pad_batch(labels.reshape(-1), self.B, out=self.labels)
        self.draw(n, generator)
        self._replay()
        ops.vote_reduce(self.logits, self.labels, self.votes, n, self.pred, self.counters)
        return self.pred[:n]

    @classmethod
    def cached(cls, model, batch_shape, npoints, **kw):
        """One step per model and (B, N_raw, npoints, votes, noisy, ...)."""
        return super().cached(model, batch_shape, npoints=int(npoints), **kw)


class SegEvalStep(_CapturedStep):
    """The eval-mode forward of a part-segmentation model (Point_MAE_unify_seg) for a fixed (B, N, 3) batch as one HIP graph, plus the
    metric launches (ops.seg_iou_update) after each replay with the batch's real row count.  The reference's protocol
    (tools/runner_unify_seg.py:301-367): model(points, one-hot label, completion_prompt=False, denoise=False, point_num=N), the label
    points being the points.  Static inputs: `pts` (B, N, 3) and `onehot` (B, num_classes), filled outside the graph; `target` (B, N)
    int64 and `pred` (B, N) int64 serve the metric.  A ragged last batch is padded (pad_batch), which needs a forward that works per
    sample: a model whose forward reads across samples (mixes_samples) is refused."""

    def __init__(self, model, batch_shape, num_classes=16, use_graph=True):
        super().__init__(model, batch_shape, use_graph, per_sample=True)
        B, N, dev = self.B, self.N, self.device
        self.num_classes = int(num_classes)
        self.pts = torch.zeros((B, N, 3), device=dev)
        self.labels = torch.zeros(B, dtype=torch.long, device=dev)
        self.onehot = torch.zeros((B, self.num_classes), device=dev)
        self._classes = torch.arange(self.num_classes, device=dev)
        self.target = torch.zeros((B, N), dtype=torch.long, device=dev)
        self.pred = torch.zeros((B, N), dtype=torch.long, device=dev)
        self.logp = None

    def _body(self):
        self.logp = self.model(self.pts, self.onehot, completion_prompt=False, denoise=False, point_num=self.N)

    def run(self, points, label, target, metric):
        """One batch of n <= B shapes: points (n, N, 3), label (n,) or (n, 1), target (n, N) -> pred (n, N) int64 (a view of the
        static `pred`), the metric (utils.evaluate.SegMetric) updated with the n real shapes."""
        n = points.shape[0]
        if tuple(points.shape[1:]) != (self.N, 3):
            raise ValueError("points %s do not fit a step of (%d, %d, 3)" % (tuple(points.shape), self.B, self.N))
        if tuple(target.shape) != (n, self.N):
            raise ValueError("target %s does not fit points %s" % (tuple(target.shape), tuple(points.shape)))
        pad_batch(points, self.B, out=self.pts)
        pad_batch(label.reshape(-1), self.B, out=self.labels)
        pad_batch(target, self.B, out=self.target)
        self.onehot.copy_(self.labels.view(-1, 1) == self._classes)
        self._replay()
        metric.update(self.logp, self.target, n_valid=n, pred=self.pred)
        return self.pred[:n]

    @classmethod
    def cached(cls, model, batch_shape, num_classes=16, **kw):
        """One step per model and (B, N, num_classes, use_graph)."""
        return super().cached(model, batch_shape, num_classes=int(num_classes), **kw)


class CompletionEvalStep(_CapturedStep):
    """The pre-task evaluation of a fixed (B, N, 3) batch of complete clouds from V viewpoints as one HIP graph
    (utils.evaluate.completion_outputs: the crop distances, upp_argsort_rows, the gathers, the three FPS launches, the eval forward, the
    concatenations; then ops.completion_cloud_metrics: two upp_chamfer_fwd and the per-cloud metric kernels into the step's own rows).
    After each replay ops.completion_accumulate adds the rows of the batch's real clouds into the metric's sums: its row count n_valid
    changes with a smaller batch, which run() pads (pad_batch) -- so a model whose forward reads across samples (mixes_samples) is
    refused.  (validate_completion_captured gives a ragged last batch a step of its own size instead, to stay bit-identical to the eager
    protocol.)  Static input: `gt` (B, N, 3) and `category` (B,) int64, filled outside the graph.  cached(model, batch_shape, **kw):
    one step per model and (B, N, mode, in_detail, npoints, threshold, ...)."""

    def __init__(self, model, batch_shape, mode='easy', in_detail=False, npoints=1024, threshold=0.01, max_clouds=None, use_graph=True):
        from utils import evaluate
        super().__init__(model, batch_shape, use_graph, per_sample=True)
        B, N, dev = self.B, self.N, self.device
        self.npoints = int(npoints)
        self.num_crop = evaluate._num_crop(N, mode, self.npoints)
        self.detail, self.threshold, self.max_clouds = bool(in_detail), float(threshold), max_clouds
        self.centers = torch.tensor(evaluate.viewpoints(self.detail), dtype=torch.float32, device=dev)
        self.V = self.centers.shape[0]
        self.gt = torch.zeros((B, N, 3), device=dev)
        self.category = torch.zeros(B, dtype=torch.long, device=dev)
        self.rows = ops.CompletionAccumulator(1, dev).reserve(self.V * B)
        self.coarse = self.dense = None

    def _body(self):
        from utils import evaluate
        self.coarse, self.dense = evaluate.completion_outputs(self.model, self.gt, self.centers, self.num_crop, self.npoints,
                                                              self.max_clouds)
        ops.completion_cloud_metrics(self.coarse, self.dense, self.gt, self.rows, self.detail, self.threshold)

    def run(self, gt, category, metric):
        """One batch of n <= B complete clouds gt (n, N, 3) and their categories (n,) (None: losses only; ignored unless in_detail) ->
        the metric (utils.evaluate.CompletionMetric) updated with the n real clouds."""
        n = gt.shape[0]
        if tuple(gt.shape[1:]) != (self.N, 3):
            raise ValueError("gt %s does not fit a step of (%d, %d, 3)" % (tuple(gt.shape), self.B, self.N))
        if metric.threshold != self.threshold:
            raise ValueError("the metric's threshold %r is not the step's %r" % (metric.threshold, self.threshold))
        cat = None
        if self.detail and category is not None:
            category = torch.as_tensor(category).reshape(-1)
            if category.shape[0] != n or category.dtype.is_floating_point:
                raise ValueError("category must be (%d,) integers" % n)
            cat = pad_batch(category.to(self.device, torch.long), self.B, out=self.category)
        pad_batch(gt, self.B, out=self.gt)
        self._replay()
        ops.completion_accumulate(metric.device_sums(self.device), self.V, self.B, cat, n, rows=self.rows)
        return metric
