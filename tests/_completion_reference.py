"""An independent numpy restatement of the reference's pre-task `validate` (tools/runner_pretask.py:314-426) and of the Metrics it
reports (utils/metrics.py:48-111): per (cloud, viewpoint) pair, in the reference's order, the four Chamfer losses x 1000 and, in detail
mode, F-Score@th, CDL1 x 1000 and CDL2 x 1000 (ignore_zeros), averaged per taxonomy and then over the taxonomies.  Nearest neighbours by
chunked float64 brute force (the reference's open3d KD-tree and Chamfer kernels, restated); means as AverageMeter takes them."""
import math

import numpy as np

VIEWPOINTS = [[1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1], [-1, -1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, -1]]
CROP_RATIO = {'easy': 1 / 4, 'median': 1 / 2, 'hard': 3 / 4}


def nearest(a, b, chunk=256):
    """a (n, 3), b (m, 3) -> (squared float64 distance of each a point to its nearest b point, that point's index)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d_out, i_out = np.empty(len(a)), np.empty(len(a), np.int64)
    for s in range(0, len(a), chunk):
        q = a[s:s + chunk]
        dx, dy, dz = (q[:, None, k] - b[None, :, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        i = d.argmin(1)
        d_out[s:s + len(q)], i_out[s:s + len(q)] = d[np.arange(len(q)), i], i
    return d_out, i_out


def nonzero_rows(x):
    """torch.sum(xyz, dim=2).ne(0) of a batch of one, in f32: (x + y) + z != 0."""
    x = np.asarray(x, np.float32)
    return (x[:, 0] + x[:, 1]) + x[:, 2] != np.float32(0)


def chamfer(x1, x2, ignore_zeros=False):
    """(dist1, dist2) of ChamferDistanceL1 / L2 at batch size 1, float64."""
    if ignore_zeros:
        x1, x2 = np.asarray(x1)[nonzero_rows(x1)], np.asarray(x2)[nonzero_rows(x2)]
    if len(x1) == 0 or len(x2) == 0:
        return np.empty(0), np.empty(0)
    return nearest(x1, x2)[0], nearest(x2, x1)[0]


def _mean(x):
    return float(np.mean(x)) if len(x) else math.nan


def cd_l1(x1, x2, ignore_zeros=False):
    d1, d2 = chamfer(x1, x2, ignore_zeros)
    return (_mean(np.sqrt(d1)) + _mean(np.sqrt(d2))) / 2


def cd_l2(x1, x2, ignore_zeros=False):
    d1, d2 = chamfer(x1, x2, ignore_zeros)
    return _mean(d1) + _mean(d2)


def f_score(pred, gt, th=0.01):
    """Metrics._get_f_score at batch size 1: open3d's compute_point_cloud_distance is the float64 nearest-neighbour distance."""
    dist1 = np.sqrt(nearest(pred, gt)[0])
    dist2 = np.sqrt(nearest(gt, pred)[0])
    recall = float(sum(d < th for d in dist2)) / float(len(dist2))
    precision = float(sum(d < th for d in dist1)) / float(len(dist1))
    return 2 * recall * precision / (recall + precision) if recall + precision else 0.


class AverageMeter:
    def __init__(self, n):
        self.sum, self.count = [0.0] * n, 0

    def update(self, values):
        self.sum = [s + v for s, v in zip(self.sum, values)]
        self.count += 1

    def avg(self):
        return [s / self.count for s in self.sum]


def reference_metrics(records, in_detail, th=0.01):
    """records: (coarse (nc, 3), dense (nd, 3), gt (N, 3), taxonomy) per (cloud, viewpoint) pair, in the reference's order (batch by
    batch, cloud-major, then viewpoint).  -> the dict of utils.evaluate.CompletionMetric.compute()."""
    losses = AverageMeter(4)
    categories = {}
    for coarse, dense, gt, taxonomy in records:
        losses.update([cd_l1(coarse, gt) * 1000, cd_l2(coarse, gt) * 1000, cd_l1(dense, gt) * 1000, cd_l2(dense, gt) * 1000])
        if in_detail:
            values = [f_score(dense, gt, th), cd_l1(dense, gt, True) * 1000, cd_l2(dense, gt, True) * 1000]
            categories.setdefault(taxonomy, AverageMeter(3)).update(values)
    overall = AverageMeter(3)
    for meter in categories.values():
        overall.update(meter.avg())
    out = dict(zip(('sparse_cd_l1', 'sparse_cd_l2', 'dense_cd_l1', 'dense_cd_l2'),
                   losses.avg() if losses.count else [math.nan] * 4))
    out.update(zip(('f_score', 'cd_l1', 'cd_l2'), overall.avg() if overall.count else [math.nan] * 3))
    out['category_metrics'] = {k: {'f_score': m.avg()[0], 'cd_l1': m.avg()[1], 'cd_l2': m.avg()[2], 'count': m.count}
                               for k, m in categories.items()}
    return out


def records_of(coarse, dense, gt, category, V):
    """Viewpoint-major batches (row v B + b) -> the reference's per-pair records, cloud-major then viewpoint."""
    B = len(gt)
    return [(coarse[v * B + b], dense[v * B + b], gt[b], int(category[b])) for b in range(B) for v in range(V)]


def _close(a, b, rel, abs_):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= abs_ + rel * abs(b)


def assert_completion_match(got, want, rel=1e-12, f_abs=0.0):
    """Every loss and CD within `rel`; F-Scores within f_abs (+ rel); the same categories with the same counts."""
    for k in ('sparse_cd_l1', 'sparse_cd_l2', 'dense_cd_l1', 'dense_cd_l2', 'cd_l1', 'cd_l2'):
        assert _close(got[k], want[k], rel, 0.0), (k, got[k], want[k])
    assert _close(got['f_score'], want['f_score'], rel, f_abs), ('f_score', got['f_score'], want['f_score'])
    assert sorted(got['category_metrics']) == sorted(want['category_metrics'])
    for c, w in want['category_metrics'].items():
        g = got['category_metrics'][c]
        assert g['count'] == w['count'], c
        for k in ('cd_l1', 'cd_l2'):
            assert _close(g[k], w[k], rel, 0.0), (c, k, g[k], w[k])
        assert _close(g['f_score'], w['f_score'], rel, f_abs), (c, g['f_score'], w['f_score'])
