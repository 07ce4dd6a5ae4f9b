"""Point-completion evaluation on a GPU-less host: CompletionMetric's CPU path against the numpy restatement of the reference's pre-task
`validate` (tests/_completion_reference.py) -- zero-sum points and an all-zero cloud, points just inside and just outside the F-Score
threshold, p + r = 0, uneven categories -- the mode and viewpoint tables, the three entry points of csrc/completion_eval.hip (declared,
bound, exported, their arguments refused before any launch), bad arguments, and a 2-rank gloo CompletionMetric against one process."""
import ctypes
import math
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from _completion_reference import CROP_RATIO, VIEWPOINTS, assert_completion_match, records_of, reference_metrics
from conftest import ROOT
from upp_hip import _abi
from utils import evaluate

NEW = ("upp_completion_cloud_metrics", "upp_completion_masked_cd", "upp_completion_accumulate")


def spread_cloud(rng, n, spacing=0.05):
    """n points in [-1, 1]^3 whose pairwise distances all exceed `spacing` (a jittered grid)."""
    k = int(math.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.linspace(-0.9, 0.9, k)] * 3, indexing='ij'), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:n]]
    return (g + rng.uniform(-0.2, 0.2, g.shape) * (1.8 / max(k - 1, 1) - spacing) / 2).astype(np.float32)


def batch(B=3, V=2, N=216, nc=20, nd=60, seed=0):
    """gt (B, N, 3), coarse (V B, nc, 3), dense (V B, nd, 3): dense points sit near gt points, some inside the threshold, some out."""
    rng = np.random.default_rng(seed)
    gt = np.stack([spread_cloud(rng, N) for _ in range(B)])
    coarse = rng.uniform(-1, 1, (V * B, nc, 3)).astype(np.float32)
    dense = np.empty((V * B, nd, 3), np.float32)
    for r in range(V * B):
        pick = rng.choice(N, nd, replace=False)
        u = rng.normal(size=(nd, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        dense[r] = gt[r % B][pick] + u * rng.choice([0.002, 0.0099, 0.0101, 0.02], nd)[:, None]
    return gt, coarse, dense


def _metric(batches, C=4, detail=True, n_valid=None, names=None):
    m = evaluate.CompletionMetric(C, names=names)
    for i, (gt, coarse, dense, cat) in enumerate(batches):
        nv = None if n_valid is None else n_valid[i]
        m.update(torch.from_numpy(coarse), torch.from_numpy(dense), torch.from_numpy(gt), torch.tensor(cat) if detail else None, nv)
    return m


def _records(batches, n_valid=None):
    out = []
    for i, (gt, coarse, dense, cat) in enumerate(batches):
        B, V = len(gt), len(coarse) // len(gt)
        nv = B if n_valid is None else n_valid[i]
        out += records_of(coarse, dense, gt, cat, V)[:nv * V]          # (cloud-major: the first nv clouds)
    return out


def _check(batches, C=4, detail=True, n_valid=None):
    got = _metric(batches, C, detail, n_valid).compute()
    want = reference_metrics(_records(batches, n_valid), detail)
    assert_completion_match(got, want, rel=1e-12)
    return got, want


# ------------------------------------------------------------------ the tables
def test_the_modes_and_the_eight_viewpoints_are_the_references():
    assert evaluate.VIEWPOINTS == tuple(tuple(float(x) for x in v) for v in VIEWPOINTS)
    assert evaluate.viewpoints(False) == evaluate.VIEWPOINTS[:1] and evaluate.viewpoints(True) == evaluate.VIEWPOINTS
    for mode, ratio in CROP_RATIO.items():
        for n in (8192, 2048, 1001):
            assert evaluate.crop_count(n, mode) == int(n * ratio)
    assert [evaluate.crop_count(8192, m) for m in ('easy', 'median', 'hard')] == [2048, 4096, 6144]
    with pytest.raises(ValueError, match="mode"):
        evaluate.crop_count(8192, 'medium')


# ------------------------------------------------------------------ the CPU path against the restatement
@pytest.mark.parametrize("detail", [True, False])
def test_the_cpu_metric_matches_the_reference(detail):
    batches = []
    for i in range(3):
        gt, coarse, dense = batch(seed=i)
        batches.append((gt, coarse, dense, [i % 4, 1, 3]))
    got, want = _check(batches, detail=detail)
    assert 0.0 < got['dense_cd_l2'] and got['sparse_cd_l1'] > got['dense_cd_l1']
    if detail:
        assert 0.0 < got['f_score'] < 1.0
        assert sorted(got['category_metrics']) == [0, 1, 2, 3]
    else:
        assert got['category_metrics'] == {} and math.isnan(got['f_score'])


def test_points_just_inside_and_just_outside_the_threshold_count_exactly():
    rng = np.random.default_rng(7)
    gt = spread_cloud(rng, 64)[None]
    u = rng.normal(size=(64, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    inside = np.arange(64) % 3 == 0
    dense = (gt[0] + u * np.where(inside, 0.0099, 0.0101)[:, None]).astype(np.float32)[None]
    m = evaluate.CompletionMetric(1)
    m.update(torch.from_numpy(gt[:, :8]), torch.from_numpy(dense), torch.from_numpy(gt), torch.tensor([0]))
    p = r = inside.sum() / 64.0                         # each dense point's partner is its own gt point, and the reverse
    assert m.compute()['f_score'] == 2 * r * p / (r + p)
    want = reference_metrics([(gt[0, :8], dense[0], gt[0], 0)], True)
    assert_completion_match(m.compute(), want)


def test_no_point_within_the_threshold_gives_f_zero():
    gt, coarse, dense = batch(B=2, V=1, seed=3)
    dense = dense + np.float32(5.0)
    got, _ = _check([(gt, coarse, dense, [0, 1])])
    assert got['f_score'] == 0.0 and got['category_metrics'][0]['f_score'] == 0.0


def test_zero_sum_points_are_removed_from_the_metric_cds_only():
    gt, coarse, dense = batch(B=3, V=1, seed=4)
    gt[0, :5] = [[0.5, -0.25, -0.25], [0, 0, 0], [0.25, 0.25, -0.5], [-1.0, 0.5, 0.5], [0.125, -0.0625, -0.0625]]
    dense[1, 3:7] = [[0.5, -0.5, 0.0], [0.0, 0.0, 0.0], [0.75, -0.25, -0.5], [-0.5, 0.25, 0.25]]
    dense[2] = [[0.5, -0.25, -0.25]] * dense.shape[1]               # every point zero-sum: CDL1 / CDL2 NaN
    for r in range(3):
        x = torch.from_numpy(dense[r] if r else gt[0])
        assert bool(evaluate._zero_sum(x).any())
    m = _metric([(gt, coarse, dense, [0, 1, 2])], C=3)
    got = m.compute()
    want = reference_metrics(_records([(gt, coarse, dense, [0, 1, 2])]), True)
    assert_completion_match(got, want)
    c = got['category_metrics']
    assert math.isnan(c[2]['cd_l1']) and math.isnan(c[2]['cd_l2']) and not math.isnan(c[2]['f_score'])
    assert math.isnan(got['cd_l1']), "the mean over categories carries the NaN, as AverageMeter does"
    assert not math.isnan(got['dense_cd_l1']), "the losses keep every point (ignore_zeros=False)"
    plain = reference_metrics([(coarse[0], dense[0], gt[0], 0)], True)['dense_cd_l1']
    assert c[0]['cd_l1'] != plain, "a cloud with zero-sum points takes the masked CDs"


def test_categories_are_averaged_then_the_category_means_are_averaged():
    gt, coarse, dense = batch(B=4, V=2, seed=5)
    g2, c2, d2 = batch(B=2, V=2, seed=6)
    batches = [(gt, coarse, dense, [3, 0, 3, 3]), (g2, c2, d2, [0, 5])]
    got, want = _check(batches, C=6)
    cm = got['category_metrics']
    assert {k: v['count'] for k, v in cm.items()} == {0: 4, 3: 6, 5: 2}
    means = [cm[k]['cd_l2'] for k in (0, 3, 5)]
    assert got['cd_l2'] == pytest.approx(sum(means) / 3, rel=1e-15)
    named = _metric(batches, C=6, names=list('abcdef')).compute()
    assert sorted(named['category_metrics']) == ['a', 'd', 'f']


def test_a_ragged_n_valid_counts_only_the_real_clouds():
    gt, coarse, dense = batch(B=3, V=2, seed=8)
    m = _metric([(gt, coarse, dense, [0, 1, 2])], C=3, n_valid=[2])
    want = reference_metrics(records_of(coarse, dense, gt, [0, 1, 2], 2)[:4], True)
    assert_completion_match(m.compute(), want)
    assert int(m.sums.counters[0]) == 4


def test_bad_arguments_are_refused():
    gt, coarse, dense = (torch.from_numpy(x) for x in batch(B=2, V=2, seed=9))
    m = evaluate.CompletionMetric(2)
    with pytest.raises(ValueError, match="V x 2"):
        m.update(coarse[:3], dense[:3], gt)
    with pytest.raises(ValueError, match="V x 2"):
        m.update(coarse, dense[:2], gt)
    with pytest.raises(ValueError, match="points, 3"):
        m.update(coarse[..., :2], dense, gt)
    with pytest.raises(ValueError, match="n_valid"):
        m.update(coarse, dense, gt, n_valid=3)
    with pytest.raises(ValueError, match="category"):
        m.update(coarse, dense, gt, torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match="category"):
        m.update(coarse, dense, gt, torch.tensor([0, 1, 1]))
    m.update(coarse, dense, gt, torch.tensor([0, 2]))
    with pytest.raises(ValueError, match="outside"):
        m.compute()
    for kw in (dict(num_categories=0), dict(threshold=0.0), dict(threshold=float('inf')), dict(num_categories=2, names=['a'])):
        with pytest.raises(ValueError):
            evaluate.CompletionMetric(**kw)


def test_cpu_tensors_are_rejected_by_ops():
    from upp_hip import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.CompletionAccumulator(2, 'cpu')
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.completion_update(torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), None)


# ------------------------------------------------------------------ the native entry points
def test_the_completion_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "upp_hip.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _abi.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, exported), name
    assert _abi.load().upp_abi_version() == 5


def test_completion_arguments_are_checked_before_any_launch():
    lib = _abi.load()
    p = ctypes.c_void_p(256)            # never dereferenced: every case below is refused on the host

    def cloud(nulls=(), B=4, n=2048, m=8192, th=0.01, detail=1):
        ptrs = [None if i in nulls else p for i in range(8)]
        return lib.upp_completion_cloud_metrics(*ptrs[:6], B, n, m, th, detail, ptrs[6], ptrs[7], None)

    def masked(nulls=(), B=4, n=2048, m=8192):
        ptrs = [None if i in nulls else p for i in range(4)]
        return lib.upp_completion_masked_cd(ptrs[0], ptrs[1], B, n, m, ptrs[2], ptrs[3], None)

    def accumulate(nulls=(), V=8, B=4, C=55, nv=4, category=True):
        ptrs = [None if i in nulls else p for i in range(7)]
        return lib.upp_completion_accumulate(ptrs[0], ptrs[1], ptrs[2] if category else None, V, B, C, nv, *ptrs[3:], None)
    for i in range(8):
        assert cloud(nulls=(i,)) == -1, i
    for kw in (dict(B=0), dict(n=0), dict(m=0), dict(th=0.0), dict(th=-0.01), dict(th=float('nan')), dict(th=float('inf')),
               dict(detail=2)):
        assert cloud(**kw) == -1, kw
    for kw in (dict(B=(1 << 20) + 1), dict(n=(1 << 22) + 1), dict(m=(1 << 22) + 1)):
        assert cloud(**kw) == -2, kw
    for i in range(4):
        assert masked(nulls=(i,)) == -1, i
    for kw in (dict(B=0), dict(n=0), dict(m=0)):
        assert masked(**kw) == -1, kw
    assert masked(B=(1 << 20) + 1) == -2
    for i in (0, 1, 3, 4, 5, 6):
        assert accumulate(nulls=(i,)) == -1, i
    for kw in (dict(V=0), dict(B=0), dict(C=0)):
        assert accumulate(**kw) == -1, kw
    for kw in (dict(nv=5), dict(nv=-1), dict(V=65), dict(C=4097), dict(V=64, B=(1 << 14) + 1)):
        assert accumulate(**kw) == -2, kw


# ------------------------------------------------------------------ distributed
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _batches():
    return [(*batch(B=2, V=2, seed=20 + i), [i % 3, (i + 1) % 3]) for i in range(4)]


def _update(m, batches):
    for gt, coarse, dense, cat in batches:
        m.update(torch.from_numpy(coarse), torch.from_numpy(dense), torch.from_numpy(gt), torch.tensor(cat))


def _dist_worker(rank, world, port, out_dir):
    sys.path[:0] = os.environ["UPP_TEST_PATHS"].split(os.pathsep)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from utils import evaluate as ev
    dist.init_process_group('gloo')
    m = ev.CompletionMetric(3)
    _update(m, _batches()[rank::world])
    out = m.compute(distributed=True)
    torch.save(out, os.path.join(out_dir, "r%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_gloo_metric_equals_one_process_over_the_union(tmp_path):
    from conftest import PKG
    os.environ["UPP_TEST_PATHS"] = os.pathsep.join([os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), PKG])
    mp.spawn(_dist_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    m = evaluate.CompletionMetric(3)
    _update(m, _batches())
    one = m.compute()
    want = reference_metrics(sum((records_of(c, d, g, k, 2) for g, c, d, k in _batches()), []), True)
    for got in (r0, r1):
        assert_completion_match(got, one, rel=1e-13)
        assert_completion_match(got, want, rel=1e-12)
