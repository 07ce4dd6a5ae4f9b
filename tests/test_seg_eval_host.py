"""Part-segmentation evaluation on a GPU-less host: the part table, SegMetric's CPU path and validate_seg against the numpy restatement
of the reference's `validate` (tests/_seg_reference.py), the two entry points of csrc/seg_eval.hip (declared, bound, exported, their
arguments refused before any launch), ops refusing CPU tensors, and a 2-rank gloo SegMetric against one process."""
import ctypes
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from _seg_reference import SEG_CLASSES, assert_metrics_match, planted_batch, reference_metrics
from conftest import ROOT
from upp_hip import _abi
from utils import evaluate

NEW = ("upp_seg_iou_counts", "upp_seg_iou_accumulate")


def _metric(batches, n_valid=None):
    m = evaluate.SegMetric()
    ious = []
    for i, (logp, target) in enumerate(batches):
        nv = None if n_valid is None else n_valid[i]
        ious.append(m.update(torch.from_numpy(logp), torch.from_numpy(target), n_valid=nv))
    return m, torch.cat(ious)


def _check(batches, n_valid=None):
    m, ious = _metric(batches, n_valid)
    cut = batches if n_valid is None else [(lp[:nv], t[:nv]) for (lp, t), nv in zip(batches, n_valid)]
    want = reference_metrics(cut)
    got = m.compute()
    assert np.array_equal(ious.numpy().view(np.int64), want['shape_iou'].view(np.int64)), (ious, want['shape_iou'])
    s = m.sums
    assert s.counters.tolist() == [want['correct'], want['seen'], 0]
    assert np.array_equal(s.part_seen.numpy(), want['part_seen'])
    assert np.array_equal(s.part_correct.numpy(), want['part_correct'])
    assert_metrics_match(got, want)
    return got, want


# ------------------------------------------------------------------ the part table
def test_the_part_table_covers_every_part_once_in_category_order():
    names, part_cat, cat_range = evaluate.seg_tables()
    assert names == sorted(SEG_CLASSES) and len(names) == 16
    assert part_cat.dtype == torch.int32 and cat_range.dtype == torch.int32 and tuple(cat_range.shape) == (16, 2)
    assert sorted(p for _, parts in evaluate.SHAPENET_PART for p in parts) == list(range(50))
    lo = 0
    for c, name in enumerate(names):
        assert list(range(int(cat_range[c, 0]), int(cat_range[c].sum()))) == SEG_CLASSES[name]
        assert int(cat_range[c, 0]) == lo                                     # contiguous, in order
        lo += int(cat_range[c, 1])
        assert (part_cat[SEG_CLASSES[name]] == c).all()
    assert lo == 50
    with pytest.raises(ValueError):
        evaluate.seg_tables((('A', (0, 2)), ('B', (1,))))
    with pytest.raises(ValueError):
        evaluate.seg_tables((('A', (0, 1)), ('B', (1,))))
    with pytest.raises(ValueError):
        evaluate.SegMetric(num_part=40)


# ------------------------------------------------------------------ SegMetric (CPU path) against the restatement
@pytest.mark.parametrize("B,N", [(1, 1), (3, 100), (8, 2048), (2, 2500)])
def test_random_and_planted_batches(B, N):
    _check([planted_batch(B, N, seed=B * 7 + N), planted_batch(B, N, seed=B * 7 + N + 1, nan_rows=False, ties=False)])


def test_a_part_absent_on_both_sides_has_iou_one_and_a_part_predicted_only_has_iou_zero():
    N = 8
    logp = np.full((2, N, 50), -10.0, dtype=np.float32)
    target = np.zeros((2, N), dtype=np.int64)
    # shape 0, Airplane (0..3): target and prediction 0 everywhere -> parts 1..3 absent on both sides -> IoU (1 + 1 + 1 + 1) / 4
    logp[0, :, 0] = -0.1
    # shape 1, Bag (4, 5): target 4 everywhere, part 5 predicted on two points -> IoU(4) = 6/8, IoU(5) = 0
    target[1] = 4
    logp[1, :, 4] = -0.1
    logp[1, :2, 5] = 0.0
    got, want = _check([(logp, target)])
    assert want['shape_iou'].tolist() == [1.0, (6 / 8 + 0.0) / 2]


def test_exact_ties_and_nan_rows_follow_np_argmax():
    logp, target = planted_batch(4, 16, seed=3)
    pred = torch.empty(4, 16, dtype=torch.long)
    m = evaluate.SegMetric()
    m.update(torch.from_numpy(logp), torch.from_numpy(target), pred=pred)
    want = reference_metrics([(logp, target)])
    assert np.array_equal(pred.numpy(), want['pred'][0])
    for i in range(4):
        lo = int(evaluate.seg_tables()[2][evaluate.seg_tables()[1][target[i, 0]], 0])
        assert pred[i, 1] == lo and pred[i, 3] == lo                         # all equal / all NaN: the first part


def test_the_category_comes_from_the_first_target_not_the_label():
    class Stub(torch.nn.Module):
        def __init__(self, logp):
            super().__init__()
            self.logp, self.seen = logp, []
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, pts, cls_label, completion_prompt=True, denoise=True, point_num=1024):
            self.seen.append((cls_label.clone(), completion_prompt, denoise, point_num, self.training))
            return self.logp[pts[:, 0, 0].long()]

    logp, target = planted_batch(5, 64, seed=9)
    label = torch.tensor([[15], [0], [3], [7], [9]])                         # (B, 1), deliberately not target's categories
    pts = torch.zeros(5, 64, 3)
    pts[:, 0, 0] = torch.arange(5.)
    model = Stub(torch.from_numpy(logp)).train()
    got, pred = evaluate.validate_seg(model, [(pts[:3], label[:3], torch.from_numpy(target[:3])),
                                              (pts[3:], label[3:], torch.from_numpy(target[3:]))], return_predictions=True)
    want = reference_metrics([(logp[:3], target[:3]), (logp[3:], target[3:])])
    assert_metrics_match(got, want)
    assert np.array_equal(pred.numpy(), np.concatenate(want['pred']))
    assert model.training, "the training flag is restored"
    onehot, cp, dn, pn, training = model.seen[0]
    assert torch.equal(onehot, torch.eye(16)[[15, 0, 3]]) and (cp, dn, pn, training) == (False, False, 64, False)


def test_missing_categories_and_parts_give_nan_as_the_reference():
    logp, target = planted_batch(2, 50, seed=4)
    got, want = _check([(logp, target)])
    assert np.isnan(got['class_avg_iou']) and np.isnan(got['class_avg_accuracy'])
    assert sum(np.isnan(v) for v in got['category_iou'].values()) >= 14
    empty = evaluate.SegMetric().compute()
    assert all(np.isnan(empty[k]) for k in ('accuracy', 'class_avg_accuracy', 'class_avg_iou', 'inctance_avg_iou'))


def test_a_ragged_n_valid_counts_only_the_real_shapes():
    a, b = planted_batch(4, 300, seed=5), planted_batch(4, 300, seed=6)
    b[1][3, 0] = 99                                                          # padding rows are never read as shapes
    _check([a, b], n_valid=[4, 2])
    _check([a, b], n_valid=[0, 1])


def test_a_first_target_outside_the_parts_raises_when_read():
    logp, target = planted_batch(3, 20, seed=8)
    target[1, 0] = 50
    m = evaluate.SegMetric()
    m.update(torch.from_numpy(logp), torch.from_numpy(target))
    assert m.sums.counters.tolist()[2] == 1
    with pytest.raises(ValueError, match="1 shape"):
        m.compute()


# ------------------------------------------------------------------ the native entry points
def test_the_seg_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "upp_hip.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _abi.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, exported), name
    assert _abi.load().upp_abi_version() == 5


def test_seg_arguments_are_checked_before_any_launch():
    lib = _abi.load()
    p = ctypes.c_void_p(256)            # never dereferenced: every case below is refused on the host
    ok = dict(ld=50, B=4, N=2048, P=50, C=16, nv=4)

    def counts(**kw):
        a = dict(ok, **kw)
        ptrs = [kw.get(k, p) for k in ("logp", "target", "part_cat", "cat_range", "scratch")]
        return lib.upp_seg_iou_counts(ptrs[0], a["ld"], ptrs[1], ptrs[2], ptrs[3], a["B"], a["N"], a["P"], a["C"], a["nv"], None,
                                      ptrs[4], None)

    def accumulate(nulls=(), **kw):
        a = dict(ok, **kw)
        ptrs = [None if i in nulls else p for i in range(11)]
        return lib.upp_seg_iou_accumulate(ptrs[0], ptrs[1], ptrs[2], ptrs[3], a["B"], a["N"], a["P"], a["C"], a["nv"], *ptrs[4:], None)
    for k in ("logp", "target", "part_cat", "cat_range", "scratch"):
        assert counts(**{k: None}) == -1, k
    for kw in (dict(B=0), dict(N=0), dict(P=0), dict(C=0), dict(ld=49)):
        assert counts(**kw) == -1, kw
    for kw in (dict(nv=5), dict(nv=-1), dict(P=1025, ld=1025), dict(C=257), dict(B=70000), dict(B=40000, N=60000)):
        assert counts(**kw) == -2, kw
    for i in range(11):
        assert accumulate(nulls=(i,)) == -1, i
    for kw in (dict(B=0), dict(N=0), dict(P=0), dict(C=0)):
        assert accumulate(**kw) == -1, kw
    for kw in (dict(nv=5), dict(nv=-1), dict(P=1025), dict(C=257)):
        assert accumulate(**kw) == -2, kw


def test_cpu_tensors_are_rejected_by_ops():
    from upp_hip import ops
    _, pc, cr = evaluate.seg_tables()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.seg_iou_update(torch.zeros(2, 8, 50), torch.zeros(2, 8, dtype=torch.long), pc, cr, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.SegAccumulator(50, 16, 'cpu')


# ------------------------------------------------------------------ distributed
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _seg_batches():
    return [planted_batch(3, 200, seed=40 + i) for i in range(4)]


def _dist_worker(rank, world, port, out_dir):
    sys.path[:0] = os.environ["UPP_TEST_PATHS"].split(os.pathsep)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from utils import evaluate as ev
    dist.init_process_group('gloo')
    m = ev.SegMetric()
    for logp, target in _seg_batches()[rank::world]:
        m.update(torch.from_numpy(logp), torch.from_numpy(target))
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
    batches = _seg_batches()
    m = evaluate.SegMetric()
    for logp, target in batches:
        m.update(torch.from_numpy(logp), torch.from_numpy(target))
    one = m.compute()
    want = reference_metrics(batches)
    for got in (r0, r1):
        assert_metrics_match(got, one)
        assert_metrics_match(got, want)
        assert got['accuracy'] == one['accuracy']                            # integer sums: exact
