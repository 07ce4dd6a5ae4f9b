"""Packed ("ragged") batches on the GPU: upp_fps_ragged against the oracle and against upp_fps on every cloud alone (bit-identical
indices: the tie order follows the cloud's OWN length), upp_cloud_norm_ragged against the numpy statement of the reference's pc_norm
(bit-identical), RaggedBatcher against the per-scan loop of the reference's RealSensorDataset, and the pair inside a captured graph."""
import os
import sys

import numpy as np
import pytest
import torch

import _seeded
import oracle as O
from conftest import ROOT
from upp_hip import functional as HF
from upp_hip import ops
from utils import evaluate, misc
from utils.ingest import RaggedBatcher

pytestmark = pytest.mark.gpu


def _pack(clouds):
    """list of (n_i,3) f32 CPU tensors -> (packed on the GPU, host offsets, lengths)."""
    lengths = [c.shape[0] for c in clouds]
    offsets, _ = ops.ragged_layout(lengths)
    return torch.cat(clouds).cuda(), offsets, lengths


def _check_fps(clouds, M, max_len=None):
    """ragged == oracle == upp_fps on the cloud alone, centres == the gathered points; the figures are printed before they are asserted."""
    packed, offsets, lengths = _pack(clouds)
    idx, cen = ops.fps_ragged(packed, offsets, max_len or max(lengths), M, want_centers=True)
    assert idx.shape == (len(clouds), M) and idx.dtype == torch.int32 and cen.shape == (len(clouds), M, 3)
    idx, cen = idx.cpu().numpy(), cen.cpu().numpy()
    bad = []
    for b, c in enumerate(clouds):
        want = O.fps(c.numpy()[None], M)[0]
        alone = ops.fps(c[None].cuda().contiguous(), M).cpu().numpy()[0]
        d_or, d_al = int((idx[b] != want).sum()), int((idx[b] != alone).sum())
        d_cen = int((cen[b].view(np.uint32) != c.numpy()[idx[b].clip(0, len(c) - 1)].view(np.uint32)).sum())
        print("cloud %d n = %d M = %d: %d indices off the oracle, %d off upp_fps, %d centre words off" % (b, len(c), M, d_or, d_al, d_cen))
        if d_or or d_al or d_cen or idx[b].min() < 0 or idx[b].max() >= len(c):
            bad.append((b, len(c)))
    assert not bad, bad


def _generic(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, 3, generator=g) * 0.4 for n in lengths]


# n < M, T < 64 (idle lanes), powers of two, the cap at T = 512, idle waves (short clouds beside a 1300-point one: 4 waves per cloud)
PARITY_LENGTHS = [1, 3, 63, 64, 65, 200, 511, 512, 513, 1300]


@pytest.mark.parametrize("M", [64, 8])
def test_fps_parity_per_cloud(M):
    _check_fps(_generic(PARITY_LENGTHS, seed=11), M)


def test_fps_parity_beside_a_large_cloud():
    """One 14,000-point cloud beside two short ones: 3 * 14000 floats do not fit the LDS -> the global-memory form, 56 slots per lane."""
    _check_fps(_generic([5, 14000, 700], seed=12), 32)


def test_fps_oversized_promise_changes_nothing():
    """max_len is a bound, not a length: a larger promise picks other launch forms (waves, slots), never other indices."""
    clouds = _generic([3, 65, 200], seed=13)
    for max_len in (200, 512, 700, 5000):
        _check_fps(clouds, 16, max_len=max_len)


def test_fps_cuts_a_cloud_that_breaks_the_promise():
    """Device-side offsets are the caller's promise; a cloud longer than max_len is sampled from its first max_len points, inside its rows."""
    clouds = _generic([40, 150, 64], seed=14)
    packed, offsets, _ = _pack(clouds)
    idx = ops.fps_ragged(packed, offsets.cuda(), 100, 16).cpu().numpy()
    for b, c in enumerate(clouds):
        assert np.array_equal(idx[b], O.fps(c.numpy()[None, :100], 16)[0]), b


def _grid(n, g, fine=False):
    """coordinates on a coarse grid (multiples of 1/8): many equal distances, duplicated points.  fine: multiples of 1/64 in [-1/64, 1/64],
    |p|^2 <= 3/4096 < 1e-3 -- never candidates."""
    if fine:
        return torch.randint(-1, 2, (n, 3), generator=g).float() / 64
    return torch.randint(-8, 9, (n, 3), generator=g).float() / 8


def test_fps_ties_and_the_skip_rule():
    g = torch.Generator().manual_seed(21)
    clouds = [_grid(n, g) for n in (5, 64, 130, 300, 600, 1100)]
    third = _grid(450, g)
    third[torch.randperm(450, generator=g)[:150]] = _grid(150, g, fine=True)          # a third of its points inside |p|^2 <= 1e-3
    inside = _grid(90, g, fine=True)                                                   # entirely inside: every round returns 0
    assert int(((third ** 2).sum(-1) <= 1e-3).sum()) >= 150 and bool(((inside ** 2).sum(-1) <= 1e-3).all())
    clouds += [third, inside]
    assert O.fps(inside.numpy()[None], 8)[0].tolist() == [0] * 8
    for M in (48, 8):
        _check_fps(clouds, M)


# ------------------------------------------------------------------ normalisation
def _pc_norm(scan):
    """datasets/RealSensorDataset.py:59-65, the numpy statement (float64)."""
    m = np.max(np.sqrt(np.sum(scan ** 2, axis=1))) * 2
    return scan / m, m


def _scans(lengths, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return [(rng.normal(size=(n, 3)) * rng.uniform(0.5, 3.0) + rng.normal(size=3)).astype(dtype) for n in lengths]


NORM_LENGTHS = [1, 2, 777, 5000]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cloud_norm_is_the_numpy_statement(dtype):
    scans = _scans(NORM_LENGTHS, seed=31, dtype=dtype)
    offsets, max_len = ops.ragged_layout(NORM_LENGTHS, fps=False)
    packed = torch.from_numpy(np.concatenate(scans)).cuda()
    out, scale = ops.cloud_norm_ragged(packed, offsets, max_len, want_scale=True)
    assert out.dtype == torch.float32 and out.shape == packed.shape and scale.dtype == torch.float64 and scale.shape == (4,)
    assert torch.equal(ops.cloud_norm_ragged(packed, offsets.cuda(), max_len, lengths=NORM_LENGTHS), out)
    out, scale, o = out.cpu().numpy(), scale.cpu().numpy(), offsets.tolist()
    bad = []
    for b, s in enumerate(scans):
        want, m = _pc_norm(s.astype(np.float64))                    # (the f32 overload: the statement applied to the upcast input)
        want = want.astype(np.float32)
        d = int((out[o[b]:o[b + 1]].view(np.uint32) != want.view(np.uint32)).sum())
        print("cloud %d n = %d: %d output words off, scale %r (numpy %r)" % (b, len(s), d, float(scale[b]), float(m)))
        if d or scale[b].view(np.uint64) != np.float64(m).view(np.uint64):
            bad.append(b)
    assert not bad, bad
    assert scale[0] == np.sqrt(np.sum(scans[0].astype(np.float64)[0] ** 2)) * 2      # a single point: its own norm, twice


# ------------------------------------------------------------------ end to end
def test_batcher_equals_the_per_scan_loop_and_feeds_validate():
    from models import build_model_from_cfg
    from utils.config import builtin_cfg
    npoints = 1024
    lengths = [1500, 1100, 2048, 1300, 1024, 3000, 1201]
    scans = [_seeded.noisy_clouds(1, n - 72, seed=40 + i)[0].double().numpy() * (1.5 + i) + 0.25 * i for i, n in enumerate(lengths)]
    assert [len(s) for s in scans] == lengths
    labels = [int(v) for v in torch.randint(0, 40, (7,), generator=torch.Generator().manual_seed(41))]
    # the reference's way (RealSensorDataset.__getitem__): normalise on the host, one FPS launch per scan
    loop = [misc.fps(torch.from_numpy(_pc_norm(s)[0]).float().cuda()[None], npoints)[0][0] for s in scans]
    want = [(torch.stack(loop[i:i + 3]), torch.tensor(labels[i:i + 3]).cuda()) for i in (0, 3, 6)]
    got = list(RaggedBatcher(zip(scans, labels), npoints, 3, "cuda"))
    assert [p.shape for p, _ in got] == [(3, npoints, 3), (3, npoints, 3), (1, npoints, 3)]
    for (p, l), (wp, wl) in zip(got, want):
        assert p.dtype == torch.float32 and torch.equal(p.view(torch.int32), wp.view(torch.int32)) and torch.equal(l, wl)
    model = _seeded.fill(build_model_from_cfg(builtin_cfg('unify_modelnet_cls').model)).cuda().eval()
    acc = evaluate.validate(model, RaggedBatcher(zip(scans, labels), npoints, 3, "cuda"), npoints)
    acc_loop = evaluate.validate(model, want, npoints)
    assert float(acc) == float(acc_loop)
    with torch.no_grad():
        pred = torch.cat([model(p, completion_prompt=False, denoise=False, point_num=npoints).argmax(-1) for p, _ in got])
        pred_loop = torch.cat([model(p, completion_prompt=False, denoise=False, point_num=npoints).argmax(-1) for p, _ in want])
    assert torch.equal(pred, pred_loop)
    assert float(acc) == float((pred == torch.tensor(labels).cuda()).sum()) / 7 * 100.


# ------------------------------------------------------------------ graph safety
def test_the_pair_replays_from_a_graph_and_issues_no_memset():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
    from memset_census import memsets_of
    M, max_len = 32, 600
    layouts = [[600, 5, 130, 265], [1, 599, 200, 200], [250, 250, 250, 250]]           # same T and B: the same buffers, other contents
    T = sum(layouts[0])
    xyz = torch.zeros(T, 3, dtype=torch.float64, device='cuda')
    offsets = torch.zeros(5, dtype=torch.int64, device='cuda')

    def fill(k):
        xyz.copy_(torch.from_numpy(np.concatenate(_scans(layouts[k], seed=50 + k))))
        offsets.copy_(ops.ragged_layout(layouts[k], T, max_len)[0])

    def pair():
        pts = ops.cloud_norm_ragged(xyz, offsets, max_len)
        return ops.fps_ragged(pts, offsets, max_len, M, want_centers=True)

    fill(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pair()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        idx, cen = pair()
    for k in (1, 2, 0):
        fill(k)
        g.replay()
        torch.cuda.synchronize()
        e_idx, e_cen = pair()
        assert torch.equal(idx, e_idx) and torch.equal(cen.view(torch.int32), e_cen.view(torch.int32)), k
        scans = _scans(layouts[k], seed=50 + k)
        for b, sc in enumerate(scans):
            pts = _pc_norm(sc)[0].astype(np.float32)
            assert np.array_equal(idx[b].cpu().numpy(), O.fps(pts[None], M)[0]), (k, b)
    found = memsets_of(pair)
    assert not found, found
