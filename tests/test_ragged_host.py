"""Packed ("ragged") batches of clouds of different lengths, the part that needs no GPU: the two entry points are exported and declared,
the integer block size and the slot bound of the ragged FPS launch are what the per-cloud FPS uses, the CPU formulations
(upp_hip.torch_cpu) follow the reference's per-item recipe, and bad input is refused before anything is launched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import oracle as O
from conftest import ROOT
from upp_hip import _abi, ops, torch_cpu
from utils import misc
from utils.ingest import RaggedBatcher

ENTRY_POINTS = ("upp_fps_ragged", "upp_cloud_norm_ragged")


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "upp_hip.h")).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in exported.splitlines() if " T upp_" in l}
    for name in ENTRY_POINTS + ("upp_cloud_norm_ragged_f32", "upp_fps_ragged_slots"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _abi.SIGNATURES, name
        assert name in exported, name
    assert re.search(r"int upp_fps_ragged\(const float \*xyz, const int64_t \*offsets, int32_t \*idx, float \*centers,\s*"
                     r"int B, int max_len, int M, void \*stream\);", hdr)
    assert re.search(r"int upp_cloud_norm_ragged\(const double \*xyz, const int64_t \*offsets, float \*out, double \*scale,\s*"
                     r"int B, int max_len, void \*stream\);", hdr)
    assert _abi.load().upp_abi_version() == 5


def _block_size_int(n):
    return min(512, 1 << (n.bit_length() - 1))


def test_integer_block_size_equals_the_upstream_double_log_for_every_length():
    """The kernel derives T per cloud with an integer floor-log2 (csrc/fps.hip fps_block_size_int); upp_fps and the oracle go through
    log(n) / log(2) in double as pointnet2_ops does.  Equal for every length the kernels serve."""
    for n in range(1, 32769):
        assert _block_size_int(n) == O.fps_block_size(n), n
    src = open(os.path.join(ROOT, "iccv2025-upp_amd", "upp_hip", "csrc", "fps.hip")).read()
    assert "31 - __builtin_clz((unsigned)n)" in src and "l >= 9 ? 512 : 1 << l" in src      # (the form restated above)


@pytest.mark.parametrize("W", [1, 2, 4, 8])
@pytest.mark.parametrize("max_len", [63, 64, 511, 512, 1300, 14000, 32768])
def test_slot_bound_is_the_maximum_over_every_length(max_len, W):
    """S is compile-time, one launch serves every cloud: it must hold U(n) Q(n) for EVERY n <= max_len, and that product is not monotone."""
    L = 64 * W
    brute = 0
    for n in range(1, max_len + 1):
        T = _block_size_int(n)
        brute = max(brute, max(1, T // L) * -(-n // T))
    assert _abi.load().upp_fps_ragged_slots(max_len, W) == brute


def test_slot_bound_of_the_librarys_own_choice_fits_the_kernels():
    lib = _abi.load()
    for max_len in (1, 2, 63, 64, 128, 129, 511, 512, 513, 1300, 8192, 14000, 16384, 16385, 32768):
        assert 1 <= lib.upp_fps_ragged_slots(max_len, 0) <= 64, max_len
    assert lib.upp_fps_ragged_slots(0, 0) == -1 and lib.upp_fps_ragged_slots(64, 3) == -1 and lib.upp_fps_ragged_slots(32769, 0) == -2


# ------------------------------------------------------------------ the CPU formulations against the reference's per-item recipe
def _scans(lengths, seed, dtype=np.float64):
    """Generic (tie-free) scans in sensor units: a few metres across, off-centre."""
    rng = np.random.default_rng(seed)
    return [(rng.normal(size=(n, 3)) * rng.uniform(0.5, 3.0) + rng.normal(size=3)).astype(dtype) for n in lengths]


def _pc_norm(scan):
    """datasets/RealSensorDataset.py:59-65, verbatim arithmetic."""
    m = np.max(np.sqrt(np.sum(scan ** 2, axis=1))) * 2
    return scan / m


def _reference_item(scan, npoints, normalize=True):
    """RealSensorDataset.__getitem__: pc_norm in float64, .float(), FPS of the one cloud -> (points (npoints,3) f32, idx (npoints,))."""
    pts = (_pc_norm(np.asarray(scan, dtype=np.float64)) if normalize else np.asarray(scan)).astype(np.float32)
    idx = O.fps(pts[None], npoints)[0]
    return pts[idx], idx


@pytest.fixture
def cpu_mode():
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    yield
    torch_cpu.enable(was)


LENGTHS = [1, 3, 40, 64, 65, 200, 513]


def test_fps_ragged_on_cpu_tensors_follows_the_per_item_recipe(cpu_mode):
    scans = _scans(LENGTHS, seed=3)
    want = [_reference_item(s, 16) for s in scans]
    packed = torch.from_numpy(np.concatenate(scans))
    for arg, lengths in ((packed, LENGTHS), (packed, torch.tensor(LENGTHS)), ([torch.from_numpy(s) for s in scans], None)):
        pts, idx = misc.fps_ragged(arg, lengths, 16, normalize=True)
        assert pts.dtype == torch.float32 and idx.dtype == torch.int32 and pts.shape == (len(LENGTHS), 16, 3)
        for b, (wp, wi) in enumerate(want):
            assert np.array_equal(idx[b].numpy(), wi), b
            assert np.array_equal(pts[b].numpy().view(np.uint32), wp.view(np.uint32)), b
    # without the normalisation: float32 clouds as they are
    f32 = [torch.from_numpy(_pc_norm(s).astype(np.float32)) for s in scans]
    pts, idx = misc.fps_ragged(f32, None, 16)
    for b, (wp, wi) in enumerate(want):
        assert np.array_equal(idx[b].numpy(), wi) and np.array_equal(pts[b].numpy(), wp)


def test_batcher_on_cpu_tensors_follows_the_per_item_recipe(cpu_mode):
    scans = _scans(LENGTHS, seed=4)
    items = [(s if i % 2 else torch.from_numpy(s), np.array([i * 3]).astype(np.int32)) for i, s in enumerate(scans)]
    out = list(RaggedBatcher(iter(items), 32, 3, "cpu"))
    assert [p.shape[0] for p, _ in out] == [3, 3, 1]
    k = 0
    for pts, label in out:
        assert pts.dtype == torch.float32 and pts.shape[1:] == (32, 3) and label.dtype == torch.int64
        for b in range(pts.shape[0]):
            wp, _ = _reference_item(scans[k], 32)
            assert np.array_equal(pts[b].numpy().view(np.uint32), wp.view(np.uint32)), k
            assert int(label[b]) == k * 3
            k += 1
    assert k == len(scans)
    # float32 scans: upcast, then the same arithmetic
    scans32 = _scans([5, 77], seed=5, dtype=np.float32)
    (pts, _), = list(RaggedBatcher([(s, 0) for s in scans32], 8, 4, "cpu"))
    for b, s in enumerate(scans32):
        assert np.array_equal(pts[b].numpy(), _reference_item(s.astype(np.float64), 8)[0])


def test_cpu_tensors_are_refused_unless_the_cpu_mode_is_on():
    assert not torch_cpu.enabled()
    x = torch.rand(10, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        misc.fps_ragged(x, [4, 6], 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fps_ragged(x, torch.tensor([0, 4, 10]), 6, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cloud_norm_ragged(x.double(), torch.tensor([0, 4, 10]), 6)


# ------------------------------------------------------------------ errors, all before any launch
def test_bad_input_is_refused_before_any_launch(cpu_mode, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("an operator was reached")
    from upp_hip import functional as HF
    monkeypatch.setattr(HF, "fps_gather_ragged", no_launch)
    monkeypatch.setattr(HF, "cloud_norm_ragged", no_launch)
    x = torch.rand(10, 3)
    with pytest.raises(ValueError, match="empty"):
        misc.fps_ragged(x, [4, 0, 6], 2)
    with pytest.raises(ValueError, match="empty"):
        misc.fps_ragged([x[:4], x[:0]], None, 2)
    with pytest.raises(ValueError, match="empty"):
        list(RaggedBatcher([(np.zeros((0, 3)), 0)], 4, 2, "cpu"))
    with pytest.raises(ValueError, match="sum to"):
        misc.fps_ragged(x, [4, 5], 2)
    with pytest.raises(ValueError, match="32768"):
        misc.fps_ragged(torch.rand(32769, 3), [32769], 2)
    with pytest.raises(RuntimeError, match="contiguous"):
        misc.fps_ragged(torch.rand(3, 10).t(), [4, 6], 2)
    with pytest.raises(RuntimeError, match="float32"):
        misc.fps_ragged(x.double(), [4, 6], 2)                      # float64 only with normalize=True
    with pytest.raises(RuntimeError, match="float64 or float32"):
        misc.fps_ragged(x.half(), [4, 6], 2, normalize=True)
    with pytest.raises(RuntimeError, match="float64 or float32"):
        list(RaggedBatcher([(np.zeros((4, 3), dtype=np.int32), 0)], 4, 2, "cpu"))
    with pytest.raises(ValueError, match="lengths"):
        misc.fps_ragged(x, None, 2)


def test_the_library_refuses_bad_arguments_before_any_launch():
    lib = _abi.load()
    assert lib.upp_fps_ragged(None, None, None, None, 1, 8, 4, None) == -1
    assert lib.upp_cloud_norm_ragged(None, None, None, None, 1, 8, None) == -1
    assert lib.upp_cloud_norm_ragged_f32(None, None, None, None, 1, 8, None) == -1
    buf = (ctypes.c_double * 8)()                                   # (never read: the range check comes first)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.upp_fps_ragged(p, p, p, None, 1, 32769, 4, None) == -2
    assert lib.upp_fps_ragged(p, p, p, None, 1, 0, 4, None) == -1 and lib.upp_fps_ragged(p, p, p, None, 1, 8, 0, None) == -1
    assert lib.upp_fps_ragged(p, p, p, None, 0, 8, 4, None) == 0    # an empty batch: nothing to do


def test_layout_is_derived_on_the_host():
    off, max_len = ops.ragged_layout([3, 1, 7], 11)
    assert off.tolist() == [0, 3, 4, 11] and off.dtype == torch.int64 and not off.is_cuda and max_len == 7
    off, max_len = ops.ragged_layout(torch.tensor([5]), 5, max_len=9)
    assert off.tolist() == [0, 5] and max_len == 9
    with pytest.raises(ValueError, match="max_len"):
        ops.ragged_layout([5, 12], 17, max_len=8)
    assert ops.ragged_layout([40000], 40000, fps=False)[1] == 40000   # the normalisation alone has no length limit
