"""Captured evaluation on a GPU-less host: the two entry points of csrc/eval.hip are declared, bound and exported, check their
arguments before any launch, and the host-side planning of EvalStep (vote chunks, padding of a ragged batch)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from upp_hip import _abi

NEW = ("upp_vote_points", "upp_vote_reduce")


def test_the_vote_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "upp_hip.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _abi.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, exported), name
    assert _abi.load().upp_abi_version() == 5


def test_vote_arguments_are_checked_before_any_launch():
    lib = _abi.load()
    p = ctypes.c_void_p(256)            # never dereferenced: every case below is refused on the host
    assert lib.upp_vote_points(None, p, None, None, p, 4, 1200, 1024, 10, None) == -1
    assert lib.upp_vote_points(p, None, None, None, p, 4, 1200, 1024, 10, None) == -1
    assert lib.upp_vote_points(p, p, None, None, None, 4, 1200, 1024, 10, None) == -1
    for B, S, N, V in ((0, 1200, 1024, 10), (4, 0, 1024, 10), (4, 1200, 0, 10), (4, 1200, 1024, 0)):
        assert lib.upp_vote_points(p, p, p, p, p, B, S, N, V, None) == -1
    assert lib.upp_vote_points(p, p, p, p, p, 1 << 16, 1200, 1024, 1 << 16, None) == -2
    assert lib.upp_vote_reduce(None, p, 10, 4, 40, 4, p, p, None) == -1
    assert lib.upp_vote_reduce(p, p, 10, 4, 40, 4, None, p, None) == -1
    assert lib.upp_vote_reduce(p, p, 10, 4, 40, 4, p, None, None) == -1
    assert lib.upp_vote_reduce(p, p, 0, 4, 40, 4, p, p, None) == -1
    assert lib.upp_vote_reduce(p, p, 10, 4, 0, 4, p, p, None) == -1
    assert lib.upp_vote_reduce(p, p, 10, 4, 40, 5, p, p, None) == -2
    assert lib.upp_vote_reduce(p, p, 10, 4, 40, -1, p, p, None) == -2
    assert lib.upp_vote_reduce(p, p, 1 << 16, 1 << 16, 40, 4, p, p, None) == -2


def test_cpu_tensors_are_rejected():
    from upp_hip import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.vote_points(torch.zeros(2, 10, 3), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.vote_reduce(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long), 1, 2, torch.zeros(2, dtype=torch.long),
                        torch.zeros(2, dtype=torch.long))


def test_vote_chunk_planning():
    from upp_hip.infer import plan_chunks
    assert plan_chunks(10, 32) == [(0, 10)]
    assert plan_chunks(10, 32, max_clouds=128) == [(0, 4), (4, 8), (8, 10)]
    assert plan_chunks(10, 32, max_clouds=320) == [(0, 10)]
    assert plan_chunks(10, 32, max_clouds=10_000) == [(0, 10)]
    assert plan_chunks(10, 32, max_clouds=8) == [(v, v + 1) for v in range(10)]      # at least one vote per forward
    assert plan_chunks(1, 4) == [(0, 1)]
    with pytest.raises(ValueError):
        plan_chunks(0, 4)


def test_padding_repeats_the_last_cloud():
    from upp_hip.infer import pad_batch
    x = torch.arange(3 * 5 * 3, dtype=torch.float32).view(3, 5, 3)
    y = pad_batch(x, 5)
    assert y.shape == (5, 5, 3) and torch.equal(y[:3], x) and torch.equal(y[3], x[2]) and torch.equal(y[4], x[2])
    out = torch.full((3, 5, 3), -1.0)
    assert pad_batch(x, 3, out=out) is out and torch.equal(out, x)
    lab = pad_batch(torch.tensor([7, 8]), 4)
    assert lab.tolist() == [7, 8, 8, 8]
    with pytest.raises(ValueError):
        pad_batch(x, 2)


def test_captured_protocols_refuse_what_test_vote_refuses():
    from utils import evaluate
    with pytest.raises(NotImplementedError):
        evaluate.test_vote_captured(None, [], 2048)
    with pytest.raises(NotImplementedError):
        evaluate.test_vote_captured(None, [], 1024, transform=lambda pc: pc)


def test_models_that_read_across_samples_are_recognised():
    from types import SimpleNamespace as NS
    from upp_hip.infer import mixes_samples
    assert mixes_samples(NS(config=NS(prompt_propagation_after=True, gather_idx=False)))
    assert not mixes_samples(NS(config=NS(prompt_propagation_after=True, gather_idx=True)))
    assert not mixes_samples(NS(config=NS(prompt_propagation_after=False, gather_idx=False)))
    from models import build_model_from_cfg
    from utils.config import builtin_cfg
    assert mixes_samples(build_model_from_cfg(builtin_cfg('unify_modelnet_cls').model))
