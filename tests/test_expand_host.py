"""The broadcast-expand entry points (csrc/expand.hip, include/upp_hip.h "broadcast expand") on a GPU-less host: they are declared,
exported and bound; the library refuses every bad argument before any launch (null DEVICE pointers: a launch would fault); and the
torch formulation that serves CPU tensors matches the numpy restatement."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _expand_reference as XR
from conftest import ROOT
from upp_hip import _abi, torch_cpu
from upp_hip import functional as HF

P = ctypes.c_void_p(64)          # a non-null pointer: every call below must be refused before anything reads it
NAMES = ("upp_expand_work_floats", "upp_expand_fwd", "upp_expand_bwd")


def _fwd(lib, P_=P, U=P, per_row=1, Wu=P, gamma=P, beta=P, eps=1e-5, slope=0.2, mode=1, h=P, mean=P, var=P, rstd=P, work=P, R=8, S=16, O=32,
         J=3):
    return lib.upp_expand_fwd(P_, U, per_row, Wu, gamma, beta, eps, slope, mode, h, mean, var, rstd, work, R, S, O, J, None)


def _bwd(lib, g_h=P, P_=P, U=P, per_row=1, Wu=P, gamma=P, beta=P, mean=P, rstd=P, slope=0.2, mode=1, g_P=P, g_U=P, g_Wu=P, g_gamma=P, g_beta=P,
         work=P, R=8, S=16, O=32, J=3):
    return lib.upp_expand_bwd(g_h, P_, U, per_row, Wu, gamma, beta, mean, rstd, slope, mode, g_P, g_U, g_Wu, g_gamma, g_beta, work,
                              R, S, O, J, None)


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "upp_hip.h")).read()
    assert "broadcast expand" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _abi.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert re.search(r" T %s$" % n, exported, flags=re.M), n
        assert n in _abi.SIGNATURES and hasattr(lib, n), n
    assert lib.upp_abi_version() == 5 == _abi.ABI_VERSION
    assert re.search(r"UPP_OPT_COUNT = 4\b", hdr) and len(_abi.OPTIONS) == 4
    assert lib.upp_get_option(3) >= 0 and lib.upp_get_option(4) == -1                # four options, no fifth


def test_work_floats():
    lib = _abi.load()
    for args in ((0, 4, 8), (4, 0, 8), (4, 4, 0), (-1, 4, 8), (4, -3, 8), (4, 4, -8)):
        assert lib.upp_expand_work_floats(*args) == 0, args
    # max(1, 256 / S) whole rows per block; per block 2 O statistics floats + 4 O of the g_Wu partials; 2 O for m1, m2
    for R, S, O in ((130, 4, 128), (7, 64, 256), (2, 224, 1024), (1, 1, 1), (5, 300, 20)):
        rows = max(1, 256 // S)
        blocks = -(-R // rows)
        assert lib.upp_expand_work_floats(R, S, O) == blocks * O * 6 + 2 * O, (R, S, O)


def test_the_library_refuses_bad_arguments_before_any_launch():
    lib = _abi.load()
    BADARG, RANGE = -1, -2
    for call in (_fwd, _bwd):
        for name in ("P_", "U", "Wu", "gamma", "beta", "mean", "rstd"):
            assert call(lib, **{name: None}) == BADARG, (call.__name__, name)
        assert call(lib, J=0) == BADARG and call(lib, J=5) == RANGE
        assert call(lib, O=0) == BADARG and call(lib, O=1025) == RANGE
        assert call(lib, R=0) == BADARG and call(lib, S=0) == BADARG and call(lib, R=-1) == BADARG and call(lib, S=-4) == BADARG
        assert call(lib, R=2 ** 16, S=2 ** 10, O=32) == RANGE                       # R S O = 2^31
        assert call(lib, R=2 ** 30, S=2 ** 30, O=1024) == RANGE                     # (the product does not fit 64 bits)
        for slope in (-0.01, 1.01, float("nan"), float("inf")):
            assert call(lib, slope=slope) == BADARG, slope
        assert call(lib, mode=3) == BADARG and call(lib, mode=-1) == BADARG
    assert _fwd(lib, h=None) == BADARG and _fwd(lib, eps=-1.0) == BADARG and _fwd(lib, eps=float("nan")) == BADARG
    assert _fwd(lib, var=None) == BADARG and _fwd(lib, work=None) == BADARG          # mode 1 writes both
    for name in ("g_h", "g_P", "g_Wu", "g_gamma", "g_beta", "work"):
        assert _bwd(lib, **{name: None}) == BADARG, name
    assert _bwd(lib, per_row=0) == BADARG                                            # g_U of a shared U
    # without a norm the norm's operands may be absent -- the size checks still come first
    none = dict(gamma=None, beta=None, mean=None, rstd=None, mode=0)
    assert _fwd(lib, J=5, var=None, work=None, **none) == RANGE and _fwd(lib, O=1025, var=None, work=None, **none) == RANGE
    assert _bwd(lib, O=1025, g_gamma=None, g_beta=None, **none) == RANGE and _bwd(lib, J=0, g_gamma=None, g_beta=None, **none) == BADARG


CPU_CASES = [(1, 1, 1, 1, False), (5, 9, 20, 2, False), (7, 16, 24, 3, True), (3, 5, 8, 4, True)]


def _cpu_inputs(case):
    R, S, O, J, per_row = case
    g = torch.Generator().manual_seed(R + 10 * S + 100 * O + J)
    return (torch.randn(R, O, generator=g), torch.randn((R, S, J) if per_row else (S, J), generator=g), torch.randn(O, J, generator=g),
            1 + 0.5 * torch.randn(O, generator=g), 0.3 * torch.randn(O, generator=g))


@pytest.mark.parametrize("case", CPU_CASES)
def test_torch_formulation_matches_the_restatement(case):
    """No norm: the restatement has the KERNEL's bits (fma chain); torch's small product may round differently, by a few f32 roundings
    of terms of size |U||Wu| -> 1e-6 of the output's scale.  With a norm: float64 against float64, 1e-12."""
    R, S, O, J, per_row = case
    P_, U, Wu, gamma, beta = _cpu_inputs(case)
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    try:
        for slope in (0.0, 0.2):
            got = HF.expand_act(P_, U, Wu, None, slope).numpy()
            want = XR.forward(P_.numpy(), U.numpy(), Wu.numpy(), slope)
            assert got.shape == (R, S, O) and got.dtype == np.float32
            assert np.abs(got.astype(np.float64) - want).max() <= 1e-6 * max(np.abs(want).max(), 1e-30), slope
        if R * S > 1:
            bn = torch.nn.BatchNorm1d(O).double()
            with torch.no_grad():
                bn.weight.copy_(gamma); bn.bias.copy_(beta)
                bn.running_mean.normal_(generator=torch.Generator().manual_seed(1)); bn.running_var.uniform_(0.5, 2.0)
            rm, rv = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
            ops64 = [t.double() for t in (P_, U, Wu)]
            for train in (True, False):
                bn.train(train)
                got = HF.expand_act(*ops64, bn, 0.2).detach().numpy()
                want, mean, rstd, y = XR.forward_f64(P_.numpy(), U.numpy(), Wu.numpy(), gamma.numpy(), beta.numpy(), bn.eps, 0.2,
                                                     None if train else rm, None if train else rv)
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), train
                if train:                          # torch's own update: momentum 0.1, the unbiased variance
                    n = R * S
                    assert np.allclose(bn.running_mean.numpy(), 0.9 * rm + 0.1 * mean, rtol=1e-12, atol=1e-14)
                    assert np.allclose(bn.running_var.numpy(), 0.9 * rv + 0.1 * y.var(axis=(0, 1)) * n / (n - 1), rtol=1e-12, atol=1e-14)
                    rm, rv = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    finally:
        torch_cpu.enable(was)


def test_cpu_tensors_are_served_only_by_the_opt_in_torch_formulation():
    P_, U, Wu, _, _ = _cpu_inputs(CPU_CASES[1])
    was = torch_cpu.enabled()
    try:
        torch_cpu.enable(False)
        with pytest.raises(RuntimeError, match="no CPU path"):
            HF.expand_act(P_, U, Wu)
        torch_cpu.enable(True)
        with pytest.raises(ValueError, match="slope"):
            HF.expand_act(P_, U, Wu, None, 1.5)
        with pytest.raises(ValueError, match="shared U"):
            HF.expand_act(P_, U.clone().requires_grad_(), Wu)
        with pytest.raises(ValueError, match="BatchNorm1d"):
            HF.expand_act(P_, U, Wu, torch.nn.BatchNorm1d(20, affine=False))
        with pytest.raises(ValueError, match="more than 1 value"):
            HF.expand_act(torch.randn(1, 4), torch.randn(1, 2), torch.randn(4, 2), torch.nn.BatchNorm1d(4))
        assert not HF.expand_usable(P_, U, Wu)                      # CPU tensors: the kernels do not serve them
    finally:
        torch_cpu.enable(was)
