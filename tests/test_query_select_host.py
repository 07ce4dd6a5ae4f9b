"""The query selection on a GPU-less host: the torch formulation (upp_hip.torch_cpu.query_select) against numpy's stable argsort -- ties,
a NaN score, Q = M -- its gradients, and the argument checks of the entry points, which happen before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from upp_hip import _abi, functional as HF, ops, torch_cpu


def numpy_select(score, cand, Q, extra=None):
    """descending, equal scores by ascending index, NaN first: numpy's stable argsort of the negated scores with NaN as -inf"""
    key = np.where(np.isnan(score), -np.inf, -score.astype(np.float64))
    order = np.argsort(key, axis=1, kind="stable")[:, :Q]
    out = np.take_along_axis(cand, order[:, :, None], axis=1)
    return (out if extra is None else np.concatenate([out, extra], axis=1)), order


def scores(kind, B, M, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(B, M, generator=g)
    if kind == "equal":
        s = torch.full((B, M), 0.25)
    elif kind == "ties":
        s = (s * 4).floor() / 4
    elif kind == "nan":
        s[:, M // 2] = float("nan")
    return s


@pytest.mark.parametrize("kind", ["distinct", "equal", "ties", "nan"])
@pytest.mark.parametrize("B, M, Q, D", [(1, 1, 1, 0), (3, 48, 32, 64), (2, 9, 9, 2)])
def test_formulation_against_numpys_stable_argsort(kind, B, M, Q, D):
    g = torch.Generator().manual_seed(3)
    s, cand = scores(kind, B, M), torch.randn(B, M, 3, generator=g)
    extra = torch.randn(B, D, 3, generator=g) if D else None
    out, order = torch_cpu.query_select(s, cand, Q, extra)
    want, want_order = numpy_select(s.numpy(), cand.numpy(), Q, None if extra is None else extra.numpy())
    assert out.shape == (B, Q + D, 3) and order.shape == (B, Q) and order.dtype == torch.int32
    assert np.array_equal(order.numpy(), want_order) and np.array_equal(out.numpy(), want)
    if kind == "equal":
        assert np.array_equal(order.numpy(), np.broadcast_to(np.arange(Q), (B, Q)))          # the identity
    if kind == "nan" and M > 1:
        assert (order[:, 0] == M // 2).all()                                                 # NaN ranks as the largest
    if Q == M:
        assert np.array_equal(np.sort(order.numpy(), axis=1), np.broadcast_to(np.arange(M), (B, M)))


def test_gradients_and_the_cpu_switch():
    g = torch.Generator().manual_seed(4)
    s = scores("ties", 2, 12).requires_grad_()
    cand, extra = torch.randn(2, 12, 3, generator=g, requires_grad=True), torch.randn(2, 5, 3, generator=g, requires_grad=True)
    g_out = torch.randn(2, 7 + 5, 3, generator=g)
    was = torch_cpu.enabled()
    try:
        torch_cpu.enable(True)
        out, order = HF.query_select(s, cand, 7, extra)
        out.backward(g_out)
        assert s.grad is None and not order.requires_grad
        want = torch.zeros(2, 12, 3)
        for b in range(2):
            want[b, order[b].long()] = g_out[b, :7]
        assert torch.equal(cand.grad, want) and torch.equal(extra.grad, g_out[:, 7:])
        with pytest.raises(ValueError, match="1 <= Q <= M"):
            HF.query_select(s, cand, 13)
        with pytest.raises(ValueError, match="1 <= Q <= M"):
            HF.query_select(s, cand, 0)
        torch_cpu.enable(False)
        with pytest.raises(RuntimeError, match="no CPU path"):
            HF.query_select(s, cand, 7, extra)
    finally:
        torch_cpu.enable(was)
    assert not HF.query_select_usable(s, cand, 7)             # CPU tensors are not the kernel's
    assert ops.query_select_usable(4096, 4096) and not ops.query_select_usable(4097, 1) and not ops.query_select_usable(8, 9)


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _abi.load()
    x = ctypes.c_void_p(16)                                   # a non-null pointer that is never followed: every call below is refused
    fwd, bwd = lib.upp_query_select_fwd, lib.upp_query_select_bwd
    assert fwd(None, x, None, x, x, 2, 8, 4, 0, None) == -1 and fwd(x, None, None, x, x, 2, 8, 4, 0, None) == -1
    assert fwd(x, x, None, None, x, 2, 8, 4, 0, None) == -1 and fwd(x, x, None, x, None, 2, 8, 4, 0, None) == -1
    assert fwd(x, x, None, x, x, 2, 8, 4, 1, None) == -1                     # D > 0 without extra
    assert fwd(x, x, None, x, x, 0, 8, 4, 0, None) == -1 and fwd(x, x, None, x, x, 2, 8, 0, 0, None) == -1
    assert fwd(x, x, None, x, x, 2, 8, 4, -1, None) == -1
    assert fwd(x, x, None, x, x, 2, 4097, 4, 0, None) == -2 and fwd(x, x, None, x, x, 2, 8, 9, 0, None) == -2
    assert bwd(None, x, x, None, 2, 8, 4, 0, None) == -1 and bwd(x, None, x, None, 2, 8, 4, 0, None) == -1
    assert bwd(x, x, None, None, 2, 8, 4, 0, None) == -1 and bwd(x, x, x, None, 2, 8, 4, 3, None) == -1
    assert bwd(x, x, x, None, 2, 4097, 4, 0, None) == -2 and bwd(x, x, x, None, 2, 8, 9, 0, None) == -2
