"""The query-selection kernels (csrc/query_select.hip, include/upp_hip.h "query selection") on the GPU: forward and backward bit-equal to
the torch formulation (upp_hip.torch_cpu.query_select: a stable descending argsort, gather, cat; autograd's zero-fill and scatter),
the stated order of ties and NaN, repeatability, capture into a graph, and the refusals."""
import os
import sys

import pytest
import torch

from conftest import ROOT
from upp_hip import functional as HF
from upp_hip import ops, torch_cpu

sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 0), (3, 48, 32, 64), (2, 257, 256, 0), (2, 4096, 4095, 1)]


def inputs(shape, kind, seed=0):
    B, M, Q, D = shape
    g = torch.Generator().manual_seed(100 * seed + M + Q)
    s = torch.rand(B, M, generator=g)
    if kind == "ties":                                        # a handful of levels, signed zeros among them
        s = (s * 6).floor() / 6 - 0.5
        s[s == 0.0] = torch.tensor([0.0, -0.0]).repeat(M)[: int((s == 0.0).sum())]
    elif kind == "equal":
        s = torch.full((B, M), 0.75)
    elif kind == "nan":
        s[:, ::7] = float("nan")
        s[:, 1 % M] = float("inf")
    cand, extra = torch.randn(B, M, 3, generator=g), (torch.randn(B, D, 3, generator=g) if D else None)
    return s, cand, extra, torch.randn(B, Q + D, 3, generator=g)


def both(shape, kind, seed=0):
    """the kernels on the GPU and the torch formulation on the CPU (a comparison sort: -0 equals +0, NaN above +inf) -> two lists of
    [out, order, g_cand(, g_extra)]"""
    got, want = [], []
    for fn, dev, res in ((HF.query_select, "cuda", got), (torch_cpu.query_select, "cpu", want)):
        s, cand, extra, g_out = (None if t is None else t.to(dev) for t in inputs(shape, kind, seed))
        c = cand.clone().requires_grad_()
        e = None if extra is None else extra.clone().requires_grad_()
        out, order = fn(s, c, shape[2], e)
        grads = torch.autograd.grad(out, [c] + ([e] if e is not None else []), g_out)
        res.extend([t.cpu() for t in [out.detach(), order] + list(grads)])
    return got, want


@pytest.mark.parametrize("kind", ["distinct", "ties", "equal", "nan"])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_backward_equal_the_torch_formulation(shape, kind):
    B, M, Q, D = shape
    HF._declined.clear()
    got, want = both(shape, kind)
    assert not HF._declined, HF._declined
    assert got[0].shape == (B, Q + D, 3) and got[1].shape == (B, Q) and got[1].dtype == torch.int32 and len(got) == len(want) == 3 + (D > 0)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b), i          # bits
    order = got[1].long()
    if kind == "equal":
        assert torch.equal(order, torch.arange(Q).expand(B, Q))                              # the identity
    if kind == "nan" and M > 7:
        n_nan = len(range(0, M, 7))
        lead = order[:, :min(n_nan, Q)]
        assert torch.equal(lead, torch.arange(0, M, 7)[:lead.shape[1]].expand(B, -1))          # NaN first, by index
        if Q > n_nan:
            assert (order[:, n_nan] == 1).all()                                              # then +inf
    if kind == "ties":
        s = inputs(shape, kind)[0]
        picked = torch.gather(s, 1, order)
        assert (picked[:, 1:] <= picked[:, :-1]).all()
        same = picked[:, 1:] == picked[:, :-1]                                               # (-0 == +0: one level)
        assert (order[:, 1:][same] > order[:, :-1][same]).all()
    # every unselected row of g_cand is an exact zero, every selected one its gradient
    assert (got[2] != 0).any(dim=-1).sum().item() <= B * Q


def test_two_calls_give_equal_bits_and_score_gets_no_gradient():
    shape = SHAPES[1]
    a, _ = both(shape, "ties")
    b, _ = both(shape, "ties")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    s, cand, extra, g_out = (t.cuda() for t in inputs(shape, "distinct"))
    s.requires_grad_(); cand.requires_grad_()
    out, order = HF.query_select(s, cand, shape[2], extra)
    out.backward(g_out)
    assert s.grad is None and cand.grad is not None and not order.requires_grad


def test_forward_and_backward_replay_from_a_graph():
    from memset_census import memsets_of
    shape = SHAPES[1]
    s, cand, extra, g_out = (t.cuda() for t in inputs(shape, "distinct"))
    cand.requires_grad_(); extra.requires_grad_()

    def step():
        out, order = HF.query_select(s, cand, shape[2], extra)
        return (out, order) + torch.autograd.grad(out, [cand, extra], g_out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not memsets_of(step)
    with HF.deterministic(True):
        assert not memsets_of(step)                 # deterministic already: the mode has nothing to add
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for seed, kind in ((1, "ties"), (2, "nan")):
        s2, c2, e2, g2 = inputs(shape, kind, seed)
        s.copy_(s2); cand.data.copy_(c2); extra.data.copy_(e2); g_out.copy_(g2)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static]
        want = step()
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want))


def test_refusals():
    r = lambda *sh: torch.randn(*sh, device="cuda")          # noqa: E731
    with pytest.raises(RuntimeError, match="4096"):
        ops.query_select_fwd(r(1, 4097), r(1, 4097, 3), 8)
    with pytest.raises(RuntimeError, match="4096"):
        ops.query_select_bwd(r(1, 8, 3), torch.zeros(1, 8, dtype=torch.int32, device="cuda"), 4097)
    with pytest.raises(RuntimeError, match="1 <= Q <= M"):
        ops.query_select_fwd(r(1, 8), r(1, 8, 3), 9)
    with pytest.raises(RuntimeError, match="cand"):
        ops.query_select_fwd(r(1, 8), r(1, 7, 3), 4)
    lib, p = ops._abi.load(), ops._abi.ptr
    s, c, o = r(1, 4097), r(1, 4097, 3), r(1, 8, 3)
    order = torch.zeros(1, 8, dtype=torch.int32, device="cuda")
    assert lib.upp_query_select_fwd(p(s), p(c), None, p(o), p(order), 1, 4097, 8, 0, None) == -2
    # off the served range the node declines, says so, and the torch formulation answers
    HF._declined.clear()
    out, got_order = HF.query_select(s, c, 8)
    assert HF._declined and torch.equal(got_order.long(), torch.argsort(s, dim=1, descending=True, stable=True)[:, :8])
    HF._declined.clear()
    # an index outside the cloud is dropped by the backward, never written through
    bad = torch.tensor([[0, 9, -1, 2]], dtype=torch.int32, device="cuda")
    g_cand, g_extra = ops.query_select_bwd(r(1, 4, 3), bad, 4)
    assert g_extra is None and (g_cand[0, 1] == 0).all() and (g_cand[0, 3] == 0).all() and torch.isfinite(g_cand).all()
