"""CPU tests of tests/_tail_reference.py, the float64 arbiter of tests/test_gpu_tail.py: against torch autograd of the plain formulation
(torch.cat for the row maps, F.layer_norm, F.linear, F.gelu, explicit masks; float64 on both sides), for every row map, with and without
each optional input, to 1e-10 of each output's maximum; plus the selection rules and a case small enough to check by hand."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _tail_reference as R

MODES = (R.IDENTITY, R.INSERT_CLS, R.INSERT, R.STRIP_CLS, R.STRIP)


def _agree(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= 1e-10 * scale, (what, float((a - b).abs().max()), scale)


def _plain_rows(x, add, prompts, y, ybias, scale_b, mode, P):
    """The row map by torch.cat / slicing; scale_b (B,) is the drop-path factor as a tensor."""
    B = x.shape[0]
    v = x if add is None else x + add
    if y is not None:
        v = v + scale_b.view(B, 1, 1) * (y if ybias is None else y + ybias)
    pr = None if prompts is None else prompts.unsqueeze(0).expand(B, -1, -1)
    if mode == R.INSERT_CLS:
        return v if P == 0 else torch.cat([v[:, :1], pr, v[:, 1:]], dim=1)
    if mode == R.INSERT:
        return v if P == 0 else torch.cat([pr, v], dim=1)
    if mode == R.STRIP_CLS:
        return torch.cat([v[:, :1], v[:, 1 + P:]], dim=1)
    if mode == R.STRIP:
        return v[:, P:]
    return v


def _scale(u, keep, B):
    if u is None:
        return torch.ones(B, dtype=torch.float64)
    return torch.from_numpy(R.drop_select(u.numpy(), keep)).double() / R.f32(keep)


def _inputs(B, Lin, D, P, mode, g):
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    c = dict(x=rnd(B, Lin, D), add=rnd(B, Lin, D), y=rnd(B, Lin, D), ybias=rnd(D), gamma=1 + 0.2 * rnd(D), beta=0.2 * rnd(D),
             prompts=rnd(P, D) if (P > 0 and mode in (R.INSERT_CLS, R.INSERT)) else None)
    c['u'] = torch.rand(B, generator=g).float()
    c['u'][0], c['u'][-1] = 0.05, 0.95                     # keep = 0.7: one sample dropped for certain, one kept for certain
    return c


@pytest.mark.parametrize("has_add,has_y,has_ybias,has_u,has_ln", [o for o in itertools.product([False, True], repeat=5)
                                                                  if (o[1] or not (o[2] or o[3]))])
@pytest.mark.parametrize("mode,P", [(m, P) for m in MODES for P in (0, 1, 3)])
def test_row_reference_equals_autograd_of_the_plain_formulation(mode, P, has_add, has_y, has_ybias, has_u, has_ln):
    g = torch.Generator().manual_seed(17 * mode + P)
    B, Lin, D, keep, eps = 3, 5, 7, 0.7, 1e-5
    c = _inputs(B, Lin, D, P, mode, g)
    Lo = R.lout(mode, Lin, P)
    add, y = (c['add'] if has_add else None), (c['y'] if has_y else None)
    ybias, u = (c['ybias'] if has_ybias else None), (c['u'] if has_u else None)
    gamma, beta = (c['gamma'], c['beta']) if has_ln else (None, None)
    g_xo, g_h = torch.randn(B, Lo, D, generator=g, dtype=torch.float64), torch.randn(B, Lo, D, generator=g, dtype=torch.float64)
    got = R.rowln(c['x'], add, c['prompts'], y, ybias, u, keep, gamma, beta, eps, mode, P, g_xo, g_h if has_ln else None, torch.float64)

    leaves = {k: v.clone().requires_grad_(True) for k, v in dict(x=c['x'], add=add, y=y, prompts=c['prompts'], gamma=gamma, beta=beta).items()
              if v is not None}
    rows = _plain_rows(leaves['x'], leaves.get('add'), leaves.get('prompts'), leaves.get('y'), ybias, _scale(u, keep, B), mode, P)
    loss = (rows * g_xo).sum()
    _agree(got['xo'], rows.detach(), "rows")
    if has_ln:
        h = F.layer_norm(rows, (D,), leaves['gamma'], leaves['beta'], eps)
        loss = loss + (h * g_h).sum()
        _agree(got['h'], h.detach(), "h")
        _agree(got['mean'], rows.detach().mean(-1), "mean")
        _agree(got['rstd'], 1 / torch.sqrt(rows.detach().var(-1, unbiased=False) + eps), "rstd")
    names = list(leaves)
    want = dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names])))
    _agree(got['g_x'], want['x'], "g_x")
    if has_add:
        _agree(got['g_x'], want['add'], "g_add")
    if has_y:
        _agree(got['g_y'], want['y'], "g_y")
    else:
        assert got['g_y'] is None
    if c['prompts'] is not None:
        _agree(got['g_prompt'], want['prompts'], "g_prompt")
        _agree(got['g_prompt_b'].sum(0), want['prompts'], "per-sample prompt gradient")
    if has_ln:
        _agree(got['g_gamma'], want['gamma'], "g_gamma")
        _agree(got['g_beta'], want['beta'], "g_beta")
    if mode in (R.STRIP_CLS, R.STRIP) and P > 0:               # the dropped rows: exact zeros
        dropped = slice(1, 1 + P) if mode == R.STRIP_CLS else slice(0, P)
        assert float(got['g_x'][:, dropped].abs().max()) == 0.0 and (not has_y or float(got['g_y'][:, dropped].abs().max()) == 0.0)
    if has_y and has_u:                                         # sample 0 is dropped: its residual gradient is an exact zero
        assert float(got['g_y'][0].abs().max()) == 0.0


def _adapter_inputs(Rr, D, g, w1_scale=1.0):
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    return dict(W1=w1_scale * rnd(R.H, D) / D ** 0.5, b1=0.1 * rnd(R.H), W2=rnd(D, R.H) / R.H ** 0.5, b2=0.1 * rnd(D))


@pytest.mark.parametrize("p,with_ud", [(0.0, False), (0.0, True), (0.1, True)])
@pytest.mark.parametrize("s", [0.7, 1.0])
def test_adapter_reference_equals_autograd_of_the_plain_formulation(s, p, with_ud):
    g = torch.Generator().manual_seed(int(10 * s) + int(10 * p))
    Rr, D = 9, 12
    w = _adapter_inputs(Rr, D, g, w1_scale=6.0)                # |s1| into GELU's tails
    ha, x, g_out = (torch.randn(Rr, D, generator=g, dtype=torch.float64) for _ in range(3))
    ud = torch.rand(Rr, R.H, generator=g).float() if with_ud else None
    got = R.adapter(ha, x, w['W1'], w['b1'], w['W2'], w['b2'], ud, p, s, g_out, torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (ha, x, w['W1'], w['b1'], w['W2'], w['b2'])]
    m = 1.0 if ud is None else torch.from_numpy(R.dropout_select(ud.numpy(), p)).double() / (1 - R.f32(p))
    s1 = F.linear(leaves[0], leaves[2], leaves[3])
    out = leaves[1] + R.f32(s) * F.linear(F.gelu(s1) * m, leaves[4], leaves[5])
    want = torch.autograd.grad((out * g_out).sum(), leaves)
    assert float(s1.detach().abs().max()) > 4.0
    _agree(got['out'], out.detach(), "out")
    _agree(got['s1'], s1.detach(), "s1")
    for k, w_ in zip(("g_ha", "g_x", "g_W1", "g_b1", "g_W2", "g_b2"), want):
        _agree(got[k], w_, k)
    # the factors give the weight gradients by themselves (adapter_wgrad_batched's contraction)
    _agree(got['ga'].t() @ ha, want[2], "ga^T ha")
    _agree(g_out.t() @ got['d'], want[4], "g_out^T d")


@pytest.mark.parametrize("has_y,has_ybias,has_u,with_ud", [(False, False, False, False), (True, False, False, True), (True, True, False, False),
                                                           (True, True, True, True), (True, False, True, False)])
@pytest.mark.parametrize("mode,P", [(R.IDENTITY, 0), (R.STRIP_CLS, 2), (R.STRIP, 2), (R.STRIP_CLS, 0)])
def test_tail_reference_equals_autograd_of_the_plain_formulation(mode, P, has_y, has_ybias, has_u, with_ud):
    g = torch.Generator().manual_seed(5 + mode + P)
    B, Lin, D, keep, eps, s, p = 3, 6, 12, 0.7, 1e-6, 0.7, 0.1
    c = _inputs(B, Lin, D, P, mode, g)
    w = _adapter_inputs(B * Lin, D, g)
    Lo = R.lout(mode, Lin, P)
    y, ybias, u = (c['y'] if has_y else None), (c['ybias'] if has_ybias else None), (c['u'] if has_u else None)
    ud = torch.rand(B * Lo, R.H, generator=g).float() if with_ud else None
    g_out = torch.randn(B, Lo, D, generator=g, dtype=torch.float64)
    got = R.tail(c['x'], y, ybias, u, keep, mode, P, c['gamma'], c['beta'], eps, w['W1'], w['b1'], w['W2'], w['b2'], ud, p, s, g_out,
                 torch.float64)
    leaves = {k: v.clone().requires_grad_(True) for k, v in dict(x=c['x'], y=y, gamma=c['gamma'], beta=c['beta'], **w).items() if v is not None}
    rows = _plain_rows(leaves['x'], None, None, leaves.get('y'), ybias, _scale(u, keep, B), mode, P)
    ha = F.layer_norm(rows, (D,), leaves['gamma'], leaves['beta'], eps)
    m = 1.0 if ud is None else (torch.from_numpy(R.dropout_select(ud.numpy(), p)).double() / (1 - R.f32(p))).view(B, Lo, R.H)
    s1 = F.linear(ha, leaves['W1'], leaves['b1'])
    out = rows + R.f32(s) * F.linear(F.gelu(s1) * m, leaves['W2'], leaves['b2'])
    names = list(leaves)
    want = dict(zip(names, torch.autograd.grad((out * g_out).sum(), [leaves[k] for k in names])))
    _agree(got['out'], out.detach(), "out")
    _agree(got['xo'], rows.detach(), "xo")
    _agree(got['s1'], s1.detach().view(-1, R.H), "s1")
    for k in names:
        _agree(got['g_' + k], want[k], "g_" + k)
    assert has_y or got['g_y'] is None
    ha_d = ha.detach().view(-1, D)
    _agree(got['fac'][:, :R.H].t() @ ha_d, want['W1'], "fac: ga^T ha")
    _agree(g_out.view(-1, D).t() @ got['fac'][:, R.H:], want['W2'], "fac: g_out^T d")


def test_selection_rules_are_taken_in_float32():
    # keep = 0.7 as a float32 is 0.699999988...: u = 0.3 (float32 0.300000012) gives keep + u = 1 in float32 arithmetic -> kept
    assert R.drop_select(np.array([0.3, 0.29, 0.31], dtype=np.float32), 0.7).tolist() == [1.0, 0.0, 1.0]
    assert R.f32(0.7) != 0.7 and R.f32(0.1) != 0.1
    # ud == float32(p) keeps the element; the next float32 below drops it
    p32 = np.float32(0.1)
    ud = np.array([p32, np.nextafter(p32, np.float32(0)), 0.0, 1.0], dtype=np.float32)
    assert R.dropout_select(ud, 0.1).tolist() == [1.0, 0.0, 0.0, 1.0]
    assert R.dropout_select(np.array([0.0], dtype=np.float32), 0.0).tolist() == [1.0]           # p = 0 with uniforms: everything kept
    m = R.dropout_mask(torch.from_numpy(ud), 0.1, torch.float64, 'cpu')
    assert m.tolist() == [1 / (1 - float(p32)), 0.0, 0.0, 1 / (1 - float(p32))]
    f = R.drop_factor(torch.tensor([0.05, 0.95]), 0.7, 2, torch.float64, 'cpu')
    assert f.tolist() == [0.0, 1 / float(np.float32(0.7))]


def test_row_maps_and_one_row_by_hand():
    assert R.row_sources(R.INSERT_CLS, 2, 5) == ([0, 3, 4], [0, 1, 2], [1, 2], [0, 1])
    assert R.row_sources(R.INSERT, 2, 4) == ([2, 3], [0, 1], [0, 1], [0, 1])
    assert R.row_sources(R.STRIP_CLS, 2, 3) == ([0, 1, 2], [0, 3, 4], [], [])
    assert R.row_sources(R.STRIP, 2, 2) == ([0, 1], [2, 3], [], [])
    assert R.row_sources(R.STRIP_CLS, 4, 1) == ([0], [0], [], [])          # Lout = 1: only the cls row is left
    # one row (1, 3): mean 2, variance 2/3 -> rstd = sqrt(1.5) at eps = 0, h = +-sqrt(1.5), 0
    x = torch.tensor([[[1.0, 2.0, 3.0]]], dtype=torch.float64)
    one, zero = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    r = R.rowln(x, None, None, None, None, None, 1.0, one, zero, 0.0, R.IDENTITY, 0, None, torch.ones_like(x), torch.float64)
    assert float(r['mean']) == 2.0 and abs(float(r['rstd']) - 1.5 ** 0.5) < 1e-15
    assert torch.allclose(r['h'], torch.tensor([[[-1.5 ** 0.5, 0.0, 1.5 ** 0.5]]], dtype=torch.float64), rtol=1e-15, atol=0)
    # a constant gradient of the LayerNorm output has no gradient in the row: dy - mean(dy) = 0 and mean(dy xhat) = 0
    assert float(r['g_x'].abs().max()) < 1e-15 and torch.equal(r['g_beta'], torch.ones(3, dtype=torch.float64))
    # a constant row: variance 0, rstd = eps^-1/2, h = beta
    r = R.rowln(torch.full((1, 1, 3), 4.0, dtype=torch.float64), None, None, None, None, None, 1.0, one, one * 0.25, 1e-6, R.IDENTITY, 0,
                None, None, torch.float64)
    assert abs(float(r['rstd']) - 1e3) < 1e-9 and torch.equal(r['h'], torch.full((1, 1, 3), 0.25, dtype=torch.float64))
    # GELU and its derivative at 0 and in the tails
    v = torch.tensor([0.0, 8.0, -8.0], dtype=torch.float64)
    assert R.gelu(v)[0] == 0 and abs(float(R.gelu(v)[1]) - 8.0) < 1e-13 and abs(float(R.gelu(v)[2])) < 1e-13
    assert float(R.gelu_grad(v)[0]) == 0.5 and abs(float(R.gelu_grad(v)[1]) - 1.0) < 1e-12 and abs(float(R.gelu_grad(v)[2])) < 1e-12
