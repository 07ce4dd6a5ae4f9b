"""CPU tests of tests/_prop_reference.py, the float64 arbiter of tests/test_gpu_prop.py: against Block._propagate_prompts (the reference
model's torch formulation, float64 on both sides), on cases small enough to check by hand, and on its tie rules."""
import numpy as np
import pytest
import torch

import _prop_reference as R
from models import upp_layers as L


def _agree(a, b, what):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= 1e-10 * scale, (what, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("training,u_given", [(True, False), (True, True), (False, False)])      # (drop-path is the identity in eval mode)
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("is_cls", [True, False])
def test_list_level_reference_equals_the_blocks_torch_formulation(is_cls, gather, training, u_given):
    torch.manual_seed(3 + is_cls + 2 * gather)
    B, T, G2, D, P = 3, 12, 9, 12, 4
    off = 1 if is_cls else 0
    Lp, G = T + P + off, T + P
    keep = 0.7
    blk = L.Block(D, 2, drop_path=(1 - keep) if u_given else 0.0).double().train(training)
    with torch.no_grad():
        blk.bnorm.weight.copy_(torch.linspace(0.5, 1.5, D)); blk.bnorm.bias.copy_(torch.linspace(-0.2, 0.2, D))
        blk.bnorm.running_mean.copy_(torch.linspace(-0.1, 0.4, D)); blk.bnorm.running_var.copy_(torch.linspace(0.6, 1.7, D))
    rm0, rv0 = blk.bnorm.running_mean.clone(), blk.bnorm.running_var.clone()
    X = (torch.randn(B, Lp, D, dtype=torch.float64) * 0.7 + 0.3)
    wgt = torch.linspace(-1, 1, X.numel(), dtype=torch.float64).view_as(X)
    c1 = torch.rand(B, T, 3, dtype=torch.float64) * 2 - 1
    if gather:                                            # per-sample rows of the cls-stripped tokens
        i1 = torch.randint(0, G, (B, G2, 8))
        i2 = torch.randint(0, G, (B, G2))
        pick = torch.stack([torch.randperm(T)[:G2] for _ in range(B)])
    else:                                                 # flat, batch offsets b*T, read in the (B*G)-row view (stride T into stride G)
        pick = torch.stack([torch.randperm(T)[:G2] for _ in range(B)])
        i1 = (torch.randint(0, T, (B, G2, 8)) + torch.arange(B).view(B, 1, 1) * T).reshape(B * G2, 8)
        i2 = (pick + torch.arange(B).view(B, 1) * T).reshape(-1)
    u = torch.rand(B * G2) if u_given else None
    if u_given:
        u[0], u[1] = 0.05, 0.95                           # one group dropped for certain, one kept for certain
        scale = torch.from_numpy(R.drop_scale(u.numpy(), keep)).double().view(-1, 1, 1) / R.keep32(keep)
        blk.drop_path.sample_scale = lambda branch: scale

    a = c1.clone().requires_grad_(True)
    b = torch.gather(a, 1, pick.unsqueeze(-1).expand(-1, -1, 3)) * 1.0
    x = X.clone().requires_grad_(True)
    kw = dict(center1=a, center1_idx=i1, center2=b, center2_idx=i2, gather_idx=gather, classification=is_cls)
    out = blk._propagate_prompts(x, kw)[0]
    want = [out.detach()] + list(torch.autograd.grad((out * wgt).sum(), [x, a, blk.bnorm.weight, blk.bnorm.bias]))
    want_rm, want_rv = blk.bnorm.running_mean.clone(), blk.bnorm.running_var.clone()

    # the same step from the lists
    with torch.no_grad():
        i1a, i2a, idx8, _ = L._prop_lists_torch(c1, b.detach(), i1, i2, gather, B, Lp, off)
    m1, m2 = R.row_maps(i1.numpy(), i2.numpy(), gather, B, G2, Lp, off)
    assert np.array_equal(m1, i1a.numpy()) and np.array_equal(m2, i2a.numpy())
    a2 = c1.clone().requires_grad_(True)
    b2 = torch.gather(a2, 1, pick.unsqueeze(-1).expand(-1, -1, 3)) * 1.0
    x2 = X.clone().requires_grad_(True)
    gamma, beta = blk.bnorm.weight.detach().clone().requires_grad_(True), blk.bnorm.bias.detach().clone().requires_grad_(True)
    w8 = R.weights(a2, b2, idx8, 1e-3)
    r = R.step(x2, i1a, i2a, idx8, w8, u, keep, gamma, beta, rm0, rv0, blk.bnorm.momentum, blk.bnorm.eps, training)
    got = [r['out'].detach()] + list(torch.autograd.grad((r['out'] * wgt).sum(), [x2, a2, gamma, beta]))
    for name, g_, w_ in zip(("tokens", "g_tokens", "g_centres", "g_bn_weight", "g_bn_bias"), got, want):
        _agree(g_, w_, name)
    assert float(want[2].abs().max()) > 1e-6
    _agree(r['running_mean'], want_rm, "running_mean")
    _agree(r['running_var'], want_rv, "running_var")
    if training:
        assert not torch.equal(want_rm, rm0)
    else:
        assert torch.equal(want_rm, rm0) and torch.equal(r['running_var'], rv0)


def test_one_group_one_column_by_hand():
    # rows 0..7 hold 1..8, one group lists them all, f = 2: v = 2..16, max 16 (k = 7), sum 72 -> pooled = 16 + 9 = 25
    X = torch.arange(1, 9, dtype=torch.float64).view(1, 8, 1)
    i1 = torch.arange(8)
    i2 = torch.tensor([2])                                 # the centre's own token: X = 3
    idx8 = torch.zeros(1, 8, 8, dtype=torch.long)
    w8 = torch.full((1, 8, 8), 0.125, dtype=torch.float64)
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    ev = R.step(X, i1, i2, idx8, w8, None, 1.0, 2 * one, one, 5 * one, 4 * one - 1e-5, 0.1, 1e-5, False)
    assert float(ev['pooled']) == 25.0 and int(ev['amax']) == 7
    # eval: lc = (25 - 5) / 2 * 2 + 1 = 21; c2 = 21 + 0.9 = 21.9; every token += 0.3 * 21.9
    assert torch.allclose(ev['out'], X + 0.3 * 21.9, rtol=1e-14, atol=0)
    tr = R.step(X, i1, i2, idx8, w8, None, 1.0, 2 * one, one, 5 * one, 4 * one, 0.1, 1e-5, True)
    # one row: mean 25, variance 0, lc = beta = 1; running: 0.9 * 5 + 0.1 * 25 = 7, 0.9 * 4 + 0.1 * 0 = 3.6
    assert float(tr['mean']) == 25.0 and abs(float(tr['rstd']) - 1e-5 ** -0.5) < 1e-9
    assert torch.allclose(tr['out'], X + 0.3 * (1 + 0.9), rtol=1e-14, atol=0)
    assert abs(float(tr['running_mean']) - 7.0) < 1e-14 and abs(float(tr['running_var']) - 3.6) < 1e-14
    # drop-path: u = 0.05, keep = 0.5 -> floor(0.55) = 0 -> f = 1: pooled = 8 + 36 / 8 = 12.5; u = 0.6 -> f = 1 + 1 / 0.5 = 3
    assert float(R.step(X, i1, i2, idx8, w8, torch.tensor([0.05]), 0.5, one, zero, zero, one, 0.1, 1e-5, False)['pooled']) == 12.5
    assert float(R.step(X, i1, i2, idx8, w8, torch.tensor([0.6]), 0.5, one, zero, zero, one, 0.1, 1e-5, False)['pooled']) == 37.5
    # only the last T rows move; gradient of sum(out) w.r.t. X through the identity path alone is 1 for the rows above them
    Xg = torch.arange(1, 11, dtype=torch.float64).view(1, 10, 1).requires_grad_(True)
    o = R.step(Xg, i1 + 2, i2 + 2, idx8, w8, None, 1.0, one, zero, zero, one, 0.1, 0.0, False)['out']
    assert torch.equal(o[0, :2].detach(), Xg[0, :2].detach())
    g = torch.autograd.grad(o.sum(), Xg)[0].view(-1)
    # eval, gamma = rstd = 1: d pooled / d X[r] = 2 * (1/8 + [r is the arg-max]); 8 tokens * 0.3 * (sum_k w8 = 1) reach the one centre
    base = 8 * 0.3 * 2 * 0.125
    want = torch.tensor([1, 1] + [1 + base] * 7 + [1 + base + 8 * 0.3 * 2], dtype=torch.float64)
    want[4] += 8 * 0.3 * 0.3                                # the centre's own token (row 2 + 2)
    assert torch.allclose(g, want, rtol=1e-14, atol=0)


def test_tie_rules_first_maximum_and_lowest_index():
    X = np.zeros((8, 3), dtype=np.float32)
    X[[2, 5], 0] = 7.0                                      # two equal maxima: k = 2 wins
    X[:, 1] = -1.0                                          # all equal: k = 0
    X[7, 2] = 1.0
    i1 = np.arange(8)
    assert R.amax_emulate(X, i1, None, 1.0).tolist() == [[2, 0, 7]]
    f = torch.full((1,), 2.0, dtype=torch.float64)
    assert R.argmax_first(torch.from_numpy(X).double(), torch.from_numpy(i1), f).tolist() == [[2, 0, 7]]
    # coincident level-2 centres: equal distances keep their index order
    c1 = np.zeros((1, 1, 3), dtype=np.float32)
    c2 = np.zeros((1, 10, 3), dtype=np.float32)
    c2[0, :, 0] = [0.5, 0.25, 0.5, 0.25, 0, 0.5, 1, 1, 0, 0.75]
    assert R.neighbour_order(c1, c2)[0, 0].tolist() == [4, 8, 1, 3, 0, 2, 5, 9]


def test_argmax_emulator_equals_the_float64_argmax_without_ties():
    rng = np.random.default_rng(11)
    rows, D, groups = 40, 65, 23
    X = rng.standard_normal((rows, D)).astype(np.float32)
    i1 = np.stack([rng.permutation(rows)[:8] for _ in range(groups)]).reshape(-1)        # distinct rows per group: no ties (continuous data)
    u = rng.random(groups).astype(np.float32)
    for uu, keep in ((None, 1.0), (u, 0.9)):
        em = R.amax_emulate(X, i1, uu, keep)
        f = R.factors(None if uu is None else torch.from_numpy(uu), keep, groups, torch.float64, 'cpu')
        ex = R.argmax_first(torch.from_numpy(X).double(), torch.from_numpy(i1), f)
        assert np.array_equal(em, ex.numpy().astype(np.uint8))


def test_row_maps_read_stride_T_indices_in_the_stride_G_view():
    # B = 2, T = 64, P = 10, cls: flat index 64 + 3 (sample 1, centre 3) lands in sample 0's view row 67 -> absolute row 0 * 75 + 1 + 67
    m1, m2 = R.row_maps(np.array([[0] * 8, [67] * 8]), np.array([[5], [64 + 73]]), False, 2, 1, 75, 1)
    assert m1[0] == 1 and m1[8] == 68 and m2.tolist() == [6, 75 + 1 + 63]
    m1, m2 = R.row_maps(np.array([[0] * 8, [67] * 8]), np.array([[5], [73]]), True, 2, 1, 75, 1)
    assert m1[0] == 1 and m1[8] == 75 + 68 and m2.tolist() == [6, 75 + 74]
