"""CPU tests of tests/_head_reference.py, the float64 arbiter of tests/test_gpu_head.py and tests/test_gpu_rows.py: every hand-written
gradient against torch autograd of the plain formulation in float64, to 1e-10 of each output's maximum; the BatchNorm functions against
F.batch_norm, the interpolation against upp_layers._inverse_distance_interp's torch branch.

The input generators of the two GPU files live here too, with the assertions that make every SELECTION agree between float32 and
float64 by construction: ReLU pre-activations |o| >= 1e-3, dropout uniforms |u - p| >= 1e-3 (but for one planted u == float32(p), which
is kept), the two largest entries of an arg-max column >= 1e-3 apart (but for planted bit-identical duplicates), neighbour distances
>= 1e-3 of their scale apart (but for planted exact ties on lattice coordinates i / 64, where every product is exact in float32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _head_reference as R

F32, F64 = torch.float32, torch.float64
GAP = 1e-3


def _agree(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= 1e-10 * scale, (what, float((a - b).abs().max()), scale)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ============================================================================================== generators
def top2_gap(h, dim):
    """Per slice along `dim` of a float64 tensor: (the distance from the maximum to the largest value that is not bit-equal to it (inf
    if there is none), the number of entries bit-equal to the maximum)."""
    m = h.max(dim, keepdim=True).values
    tie = h == m
    rest = torch.where(tie, torch.full_like(h, -float("inf")), h).max(dim).values
    return m.squeeze(dim) - rest, tie.sum(dim)


def cls_inputs(B, L, D, seed, kind="rand"):
    """x (B, L, D), gamma, beta, g_feat (B, 2 D) as float32 CPU tensors, and the float64 arg-max.  kinds:
         rand     random rows
         dup      rows 3, 12 and 21 of every sample bit-identical (three different waves of the kernel) and spiky in every 8th column:
                  there that row is the maximum, and the tie goes to row 3
         dup2     rows 5 and 10 likewise: the LOWER row sits in the HIGHER wave (5 and 2) -- the merge must compare rows, not waves
         const    row 2 (and row 0 of sample 0) constant 0.5: x - mean is an exact 0 in every precision, rstd = eps^-1/2, h = beta
         offset   every row 1e3 +- 1e-2; rows 1.. of a sample are bit-identical copies (a float32 LayerNorm keeps three digits of such a
                  row: a gap of 1e-3 between different rows would not survive), so the arg-max is row 1 by the tie rule
         gzero    as rand, the gradient of the [row 0] half zero in sample 0 and of the max half zero in the last sample
    The generator nudges x until the two largest DIFFERENT values of every (sample, column) are >= 1e-3 apart."""
    g = _gen(seed)
    x = torch.randn(B, L, D, generator=g) * 1.3 + 0.2
    gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    g_feat = torch.randn(B, 2 * D, generator=g)
    protected = []
    if kind == "dup":
        assert L >= 22
        x[:, 3] *= 0.1
        x[:, 3, (0 if D < 8 else 1)::8] += 4.0               # a spiky row: after the LayerNorm its spikes are the maxima of their columns
        x[:, 12], x[:, 21] = x[:, 3], x[:, 3]
        protected = [3, 12, 21]
    elif kind == "dup2":
        assert L >= 11
        x[:, 5] *= 0.1
        x[:, 5, (0 if D < 8 else 1)::8] += 4.0
        x[:, 10] = x[:, 5]
        protected = [5, 10]
    elif kind == "const":
        assert L >= 3
        x[:, 2] = 0.5
        x[0, 0] = 0.5
        protected = [2]
    elif kind == "offset":
        x = 1e3 + 1e-2 * torch.randn(B, L, D, generator=g)
        x[:, 1:] = x[:, 1:2]
    elif kind == "gzero":
        g_feat[0, :D] = 0.0
        g_feat[-1, D:] = 0.0
    eps = 1e-5
    for _ in range(40):
        h = R.layer_norm(x, gamma, beta, eps, F64)[0][:, 1:]
        gap, _n = top2_gap(h, 1)
        bad = (gap < GAP).nonzero()
        if kind == "offset" or len(bad) == 0:
            break
        am = R.first_max(h, 1) + 1
        for b, c in bad.tolist():
            t = int(am[b, c])
            if t in protected:                              # never touch a planted row: lower the runner-up instead
                hh = h[b, :, c].clone()
                hh[[p - 1 for p in protected]] = -float("inf")
                x[b, int(hh.argmax()) + 1, c] -= 0.03 * float(torch.sign(gamma[c]))
            else:
                x[b, t, c] += 0.03 * float(torch.sign(gamma[c]))
    amax = R.cls_pool_select(x, gamma, beta, eps)
    h = R.layer_norm(x, gamma, beta, eps, F64)[0][:, 1:]
    gap, ties = top2_gap(h, 1)
    assert float(gap.min()) >= GAP, float(gap.min())
    if kind == "rand" and D > 1:
        assert int(ties.max()) == 1
    if kind == "dup":
        assert int(((amax == 3) & (ties == 3)).sum()) >= 2 and not bool(((amax == 12) | (amax == 21)).any())
    if kind == "dup2":
        assert int(((amax == 5) & (ties == 2)).sum()) >= 2 and not bool((amax == 10).any())
    if kind == "offset":
        assert bool((amax == 1).all()) and bool((ties == L - 1).all())
    if kind == "const":
        hc = R.layer_norm(x, gamma, beta, eps, F32)
        assert torch.equal(hc[0][:, 2], beta.expand(B, D)) and float((hc[3][:, 2] - eps ** -0.5).abs().max()) < 1e-3 * eps ** -0.5
    return dict(x=x, gamma=gamma, beta=beta, g_feat=g_feat, eps=eps, amax=amax)


CE_KINDS = ("rand", "tie_first", "tie_second", "confident", "spread", "neginf")


def ce_inputs(B, C, seed, kind="rand", offset=0.0):
    """logits (B, C) float32, labels (B,) int64, first (B,) int64.  kinds:
         rand        randn * 3, random labels (sample 0 correct)
         tie_first   two bit-identical maxima per row, the label on the first of them (correct: torch.argmax takes the first)
         tie_second  ... the label on the second (wrong)
         confident   the label's logit + 12: every sample correct, mean loss ~ C * 1e-5 -- where a common offset costs the most
         spread      randn * 20: logits 120 apart, exp underflows to 0
         neginf      -inf in a third of the classes (never the label's)
    `offset` is added to every logit in float32 (the reference sees the rounded sums).  The two largest DIFFERENT logits of a row are
    >= 1e-3 apart (the arg-max compares the float32 inputs themselves: exact in every precision)."""
    g = _gen(seed)
    v = torch.randn(B, C, generator=g) * (20.0 if kind == "spread" else 3.0)
    labels = torch.randint(0, C, (B,), generator=g)
    if kind == "confident":
        v = v / 3.0
        v[torch.arange(B), labels] += 12.0
    if kind == "neginf" and C > 2:
        drop = torch.rand(B, C, generator=g) < 0.33
        drop[torch.arange(B), labels] = False
        drop[:, 0] = False
        v[drop] = -float("inf")
    if kind in ("tie_first", "tie_second") and C >= 2:
        top = v.max(1).values + 1.0
        for b in range(B):
            i, j = sorted(torch.randperm(C, generator=g)[:2].tolist())
            v[b, i] = v[b, j] = top[b]
            labels[b] = i if kind == "tie_first" else j
    v[0, labels[0]] = v[0].max() + (0.0 if kind.startswith("tie") else 1.0)
    v = (v + np.float32(offset)).float()
    scale = GAP
    for _ in range(20):
        gap, _n = top2_gap(v.double(), 1)
        bad = (gap < scale).nonzero().view(-1).tolist()
        if not bad:
            break
        for b in bad:
            m = v[b].max()
            v[b][v[b] == m] = m + np.float32(4 * scale)
    gap, ties = top2_gap(v.double(), 1)
    assert float(gap.min()) >= scale
    first = R.ce_select(v)
    if kind == "tie_first" and C >= 2:
        assert bool((ties == 2).all()) and bool((first == labels).all())
    if kind == "tie_second" and C >= 2:
        assert bool((ties == 2).all()) and not bool((first == labels)[1:].any())
    if kind == "confident":
        assert bool((first == labels).all())
    assert bool(torch.isfinite(v[torch.arange(B), labels]).all())
    return dict(logits=v, labels=labels, first=first)


def dropout_uniforms(shape, p, seed, plant=True):
    """Uniforms with |u - p| >= 1e-3, except the planted u[0, 0] == float32(p) (kept)."""
    p32 = np.float32(p)
    u = torch.rand(*shape, generator=_gen(seed))
    near = (u.double() - float(p32)).abs() < 1.5 * GAP
    u[near] = u[near] + 4 * GAP
    d = (u.double() - float(p32)).abs()
    if plant and p > 0:
        u.view(-1)[0] = float(p32)
        d.view(-1)[0] = 1.0
        assert R.dropout_select(u, p).reshape(-1)[0] == 1.0
    assert float(d.min()) >= GAP and float(u.max()) < 1.0
    assert np.array_equal(R.dropout_select(u, p), (u.double().numpy() >= float(p32)).astype(np.float32))
    return u


def bn_inputs(Rr, C, seed, training=True, kind="rand", slab=8):
    """z (R, C), gamma, beta, running statistics, g as float32 CPU tensors with every ReLU pre-activation |o| >= 1e-3 (float64).  kinds:
         rand      randn * 1.5 + 0.3
         offset    columns c % 4 == 1 and 3 carry an offset of 40 sigma, in columns c % 4 == 2 and 3 the first row of every `slab` rows is
                   a 30 sigma outlier (the slab statistics of bn_rows are shifted by that row), column 0 is constant 0.5 (training: an
                   exact zero variance, o = beta)
    Entries are nudged (never the constant column in training) until the assertion holds."""
    g = _gen(seed)
    z = torch.randn(Rr, C, generator=g) * 1.5 + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    beta[beta.abs() < 0.01] = 0.05
    rm, rv = 0.2 * torch.randn(C, generator=g), 0.6 + torch.rand(C, generator=g)
    gr = torch.randn(Rr, C, generator=g)
    if kind == "offset":
        z[:, 1::2] += 60.0
        z[::slab, 2::4] += 45.0
        z[::slab, 3::4] += 45.0
        z[:, 0] = 0.5
    for _ in range(40):
        o = R.batch_norm(z, gamma, beta, rm, rv, 0.0, 1e-5, training, None, None, 0.0, F64)["o"]
        bad = o.abs() < GAP
        if kind == "offset" and training:
            bad[:, 0] = False
        if not bool(bad.any()):
            break
        z[bad] += 0.05
    o = R.batch_norm(z, gamma, beta, rm, rv, 0.0, 1e-5, training, None, None, 0.0, F64)["o"]
    assert float(o.abs().min()) >= GAP, float(o.abs().min())
    return dict(z=z, gamma=gamma, beta=beta, rm=rm, rv=rv, g=gr, eps=1e-5, momentum=0.1)


def lattice_cloud(B, n, seed, span=64):
    """(B, n, 3) points on the lattice i / 64, |i| <= span: every product and sum of |a|^2 + |b|^2 - 2 a.b is exact in float32 (integers
    below 2^24 over 2^12), so float32, float64 and the kernel agree BIT FOR BIT and equal distances are exact ties."""
    return torch.randint(-span, span + 1, (B, n, 3), generator=_gen(seed)).float() / 64.0


def random_cloud(B, N, S, k, seed):
    """q (B, N, 3), src (B, S, 3) with the sorted float64 |a - b|^2 of every query >= 1e-3 of the scale max(|a|^2 + |b|^2) apart around
    the k-th rank -- positions k - 1 | k decide the LIST; inside the list an order swap of near-equal distances is within the bound."""
    g = _gen(seed)
    q, src = torch.randn(B, N, 3, generator=g), torch.randn(B, S, 3, generator=g)
    scale = float(((q ** 2).sum(-1).max() + (src ** 2).sum(-1).max()))
    if k < S:
        for _ in range(40):
            d = ((q.double().unsqueeze(2) - src.double().unsqueeze(1)) ** 2).sum(-1).sort(-1).values
            bad = ((d[..., k] - d[..., k - 1]) < GAP * scale).nonzero()
            if len(bad) == 0:
                break
            for b, n in bad.tolist():
                q[b, n] += 0.05 * torch.randn(3, generator=g)
        d = ((q.double().unsqueeze(2) - src.double().unsqueeze(1)) ** 2).sum(-1).sort(-1).values
        assert float((d[..., k] - d[..., k - 1]).min()) >= GAP * scale
    return q, src, scale


def neighbour_table(B, N, S, k, seed, ld=None, first=None):
    """A sorted neighbour table for the interpolation kernels: idx (B, N, ld) int64 with k DISTINCT sources per row (the kernels' hit
    lists hold one entry per row), dist (B, N, ld) float32 ascending, >= 0.  first: a source every row lists first.  Entries past k are
    filled with valid but unused values."""
    g = _gen(seed)
    ld = k if ld is None else ld
    assert k <= S and ld >= k
    perm = torch.stack([torch.randperm(S, generator=g) for _ in range(B * N)]).view(B, N, S)
    if first is not None:
        other = torch.where(perm == first, perm[..., :1].expand_as(perm), perm)       # swap `first` to the front
        other[..., 0] = first
        perm = other
    idx = torch.zeros(B, N, ld, dtype=torch.int64)
    idx[..., :k] = perm[..., :k]
    dist = torch.zeros(B, N, ld)
    dist[..., :k] = (torch.rand(B, N, k, generator=g) * 0.5 + 0.01).sort(-1).values
    if ld > k:
        dist[..., k:] = 7.0
    for r in idx[..., :k].reshape(-1, k).tolist()[:64]:
        assert len(set(r)) == k
    assert int(idx.min()) >= 0 and int(idx.max()) < S
    return dist, idx


def group_inputs(Rr, k, C, seed):
    """x (R, k, C) with the two largest different values of every (group, column) >= 1e-3 apart."""
    g = _gen(seed)
    x = torch.randn(Rr, k, C, generator=g)
    if k > 1:
        for _ in range(40):
            gap, _n = top2_gap(x.double(), 1)
            bad = (gap < GAP).nonzero()
            if len(bad) == 0:
                break
            am = R.first_max(x.double(), 1)
            for r, c in bad.tolist():
                x[r, int(am[r, c]), c] += 0.01
        assert float(top2_gap(x.double(), 1)[0].min()) >= GAP
    return x, torch.randn(Rr, C, generator=g)


# ============================================================================================== the reference against autograd
@pytest.mark.parametrize("kind", ["rand", "dup", "dup2", "const", "gzero"])
def test_cls_pool_reference_equals_autograd(kind):
    c = cls_inputs(2, 25, 7, 3, kind)
    x = c["x"].double().requires_grad_(True)
    h = F.layer_norm(x, (7,), c["gamma"].double(), c["beta"].double(), R.f32(c["eps"]))
    mx, am = h[:, 1:].max(1)
    feat = torch.cat([h[:, 0], mx], -1)
    (gx,) = torch.autograd.grad((feat * c["g_feat"].double()).sum(), x)
    got = R.cls_pool(c["x"], c["gamma"], c["beta"], c["eps"], c["amax"], F64, c["g_feat"])
    _agree(got["feat"], feat.detach(), "feat")
    assert torch.equal(c["amax"], am + 1), "first maximum"
    _agree(got["g_x"], gx, "g_x")
    var = c["x"].double().var(-1, unbiased=False)
    _agree(got["rstd"], (1 / torch.sqrt(var + R.f32(c["eps"]))).reshape(-1), "rstd")


def test_first_max_takes_the_first_nan_as_torch_does():
    h = torch.tensor([[1.0, 5.0, 5.0, 2.0], [1.0, float("nan"), 9.0, float("nan")], [3.0, 3.0, 3.0, 3.0]], dtype=F64)
    assert R.first_max(h, 1).tolist() == [1, 1, 0] == h.max(1).indices.tolist()


@pytest.mark.parametrize("kind", CE_KINDS)
@pytest.mark.parametrize("offset", [0.0, -30.0, 1e3])
def test_ce_reference_equals_autograd(kind, offset):
    c = ce_inputs(5, 7, 11, kind, offset)
    v = c["logits"].double().requires_grad_(True)
    loss = F.cross_entropy(v, c["labels"])
    (gv,) = torch.autograd.grad(loss, v)
    got = R.ce_acc(c["logits"], c["labels"], c["first"], F64)
    _agree(got["loss"], loss.detach(), "loss")
    _agree(got["dlogits"], gv, "dlogits")
    assert torch.equal(c["first"], c["logits"].argmax(1))
    assert got["acc"] == np.float32(float((c["logits"].argmax(1) == c["labels"]).sum()) / 5 * 100)


@pytest.mark.parametrize("C,ld,Cpad,bias", [(5, 5, 5, True), (5, 8, 7, False), (1, 3, 1, True)])
def test_logsoftmax_and_nll_reference_equal_autograd(C, ld, Cpad, bias):
    g = _gen(C + ld)
    y = torch.randn(9, ld, generator=g, dtype=F64).requires_grad_(True)
    b = torch.randn(C, generator=g, dtype=F64) if bias else None
    go = torch.randn(9, C, generator=g, dtype=F64)
    logp = F.log_softmax(y[:, :C] + (b if bias else 0.0), -1)
    (gy,) = torch.autograd.grad((logp * go).sum(), y)
    got = R.logsoftmax_rows(y.detach(), b, C, F64, go, Cpad)
    _agree(got["logp"], logp.detach(), "logp")
    _agree(got["g_y"][:, :C], gy[:, :C], "g_y")
    assert float(got["g_y"][:, C:].abs().max()) == 0.0 if Cpad > C else True
    t = torch.randint(0, C, (9,), generator=g)
    lp = logp.detach().clone().requires_grad_(True)
    loss = F.nll_loss(lp, t)
    (glp,) = torch.autograd.grad(loss * 1.7, lp)
    got = R.nll_mean(logp.detach(), t, F64, torch.tensor([1.7], dtype=F64))
    _agree(got["loss"], loss.detach(), "nll")
    _agree(got["g_logp"], glp, "g_logp")
    # a target outside [0, C): nothing added, R still divides, a zero row
    t2 = t.clone()
    t2[0], t2[4] = -1, C
    got2 = R.nll_mean(logp.detach(), t2, F64, torch.tensor([1.0], dtype=F64))
    keep = torch.ones(9, dtype=torch.bool)
    keep[0] = keep[4] = False
    _agree(got2["loss"], -(logp.detach()[keep].gather(1, t[keep].view(-1, 1)).sum() / 9), "nll, targets outside")
    assert float(got2["g_logp"][~keep].abs().max()) == 0.0


@pytest.mark.parametrize("B,P,pn", [(2, 5, 1), (3, 4, 3), (1, 2, 1)])
def test_noise_loss_reference_equals_autograd(B, P, pn):
    g = _gen(B * P + pn)
    pred = torch.randn(B, P, 3, generator=g, dtype=F64).requires_grad_(True)
    nv = torch.randn(B, P - pn, 3, generator=g, dtype=F64)
    pos = torch.mean(torch.norm(pred[:, pn:] - nv, dim=-1, keepdim=True) ** 2)
    neg = torch.mean(torch.norm(pred[:, :pn], dim=-1, keepdim=True) ** 2)
    (gp,) = torch.autograd.grad((pos + neg) * 0.7, pred)
    got = R.noise_loss(pred.detach(), nv, pn, F64, torch.tensor([0.7], dtype=F64))
    _agree(got["loss"], (pos + neg).detach(), "loss")
    _agree(got["score"], torch.norm(pred.detach(), dim=-1), "score")
    _agree(got["g_pred"], gp, "g_pred")
    p32 = pred.detach().float()
    s = R.score_f32(p32)
    assert float((s.double() - got["score"]).abs().max()) <= 2e-7 * float(got["score"].max())


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu,p,affine", [(True, 0.5, True), (True, 0.0, True), (False, 0.0, True), (False, 0.3, False)])
def test_batch_norm_reference_equals_autograd_and_f_batch_norm(training, relu, p, affine):
    c = bn_inputs(7, 5, 21, training)
    gamma, beta = (c["gamma"], c["beta"]) if affine else (None, None)
    z = c["z"].double().requires_grad_(True)
    ga = c["gamma"].double().requires_grad_(True)
    be = c["beta"].double().requires_grad_(True)
    rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
    o = F.batch_norm(z, rm, rv, ga if affine else None, be if affine else None, training, R.f32(c["momentum"]), R.f32(c["eps"]))
    u = dropout_uniforms((7, 5), p, 5) if p > 0 else None
    keep = None if u is None else torch.from_numpy(R.dropout_select(u, p)).double()
    a = F.relu(o) if relu else o
    if keep is not None:
        a = a * keep / (1.0 - R.f32(p))
    grads = torch.autograd.grad((a * c["g"].double()).sum(), [z] + ([ga, be] if affine else []))
    gate = R.bn_select(c["z"], gamma, beta, c["rm"], c["rv"], c["eps"], training) if relu else None
    if relu and affine:
        assert torch.equal(gate, (o.detach() > 0).double())
    got = R.batch_norm(c["z"], gamma, beta, c["rm"], c["rv"], c["momentum"], c["eps"], training, gate, keep, p, F64, c["g"])
    _agree(got["a"], a.detach(), "a")
    _agree(got["g_z"], grads[0], "g_z")
    if affine:
        _agree(got["g_gamma"], grads[1], "g_gamma")
        _agree(got["g_beta"], grads[2], "g_beta")
    if training:
        _agree(got["running_mean"], rm, "running_mean")
        _agree(got["running_var"], rv, "running_var")
    else:
        assert got["running_mean"] is None and torch.equal(rm, c["rm"].double())


@pytest.mark.parametrize("k,affine", [(1, False), (3, False), (4, True), (6, False)])
def test_interp_reference_equals_autograd_and_the_models_torch_branch(k, affine):
    g = _gen(40 + k)
    B, N, S, C, eps = 2, 9, 6, 5, 1e-8
    x1 = torch.randn(B, N, 3, generator=g, dtype=F64).requires_grad_(True)
    x2 = torch.randn(B, S, 3, generator=g, dtype=F64).requires_grad_(True)
    feat = torch.randn(B, S, C, generator=g, dtype=F64).requires_grad_(True)
    go = torch.randn(B, N, C, generator=g, dtype=F64)
    x3 = torch.randn(B, N, 3, generator=g, dtype=F64) if affine else None
    wt = torch.randn(3, C, generator=g, dtype=F64) if affine else None
    d_all = ((x1.unsqueeze(2) - x2.unsqueeze(1)) ** 2).sum(-1)
    dist, idx = R.topk_select(d_all, k)
    r = 1.0 / (dist + R.f32(eps))
    w = r / r.sum(-1, keepdim=True)
    nb = torch.stack([feat[b][idx[b]] for b in range(B)])
    out = (nb * w.unsqueeze(-1)).sum(2)
    if affine:
        out = out + x3 @ wt
    gf, g1, g2 = torch.autograd.grad((out * go).sum(), [feat, x1, x2])
    got = R.interp(dist.detach(), idx, feat.detach(), k, eps, F64, x3, wt, go)
    _agree(got["out"], out.detach(), "out")
    _agree(got["g_feat"], gf, "g_feat")
    geo = R.interp_geo(dist.detach(), idx, feat.detach(), go, x1.detach(), x2.detach(), k, eps, F64)
    if k == 1:                      # one neighbour: the weight is 1 whatever the geometry -- an exact 0 here, cancellation noise in autograd
        assert float(geo["g_xyz1"].abs().max()) == 0.0 == float(geo["g_xyz2"].abs().max()) and float(g1.abs().max()) < 1e-12
    else:
        _agree(geo["g_xyz1"], g1, "g_xyz1")
        _agree(geo["g_xyz2"], g2, "g_xyz2")
    if not affine:
        from models import upp_layers as L
        want = L._inverse_distance_interp(x1.detach(), x2.detach(), feat.detach(), k, R.f32(eps))
        assert float((want - got["out"]).abs().max()) <= 1e-9 * float(want.abs().max())     # (its distances take the three-term form)


def test_topk_group_max_and_posenc_references():
    q, src = lattice_cloud(2, 7, 1), lattice_cloud(2, 9, 2, span=2)                      # a coarse lattice: many exact ties
    d64, d32 = R.sqdist(q, src, F64), R.sqdist(q, src, F32)
    assert torch.equal(d64, d32.double()) and torch.equal(d64, ((q.double().unsqueeze(2) - src.double().unsqueeze(1)) ** 2).sum(-1))
    dist, idx = R.topk_select(d64, 9)
    assert bool((idx.sort(-1).values == torch.arange(9)).all())
    same = dist[..., 1:] == dist[..., :-1]
    assert bool(same.any()) and bool((idx[..., 1:] > idx[..., :-1])[same].all()), "ties go to the lowest index"
    d = torch.tensor([[3.0, float("nan"), 1.0, -float("nan"), 1.0]], dtype=F64)
    assert R.topk_select(d, 5)[1].tolist() == [[2, 4, 0, 1, 3]], "NaN last, whatever its sign"
    x, g = group_inputs(5, 4, 8, 3)
    x[0, :, 0] = torch.tensor([1.0, 2.0, 2.0, 0.0])
    x[1, :, 1] = torch.tensor([0.0, float("nan"), 9.0, float("nan")])
    am = R.group_max_select(x)
    mx, ai = x.double().max(1)
    assert torch.equal(am, ai) and am[0, 0] == 1 and am[1, 1] == 1
    xx = x.double().nan_to_num(0.0).requires_grad_(True)
    (gx,) = torch.autograd.grad((xx.gather(1, am.view(5, 1, 8)).view(5, 8) * g.double()).sum(), xx)
    _agree(R.group_max(x.nan_to_num(0.0), am, F64, g)["g_x"], gx, "group_max g_x")
    p = torch.randn(4, 3, dtype=F64)
    freqs = [1.0, 2.0, 4.0]
    want = torch.cat([p] + [t for f in freqs for t in (torch.sin(f * p), torch.cos(f * p))], -1)
    _agree(R.posenc(p, freqs, F64), want, "posenc")
    assert R.posenc(p, [], F64).shape == (4, 3)


def test_generators_hold_their_promises():
    for D, L in ((1, 2), (63, 25), (65, 130)):
        cls_inputs(3, L, D, D + L)
    cls_inputs(2, 9, 65, 4, "offset")
    for kind in CE_KINDS:
        ce_inputs(17, 40, 9, kind, 1e3)
    ce_inputs(3, 1, 1)
    c = bn_inputs(130, 65, 8, True, "offset")
    assert float(c["z"][:, 0].std()) == 0.0
    u = dropout_uniforms((7, 5), 0.5, 2)
    assert float(u[0, 0]) == 0.5
    q, src, scale = random_cloud(2, 7, 65, 5, 3)
    dist, idx = neighbour_table(2, 9, 5, 3, 1, ld=6, first=0)
    assert bool((idx[..., 0] == 0).all()) and bool((dist[..., :3].diff(dim=-1) >= 0).all())
    group_inputs(5, 9, 12, 1)


def test_bn_rows_layer_refuses_cumulative_momentum_outside_sync():
    """upp_layers._bn_rows with a momentum=None layer in training mode: ValueError on every path but synchronised BatchNorm (momentum 0
    in the average's place would freeze the running statistics silently); eval mode and a layer without running statistics are served."""
    from models import upp_layers as L
    x = torch.randn(7, 5, generator=_gen(1))
    bn = torch.nn.BatchNorm1d(5, momentum=None)
    with torch.no_grad():
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 1.5)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    for relu in (False, True):
        with pytest.raises(ValueError):
            L._bn_rows(x, bn, True, relu)
    with pytest.raises(ValueError):
        L._bn_rows(x, bn, True, drop=torch.nn.Dropout(0.5))
    assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
    want = F.batch_norm(x, rm, rv, bn.weight, bn.bias, False, 0.0, bn.eps)
    assert torch.equal(L._bn_rows(x, bn, False), want) and torch.equal(L._bn_rows(x, bn, False, relu=True), F.relu(want))
    free = torch.nn.BatchNorm1d(5, momentum=None, track_running_stats=False)
    assert torch.equal(L._bn_rows(x, free, True), F.batch_norm(x, None, None, free.weight, free.bias, True, 0.0, free.eps))
