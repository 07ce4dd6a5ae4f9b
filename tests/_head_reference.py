"""Plain torch reference of the head, loss and per-point row operators of csrc/head.hip and csrc/pointwise.hip, forward AND backward, with
the gradients written out -- no autograd, none of the project's kernels.  One set of functions evaluates a formulation in any dtype on
any device, so the same code is the float64 arbiter and the float32 yardstick of tests/test_gpu_head.py and tests/test_gpu_rows.py;
tests/test_head_host.py checks every hand-written gradient against torch autograd of the plain formulation on the CPU.

    cls_pool      feat = [LN(x)[:, 0] | LN(x)[b, amax[b, c], c]],  amax = first maximum over rows 1.. (the first NaN, if there is one)
    ce_acc        loss = mean_b -log_softmax(v_b)[y_b], acc = 100 * #{first arg-max == y} / B, dlogits = (softmax - onehot) / B
    logsoftmax    logp = log_softmax(y[:, :C] + bias);  g_y = [g - exp(logp) * sum_c g | 0 in the pad columns]
    nll_mean      loss = -mean_r logp[r, t_r];  a target outside [0, C) adds nothing to the sum (R still divides) and gets a zero row
    noise_loss    mean |pred_noise - nv|^2 + mean |pred_pure|^2 (means over points), score = |pred|
    batch_norm    o = (z - mean) * rstd * gamma + beta (+ ReLU gate) (* keep / (1 - p)); biased variance for o, unbiased for the running update
    interp        out = sum_j w_j feat[idx_j], w_j = r_j / sum_l r_l, r_j = 1 / (d_j + eps)  (+ x3 . wt);  gradients to feat and to both geometries
    sqdist_topk   the k smallest |a|^2 + |b|^2 - 2 a.b by ascending (d, index), NaN last
    group_max     max over the k rows of a group with the first arg-max (the first NaN, if there is one)
    posenc        [x | sin(f_0 x) | cos(f_0 x) | sin(f_1 x) | ...]

SELECTIONS -- arg-max rows, ReLU gates, dropout keeps, neighbour lists -- are taken once, in float64 (the *_select functions), and handed
to both precisions; scalars (eps, p, momentum) enter the arithmetic as the float32 values the kernels receive.
"""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64


def f32(v):
    """A scalar as the kernels receive it (a C float), as a Python float."""
    return float(np.float32(v))


def _t(x, dt):
    return None if x is None else x.to(dt)


def first_max(h, dim):
    """Index of the first maximum of h along `dim`; a NaN is the maximum and the first NaN wins (torch.max(dim) on either device)."""
    key = torch.where(torch.isnan(h), torch.full_like(h, float("inf")), h)
    nan_any = torch.isnan(h).any(dim, keepdim=True)
    hit = torch.where(nan_any, torch.isnan(h), key == key.max(dim, keepdim=True).values)
    n = h.shape[dim]
    shape = [1] * h.dim()
    shape[dim] = n
    ar = torch.arange(n, device=h.device).view(shape).expand_as(h)
    return torch.where(hit, ar, torch.full_like(ar, n)).min(dim).values


# ---------------------------------------------------------------------------------------------- cls_pool
def layer_norm(x, gamma, beta, eps, dt):
    """-> (h, xhat, mean (...,), rstd (...,)) over the last dim; biased variance about the mean."""
    x = x.to(dt)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    xh = (x - mean) * rstd
    return xh * gamma.to(dt) + beta.to(dt), xh, mean.squeeze(-1), rstd.squeeze(-1)


def cls_pool_select(x, gamma, beta, eps):
    """amax (B, D) int64 in [1, L): the first maximal row among rows 1.. of the float64 LayerNorm."""
    h = layer_norm(x, gamma, beta, eps, F64)[0]
    return first_max(h[:, 1:], 1) + 1


def cls_pool(x, gamma, beta, eps, amax, dt, g_feat=None):
    B, L, D = x.shape
    h, xh, mean, rstd = layer_norm(x, gamma, beta, eps, dt)
    feat = torch.cat([h[:, 0], h.gather(1, amax.view(B, 1, D)).view(B, D)], -1)
    res = dict(feat=feat, mean=mean.reshape(-1), rstd=rstd.reshape(-1), g_x=None)
    if g_feat is not None:
        g = g_feat.to(dt)
        g_h = torch.zeros(B, L, D, dtype=dt, device=x.device)
        g_h[:, 0] = g[:, :D]
        g_h.scatter_add_(1, amax.view(B, 1, D), g[:, D:].reshape(B, 1, D))
        dy = g_h * gamma.to(dt)
        res["g_x"] = rstd.unsqueeze(-1) * (dy - dy.mean(-1, keepdim=True) - xh * (dy * xh).mean(-1, keepdim=True))
    return res


# ---------------------------------------------------------------------------------------------- ce_acc
def ce_select(logits):
    """first (B,) int64: the first class holding the row maximum (torch.argmax)."""
    return first_max(logits.to(F64), 1)


def ce_acc(logits, labels, first, dt):
    """-> loss (), acc (float32 scalar: the correctly rounded percentage), dlogits (B, C).  Labels inside [0, C)."""
    v = logits.to(dt)
    B, C = v.shape
    mx = v.max(1, keepdim=True).values
    logp = (v - mx) - torch.log(torch.exp(v - mx).sum(1, keepdim=True))
    onehot = torch.zeros_like(v).scatter_(1, labels.view(B, 1), 1.0)
    loss = -(logp.gather(1, labels.view(B, 1))).sum() / B
    count = int((first == labels).sum())
    return dict(loss=loss, acc=np.float32(count / B * 100), dlogits=(torch.exp(logp) - onehot) / B)


# ---------------------------------------------------------------------------------------------- log-softmax rows / NLL
def logsoftmax_rows(y, bias, C, dt, g=None, Cpad=None):
    """y (R, >= C): logp (R, C) = log_softmax(y[:, :C] + bias); g_y (R, Cpad) with exact zeros in the pad columns."""
    x = y[:, :C].to(dt)
    if bias is not None:
        x = x + bias.to(dt)
    mx = x.max(1, keepdim=True).values
    logp = (x - mx) - torch.log(torch.exp(x - mx).sum(1, keepdim=True))
    res = dict(logp=logp, g_y=None)
    if g is not None:
        g = g.to(dt)
        core = g - torch.exp(logp) * g.sum(1, keepdim=True)
        res["g_y"] = torch.cat([core, torch.zeros(core.shape[0], Cpad - C, dtype=dt, device=core.device)], 1)
    return res


def nll_mean(logp, target, dt, g_loss=None):
    """-> loss (), g_logp (R, C).  A target outside [0, C) contributes 0 to the sum -- R still divides -- and a zero gradient row."""
    lp = logp.to(dt)
    R, C = lp.shape
    ok = (target >= 0) & (target < C)
    t = torch.where(ok, target, torch.zeros_like(target)).view(R, 1)
    picked = torch.where(ok, lp.gather(1, t).view(R), torch.zeros(R, dtype=dt, device=lp.device))
    res = dict(loss=-(picked.sum() / R), g_logp=None)
    if g_loss is not None:
        onehot = torch.zeros_like(lp).scatter_(1, t, 1.0) * ok.view(R, 1).to(dt)
        res["g_logp"] = onehot * (-(g_loss.to(dt).reshape(()) / R))
    return res


# ---------------------------------------------------------------------------------------------- noise loss
def noise_loss(pred, nv, pn, dt, g_loss=None):
    """pred (B, P, 3) = [pn shape points | P - pn noise points], nv (B, P - pn, 3)."""
    p, q = pred.to(dt), nv.to(dt)
    B, P, _ = p.shape
    d_noise = p[:, pn:] - q
    loss = (d_noise ** 2).sum() / (B * (P - pn)) + (p[:, :pn] ** 2).sum() / (B * pn)
    res = dict(loss=loss, score=torch.sqrt((p ** 2).sum(-1)), g_pred=None)
    if g_loss is not None:
        g = g_loss.to(dt).reshape(())
        res["g_pred"] = torch.cat([p[:, :pn] * (2.0 * g / (B * pn)), d_noise * (2.0 * g / (B * (P - pn)))], 1)
    return res


def score_f32(pred):
    """The score as the kernels form it: float32 sqrt of fma(z, z, fma(x, x, y * y)) -- numpy float64 emulates each fused step exactly
    (the product of two float32 values is exact in float64; one rounding to float32 per step)."""
    p = pred.detach().cpu().numpy().astype(np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    t = (y * y).astype(np.float32).astype(np.float64)
    t = (x * x + t).astype(np.float32).astype(np.float64)
    t = (z * z + t).astype(np.float32)
    return torch.from_numpy(np.sqrt(t))


# ---------------------------------------------------------------------------------------------- BatchNorm over rows
def dropout_select(u, p):
    """u >= p on the float32 values (1 keeps the element; u == float32(p) keeps it); None without uniforms."""
    if u is None:
        return None
    return (u.detach().cpu().numpy().astype(np.float32) >= np.float32(p)).astype(np.float32)


def bn_select(z, gamma, beta, rm, rv, eps, training):
    """The ReLU gate o > 0 of the float64 BatchNorm output, as a 0 / 1 float64 tensor on z's device."""
    return (batch_norm(z, gamma, beta, rm, rv, 0.0, eps, training, None, None, 0.0, F64)["o"] > 0).to(F64)


def batch_norm(z, gamma, beta, rm, rv, momentum, eps, training, gate, keep, p, dt, g=None, want_gz=True):
    """z (R, C).  gate: 0 / 1 (R, C) or None (no ReLU); keep: 0 / 1 (R, C) or None (no dropout), kept values scaled by 1 / (1 - p).
    -> a, o (before gate and dropout), mean, rstd, running_mean, running_var (None where there are no running buffers), g_z, g_gamma, g_beta."""
    x = z.to(dt)
    R, C = x.shape
    ga = torch.ones(C, dtype=dt, device=x.device) if gamma is None else gamma.to(dt)
    be = torch.zeros(C, dtype=dt, device=x.device) if beta is None else beta.to(dt)
    new_rm = new_rv = None
    if training:
        mean = x.mean(0)
        m2 = ((x - mean) ** 2).sum(0)
        rstd = 1.0 / torch.sqrt(m2 / R + f32(eps))
        if rm is not None:
            m = f32(momentum)
            new_rm = (1.0 - m) * rm.to(dt) + m * mean
            new_rv = (1.0 - m) * rv.to(dt) + m * (m2 / (R - 1 if R > 1 else 1))
    else:
        mean, rstd = rm.to(dt), 1.0 / torch.sqrt(rv.to(dt) + f32(eps))
    xh = (x - mean) * rstd
    o = xh * ga + be
    f = torch.ones_like(o)
    if gate is not None:
        f = f * gate.to(device=x.device, dtype=dt)
    if keep is not None:
        f = f * keep.to(device=x.device, dtype=dt) / (1.0 - f32(p))
    res = dict(a=o * f, o=o, mean=mean, rstd=rstd, running_mean=new_rm, running_var=new_rv, g_z=None, g_gamma=None, g_beta=None)
    if g is not None:
        d = g.to(dt) * f
        gb, gg = d.sum(0), (d * xh).sum(0)
        res["g_beta"], res["g_gamma"] = gb, gg
        if want_gz:
            res["g_z"] = ga * rstd * (d - gb / R - xh * gg / R) if training else ga * rstd * d
    return res


# ---------------------------------------------------------------------------------------------- interpolation
def interp_weights(dist, k, eps, dt):
    r = 1.0 / (dist[..., :k].to(dt) + f32(eps))
    return r / r.sum(-1, keepdim=True), r


def _rows_of(idx, k, S):
    """Flat source rows (B N k,) of a (B, N, >= k) table into a (B S, ...) matrix."""
    B = idx.shape[0]
    return (idx[..., :k] + (torch.arange(B, device=idx.device) * S).view(B, 1, 1)).reshape(-1)


def interp(dist, idx, feat, k, eps, dt, x3=None, wt=None, g_out=None):
    """dist / idx (B, N, >= k), feat (B, S, C) -> out (B, N, C) (+ x3 (B, N, 3) . wt (3, C)); g_feat (B, S, C) of g_out (B, N, C)."""
    B, S, C = feat.shape
    N = dist.shape[1]
    w, _ = interp_weights(dist, k, eps, dt)
    rows = _rows_of(idx, k, S)
    nb = feat.to(dt).reshape(B * S, C)[rows].view(B, N, k, C)
    out = (nb * w.unsqueeze(-1)).sum(2)
    if x3 is not None:
        out = out + x3.to(dt) @ wt.to(dt)
    res = dict(out=out, g_feat=None)
    if g_out is not None:
        contrib = (g_out.to(dt).unsqueeze(2) * w.unsqueeze(-1)).reshape(B * N * k, C)
        res["g_feat"] = torch.zeros(B * S, C, dtype=dt, device=feat.device).index_add_(0, rows, contrib).view(B, S, C)
    return res


def interp_geo(dist, idx, feat, g_out, xyz1, xyz2, k, eps, dt):
    """Gradients of interp's output w.r.t. the geometry behind d_j = |x1 - x2_j|^2 (the table's d enters the weights as it stands):
    g_w_j = <g_out, feat_j>, g_r_j = (g_w_j - sum_l g_w_l w_l) / sum_l r_l, g_d_j = -g_r_j r_j^2,
    g_x1 = sum_j 2 g_d_j (x1 - x2_j), g_x2[idx_j] -= 2 g_d_j (x1 - x2_j).  -> g_xyz1 (B, N, 3), g_xyz2 (B, S, 3)."""
    B, S, C = feat.shape
    N = dist.shape[1]
    w, r = interp_weights(dist, k, eps, dt)
    rows = _rows_of(idx, k, S)
    nb = feat.to(dt).reshape(B * S, C)[rows].view(B, N, k, C)
    gw = (nb * g_out.to(dt).unsqueeze(2)).sum(-1)
    mix = (gw * w).sum(-1, keepdim=True)
    gd2 = -2.0 * ((gw - mix) / r.sum(-1, keepdim=True)) * r * r
    diff = xyz1.to(dt).unsqueeze(2) - xyz2.to(dt).reshape(B * S, 3)[rows].view(B, N, k, 3)
    c = diff * gd2.unsqueeze(-1)
    g2 = torch.zeros(B * S, 3, dtype=dt, device=feat.device).index_add_(0, rows, -c.reshape(-1, 3)).view(B, S, 3)
    return dict(g_xyz1=c.sum(2), g_xyz2=g2)


# ---------------------------------------------------------------------------------------------- k nearest by the three-term distance
def sqdist(q, src, dt):
    """|a|^2 + |b|^2 - 2 a.b (B, N, S), the reference's square_distance, in dt."""
    a, b = q.to(dt), src.to(dt)
    d = -2.0 * (a @ b.transpose(1, 2))
    d = d + (a ** 2).sum(-1).unsqueeze(-1)
    return d + (b ** 2).sum(-1).unsqueeze(1)


def topk_select(d, k):
    """The k smallest of every row of d by ascending (d, index), NaN last (torch's stable sort) -> (dist (..., k), idx (..., k) int64)."""
    nan = torch.isnan(d)
    i1 = torch.sort(torch.where(nan, torch.full_like(d, float("inf")), d), dim=-1, stable=True).indices
    i2 = torch.sort(nan.gather(-1, i1).to(torch.int8), dim=-1, stable=True).indices        # (a device sort ranks a NaN by its sign bit: not here)
    i = i1.gather(-1, i2)[..., :k]
    return d.gather(-1, i), i


# ---------------------------------------------------------------------------------------------- group max, positional encoding
def group_max_select(x):
    """amax (R, C) int64: the first maximal row of every (group, column) of x (R, k, C)."""
    return first_max(x.to(F64), 1)


def group_max(x, amax, dt, g=None):
    R, k, C = x.shape
    out = x.to(dt).gather(1, amax.view(R, 1, C)).view(R, C)
    res = dict(out=out, g_x=None)
    if g is not None:
        res["g_x"] = torch.zeros(R, k, C, dtype=dt, device=x.device).scatter_(1, amax.view(R, 1, C), g.to(dt).view(R, 1, C))
    return res


def posenc(x, freqs, dt):
    """x (..., 3) -> (..., 3 (2 F + 1)); every frequency enters as its float32 value."""
    v = x.to(dt)
    cols = [v]
    for f in freqs:
        cols += [torch.sin(f32(f) * v), torch.cos(f32(f) * v)]
    return torch.cat(cols, -1)
