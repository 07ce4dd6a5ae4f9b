"""Plain numpy / torch reference of the prompt-propagation step at LIST level: it takes exactly what the kernels of csrc/prop.hip take
(absolute row lists, neighbour lists and weights, drop-path uniforms, BatchNorm parameters and statistics) and uses none of the project's
kernels.  One function evaluates the formulation in any dtype on any device, so the same code is the float64 arbiter and the float32
yardstick of tests/test_gpu_prop.py; tests/test_prop_host.py checks it against Block._propagate_prompts on the CPU.

    f      = 1 + (floor(keep + u) / keep  if u is given else 1)                 per group (x + drop_path(x))
    v      = X[i1] * f                                                           (groups, 8, D)
    pooled = v[arg-max] + sum_k v / 8                                            the arg-max is an INPUT (first maximum)
    lc     = BatchNorm1d(pooled) over the `groups` rows
    out    = X, its last T rows of every sample += 0.3 * sum_k w8 * (lc + 0.3 * X[i2])[idx8]
"""
import numpy as np
import torch

NB = 8          # neighbours per level-2 group and per interpolation


def keep32(keep):
    """`keep` as the kernels receive it (a C float), as a Python float."""
    return float(np.float32(keep))


def drop_scale(u, keep):
    """floor(keep + u) in float32, the kernel's arithmetic: a SELECTION (0 or 1 per group), shared by every dtype like the arg-max."""
    return np.floor(np.float32(keep) + np.asarray(u, dtype=np.float32)).astype(np.float32)


def factors(u, keep, groups, dtype, device):
    """f (groups,) in `dtype`."""
    if u is None:
        return torch.full((groups,), 2.0, dtype=dtype, device=device)
    s = torch.from_numpy(drop_scale(u.detach().cpu().numpy(), keep)).to(device=device, dtype=dtype)
    return 1.0 + s / keep32(keep)


def amax_emulate(X, i1, u, keep):
    """The kernel's arg-max, exactly: float32 X[i1] * float32(f), first maximum.  The build uses -ffp-contract=off and the kernel compares
    the rounded product.  X: (rows, D) or (B, Lp, D) float32 array; i1 (groups*8) -> (groups, D) uint8."""
    X = np.asarray(X, dtype=np.float32).reshape(-1, np.shape(X)[-1])
    i1 = np.asarray(i1).reshape(-1, NB)
    if u is None:
        f = np.full((i1.shape[0],), 2.0, dtype=np.float32)
    else:
        f = (np.float32(1.0) + drop_scale(u, keep) / np.float32(keep)).astype(np.float32)
    v = X[i1] * f[:, None, None]
    assert v.dtype == np.float32
    v = np.where(np.isnan(v), -np.inf, v)                 # `v > max` is false for a NaN: the kernel never selects one
    return np.argmax(v, axis=1).astype(np.uint8)          # numpy: the first occurrence of the maximum


def argmax_first(X, i1, f):
    """First arg-max of X[i1] * f in X's own dtype (torch), (groups, D) int64."""
    v = X.reshape(-1, X.shape[-1])[i1.long().view(-1, NB)] * f.view(-1, 1, 1)
    mx = v.max(dim=1, keepdim=True)[0]
    k = torch.arange(NB, device=X.device).view(1, NB, 1).expand_as(v)
    return torch.where(v == mx, k, torch.full_like(k, NB)).min(dim=1)[0]


def pool(X, i1, f, amax):
    """-> pooled (groups, D)."""
    v = X.reshape(-1, X.shape[-1])[i1.long().view(-1, NB)] * f.view(-1, 1, 1)
    return v.gather(1, amax.long().unsqueeze(1)).squeeze(1) + v.sum(dim=1) / 8


def batchnorm(pooled, gamma, beta, running_mean, running_var, momentum, eps, training):
    """-> (lc, mean, rstd, new running_mean, new running_var); nothing is updated in place.  Batch statistics: biased variance for the
    normalisation, unbiased (n - 1, or 1 for a single row) for the running update; eval: the running statistics."""
    n = pooled.shape[0]
    if training:
        mean = pooled.mean(dim=0)
        m2 = ((pooled - mean) ** 2).sum(dim=0)
        var = m2 / n
        new_rm, new_rv = running_mean, running_var
        if running_mean is not None:
            new_rm = (1 - momentum) * running_mean + momentum * mean.detach()
            new_rv = (1 - momentum) * running_var + momentum * (m2.detach() / max(n - 1, 1))
    else:
        mean, var, new_rm, new_rv = running_mean, running_var, running_mean, running_var
    rstd = 1.0 / torch.sqrt(var + eps)
    return (pooled - mean) * rstd * gamma + beta, mean, rstd, new_rm, new_rv


def interpolate(X, lc, i2, idx8, w8):
    """X (B, Lp, D), lc (B*G2, D), i2 (B*G2) absolute rows, idx8 / w8 (B, T, 8) -> out (B, Lp, D)."""
    B, Lp, D = X.shape
    T = idx8.shape[1]
    G2 = lc.shape[0] // B
    c2 = (lc + 0.3 * X.reshape(-1, D)[i2.long()]).view(B, G2, D)
    j = idx8.long().reshape(B, T * NB, 1).expand(-1, -1, D)
    nb = torch.gather(c2, 1, j).view(B, T, NB, D)
    add = 0.3 * (w8.unsqueeze(-1) * nb).sum(dim=2)
    return torch.cat([X[:, :Lp - T], X[:, Lp - T:] + add], dim=1)


def step(X, i1, i2, idx8, w8, u, keep, gamma, beta, running_mean, running_var, momentum, eps, training, amax=None):
    """The whole step in X's dtype.  -> dict(out, pooled, lc, mean, rstd, running_mean, running_var, amax)."""
    groups = i2.numel()
    f = factors(u, keep, groups, X.dtype, X.device)
    if amax is None:
        amax = argmax_first(X.detach(), i1, f)
    pooled = pool(X, i1, f, amax)
    lc, mean, rstd, rm, rv = batchnorm(pooled, gamma, beta, running_mean, running_var, momentum, eps, training)
    out = interpolate(X, lc, i2, idx8, w8)
    return dict(out=out, pooled=pooled, lc=lc, mean=mean, rstd=rstd, running_mean=rm, running_var=rv, amax=amax)


def step_with_grads(X, i1, i2, idx8, w8, u, keep, gamma, beta, running_mean, running_var, momentum, eps, training, amax, wgt, dtype,
                    device=None):
    """step() in `dtype` with the gradients of sum(out * wgt) by torch autograd.  Tensors are converted; the lists are kept.
    -> dict of DETACHED float64 tensors: out, pooled, mean, rstd, running_mean, running_var, g_X, g_gamma, g_beta, g_w8."""
    device = device or X.device
    cv = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype)          # noqa: E731
    x, g, b, w = (cv(t).clone().requires_grad_(True) for t in (X, gamma, beta, w8))
    mv = lambda t: t.to(device)                                                              # noqa: E731
    r = step(x, mv(i1), mv(i2), mv(idx8), w, u, keep, g, b, cv(running_mean), cv(running_var), momentum, eps, training, mv(amax))
    grads = torch.autograd.grad((r['out'] * cv(wgt)).sum(), [x, g, b, w], allow_unused=True)
    res = {k: r[k] for k in ('out', 'pooled', 'mean', 'rstd', 'running_mean', 'running_var')}
    res.update(g_X=grads[0], g_gamma=grads[1], g_beta=grads[2], g_w8=grads[3])
    return {k: (None if v is None else v.detach().double()) for k, v in res.items()}


# ---------------------------------------------------------------------------------------------- the index builder
def square_distance(a, b):
    """The reference's three-term form, (B,N,3) x (B,M,3) -> (B,N,M): dist = -2 a.b; dist += |a|^2; dist += |b|^2."""
    d = -2 * (a.unsqueeze(2) * b.unsqueeze(1)).sum(-1)
    d = d + (a ** 2).sum(-1).unsqueeze(-1)
    return d + (b ** 2).sum(-1).unsqueeze(1)


def weights(c1, c2, idx8, eps):
    """w8(c1, c2 | idx8) = (1 / (d + eps)) / sum_k, differentiable in the centres."""
    recip = 1.0 / (square_distance(c1, c2).gather(-1, idx8.long()) + eps)
    return recip / recip.sum(dim=-1, keepdim=True)


def row_maps(i1, i2, gather_idx, B, G2, Lp, off):
    """Absolute rows of the (B*Lp)-row token matrix for the reference's index tensors (integers, numpy int64), both conventions as
    upp_layers._prop_lists_torch states them: per-sample indices behind `off` leading rows (gather_idx), or flat indices into the
    (B*G)-row view of the tokens without those rows, G = Lp - off."""
    i1 = np.asarray(i1, dtype=np.int64).reshape(B, -1)
    i2 = np.asarray(i2, dtype=np.int64).reshape(B, -1)
    if gather_idx:
        base = (np.arange(B, dtype=np.int64) * Lp + off).reshape(B, 1)
        return (base + i1).reshape(-1), (base + i2).reshape(-1)
    G = Lp - off
    return ((i1 // G) * Lp + off + i1 % G).reshape(-1), ((i2 // G) * Lp + off + i2 % G).reshape(-1)


def distances64(c1, c2):
    """|a - b|^2 in float64 from float arrays (B,T,3), (B,G2,3) -> (B,T,G2)."""
    a, b = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
    return ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)


def lattice(shape, rng):
    """Coordinates k * 0.25, integer k in [-4, 4]: every product and sum of the kernel's distance formula is exact in float32, so
    distances, their order and their ties are determined without any tolerance."""
    return (rng.integers(-4, 5, size=shape) * 0.25).astype(np.float32)


def neighbour_order(c1, c2, k=NB):
    """(B,T,k) nearest level-2 centres ascending by (distance, index) -- for lattice inputs, where float64 distances are exact."""
    return np.argsort(distances64(c1, c2), axis=-1, kind='stable')[:, :, :k]
