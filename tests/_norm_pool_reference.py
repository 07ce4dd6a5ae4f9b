"""numpy restatements of csrc/norm_pool.hip (include/upp_hip.h "LayerNorm + token pooling with parameter gradients"), test-side only.

    tap_pool(f0, f1, f2, gamma, beta, eps, dt) -> x (B,G,3C), gmax (B,3C), arg (B,3C), gmean (B,3C), mean / rstd (B,G,3) in dtype dt.
        The LayerNorm here is the textbook one (its f32 bits are NOT the kernel's: the kernel's x is held to HF.layer_norm's bits by the
        tests); what this file pins is the POOLING of a given x:
    pool(x) -> gmax, arg, gmean of a given x (B,G,W), in x's dtype: arg the lowest g among equal maxima, the first NaN of a column its
        maximum; gmean the sum over g ascending, one rounded addition at a time, then one division by dtype(G).
    cls_param_grads(x, mean, rstd, amax, g_feat, dt) -> g_gamma, g_beta (D): the two sums of upp_cls_pool_bwd_ln over the rows that
        carry a gradient, (b, l) ascending.
"""
import numpy as np


def pool(x):
    B, G, W = x.shape
    best = x[:, 0].copy()
    arg = np.zeros((B, W), dtype=np.int32)
    s = x[:, 0].copy()
    for g in range(1, G):
        h = x[:, g]
        s = (s + h).astype(x.dtype)
        with np.errstate(invalid="ignore"):
            take = (h > best) | (np.isnan(h) & ~np.isnan(best))
        best = np.where(take, h, best)
        arg = np.where(take, np.int32(g), arg)
    return best, arg, (s / x.dtype.type(G)).astype(x.dtype)


def layer_norm(f, gamma, beta, eps, dt):
    f = f.astype(dt)
    mean = f.mean(-1, keepdims=True, dtype=dt)
    var = ((f - mean) ** 2).mean(-1, keepdims=True, dtype=dt)
    rstd = 1.0 / np.sqrt(var + dt(eps))
    return ((f - mean) * rstd * gamma.astype(dt) + beta.astype(dt)).astype(dt), mean[..., 0], rstd[..., 0]


def tap_pool(f0, f1, f2, gamma, beta, eps, dt=np.float64):
    parts = [layer_norm(f, gamma, beta, eps, dt) for f in (f0, f1, f2)]
    x = np.concatenate([p[0] for p in parts], axis=-1)
    gmax, arg, gmean = pool(x)
    return x, gmax, arg, gmean, np.stack([p[1] for p in parts], -1), np.stack([p[2] for p in parts], -1)


def cls_param_grads(x, mean, rstd, amax, g_feat, dt=np.float64):
    B, L, D = x.shape
    x, g_feat = x.astype(dt), g_feat.astype(dt)
    mean, rstd = mean.reshape(B, L).astype(dt), rstd.reshape(B, L).astype(dt)
    gg, gb = np.zeros(D, dt), np.zeros(D, dt)
    cols = np.arange(D)
    for b in range(B):
        for rows, g in ((np.zeros(D, np.int64), g_feat[b, :D]), (amax[b].astype(np.int64), g_feat[b, D:])):
            xh = (x[b, rows, cols] - mean[b, rows]) * rstd[b, rows]
            gg = (gg + g * xh).astype(dt)
            gb = (gb + g).astype(dt)
    return gg, gb
