"""Numpy restatements of the interpolate-max operator (include/upp_hip.h "deformable graph attention"): plain loops in np.float32, one
rounded operation per statement, so that the kernels can be compared with them bit for bit.
    forward        y_s = Bq, then fma(w3, PW[idx3], y_s) for ascending j (the fma as one float64 multiply-add rounded to f32: exact for
                   f32 operands up to double rounding, which the tests' inputs -- multiples of 2^-10 of moderate size -- cannot reach);
                   the lowest s of the maximum, a NaN never wins; lrelu
    scatter_det    the defined order of upp_interp_max_bwd_det; `reverse=True` walks the sources backwards -- the order the kernel
                   must NOT produce
    ball_offset    float64 statement of upp_deform_offset_ball_fwd"""
import numpy as np

F = np.float32


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def forward(PW, Bq, idx3, w3, slope):
    """PW (B,NK,O), Bq (B,N,O), idx3 / w3 (B, N k, 3) -> out (B,N,O) f32, arg (B,N,O) uint8, m (B,N,O) the maximum itself"""
    PW, Bq, w3 = (np.asarray(t, F) for t in (PW, Bq, w3))
    B, N, O = Bq.shape
    NK = PW.shape[1]
    k = idx3.shape[1] // N
    m = np.full((B, N, O), -np.inf, F)
    arg = np.zeros((B, N, O), np.uint8)
    for b in range(B):
        for n in range(N):
            for s in range(k):
                y = Bq[b, n].copy()
                for j in range(3):
                    i = int(idx3[b, n * k + s, j])
                    if 0 <= i < NK:
                        y = fma(w3[b, n * k + s, j], PW[b, i], y)
                win = y > m[b, n]
                m[b, n] = np.where(win, y, m[b, n])
                arg[b, n] = np.where(win, s, arg[b, n])
    with np.errstate(invalid="ignore"):
        out = np.where(m > 0, m, (m * F(slope)).astype(F)).astype(F)
    return out, arg, m


def scatter_det(g_out, out, arg, idx3, w3, slope, NK, reverse=False):
    """g_out, out (B,N,O), arg (B,N,O) as the forward saved them, idx3 / w3 (B, N k, 3) -> d_Bq (B,N,O), d_PW (B,NK,O): g = g_out *
    (out > 0 ? 1 : slope); every target starts at +0.0f and takes w3 * g of every source (n, j) with idx3[b, n k + arg, j] == target, in
    ascending 3 n + j, one rounded addition each; an index outside [0, NK) is skipped."""
    g_out, out, w3 = (np.asarray(t, F) for t in (g_out, out, w3))
    B, N, O = g_out.shape
    k = idx3.shape[1] // N
    g = (g_out * np.where(out > 0, F(1), F(slope)).astype(F)).astype(F)
    d_PW = np.zeros((B, NK, O), F)
    order = range(3 * N - 1, -1, -1) if reverse else range(3 * N)
    ch = np.arange(O)
    for b in range(B):
        for src in order:
            n, j = src // 3, src % 3
            slot = n * k + np.minimum(arg[b, n].astype(np.int64), k - 1)           # (O,): the arg is per channel
            r = idx3[b, slot, j].astype(np.int64)
            ok = (r >= 0) & (r < NK)
            t = (w3[b, slot, j] * g[b, n]).astype(F)
            d_PW[b, r[ok], ch[ok]] = (d_PW[b, r[ok], ch[ok]] + t[ok]).astype(F)
    return g, d_PW


def ball_offset(A, Bq, idx, pos, gamma, beta, eps, W3):
    """float64: shift (B,G,N k,3) = pos[idx] + tanh(W3 gelu(LayerNorm(A[idx] + Bq))) * 0.5 (max_s pos[idx] - min_s pos[idx])"""
    from math import erf
    A, Bq, pos, gamma, beta, W3 = (np.asarray(t, np.float64) for t in (A, Bq, pos, gamma, beta, W3))
    B, G, NK, C = A.shape
    N, k = idx.shape[1], idx.shape[2]
    verf = np.vectorize(erf)
    out = np.empty((B, G, N * k, 3))
    for b in range(B):
        local = pos[b][idx[b]]                                                      # (N,k,3)
        half = 0.5 * (local.max(1) - local.min(1))                                 # (N,3)
        for g in range(G):
            y = A[b, g][idx[b]] + Bq[b, g][:, None, :]                              # (N,k,C)
            mu = y.mean(-1, keepdims=True)
            z = (y - mu) / np.sqrt(((y - mu) ** 2).mean(-1, keepdims=True) + eps) * gamma + beta
            h = 0.5 * z * (1.0 + verf(z / np.sqrt(2.0)))
            out[b, g] = (local + np.tanh(h @ W3.T) * half[:, None, :]).reshape(N * k, 3)
    return out
