"""Numpy restatement of the defined summation order of upp_deform_attn_bwd_det (include/upp_hip.h "deformable local cross-attention"):
plain loops in np.float32, one rounded operation per statement, so that the kernel can be compared with it bit for bit.  `reverse=True`
walks the sources backwards -- the order the kernel must NOT produce."""
import numpy as np

F = np.float32


def scatter_det(q, d_ctx, p, ds, idx3, w3, scale, NK, reverse=False):
    """q, d_ctx (B,N,C), p, ds (B,N,H,k) as the kernels saved them, idx3 / w3 (B,G,N k,3) -> d_PK, d_PV (B,G,NK,C): every target starts
    at +0.0f and takes w3 * ((scale * ds) * q) resp. w3 * (p * d_ctx) of every source (n, s, j) with idx3 == target, in ascending
    (n k + s) 3 + j, one rounded addition each; an index outside [0, NK) is skipped."""
    q, d_ctx, p, ds, w3 = (np.asarray(t, F) for t in (q, d_ctx, p, ds, w3))
    B, N, C = q.shape
    H, k = p.shape[2], p.shape[3]
    G = idx3.shape[1]
    scale = F(scale)
    d_PK, d_PV = np.zeros((B, G, NK, C), F), np.zeros((B, G, NK, C), F)
    head = np.arange(C) // 64
    order = range(N * k * 3 - 1, -1, -1) if reverse else range(N * k * 3)
    for b in range(B):
        for g in range(G):
            for src in order:
                j, ns = src % 3, src // 3
                n, s = ns // k, ns % k
                r = int(idx3[b, g, ns, j])
                if not 0 <= r < NK:
                    continue
                w = w3[b, g, ns, j]
                dk = ((scale * ds[b, n, :, s]).astype(F)[head] * q[b, n]).astype(F)
                dv = (p[b, n, :, s][head] * d_ctx[b, n]).astype(F)
                d_PK[b, g, r] = (d_PK[b, g, r] + (w * dk).astype(F)).astype(F)
                d_PV[b, g, r] = (d_PV[b, g, r] + (w * dv).astype(F)).astype(F)
    return d_PK, d_PV
