"""The stated order of upp_region_attn_bwd_det's three scatter-adds (include/upp_hip.h "region-wise deformable attention") in numpy f32:
every addition and every product is one f32 operation rounded to nearest, every target starts from +0.0f.
    d_q[b, idx[b,n,t]]            += rows[0,b,n,t]                      in ascending n k + t
    d_PK[b, g, idx3[b,g,n k+s,j]] += w3[b,g,n k+s,j] * rows[1,b,n,s]    in ascending (n k + s) 3 + j;  d_PV likewise from rows[2]
An index outside its range is skipped."""
import numpy as np


def scatter_det(rows, idx, idx3, w3, NK, reverse=False):
    """rows (3,B,N,k,C) f32, idx (B,N,k) int64, idx3 int32 and w3 f32 (B,G,N k,3) -> d_q (B,N,C), d_PK, d_PV (B,G,NK,C); reverse walks
    the sources in descending order (what the order is worth on an input)."""
    _, B, N, k, C = rows.shape
    G = idx3.shape[1]
    rows = rows.astype(np.float32)
    d_q = np.zeros((B, N, C), np.float32)
    d_PK, d_PV = np.zeros((B, G, NK, C), np.float32), np.zeros((B, G, NK, C), np.float32)
    order = range(N * k - 1, -1, -1) if reverse else range(N * k)
    js = (2, 1, 0) if reverse else (0, 1, 2)
    for b in range(B):
        flat = rows[:, b].reshape(3, N * k, C)
        for src in order:
            j = int(idx[b, src // k, src % k])
            if 0 <= j < N:
                d_q[b, j] = d_q[b, j] + flat[0, src]
        for g in range(G):
            for src in order:
                for j in js:
                    r = int(idx3[b, g, src, j])
                    if 0 <= r < NK:
                        w = np.float32(w3[b, g, src, j])
                        d_PK[b, g, r] = d_PK[b, g, r] + w * flat[1, src]
                        d_PV[b, g, r] = d_PV[b, g, r] + w * flat[2, src]
    return d_q, d_PK, d_PV
