"""Numpy restatements of the five DEFINED summation orders of the library's deterministic scatter-adds (include/upp_hip.h
"deterministic scatter-adds"): plain loops in np.float32, one rounded operation per statement (a statement on a row of 3 is three
independent scalar operations), so that the kernels can be compared with them bit for bit.  `reverse=True` walks every list of foreign
terms backwards -- the order the kernels must NOT produce; the host tests use it to show that these restatements can see order."""
import numpy as np

F = np.float32


def _order(n, reverse):
    return range(n - 1, -1, -1) if reverse else range(n)


def chamfer_terms(a, b, idx, gd):
    """t(j)[c] = (gd[j] * 2.0f) * (a[j][c] - b[idx[j]][c]) of one cloud pair: a (n,3), b (m,3), idx (n,), gd (n,) -> (n,3)."""
    a, b, gd = np.asarray(a, F), np.asarray(b, F), np.asarray(gd, F)
    out = np.empty((a.shape[0], 3), F)
    for j in range(a.shape[0]):
        g = F(gd[j] * F(2.0))
        d = (a[j] - b[int(idx[j])]).astype(F)
        out[j] = (g * d).astype(F)
    return out


def chamfer_bwd(xyz1, xyz2, idx1, idx2, gd1, gd2, reverse=False):
    """g1[b][j] = +0.0f + t1(j), then - t2(i) for every i with idx2[b][i] == j in ascending i; g2 the mirror image."""
    xyz1, xyz2 = np.asarray(xyz1, F), np.asarray(xyz2, F)
    g1, g2 = np.empty_like(xyz1), np.empty_like(xyz2)
    for b in range(xyz1.shape[0]):
        t1 = chamfer_terms(xyz1[b], xyz2[b], idx1[b], gd1[b])
        t2 = chamfer_terms(xyz2[b], xyz1[b], idx2[b], gd2[b])
        for own, foreign, fidx, out in ((t1, t2, idx2[b], g1[b]), (t2, t1, idx1[b], g2[b])):
            acc = np.zeros_like(own)
            acc = (acc + own).astype(F)
            for i in _order(foreign.shape[0], reverse):
                j = int(fidx[i])
                acc[j] = (acc[j] - foreign[i]).astype(F)
            out[...] = acc
    return g1, g2


def foreign_counts(idx_other, n):
    """(B, n): how many points of the other cloud chose each target."""
    return np.stack([np.bincount(np.asarray(r, np.int64), minlength=n) for r in idx_other])


def rows_scatter(vals, idx, N, reverse=False):
    """out[b][r] = +0.0f, then + vals[b][s] for every s with idx[b][s] == r in ascending s; vals (B,S,W), idx (B,S) -> (B,N,W).
    Indices outside [0, N) are skipped."""
    vals = np.asarray(vals, F)
    B, S, W = vals.shape
    out = np.zeros((B, N, W), F)
    for b in range(B):
        for s in _order(S, reverse):
            r = int(idx[b][s])
            if 0 <= r < N:
                out[b, r] = (out[b, r] + vals[b, s]).astype(F)
    return out


def group_bwd(grad_out, idx, N, reverse=False):
    """grad_out (B,G,K,3), idx (B,G,K) -> grad_xyz (B,N,3) in ascending g * K + k, grad_center (B,G,3) = -(k-ascending sum)."""
    grad_out = np.asarray(grad_out, F)
    B, G, K, _ = grad_out.shape
    gx = rows_scatter(grad_out.reshape(B, G * K, 3), np.asarray(idx).reshape(B, G * K), N, reverse)
    s = np.zeros((B, G, 3), F)
    for k in range(K):
        s = (s + grad_out[:, :, k]).astype(F)
    return gx, (-s).astype(F)


def gather_bwd(grad_out, idx, N, reverse=False):
    """grad_out (B,C,M), idx (B,M) -> grad_feat (B,C,N) in ascending j."""
    grad_out = np.asarray(grad_out, F)
    return np.ascontiguousarray(rows_scatter(grad_out.transpose(0, 2, 1), idx, N, reverse).transpose(0, 2, 1))


def fps_gather_bwd(g_centers, idx, N, reverse=False):
    """g_centers (B,M,3), idx (B,M) -> g_xyz (B,N,3) in ascending j."""
    return rows_scatter(g_centers, idx, N, reverse)


# ---- inputs at the edges of the kernels' shared body (csrc/det_scan.h): a second chunk of fewer than four sources (S = 1,027 / 1,029),
# a second tile with one live lane (T = 257), a second channel group with one live channel (5 channels), keys of -1 and of T -----------
def edge_indices(rng, B, S, T):
    """(B,S) int64 drawn with repetition from [0, T).  Target T - 1 owns the first, a middle and the LAST source (chunk two, tile two);
    sources 3 and S - 2 are -1 and sources 7 and S - 3 are T: outside [0, T), skipped by the `_det` kernels -- their atomic siblings do
    not range-check and must not see these lists."""
    idx = rng.integers(0, T, (B, S))
    idx[:, [0, S // 2, S - 1]] = T - 1
    idx[:, [3, S - 2]] = -1
    idx[:, [7, S - 3]] = T
    return idx


def mixed_upstream(rng, shape):
    """signed f32 gradients over seven decades of magnitude: a sum of three or more of them depends on the order in its last bits"""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(F)


def ordered_sum(parts, reverse=False):
    """((+0.0f + p_0) + p_1) + ... along the last axis: the EMD cost from its tiles' partial costs."""
    parts = np.asarray(parts, F)
    s = np.zeros(parts.shape[:-1], F)
    for t in _order(parts.shape[-1], reverse):
        s = (s + parts[..., t]).astype(F)
    return s
