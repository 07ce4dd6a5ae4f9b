"""Numpy restatement of the rules of include/upp_hip.h "the pytorch3d.ops surface" (knn_points, knn_gather, their backward terms and the
defined order of the `_det` scatter), written as plain f32 steps so that the kernels can be compared with it bit for bit.  The upstream
CUDA sources were not at hand: like tests/_pointnet2_reference.py this restates the header, it does not pin upstream.

The distance is a chain of fused multiply-adds.  numpy has none, so fma32 forms the exact product and the sum in float64 and rounds that
sum TO ODD before the final rounding to float32 -- with 29 spare bits the double rounding is then the single rounding of a real fma."""
import numpy as np

from _det_reference import rows_scatter

F = np.float32


def fma32(a, b, c):
    """round_f32(a * b + c) with ONE rounding, elementwise on float32 arrays."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b                                            # exact: 24 x 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                      # TwoSum: p + c = s + err exactly
    bits = np.atleast_1d(s).copy().view(np.int64)
    inexact = np.atleast_1d(err != 0)
    toward_zero = np.atleast_1d((err > 0) != (s > 0))    # the exact sum lies between s and zero: step the magnitude down first
    mag = bits & np.int64(0x7FFFFFFFFFFFFFFF)
    mag = np.where(inexact & toward_zero, mag - 1, mag)
    mag = np.where(inexact, mag | 1, mag)
    bits = (bits & np.int64(-0x8000000000000000)) | mag
    return bits.view(np.float64).reshape(np.shape(s)).astype(F)


def clamp_lengths(lengths, N, P):
    if lengths is None:
        return np.full(N, P, np.int64)
    return np.clip(np.asarray(lengths, np.int64).reshape(N), 0, P)


def distances(q, pts, norm=2):
    """q (P1,D), pts (P2,D) f32 -> (P1,P2) f32: d = 0; for j ascending: diff = q[j] - p[j]; d = fma(diff, diff, d)  or  d = d + |diff|."""
    q, pts = np.asarray(q, F), np.asarray(pts, F)
    d = np.zeros((q.shape[0], pts.shape[0]), F)
    for j in range(q.shape[1]):
        diff = (q[:, None, j] - pts[None, :, j]).astype(F)
        d = fma32(diff, diff, d) if norm == 2 else (d + np.abs(diff)).astype(F)
    return d


def distances64(q, pts, norm=2):
    diff = np.asarray(q, np.float64)[:, None, :] - np.asarray(pts, np.float64)[None, :, :]
    return (diff * diff).sum(-1) if norm == 2 else np.abs(diff).sum(-1)


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, dist=distances):
    """-> dists (N,P1,K) f32, idx (N,P1,K) int64, nn (N,P1,K,D) f32: ascending (distance, index) over the first lengths2[n] points; zeros in
    slots k >= min(K, lengths2[n]) and in rows i >= lengths1[n]."""
    p1, p2 = np.asarray(p1, F), np.asarray(p2, F)
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    len1, len2 = clamp_lengths(lengths1, N, P1), clamp_lengths(lengths2, N, P2)
    dists, idx, nn = np.zeros((N, P1, K), F), np.zeros((N, P1, K), np.int64), np.zeros((N, P1, K, D), F)
    for n in range(N):
        kk, rows = min(K, int(len2[n])), int(len1[n])
        if kk == 0 or rows == 0:
            continue
        d = dist(p1[n, :rows], p2[n, :len2[n]], norm)
        order = np.argsort(d, axis=1, kind="stable")[:, :kk]                       # stable: equal distances keep the lower index first
        idx[n, :rows, :kk] = order
        dists[n, :rows, :kk] = np.take_along_axis(d, order, 1)
        nn[n, :rows, :kk] = p2[n][order]
    return dists, idx, nn


def knn_gather(x, idx, lengths=None):
    """x (N,M,U), idx (N,L,K) -> (N,L,K,U) = x[n, idx[n,l,k]], zeros in slots k >= lengths[n]."""
    x = np.asarray(x, F)
    N, L, K = idx.shape
    lens = clamp_lengths(lengths, N, K)
    out = np.zeros((N, L, K, x.shape[2]), F)
    for n in range(N):
        out[n, :, :lens[n]] = x[n][idx[n, :, :lens[n]]]
    return out


def live_slots(N, P1, K, P2, lengths1=None, lengths2=None):
    """(N,P1,K) bool: the slots that hold a neighbour."""
    len1, len2 = clamp_lengths(lengths1, N, P1), clamp_lengths(lengths2, N, P2)
    return (np.arange(P1)[None, :, None] < len1[:, None, None]) & (np.arange(K)[None, None, :] < np.minimum(len2, K)[:, None, None])


def knn_points_bwd(p1, p2, idx, grad_dists, lengths1=None, lengths2=None, norm=2):
    """-> g_p1 (N,P1,D), t (N,P1,K,D): t = (2 g) * diff (norm 2) or sign(diff) * g (norm 1), diff = p1 - p2[idx], zero in padded slots;
    g_p1 = +0.0f, then + t over the filled slots in ascending k."""
    p1, p2, g = np.asarray(p1, F), np.asarray(p2, F), np.asarray(grad_dists, F)
    N, P1, D = p1.shape
    K = idx.shape[2]
    live = live_slots(N, P1, K, p2.shape[1], lengths1, lengths2)
    t, g_p1 = np.zeros((N, P1, K, D), F), np.zeros((N, P1, D), F)
    for n in range(N):
        for k in range(K):
            diff = (p1[n] - p2[n][idx[n, :, k]]).astype(F)
            if norm == 2:
                tv = ((F(2.0) * g[n, :, k]).astype(F)[:, None] * diff).astype(F)
            else:
                gk = g[n, :, k][:, None]
                tv = np.where(diff > 0, gk, np.where(diff < 0, -gk, F(0.0))).astype(F)              # sign(0) = 0: +0.0f
            tv = np.where(live[n, :, k][:, None], tv, F(0.0))
            t[n, :, k] = tv
            g_p1[n] = np.where(live[n, :, k][:, None], (g_p1[n] + tv).astype(F), g_p1[n])
    return g_p1, t


def scatter_add_det(src, idx, M, rows=None, slots=None, negate=False, reverse=False):
    """src (N,L,K,U), idx (N,L,K) -> out (N,M,U): out[n][r] = +0.0f, then + src[n][l][k] (negate: - src) for every slot with l < rows[n],
    k < slots[n] and idx == r, in ascending l * K + k, one rounded f32 addition at a time.  reverse: the order the kernel must NOT use."""
    src = np.asarray(src, F)
    N, L, K, U = src.shape
    nrows, nslots = clamp_lengths(rows, N, L), clamp_lengths(slots, N, K)
    live = (np.arange(L)[None, :, None] < nrows[:, None, None]) & (np.arange(K)[None, None, :] < nslots[:, None, None])
    keys = np.where(live, np.asarray(idx, np.int64), -1)                                 # a slot that takes no part: a key nobody owns
    return rows_scatter((-src if negate else src).reshape(N, L * K, U), keys.reshape(N, L * K), M, reverse)         # (adding -x IS subtracting x)


def scatter_bound(src, idx, M, rows=None, slots=None):
    """-> (float64 sums (N,M,U), the rounding bound (m + 2) * 2^-24 * sum |terms| per target, m = its number of terms)."""
    src = np.asarray(src, np.float64)
    N, L, K, U = src.shape
    nrows, nslots = clamp_lengths(rows, N, L), clamp_lengths(slots, N, K)
    total, mag, cnt = np.zeros((N, M, U)), np.zeros((N, M, U)), np.zeros((N, M, 1))
    for n in range(N):
        ok = (np.arange(L)[:, None] < nrows[n]) & (np.arange(K)[None, :] < nslots[n]) & (idx[n] >= 0) & (idx[n] < M)
        r, v = idx[n][ok], src[n][ok]
        np.add.at(total[n], r, v)
        np.add.at(mag[n], r, np.abs(v))
        np.add.at(cnt[n], r, 1.0)
    return total, (cnt + 2.0) * 2.0 ** -24 * mag


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def lattice_case(N, P1, P2, D, seed, span=24):
    """Coordinates k / 256 with small k: every difference, product and sum of the distance is exact in f32, so any correct formulation
    has the same bits, and ties and duplicates abound.  Half of p1 is copied from p2 (zero distances)."""
    g = np.random.default_rng(seed)
    p2 = (g.integers(-span, span + 1, (N, P2, D)) / 256.0).astype(F)
    p1 = (g.integers(-span, span + 1, (N, P1, D)) / 256.0).astype(F)
    take = g.integers(0, P2, (N, P1))
    for n in range(N):
        p1[n, ::2] = p2[n, take[n, ::2]]
    if P2 > 2:
        p2[:, P2 // 2] = p2[:, 0]                        # a duplicated point: a tie at every query
    return p1, p2


def ragged_lengths(N, P, seed, special=()):
    """lengths in [1, P], with the entries of `special` (e.g. 0, a value below K, a value above P) put first."""
    g = np.random.default_rng(seed)
    out = g.integers(1, P + 1, N).astype(np.int64)
    for i, v in enumerate(special[:N]):
        out[i] = v
    return out


def random_case(N, P1, P2, D, seed):
    g = np.random.default_rng(seed)
    return g.random((N, P1, D), dtype=F) - F(0.5), g.random((N, P2, D), dtype=F) - F(0.5)


def separated_queries(p1, p2, K, norm=2, rel=1e-5):
    """(N,P1) bool: queries whose K + 1 smallest float64 distances are pairwise more than `rel` apart, relative (their f32 neighbour list
    cannot depend on rounding)."""
    N, P1, _ = p1.shape
    ok = np.zeros((N, P1), bool)
    for n in range(N):
        d = np.sort(distances64(p1[n], p2[n], norm), axis=1)[:, :K + 1]
        ok[n] = ((d[:, 1:] - d[:, :-1]) > rel * d[:, 1:]).all(1)
    return ok


# the grid of the forward comparison (tests/test_gpu_knn_points.py): (N, P1, P2, D, K); K > P2 pads; P2 = 4097 spans two LDS chunks at
# D = 3 (4,096 points each), P2 = 1000 three at D = 32 (384 points each) and is no multiple of 64
FORWARD_GRID = [
    (3, 1, 1, 1, 1), (3, 5, 1, 3, 4), (3, 72, 63, 3, 4), (3, 5, 64, 5, 64), (3, 72, 65, 1, 64), (3, 5, 65, 32, 4),
    (3, 72, 1000, 3, 4), (3, 5, 1000, 5, 64), (3, 72, 1000, 32, 64), (3, 1, 1000, 32, 1), (3, 72, 63, 32, 64), (3, 5, 64, 3, 1),
    (3, 5, 4097, 3, 4), (3, 72, 1000, 1, 1),
]
RANDOM_GRID = [(3, 72, 1000, 3, 4, 11), (3, 72, 1000, 32, 4, 12), (3, 5, 4097, 3, 4, 13), (3, 72, 65, 5, 4, 14), (3, 72, 1000, 5, 16, 15)]   # (..., seed)
