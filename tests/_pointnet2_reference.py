"""Numpy restatements of the four pointnet2_ops operators the library serves beside FPS and gather (include/upp_hip.h "the
pointnet2_ops surface") and of the two defined summation orders of their `_det` backward passes: plain loops in np.float32, one rounded
operation per statement, so that the kernels can be compared with them bit for bit.  `reverse=True` walks the sources backwards -- the
order the kernels must NOT produce.

Distances.  `sqdist32` is the library's convention, fma(z, z, fma(x, x, y * y)) on the f32 differences, with each fma emulated as one
float64 multiply-add rounded to f32.  On LATTICE clouds (coordinates k / 256 in [-1, 1]) every difference, product and sum is exactly
representable in f32, so the emulation -- and contraction of any kind -- cannot matter, and ties are plentiful.  On random f32 clouds
the tests select in float64 (`sqdist64`) under preconditions checked on these arrays alone (`gaps_first4`, `gap_to`): with every
relevant pair of distances more than 1e-5 apart relatively, an f32 evaluation (error < 1e-6 relative) selects the same indices."""
import numpy as np

from _det_reference import rows_scatter

F = np.float32


def lattice_clouds(B, N, seed, dense=0.5):
    """(B,N,3) f32, coordinates k / 256 in [-1, 1]: a coarse lattice of step 1/8 over the whole cube and -- a fraction `dense` of the points --
    a core of step 1/16 inside [-1/4, 1/4]^3, so that a radius of 0.5 holds many points for some queries and few for others; the second half of
    each kind repeats points (duplicates)."""
    g = np.random.default_rng(seed)
    k = g.integers(-8, 9, (B, N, 3)) * 32
    core = g.random((B, N)) < dense
    k[core] = g.integers(-4, 5, (int(core.sum()), 3)) * 16
    dup = g.random((B, N)) < 0.25
    src = g.integers(0, N, (B, N))
    for b in range(B):
        k[b, dup[b]] = k[b, src[b, dup[b]]]
    return (k.astype(np.float64) / 256.0).astype(F)


def sqdist64(q, cloud):
    """(P,3), (N,3) f32 -> (P,N) float64 squared distances of the f32 coordinates."""
    d = np.asarray(q, np.float64)[:, None, :] - np.asarray(cloud, np.float64)[None, :, :]
    return (d * d).sum(-1)


def sqdist32(q, cloud):
    """(P,3), (N,3) f32 -> (P,N) f32: t = y * y; t = fma(x, x, t); t = fma(z, z, t) on the f32 differences (csrc/common.h sumsq3)."""
    d = (np.asarray(q, F)[:, None, :] - np.asarray(cloud, F)[None, :, :]).astype(F)
    x, y, z = (d[..., c].astype(np.float64) for c in range(3))
    t = (d[..., 1] * d[..., 1]).astype(F)
    t = (x * x + t.astype(np.float64)).astype(F)
    return (z * z + t.astype(np.float64)).astype(F)


def gaps_first4(d):
    """Smallest relative gap between consecutive entries of the four smallest distances of every row of d (P,N) float64 (inf if N < 2)."""
    s = np.sort(d, axis=1)[:, :4]
    if s.shape[1] < 2:
        return np.inf
    return float(((s[:, 1:] - s[:, :-1]) / np.maximum(s[:, 1:], 1e-300)).min())


def gap_to(d, value):
    """Smallest relative distance of any entry of d from `value`."""
    return float((np.abs(d - value) / value).min())


def ball_query(xyz, new_xyz, radius, nsample, dist=sqdist32):
    """xyz (B,N,3), new_xyz (B,P,3) -> (B,P,nsample) int32 -- and the number of in-radius points per query (B,P), uncapped."""
    B, N, _ = xyz.shape
    P = new_xyz.shape[1]
    r2 = F(F(radius) * F(radius))
    if dist is sqdist64:
        r2 = np.float64(r2)
    idx = np.zeros((B, P, nsample), np.int32)
    hits = np.zeros((B, P), np.int64)
    for b in range(B):
        d2 = dist(new_xyz[b], xyz[b])
        for j in range(P):
            cnt = 0
            for k in range(N):
                if d2[j, k] < r2:
                    hits[b, j] += 1
                    if cnt < nsample:
                        if cnt == 0:
                            idx[b, j, :] = k
                        idx[b, j, cnt] = k
                        cnt += 1
    return idx, hits


def three_nn(unknown, known, dist=sqdist32):
    """unknown (B,n,3), known (B,m,3) -> (dist (B,n,3) = sqrt of the squared distance in the precision of `dist`, idx (B,n,3) int32)."""
    B, n, _ = unknown.shape
    m = known.shape[1]
    idx = np.zeros((B, n, 3), np.int32)
    best = np.full((B, n, 3), np.inf, np.float64 if dist is sqdist64 else F)
    for b in range(B):
        d2 = dist(unknown[b], known[b])
        for i in range(n):
            b1 = b2 = b3 = np.inf
            i1 = i2 = i3 = 0
            for k in range(m):
                d = d2[i, k]
                if d < b1:
                    b3, i3, b2, i2, b1, i1 = b2, i2, b1, i1, d, k
                elif d < b2:
                    b3, i3, b2, i2 = b2, i2, d, k
                elif d < b3:
                    b3, i3 = d, k
            best[b, i] = (b1, b2, b3)
            idx[b, i] = (i1, i2, i3)
    return np.sqrt(best), idx


def three_interpolate(features, idx, weight):
    """features (B,C,m), idx (B,n,3), weight (B,n,3) -> (B,C,n): (w0 * f[i0] + w1 * f[i1]) + w2 * f[i2], five rounded operations."""
    features, weight = np.asarray(features, F), np.asarray(weight, F)
    B, C, _ = features.shape
    n = idx.shape[1]
    out = np.empty((B, C, n), F)
    for b in range(B):
        for i in range(n):
            t0 = (weight[b, i, 0] * features[b, :, idx[b, i, 0]]).astype(F)
            t1 = (weight[b, i, 1] * features[b, :, idx[b, i, 1]]).astype(F)
            t2 = (weight[b, i, 2] * features[b, :, idx[b, i, 2]]).astype(F)
            s = (t0 + t1).astype(F)
            out[b, :, i] = (s + t2).astype(F)
    return out


def grouping(features, idx):
    """features (B,C,N), idx (B,P,S) -> (B,C,P,S)."""
    features = np.asarray(features, F)
    B, C, _ = features.shape
    _, P, S = idx.shape
    out = np.empty((B, C, P, S), F)
    for b in range(B):
        out[b] = features[b][:, idx[b].reshape(-1)].reshape(C, P, S)
    return out


def three_interpolate_bwd_det(grad_out, idx, weight, m, reverse=False):
    """grad_features[b][c][r] = +0.0f, then + (grad_out[b][c][i] * weight[b][i][j]) for every (i, j) with idx[b][i][j] == r, in ascending
    i * 3 + j: the product rounded, then the sum.  Indices outside [0, m) are skipped."""
    grad_out, weight = np.asarray(grad_out, F), np.asarray(weight, F)
    B, C, n = grad_out.shape
    terms = (grad_out.transpose(0, 2, 1)[:, :, None, :] * weight[:, :, :, None]).astype(F)          # (B,n,3,C): one rounded product each
    out = rows_scatter(terms.reshape(B, 3 * n, C), np.asarray(idx).reshape(B, 3 * n), m, reverse)
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def grouping_bwd_det(grad_out, idx, N, reverse=False):
    """grad_features[b][c][r] = +0.0f, then + grad_out[b][c][p][s] for every (p, s) with idx[b][p][s] == r, in ascending p * S + s."""
    grad_out = np.asarray(grad_out, F)
    B, C, P, S = grad_out.shape
    out = rows_scatter(grad_out.reshape(B, C, P * S).transpose(0, 2, 1), np.asarray(idx).reshape(B, P * S), N, reverse)
    return np.ascontiguousarray(out.transpose(0, 2, 1))


# ---- the cases of the host and GPU tests: the smallest shapes that reach every branch (one and several tiles of 128 queries, clouds
# shorter than a wave, m < 3, nsample = 1) ------------------------------------------------------------------------------------------
RADIUS = 0.5
BALL_SHAPES = [(2, 130, 9, 16), (1, 64, 64, 1), (3, 257, 5, 32), (1, 5, 3, 8)]          # (B, N, P, nsample)
NN_SHAPES = [(2, 7, 3), (1, 65, 130), (2, 129, 64), (1, 4, 2), (1, 4, 1)]                # (B, n, m)
# the searches stage the searched cloud in tiles of 1,024 points and serve 128 queries per workgroup: one shape each beyond both
BALL_SHAPES_LONG = [(2, 1100, 130, 4)]
NN_SHAPES_LONG = [(2, 130, 1030)]
# seeds under which the preconditions of the random cases hold (checked on the CPU: tests/test_pointnet2_host.py)
BALL_SEEDS = {(2, 130, 9, 16): 0, (1, 64, 64, 1): 0, (3, 257, 5, 32): 0, (1, 5, 3, 8): 0, (2, 1100, 130, 4): 0}
NN_SEEDS = {(2, 7, 3): 0, (1, 65, 130): 0, (2, 129, 64): 0, (1, 4, 2): 0, (1, 4, 1): 0, (2, 130, 1030): 0}


def lattice_ball_case(shape):
    """-> xyz (B,N,3), new_xyz (B,P,3): lattice clouds; the queries are points of the cloud (distance 0, duplicates tie) except the last
    one, the cube's corner; point 0 of every cloud lies at EXACTLY `RADIUS` from query 0 (it must be excluded -- were it included it
    would be the first hit and fill every slot)."""
    B, N, P, _ = shape
    xyz = lattice_clouds(B, N, seed=N * 31 + P)
    g = np.random.default_rng(N + P)
    new_xyz = np.stack([xyz[b, g.permutation(N)[np.arange(P) % N]] for b in range(B)])
    new_xyz[:, -1] = (1.0, 1.0, 1.0)
    new_xyz[:, 0] = (0.25, 0.0, -0.25)
    xyz[:, 0] = (0.75, 0.0, -0.25)
    return xyz, np.ascontiguousarray(new_xyz)


def random_ball_case(shape, seed=None):
    """-> xyz in [-1, 1]^3, new_xyz in [-1.4, 1.4]^3 (some queries far from every point), uniform f32."""
    B, N, P, _ = shape
    g = np.random.default_rng(BALL_SEEDS[shape] if seed is None else seed)
    return (g.random((B, N, 3), dtype=F) * F(2) - F(1)).astype(F), (g.random((B, P, 3), dtype=F) * F(2.8) - F(1.4)).astype(F)


def ball_preconditions(xyz, new_xyz, nsample):
    """On the float64 distances alone: every distance more than 1e-5 (relative) away from radius^2, a query without a hit and -- where
    nsample > 1 leaves room for one -- a query with some but fewer than nsample hits, each among several queries."""
    r2 = float(F(F(RADIUS) * F(RADIUS)))
    zero = part = False
    for b in range(xyz.shape[0]):
        d = sqdist64(new_xyz[b], xyz[b])
        if gap_to(d, r2) <= 1e-5:
            return False
        hits = (d < r2).sum(1)
        zero |= bool((hits == 0).any())
        part |= bool(((hits > 0) & (hits < nsample)).any())
    return zero and (part or nsample == 1) and xyz.shape[0] * new_xyz.shape[1] > 1


def lattice_nn_case(shape):
    B, n, m = shape
    known = lattice_clouds(B, m, seed=n * 17 + m)
    g = np.random.default_rng(n + m)
    unknown = lattice_clouds(B, n, seed=n * 13 + m + 1)
    take = g.random((B, n)) < 0.5                                   # half the unknown points ARE known points
    for b in range(B):
        unknown[b, take[b]] = known[b, g.integers(0, m, int(take[b].sum()))]
    return unknown, known


def random_nn_case(shape, seed=None):
    B, n, m = shape
    g = np.random.default_rng(NN_SEEDS[shape] if seed is None else seed)
    return (g.random((B, n, 3), dtype=F) * F(2) - F(1)).astype(F), (g.random((B, m, 3), dtype=F) * F(2) - F(1)).astype(F)


def nn_preconditions(unknown, known):
    """On the float64 distances alone: for every query the four smallest distances are more than 1e-5 (relative) apart."""
    return all(gaps_first4(sqdist64(unknown[b], known[b])) > 1e-5 for b in range(unknown.shape[0]))
