"""Plain torch reference of the two completion losses -- csrc/chamfer.hip and csrc/emd.hip -- forward AND backward, with the gradients
written out: no autograd, none of the project's kernels.  One set of functions evaluates a formulation in any dtype on any device, so
the same code is the float64 arbiter and the float32 yardstick of tests/test_gpu_losses.py; tests/test_loss_host.py checks it on the CPU
against the C oracle, against torch autograd and against the reference's known answers.

    chamfer        d[j, i] = |xyz1_j - xyz2_i|^2;  dist1 = min_i, idx1 = the LOWEST i of the minimum; dist2 / idx2 the other direction
    chamfer_bwd    g1_j = 2 gd1_j (xyz1_j - xyz2_idx1[j]) - sum_{i: idx2[i] = j} 2 gd2_i (xyz2_i - xyz1_j);  g2 the mirror image
    chamfer_loss   L1: (mean sqrt d1 + mean sqrt d2) / 2, L2: mean d1 + mean d2;  fac = d loss / d dist element-wise (+inf at d = 0 under L1)
    emd auction    10 levels (-4^7 ... -4^-1, 0) of: ratioL = remL / (1e-9 + sum_l e remR), sumr = remR sum_k e ratioL,
                   ratioR = min(remR / (sumr + 1e-9), 1) remR, remR = max(0, remR - sumr), match += e ratioL ratioR,
                   remL = max(0, remL - sum_l e ratioL ratioR), with e[l, k] = exp(level d[l, k])
    emd one step   the same level from GIVEN factors: the remains are rebuilt level by level from a caller's ratioL / ratioR (the device's),
                   and each level's ratioL, ratioR and the match are what the formulas give from those remains -- no error is carried
                   through the auction, which amplifies last bits (two float32 runs of it differ by up to 8e-4 of max|match| at 64 x 64)
    emd cost       cost_b = sum_{l,k} d[l, k] match[l, k];  grad1_k = gc_b sum_l 2 match[l, k] (xyz1_k - xyz2_l),  grad2 the mirror image

SELECTIONS -- the arg-min of Chamfer -- are taken once, in float64, and handed to both precisions.
"""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64

LEVELS = tuple(-(4.0 ** j) for j in range(7, -2, -1)) + (0.0,)      # emd_kernel.cu:45-49: -4^7 ... -4^-1, then 0
TINY = float(np.float32(1e-9))                                       # the C float the kernels add to both denominators


def sqdist(a, b, dt):
    """(B, n, 3), (B, m, 3) -> (B, n, m): (dx dx + dy dy) + dz dz in dt."""
    a, b = a.to(dt), b.to(dt)
    df = a[:, :, None, :] - b[:, None, :, :]
    return (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]


def first_min(d, dim):
    """(min, index of its FIRST occurrence) along dim; no NaN expected."""
    mn = d.min(dim, keepdim=True).values
    n = d.shape[dim]
    shape = [1] * d.dim()
    shape[dim] = n
    ar = torch.arange(n, device=d.device).view(shape).expand_as(d)
    return mn.squeeze(dim), torch.where(d == mn, ar, torch.full_like(ar, n)).min(dim).values


# ---------------------------------------------------------------------------------------------- Chamfer
def chamfer_select(xyz1, xyz2):
    """idx1 (B, n), idx2 (B, m) int64: the float64 arg-min with the lowest-index rule, one sample at a time (memory)."""
    i1, i2 = [], []
    for b in range(xyz1.shape[0]):
        d = sqdist(xyz1[b:b + 1], xyz2[b:b + 1], F64)[0]
        i1.append(first_min(d, 1)[1])
        i2.append(first_min(d, 0)[1])
    return torch.stack(i1), torch.stack(i2)


def _pair_sq(a, b, idx, dt):
    a = a.to(dt)
    p = torch.gather(b.to(dt), 1, idx[..., None].expand(-1, -1, 3))
    df = a - p
    return (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]


def chamfer(xyz1, xyz2, idx1, idx2, dt):
    """dist1 (B, n), dist2 (B, m) in dt at the GIVEN partners."""
    return dict(dist1=_pair_sq(xyz1, xyz2, idx1, dt), dist2=_pair_sq(xyz2, xyz1, idx2, dt))


def chamfer_bwd(xyz1, xyz2, idx1, idx2, gd1, gd2, dt):
    """g1 (B, n, 3), g2 (B, m, 3): own term, minus the terms of the other cloud's points that chose the row (index_add_: on the CPU the
    terms arrive in ascending index, on the device in any order)."""
    a, b = xyz1.to(dt), xyz2.to(dt)
    B, n, _ = a.shape
    m = b.shape[1]
    t1 = (gd1.to(dt) * 2)[..., None] * (a - torch.gather(b, 1, idx1[..., None].expand(-1, -1, 3)))
    t2 = (gd2.to(dt) * 2)[..., None] * (b - torch.gather(a, 1, idx2[..., None].expand(-1, -1, 3)))
    off1 = (torch.arange(B, device=a.device) * m).view(B, 1)
    off2 = (torch.arange(B, device=a.device) * n).view(B, 1)
    g1 = t1.reshape(-1, 3).clone().index_add_(0, (idx2 + off2).reshape(-1), -t2.reshape(-1, 3))
    g2 = t2.reshape(-1, 3).clone().index_add_(0, (idx1 + off1).reshape(-1), -t1.reshape(-1, 3))
    return dict(g1=g1.view(B, n, 3), g2=g2.view(B, m, 3))


def chamfer_loss(dist1, dist2, l1, dt):
    """loss (scalar), fac1, fac2: the modules' reductions (reference extensions/chamfer_dist/__init__.py:44-84) and their derivative with
    respect to every distance, as torch.sqrt's backward gives it: +inf at an exact 0 under L1."""
    d1, d2 = dist1.to(dt), dist2.to(dt)
    if l1:
        r1, r2 = torch.sqrt(d1), torch.sqrt(d2)
        return dict(loss=(r1.mean() + r2.mean()) / 2, fac1=0.5 / d1.numel() * (0.5 / r1), fac2=0.5 / d2.numel() * (0.5 / r2))
    return dict(loss=d1.mean() + d2.mean(), fac1=torch.full_like(d1, 1.0 / d1.numel()), fac2=torch.full_like(d2, 1.0 / d2.numel()))


# ---------------------------------------------------------------------------------------------- EMD
def emd_multi(n, m):
    """(multiL, multiR): the masses of a point of xyz1 / xyz2, integer division (emd_kernel.cu:28-34)."""
    return (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)


LOG2E = float(np.float32(1.4426950408889634))


def _level(d, it, remL, remR, ratioL=None, ratioR=None, fast_exp=False):
    """One level from the remains (B, n) / (B, m), with d (B, m, n).  ratioL / ratioR given: the sums that FOLLOW them use the given ones
    (the one-step recipe); None: the level's own (the auction).  fast_exp: the exponential as the fast intrinsic of the reference and of
    the kernels forms it, 2^((level d) log2 e) with the product rounded.  -> dict of the level's quantities and the remains after it."""
    e = torch.exp2((LEVELS[it] * d) * LOG2E) if fast_exp else torch.exp(LEVELS[it] * d)
    suml = TINY + torch.einsum("bmn,bm->bn", e, remR)
    pl = remL / suml
    rl = pl if ratioL is None else ratioL
    sumr = torch.einsum("bmn,bn->bm", e, rl) * remR
    pr = torch.clamp(remR / (sumr + TINY), max=1.0) * remR
    rr = pr if ratioR is None else ratioR
    w = e * rl[:, None, :] * rr[:, :, None]
    return dict(ratioL=pl, ratioR=pr, suml=suml, esum=e.sum(1), remL=remL, remR=remR, w=w,
                remR_next=torch.clamp(remR - sumr, min=0.0), remL_next=torch.clamp(remL - w.sum(1), min=0.0))


def _start(xyz1, xyz2, dt):
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    multiL, multiR = emd_multi(n, m)
    d = sqdist(xyz2, xyz1, dt)                                        # (B, m, n): match's layout, [l, k]
    return d, torch.full((B, n), multiL, dtype=dt, device=xyz1.device), torch.full((B, m), multiR, dtype=dt, device=xyz1.device)


def emd_auction(xyz1, xyz2, dt, fast_exp=False):
    """The whole auction in dt -> match (B, m, n), ratioL (10, B, n), ratioR (10, B, m), cost (B,)."""
    d, remL, remR = _start(xyz1, xyz2, dt)
    match, RL, RR = torch.zeros_like(d), [], []
    for it in range(len(LEVELS)):
        s = _level(d, it, remL, remR, fast_exp=fast_exp)
        match = match + s["w"]
        RL.append(s["ratioL"]); RR.append(s["ratioR"])
        remL, remR = s["remL_next"], s["remR_next"]
    return dict(match=match, ratioL=torch.stack(RL), ratioR=torch.stack(RR), cost=(d * match).sum((1, 2)))


def emd_one_step(xyz1, xyz2, ratioL, ratioR, dt):
    """Each level from the remains that the GIVEN factors (10, B, n) / (10, B, m) leave, everything in dt -> the level's own ratioL / ratioR
    (what the passes give from those remains), suml and esum = sum_l e for the conditioning, the remains before each level, and the match
    of the given factors."""
    d, remL, remR = _start(xyz1, xyz2, dt)
    gl, gr = ratioL.to(dt), ratioR.to(dt)
    match, out = torch.zeros_like(d), {k: [] for k in ("ratioL", "ratioR", "suml", "esum", "remL", "remR")}
    for it in range(len(LEVELS)):
        s = _level(d, it, remL, remR, gl[it], gr[it])
        match = match + s["w"]
        for k in out:
            out[k].append(s[k])
        remL, remR = s["remL_next"], s["remR_next"]
    out = {k: torch.stack(v) for k, v in out.items()}
    out["match"] = match
    return out


def emd_residuals(step64, ratioL, ratioR, n, m):
    """The two normalised residuals of factors (10, B, n) / (10, B, m) against the float64 one-step recipe, in float64 -- judged against 0:
        resL = (ratioL suml64 - remL64) / (multiL + ratioL multiR sum_l e)      the plain difference is ill-conditioned wherever suml is
                                                                               made of nearly exhausted columns
        resR = (ratioR - ratioR64) / multiR"""
    multiL, multiR = emd_multi(n, m)
    x, y = ratioL.double(), ratioR.double()
    return dict(ratioL=(x * step64["suml"] - step64["remL"]) / (multiL + x * multiR * step64["esum"]), ratioR=(y - step64["ratioR"]) / multiR)


def emd_matchcost(xyz1, xyz2, match, gc, dt):
    """cost (B,), grad1 (B, n, 3), grad2 (B, m, 3) for a GIVEN match (B, m, n) and upstream gc (B,)."""
    a, b, mt = xyz1.to(dt), xyz2.to(dt), match.to(dt)
    cost = (sqdist(xyz2, xyz1, dt) * mt).sum((1, 2))
    w = (mt * 2)[..., None] * (a[:, None, :, :] - b[:, :, None, :])             # (B, m, n, 3): 2 match[l, k] (xyz1_k - xyz2_l)
    g = gc.to(dt).view(-1, 1, 1)
    return dict(cost=cost, grad1=w.sum(1) * g, grad2=-w.sum(2) * g)
