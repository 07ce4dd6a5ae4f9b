"""pytorch3d.ops.knn_points / knn_gather with upstream's signatures, served by upp_hip (include/upp_hip.h "the pytorch3d.ops surface").

CPU tensors raise unless the opt-in torch formulations are on (upp_hip.torch_cpu.enable() / UPP_TORCH_CPU=1), as everywhere in this
tree.  There is no slower path behind the kernels: D > 32 or K > 64 is an error that names the limit."""
from collections import namedtuple

from upp_hip import functional as _F

_KNN = namedtuple("KNN", "dists idx knn")


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True):
    """K nearest neighbours in p2 of every point of p1.

    p1 (N,P1,D), p2 (N,P2,D); lengths1 / lengths2: None, an int64 tensor (N,) on the points' device, or a CPU tensor / list (uploaded).
    The lengths are applied by the kernel (clamped to [0, P]) and never read back, so the call does not synchronise and can be captured
    into a graph -- upstream takes lengths2.min() on the host.

    Returns the namedtuple (dists, idx, knn):
      dists (N,P1,K) f32: SQUARED L2 distances for norm=2, L1 distances for norm=1 (no square root, as upstream); differentiable w.r.t.
            p1 and p2.
      idx   (N,P1,K) int64, non-differentiable: neighbours in ascending (distance, index).
      knn   (N,P1,K,D) = knn_gather(p2, idx, lengths2) if return_nn, else None; differentiable w.r.t. p2.
    Slots k >= min(K, lengths2[n]) hold dists 0, idx 0 and knn 0.  Rows i >= lengths1[n] are zero in all three outputs (upstream's
    gather of its zero index puts p2[n, 0] into knn there: a deliberate deviation).

    version is accepted and ignored (one kernel serves every shape).  return_sorted=False returns the same sorted lists: any order is a
    valid "unsorted" answer, and the sorted one costs nothing extra here.
    Raises ValueError for a norm outside {1, 2} and for p1 / p2 that disagree in N or D; RuntimeError beyond 1 <= D <= 32, 1 <= K <= 64."""
    return _KNN(*_F.knn_points(p1, p2, lengths1, lengths2, norm=norm, K=K, version=version, return_nn=return_nn,
                               return_sorted=return_sorted))


def knn_gather(x, idx, lengths=None):
    """x (N,M,U), idx (N,L,K) int64 (as knn_points returns it), lengths (N,) | None -> (N,L,K,U) = x[n, idx[n,l,k]]; slots k >= lengths[n]
    are zero.  Differentiable w.r.t. x."""
    return _F.knn_gather(x, idx, lengths)
