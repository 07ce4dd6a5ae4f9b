"""numpy restatement of include/upp_hip.h "broadcast expand" (csrc/expand.hip), shared by tests/test_expand_host.py and
tests/test_gpu_expand.py.  y is built with the header's f32 operations (one product, fma in ascending j, one addition), so without a
norm the result has the kernel's bits; the normalised path is evaluated in float64 from float64 operands."""
import numpy as np

from _knn_points_reference import fma32

F = np.float32


def y32(P, U, Wu):
    """y (R,S,O) f32 by the header's rule: t = U[.,s,0] * Wu[o,0]; t = fma(U[.,s,j], Wu[o,j], t) for ascending j; y = P[r,o] + t."""
    P, U, Wu = (np.asarray(v, F) for v in (P, U, Wu))
    R, O = P.shape
    if U.ndim == 2:
        U = np.broadcast_to(U[None], (R,) + U.shape)
    J = U.shape[2]
    u = [np.broadcast_to(U[:, :, j, None], U.shape[:2] + (O,)) for j in range(J)]
    w = [np.broadcast_to(Wu[None, None, :, j], U.shape[:2] + (O,)) for j in range(J)]
    t = (u[0] * w[0]).astype(F)
    for j in range(1, J):
        t = fma32(u[j], w[j], t)
    return (P[:, None, :] + t).astype(F)


def lrelu(z, slope):
    return np.where(z > 0, z, z * z.dtype.type(slope))


def forward(P, U, Wu, slope=0.0):
    """No norm: h (R,S,O) f32, the kernel's bits."""
    return lrelu(y32(P, U, Wu), slope).astype(F)


def forward_f64(P, U, Wu, gamma, beta, eps, slope, mean=None, var=None):
    """The normalised path in float64 from float64 operands -> (h, mean, rstd, y).  mean / var None: the batch statistics (biased
    variance over all R S values per channel); given: the running buffers of eval mode."""
    P, U, Wu = (np.asarray(v, np.float64) for v in (P, U, Wu))
    if U.ndim == 2:
        U = np.broadcast_to(U[None], (P.shape[0],) + U.shape)
    y = P[:, None, :] + U @ Wu.T
    if mean is None:
        mean, var = y.mean(axis=(0, 1)), y.var(axis=(0, 1))
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    rstd = 1.0 / np.sqrt(var + eps)
    z = (y - mean) * rstd * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return lrelu(z, slope), mean, rstd, y
