"""Torch-facing operators over the C ABI (include/upp_hip.h).

Each function validates its tensors the way the reference extensions do
(device, dtype, contiguity, shape), allocates outputs with torch (the library
never allocates), and enqueues the HIP kernels on torch's current stream.
CPU tensors raise: there is no fallback path.
"""
import os

import torch

from . import _abi, _derived


def _need(t, name, dtype, ndim=None, last=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a HIP (cuda) tensor; upp_hip has no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError(f"{name} must have {ndim} dims, got {tuple(t.shape)}")
    if last is not None and t.shape[-1] != last:
        raise RuntimeError(f"{name} last dim must be {last}, got {tuple(t.shape)}")


def _need_f32(t, name, shape, optional=False):
    """_need for an f32 operand of exactly `shape`; None passes where the operand is optional.  Metadata only: no synchronisation, no copy."""
    if t is None and optional:
        return
    _need(t, name, torch.float32)
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")


def _same_device(*ts):
    d = ts[0].device
    for t in ts[1:]:
        if t.device != d:
            raise RuntimeError("all tensors must be on the same device")


def _call(dev, name, *args):
    """Enqueue one C-ABI entry point on `dev`'s current stream; raise on a non-zero status."""
    with torch.cuda.device(dev):
        _abi.check(getattr(_abi.load(), name)(*args, _abi.stream()))


# ------------------------------------------------------------------ FPS / gather
import threading

_FPS_FORM = threading.local()          # .form: bits 8-12 of upp_fps_ex's `waves` (clouds per workgroup, whole-LDS reservation); per THREAD


def _fps_form_bits():
    return getattr(_FPS_FORM, "form", 0)


class fps_form:
    """with ops.fps_form(2, True): ... -- FPS launches of THIS thread inside pack `clouds` (1 / 2 / 4) clouds into a workgroup and, with
    `exclusive`, reserve their CUs' whole LDS.  Same indices.  For a stream that runs BESIDE another one (the pipelined step's front-end): a
    32-cloud FPS that shares 32 CUs with the other stream's workgroups slows every one-round GEMM of that stream for as long as it is resident;
    16 CUs of its own cost the FPS 11 % and return 1.5 % of the step (tools/micro/fps_cpw_ab.sh).  Stand-alone the spread form is the faster
    one: the default.  The form is thread-local: another thread's FPS calls issued meanwhile keep their own."""

    def __init__(self, clouds, exclusive=False):
        if clouds not in (1, 2, 4):
            raise ValueError("clouds per workgroup: 1, 2 or 4")
        self.form = (int(clouds) << 8) | (0x1000 if exclusive else 0)

    def __enter__(self):
        self.prev = _fps_form_bits()
        _FPS_FORM.form = self.form

    def __exit__(self, *exc):
        _FPS_FORM.form = self.prev
        return False


class option:
    """with ops.option("EMBED_SPLIT_BF16", 0): ... -- one of the library's four documented process-wide options (include/upp_hip.h
    upp_set_option: SB_TUNED, SB_XCD2D, STORE_WT, EMBED_SPLIT_BF16) set for the duration of the block; tests and A/B measurements."""

    def __init__(self, name, value):
        self.key, self.value = _abi.OPTIONS[name], int(value)

    def __enter__(self):
        lib = _abi.load()
        self.prev = int(lib.upp_get_option(self.key))
        _abi.check(lib.upp_set_option(self.key, self.value))

    def __exit__(self, *exc):
        _abi.check(_abi.load().upp_set_option(self.key, self.prev))
        return False


def get_option(name):
    return int(_abi.load().upp_get_option(_abi.OPTIONS[name]))


def fps(xyz, npoint, want_centers=False, waves=0):
    """(B,N,3) f32 -> idx (B,npoint) int32 [, centers (B,npoint,3)].  waves: wavefronts per cloud (0 = the library's choice).
    Precondition: finite coordinates (include/upp_hip.h upp_fps: with a NaN in a cloud the indices stay in range but need not be the
    reference kernel's; not checked here -- a check would be a host synchronisation on the hot path)."""
    _need(xyz, "xyz", torch.float32, 3, 3)
    B, N, _ = xyz.shape
    npoint = int(npoint)
    idx = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
    centers = torch.empty((B, npoint, 3), dtype=torch.float32, device=xyz.device) if want_centers else None
    if B == 0:                               # an empty batch: nothing to launch (an empty tensor has no device pointer to hand over)
        return (idx, centers) if want_centers else idx
    _call(xyz.device, "upp_fps_ex", _abi.ptr(xyz), _abi.ptr(idx), _abi.ptr(centers), B, N, npoint, int(waves) | _fps_form_bits())
    return (idx, centers) if want_centers else idx


FPS_MAX_POINTS = 32768          # include/upp_hip.h upp_fps / upp_fps_ragged: 15-bit point ids


def ragged_layout(lengths, total=None, max_len=None, fps=True):
    """Host-side layout of a packed batch: lengths (a sequence or a CPU tensor of B ints) -> (offsets (B+1,) int64 CPU tensor, max_len).
    Raises -- before anything is launched -- on an empty cloud, on lengths that do not sum to `total`, on a length above the promised
    `max_len`, and (for the sampling kernel) on max_len > 32768.  Never touches a device."""
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda:
            raise RuntimeError("lengths must be known on the host (a sequence or a CPU tensor): reading them from the device would synchronise")
        lengths = lengths.reshape(-1).tolist()
    lengths = [int(n) for n in lengths]
    if any(n < 1 for n in lengths):
        raise ValueError("ragged batch: cloud %d is empty (every cloud needs at least one point)" % [n < 1 for n in lengths].index(True))
    longest = max(lengths, default=1)
    if max_len is None:
        max_len = longest
    max_len = int(max_len)
    if longest > max_len:
        raise ValueError("ragged batch: a cloud of %d points, max_len = %d" % (longest, max_len))
    if fps and max_len > FPS_MAX_POINTS:
        raise ValueError("ragged batch: max_len = %d, furthest point sampling serves clouds of at most %d points" % (max_len, FPS_MAX_POINTS))
    if total is not None and sum(lengths) != int(total):
        raise ValueError("ragged batch: the lengths sum to %d, the packed array has %d points" % (sum(lengths), int(total)))
    offsets = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    if lengths:
        offsets[1:] = torch.tensor(lengths, dtype=torch.int64).cumsum(0)
    return offsets, max_len


def _ragged_args(xyz, dtypes, offsets, max_len, lengths, fps):
    """The checks of the two packed-batch operators.  offsets: a CPU int64 tensor (checked here, then uploaded) or a device tensor (its
    CONTENT is the caller's promise unless `lengths` -- host -- is given too: reading it back would synchronise).  -> (offsets on the device, B)."""
    if not isinstance(xyz, torch.Tensor):
        raise TypeError("xyz must be a torch.Tensor")
    if not xyz.is_cuda:
        raise RuntimeError("xyz must be a HIP (cuda) tensor; upp_hip has no CPU path")
    if xyz.dtype not in dtypes:
        raise RuntimeError(f"xyz must be {' or '.join(str(d) for d in dtypes)}, got {xyz.dtype}")
    if not xyz.is_contiguous():
        raise RuntimeError("xyz must be contiguous")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError(f"xyz must be a packed (T, 3) array, got {tuple(xyz.shape)}")
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise RuntimeError("offsets must be a 1-D int64 tensor of B + 1 entries")
    if not offsets.is_contiguous():
        raise RuntimeError("offsets must be contiguous")
    max_len = int(max_len)
    if max_len < 1 or (fps and max_len > FPS_MAX_POINTS):
        raise ValueError("max_len = %d: must be in [1, %d]" % (max_len, FPS_MAX_POINTS) if fps else "max_len = %d: must be positive" % max_len)
    B = offsets.numel() - 1
    if not offsets.is_cuda:
        if int(offsets[0]) != 0:
            raise ValueError("offsets must start at 0")
        lengths = (offsets[1:] - offsets[:-1]).tolist()
    if lengths is not None:
        host, _ = ragged_layout(lengths, xyz.shape[0], max_len, fps)
        if host.numel() != B + 1:
            raise ValueError("offsets hold %d clouds, lengths %d" % (B, host.numel() - 1))
    if not offsets.is_cuda:
        offsets = offsets.to(xyz.device, non_blocking=True)
    elif offsets.device != xyz.device:
        raise RuntimeError("all tensors must be on the same device")
    return offsets, B, max_len


def fps_ragged(xyz, offsets, max_len, npoint, want_centers=False, lengths=None):
    """Furthest point sampling of every cloud of a packed batch in ONE launch (include/upp_hip.h upp_fps_ragged).
    xyz (T,3) f32: the clouds back to back; offsets (B+1,) int64; max_len >= every length (host int) -> idx (B,npoint) int32, local to
    each cloud and bit-identical to fps(cloud[None], npoint) [, centers (B,npoint,3)]."""
    offsets, B, max_len = _ragged_args(xyz, (torch.float32,), offsets, max_len, lengths, True)
    npoint = int(npoint)
    if npoint < 1:
        raise ValueError("npoint must be positive")
    idx = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
    centers = torch.empty((B, npoint, 3), dtype=torch.float32, device=xyz.device) if want_centers else None
    if B > 0:
        _call(xyz.device, "upp_fps_ragged", _abi.ptr(xyz), _abi.ptr(offsets), _abi.ptr(idx), _abi.ptr(centers), B, max_len, npoint)
    return (idx, centers) if want_centers else idx


def cloud_norm_ragged(xyz, offsets, max_len, want_scale=False, lengths=None):
    """The reference's pc_norm (datasets/RealSensorDataset.py:59-65) of every cloud of a packed batch in ONE launch: xyz (T,3) f64 (or f32:
    upcast first) -> (T,3) f32 = (float)(p / (2 max |p|)), float64 arithmetic, the bits of the numpy expression [, scale (B,) f64]."""
    offsets, B, max_len = _ragged_args(xyz, (torch.float64, torch.float32), offsets, max_len, lengths, False)
    out = torch.empty(xyz.shape, dtype=torch.float32, device=xyz.device)
    scale = torch.empty((B,), dtype=torch.float64, device=xyz.device) if want_scale else None
    if B > 0:
        name = "upp_cloud_norm_ragged" if xyz.dtype == torch.float64 else "upp_cloud_norm_ragged_f32"
        _call(xyz.device, name, _abi.ptr(xyz), _abi.ptr(offsets), _abi.ptr(out), _abi.ptr(scale), B, max_len)
    return (out, scale) if want_scale else out


def gather_fwd(features, idx):
    _need(features, "features", torch.float32, 3)
    _need(idx, "idx", torch.int32, 2)
    _same_device(features, idx)
    B, C, N = features.shape
    M = idx.shape[1]
    out = torch.empty((B, C, M), dtype=torch.float32, device=features.device)
    _call(features.device, "upp_gather_fwd", _abi.ptr(features), _abi.ptr(idx), _abi.ptr(out), B, C, N, M)
    return out


def _scatter_target(grad_out, shape, name, deterministic):
    """-> the f32 array a scatter-add backward fills and the entry point that fills it: zeros for the f32 atomics of `name`, an
    uninitialised array for `name`_det, which writes every element."""
    if deterministic:
        return torch.empty(shape, dtype=torch.float32, device=grad_out.device), name + "_det"
    return torch.zeros(shape, dtype=torch.float32, device=grad_out.device), name


def gather_bwd(grad_out, idx, N, deterministic=False):
    """deterministic: the sums in ascending source index (upp_gather_bwd_det, include/upp_hip.h) instead of f32 atomics."""
    _need(grad_out, "grad_out", torch.float32, 3)
    _need(idx, "idx", torch.int32, 2)
    B, C, M = grad_out.shape
    grad, name = _scatter_target(grad_out, (B, C, N), "upp_gather_bwd", deterministic)
    if deterministic and not (B and C):
        return grad                                      # (nothing to write; the atomic entry point is called, and checks N, even so)
    _call(grad_out.device, name, _abi.ptr(grad_out), _abi.ptr(idx), _abi.ptr(grad), B, C, N, M)
    return grad


# ------------------------------------------------------------------ kNN / group
def knn(ref, query, k, want_dist=True, want_neigh=False, prefilter=True):
    """ref (B,N,3), query (B,Q,3) -> dist (B,Q,k) f32 | None, idx (B,Q,k) int64 [, neigh (B,Q,k,3)]."""
    _need(ref, "ref", torch.float32, 3, 3)
    _need(query, "query", torch.float32, 3, 3)
    _same_device(ref, query)
    B, N, _ = ref.shape
    Q = query.shape[1]
    if query.shape[0] != B:
        raise RuntimeError("ref and query batch sizes differ")
    k = int(k)
    idx = torch.empty((B, Q, k), dtype=torch.int64, device=ref.device)
    dist = torch.empty((B, Q, k), dtype=torch.float32, device=ref.device) if want_dist else None
    neigh = torch.empty((B, Q, k, 3), dtype=torch.float32, device=ref.device) if want_neigh else None
    if B == 0:
        if k < 1 or k > min(N, 64):
            raise RuntimeError("knn: k must be in [1, min(N, 64)]")
        return dist, idx, neigh
    _call(ref.device, "upp_knn_ex", _abi.ptr(ref), _abi.ptr(query), _abi.ptr(dist), _abi.ptr(idx), _abi.ptr(neigh), B, N, Q, k, int(bool(prefilter)))
    return dist, idx, neigh


def group_fwd(xyz, center, idx):
    _need(xyz, "xyz", torch.float32, 3, 3)
    _need(center, "center", torch.float32, 3, 3)
    _need(idx, "idx", torch.int64, 3)
    _same_device(xyz, center, idx)
    B, N, _ = xyz.shape
    _, G, K = idx.shape
    out = torch.empty((B, G, K, 3), dtype=torch.float32, device=xyz.device)
    _call(xyz.device, "upp_group_fwd", _abi.ptr(xyz), _abi.ptr(center), _abi.ptr(idx), _abi.ptr(out), B, N, G, K)
    return out


def group_bwd(grad_out, idx, N, need_xyz=True, need_center=True, deterministic=False):
    """deterministic: grad_xyz summed in ascending g * K + k (upp_group_bwd_det, include/upp_hip.h) instead of f32 atomics."""
    _need(grad_out, "grad_out", torch.float32, 4, 3)
    _need(idx, "idx", torch.int64, 3)
    B, G, K = idx.shape
    if deterministic:
        gx = torch.empty((B, N, 3), dtype=torch.float32, device=grad_out.device) if need_xyz else None      # (overwritten in full)
        gc = torch.empty((B, G, 3), dtype=torch.float32, device=grad_out.device) if need_center else None
        if B:
            _call(grad_out.device, "upp_group_bwd_det", _abi.ptr(grad_out), _abi.ptr(idx), _abi.ptr(gx), _abi.ptr(gc), B, N, G, K)
        return gx, gc
    gx = torch.zeros((B, N, 3), dtype=torch.float32, device=grad_out.device) if need_xyz else None
    gc = torch.empty((B, G, 3), dtype=torch.float32, device=grad_out.device) if need_center else None
    _call(grad_out.device, "upp_group_bwd", _abi.ptr(grad_out), _abi.ptr(idx), _abi.ptr(gx), _abi.ptr(gc), B, N, G, K)
    return gx, gc


def fps_gather_bwd(grad_centers, idx, N, deterministic=False):
    """Gradient of the FPS centre gather: grad_centers (B,M,3), idx (B,M) int32 -> (B,N,3) (upp_fps_gather_bwd: one launch).
    deterministic: repeated indices summed in ascending j (upp_fps_gather_bwd_det)."""
    _need(grad_centers, "grad_centers", torch.float32, 3, 3)
    _need(idx, "idx", torch.int32, 2)
    B, M = idx.shape
    if tuple(grad_centers.shape) != (B, M, 3):
        raise RuntimeError("fps_gather_bwd: grad_centers must be (B, M, 3) for idx (B, M)")
    gx = torch.empty((B, int(N), 3), dtype=torch.float32, device=grad_centers.device)
    if B:
        _call(grad_centers.device, "upp_fps_gather_bwd_det" if deterministic else "upp_fps_gather_bwd", _abi.ptr(grad_centers), _abi.ptr(idx), _abi.ptr(gx), B, int(N), M)
    return gx


# ------------------------------------------------------------------ the pointnet2_ops surface (include/upp_hip.h)
def ball_query(radius, nsample, xyz, new_xyz):
    """xyz (B,N,3), new_xyz (B,P,3) -> idx (B,P,nsample) int32: the first nsample points (ascending index) strictly inside `radius` of each
    query, the first hit filling every slot first, zeros for a query without a hit (upp_ball_query).  Every element is written by the kernel."""
    _need(xyz, "xyz", torch.float32, 3, 3)
    _need(new_xyz, "new_xyz", torch.float32, 3, 3)
    _same_device(xyz, new_xyz)
    B, N, _ = xyz.shape
    P = new_xyz.shape[1]
    if new_xyz.shape[0] != B:
        raise RuntimeError("xyz and new_xyz batch sizes differ")
    radius, nsample = float(radius), int(nsample)
    if not (radius > 0.0 and radius != float("inf")) or nsample < 1:
        raise ValueError("ball_query: radius must be finite and positive, nsample positive")
    idx = torch.empty((B, P, nsample), dtype=torch.int32, device=xyz.device)
    if B:
        _call(xyz.device, "upp_ball_query", _abi.ptr(xyz), _abi.ptr(new_xyz), radius, nsample, _abi.ptr(idx), B, N, P)
    return idx


def three_nn(unknown, known):
    """unknown (B,n,3), known (B,m,3) -> dist (B,n,3) f32 Euclidean distances ascending, idx (B,n,3) int32 (ties: lower index first; with
    m < 3 the unfilled slots are index 0 / +inf): upp_three_nn."""
    _need(unknown, "unknown", torch.float32, 3, 3)
    _need(known, "known", torch.float32, 3, 3)
    _same_device(unknown, known)
    B, n, _ = unknown.shape
    m = known.shape[1]
    if known.shape[0] != B:
        raise RuntimeError("unknown and known batch sizes differ")
    dist = torch.empty((B, n, 3), dtype=torch.float32, device=unknown.device)
    idx = torch.empty((B, n, 3), dtype=torch.int32, device=unknown.device)
    if B:
        _call(unknown.device, "upp_three_nn", _abi.ptr(unknown), _abi.ptr(known), _abi.ptr(dist), _abi.ptr(idx), B, n, m)
    return dist, idx


def _interp_args(dense, idx, weight):
    _need(dense, "features", torch.float32, 3)
    _need(idx, "idx", torch.int32, 3, 3)
    _need(weight, "weight", torch.float32, 3, 3)
    _same_device(dense, idx, weight)
    if idx.shape != weight.shape or idx.shape[0] != dense.shape[0]:
        raise RuntimeError("three_interpolate: idx and weight must both be (B, n, 3) for features (B, C, m)")


def three_interpolate_fwd(features, idx, weight):
    """features (B,C,m), idx (B,n,3) int32, weight (B,n,3) -> (B,C,n) = (w0 f[i0] + w1 f[i1]) + w2 f[i2], every operation rounded once."""
    _interp_args(features, idx, weight)
    B, C, m = features.shape
    n = idx.shape[1]
    out = torch.empty((B, C, n), dtype=torch.float32, device=features.device)
    if B:
        _call(features.device, "upp_three_interpolate_fwd", _abi.ptr(features), _abi.ptr(idx), _abi.ptr(weight), _abi.ptr(out), B, C, m, n)
    return out


def three_interpolate_bwd(grad_out, idx, weight, m, deterministic=False):
    """grad_out (B,C,n) -> grad_features (B,C,m).  deterministic: the sums in ascending i * 3 + j (upp_three_interpolate_bwd_det,
    include/upp_hip.h) instead of f32 atomics."""
    _interp_args(grad_out, idx, weight)
    B, C, n = grad_out.shape
    if idx.shape[1] != n:
        raise RuntimeError("three_interpolate_bwd: grad_out must be (B, C, n) for idx (B, n, 3)")
    m = int(m)
    grad, name = _scatter_target(grad_out, (B, C, m), "upp_three_interpolate_bwd", deterministic)
    if B:
        _call(grad_out.device, name, _abi.ptr(grad_out), _abi.ptr(idx), _abi.ptr(weight), _abi.ptr(grad), B, C, m, n)
    return grad


def grouping_fwd(features, idx):
    """features (B,C,N), idx (B,P,S) int32 -> (B,C,P,S) = features[b, c, idx[b, p, s]] (upp_grouping_fwd)."""
    _need(features, "features", torch.float32, 3)
    _need(idx, "idx", torch.int32, 3)
    _same_device(features, idx)
    B, C, N = features.shape
    _, P, S = idx.shape
    if idx.shape[0] != B:
        raise RuntimeError("features and idx batch sizes differ")
    out = torch.empty((B, C, P, S), dtype=torch.float32, device=features.device)
    if B:
        _call(features.device, "upp_grouping_fwd", _abi.ptr(features), _abi.ptr(idx), _abi.ptr(out), B, C, N, P, S)
    return out


def grouping_bwd(grad_out, idx, N, deterministic=False):
    """grad_out (B,C,P,S) -> grad_features (B,C,N).  deterministic: the sums in ascending p * S + s (upp_grouping_bwd_det,
    include/upp_hip.h) instead of f32 atomics."""
    _need(grad_out, "grad_out", torch.float32, 4)
    _need(idx, "idx", torch.int32, 3)
    _same_device(grad_out, idx)
    B, C, P, S = grad_out.shape
    if tuple(idx.shape) != (B, P, S):
        raise RuntimeError("grouping_bwd: grad_out must be (B, C, P, S) for idx (B, P, S)")
    N = int(N)
    grad, name = _scatter_target(grad_out, (B, C, N), "upp_grouping_bwd", deterministic)
    if B:
        _call(grad_out.device, name, _abi.ptr(grad_out), _abi.ptr(idx), _abi.ptr(grad), B, C, N, P, S)
    return grad


# ------------------------------------------------------------------ the pytorch3d.ops surface (include/upp_hip.h)
KNN_POINTS_MAX_D, KNN_POINTS_MAX_K = 32, 64


def _lengths(lengths, N, dev, name):
    """None | a device int64 tensor (N,) | a CPU tensor or a sequence (uploaded) -> a device int64 tensor or None.  Its CONTENT is never
    read here: the kernels clamp it to the array's extent (reading it back would synchronise)."""
    if lengths is None:
        return None
    if not isinstance(lengths, torch.Tensor):
        lengths = torch.as_tensor(lengths, dtype=torch.int64)
    if lengths.dim() != 1 or lengths.numel() != N:
        raise ValueError(f"{name} must hold one length per cloud: ({N},), got {tuple(lengths.shape)}")
    if lengths.is_cuda:
        if lengths.device != dev:
            raise RuntimeError("all tensors must be on the same device")
        if lengths.dtype != torch.int64:
            raise RuntimeError(f"{name} must be torch.int64 on the device, got {lengths.dtype}")
        return lengths.contiguous()
    return lengths.to(torch.int64).to(dev, non_blocking=True)


def _knn_points_args(p1, p2, K, norm):
    _need(p1, "p1", torch.float32, 3)
    _need(p2, "p2", torch.float32, 3)
    _same_device(p1, p2)
    if norm not in (1, 2):
        raise ValueError("knn_points: norm must be 1 or 2")
    if p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise ValueError("knn_points: p1 (N,P1,D) and p2 (N,P2,D) must agree in N and D, got %s and %s" % (tuple(p1.shape), tuple(p2.shape)))
    N, P1, D = p1.shape
    K = int(K)
    if not (1 <= D <= KNN_POINTS_MAX_D) or not (1 <= K <= KNN_POINTS_MAX_K):
        # what the library answers with UPP_E_RANGE, said with the limit's name (there is no slower path to fall back to)
        raise RuntimeError("knn_points: D = %d, K = %d is outside the served range 1 <= D <= %d, 1 <= K <= %d (UPP_E_RANGE)"
                           % (D, K, KNN_POINTS_MAX_D, KNN_POINTS_MAX_K))
    if P1 < 1 or p2.shape[1] < 1:
        raise ValueError("knn_points: p1 and p2 need at least one point per cloud (ragged batches: lengths1 / lengths2)")
    return N, P1, p2.shape[1], D, K


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, norm=2, want_nn=False):
    """p1 (N,P1,D), p2 (N,P2,D) -> dists (N,P1,K) f32 (squared L2 / L1), idx (N,P1,K) int64, nn (N,P1,K,D) | None: the K nearest p2
    points of every p1 point in ascending (distance, index); zeros in slots k >= min(K, lengths2) and rows i >= lengths1
    (upp_knn_points: one launch that writes every element, lengths applied on the device)."""
    N, P1, P2, D, K = _knn_points_args(p1, p2, K, norm)
    dev = p1.device
    lengths1, lengths2 = _lengths(lengths1, N, dev, "lengths1"), _lengths(lengths2, N, dev, "lengths2")
    dists = torch.empty((N, P1, K), dtype=torch.float32, device=dev)
    idx = torch.empty((N, P1, K), dtype=torch.int64, device=dev)
    nn = torch.empty((N, P1, K, D), dtype=torch.float32, device=dev) if want_nn else None
    if N:
        _call(dev, "upp_knn_points", _abi.ptr(p1), _abi.ptr(p2), _abi.ptr(lengths1), _abi.ptr(lengths2), _abi.ptr(dists), _abi.ptr(idx),
              _abi.ptr(nn), N, P1, P2, D, K, int(norm))
    return dists, idx, nn


def knn_points_bwd(p1, p2, idx, grad_dists, lengths1=None, lengths2=None, norm=2):
    """-> g_p1 (N,P1,D) summed over k ascending, t (N,P1,K,D) the per-slot terms (zero in padded slots); the gradient of p2 is
    knn_scatter_add(t, idx, P2, ..., negate=True) (upp_knn_points_bwd)."""
    _need(idx, "idx", torch.int64, 3)
    _need(grad_dists, "grad_dists", torch.float32, 3)
    N, P1, P2, D, K = _knn_points_args(p1, p2, idx.shape[2], norm)
    _same_device(p1, idx, grad_dists)
    if tuple(idx.shape) != (N, P1, K) or tuple(grad_dists.shape) != (N, P1, K):
        raise RuntimeError("knn_points_bwd: idx and grad_dists must both be (N, P1, K)")
    dev = p1.device
    lengths1, lengths2 = _lengths(lengths1, N, dev, "lengths1"), _lengths(lengths2, N, dev, "lengths2")
    g_p1 = torch.empty((N, P1, D), dtype=torch.float32, device=dev)
    t = torch.empty((N, P1, K, D), dtype=torch.float32, device=dev)
    if N:
        _call(dev, "upp_knn_points_bwd", _abi.ptr(p1), _abi.ptr(p2), _abi.ptr(idx), _abi.ptr(grad_dists), _abi.ptr(lengths1),
              _abi.ptr(lengths2), _abi.ptr(g_p1), _abi.ptr(t), N, P1, P2, D, K, int(norm))
    return g_p1, t


def knn_gather(x, idx, lengths=None):
    """x (N,M,U), idx (N,L,K) int64 -> (N,L,K,U) = x[n, idx[n,l,k]], zeros in slots k >= lengths[n] (upp_knn_gather)."""
    _need(x, "x", torch.float32, 3)
    _need(idx, "idx", torch.int64, 3)
    _same_device(x, idx)
    N, M, U = x.shape
    if idx.shape[0] != N:
        raise ValueError("knn_gather: x and idx batch sizes differ")
    _, L, K = idx.shape
    lengths = _lengths(lengths, N, x.device, "lengths")
    out = torch.empty((N, L, K, U), dtype=torch.float32, device=x.device)
    if out.numel():
        if M < 1:
            raise ValueError("knn_gather: x has no rows to gather")
        _call(x.device, "upp_knn_gather", _abi.ptr(x), _abi.ptr(idx), _abi.ptr(lengths), _abi.ptr(out), N, M, L, K, U)
    return out


def knn_scatter_add(src, idx, M, rows=None, slots=None, negate=False, deterministic=False):
    """src (N,L,K,U), idx (N,L,K) int64 -> (N,M,U): src[n,l,k] added to (negate: subtracted from) row idx[n,l,k], over the slots with
    l < rows[n] and k < slots[n].  f32 atomics into an array the library zeroes with a kernel (upp_knn_scatter_add), or -- deterministic
    -- every row's sum in ascending l * K + k (upp_knn_scatter_add_det).  The gradient of p2 in knn_points and the backward of knn_gather."""
    _need(src, "src", torch.float32, 4)
    _need(idx, "idx", torch.int64, 3)
    _same_device(src, idx)
    N, L, K, U = src.shape
    if tuple(idx.shape) != (N, L, K):
        raise RuntimeError("knn_scatter_add: src must be (N, L, K, U) for idx (N, L, K)")
    M = int(M)
    rows, slots = _lengths(rows, N, src.device, "rows"), _lengths(slots, N, src.device, "slots")
    out = torch.empty((N, M, U), dtype=torch.float32, device=src.device)                 # (written in full by either entry point)
    if out.numel():
        if src.numel() == 0:
            raise ValueError("knn_scatter_add: an empty source list")
        _call(src.device, "upp_knn_scatter_add_det" if deterministic else "upp_knn_scatter_add", _abi.ptr(src), _abi.ptr(idx),
              _abi.ptr(rows), _abi.ptr(slots), _abi.ptr(out), N, M, L, K, U, int(bool(negate)))
    return out


# ------------------------------------------------------------------ edge convolution (include/upp_hip.h "edge convolution")
EDGE_CONV_MAX_K, EDGE_CONV_MAX_O = 64, 512


def edge_conv_usable(B, Nk, Nq, K, O, G=0):
    """The served range of upp_edge_conv_fwd / _bwd (sizes only)."""
    return (1 <= K <= EDGE_CONV_MAX_K and 1 <= O <= EDGE_CONV_MAX_O and (G == 0 or (G > 0 and O % G == 0)) and 0 <= B <= 65535 and Nk >= 1
            and 1 <= Nq < 2 ** 30 and Nq * K < 2 ** 31 and Nq * O < 2 ** 31 and Nk * O < 2 ** 31)


def _edge_conv_args(A, Bq, idx, gamma, beta, G):
    _need(A, "A", torch.float32, 3)
    _need(Bq, "Bq", torch.float32, 3)
    _need(idx, "idx", torch.int64, 3)
    _same_device(A, Bq, idx)
    B, Nk, O = A.shape
    _, Nq, K = idx.shape
    if tuple(Bq.shape) != (B, Nq, O) or idx.shape[0] != B:
        raise RuntimeError("edge_conv: A (B, Nk, O), Bq (B, Nq, O) and idx (B, Nq, K) do not fit together")
    G = int(G)
    if G:
        _need(gamma, "gamma", torch.float32, 1, O)
        _need(beta, "beta", torch.float32, 1, O)
        _same_device(A, gamma, beta)
    return B, Nk, Nq, K, O, G


def _edge_conv_work(A, B, Nq, O, G):
    return torch.empty(int(_abi.load().upp_edge_conv_work_floats(B, Nq, O)), dtype=torch.float32, device=A.device) if G else None


def edge_conv_fwd(A, Bq, idx, gamma=None, beta=None, groups=0, eps=1e-5, slope=0.2):
    """A (B,Nk,O), Bq (B,Nq,O), idx (B,Nq,K) int64 -> out (B,Nq,O) = max_k lrelu(GroupNorm(A[idx] + Bq)), arg (B,Nq,O) uint8,
    mean / rstd (B,G) | None (groups == 0: no norm).  y = A[idx] + Bq is never stored."""
    B, Nk, Nq, K, O, G = _edge_conv_args(A, Bq, idx, gamma, beta, groups)
    out = torch.empty((B, Nq, O), dtype=torch.float32, device=A.device)
    arg = torch.empty((B, Nq, O), dtype=torch.uint8, device=A.device)
    mean = torch.empty((B, G), dtype=torch.float32, device=A.device) if G else None
    rstd = torch.empty((B, G), dtype=torch.float32, device=A.device) if G else None
    work = _edge_conv_work(A, B, Nq, O, G)
    if B == 0:
        return out, arg, mean, rstd
    _call(A.device, "upp_edge_conv_fwd", _abi.ptr(A), _abi.ptr(Bq), _abi.ptr(idx), _abi.ptr(gamma if G else None),
          _abi.ptr(beta if G else None), float(eps), float(slope), G, _abi.ptr(out), _abi.ptr(arg), _abi.ptr(mean), _abi.ptr(rstd),
          _abi.ptr(work), B, Nk, Nq, K, O)
    return out, arg, mean, rstd


def edge_conv_bwd(g_out, A, Bq, idx, arg, gamma=None, beta=None, mean=None, rstd=None, groups=0, slope=0.2, deterministic=False):
    """-> g_A (B,Nk,O), g_Bq (B,Nq,O), g_gamma (O,) | None, g_beta (O,) | None.  g_A is summed by f32 atomics (into zeros written by a
    kernel), or -- deterministic -- in ascending q * K + k from a stored g_y (B,Nq,K,O); everything else has a fixed order in both modes."""
    B, Nk, Nq, K, O, G = _edge_conv_args(A, Bq, idx, gamma, beta, groups)
    _need(g_out, "g_out", torch.float32, 3)
    _need(arg, "arg", torch.uint8, 3)
    if tuple(g_out.shape) != (B, Nq, O) or tuple(arg.shape) != (B, Nq, O):
        raise RuntimeError("edge_conv_bwd: g_out and arg must be (B, Nq, O)")
    if G:
        _need(mean, "mean", torch.float32, 2, G)
        _need(rstd, "rstd", torch.float32, 2, G)
    g_A = torch.empty((B, Nk, O), dtype=torch.float32, device=A.device)
    g_Bq = torch.empty((B, Nq, O), dtype=torch.float32, device=A.device)
    g_gamma = torch.empty((O,), dtype=torch.float32, device=A.device) if G else None
    g_beta = torch.empty((O,), dtype=torch.float32, device=A.device) if G else None
    if B == 0:
        if G:
            g_gamma.zero_(); g_beta.zero_()
        return g_A, g_Bq, g_gamma, g_beta
    work = _edge_conv_work(A, B, Nq, O, G)
    g_y = torch.empty((B, Nq, K, O), dtype=torch.float32, device=A.device) if deterministic else None
    _call(A.device, "upp_edge_conv_bwd", _abi.ptr(g_out), _abi.ptr(A), _abi.ptr(Bq), _abi.ptr(idx), _abi.ptr(arg),
          _abi.ptr(gamma if G else None), _abi.ptr(beta if G else None), _abi.ptr(mean if G else None), _abi.ptr(rstd if G else None),
          float(slope), G, _abi.ptr(g_A), _abi.ptr(g_Bq), _abi.ptr(g_gamma), _abi.ptr(g_beta), _abi.ptr(work), _abi.ptr(g_y),
          B, Nk, Nq, K, O)
    return g_A, g_Bq, g_gamma, g_beta


# ------------------------------------------------------------------ broadcast expand (include/upp_hip.h "broadcast expand")
EXPAND_MAX_J, EXPAND_MAX_O = 4, 1024
EXPAND_NONE, EXPAND_TRAIN, EXPAND_EVAL = 0, 1, 2


def expand_usable(R, S, O, J):
    """The served range of upp_expand_fwd / _bwd (sizes only)."""
    return 1 <= J <= EXPAND_MAX_J and 1 <= O <= EXPAND_MAX_O and S >= 1 and R >= 1 and R * S * O < 2 ** 31


def _expand_args(P, U, Wu, gamma, beta, mean, rstd, mode, slope, stats_given):
    _need(P, "P", torch.float32, 2)
    _need(Wu, "Wu", torch.float32, 2)
    _need(U, "U", torch.float32)
    _same_device(P, U, Wu)
    R, O = P.shape
    J = Wu.shape[1]
    if U.dim() not in (2, 3) or U.shape[-1] != J or Wu.shape[0] != O or (U.dim() == 3 and U.shape[0] != R):
        raise RuntimeError("expand: P (R, O), U (S, J) or (R, S, J) and Wu (O, J) do not fit together")
    S = U.shape[-2]
    mode = int(mode)
    if mode not in (EXPAND_NONE, EXPAND_TRAIN, EXPAND_EVAL):
        raise ValueError("expand: mode must be 0 (no norm), 1 (training norm) or 2 (eval norm)")
    if not 0.0 <= float(slope) <= 1.0:
        raise ValueError("expand: slope must be in [0, 1]")
    if J > EXPAND_MAX_J or J < 1:
        raise RuntimeError("expand: 1 <= J <= %d is served, got J = %d" % (EXPAND_MAX_J, J))
    if O > EXPAND_MAX_O or O < 1:
        raise RuntimeError("expand: 1 <= O <= %d is served, got O = %d" % (EXPAND_MAX_O, O))
    if R < 1 or S < 1 or R * S * O >= 2 ** 31:
        raise RuntimeError("expand: R >= 1, S >= 1 and R S O < 2^31 are served, got R = %d, S = %d, O = %d" % (R, S, O))
    if mode:
        _need(gamma, "gamma", torch.float32, 1, O)
        _need(beta, "beta", torch.float32, 1, O)
        _same_device(P, gamma, beta)
        if stats_given:
            _need(mean, "mean", torch.float32, 1, O)
            _need(rstd, "rstd", torch.float32, 1, O)
            _same_device(P, mean, rstd)
    return R, S, O, J, mode, int(U.dim() == 3)


def _expand_work(P, R, S, O):
    return torch.empty(int(_abi.load().upp_expand_work_floats(R, S, O)), dtype=torch.float32, device=P.device)


def expand_fwd(P, U, Wu, gamma=None, beta=None, mean=None, rstd=None, mode=0, eps=1e-5, slope=0.0):
    """P (R,O), U (S,J) | (R,S,J), Wu (O,J) -> h (R,S,O) = lrelu(norm(P[r] + Wu U[.,s])), mean, var, rstd (O,) | None.  mode 0: no norm;
    1: batch statistics (mean, biased var, rstd are computed and returned); 2: the given mean / rstd.  y is never stored."""
    R, S, O, J, mode, per_row = _expand_args(P, U, Wu, gamma, beta, mean, rstd, mode, slope, mode == EXPAND_EVAL)
    if mode == EXPAND_TRAIN and R * S == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % ((R, S, O),))
    h = torch.empty((R, S, O), dtype=torch.float32, device=P.device)
    var = work = None
    if mode == EXPAND_TRAIN:
        mean, var, rstd = (torch.empty((O,), dtype=torch.float32, device=P.device) for _ in range(3))
        work = _expand_work(P, R, S, O)
    _call(P.device, "upp_expand_fwd", _abi.ptr(P), _abi.ptr(U), per_row, _abi.ptr(Wu), _abi.ptr(gamma if mode else None),
          _abi.ptr(beta if mode else None), float(eps), float(slope), mode, _abi.ptr(h), _abi.ptr(mean if mode else None), _abi.ptr(var),
          _abi.ptr(rstd if mode else None), _abi.ptr(work), R, S, O, J)
    return h, (mean if mode else None), var, (rstd if mode else None)


def expand_bwd(g_h, P, U, Wu, gamma=None, beta=None, mean=None, rstd=None, mode=0, slope=0.0, want_gU=True):
    """-> g_P (R,O), g_U (R,S,J) | None (a shared U, or not wanted), g_Wu (O,J), g_gamma (O,) | None, g_beta (O,) | None: every sum in a
    fixed order, nothing zeroed, g_y never stored."""
    R, S, O, J, mode, per_row = _expand_args(P, U, Wu, gamma, beta, mean, rstd, mode, slope, True)
    _need(g_h, "g_h", torch.float32, 3)
    _same_device(P, g_h)
    if tuple(g_h.shape) != (R, S, O):
        raise RuntimeError("expand_bwd: g_h must be (R, S, O)")
    if want_gU and not per_row:
        raise RuntimeError("expand_bwd: a shared U (S, J) has no gradient here")
    g_P = torch.empty((R, O), dtype=torch.float32, device=P.device)
    g_U = torch.empty((R, S, J), dtype=torch.float32, device=P.device) if want_gU else None
    g_Wu = torch.empty((O, J), dtype=torch.float32, device=P.device)
    g_gamma = torch.empty((O,), dtype=torch.float32, device=P.device) if mode else None
    g_beta = torch.empty((O,), dtype=torch.float32, device=P.device) if mode else None
    work = _expand_work(P, R, S, O)
    _call(P.device, "upp_expand_bwd", _abi.ptr(g_h), _abi.ptr(P), _abi.ptr(U), per_row, _abi.ptr(Wu), _abi.ptr(gamma if mode else None),
          _abi.ptr(beta if mode else None), _abi.ptr(mean if mode else None), _abi.ptr(rstd if mode else None), float(slope), mode,
          _abi.ptr(g_P), _abi.ptr(g_U), _abi.ptr(g_Wu), _abi.ptr(g_gamma), _abi.ptr(g_beta), _abi.ptr(work), R, S, O, J)
    return g_P, g_U, g_Wu, g_gamma, g_beta


# ------------------------------------------------------------------ query selection (include/upp_hip.h)
QUERY_SELECT_MAX_M = 4096


def query_select_usable(M, Q):
    return 1 <= Q <= M <= QUERY_SELECT_MAX_M


def _query_select_sizes(B, M, Q, D):
    if not 1 <= Q <= M:
        raise RuntimeError("query_select: 1 <= Q <= M is needed, got Q = %d, M = %d" % (Q, M))
    if M > QUERY_SELECT_MAX_M:
        raise RuntimeError("query_select: M <= %d is served, got M = %d" % (QUERY_SELECT_MAX_M, M))
    if B < 1 or 3 * B * (Q + D) >= 2 ** 31:
        raise RuntimeError("query_select: B >= 1 and 3 B (Q + D) < 2^31 are served, got B = %d, Q = %d, D = %d" % (B, Q, D))


def query_select_fwd(score, cand, Q, extra=None):
    """score (B,M), cand (B,M,3), extra (B,D,3) | None -> out (B,Q+D,3), order (B,Q) int32: the Q candidates of greatest score in
    descending order (equal scores by ascending index, NaN first), then the extra points."""
    _need(score, "score", torch.float32, 2)
    B, M = score.shape
    _need_f32(cand, "cand", (B, M, 3))
    _same_device(score, cand)
    D = 0
    if extra is not None:
        _need(extra, "extra", torch.float32, 3, 3)
        _same_device(score, extra)
        if extra.shape[0] != B:
            raise RuntimeError("query_select: extra must be (B, D, 3)")
        D = extra.shape[1]
    Q = int(Q)
    _query_select_sizes(B, M, Q, D)
    out = torch.empty((B, Q + D, 3), dtype=torch.float32, device=score.device)
    order = torch.empty((B, Q), dtype=torch.int32, device=score.device)
    _call(score.device, "upp_query_select_fwd", _abi.ptr(score), _abi.ptr(cand), _abi.ptr(extra if D else None), _abi.ptr(out),
          _abi.ptr(order), B, M, Q, D)
    return out, order


def query_select_bwd(g_out, order, M):
    """g_out (B,Q+D,3), order (B,Q) int32 -> g_cand (B,M,3) (every row written once), g_extra (B,D,3) | None."""
    _need(order, "order", torch.int32, 2)
    B, Q = order.shape
    _need(g_out, "g_out", torch.float32, 3, 3)
    _same_device(g_out, order)
    M = int(M)
    D = g_out.shape[1] - Q
    if g_out.shape[0] != B or D < 0:
        raise RuntimeError("query_select_bwd: g_out must be (B, Q + D, 3) for order (B, Q)")
    _query_select_sizes(B, M, Q, D)
    g_cand = torch.empty((B, M, 3), dtype=torch.float32, device=g_out.device)
    g_extra = torch.empty((B, D, 3), dtype=torch.float32, device=g_out.device) if D else None
    _call(g_out.device, "upp_query_select_bwd", _abi.ptr(g_out), _abi.ptr(order), _abi.ptr(g_cand), _abi.ptr(g_extra), B, M, Q, D)
    return g_cand, g_extra


# ------------------------------------------------------------------ deformable local cross-attention (include/upp_hip.h)
DEFORM_MAX_H = 16
DEFORM_MAX_K = 32


def _deform_range(B, N, NK, k, H, G, arrays):
    """da_sizes of csrc/deform_row.h: positive sizes, the family's limits, and every array (its element count) below 2^31"""
    return min(B, N, NK, k, H, G) >= 1 and H <= DEFORM_MAX_H and k <= DEFORM_MAX_K and H % G == 0 and B <= 65535 and max(arrays) < 2 ** 31


def deform_attn_usable(B, N, NK, k, H, G):
    """The served range of upp_deform_offset_fwd / upp_deform_attn_* (head_dim 64 is the caller's C == 64 H)."""
    C = 64 * H
    return _deform_range(B, N, NK, k, H, G, (B * N * k * H, B * G * NK * C, B * G * N * C, B * G * N * k * 3))


def _served(who, usable, limits, **sizes):
    """Raise unless the sizes -- named, in `usable`'s argument order -- are positive and `usable` (an *_usable of this file) serves
    them; `limits` is the range, in words."""
    got = ", ".join("%s = %d" % s for s in sizes.items())
    if min(sizes.values()) < 1:
        raise RuntimeError("%s: every size must be positive, got %s" % (who, got))
    if not usable(*sizes.values()):
        raise RuntimeError("%s: %s is outside the served range %s, B <= 65535, every array below 2^31 elements (UPP_E_RANGE)" % (who, got, limits))


_DEFORM_LIMITS = "head_dim 64, 1 <= H <= %d, G | H, 1 <= k <= %d" % (DEFORM_MAX_H, DEFORM_MAX_K)


def _aligned16(who, **tensors):
    for name, t in tensors.items():
        if t is not None and t.data_ptr() % 16:
            raise RuntimeError("%s: %s must be 16-byte aligned" % (who, name))


def _positive(who, name, v):
    v = float(v)
    if not (v > 0.0 and v != float("inf")):
        raise RuntimeError("%s: %s must be finite and positive, got %r" % (who, name, v))
    return v


def deform_offset_fwd(A, Bq, idx, pos, gamma, beta, W3, eps, ball=False):
    """A (B,G,NK,C), Bq (B,G,N,C), idx (B,N,k) int64, pos (B,NK,3), gamma / beta (C), W3 (3,C) -> shift (B,G,N k,3) =
    pos[idx] + tanh(W3 gelu(LayerNorm(A[idx] + Bq))): upp_deform_offset_fwd, 1 launch, no (B,G,N,k,C) tensor.  ball: the tanh is scaled by
    0.5 (max_s pos[idx] - min_s pos[idx]) over the k slots of the query (upp_deform_offset_ball_fwd)."""
    _need(A, "A", torch.float32, 4)
    B, G, NK, C = A.shape
    _need(Bq, "Bq", torch.float32, 4)
    N = Bq.shape[2]
    _need_f32(Bq, "Bq", (B, G, N, C))
    _need(idx, "idx", torch.int64, 3)
    k = idx.shape[2]
    if tuple(idx.shape) != (B, N, k):
        raise RuntimeError("deform_offset: idx must be (B, N, k) = (%d, %d, k), got %s" % (B, N, tuple(idx.shape)))
    _need_f32(pos, "pos", (B, NK, 3))
    _need_f32(gamma, "gamma", (C,))
    _need_f32(beta, "beta", (C,))
    _need_f32(W3, "W3", (3, C))
    _same_device(A, Bq, idx, pos, gamma, beta, W3)
    eps = _positive("deform_offset", "eps", eps)
    if C % 64:
        raise RuntimeError("deform_offset: C = %d is outside the served range (a multiple of 64: UPP_E_RANGE)" % C)
    _served("deform_offset", deform_attn_usable, _DEFORM_LIMITS, B=B, N=N, NK=NK, k=k, H=C // 64, G=G)
    _aligned16("deform_offset", A=A, Bq=Bq, idx=idx, pos=pos, gamma=gamma, beta=beta, W3=W3)
    shift = torch.empty((B, G, N * k, 3), dtype=torch.float32, device=A.device)
    _call(A.device, "upp_deform_offset_ball_fwd" if ball else "upp_deform_offset_fwd", _abi.ptr(A), _abi.ptr(Bq), _abi.ptr(idx), _abi.ptr(pos),
          _abi.ptr(gamma), _abi.ptr(beta), _abi.ptr(W3), _abi.ptr(shift), eps, B, G, N, NK, k, C)
    return shift


def _deform_attn_args(who, q, PK, PV, bk, bv, idx3, w3, H, scale, idx=None):
    """The operands of upp_deform_attn_* (idx None: k is idx3's) and upp_region_attn_* (idx (B,N,k) int64 gives k, and idx3 must be
    exactly (B, G, N k, 3)) -> B, N, NK, k, H, G, C, scale"""
    _need(q, "q", torch.float32, 3)
    B, N, C = q.shape
    if idx is not None:
        _need(idx, "idx", torch.int64, 3)
        if tuple(idx.shape) != (B, N, idx.shape[2]):
            raise RuntimeError("%s: idx must be (B, N, k) = (%d, %d, k), got %s" % (who, B, N, tuple(idx.shape)))
    _need(PK, "PK", torch.float32, 4)
    G, NK = PK.shape[1], PK.shape[2]
    _need_f32(PK, "PK", (B, G, NK, C))
    _need_f32(PV, "PV", (B, G, NK, C))
    _need_f32(bk, "bk", (C,), optional=True)
    _need_f32(bv, "bv", (C,), optional=True)
    _need(idx3, "idx3", torch.int32, 4, 3)
    _need(w3, "w3", torch.float32, 4, 3)
    rows = "%d k" % N if idx is None else N * idx.shape[2]
    if idx3.shape != w3.shape or tuple(idx3.shape[:2]) != (B, G) or (idx3.shape[2] % N if idx is None else idx3.shape[2] != rows):
        raise RuntimeError("%s: idx3 and w3 must both be (B, G, N k, 3) = (%d, %d, %s, 3), got %s and %s"
                           % (who, B, G, rows, tuple(idx3.shape), tuple(w3.shape)))
    k = idx3.shape[2] // N if idx is None else idx.shape[2]
    _same_device(q, PK, PV, idx3, w3, *[t for t in (idx, bk, bv) if t is not None])
    H = int(H)
    scale = _positive(who, "scale", scale)
    if H < 1 or C != 64 * H:
        raise RuntimeError("%s: C = %d with %d heads is outside the served range (head_dim 64: UPP_E_RANGE)" % (who, C, H))
    _served(who, deform_attn_usable if idx is None else region_attn_usable, _DEFORM_LIMITS, B=B, N=N, NK=NK, k=k, H=H, G=G)
    _aligned16(who, q=q, idx=idx, PK=PK, PV=PV, bk=bk, bv=bv, idx3=idx3, w3=w3)
    return B, N, NK, k, H, G, C, scale


def _need_arg(who, arg, shape, like):
    """the uint8 arg of the max (B, N, channels) that a backward reads, on `like`'s device"""
    _need(arg, "arg", torch.uint8, 3)
    if tuple(arg.shape) != tuple(shape):
        raise RuntimeError("%s: arg must be %s, got %s" % (who, tuple(shape), tuple(arg.shape)))
    _same_device(like, arg)
    _aligned16(who, arg=arg)


def deform_attn_fwd(q, PK, PV, bk, bv, idx3, w3, H, scale):
    """q (B,N,C), PK / PV (B,G,NK,C), bk / bv (C) | None, idx3 int32 and w3 (B,G,N k,3) -> ctx (B,N,C), p (B,N,H,k): upp_deform_attn_fwd."""
    B, N, NK, k, H, G, C, scale = _deform_attn_args("deform_attention", q, PK, PV, bk, bv, idx3, w3, H, scale)
    ctx = torch.empty((B, N, C), dtype=torch.float32, device=q.device)
    p = torch.empty((B, N, H, k), dtype=torch.float32, device=q.device)
    _call(q.device, "upp_deform_attn_fwd", _abi.ptr(q), _abi.ptr(PK), _abi.ptr(PV), _abi.ptr(bk), _abi.ptr(bv), _abi.ptr(idx3), _abi.ptr(w3),
          _abi.ptr(ctx), _abi.ptr(p), scale, B, N, NK, k, H, G)
    return ctx, p


def deform_attn_bwd(q, PK, PV, bk, bv, idx3, w3, p, d_ctx, H, scale, deterministic=False, want_krow=False):
    """-> d_q (B,N,C), d_PK, d_PV (B,G,NK,C), ds (B,N,H,k), d_krow (B,N,C) | None (the rows whose column sums are d_bk).  d_PK / d_PV by
    f32 atomics into arrays the entry point zeroes with a kernel (upp_deform_attn_bwd) or, deterministic, in ascending (n k + s) 3 + j
    (upp_deform_attn_bwd_det, include/upp_hip.h)."""
    B, N, NK, k, H, G, C, scale = _deform_attn_args("deform_attention_bwd", q, PK, PV, bk, bv, idx3, w3, H, scale)
    _need_f32(p, "p", (B, N, H, k))
    _need_f32(d_ctx, "d_ctx", (B, N, C))
    _same_device(q, p, d_ctx)
    _aligned16("deform_attention_bwd", p=p, d_ctx=d_ctx)
    dev = q.device
    d_q = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    d_PK = torch.empty((B, G, NK, C), dtype=torch.float32, device=dev)
    d_PV = torch.empty((B, G, NK, C), dtype=torch.float32, device=dev)
    ds = torch.empty((B, N, H, k), dtype=torch.float32, device=dev)
    d_krow = torch.empty((B, N, C), dtype=torch.float32, device=dev) if want_krow else None
    _call(dev, "upp_deform_attn_bwd_det" if deterministic else "upp_deform_attn_bwd", _abi.ptr(q), _abi.ptr(PK), _abi.ptr(PV), _abi.ptr(bk),
          _abi.ptr(bv), _abi.ptr(idx3), _abi.ptr(w3), _abi.ptr(p), _abi.ptr(d_ctx), _abi.ptr(d_q), _abi.ptr(d_PK), _abi.ptr(d_PV),
          _abi.ptr(d_krow), _abi.ptr(ds), scale, B, N, NK, k, H, G)
    return d_q, d_PK, d_PV, ds, d_krow


# ------------------------------------------------------------------ deformable graph attention (include/upp_hip.h)
INTERP_MAX_K, INTERP_MAX_O = 32, 1024


def interp_max_usable(B, N, NK, k, O):
    """The served range of upp_interp_max_fwd / _bwd / _bwd_det (sizes only)."""
    if min(B, N, NK, k, O) < 1 or k > INTERP_MAX_K or O > INTERP_MAX_O or B > 65535:
        return False
    return max(B * NK * O, B * N * O, B * N * k * 3) < 2 ** 31


def _interp_max_args(who, a, a_name, b, b_name, idx3, w3, slope, NK=None):
    """a (B,NK,O) for the forward (NK None) or (B,N,O) for the backward, b (B,N,O), idx3 / w3 (B, N k, 3) -> B, N, NK, k, O, slope"""
    _need(a, a_name, torch.float32, 3)
    _need(b, b_name, torch.float32, 3)
    B, N, O = b.shape
    NK = a.shape[1] if NK is None else int(NK)
    _need_f32(a, a_name, (B, a.shape[1], O))
    _need(idx3, "idx3", torch.int32, 3, 3)
    _need(w3, "w3", torch.float32, 3, 3)
    if idx3.shape != w3.shape or idx3.shape[0] != B or N < 1 or idx3.shape[1] % N:
        raise RuntimeError("%s: idx3 and w3 must both be (B, N k, 3) = (%d, %d k, 3), got %s and %s"
                           % (who, B, N, tuple(idx3.shape), tuple(w3.shape)))
    k = idx3.shape[1] // N
    _same_device(a, b, idx3, w3)
    slope = float(slope)
    if not 0.0 <= slope <= 1.0:
        raise RuntimeError("%s: slope must be in [0, 1], got %r (UPP_E_BADARG)" % (who, slope))
    _served(who, interp_max_usable, "1 <= k <= %d, 1 <= O <= %d" % (INTERP_MAX_K, INTERP_MAX_O), B=B, N=N, NK=NK, k=k, O=O)
    _aligned16(who, **{a_name: a, b_name: b, "idx3": idx3, "w3": w3})
    return B, N, NK, k, O, slope


def interp_max_fwd(PW, Bq, idx3, w3, slope=0.2):
    """PW (B,NK,O), Bq (B,N,O), idx3 int32 and w3 (B, N k, 3) -> out (B,N,O) = lrelu(max_s (Bq + sum_j w3 PW[idx3])), arg (B,N,O) uint8:
    upp_interp_max_fwd, 1 launch, no (B,N,k,O) tensor."""
    B, N, NK, k, O, slope = _interp_max_args("interp_edge_max", PW, "PW", Bq, "Bq", idx3, w3, slope)
    out = torch.empty((B, N, O), dtype=torch.float32, device=PW.device)
    arg = torch.empty((B, N, O), dtype=torch.uint8, device=PW.device)
    _call(PW.device, "upp_interp_max_fwd", _abi.ptr(PW), _abi.ptr(Bq), _abi.ptr(idx3), _abi.ptr(w3), _abi.ptr(out), _abi.ptr(arg), slope,
          B, N, NK, k, O)
    return out, arg


def interp_max_bwd(g_out, out, arg, idx3, w3, NK, slope=0.2, deterministic=False):
    """g_out, out (B,N,O), arg (B,N,O) uint8 -> d_Bq (B,N,O), d_PW (B,NK,O).  d_PW by f32 atomics into an array the entry point zeroes with
    a kernel (upp_interp_max_bwd) or, deterministic, in ascending 3 n + j (upp_interp_max_bwd_det, include/upp_hip.h)."""
    B, N, NK, k, O, slope = _interp_max_args("interp_edge_max_bwd", g_out, "g_out", out, "out", idx3, w3, slope, NK=NK)
    _need_f32(g_out, "g_out", (B, N, O))
    _need_arg("interp_edge_max_bwd", arg, (B, N, O), g_out)
    d_Bq = torch.empty((B, N, O), dtype=torch.float32, device=g_out.device)
    d_PW = torch.empty((B, NK, O), dtype=torch.float32, device=g_out.device)
    _call(g_out.device, "upp_interp_max_bwd_det" if deterministic else "upp_interp_max_bwd", _abi.ptr(g_out), _abi.ptr(out), _abi.ptr(arg),
          _abi.ptr(idx3), _abi.ptr(w3), _abi.ptr(d_Bq), _abi.ptr(d_PW), slope, B, N, NK, k, O)
    return d_Bq, d_PW


# ------------------------------------------------------------------ region-wise deformable attention (include/upp_hip.h)
def region_attn_usable(B, N, NK, k, H, G):
    """The served range of upp_region_attn_fwd / _bwd / _bwd_det (sizes only; head_dim 64 is the caller's C == 64 H)."""
    C = 64 * H
    return _deform_range(B, N, NK, k, H, G, (B * G * NK * C, 3 * B * N * k * C, B * G * N * k * 3))


def region_attn_fwd(q, idx, PK, PV, bk, bv, idx3, w3, H, scale):
    """q (B,N,C), idx (B,N,k) int64 rows of q, PK / PV (B,G,NK,C), bk / bv (C) | None, idx3 int32 and w3 (B,G,N k,3) -> out (B,N,C),
    arg (B,N,C) uint8: upp_region_attn_fwd, 1 launch, no (B,N,k,C) tensor and no (B,N,H,k,k) probabilities."""
    B, N, NK, k, H, G, C, scale = _deform_attn_args("region_attention", q, PK, PV, bk, bv, idx3, w3, H, scale, idx)
    out = torch.empty((B, N, C), dtype=torch.float32, device=q.device)
    arg = torch.empty((B, N, C), dtype=torch.uint8, device=q.device)
    _call(q.device, "upp_region_attn_fwd", _abi.ptr(q), _abi.ptr(idx), _abi.ptr(PK), _abi.ptr(PV), _abi.ptr(bk), _abi.ptr(bv), _abi.ptr(idx3),
          _abi.ptr(w3), _abi.ptr(out), _abi.ptr(arg), scale, B, N, NK, k, H, G)
    return out, arg


def region_attn_bwd(q, idx, PK, PV, bk, bv, idx3, w3, arg, d_out, H, scale, deterministic=False, want_krow=False, want_vrow=False,
                    rows=None):
    """-> d_q (B,N,C), d_PK, d_PV (B,G,NK,C), d_krow, d_vrow (B,N,C) | None (the rows whose column sums are d_bk / d_bv), rows | None.
    The three scatter-adds by f32 atomics into arrays the entry point zeroes with a kernel (upp_region_attn_bwd) or, deterministic,
    through the workspace rows (3,B,N,k,C) -- allocated here when None -- in ascending n k + t and (n k + s) 3 + j
    (upp_region_attn_bwd_det, include/upp_hip.h)."""
    B, N, NK, k, H, G, C, scale = _deform_attn_args("region_attention_bwd", q, PK, PV, bk, bv, idx3, w3, H, scale, idx)
    _need_f32(d_out, "d_out", (B, N, C))
    _need_arg("region_attention_bwd", arg, (B, N, C), q)
    _same_device(q, d_out)
    _aligned16("region_attention_bwd", d_out=d_out)
    dev = q.device
    d_q = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    d_PK = torch.empty((B, G, NK, C), dtype=torch.float32, device=dev)
    d_PV = torch.empty((B, G, NK, C), dtype=torch.float32, device=dev)
    d_krow = torch.empty((B, N, C), dtype=torch.float32, device=dev) if want_krow else None
    d_vrow = torch.empty((B, N, C), dtype=torch.float32, device=dev) if want_vrow else None
    if deterministic:
        if rows is None:
            rows = torch.empty((3, B, N, k, C), dtype=torch.float32, device=dev)
        _need_f32(rows, "rows", (3, B, N, k, C))
        _same_device(q, rows)
        _aligned16("region_attention_bwd", rows=rows)
        _call(dev, "upp_region_attn_bwd_det", _abi.ptr(q), _abi.ptr(idx), _abi.ptr(PK), _abi.ptr(PV), _abi.ptr(bk), _abi.ptr(bv),
              _abi.ptr(idx3), _abi.ptr(w3), _abi.ptr(arg), _abi.ptr(d_out), _abi.ptr(d_q), _abi.ptr(d_PK), _abi.ptr(d_PV),
              _abi.ptr(d_krow), _abi.ptr(d_vrow), _abi.ptr(rows), scale, B, N, NK, k, H, G)
    else:
        rows = None
        _call(dev, "upp_region_attn_bwd", _abi.ptr(q), _abi.ptr(idx), _abi.ptr(PK), _abi.ptr(PV), _abi.ptr(bk), _abi.ptr(bv), _abi.ptr(idx3),
              _abi.ptr(w3), _abi.ptr(arg), _abi.ptr(d_out), _abi.ptr(d_q), _abi.ptr(d_PK), _abi.ptr(d_PV), _abi.ptr(d_krow),
              _abi.ptr(d_vrow), scale, B, N, NK, k, H, G)
    return d_q, d_PK, d_PV, d_krow, d_vrow, rows


# ------------------------------------------------------------------ Chamfer
def chamfer_fwd(xyz1, xyz2):
    _need(xyz1, "xyz1", torch.float32, 3, 3)
    _need(xyz2, "xyz2", torch.float32, 3, 3)
    _same_device(xyz1, xyz2)
    B, n, _ = xyz1.shape
    if xyz2.shape[0] != B:
        raise RuntimeError("xyz1 and xyz2 batch sizes differ")
    m = xyz2.shape[1]
    dev = xyz1.device
    dist1 = torch.empty((B, n), dtype=torch.float32, device=dev)
    dist2 = torch.empty((B, m), dtype=torch.float32, device=dev)
    idx1 = torch.empty((B, n), dtype=torch.int32, device=dev)
    idx2 = torch.empty((B, m), dtype=torch.int32, device=dev)
    if B == 0:
        return dist1, dist2, idx1, idx2
    _call(xyz1.device, "upp_chamfer_fwd", _abi.ptr(xyz1), _abi.ptr(xyz2), _abi.ptr(dist1), _abi.ptr(dist2),
          _abi.ptr(idx1), _abi.ptr(idx2), B, n, m)
    return dist1, dist2, idx1, idx2


def _need_i32(t, name, shape):
    """_need for an int32 index operand of exactly `shape`.  Metadata only; the VALUES cannot be checked without a synchronisation."""
    _need(t, name, torch.int32)
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")


def _cloud_pair(xyz1, xyz2):
    """-> (B, n, m) of two f32 clouds (B,n,3), (B,m,3) on one device."""
    _need(xyz1, "xyz1", torch.float32, 3, 3)
    _need(xyz2, "xyz2", torch.float32, 3, 3)
    _same_device(xyz1, xyz2)
    if xyz2.shape[0] != xyz1.shape[0]:
        raise RuntimeError("xyz1 and xyz2 batch sizes differ")
    return xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]


def chamfer_bwd(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2, deterministic=False):
    """deterministic: every gradient row = own term, then the other cloud's terms in ascending index (upp_chamfer_bwd_det,
    include/upp_hip.h) instead of f32 atomics.  Every tensor is checked from its metadata (device, dtype, contiguity, exact shape); the
    index VALUES are the caller's: they must lie inside the other cloud (include/upp_hip.h)."""
    B, n, m = _cloud_pair(xyz1, xyz2)
    _need_i32(idx1, "idx1", (B, n))
    _need_i32(idx2, "idx2", (B, m))
    _need_f32(grad_dist1, "grad_dist1", (B, n))
    _need_f32(grad_dist2, "grad_dist2", (B, m))
    _same_device(xyz1, idx1, idx2, grad_dist1, grad_dist2)
    g1 = torch.empty_like(xyz1)          # (overwritten by the kernel: include/upp_hip.h)
    g2 = torch.empty_like(xyz2)
    if B == 0:
        return g1, g2
    _call(xyz1.device, "upp_chamfer_bwd_det" if deterministic else "upp_chamfer_bwd", _abi.ptr(xyz1), _abi.ptr(xyz2), _abi.ptr(idx1), _abi.ptr(idx2),
          _abi.ptr(grad_dist1), _abi.ptr(grad_dist2), _abi.ptr(g1), _abi.ptr(g2), B, n, m)
    return g1, g2


def chamfer_loss(dist1, dist2, l1):
    """-> (loss (1,), fac1 (B,n), fac2 (B,m)): the reduction of ChamferDistanceL1 (l1) / L2 and d loss / d dist (upp_chamfer_loss)."""
    _need(dist1, "dist1", torch.float32, 2)
    _need(dist2, "dist2", torch.float32, 2)
    _same_device(dist1, dist2)
    B, n = dist1.shape
    m = dist2.shape[1]
    if dist2.shape[0] != B:
        raise RuntimeError("dist1 and dist2 batch sizes differ")
    if B < 1 or n < 1 or m < 1:
        raise RuntimeError("chamfer_loss: a mean over nothing")
    dev = dist1.device
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    fac1, fac2 = torch.empty_like(dist1), torch.empty_like(dist2)
    work = torch.empty((int(_abi.load().upp_chamfer_loss_work_floats()),), dtype=torch.float32, device=dev)
    _call(dev, "upp_chamfer_loss", _abi.ptr(dist1), _abi.ptr(dist2), B, n, m, 1 if l1 else 0, _abi.ptr(loss), _abi.ptr(fac1), _abi.ptr(fac2), _abi.ptr(work))
    return loss, fac1, fac2


# ------------------------------------------------------------------ EMD
def emd_approxmatch(xyz1, xyz2):
    _need(xyz1, "xyz1", torch.float32, 3, 3)
    _need(xyz2, "xyz2", torch.float32, 3, 3)
    _same_device(xyz1, xyz2)
    B, n, _ = xyz1.shape
    if xyz2.shape[0] != B:
        raise RuntimeError("xyz1 and xyz2 batch sizes differ")
    m = xyz2.shape[1]
    match = torch.empty((B, m, n), dtype=torch.float32, device=xyz1.device)
    if B == 0:
        return match
    nwork = int(_abi.load().upp_emd_work_floats(B, n, m))
    work = torch.empty((max(nwork, 1),), dtype=torch.float32, device=xyz1.device)
    _call(xyz1.device, "upp_emd_approxmatch", _abi.ptr(xyz1), _abi.ptr(xyz2), _abi.ptr(match), _abi.ptr(work), B, n, m)
    return match


def emd_matchcost(xyz1, xyz2, match, deterministic=False):
    """deterministic: the 64-point tiles' partial costs summed in ascending tile order (upp_emd_matchcost_det) instead of atomics."""
    B, n, m = _cloud_pair(xyz1, xyz2)
    _need_f32(match, "match", (B, m, n))
    _same_device(xyz1, match)
    cost = torch.empty((B,), dtype=torch.float32, device=xyz1.device)
    if B == 0:
        return cost
    if deterministic:
        nwork = int(_abi.load().upp_emd_matchcost_det_work_bytes(B, n, m))
        work = torch.empty(((max(nwork, 4) + 3) // 4,), dtype=torch.float32, device=xyz1.device)
        _call(xyz1.device, "upp_emd_matchcost_det", _abi.ptr(xyz1), _abi.ptr(xyz2), _abi.ptr(match), _abi.ptr(cost), _abi.ptr(work), B, n, m)
        return cost
    _call(xyz1.device, "upp_emd_matchcost", _abi.ptr(xyz1), _abi.ptr(xyz2), _abi.ptr(match), _abi.ptr(cost), B, n, m)
    return cost


def emd_matchcost_bwd(grad_cost, xyz1, xyz2, match):
    B, n, m = _cloud_pair(xyz1, xyz2)
    _need_f32(grad_cost, "grad_cost", (B,))
    _need_f32(match, "match", (B, m, n))
    _same_device(xyz1, grad_cost, match)
    g1 = torch.empty_like(xyz1)
    g2 = torch.empty_like(xyz2)
    if B == 0:
        return g1, g2
    _call(xyz1.device, "upp_emd_matchcost_bwd", _abi.ptr(grad_cost), _abi.ptr(xyz1), _abi.ptr(xyz2), _abi.ptr(match),
          _abi.ptr(g1), _abi.ptr(g2), B, n, m)
    return g1, g2


# ------------------------------------------------------------------ patch embedding (forward only)
def patch_embed_fwd(point_groups, enc, training):
    """point_groups (B,G,n,3) -> (B,G,C) through upp_patch_embed_fwd.  `enc` is an Encoder-shaped
    module (first_conv / second_conv Sequentials with the reference's layer sizes)."""
    _need(point_groups, "point_groups", torch.float32, 4, 3)
    B, G, n, _ = point_groups.shape
    c1, bn1, _, c2 = enc.first_conv
    c3, bn3, _, c4 = enc.second_conv
    C = c4.weight.shape[0]
    R = B * G * n
    dev = point_groups.device
    work = torch.empty((int(_abi.load().upp_patch_embed_work_floats(R, n)),), dtype=torch.float32, device=dev)
    out = torch.empty((B, G, C), dtype=torch.float32, device=dev)
    mom = 0.1 if bn1.momentum is None else float(bn1.momentum)
    _call(dev, "upp_patch_embed_fwd", _abi.ptr(point_groups), R, n,
          _abi.ptr(c1.weight), _abi.ptr(c1.bias), _abi.ptr(bn1.weight), _abi.ptr(bn1.bias),
          _abi.ptr(bn1.running_mean), _abi.ptr(bn1.running_var),
          _abi.ptr(c2.weight), _abi.ptr(c2.bias),
          _abi.ptr(c3.weight), _abi.ptr(c3.bias), _abi.ptr(bn3.weight), _abi.ptr(bn3.bias),
          _abi.ptr(bn3.running_mean), _abi.ptr(bn3.running_var),
          _abi.ptr(c4.weight), _abi.ptr(c4.bias), C, mom, float(bn1.eps), 1 if training else 0,
          _abi.ptr(work), _abi.ptr(out))
    return out


# ------------------------------------------------------------------ Transformer block glue
LIN_NONE, LIN_BIAS, LIN_BIAS_GELU, LIN_BIAS_GELU_D, LIN_MUL, LIN_BIAS_RELU = 0, 1, 2, 3, 4, 5


class time_linear_calls:
    """Measurement scope (bench.py): every upp_linear_f32 / upp_linear_sb_f32 launch inside it is bracketed by a pair of HIP events recorded
    on the launch stream; `.report()` -> [(M, N, K, epilogue, ms, sb)] after a synchronize (sb: the split-bf16 kernel's tile code, 0 = the
    exact-f32 kernel).  Eager launches only (not under capture)."""
    active = None

    def __enter__(self):
        self.calls = []
        self.wgrad_groups = []          # [(M, N, K), ...] per upp_linear_wgrad_grouped_f32 launch
        self.group_bias = []            # (M, N, K) per group-bias launch (also listed in `calls`)
        time_linear_calls.active = self
        return self

    def __exit__(self, *exc):
        time_linear_calls.active = None
        return False

    def report(self):
        torch.cuda.synchronize()
        return [(M, N, K, e, a.elapsed_time(b), sb) for (M, N, K, e, a, b, sb) in self.calls]

    @classmethod
    def bracket(cls, ev0=None, *what):
        """bracket() before a launch -> its start event (None outside a scope); bracket(ev0, M, N, K, epilogue, sb) after it."""
        if cls.active is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        if what:
            cls.active.calls.append(what[:4] + (ev0, ev) + what[4:])
        return ev


def _is_matrix(t):                     # a 2-D f32 HIP matrix with contiguous rows: what the Linear kernels read through a row stride
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1


def _need_matrix(t, name):
    if not _is_matrix(t):
        raise RuntimeError(f"{name} must be a 2-D f32 HIP (cuda) matrix with contiguous rows; upp_hip has no CPU path")


def aligned_rows(t):                   # rows the matrix-core kernels load 16 bytes at a time: whole float4s from a 16-byte aligned base
    return t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


SPLIT_BF16 = os.environ.get("UPP_SPLIT_BF16", "1") != "0"      # frozen weights on the bf16 matrix pipe at f32 accuracy (csrc/linear_sb.hip)


class _WeightPlanes(_derived.DerivedWeights):
    """bf16 plane images (upp_linear_sb_prep) of weights and of their cached transposes: the _derived.DerivedWeights (protocol and CONTRACT
    there) of the split-bf16 kernels, kept only for PERSISTENT owners -- an nn.Parameter, or a buffer marked `_upp_persistent` by its keeper
    (functional.TRANSPOSED's W^T copies, the patch embedding's zero-padded first-layer weight).  A step driver's trainable weights have the
    images of W (forward) and of W^T (data gradient, split straight from W: the entry's tag) re-split by one launch per step; outside a
    driver a trainable weight stays on the exact-f32 kernel."""

    def __init__(self):
        super().__init__("bf16 plane image", lambda w, transposed: self._split(w, None, bool(transposed)),
                         lambda w, planes, transposed: self._split(w, planes, bool(transposed)), _derived.persistent_owner, self._split_batched)

    @staticmethod
    def _split(w, planes=None, transposed=False):
        """planes of the (N,K) operand `w`, or -- transposed -- of w^T for a row-major w (K,N) (upp_linear_sb_prep reads it transposed)."""
        N, K = (w.shape[1], w.shape[0]) if transposed else w.shape
        if planes is None:
            planes = torch.empty(int(_abi.load().upp_linear_sb_planes_bytes(N, K)), dtype=torch.uint8, device=w.device)
        _call(w.device, "upp_linear_sb_prep", _abi.ptr(w), w.stride(0), N, K, 1 if transposed else 0, _abi.ptr(planes))
        return planes

    @staticmethod
    def _split_batched(jobs):
        """jobs: [(w, planes, transposed)] -- every image re-split by ONE launch (upp_linear_sb_prep_batched)."""
        import ctypes
        k = len(jobs)
        W = (ctypes.c_void_p * k)(*[w.data_ptr() for w, _, _ in jobs])
        ld = (ctypes.c_longlong * k)(*[w.stride(0) for w, _, _ in jobs])
        N = (ctypes.c_int * k)(*[(w.shape[1] if tr else w.shape[0]) for w, _, tr in jobs])
        K = (ctypes.c_int * k)(*[(w.shape[0] if tr else w.shape[1]) for w, _, tr in jobs])
        T = (ctypes.c_int * k)(*[1 if tr else 0 for _, _, tr in jobs])
        P = (ctypes.c_void_p * k)(*[p.data_ptr() for _, p, _ in jobs])
        _call(jobs[0][0].device, "upp_linear_sb_prep_batched", W, ld, N, K, T, P, k)


PLANES = _WeightPlanes()


def linear_sb_tile(M, N, K):
    """Tile code of the split-bf16 kernel for (M,N,K), 0 = not a problem for it (upp_linear_sb_tile)."""
    return max(0, int(_abi.load().upp_linear_sb_tile(int(M), int(N), int(K))))


def _sb_servable(N, K, out, bias, aux):
    return (N % 4 == 0 and K % 32 == 0 and out.data_ptr() % 16 == 0 and (bias is None or bias.data_ptr() % 16 == 0)
            and (aux is None or aux.data_ptr() % 16 == 0))


def linear_sb_usable(M, N, K):
    """Does the split-bf16 kernel take an (M,K) x (N,K)^T product (freshly allocated, 16-byte aligned operands assumed)?"""
    return bool(SPLIT_BF16 and N % 4 == 0 and K % 32 == 0 and linear_sb_tile(M, N, K))


def linear_f32(a, w, bias=None, epilogue=LIN_NONE, aux=None, tile=0, out=None, frozen=False, planes=None, wshape=None):
    """C (M,N) = epilogue(a (M,K) . w (N,K)^T) on the matrix cores: upp_linear_f32 (exact f32 MFMA, bit-pinned order), or -- frozen=True: w
    is a frozen weight or a cached copy of one, its contents change only through torch (version counter) -- upp_linear_sb_f32 (three-way
    bf16 split of both operands, six bf16 MFMA products, f32 accumulate: f32 accuracy at 6/16 of the matrix-pipe time) where that kernel
    takes the shape.  planes / wshape: the plane image of the (N,K) operand made by the caller (ops.PLANES.get_trainable: a trainable
    weight inside a step driver, or its transpose) -- then w may be None and the split-bf16 kernel is taken (linear_sb_usable must hold).
    a: (..., K) f32 whose rows are K-contiguous with one common row stride; w: (N,K).
    epilogue LIN_BIAS_GELU_D returns (C, GELU'); LIN_MUL multiplies by aux (M,N)."""
    if planes is not None:
        N, Kw = wshape
    else:
        _need_matrix(w, "w")
        _same_device(a, w)
        N, Kw = w.shape
    if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32):
        raise RuntimeError("a must be a f32 HIP (cuda) tensor; upp_hip has no CPU path")
    K = a.shape[-1]
    if Kw != K:
        raise RuntimeError(f"linear_f32: a (...,{K}) against w ({N},{Kw})")
    a2 = a.reshape(-1, K)
    if not aligned_rows(a2):                                                        # (a column window with a misaligned base: one copy)
        a2 = a2.contiguous()
    M = a2.shape[0]
    lead = tuple(a.shape[:-1])
    if out is None:
        out = torch.empty(lead + (N,), dtype=torch.float32, device=a.device)
    d = None
    if epilogue == LIN_BIAS_GELU_D:
        d = torch.empty(lead + (N,), dtype=torch.float32, device=a.device)
        aux = d
    if epilogue == LIN_MUL:
        _need(aux, "aux", torch.float32)
        if aux.numel() != M * N:
            raise RuntimeError("linear_f32: aux must be (M,N)")
    if bias is not None:
        _need(bias, "bias", torch.float32, 1, N)
    sb = 0
    if planes is None and frozen and SPLIT_BF16 and tile == 0 and _sb_servable(N, K, out, bias, aux):
        sb = linear_sb_tile(M, N, K)
        if sb:
            planes = PLANES.get(w)
    elif planes is not None:
        sb = linear_sb_tile(M, N, K)
        if not (sb and _sb_servable(N, K, out, bias, aux)):
            raise RuntimeError("linear_f32: plane images given for a problem the split-bf16 kernel does not take (ask linear_sb_usable first)")
    ev0 = time_linear_calls.bracket()
    if sb:
        _call(a.device, "upp_linear_sb_f32", _abi.ptr(a2), a2.stride(0), _abi.ptr(planes), _abi.ptr(bias), _abi.ptr(out), N,
              _abi.ptr(aux), N, M, N, K, int(epilogue), sb)
    else:
        _call(a.device, "upp_linear_f32", _abi.ptr(a2), a2.stride(0), _abi.ptr(w), w.stride(0), _abi.ptr(bias), _abi.ptr(out), N,
              _abi.ptr(aux), N, M, N, K, int(epilogue), int(tile))
    time_linear_calls.bracket(ev0, M, N, K, int(epilogue), sb)
    return (out, d) if epilogue == LIN_BIAS_GELU_D else out


def colsum_partials(part, offset, length, chunks=None):
    """(chunks, length) partial column sums of columns [offset, offset + length) of the tall 2-D matrix `part` (upp_colsum_partials)."""
    if not _is_matrix(part):
        raise RuntimeError("colsum_partials: a 2-D f32 HIP (cuda) matrix with contiguous rows is required; upp_hip has no CPU path")
    if offset < 0 or length < 1 or offset + length > part.shape[1]:
        raise RuntimeError(f"colsum_partials: columns [{offset}, {offset + length}) outside {tuple(part.shape)}")
    n = part.shape[0]
    if chunks is None:
        chunks = max(1, min(256, (n + 255) // 256))
    dst = torch.empty((chunks, length), dtype=torch.float32, device=part.device)
    view = part[:, offset:offset + length]
    _call(part.device, "upp_colsum_partials", _abi.ptr(view), part.stride(0), n, length, chunks, _abi.ptr(dst))
    return dst


def sum_rows(part, offset=0, length=None):
    """Column sums of columns [offset, offset + length) of a 2-D f32 HIP matrix on this library's kernels (two stages of
    upp_colsum_partials for tall matrices) -> (length,).  NOT torch.sum: a torch reduction that splits its rows over workgroups zeroes its
    semaphores with a memset, and a memset NODE of a captured step graph works in the first replay only on this stack (NOTEBOOK 12.11)."""
    if length is None:
        length = part.shape[1] - offset
    while part.shape[0] > 256:
        part, offset = colsum_partials(part, offset, length), 0
    return colsum_partials(part, offset, length, chunks=1)[0]


def logsoftmax_rows_fwd(y, bias, C):
    """log_softmax over the first C columns of the rows of y (R, >= C) (+ bias (C)) -> logp (R, C); upp_logsoftmax_rows_fwd."""
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1 and y.shape[1] >= C):
        raise RuntimeError("logsoftmax_rows_fwd: a 2-D f32 HIP (cuda) matrix with contiguous rows of at least C columns is required; upp_hip has no CPU path")
    if bias is not None:
        _need(bias, "bias", torch.float32, 1, int(C))
    R = y.shape[0]
    logp = torch.empty((R, int(C)), dtype=torch.float32, device=y.device)
    _call(y.device, "upp_logsoftmax_rows_fwd", _abi.ptr(y), y.stride(0), _abi.ptr(bias), R, int(C), _abi.ptr(logp))
    return logp


def logsoftmax_rows_bwd(g_logp, logp, Cpad):
    """-> g_y (R, Cpad): the log-softmax backward in the first C columns, zeros in the pad columns; upp_logsoftmax_rows_bwd."""
    _need(g_logp, "g_logp", torch.float32, ndim=2)
    _need(logp, "logp", torch.float32, ndim=2)
    R, C = logp.shape
    if tuple(g_logp.shape) != (R, C):
        raise RuntimeError("logsoftmax_rows_bwd: g_logp must match logp")
    g_y = torch.empty((R, int(Cpad)), dtype=torch.float32, device=logp.device)
    _call(logp.device, "upp_logsoftmax_rows_bwd", _abi.ptr(g_logp), _abi.ptr(logp), R, C, _abi.ptr(g_y), int(Cpad), int(Cpad))
    return g_y


def nll_mean_fwd(logp, target):
    """F.nll_loss(logp, target) (mean) -> (1,) f32; upp_nll_mean_fwd (two launches, fixed-order sums)."""
    _need(logp, "logp", torch.float32, ndim=2)
    R, C = logp.shape
    if not (isinstance(target, torch.Tensor) and target.is_cuda and target.dtype == torch.int64 and target.numel() == R and target.is_contiguous()):
        raise RuntimeError("nll_mean_fwd: target must be a contiguous int64 HIP (cuda) tensor with one entry per row")
    part = torch.empty(int(_abi.load().upp_nll_mean_part_floats(R)), dtype=torch.float32, device=logp.device)
    out = torch.empty(1, dtype=torch.float32, device=logp.device)
    _call(logp.device, "upp_nll_mean_fwd", _abi.ptr(logp), _abi.ptr(target), R, C, _abi.ptr(part), _abi.ptr(out))
    return out


def nll_mean_bwd(g_loss, target, R, C):
    """-> g_logp (R, C) = -g_loss / R at (r, target[r]), 0 elsewhere; g_loss a one-element device tensor; upp_nll_mean_bwd."""
    _need(target, "target", torch.int64)
    if tuple(target.shape) != (int(R),):
        raise RuntimeError(f"nll_mean_bwd: target must be ({int(R)},), got {tuple(target.shape)}")
    _need_f32(g_loss, "g_loss", (1,))
    _same_device(target, g_loss)
    g_logp = torch.empty((int(R), int(C)), dtype=torch.float32, device=target.device)
    _call(target.device, "upp_nll_mean_bwd", _abi.ptr(g_loss), _abi.ptr(target), int(R), int(C), _abi.ptr(g_logp))
    return g_logp


def noise_loss_fwd(pred, noise_vector, pn, want_score=True):
    """-> (loss (1,), score (B,P) or None) of the pre-task noise supervision (upp_noise_loss_fwd): pred (B,P,3), noise_vector (B,P-pn,3)."""
    _need(pred, "pred", torch.float32, 3, 3)
    _need(noise_vector, "noise_vector", torch.float32, 3, 3)
    B, P, _ = pred.shape
    if tuple(noise_vector.shape) != (B, P - int(pn), 3):
        raise RuntimeError("noise_loss_fwd: noise_vector must be (B, P - pn, 3)")
    part = torch.empty(int(_abi.load().upp_noise_loss_part_floats(B, P)), dtype=torch.float32, device=pred.device)
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    score = torch.empty((B, P), dtype=torch.float32, device=pred.device) if want_score else None
    _call(pred.device, "upp_noise_loss_fwd", _abi.ptr(pred), _abi.ptr(noise_vector), B, P, int(pn), _abi.ptr(part), _abi.ptr(loss), _abi.ptr(score))
    return loss, score


def noise_loss_bwd(g_loss, pred, noise_vector, pn):
    _need(pred, "pred", torch.float32, 3, 3)
    B, P, _ = pred.shape
    _need_f32(noise_vector, "noise_vector", (B, P - int(pn), 3))
    _need_f32(g_loss, "g_loss", (1,))
    _same_device(pred, noise_vector, g_loss)
    g_pred = torch.empty_like(pred)
    _call(pred.device, "upp_noise_loss_bwd", _abi.ptr(g_loss), _abi.ptr(pred), _abi.ptr(noise_vector), B, P, int(pn), _abi.ptr(g_pred))
    return g_pred


def rectify_select(feature, w0, b0, w1, b1, pts, keep, u=None, p=0.0, factor=1.0, nudge=0.2, want_pred=False, want_order=False, want_score=False):
    """Tail of the denoising prompter in two launches (upp_rectify_select): pred = score head(feature) * factor, moved = pts + nudge * pred,
    the `keep` least suspicious points of every cloud in descending-score order.  -> out (B,keep,3) [, pred (B,N,3)] [, order (B,N) int64] [, score (B,N)]."""
    _need(pts, "pts", torch.float32, 3, 3)
    B, N, _ = pts.shape
    for t, n_, shp in ((feature, "feature", (B, N, 32)), (w0, "w0", (64, 32)), (b0, "b0", (64,)), (w1, "w1", (3, 64)), (b1, "b1", (3,))):
        _need(t, n_, torch.float32)
        if tuple(t.shape) != shp:
            raise RuntimeError(f"rectify_select: {n_} must be {shp}, got {tuple(t.shape)}")
    if u is not None:
        _need(u, "u", torch.float32)
        if u.numel() != B * N * 64:
            raise RuntimeError("rectify_select: u must hold B*N*64 uniforms")
    dev = pts.device
    moved = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    score = torch.empty((B, N), dtype=torch.float32, device=dev)
    out = torch.empty((B, int(keep), 3), dtype=torch.float32, device=dev)
    pred = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if want_pred else None
    order = torch.empty((B, N), dtype=torch.int64, device=dev) if want_order else None
    _call(dev, "upp_rectify_select", _abi.ptr(feature), _abi.ptr(w0), _abi.ptr(b0), _abi.ptr(w1), _abi.ptr(b1), _abi.ptr(u), float(p), float(factor),
          _abi.ptr(pts), float(nudge), B, N, int(keep), _abi.ptr(pred), _abi.ptr(moved), _abi.ptr(score), _abi.ptr(out), _abi.ptr(order))
    res = (out,) + ((pred,) if want_pred else ()) + ((order,) if want_order else ()) + ((score,) if want_score else ())
    return res if len(res) > 1 else out


def group_max_fwd(x):
    """x (R,k,C) f32 contiguous -> (max over k (R,C), arg-max (R,C) uint8)  (upp_group_max_fwd)."""
    _need(x, "x", torch.float32, ndim=3)
    R, k, C = x.shape
    out = torch.empty((R, C), dtype=torch.float32, device=x.device)
    amax = torch.empty((R, C), dtype=torch.uint8, device=x.device)
    _call(x.device, "upp_group_max_fwd", _abi.ptr(x), R, k, C, _abi.ptr(out), _abi.ptr(amax))
    return out, amax


def group_max_bwd(g, amax, k):
    """g (R,C), amax (R,C) uint8 -> g_x (R,k,C): g at the arg-max row of every (group, column), zero elsewhere (upp_group_max_bwd)."""
    _need(g, "g", torch.float32, ndim=2)
    R, C = g.shape
    _need(amax, "amax", torch.uint8)
    if tuple(amax.shape) != (R, C):
        raise RuntimeError(f"group_max_bwd: amax must be ({R}, {C}), got {tuple(amax.shape)}")
    _same_device(g, amax)
    g_x = torch.empty((R, int(k), C), dtype=torch.float32, device=g.device)
    _call(g.device, "upp_group_max_bwd", _abi.ptr(g), _abi.ptr(amax), R, int(k), C, _abi.ptr(g_x))
    return g_x


def argsort_rows(key, descending=False):
    """Stable argsort of every row of `key` (..., N) f32 -> int64 indices of the same shape (upp_argsort_rows: rank counting, no library
    sort; NaN ranks as +inf, equal keys in index order)."""
    _need(key, "key", torch.float32)
    N = key.shape[-1]
    k2 = key.reshape(-1, N).contiguous()
    order = torch.empty(k2.shape, dtype=torch.int64, device=key.device)
    _call(key.device, "upp_argsort_rows", _abi.ptr(k2), k2.shape[0], N, 1 if descending else 0, _abi.ptr(order))
    return order.view(key.shape)


def wcolsum_partials(src, wts, chunks=None):
    """(chunks, W, C) partials of wts (n,W)^T . src (n,C) for W <= 4 over very many rows (upp_wcolsum_partials); sum over dim 0 = the product."""
    for t_, n_ in ((src, "src"), (wts, "wts")):
        if not (isinstance(t_, torch.Tensor) and t_.is_cuda and t_.dtype == torch.float32 and t_.dim() == 2 and t_.stride(1) == 1):
            raise RuntimeError(f"{n_} must be a 2-D f32 HIP (cuda) matrix with contiguous rows; upp_hip has no CPU path")
    _same_device(src, wts)
    n, C = src.shape
    W = wts.shape[1]
    if wts.shape[0] != n or W > 4 or C % 4:
        raise RuntimeError(f"wcolsum_partials: wts {tuple(wts.shape)} against src {tuple(src.shape)} (W <= 4, C % 4 == 0)")
    if chunks is None:
        chunks = max(1, min(256, (n + 255) // 256))
    dst = torch.empty((chunks, W, C), dtype=torch.float32, device=src.device)
    _call(src.device, "upp_wcolsum_partials", _abi.ptr(src), src.stride(0), _abi.ptr(wts), wts.stride(0), W, n, C, chunks, _abi.ptr(dst))
    return dst


def linear_smallk(x, w, bias=None, act=0):
    """act(x (...,K) . w (N,K)^T + bias) for K <= 64, N <= 256, any alignment (upp_linear_smallk_f32); act 0 none / 1 ReLU / 2 GELU."""
    for t_, n_ in ((x, "x"), (w, "w")):
        if not (isinstance(t_, torch.Tensor) and t_.is_cuda and t_.dtype == torch.float32):
            raise RuntimeError(f"{n_} must be a f32 HIP (cuda) tensor; upp_hip has no CPU path")
    _same_device(x, w)
    K, N = x.shape[-1], w.shape[0]
    if w.dim() != 2 or w.shape[1] != K:
        raise RuntimeError(f"linear_smallk: x (...,{K}) against w {tuple(w.shape)}")
    if bias is not None:
        _need(bias, "bias", torch.float32, 1, N)
    if K > 64 or N > 256:
        raise RuntimeError(f"linear_smallk serves K <= 64 and N <= 256, got K = {K}, N = {N}")
    x2 = x.reshape(-1, K)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    if w.stride(1) != 1:
        w = w.contiguous()
    out = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=torch.float32, device=x.device)
    _call(x.device, "upp_linear_smallk_f32", _abi.ptr(x2), x2.stride(0), _abi.ptr(w), w.stride(0), _abi.ptr(bias), _abi.ptr(out), N,
          x2.shape[0], N, K, int(act))
    return out


def linear_smallk_wgrad(g, x, chunks=None):
    """(chunks, N, K) partial weight gradients of a small Linear: sum over dim 0 = g^T . x (g (M,N), x (M,K), N K <= 2048);
    upp_linear_smallk_wgrad_f32."""
    _need_matrix(g, "g")
    _need_matrix(x, "x")
    M, N = g.shape
    K = x.shape[1]
    if x.shape[0] != M or N * K > 2048:
        raise RuntimeError(f"linear_smallk_wgrad: g {tuple(g.shape)} against x {tuple(x.shape)} (N K <= 2048)")
    if chunks is None:
        chunks = max(1, min(512, (M + 63) // 64))
    part = torch.empty((chunks, N, K), dtype=torch.float32, device=g.device)
    _call(g.device, "upp_linear_smallk_wgrad_f32", _abi.ptr(g), g.stride(0), _abi.ptr(x), x.stride(0), _abi.ptr(part), M, N, K, chunks)
    return part


def linear_smallk_gelu_d(x, w, bias):
    """-> (GELU(x . w^T + bias), GELU'(x . w^T + bias)) for K <= 64, N <= 256 in one pass (upp_linear_smallk_gelu_d_f32)."""
    for t_, n_ in ((x, "x"), (w, "w")):
        if not (isinstance(t_, torch.Tensor) and t_.is_cuda and t_.dtype == torch.float32):
            raise RuntimeError(f"{n_} must be a f32 HIP (cuda) tensor; upp_hip has no CPU path")
    _same_device(x, w)
    K, N = x.shape[-1], w.shape[0]
    if w.dim() != 2 or w.shape[1] != K or K > 64 or N > 256:
        raise RuntimeError(f"linear_smallk_gelu_d: x (...,{K}) against w {tuple(w.shape)} (K <= 64, N <= 256)")
    if bias is not None:
        _need(bias, "bias", torch.float32, 1, N)
    x2 = x.reshape(-1, K)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    if w.stride(1) != 1:
        w = w.contiguous()
    out = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=torch.float32, device=x.device)
    d = torch.empty_like(out)
    _call(x.device, "upp_linear_smallk_gelu_d_f32", _abi.ptr(x2), x2.stride(0), _abi.ptr(w), w.stride(0), _abi.ptr(bias), _abi.ptr(out), N,
          _abi.ptr(d), N, x2.shape[0], N, K)
    return out, d


def transpose(w, out=None):
    """W^T of a 2-D f32 matrix with contiguous rows (upp_transpose_f32); `out` (cols, rows) is overwritten in place when given."""
    if not _is_matrix(w):
        raise RuntimeError("transpose: a 2-D f32 HIP (cuda) matrix with contiguous rows is required (column windows are fine)")
    rows, cols = w.shape
    if out is None:
        out = torch.empty((cols, rows), dtype=torch.float32, device=w.device)
    _call(w.device, "upp_transpose_f32", _abi.ptr(w), w.stride(0), _abi.ptr(out), out.stride(0), rows, cols)
    return out


def linear_wgrad(g, x):
    """Partial weight gradients (splits, N, K) of y = x . W^T: sum over dim 0 = g^T . x  (g (M,N), x (M,K); upp_linear_wgrad_f32).
    The caller sums the splits (batched_sum / the deferred sums of a training step)."""
    _need_matrix(g, "g")
    _need_matrix(x, "x")
    _same_device(g, x)
    M, N = g.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise RuntimeError("linear_wgrad: row counts differ")
    if SPLIT_BF16 and WGRAD_SPLIT_BF16:
        return linear_wgrad_grouped([(g, x)])[0]
    splits = _abi.load().upp_linear_wgrad_splits(M, N, K)
    part = torch.empty((splits, N, K), dtype=torch.float32, device=g.device)
    _call(g.device, "upp_linear_wgrad_f32", _abi.ptr(g), g.stride(0), _abi.ptr(x), x.stride(0), _abi.ptr(part), M, N, K)
    return part


def linear_group_bias_usable(M, N, K, rows_per_group):
    """Does upp_linear_group_bias_f32 serve this problem (tall: the register-tiled kernel; groups of 2^s >= 32 rows; N, K % 4 == 0)?"""
    r = int(rows_per_group)
    if not (r >= 32 and (r & (r - 1)) == 0 and M % r == 0 and N % 4 == 0 and K % 4 == 0):
        return False
    tile = int(_abi.load().upp_linear_tile(M, N, K))
    return tile > 0 and bool(tile & 0x10000)


def linear_group_bias(a, w, bias, rows_per_group, frozen=False, planes=None):
    """C (M,N) = a (M,K) . w (N,K)^T + bias[m // rows_per_group] -- the bias of a GROUP of rows added in the GEMM's epilogue
    (upp_linear_group_bias_f32, or upp_linear_sb_group_bias_f32 for a frozen weight / a plane image handed over by the caller: see
    linear_f32); bias (M / rows_per_group, N) contiguous."""
    _need_matrix(a, "a")
    _need_matrix(w, "w")
    _need_matrix(bias, "bias")
    _same_device(a, w, bias)
    M, K = a.shape
    N = w.shape[0]
    r = int(rows_per_group)
    if w.shape[1] != K or not bias.is_contiguous() or tuple(bias.shape) != (M // r, N) or not linear_group_bias_usable(M, N, K, r):
        raise RuntimeError("linear_group_bias: shapes do not fit (see linear_group_bias_usable)")
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    sb = 0
    if (planes is not None or frozen) and linear_sb_usable(M, N, K) and a.stride(0) % 4 == 0 and a.data_ptr() % 16 == 0 and bias.data_ptr() % 16 == 0:
        sb = linear_sb_tile(M, N, K)
        if planes is None:
            planes = PLANES.get(w)
    ev0 = time_linear_calls.bracket()
    if sb:
        _call(a.device, "upp_linear_sb_group_bias_f32", _abi.ptr(a), a.stride(0), _abi.ptr(planes), _abi.ptr(bias), r.bit_length() - 1,
              _abi.ptr(out), N, M, N, K)
    else:
        _call(a.device, "upp_linear_group_bias_f32", _abi.ptr(a), a.stride(0), _abi.ptr(w), w.stride(0), _abi.ptr(bias), r.bit_length() - 1,
              _abi.ptr(out), N, M, N, K)
    if ev0 is not None:
        time_linear_calls.active.group_bias.append((M, N, K))
    time_linear_calls.bracket(ev0, M, N, K, LIN_BIAS, sb)
    return out


WGRAD_SPLIT_BF16 = os.environ.get("UPP_WGRAD_SPLIT_BF16", "1") != "0"     # grouped weight gradients on the bf16 pipe (wgrad_sb.hip)


def linear_wgrad_grouped(pairs):
    """pairs: list of (g (M,N), x (M,K)) -- the weight gradients of several Linear layers in ONE launch (upp_linear_wgrad_grouped_f32).
    -> list of partial gradients (splits_p, N_p, K_p); the caller sums each over dim 0 in order (batched_sum)."""
    if not pairs:
        return []
    import ctypes
    k = len(pairs)
    dev = pairs[0][0].device
    for g, x in pairs:
        for t, name in ((g, "g"), (x, "x")):
            if not (_is_matrix(t) and t.device == dev):
                raise RuntimeError(f"{name} must be a 2-D f32 matrix with contiguous rows on one HIP (cuda) device; upp_hip has no CPU path")
        if x.shape[0] != g.shape[0]:
            raise RuntimeError("linear_wgrad_grouped: row counts differ")
    M = (ctypes.c_int * k)(*[g.shape[0] for g, _ in pairs])
    N = (ctypes.c_int * k)(*[g.shape[1] for g, _ in pairs])
    K = (ctypes.c_int * k)(*[x.shape[1] for _, x in pairs])
    rows = (ctypes.c_int * k)()
    sb = SPLIT_BF16 and WGRAD_SPLIT_BF16
    _abi.check((_abi.load().upp_linear_wgrad_grouped_sb_rows if sb else _abi.load().upp_linear_wgrad_grouped_rows)(k, M, N, K, rows))
    parts = [torch.empty(((M[i] + rows[i] - 1) // rows[i], N[i], K[i]), dtype=torch.float32, device=dev) for i in range(k)]
    G = (ctypes.c_void_p * k)(*[g.data_ptr() for g, _ in pairs])
    X = (ctypes.c_void_p * k)(*[x.data_ptr() for _, x in pairs])
    P = (ctypes.c_void_p * k)(*[q.data_ptr() for q in parts])
    ldg = (ctypes.c_longlong * k)(*[g.stride(0) for g, _ in pairs])
    ldx = (ctypes.c_longlong * k)(*[x.stride(0) for _, x in pairs])
    _call(dev, "upp_linear_wgrad_grouped_sb" if sb else "upp_linear_wgrad_grouped_f32", G, ldg, X, ldx, P, M, N, K, rows, k)
    if time_linear_calls.active is not None:
        time_linear_calls.active.wgrad_groups.append([(M[i], N[i], K[i]) for i in range(k)])
    return parts


def rowln_fwd(x, add, prompts, mode, P, y, u, keep, gamma, beta, eps, Lout, want_xo=True, ybias=None):
    _need(x, "x", torch.float32, ndim=3)
    B, Lin, D = x.shape
    dev = x.device
    _need_f32(add, "add", (B, Lin, D), optional=True)
    if prompts is not None:
        if int(mode) in (1, 2):
            _need_f32(prompts, "prompts", (int(P), D))
        else:
            _need(prompts, "prompts", torch.float32)
    _need_f32(y, "y", (B, Lin, D), optional=True)
    _need_f32(ybias, "ybias", (D,), optional=True)
    _need_f32(u, "u", (B,), optional=True)
    _need_f32(gamma, "gamma", (D,), optional=True)
    _need_f32(beta, "beta", (D,), optional=gamma is None)
    _same_device(*[t for t in (x, add, prompts, y, ybias, u, gamma, beta) if t is not None])
    xo = torch.empty((B, Lout, D), dtype=torch.float32, device=dev) if want_xo else None
    if gamma is not None:
        h = torch.empty((B, Lout, D), dtype=torch.float32, device=dev)
        mean = torch.empty((B, Lout), dtype=torch.float32, device=dev)
        rstd = torch.empty((B, Lout), dtype=torch.float32, device=dev)
    else:
        h = mean = rstd = None
    _call(dev, "upp_rowln_fwd", _abi.ptr(x), _abi.ptr(add), _abi.ptr(prompts), int(mode), int(P), _abi.ptr(y), _abi.ptr(ybias),
          _abi.ptr(u), float(keep), _abi.ptr(gamma), _abi.ptr(beta), float(eps), _abi.ptr(xo), _abi.ptr(h), _abi.ptr(mean), _abi.ptr(rstd),
          B, Lin, Lout, D)
    return xo, h, mean, rstd


def rowln_bwd(g_xo, g_h, xo, mean, rstd, gamma, mode, u, keep, B, Lin, Lout, D, P, need_x, need_prompt, need_y, need_ln_part=False):
    if g_xo is None and g_h is None:
        raise RuntimeError("rowln_bwd: one of g_xo, g_h is required")
    _need_f32(g_xo, "g_xo", (B, Lout, D), optional=True)
    _need_f32(g_h, "g_h", (B, Lout, D), optional=True)
    with_ln = g_h is not None                                  # the saved rows and statistics are read only for the LayerNorm's backward
    _need_f32(xo, "xo", (B, Lout, D), optional=not with_ln)
    _need_f32(mean, "mean", (B, Lout), optional=not with_ln)
    _need_f32(rstd, "rstd", (B, Lout), optional=not with_ln)
    _need_f32(gamma, "gamma", (D,), optional=not with_ln)
    _need_f32(u, "u", (B,), optional=True)
    _same_device(*[t for t in (g_xo, g_h, xo, mean, rstd, gamma, u) if t is not None])
    dev = (g_xo if g_xo is not None else g_h).device
    g_x = torch.empty((B, Lin, D), dtype=torch.float32, device=dev) if need_x else None      # the kernel writes every row
    g_p = torch.empty((B, P, D), dtype=torch.float32, device=dev) if (need_prompt and P > 0 and mode in (1, 2)) else None
    g_y = torch.empty((B, Lin, D), dtype=torch.float32, device=dev) if need_y else None
    part = None
    if need_ln_part and g_h is not None:
        n = int(_abi.load().upp_rowln_part_floats(B, Lin, Lout, D, int(mode)))
        part = torch.empty((n // (2 * D), 2 * D), dtype=torch.float32, device=dev)     # per workgroup: [d_gamma | d_beta]
    _call(dev, "upp_rowln_bwd", _abi.ptr(g_xo), _abi.ptr(g_h), _abi.ptr(xo), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(gamma),
          int(mode), _abi.ptr(u), float(keep), _abi.ptr(g_x), _abi.ptr(g_p), _abi.ptr(g_y), _abi.ptr(part), B, Lin, Lout, D, P)
    return g_x, g_p, g_y, part


def bias_gelu_fwd(z, bias):
    _need(z, "z", torch.float32)
    _need(bias, "bias", torch.float32, ndim=1, last=z.shape[-1])
    h = torch.empty_like(z)
    _call(z.device, "upp_bias_gelu_fwd", _abi.ptr(z), _abi.ptr(bias), _abi.ptr(h), z.numel() // z.shape[-1], z.shape[-1])
    return h


def bias_gelu_fwd_d(z, bias):
    """-> (GELU(z + bias), GELU'(z + bias)) in one pass."""
    _need(z, "z", torch.float32)
    _need(bias, "bias", torch.float32, ndim=1, last=z.shape[-1])
    h, d = torch.empty_like(z), torch.empty_like(z)
    _call(z.device, "upp_bias_gelu_fwd_d", _abi.ptr(z), _abi.ptr(bias), _abi.ptr(h), _abi.ptr(d), z.numel() // z.shape[-1], z.shape[-1])
    return h, d


def bias_gelu_bwd(g_h, z, bias):
    g_z = torch.empty_like(z)
    _call(z.device, "upp_bias_gelu_bwd", _abi.ptr(g_h), _abi.ptr(z), _abi.ptr(bias), _abi.ptr(g_z), z.numel() // z.shape[-1], z.shape[-1])
    return g_z


def ln_param_grad(g_h, xo, mean, rstd, chunks=32):
    rows = g_h.numel() // g_h.shape[-1]
    D = g_h.shape[-1]
    part = torch.empty((2, chunks, D), dtype=torch.float32, device=g_h.device)
    _call(g_h.device, "upp_ln_param_grad", _abi.ptr(g_h), _abi.ptr(xo), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(part), rows, D, chunks)
    return part          # (2, chunks, D): [0] d_gamma partials, [1] d_beta partials; the caller sums over the chunks


# The longest sequence upp_attn_fwd / upp_attn_bwd serve (UPP_ATTN_MAX_L of include/upp_hip.h; tests/test_attention_stream_host.py holds the
# two together).  The models' `fusable` predicates read it, so a longer sequence takes the torch formulation instead of raising.
ATTN_MAX_L = 2048


def _attn_operand(t, name, count, aligned=True):
    """float32, contiguous, `count` elements; 16-byte aligned where the kernels load the operand in 16-byte pieces"""
    _need(t, name, torch.float32)
    if t.numel() != count:
        raise RuntimeError(f"{name} must hold {count} elements, got {tuple(t.shape)}")
    if aligned and t.data_ptr() % 16:
        raise RuntimeError(f"{name} must be 16-byte aligned (the attention kernels load 16-byte pieces); got a view at a storage offset")


def attn_fwd(qkv, B, L, H, scale):
    """qkv (B, L, 3, H, 64) -> ctx (B, L, H * 64), lse (B, H, L).  L <= 96: attn_flash16.hip, L <= 160: attn_long.hip,
    L <= ATTN_MAX_L: attn_stream.hip (K / V streamed through the LDS, online softmax); longer sequences raise.
    qkv: float32, contiguous, 16-byte aligned."""
    hd = 64
    _attn_operand(qkv, "qkv", B * L * 3 * H * hd)
    ctx = torch.empty((B, L, H * hd), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=qkv.device)
    _call(qkv.device, "upp_attn_fwd", _abi.ptr(qkv), _abi.ptr(ctx), _abi.ptr(lse), B, L, H, hd, float(scale))
    return ctx, lse


def attn_bwd(qkv, ctx, d_ctx, lse, B, L, H, scale):
    """d_qkv (B, L, 3, H, 64) from d_ctx and the forward's ctx / lse; the same three kernel families and the same range as attn_fwd.
    No atomics at any L: two calls on the same inputs give the same bits.
    All four operands: float32, contiguous, on one device; qkv, ctx and d_ctx 16-byte aligned."""
    hd = 64
    _attn_operand(qkv, "qkv", B * L * 3 * H * hd)
    _attn_operand(ctx, "ctx", B * L * H * hd)
    _attn_operand(d_ctx, "d_ctx", B * L * H * hd)
    _attn_operand(lse, "lse", B * H * L, aligned=False)
    _same_device(qkv, ctx, d_ctx, lse)
    d_qkv = torch.empty_like(qkv)
    _call(qkv.device, "upp_attn_bwd", _abi.ptr(qkv), _abi.ptr(ctx), _abi.ptr(d_ctx), _abi.ptr(lse), _abi.ptr(d_qkv), B, L, H, hd, float(scale))
    return d_qkv


def _xattn_operand(t, name, B, L, H):
    """One strided operand of upp_xattn_fwd / _bwd: float32 (B, L, H * 64) whose last dimension is contiguous, whose row stride rs is a
    multiple of 4 and >= H * 64, whose sample stride is L * rs, 16-byte aligned -> rs.  (The device is checked after every operand's layout, by
    _xattn_device, so that the layout rules can be tested on a host without one.)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be torch.float32, got {t.dtype}")
    if t.dim() != 3 or t.shape[0] != B or t.shape[1] != L:
        raise RuntimeError(f"{name} must be (B, L, H * 64) = ({B}, {L}, {H * 64}), got {tuple(t.shape)}")
    if t.shape[2] != H * 64:
        raise RuntimeError(f"{name}: the cross-attention kernels serve head_dim 64 only (last dimension {H * 64} for {H} heads), got {t.shape[2]}")
    if t.stride(2) != 1:
        raise RuntimeError(f"{name}: the last dimension must be contiguous, got strides {tuple(t.stride())}")
    rs = t.stride(1) if L > 1 else (t.stride(0) if B > 1 else H * 64)
    if rs < H * 64 or rs % 4:
        raise RuntimeError(f"{name}: the row stride must be a multiple of 4 floats and at least H * 64 = {H * 64}, got {rs}")
    if B > 1 and t.stride(0) != L * rs:
        raise RuntimeError(f"{name}: the sample stride must be L * row stride = {L * rs}, got {t.stride(0)}")
    if t.data_ptr() % 16:
        raise RuntimeError(f"{name} must be 16-byte aligned (the attention kernels load 16-byte pieces); got a view at a storage offset")
    return rs


def _xattn_device(**tensors):
    for name, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a HIP (cuda) tensor; upp_hip has no CPU path")
    _same_device(*tensors.values())


def _xattn_lengths(B, Lq, Lk, H):
    B, Lq, Lk, H = int(B), int(Lq), int(Lk), int(H)
    if B < 0 or H < 1 or Lq < 1 or Lk < 1:
        raise RuntimeError(f"cross-attention needs B >= 0, H >= 1 and lengths >= 1, got B = {B}, H = {H}, Lq = {Lq}, Lk = {Lk}")
    if Lq > ATTN_MAX_L or Lk > ATTN_MAX_L:
        raise RuntimeError(f"cross-attention serves lengths up to ATTN_MAX_L = {ATTN_MAX_L}, got Lq = {Lq}, Lk = {Lk}")
    return B, Lq, Lk, H


def _xattn_dense(ctx, d_ctx, lse, B, Lq, H):
    """The dense operands of the backward entry points: ctx, d_ctx (B, Lq, H * 64) 16-byte aligned, lse (B, H, Lq)."""
    for t, name, count, aligned in ((ctx, "ctx", B * Lq * H * 64, True), (d_ctx, "d_ctx", B * Lq * H * 64, True), (lse, "lse", B * H * Lq, False)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != count:
            raise RuntimeError(f"{name} must be a dense float32 tensor of {count} elements")
        if aligned and t.data_ptr() % 16:
            raise RuntimeError(f"{name} must be 16-byte aligned (the attention kernels load 16-byte pieces); got a view at a storage offset")


def _xattn_splits(Lq, Lk, split_q, split_k):
    split_q, split_k = int(split_q), int(split_k)
    if not 0 <= split_q <= Lq:
        raise RuntimeError(f"prefix attention needs 0 <= split_q <= Lq = {Lq}, got {split_q}")
    if not 1 <= split_k <= Lk:
        raise RuntimeError(f"prefix attention needs 1 <= split_k <= Lk = {Lk} (every query row sees at least one key), got {split_k}")
    return split_q, split_k


def _xattn_fwd(q, k, v, B, Lq, Lk, H, scale, splits=None):
    """xattn_fwd (splits None: upp_xattn_fwd) and xattn_prefix_fwd (splits (split_q, split_k): upp_xattn_prefix_fwd)"""
    B, Lq, Lk, H = _xattn_lengths(B, Lq, Lk, H)
    tail = () if splits is None else _xattn_splits(Lq, Lk, *splits)
    q_rs = _xattn_operand(q, "q", B, Lq, H)
    k_rs = _xattn_operand(k, "k", B, Lk, H)
    v_rs = _xattn_operand(v, "v", B, Lk, H)
    _xattn_device(q=q, k=k, v=v)
    ctx = torch.empty((B, Lq, H * 64), dtype=torch.float32, device=q.device)
    lse = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    _call(q.device, "upp_xattn_fwd" if splits is None else "upp_xattn_prefix_fwd", _abi.ptr(q), _abi.ptr(k), _abi.ptr(v), _abi.ptr(ctx),
          _abi.ptr(lse), B, Lq, Lk, H, 64, q_rs, k_rs, v_rs, float(scale), *tail)
    return ctx, lse


def _xattn_bwd(q, k, v, ctx, d_ctx, lse, B, Lq, Lk, H, scale, splits=None):
    """xattn_bwd (splits None: upp_xattn_bwd) and xattn_prefix_bwd (splits (split_q, split_k): upp_xattn_prefix_bwd)"""
    B, Lq, Lk, H = _xattn_lengths(B, Lq, Lk, H)
    tail = () if splits is None else _xattn_splits(Lq, Lk, *splits)
    q_rs = _xattn_operand(q, "q", B, Lq, H)
    k_rs = _xattn_operand(k, "k", B, Lk, H)
    v_rs = _xattn_operand(v, "v", B, Lk, H)
    _xattn_dense(ctx, d_ctx, lse, B, Lq, H)
    _xattn_device(q=q, k=k, v=v, ctx=ctx, d_ctx=d_ctx, lse=lse)
    d_q = torch.empty((B, Lq, H * 64), dtype=torch.float32, device=q.device)
    d_k = torch.empty((B, Lk, H * 64), dtype=torch.float32, device=q.device)
    d_v = torch.empty((B, Lk, H * 64), dtype=torch.float32, device=q.device)
    _call(q.device, "upp_xattn_bwd" if splits is None else "upp_xattn_prefix_bwd", _abi.ptr(q), _abi.ptr(k), _abi.ptr(v), _abi.ptr(ctx),
          _abi.ptr(d_ctx), _abi.ptr(lse), _abi.ptr(d_q), _abi.ptr(d_k), _abi.ptr(d_v), B, Lq, Lk, H, 64, q_rs, k_rs, v_rs, H * 64, H * 64, H * 64,
          float(scale), *tail)
    return d_q, d_k, d_v


def xattn_fwd(q, k, v, B, Lq, Lk, H, scale):
    """softmax(q k^T scale) v with queries and keys from two sequences (csrc/attn_stream.hip): q (B, Lq, H * 64), k and v (B, Lk, H * 64)
    -> ctx (B, Lq, H * 64), lse (B, H, Lq), both dense.  The operands may be views (a slice of a packed [k|v] or qkv product): see
    _xattn_operand for the stride rule; the strides are taken from the tensors.  1 <= Lq, Lk <= ATTN_MAX_L; everything else raises
    before a launch."""
    return _xattn_fwd(q, k, v, B, Lq, Lk, H, scale)


def xattn_bwd(q, k, v, ctx, d_ctx, lse, B, Lq, Lk, H, scale):
    """-> (d_q (B, Lq, H * 64), d_k, d_v (B, Lk, H * 64)) from d_ctx and the forward's ctx / lse.  q, k, v as in xattn_fwd; ctx, d_ctx and
    lse dense.  The three gradients are fresh dense tensors (so they overlap nothing), every element written by exactly one workgroup: no
    atomics, two calls give the same bits."""
    return _xattn_bwd(q, k, v, ctx, d_ctx, lse, B, Lq, Lk, H, scale)


def xattn_prefix_fwd(q, k, v, B, Lq, Lk, H, scale, split_q, split_k):
    """xattn_fwd under the prefix-visibility mask of csrc/attn_stream.hip: query rows < split_q see the keys < split_k, the other rows see
    all Lk keys (AdaPoinTr's denoising queries: Lq = Lk = L, both splits L - D) -> ctx (B, Lq, H * 64), lse (B, H, Lq) over the visible keys.
    Operands and their checks as in xattn_fwd; 0 <= split_q <= Lq and 1 <= split_k <= Lk, everything else raises before a launch."""
    return _xattn_fwd(q, k, v, B, Lq, Lk, H, scale, (split_q, split_k))


def xattn_prefix_bwd(q, k, v, ctx, d_ctx, lse, B, Lq, Lk, H, scale, split_q, split_k):
    """-> (d_q, d_k, d_v) of xattn_prefix_fwd, as xattn_bwd returns them: fresh dense tensors, every element written by exactly one
    workgroup, two calls give the same bits.  Keys no row sees (split_q == Lq, keys >= split_k) get zero gradients."""
    return _xattn_bwd(q, k, v, ctx, d_ctx, lse, B, Lq, Lk, H, scale, (split_q, split_k))


# ------------------------------------------------------------------ prompt propagation
def prop_pool_fwd(X, i1, u, keep, groups):
    D = X.shape[-1]
    pooled = torch.empty((groups, D), dtype=torch.float32, device=X.device)
    amax = torch.empty((groups, D), dtype=torch.uint8, device=X.device)
    _call(X.device, "upp_prop_pool_fwd", _abi.ptr(X), _abi.ptr(i1), _abi.ptr(u), float(keep), _abi.ptr(pooled), _abi.ptr(amax), groups, D)
    return pooled, amax


def prop_pool_bwd(g_pooled, amax, i1, u, keep, rows):
    groups, D = g_pooled.shape
    g_X = torch.empty((rows, D), dtype=torch.float32, device=g_pooled.device)
    _call(g_pooled.device, "upp_prop_pool_bwd", _abi.ptr(g_pooled), _abi.ptr(amax), _abi.ptr(i1), _abi.ptr(u), float(keep),
          _abi.ptr(g_X), rows, groups, D)
    return g_X


def prop_interp_fwd(X, lc, i2, idx8, w8, B, Lp, T, G2):
    D = X.shape[-1]
    out = torch.empty_like(X)
    _call(X.device, "upp_prop_interp_fwd", _abi.ptr(X), _abi.ptr(lc), _abi.ptr(i2), _abi.ptr(idx8), _abi.ptr(w8), _abi.ptr(out), B, Lp, T, G2, D)
    return out


def prop_interp_bwd(g_out, i2, idx8, w8, B, Lp, T, G2):
    D = g_out.shape[-1]
    g_c2 = torch.empty((B * G2, D), dtype=torch.float32, device=g_out.device)
    g_X = torch.empty_like(g_out)
    _call(g_out.device, "upp_prop_interp_bwd", _abi.ptr(g_out), _abi.ptr(i2), _abi.ptr(idx8), _abi.ptr(w8), _abi.ptr(g_c2), _abi.ptr(g_X),
          B, Lp, T, G2, D)
    return g_c2, g_X


CSR_MAX_ROWS = 15360       # upp_csr_build keeps one counter per row beside its 1024-entry scan in 64 KB of LDS; beyond: UPP_E_RANGE


def csr_build(keys, rows, seg_len=None, seg_rows=0):
    """Stable inverse of an int32 index list -> (start (rows+1), perm (n)); see upp_csr_build."""
    _need(keys, "keys", torch.int32)
    n = keys.numel()
    start = torch.empty(rows + 1, dtype=torch.int32, device=keys.device)
    perm = torch.empty(n, dtype=torch.int32, device=keys.device)
    _call(keys.device, "upp_csr_build", _abi.ptr(keys), n, int(seg_len or n), int(seg_rows), int(rows), _abi.ptr(start), _abi.ptr(perm))
    return start, perm


def prop_index(c1, c2, i1, i2, gather_idx, Lp, off, eps):
    """-> (i1a, i2a int32 absolute rows, idx8 int32 (B,T,8), w8 f32 (B,T,8)); see upp_prop_index."""
    _need(c1, "center1", torch.float32, 3, 3)
    _need(c2, "center2", torch.float32, 3, 3)
    _need(i1, "center1_idx", torch.int64)
    _need(i2, "center2_idx", torch.int64)
    B, T, _ = c1.shape
    G2 = c2.shape[1]
    if i1.numel() != B * G2 * 8 or i2.numel() != B * G2:
        raise RuntimeError("prop_index: index tensors do not match the centre shapes")
    dev = c1.device
    i1a = torch.empty(B * G2 * 8, dtype=torch.int32, device=dev)
    i2a = torch.empty(B * G2, dtype=torch.int32, device=dev)
    idx8 = torch.empty((B, T, 8), dtype=torch.int32, device=dev)
    w8 = torch.empty((B, T, 8), dtype=torch.float32, device=dev)
    _call(dev, "upp_prop_index", _abi.ptr(c1), _abi.ptr(c2), _abi.ptr(i1), _abi.ptr(i2), int(bool(gather_idx)), B, T, G2, int(Lp), int(off),
          float(eps), _abi.ptr(i1a), _abi.ptr(i2a), _abi.ptr(idx8), _abi.ptr(w8))
    return i1a, i2a, idx8, w8


def _prop_args(B, Lp, D, rows, cols=(), mbias=None, u=None, groups=None, u_dp=None):
    """The operand check of the fused step's wrappers, metadata only: rows = (name, tensor) token matrices (B, L', D), cols = per-column
    vectors (D,), all f32; optional: the frozen bias mbias (D,), the stochastic-depth uniforms u (groups,) per group and u_dp (B,) per sample."""
    for name, t in rows:
        _need_f32(t, name, (B, Lp, D))
    for name, t in cols:
        _need_f32(t, name, (D,))
    _need_f32(mbias, "mbias", (D,), optional=True)
    _need_f32(u, "u", (groups,), optional=True)
    _need_f32(u_dp, "u_dp", (B,), optional=True)
    _same_device(*[t for _, t in (*rows, *cols)], *[t for t in (mbias, u, u_dp) if t is not None])


def _prop_fwd_outputs(groups, D, dev):
    """(pooled, amax, part, mean, rstd) of the step's forward."""
    f32 = dict(dtype=torch.float32, device=dev)
    return (torch.empty((groups, D), **f32), torch.empty((groups, D), dtype=torch.uint8, device=dev),
            torch.empty(_abi.load().upp_prop_part_floats(groups, D), **f32), torch.empty(D, **f32), torch.empty(D, **f32))


def _prop_bwd_outputs(groups, D, dev):
    """(g_c2, part, g_gamma, g_beta) of the step's backward."""
    f32 = dict(dtype=torch.float32, device=dev)
    return (torch.empty((groups, D), **f32), torch.empty(_abi.load().upp_prop_part_floats(groups, D), **f32), torch.empty(D, **f32),
            torch.empty(D, **f32))


def prop_fwd(X, i1, u, keep, i2, idx8, w8, gamma, beta, running_mean, running_var, momentum, eps, training, B, Lp, T, G2):
    """-> (out, pooled, amax, mean, rstd); upp_prop_fwd."""
    D, dev = X.shape[-1], X.device
    _prop_args(B, Lp, D, (("X", X),), (("gamma", gamma), ("beta", beta)), u=u, groups=B * G2)
    pooled, amax, part, mean, rstd = _prop_fwd_outputs(B * G2, D, dev)
    out = torch.empty_like(X)
    _call(dev, "upp_prop_fwd", _abi.ptr(X), _abi.ptr(i1), _abi.ptr(u), float(keep), _abi.ptr(i2), _abi.ptr(idx8), _abi.ptr(w8),
          _abi.ptr(gamma), _abi.ptr(beta), _abi.ptr(running_mean), _abi.ptr(running_var), float(momentum), float(eps), int(bool(training)),
          _abi.ptr(pooled), _abi.ptr(amax), _abi.ptr(part), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(out), B, Lp, T, G2, D)
    return out, pooled, amax, mean, rstd


def prop_bwd(g_out, pooled, amax, mean, rstd, gamma, u, keep, w8, csr1, csr2, csr8, training, B, Lp, T, G2):
    """-> (g_X, g_gamma, g_beta); upp_prop_bwd."""
    D, dev = g_out.shape[-1], g_out.device
    _prop_args(B, Lp, D, (("g_out", g_out),), (("mean", mean), ("rstd", rstd), ("gamma", gamma)), u=u, groups=B * G2)
    g_c2, part, g_gamma, g_beta = _prop_bwd_outputs(B * G2, D, dev)
    g_X = torch.empty_like(g_out)
    _call(dev, "upp_prop_bwd", _abi.ptr(g_out), _abi.ptr(pooled), _abi.ptr(amax), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(gamma), _abi.ptr(u),
          float(keep), _abi.ptr(w8), _abi.ptr(csr1[0]), _abi.ptr(csr1[1]), _abi.ptr(csr2[0]), _abi.ptr(csr2[1]), _abi.ptr(csr8[0]),
          _abi.ptr(csr8[1]), int(bool(training)), _abi.ptr(g_c2), _abi.ptr(part), _abi.ptr(g_gamma), _abi.ptr(g_beta), _abi.ptr(g_X),
          B, Lp, T, G2, D)
    return g_X, g_gamma, g_beta


def prop_res_pool_fwd(x2, m, mbias, u_dp, keep_dp, i1, u, keep, running_mean, running_var, momentum, eps, training, G2):
    """The pool + statistics + finalize launches of prop_fwd on the rows x3 = x2 + dp_scale(u_dp) (m + mbias), formed where they are gathered
    -> (pooled, amax, part, mean, rstd); upp_prop_res_pool_fwd."""
    _need(x2, "x2", torch.float32, ndim=3)
    B, Lp, D = x2.shape
    _prop_args(B, Lp, D, (("x2", x2), ("m", m)), mbias=mbias, u=u, groups=B * G2, u_dp=u_dp)
    _need(i1, "i1", torch.int32)
    if i1.numel() != B * G2 * 8:
        raise RuntimeError("prop_res_pool_fwd: i1 must hold 8 rows for each of the B * G2 groups")
    pooled, amax, part, mean, rstd = _prop_fwd_outputs(B * G2, D, x2.device)
    _call(x2.device, "upp_prop_res_pool_fwd", _abi.ptr(x2), _abi.ptr(m), _abi.ptr(mbias), _abi.ptr(u_dp), float(keep_dp), _abi.ptr(i1), _abi.ptr(u),
          float(keep), _abi.ptr(running_mean), _abi.ptr(running_var), float(momentum), float(eps), int(bool(training)), _abi.ptr(pooled),
          _abi.ptr(amax), _abi.ptr(part), _abi.ptr(mean), _abi.ptr(rstd), B, Lp, int(G2), D)
    return pooled, amax, part, mean, rstd


def prop_res_bwd(g_out, pooled, amax, mean, rstd, gamma, u, keep, w8, csr1, csr2, csr8, training, u_dp, keep_dp, B, Lp, T, G2):
    """prop_bwd with the gradient of x3 leaving as the residual's two gradients -> (g_x2, g_m, g_gamma, g_beta); upp_prop_res_bwd."""
    D, dev = g_out.shape[-1], g_out.device
    _prop_args(B, Lp, D, (("g_out", g_out),), (("mean", mean), ("rstd", rstd), ("gamma", gamma)), u=u, groups=B * G2, u_dp=u_dp)
    g_c2, part, g_gamma, g_beta = _prop_bwd_outputs(B * G2, D, dev)
    g_x2, g_m = torch.empty_like(g_out), torch.empty_like(g_out)
    _call(dev, "upp_prop_res_bwd", _abi.ptr(g_out), _abi.ptr(pooled), _abi.ptr(amax), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(gamma),
          _abi.ptr(u), float(keep), _abi.ptr(w8), _abi.ptr(csr1[0]), _abi.ptr(csr1[1]), _abi.ptr(csr2[0]), _abi.ptr(csr2[1]),
          _abi.ptr(csr8[0]), _abi.ptr(csr8[1]), int(bool(training)), _abi.ptr(u_dp), float(keep_dp), _abi.ptr(g_c2), _abi.ptr(part),
          _abi.ptr(g_gamma), _abi.ptr(g_beta), _abi.ptr(g_x2), _abi.ptr(g_m), B, Lp, T, G2, D)
    return g_x2, g_m, g_gamma, g_beta


def prop_w8_grad(g_out, X, pooled, bn_stats, i2, idx8, B, Lp, T, G2):
    """Gradient w.r.t. the interpolation weights (B,T,8); bn_stats = (mean, rstd, gamma, beta) saved by prop_fwd, or None when `pooled`
    already holds the post-BatchNorm rows (prop_interp).  See upp_prop_w8_grad."""
    _need(g_out, "g_out", torch.float32)
    _need(X, "X", torch.float32)
    _need(pooled, "pooled", torch.float32)
    D = g_out.shape[-1]
    if g_out.numel() != B * Lp * D or X.numel() != B * Lp * D or pooled.numel() != B * G2 * D or idx8.numel() != B * T * 8 or i2.numel() != B * G2:
        raise RuntimeError("prop_w8_grad: operand shapes do not match (B, L', T, G2, D)")
    g_w8 = torch.empty((B, T, 8), dtype=torch.float32, device=g_out.device)
    st = bn_stats if bn_stats is not None else (None, None, None, None)
    _call(g_out.device, "upp_prop_w8_grad", _abi.ptr(g_out), _abi.ptr(X), _abi.ptr(pooled), _abi.ptr(st[0]), _abi.ptr(st[1]), _abi.ptr(st[2]),
          _abi.ptr(st[3]), _abi.ptr(i2), _abi.ptr(idx8), _abi.ptr(g_w8), B, Lp, T, G2, D)
    return g_w8


def prop_weights_bwd(c1, c2, idx8, g_w8, eps):
    """(g_c1 (B,T,3), g_c2 (B,G2,3)) from the gradient of the interpolation weights; see upp_prop_weights_bwd."""
    _need(c1, "c1", torch.float32, ndim=3)
    _need(c2, "c2", torch.float32, ndim=3)
    _need(g_w8, "g_w8", torch.float32)
    B, T, _ = c1.shape
    G2 = c2.shape[1]
    if c1.shape[2] != 3 or c2.shape[2] != 3 or c2.shape[0] != B or idx8.numel() != B * T * 8 or g_w8.numel() != B * T * 8 or idx8.dtype != torch.int32:
        raise RuntimeError("prop_weights_bwd: operand shapes do not match")
    g_c1, g_c2 = torch.empty_like(c1), torch.empty_like(c2)
    _call(c1.device, "upp_prop_weights_bwd", _abi.ptr(c1), _abi.ptr(c2), _abi.ptr(idx8), _abi.ptr(g_w8), float(eps), _abi.ptr(g_c1), _abi.ptr(g_c2),
          B, T, G2)
    return g_c1, g_c2


# ------------------------------------------------------------------ row operators of the frozen prompter branches
def _drop_seed(drop):
    """drop = (p, seed int64 device scalar, seed_add, salt) -> checked tuple for upp_bn_rows_drop_fwd / _bwd."""
    p, seed, add, salt = drop
    if not (isinstance(seed, torch.Tensor) and seed.is_cuda and seed.dtype == torch.int64 and seed.numel() == 1):
        raise RuntimeError("dropout seed must be a one-element int64 HIP (cuda) tensor (the layer's num_batches_tracked)")
    return float(p), seed, int(add), int(salt) & 0xFFFFFFFF


def _bn_params(x, gamma, beta, running_mean, running_var, training, affine_optional=True):
    """The per-column operands of a BatchNorm over the rows of x (R, C): each (C,) f32 on x's device, or None where the kernel takes that
    (identity affine; batch statistics without running buffers).  Training-mode statistics of ONE row are refused, as torch refuses them
    ("Expected more than 1 value per channel when training"): the variance is 0 and its unbiased form 0 / 0."""
    R, C = x.shape
    for t, name, optional in ((gamma, "gamma", affine_optional), (beta, "beta", affine_optional),
                              (running_mean, "running_mean", bool(training)), (running_var, "running_var", bool(training))):
        _need_f32(t, name, (C,), optional=optional)
        if t is not None:
            _same_device(x, t)
    if (running_mean is None) != (running_var is None):
        raise RuntimeError("running_mean and running_var come together or not at all")
    if training and R < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")


def bn_rows_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, training, relu, want_stats=False, drop=None):
    """drop = (p, seed, seed_add, salt): nn.Dropout(p) on the output in the same pass (training only; upp_bn_rows_drop_fwd)."""
    _need(x, "x", torch.float32, ndim=2)
    R, C = x.shape
    dev = x.device
    _bn_params(x, gamma, beta, running_mean, running_var, training)
    part = torch.empty(_abi.load().upp_bn_rows_part_floats(R, C), dtype=torch.float32, device=dev) if training else None
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    if drop is not None and drop[0] > 0.0:
        if not training:
            raise RuntimeError("bn_rows_fwd: dropout belongs to the training-mode form")
        p, seed, add, salt = _drop_seed(drop)
        _call(dev, "upp_bn_rows_drop_fwd", _abi.ptr(x), _abi.ptr(gamma), _abi.ptr(beta), _abi.ptr(running_mean), _abi.ptr(running_var),
              float(momentum), float(eps), int(bool(relu)), p, _abi.ptr(seed), add, salt, _abi.ptr(part), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(y), R, C)
    else:
        _call(dev, "upp_bn_rows_fwd", _abi.ptr(x), _abi.ptr(gamma), _abi.ptr(beta), _abi.ptr(running_mean), _abi.ptr(running_var),
              float(momentum), float(eps), int(bool(training)), int(bool(relu)), _abi.ptr(part), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(y), R, C)
    return (y, mean, rstd) if want_stats else y


def bn_rows_bwd(x, g, mean, rstd, gamma, beta, relu, want_gx=True, drop=None):
    """Backward of the training-mode bn_rows_fwd: -> (g_x or None, g_gamma, g_beta).  drop: (p, seed, seed_add, salt) -- the forward's mask."""
    _need(x, "x", torch.float32, ndim=2)
    _need(g, "g", torch.float32, ndim=2)
    R, C = x.shape
    dev = x.device
    _need(mean, "mean", torch.float32, ndim=1, last=C)
    _need(rstd, "rstd", torch.float32, ndim=1, last=C)
    if g.shape != x.shape or any(t is not None and (t.shape != (C,) or t.dtype != torch.float32 or not t.is_cuda) for t in (gamma, beta)):
        raise RuntimeError("bn_rows_bwd: g must match x, gamma / beta must be (C,) f32 HIP tensors")
    part = torch.empty(_abi.load().upp_bn_rows_part_floats(R, C), dtype=torch.float32, device=dev)
    g_gamma = torch.empty(C, dtype=torch.float32, device=dev)
    g_beta = torch.empty(C, dtype=torch.float32, device=dev)
    g_x = torch.empty_like(x) if want_gx else None
    if drop is not None and drop[0] > 0.0:
        p, seed, add, salt = _drop_seed(drop)
        _call(dev, "upp_bn_rows_drop_bwd", _abi.ptr(x), _abi.ptr(g), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(gamma), _abi.ptr(beta), int(bool(relu)),
              p, _abi.ptr(seed), add, salt, _abi.ptr(part), _abi.ptr(g_gamma), _abi.ptr(g_beta), _abi.ptr(g_x), R, C)
    else:
        _call(dev, "upp_bn_rows_bwd", _abi.ptr(x), _abi.ptr(g), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(gamma), _abi.ptr(beta), int(bool(relu)),
              _abi.ptr(part), _abi.ptr(g_gamma), _abi.ptr(g_beta), _abi.ptr(g_x), R, C)
    return g_x, g_gamma, g_beta


def sqdist_topk(q, src, k):
    """q (B,N,3), src (B,S,3) -> (dist (B,N,k) f32, idx (B,N,k) int64): k nearest by the reference's square_distance form."""
    _need(q, "q", torch.float32, ndim=3, last=3)
    _need(src, "src", torch.float32, ndim=3, last=3)
    _same_device(q, src)
    B, N, _ = q.shape
    S = src.shape[1]
    if src.shape[0] != B:
        raise RuntimeError("q / src batch sizes differ")
    dist = torch.empty((B, N, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, N, k), dtype=torch.int64, device=q.device)
    _call(q.device, "upp_sqdist_topk", _abi.ptr(q), _abi.ptr(src), _abi.ptr(dist), _abi.ptr(idx), B, N, S, int(k))
    return dist, idx


def interp_fwd(dist, idx, feat, k, eps, out=None, col0=0):
    """dist / idx: (B,N,S') views whose last dim is contiguous (a sorted neighbour table); feat (B,S,C)."""
    _need(feat, "feat", torch.float32, ndim=3)
    B, S, C = feat.shape
    N = dist.shape[1]
    for t, name, dt in ((dist, "dist", torch.float32), (idx, "idx", torch.int64)):
        if not t.is_cuda or t.dtype != dt or t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != N * t.stride(1):
            raise RuntimeError(f"{name} must be a HIP {dt} (B,N,S') table with contiguous rows")
    if dist.stride(1) != idx.stride(1) or dist.shape[:2] != idx.shape[:2] or dist.shape[0] != B:
        raise RuntimeError("dist / idx must share shape and row stride")
    if out is None:
        out = torch.empty((B, N, C), dtype=torch.float32, device=feat.device)
    _need(out, "out", torch.float32, ndim=3)
    if tuple(out.shape[:2]) != (B, N) or int(col0) < 0 or out.shape[2] < int(col0) + C:
        raise RuntimeError(f"out must be ({B}, {N}, >= col0 + {C}), got {tuple(out.shape)} with col0 = {int(col0)}")
    _same_device(feat, out, dist, idx)
    _call(feat.device, "upp_interp_fwd", _abi.ptr(dist), _abi.ptr(idx), dist.stride(1), _abi.ptr(feat), _abi.ptr(out), out.shape[-1], int(col0),
          B, N, S, C, int(k), float(eps))
    return out


def interp_affine_fwd(dist, idx, feat, x3, wt, k, eps):
    """interp_fwd into a dense (B,N,C) matrix plus x3 (B,N,3) . wt (3,C); k <= 4, C >= 256, C % 4 == 0."""
    _need(feat, "feat", torch.float32, ndim=3)
    _need(x3, "x3", torch.float32, ndim=3, last=3)
    B, S, C = feat.shape
    _need(wt, "wt", torch.float32, ndim=2, last=C)
    N = dist.shape[1]
    for t, name, dt in ((dist, "dist", torch.float32), (idx, "idx", torch.int64)):
        if not t.is_cuda or t.dtype != dt or t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != N * t.stride(1):
            raise RuntimeError(f"{name} must be a HIP {dt} (B,N,S') table with contiguous rows")
    if dist.stride(1) != idx.stride(1) or dist.shape[:2] != idx.shape[:2] or dist.shape[0] != B or x3.shape[:2] != dist.shape[:2] or wt.shape[0] != 3:
        raise RuntimeError("dist / idx / x3 / wt shapes do not match")
    out = torch.empty((B, N, C), dtype=torch.float32, device=feat.device)
    _call(feat.device, "upp_interp_affine_fwd", _abi.ptr(dist), _abi.ptr(idx), dist.stride(1), _abi.ptr(feat), _abi.ptr(x3), _abi.ptr(wt),
          _abi.ptr(out), B, N, S, C, int(k), float(eps))
    return out


def interp_bwd(dist, idx, g_out, S, k, eps):
    """Gradient of interp_fwd w.r.t. feat: g_out (B,N,C) -> (B,S,C); dist / idx as in interp_fwd."""
    _need(g_out, "g_out", torch.float32, ndim=3)
    B, N, C = g_out.shape
    for t, name, dt in ((dist, "dist", torch.float32), (idx, "idx", torch.int64)):
        if not t.is_cuda or t.dtype != dt or t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != N * t.stride(1):
            raise RuntimeError(f"{name} must be a HIP {dt} (B,N,S') table with contiguous rows")
    if dist.stride(1) != idx.stride(1) or dist.shape[:2] != idx.shape[:2] or tuple(dist.shape[:2]) != (B, N):
        raise RuntimeError("dist / idx must share shape and row stride and match g_out")
    g_feat = torch.empty((B, S, C), dtype=torch.float32, device=g_out.device)
    _call(g_out.device, "upp_interp_bwd", _abi.ptr(dist), _abi.ptr(idx), dist.stride(1), _abi.ptr(g_out), C, 0, _abi.ptr(g_feat),
          B, N, int(S), C, int(k), float(eps))
    return g_feat


def interp_geo_bwd(dist, idx, feat, g_out, xyz1, xyz2, k, eps, need1=True, need2=True):
    """Gradient of interp_fwd w.r.t. the geometry behind the neighbour table: -> (g_xyz1 (B,N,3) or None, g_xyz2 (B,S,3) or None);
    upp_interp_geo_bwd."""
    _need(g_out, "g_out", torch.float32, ndim=3)
    _need(feat, "feat", torch.float32, ndim=3)
    _need(xyz1, "xyz1", torch.float32, ndim=3, last=3)
    _need(xyz2, "xyz2", torch.float32, ndim=3, last=3)
    B, N, C = g_out.shape
    S = feat.shape[1]
    for t, name, dt in ((dist, "dist", torch.float32), (idx, "idx", torch.int64)):
        if not t.is_cuda or t.dtype != dt or t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != N * t.stride(1):
            raise RuntimeError(f"{name} must be a HIP {dt} (B,N,S') table with contiguous rows")
    if dist.stride(1) != idx.stride(1) or tuple(dist.shape[:2]) != (B, N) or tuple(xyz1.shape[:2]) != (B, N) or tuple(xyz2.shape[:2]) != (B, S) or feat.shape[2] != C:
        raise RuntimeError("interp_geo_bwd: shapes do not match")
    dev = g_out.device
    g1 = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if need1 else None
    g2 = torch.empty((B, S, 3), dtype=torch.float32, device=dev) if need2 else None
    contrib = torch.empty((B * N, int(k), 3), dtype=torch.float32, device=dev) if need2 else None
    _call(dev, "upp_interp_geo_bwd", _abi.ptr(dist), _abi.ptr(idx), dist.stride(1), _abi.ptr(feat), _abi.ptr(g_out), C, 0, _abi.ptr(xyz1), _abi.ptr(xyz2),
          B, N, S, C, int(k), float(eps), _abi.ptr(g1), _abi.ptr(g2), _abi.ptr(contrib))
    return g1, g2


def posenc_fwd(x, freqs, out=None, col0=0):
    _need(x, "x", torch.float32, last=3)
    F = len(freqs)
    rows = x.numel() // 3
    width = 3 * (2 * F + 1)
    if out is None:
        out = torch.empty(x.shape[:-1] + (width,), dtype=torch.float32, device=x.device)
    _need(out, "out", torch.float32)
    import ctypes
    arr = (ctypes.c_float * max(F, 1))(*[float(f) for f in freqs])
    _call(x.device, "upp_posenc_fwd", _abi.ptr(x), arr, F, _abi.ptr(out), out.shape[-1], int(col0), rows)
    return out


# ------------------------------------------------------------------ classification tail
def cls_pool_fwd(x, gamma, beta, eps):
    _need(x, "x", torch.float32, ndim=3)
    B, L, D = x.shape
    dev = x.device
    _need_f32(gamma, "gamma", (D,))
    _need_f32(beta, "beta", (D,))
    _same_device(x, gamma, beta)
    feat = torch.empty((B, 2 * D), dtype=torch.float32, device=dev)
    amax = torch.empty((B, D), dtype=torch.int32, device=dev)
    mean = torch.empty(B * L, dtype=torch.float32, device=dev)
    rstd = torch.empty(B * L, dtype=torch.float32, device=dev)
    _call(dev, "upp_cls_pool_fwd", _abi.ptr(x), _abi.ptr(gamma), _abi.ptr(beta), float(eps), _abi.ptr(feat), _abi.ptr(amax), _abi.ptr(mean),
          _abi.ptr(rstd), B, L, D)
    return feat, amax, mean, rstd


def cls_pool_bwd(g_feat, x, mean, rstd, gamma, amax):
    _need(x, "x", torch.float32, ndim=3)
    B, L, D = x.shape
    _need_f32(g_feat, "g_feat", (B, 2 * D))
    _need_f32(mean, "mean", (B * L,))
    _need_f32(rstd, "rstd", (B * L,))
    _need_f32(gamma, "gamma", (D,))
    _need(amax, "amax", torch.int32)
    if tuple(amax.shape) != (B, D):
        raise RuntimeError(f"cls_pool_bwd: amax must be ({B}, {D}), got {tuple(amax.shape)}")
    _same_device(x, g_feat, mean, rstd, gamma, amax)
    g_x = torch.empty_like(x)
    _call(x.device, "upp_cls_pool_bwd", _abi.ptr(g_feat), _abi.ptr(x), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(gamma), _abi.ptr(amax),
          _abi.ptr(g_x), B, L, D)
    return g_x


def cls_pool_bwd_ln(g_feat, x, mean, rstd, gamma, amax):
    """cls_pool_bwd with the LayerNorm's parameter gradients: -> (g_x, g_gamma (D), g_beta (D)); upp_cls_pool_bwd_ln."""
    _need(x, "x", torch.float32, ndim=3)
    B, L, D = x.shape
    _need_f32(g_feat, "g_feat", (B, 2 * D))
    _need_f32(mean, "mean", (B * L,))
    _need_f32(rstd, "rstd", (B * L,))
    _need_f32(gamma, "gamma", (D,))
    _need(amax, "amax", torch.int32)
    if tuple(amax.shape) != (B, D):
        raise RuntimeError(f"cls_pool_bwd_ln: amax must be ({B}, {D}), got {tuple(amax.shape)}")
    _same_device(x, g_feat, mean, rstd, gamma, amax)
    g_x = torch.empty_like(x)
    g_par = torch.empty((2, D), dtype=torch.float32, device=x.device)
    _call(x.device, "upp_cls_pool_bwd_ln", _abi.ptr(g_feat), _abi.ptr(x), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(gamma), _abi.ptr(amax),
          _abi.ptr(g_x), _abi.ptr(g_par[0]), _abi.ptr(g_par[1]), B, L, D)
    return g_x, g_par[0], g_par[1]


# ------------------------------------------------------------------ LayerNorm of three feature taps + token pooling (csrc/norm_pool.hip)
def tap_pool_fwd(f0, f1, f2, gamma, beta, eps):
    """-> x (B,G,3C) = [LN(f0) | LN(f1) | LN(f2)], gmax (B,3C), arg (B,3C) int32, gmean (B,3C), mean (B,G,3), rstd (B,G,3); upp_tap_pool_fwd."""
    _need(f0, "f0", torch.float32, ndim=3)
    B, G, C = f0.shape
    dev = f0.device
    _need_f32(f1, "f1", (B, G, C))
    _need_f32(f2, "f2", (B, G, C))
    _need_f32(gamma, "gamma", (C,))
    _need_f32(beta, "beta", (C,))
    _same_device(f0, f1, f2, gamma, beta)
    x = torch.empty((B, G, 3 * C), dtype=torch.float32, device=dev)
    gmax = torch.empty((B, 3 * C), dtype=torch.float32, device=dev)
    arg = torch.empty((B, 3 * C), dtype=torch.int32, device=dev)
    gmean = torch.empty((B, 3 * C), dtype=torch.float32, device=dev)
    mean = torch.empty((B, G, 3), dtype=torch.float32, device=dev)
    rstd = torch.empty((B, G, 3), dtype=torch.float32, device=dev)
    _call(dev, "upp_tap_pool_fwd", _abi.ptr(f0), _abi.ptr(f1), _abi.ptr(f2), _abi.ptr(gamma), _abi.ptr(beta), float(eps), _abi.ptr(x),
          _abi.ptr(gmax), _abi.ptr(arg), _abi.ptr(gmean), _abi.ptr(mean), _abi.ptr(rstd), B, G, C)
    return x, gmax, arg, gmean, mean, rstd


def tap_pool_bwd(d_x, d_gmax, d_gmean, f0, f1, f2, mean, rstd, gamma, arg):
    """-> (d_f0, d_f1, d_f2 (B,G,C), d_gamma (C), d_beta (C)); upp_tap_pool_bwd (two launches, fixed-order sums)."""
    _need(f0, "f0", torch.float32, ndim=3)
    B, G, C = f0.shape
    dev = f0.device
    _need_f32(f1, "f1", (B, G, C))
    _need_f32(f2, "f2", (B, G, C))
    _need_f32(d_x, "d_x", (B, G, 3 * C))
    _need_f32(d_gmax, "d_gmax", (B, 3 * C))
    _need_f32(d_gmean, "d_gmean", (B, 3 * C))
    _need_f32(mean, "mean", (B, G, 3))
    _need_f32(rstd, "rstd", (B, G, 3))
    _need_f32(gamma, "gamma", (C,))
    _need(arg, "arg", torch.int32)
    if tuple(arg.shape) != (B, 3 * C):
        raise RuntimeError(f"tap_pool_bwd: arg must be ({B}, {3 * C}), got {tuple(arg.shape)}")
    _same_device(f0, f1, f2, d_x, d_gmax, d_gmean, mean, rstd, gamma, arg)
    n = int(_abi.load().upp_tap_pool_part_floats(B, G, C))
    if n < 1:
        _abi.check(-2 if min(B, G, C) >= 1 else -1)
    part = torch.empty(n, dtype=torch.float32, device=dev)
    d_f = torch.empty((3, B, G, C), dtype=torch.float32, device=dev)
    d_par = torch.empty((2, C), dtype=torch.float32, device=dev)
    _call(dev, "upp_tap_pool_bwd", _abi.ptr(d_x), _abi.ptr(d_gmax), _abi.ptr(d_gmean), _abi.ptr(f0), _abi.ptr(f1), _abi.ptr(f2), _abi.ptr(mean),
          _abi.ptr(rstd), _abi.ptr(gamma), _abi.ptr(arg), _abi.ptr(part), _abi.ptr(d_f[0]), _abi.ptr(d_f[1]), _abi.ptr(d_f[2]),
          _abi.ptr(d_par[0]), _abi.ptr(d_par[1]), B, G, C)
    return d_f[0], d_f[1], d_f[2], d_par[0], d_par[1]


def ce_acc(logits, labels):
    _need(logits, "logits", torch.float32, ndim=2)
    _need(labels, "labels", torch.int64, ndim=1)
    B, C = logits.shape
    if labels.shape[0] != B:
        raise RuntimeError(f"ce_acc: labels must be ({B},), got {tuple(labels.shape)}")
    _same_device(logits, labels)
    out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    _call(logits.device, "upp_ce_acc", _abi.ptr(logits), _abi.ptr(labels), _abi.ptr(out2), _abi.ptr(dlogits), B, C)
    return out2, dlogits


def vote_points(superset, pick, scale=None, shift=None, out=None):
    """superset (B,S,3) f32, pick (V,N) int32 indices into [0,S), scale / shift (V,B,3) f32 or None -> (V*B, N, 3) vote-major:
    row v*B + b = superset[b, pick[v]] * scale[v,b] + shift[v,b] (upp_vote_points; bit-identical to misc.scale_translate's arithmetic)."""
    _need(superset, "superset", torch.float32, 3, 3)
    _need(pick, "pick", torch.int32, 2)
    B, S, _ = superset.shape
    V, N = pick.shape
    for t, name in ((scale, "scale"), (shift, "shift")):
        if t is not None:
            _need(t, name, torch.float32, 3, 3)
            if tuple(t.shape) != (V, B, 3):
                raise RuntimeError(f"{name} must be ({V}, {B}, 3), got {tuple(t.shape)}")
            _same_device(superset, t)
    _same_device(superset, pick)
    if out is None:
        out = torch.empty((V * B, N, 3), dtype=torch.float32, device=superset.device)
    else:
        _need(out, "out", torch.float32, 3, 3)
        if tuple(out.shape) != (V * B, N, 3):
            raise RuntimeError(f"out must be ({V * B}, {N}, 3), got {tuple(out.shape)}")
    _call(superset.device, "upp_vote_points", _abi.ptr(superset), _abi.ptr(pick), _abi.ptr(scale), _abi.ptr(shift), _abi.ptr(out),
          B, S, N, V)
    return out


def vote_reduce(logits, labels, votes, n_valid, pred, counters):
    """logits (votes*B, C) f32 vote-major, labels (B) int64 -> pred (B) int64 = first arg-max of the mean over the votes (written in
    place); counters (2) int64 += (correct rows among the first n_valid, n_valid) (upp_vote_reduce: one workgroup, no memset)."""
    _need(logits, "logits", torch.float32, 2)
    _need(labels, "labels", torch.int64, 1)
    _need(pred, "pred", torch.int64, 1)
    _need(counters, "counters", torch.int64, 1)
    _same_device(logits, labels, pred, counters)
    B, V = labels.shape[0], int(votes)
    if V < 1 or logits.shape[0] != V * B or pred.shape[0] != B or counters.shape[0] != 2:
        raise RuntimeError(f"vote_reduce: logits {tuple(logits.shape)}, labels ({B},), pred {tuple(pred.shape)}, counters "
                           f"{tuple(counters.shape)} do not fit {V} votes")
    _call(logits.device, "upp_vote_reduce", _abi.ptr(logits), _abi.ptr(labels), V, B, logits.shape[1], int(n_valid), _abi.ptr(pred),
          _abi.ptr(counters))
    return pred, counters


class SegAccumulator:
    """Device sums of a part-segmentation evaluation (upp_seg_iou_accumulate adds into them): counters (3) int64 = (correct points, seen
    points, invalid shapes), part_seen / part_correct (P) int64, cat_sum (C) f64 and cat_cnt (C) int64 = the shape IoUs per category and
    their count.  shape_iou (B) f64 / shape_cat (B) int32 hold the last update's shapes.  The int32 scratch of upp_seg_iou_counts is
    zeroed once here and re-zeroed by every accumulate launch, so an update issues kernel launches only."""

    def __init__(self, num_part, num_classes, device):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError("SegAccumulator lives on a HIP (cuda) device; upp_hip has no CPU path")
        self.P, self.C, self.device = int(num_part), int(num_classes), dev
        self.counters = torch.zeros(3, dtype=torch.int64, device=dev)
        self.part_seen = torch.zeros(self.P, dtype=torch.int64, device=dev)
        self.part_correct = torch.zeros(self.P, dtype=torch.int64, device=dev)
        self.cat_sum = torch.zeros(self.C, dtype=torch.float64, device=dev)
        self.cat_cnt = torch.zeros(self.C, dtype=torch.int64, device=dev)
        self.scratch = self.shape_iou = self.shape_cat = None
        self.batch = 0

    def zero_(self):
        for t in (self.counters, self.part_seen, self.part_correct, self.cat_sum, self.cat_cnt):
            t.zero_()
        return self

    def reserve(self, batch):
        """Room for updates of up to `batch` shapes (a larger batch reallocates the scratch, zeroed)."""
        if batch > self.batch:
            self.scratch = torch.zeros(3 * batch * self.P + 2 * self.P + 1, dtype=torch.int32, device=self.device)
            self.shape_iou = torch.empty(batch, dtype=torch.float64, device=self.device)
            self.shape_cat = torch.empty(batch, dtype=torch.int32, device=self.device)
            self.batch = batch
        return self


def seg_iou_update(logp, target, part_cat, cat_range, acc, n_valid=None, pred=None):
    """The part-segmentation metrics of shapes [0, n_valid) of one batch, added into `acc` (a SegAccumulator) in two launches
    (upp_seg_iou_counts, upp_seg_iou_accumulate).  logp (B, N, P) f32 whose rows may be strided (stride(1) >= P, a view of a padded head
    output), target (B, N) int64, part_cat (P) int32, cat_range (C, 2) int32.  pred: None or (B, N) int64, written with the in-category
    arg-max of every row (padding rows included).  -> acc.shape_iou[:n_valid] (the IoU of each shape, f64)."""
    if not isinstance(logp, torch.Tensor) or not logp.is_cuda:
        raise RuntimeError("logp must be a HIP (cuda) tensor; upp_hip has no CPU path")
    if logp.dtype != torch.float32 or logp.dim() != 3:
        raise RuntimeError(f"logp must be a 3-D float32 tensor, got {logp.dtype} {tuple(logp.shape)}")
    B, N, P = logp.shape
    ld = logp.stride(1)
    if logp.stride(2) != 1 or ld < P or logp.stride(0) != N * ld:
        raise RuntimeError(f"logp rows must be unit-stride with a common row stride >= {P}, got strides {logp.stride()}")
    _need(target, "target", torch.int64, 2)
    _need(part_cat, "part_cat", torch.int32, 1)
    _need(cat_range, "cat_range", torch.int32, 2, 2)
    if not isinstance(acc, SegAccumulator):
        raise TypeError("acc must be a SegAccumulator")
    _same_device(logp, target, part_cat, cat_range, acc.counters)
    C = cat_range.shape[0]
    if tuple(target.shape) != (B, N):
        raise RuntimeError(f"target must be ({B}, {N}), got {tuple(target.shape)}")
    if part_cat.shape[0] != P or acc.P != P or acc.C != C:
        raise RuntimeError(f"seg_iou_update: logp has {P} parts; the table ({part_cat.shape[0]} parts, {C} categories) and the "
                           f"accumulator ({acc.P}, {acc.C}) must agree")
    if pred is not None:
        _need(pred, "pred", torch.int64, 2)
        _same_device(logp, pred)
        if tuple(pred.shape) != (B, N):
            raise RuntimeError(f"pred must be ({B}, {N}), got {tuple(pred.shape)}")
    n_valid = B if n_valid is None else int(n_valid)
    if not 0 <= n_valid <= B:
        raise RuntimeError(f"n_valid {n_valid} outside [0, {B}]")
    acc.reserve(B)
    _call(logp.device, "upp_seg_iou_counts", _abi.ptr(logp), ld, _abi.ptr(target), _abi.ptr(part_cat), _abi.ptr(cat_range), B, N, P, C,
          n_valid, _abi.ptr(pred), _abi.ptr(acc.scratch))
    _call(logp.device, "upp_seg_iou_accumulate", _abi.ptr(acc.scratch), _abi.ptr(target), _abi.ptr(part_cat), _abi.ptr(cat_range), B,
          N, P, C, n_valid, _abi.ptr(acc.shape_iou), _abi.ptr(acc.shape_cat), _abi.ptr(acc.cat_sum), _abi.ptr(acc.cat_cnt),
          _abi.ptr(acc.part_seen), _abi.ptr(acc.part_correct), _abi.ptr(acc.counters))
    return acc.shape_iou[:n_valid]


class CompletionAccumulator:
    """Device sums of a point-completion evaluation (upp_completion_accumulate adds into them): loss_sum (4) f64 = 1000 x the sparse
    CD-L1, sparse CD-L2, dense CD-L1, dense CD-L2 summed over (cloud, viewpoint) pairs; counters (2) int64 = (pairs, pairs of a cloud
    whose category is outside [0, C)); cat_sum (C, 3) f64 = per category the sums of F-Score, 1000 CDL1 and 1000 CDL2, cat_cnt (C) int64
    their count.  The per-(cloud, viewpoint) rows of the last update -- sparse / dense (R, 8) f64 and sparse_counts / dense_counts (R, 4)
    int32, include/upp_hip.h upp_completion_cloud_metrics -- are reserved per row count; every launch writes them whole, so an update
    issues kernel launches only (no memset)."""

    def __init__(self, num_categories, device):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError("CompletionAccumulator lives on a HIP (cuda) device; upp_hip has no CPU path")
        self.C, self.device = int(num_categories), dev
        if self.C < 1:
            raise ValueError("num_categories must be positive")
        self.loss_sum = torch.zeros(4, dtype=torch.float64, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)
        self.cat_sum = torch.zeros((self.C, 3), dtype=torch.float64, device=dev)
        self.cat_cnt = torch.zeros(self.C, dtype=torch.int64, device=dev)
        self.sparse = self.dense = self.sparse_counts = self.dense_counts = None
        self.rows = 0

    def zero_(self):
        for t in (self.loss_sum, self.counters, self.cat_sum, self.cat_cnt):
            t.zero_()
        return self

    def reserve(self, rows):
        """Room for updates of up to `rows` (cloud, viewpoint) pairs (a larger count reallocates)."""
        if rows > self.rows:
            dev = self.device
            self.sparse = torch.empty((rows, 8), dtype=torch.float64, device=dev)
            self.dense = torch.empty((rows, 8), dtype=torch.float64, device=dev)
            self.sparse_counts = torch.empty((rows, 4), dtype=torch.int32, device=dev)
            self.dense_counts = torch.empty((rows, 4), dtype=torch.int32, device=dev)
            self.rows = rows
        return self


def _completion_inputs(coarse, dense, gt, acc):
    _need(coarse, "coarse", torch.float32, 3, 3)
    _need(dense, "dense", torch.float32, 3, 3)
    _need(gt, "gt", torch.float32, 3, 3)
    if not isinstance(acc, CompletionAccumulator):
        raise TypeError("acc must be a CompletionAccumulator")
    _same_device(coarse, dense, gt, acc.loss_sum)
    R, B = coarse.shape[0], gt.shape[0]
    if dense.shape[0] != R or B < 1 or R < B or R % B:
        raise RuntimeError(f"coarse {tuple(coarse.shape)} and dense {tuple(dense.shape)} must hold V x {B} clouds, viewpoint-major, "
                           f"for gt {tuple(gt.shape)}")
    if min(coarse.shape[1], dense.shape[1], gt.shape[1]) < 1:
        raise RuntimeError("every cloud needs at least one point")
    return R, B, R // B


def completion_cloud_metrics(coarse, dense, gt, acc, detail, th=0.01):
    """The per-(cloud, viewpoint) rows of one viewpoint-expanded batch, all on the device: coarse (V B, nc, 3) and dense (V B, nd, 3) f32
    against gt (B, N, 3), row v B + b against gt[b].  upp_chamfer_fwd on both pairs, upp_completion_cloud_metrics on each (F-Score and
    the zero-sum flag on the dense pair when `detail`), then upp_completion_masked_cd (its workgroups return at once unless a pair holds
    a zero-sum point).  -> (V, B); the rows are acc.sparse / acc.dense[:V B]."""
    R, B, V = _completion_inputs(coarse, dense, gt, acc)
    th = float(th)
    if not (th > 0.0 and th != float('inf')):
        raise RuntimeError(f"th must be positive and finite, got {th}")
    target = gt if V == 1 else gt.repeat(V, 1, 1)
    acc.reserve(R)
    dev = gt.device
    for pts, stats, counts, det in ((coarse, acc.sparse, acc.sparse_counts, 0), (dense, acc.dense, acc.dense_counts, int(bool(detail)))):
        d1, d2, i1, i2 = chamfer_fwd(pts, target)
        n, m = pts.shape[1], target.shape[1]
        _call(dev, "upp_completion_cloud_metrics", _abi.ptr(pts), _abi.ptr(target), _abi.ptr(d1), _abi.ptr(i1), _abi.ptr(d2), _abi.ptr(i2),
              R, n, m, th, det, _abi.ptr(stats), _abi.ptr(counts))
        if det:
            _call(dev, "upp_completion_masked_cd", _abi.ptr(pts), _abi.ptr(target), R, n, m, _abi.ptr(counts), _abi.ptr(stats))
    return V, B


def completion_accumulate(acc, V, B, category=None, n_valid=None, rows=None):
    """Add the rows of clouds [0, n_valid) of the last completion_cloud_metrics(V B rows) into acc, in the reference's order (cloud, then
    viewpoint).  category: None (losses only) or (B,) int64 on acc's device, the detail metrics then go to its categories.  rows: the
    CompletionAccumulator whose sparse / dense rows are read (default acc; a captured step keeps its own)."""
    rows = acc if rows is None else rows
    if not isinstance(acc, CompletionAccumulator) or not isinstance(rows, CompletionAccumulator):
        raise TypeError("acc and rows must be CompletionAccumulators")
    V, B = int(V), int(B)
    if V < 1 or B < 1 or V * B > rows.rows:
        raise RuntimeError(f"{V} x {B} rows: not what the accumulator holds ({rows.rows} reserved)")
    _same_device(acc.loss_sum, rows.loss_sum)
    n_valid = B if n_valid is None else int(n_valid)
    if not 0 <= n_valid <= B:
        raise RuntimeError(f"n_valid {n_valid} outside [0, {B}]")
    if category is not None:
        _need(category, "category", torch.int64, 1)
        _same_device(category, acc.loss_sum)
        if category.shape[0] != B:
            raise RuntimeError(f"category must be ({B},), got {tuple(category.shape)}")
    _call(acc.device, "upp_completion_accumulate", _abi.ptr(rows.sparse), _abi.ptr(rows.dense), _abi.ptr(category), V, B, acc.C, n_valid,
          _abi.ptr(acc.loss_sum), _abi.ptr(acc.counters), _abi.ptr(acc.cat_sum), _abi.ptr(acc.cat_cnt))
    return acc


def completion_update(coarse, dense, gt, acc, category=None, n_valid=None, th=0.01):
    """One viewpoint-expanded batch into acc (a CompletionAccumulator): completion_cloud_metrics (detail = a category is given), then
    completion_accumulate over clouds [0, n_valid).  Every tensor is checked (f32 contiguous (.., .., 3) clouds on one device, int64
    categories) before the first launch.  -> acc."""
    R, B, V = _completion_inputs(coarse, dense, gt, acc)
    n_valid = B if n_valid is None else int(n_valid)
    if not 0 <= n_valid <= B:
        raise RuntimeError(f"n_valid {n_valid} outside [0, {B}]")
    if category is not None:
        _need(category, "category", torch.int64, 1)
        _same_device(category, gt)
        if category.shape[0] != B:
            raise RuntimeError(f"category must be ({B},), got {tuple(category.shape)}")
    completion_cloud_metrics(coarse, dense, gt, acc, category is not None, th)
    return completion_accumulate(acc, V, B, category, n_valid)


def bn_relu_drop_fwd(z, gamma, beta, running_mean, running_var, momentum, eps, training, u, p):
    _need(z, "z", torch.float32, ndim=2)
    R, C = z.shape
    _bn_params(z, gamma, beta, running_mean, running_var, training, affine_optional=False)
    _need_f32(u, "u", (R, C), optional=True)
    if u is not None:
        _same_device(z, u)
    a = torch.empty_like(z)
    mean = torch.empty(C, dtype=torch.float32, device=z.device)
    rstd = torch.empty(C, dtype=torch.float32, device=z.device)
    _call(z.device, "upp_bn_relu_drop_fwd", _abi.ptr(z), _abi.ptr(gamma), _abi.ptr(beta), _abi.ptr(running_mean), _abi.ptr(running_var),
          float(momentum), float(eps), int(bool(training)), _abi.ptr(u), float(p), _abi.ptr(a), _abi.ptr(mean), _abi.ptr(rstd), R, C)
    return a, mean, rstd


def bn_relu_drop_bwd(g_a, z, gamma, beta, mean, rstd, training, u, p):
    _need(z, "z", torch.float32, ndim=2)
    R, C = z.shape
    _need_f32(g_a, "g_a", (R, C))
    _need_f32(u, "u", (R, C), optional=True)
    for t, name in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (rstd, "rstd")):
        _need_f32(t, name, (C,))
    _same_device(z, g_a, gamma, beta, mean, rstd, *(() if u is None else (u,)))
    g_z = torch.empty_like(z)
    g_gamma = torch.empty(C, dtype=torch.float32, device=z.device)
    g_beta = torch.empty(C, dtype=torch.float32, device=z.device)
    _call(z.device, "upp_bn_relu_drop_bwd", _abi.ptr(g_a), _abi.ptr(z), _abi.ptr(gamma), _abi.ptr(beta), _abi.ptr(mean), _abi.ptr(rstd),
          int(bool(training)), _abi.ptr(u), float(p), _abi.ptr(g_z), _abi.ptr(g_gamma), _abi.ptr(g_beta), R, C)
    return g_z, g_gamma, g_beta


# ------------------------------------------------------------------ optimizer tail
def batched_sum(jobs):
    """jobs: list of (part 2-D f32, column offset, rows n, length, row stride, dst f32, accumulate):
    dst (+)= sum over the n rows of part[:, offset:offset+length], every job in one launch (upp_batched_sum).  dst: `length` contiguous
    elements, or a 2-D WINDOW (rows, w) with rows * w == length, unit column stride and any row pitch (a column range of a wider matrix)."""
    if not jobs:
        return
    import ctypes
    k = len(jobs)
    dw, dp = [], []
    for part, off, n, length, ld, dst, acc in jobs:
        if not (isinstance(dst, torch.Tensor) and dst.is_cuda and dst.dtype == torch.float32):
            raise RuntimeError("batched_sum: dst must be an f32 HIP (cuda) tensor; upp_hip has no CPU path")
        if not part.is_cuda or part.dtype != torch.float32 or part.dim() != 2 or part.stride(1) != 1 or part.stride(0) != ld:
            raise RuntimeError("batched_sum: part must be a HIP f32 matrix with contiguous rows")
        if n != part.shape[0] or off < 0 or off + length > part.shape[1] or dst.numel() != length:
            raise RuntimeError("batched_sum: job geometry does not match its tensors")
        if dst.is_contiguous():
            dw.append(0), dp.append(0)
        elif dst.dim() == 2 and dst.stride(1) == 1 and dst.stride(0) >= dst.shape[1]:
            dw.append(dst.shape[1]), dp.append(dst.stride(0))
        else:
            raise RuntimeError("batched_sum: dst must be contiguous or a 2-D window with contiguous rows")
    src = (ctypes.c_void_p * k)(*[j[0].data_ptr() + 4 * j[1] for j in jobs])
    dst = (ctypes.c_void_p * k)(*[j[5].data_ptr() for j in jobs])
    n = (ctypes.c_int * k)(*[j[2] for j in jobs])
    ln = (ctypes.c_int * k)(*[j[3] for j in jobs])
    ld = (ctypes.c_int * k)(*[j[4] for j in jobs])
    acc = (ctypes.c_int * k)(*[int(bool(j[6])) for j in jobs])
    windows = any(dw)
    _call(jobs[0][0].device, "upp_batched_sum", src, dst, n, ln, ld, acc, (ctypes.c_int * k)(*dw) if windows else None,
          (ctypes.c_int * k)(*dp) if windows else None, k)


def copy_batched(dsts, srcs):
    """dst_j.copy_(src_j) for contiguous same-shape / same-dtype HIP tensors, every pair in one launch (upp_copy_batched)."""
    if not dsts:
        return
    import ctypes
    k = len(dsts)
    if len(srcs) != k:
        raise RuntimeError("copy_batched: as many sources as destinations")
    for d, s_ in zip(dsts, srcs):
        if not (d.is_cuda and s_.is_cuda and d.dtype == s_.dtype and d.shape == s_.shape and d.is_contiguous() and s_.is_contiguous()):
            raise RuntimeError("copy_batched: contiguous HIP (cuda) tensors of equal shape and dtype are required")
    pairs = [(d, s_) for d, s_ in zip(dsts, srcs) if d.numel() > 0]        # an empty tensor's data_ptr() is NULL, which the library refuses
    if not pairs:
        return
    dsts, srcs, k = [d for d, _ in pairs], [s_ for _, s_ in pairs], len(pairs)
    S =(ctypes.c_void_p * k)(*[t.data_ptr() for t in srcs])
    D = (ctypes.c_void_p * k)(*[t.data_ptr() for t in dsts])
    n = (ctypes.c_longlong * k)(*[t.numel() * t.element_size() for t in dsts])
    _call(dsts[0].device, "upp_copy_batched", S, D, n, k)


def transpose_batched(pairs):
    """pairs: list of (src (rows, cols) contiguous f32, dst (cols, rows) contiguous f32): dst = src^T for all of them in one launch
    (upp_transpose_batched_f32)."""
    if not pairs:
        return
    import ctypes
    k = len(pairs)
    for src, dst in pairs:
        _need(src, "src", torch.float32, ndim=2)
        _need(dst, "dst", torch.float32, ndim=2)
        if tuple(dst.shape) != (src.shape[1], src.shape[0]):
            raise RuntimeError("transpose_batched: dst must be (cols, rows) of src")
    srcs = (ctypes.c_void_p * k)(*[a.data_ptr() for a, _ in pairs])
    dsts = (ctypes.c_void_p * k)(*[b.data_ptr() for _, b in pairs])
    rows = (ctypes.c_int * k)(*[a.shape[0] for a, _ in pairs])
    cols = (ctypes.c_int * k)(*[a.shape[1] for a, _ in pairs])
    _call(pairs[0][0].device, "upp_transpose_batched_f32", srcs, dsts, rows, cols, k)


def adamw_flat(p, g, m, v, n, split, state, scratch, lr, beta1, beta2, eps, weight_decay, max_norm):
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (state, "state"), (scratch, "scratch")):
        _need(t, name, torch.float32)
    _call(p.device, "upp_adamw_flat", _abi.ptr(p), _abi.ptr(g), _abi.ptr(m), _abi.ptr(v), int(n), int(split), _abi.ptr(state),
          _abi.ptr(scratch), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), float(max_norm))


# ------------------------------------------------------------------ bottleneck adapter
def _adapter_args(who, rows, W1, W2, u, s1=None, **row_tensors):
    """The operands every adapter entry point shares: row tensors (..., D) of ONE shape, W1 (H, D), W2 (D, H), the optional dropout
    uniforms (R, H) and the saved s1 (R, H).  -> (R, D, H)"""
    _need(rows, who + ": rows", torch.float32)
    if rows.dim() not in (2, 3):
        raise RuntimeError(f"{who}: row tensors must be (R, D) or (B, L, D), got {tuple(rows.shape)}")
    D = rows.shape[-1]
    R = rows.numel() // D
    _need(W1, "W1", torch.float32, ndim=2, last=D)
    H = W1.shape[0]
    _need_f32(W2, "W2", (D, H))
    for name, t in row_tensors.items():
        _need_f32(t, name, rows.shape)
    _need_f32(u, "dropout uniforms", (R, H), optional=True)
    _need_f32(s1, "s1", (R, H), optional=True)
    _same_device(*[t for t in (rows, W1, W2, u, s1) + tuple(row_tensors.values()) if t is not None])
    return R, D, H


def adapter_fwd(ha, x, W1, b1, W2, b2, u, p, scale):
    R, D, H = _adapter_args("adapter_fwd", ha, W1, W2, u, ha=ha, x=x)
    _need_f32(b1, "b1", (H,))
    _need_f32(b2, "b2", (D,))
    _same_device(ha, b1, b2)
    out = torch.empty_like(x)
    s1 = torch.empty((R, H), dtype=torch.float32, device=ha.device)
    _call(ha.device, "upp_adapter_fwd", _abi.ptr(ha), _abi.ptr(x), _abi.ptr(W1), _abi.ptr(b1), _abi.ptr(W2), _abi.ptr(b2), _abi.ptr(u),
          float(p), float(scale), _abi.ptr(out), _abi.ptr(s1), R, D, H)
    return out, s1


def ln_adapter_fwd(x, y, ybias, u, keep, mode, P, gamma, beta, eps, W1, b1, W2, b2, ud, p, scale, Lout):
    """Residual + prompt strip + adapter LayerNorm + adapter in one launch -> (out, xo, mean, rstd, s1); upp_ln_adapter_fwd."""
    _need(x, "x", torch.float32, ndim=3)
    B, Lin, D = x.shape
    H = W1.shape[0]
    dev = x.device
    for t_, n_, shp in ((gamma, "gamma", (D,)), (beta, "beta", (D,)), (W1, "W1", (H, D)), (b1, "b1", (H,)), (W2, "W2", (D, H)), (b2, "b2", (D,))):
        _need(t_, n_, torch.float32)
        if tuple(t_.shape) != shp:
            raise RuntimeError(f"ln_adapter_fwd: {n_} must be {shp}, got {tuple(t_.shape)}")
    _need_f32(y, "y", (B, Lin, D), optional=True)
    _need_f32(ybias, "ybias", (D,), optional=True)
    _need_f32(u, "u", (B,), optional=True)
    _need_f32(ud, "ud", (B * Lout, H), optional=True)
    _same_device(*[t for t in (x, y, ybias, u, gamma, beta, W1, b1, W2, b2, ud) if t is not None])
    xo = torch.empty((B, Lout, D), dtype=torch.float32, device=dev)
    out = torch.empty((B, Lout, D), dtype=torch.float32, device=dev)
    mean = torch.empty((B, Lout), dtype=torch.float32, device=dev)
    rstd = torch.empty((B, Lout), dtype=torch.float32, device=dev)
    s1 = torch.empty((B * Lout, H), dtype=torch.float32, device=dev)
    _call(dev, "upp_ln_adapter_fwd", _abi.ptr(x), _abi.ptr(y), _abi.ptr(ybias), _abi.ptr(u), float(keep), int(mode), int(P), _abi.ptr(gamma),
          _abi.ptr(beta), float(eps), _abi.ptr(W1), _abi.ptr(b1), _abi.ptr(W2), _abi.ptr(b2), _abi.ptr(ud), float(p), float(scale),
          _abi.ptr(xo), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(s1), _abi.ptr(out), B, Lin, Lout, D, H)
    return out, xo, mean, rstd, s1


def ln_adapter_prop_fwd(x2, m, mbias, u_dp, keep_dp, mode, P, pooled, bn_mean, bn_rstd, bn_gamma, bn_beta, i2, idx8, w8, gamma, beta, eps,
                        W1, b1, W2, b2, ud, p, scale, Lout):
    """ln_adapter_fwd of a prompted block with the propagation step's interpolation (and the MLP residual under it) as its row phase
    -> (out, xo, mean, rstd, s1); upp_ln_adapter_prop_fwd.  pooled, bn_mean, bn_rstd: what prop_res_pool_fwd wrote."""
    _need(x2, "x2", torch.float32, ndim=3)
    B, Lin, D = x2.shape
    H = W1.shape[0]
    dev = x2.device
    _prop_args(B, Lin, D, (("x2", x2), ("m", m)), mbias=mbias, u_dp=u_dp)
    for t_, n_, shp in ((gamma, "gamma", (D,)), (beta, "beta", (D,)), (W1, "W1", (H, D)), (b1, "b1", (H,)), (W2, "W2", (D, H)), (b2, "b2", (D,)),
                        (bn_mean, "bn_mean", (D,)), (bn_rstd, "bn_rstd", (D,)), (bn_gamma, "bn_gamma", (D,)), (bn_beta, "bn_beta", (D,))):
        _need_f32(t_, n_, shp)
    _need(idx8, "idx8", torch.int32, ndim=3, last=8)
    _need(i2, "i2", torch.int32)
    T = idx8.shape[1]
    if idx8.shape[0] != B or i2.numel() % B != 0:
        raise RuntimeError("ln_adapter_prop_fwd: idx8 must be (B, T, 8) and i2 (B * G2)")
    G2 = i2.numel() // B
    _need_f32(w8, "w8", (B, T, 8))
    _need_f32(pooled, "pooled", (B * G2, D))
    _need_f32(ud, "ud", (B * Lout, H), optional=True)
    _same_device(*[t for t in (x2, pooled, bn_mean, bn_rstd, bn_gamma, bn_beta, i2, idx8, w8, gamma, beta, W1, b1, W2, b2, ud) if t is not None])
    xo = torch.empty((B, Lout, D), dtype=torch.float32, device=dev)
    out = torch.empty((B, Lout, D), dtype=torch.float32, device=dev)
    mean = torch.empty((B, Lout), dtype=torch.float32, device=dev)
    rstd = torch.empty((B, Lout), dtype=torch.float32, device=dev)
    s1 = torch.empty((B * Lout, H), dtype=torch.float32, device=dev)
    _call(dev, "upp_ln_adapter_prop_fwd", _abi.ptr(x2), _abi.ptr(m), _abi.ptr(mbias), _abi.ptr(u_dp), float(keep_dp), int(mode), int(P),
          _abi.ptr(pooled), _abi.ptr(bn_mean), _abi.ptr(bn_rstd), _abi.ptr(bn_gamma), _abi.ptr(bn_beta), _abi.ptr(i2), _abi.ptr(idx8), _abi.ptr(w8),
          T, G2, _abi.ptr(gamma), _abi.ptr(beta), float(eps), _abi.ptr(W1), _abi.ptr(b1), _abi.ptr(W2), _abi.ptr(b2), _abi.ptr(ud), float(p),
          float(scale), _abi.ptr(xo), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(s1), _abi.ptr(out), B, Lin, Lout, D, H)
    return out, xo, mean, rstd, s1


def ln_adapter_bwd(g_out, xo, mean, rstd, gamma, beta, s1, W1, W2, u, p, scale):
    """upp_adapter_bwd with the LayerNorm output rebuilt from the saved rows and statistics -> (g_ha, partials)."""
    R, D, H = _adapter_args("ln_adapter_bwd", xo, W1, W2, u, s1=s1, xo=xo, g_out=g_out)
    _need_f32(mean, "mean", xo.shape[:-1])
    _need_f32(rstd, "rstd", xo.shape[:-1])
    _need_f32(gamma, "gamma", (D,))
    _need_f32(beta, "beta", (D,))
    _same_device(xo, mean, rstd, gamma, beta)
    g_ha = torch.empty_like(xo)
    n = int(_abi.load().upp_adapter_part_floats(R, D))
    nblk = (R + 31) // 32
    part = torch.empty((nblk, n // nblk), dtype=torch.float32, device=xo.device)
    _call(xo.device, "upp_ln_adapter_bwd", _abi.ptr(g_out), _abi.ptr(xo), _abi.ptr(mean), _abi.ptr(rstd), _abi.ptr(gamma), _abi.ptr(beta),
          _abi.ptr(s1), _abi.ptr(W1), _abi.ptr(W2), _abi.ptr(u), float(p), float(scale), _abi.ptr(g_ha), _abi.ptr(part), R, D, H)
    return g_ha, part


def ln_adapter_bwd_fused(g_out, xo, mean, rstd, gamma, beta, s1, W1, W2, ud, p, scale, u, keep, mode, P, Lin, need_x, need_y, need_adapter,
                         need_ln, factors=False):
    """Backward of ln_adapter_fwd in one launch -> (g_x, g_y, adapter partials, LayerNorm partials); upp_ln_adapter_bwd_fused.
    factors=True: the third result is `fac` (B*Lout, 2 H) = [ga | d] per row instead of the per-workgroup partial matrices
    (upp_ln_adapter_bwd_factors; the weight gradients are then formed by adapter_wgrad_batched)."""
    _need(xo, "xo", torch.float32, ndim=3)
    B, Lout, D = xo.shape
    R, D, H = _adapter_args("ln_adapter_bwd_fused", xo, W1, W2, ud, s1=s1, xo=xo, g_out=g_out)
    _need_f32(mean, "mean", (B, Lout))
    _need_f32(rstd, "rstd", (B, Lout))
    _need_f32(gamma, "gamma", (D,))
    _need_f32(beta, "beta", (D,))
    _need_f32(u, "u", (B,), optional=True)
    _same_device(*[t for t in (xo, mean, rstd, gamma, beta, u) if t is not None])
    dev = xo.device
    nwg = (R + 15) // 16
    g_x = torch.empty((B, Lin, D), dtype=torch.float32, device=dev) if need_x else None
    g_y = torch.empty((B, Lin, D), dtype=torch.float32, device=dev) if need_y else None
    ln_part = torch.empty((nwg, 2 * D), dtype=torch.float32, device=dev) if need_ln else None
    if factors:
        part = torch.empty((R, 2 * H), dtype=torch.float32, device=dev)
    else:
        part = torch.empty((nwg, int(_abi.load().upp_ln_adapter_part_floats(R, D)) // nwg), dtype=torch.float32, device=dev) if need_adapter else None
    _call(dev, "upp_ln_adapter_bwd_factors" if factors else "upp_ln_adapter_bwd_fused", _abi.ptr(g_out), _abi.ptr(xo), _abi.ptr(mean), _abi.ptr(rstd),
          _abi.ptr(gamma), _abi.ptr(beta), _abi.ptr(s1), _abi.ptr(W1), _abi.ptr(W2), _abi.ptr(ud), float(p), float(scale), _abi.ptr(u), float(keep),
          int(mode), int(P), _abi.ptr(g_x), _abi.ptr(g_y), _abi.ptr(part), _abi.ptr(ln_part), B, Lin, Lout, D, H)
    return g_x, g_y, part, ln_part


def adapter_wgrad_batched(jobs, H=32):
    """jobs: list of (xo (R, D), mean (R), rstd (R), gamma, beta, g_out (R, D), fac (R, 2 H), scale) -- the saved rows and statistics of a
    block's tail, the gradient that reached it and the factors ln_adapter_bwd_fused(factors=True) wrote.  ONE launch (per 16 jobs) forms
    every block's [dW1 | dW2 | db1 | db2] over `splits` row ranges -> list of (splits, 2 H D + H + D) partial matrices, to be summed over
    their rows (batched_sum); upp_adapter_wgrad_batched."""
    if not jobs:
        return []
    import ctypes
    k = len(jobs)
    lib = _abi.load()
    D = jobs[0][0].shape[-1]
    for xo, mean, rstd, gamma, beta, g_out, fac, _ in jobs:
        R = xo.numel() // D
        for t, name, n in ((xo, "xo", R * D), (g_out, "g_out", R * D), (mean, "mean", R), (rstd, "rstd", R), (gamma, "gamma", D), (beta, "beta", D),
                           (fac, "fac", R * 2 * H)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
                raise RuntimeError("adapter_wgrad_batched: %s must be a contiguous f32 HIP tensor of %d elements" % (name, n))
    rows = [j[0].numel() // D for j in jobs]
    splits = int(lib.upp_adapter_wgrad_splits(max(rows)))
    psz = 2 * H * D + H + D
    parts = [torch.empty((splits, psz), dtype=torch.float32, device=jobs[0][0].device) for _ in jobs]
    arr = lambda i: (ctypes.c_void_p * k)(*[j[i].data_ptr() for j in jobs])
    _call(jobs[0][0].device, "upp_adapter_wgrad_batched", arr(0), arr(1), arr(2), arr(3), arr(4), arr(5), arr(6), (ctypes.c_int * k)(*rows),
          (ctypes.c_float * k)(*[float(j[7]) for j in jobs]), (ctypes.c_void_p * k)(*[p_.data_ptr() for p_ in parts]), k, splits, D, H)
    return parts


def adapter_bwd(g_out, ha, s1, W1, W2, u, p, scale):
    R, D, H = _adapter_args("adapter_bwd", ha, W1, W2, u, s1=s1, ha=ha, g_out=g_out)
    g_ha = torch.empty_like(ha)
    n = int(_abi.load().upp_adapter_part_floats(R, D))
    nblk = (R + 31) // 32
    part = torch.empty((nblk, n // nblk), dtype=torch.float32, device=ha.device)
    _call(ha.device, "upp_adapter_bwd", _abi.ptr(g_out), _abi.ptr(ha), _abi.ptr(s1), _abi.ptr(W1), _abi.ptr(W2), _abi.ptr(u),
          float(p), float(scale), _abi.ptr(g_ha), _abi.ptr(part), R, D, H)
    return g_ha, part
