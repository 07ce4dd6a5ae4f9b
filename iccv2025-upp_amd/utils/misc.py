"""Hot-path helpers of the reference's utils/misc.py."""
import torch

from upp_hip import functional as _F


def fps(data, number):
    """data (B,N,3), number -> (fps_data (B,number,3), fps_idx (B,number) int32).

    Reference utils/misc.py:13-20 runs furthest_point_sample, then gather_operation on a
    transposed copy and transposes back; here the sampled coordinates come out of the FPS
    kernel itself (same values: a gather is an exact copy)."""
    fps_data, fps_idx = _F.fps_gather(data.contiguous(), number)
    from models import upp_layers as L
    if L.POOL_TRACE is not None:          # (test instrument, see upp_layers.trace_idx)
        fps_idx = L.trace_idx('misc.fps', fps_idx)
        fps_data = L.index_points(data, fps_idx.long())
    return fps_data, fps_idx


def fps_ragged(clouds_or_packed, lengths, number, normalize=False):
    """FPS of a batch of clouds of DIFFERENT lengths in one launch -> (points (B,number,3) f32, idx (B,number) int32, local to each cloud):
    cloud b's rows are those of fps(cloud_b[None], number).

    clouds_or_packed: a sequence of (n_i,3) tensors on one device (lengths may be None), or one packed (T,3) tensor holding the clouds
    back to back with `lengths` a host sequence / CPU tensor of the B lengths (a data loader knows them: offsets and the longest length
    are derived on the host, nothing is read back from the device).  normalize=True first applies the reference's pc_norm
    (datasets/RealSensorDataset.py:59-65: p / (2 max |p|), float64 arithmetic) to every cloud -- float64 or float32 input; without it the
    input must be float32.  Two launches at the most, no per-cloud loop, no padding (padded zeros would change the tie order)."""
    from upp_hip import ops
    if isinstance(clouds_or_packed, (list, tuple)):
        for c in clouds_or_packed:
            if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 3:
                raise ValueError("fps_ragged: every cloud must be a (n, 3) tensor")
        if lengths is None:
            lengths = [c.shape[0] for c in clouds_or_packed]
        elif [int(n) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)] != [c.shape[0] for c in clouds_or_packed]:
            raise ValueError("fps_ragged: lengths do not match the clouds")
        if any(c.shape[0] < 1 for c in clouds_or_packed):
            raise ValueError("ragged batch: cloud %d is empty (every cloud needs at least one point)" % [c.shape[0] < 1 for c in clouds_or_packed].index(True))
        packed = torch.cat(list(clouds_or_packed)) if clouds_or_packed else torch.empty(0, 3)
    else:
        packed = clouds_or_packed
    if not isinstance(packed, torch.Tensor) or packed.dim() != 2 or packed.shape[1] != 3:
        raise ValueError("fps_ragged: a packed (T, 3) tensor or a sequence of (n, 3) tensors is required")
    if packed.dtype not in ((torch.float64, torch.float32) if normalize else (torch.float32,)):
        raise RuntimeError("fps_ragged: the points must be %s, got %s" % ("float64 or float32" if normalize else "float32", packed.dtype))
    if not packed.is_contiguous():
        raise RuntimeError("fps_ragged: the packed points must be contiguous")
    if lengths is None:
        raise ValueError("fps_ragged: a packed tensor needs the lengths of its clouds")
    offsets, max_len = ops.ragged_layout(lengths, packed.shape[0])
    if packed.is_cuda:
        offsets = offsets.to(packed.device, non_blocking=True)
    if normalize:
        packed = _F.cloud_norm_ragged(packed, offsets, max_len)
    return _F.fps_gather_ragged(packed, offsets, max_len, number)


def peft_detect(name, targets):
    """reference utils/misc.py:22-26"""
    return any(t in name for t in targets)


def lidar_noise(points, number=64, scale=1.3, low=1.02, generator=None):
    """Outlier points p * U(low, scale) of `number` random existing points (reference
    utils/misc.py:38-46; host numpy RNG there, device RNG here)."""
    B, P, _ = points.shape
    idx = torch.randint(0, P, (number,), device=points.device, generator=generator)
    factor = torch.empty((1, number, 1), device=points.device).uniform_(low, scale, generator=generator)
    return points[:, idx, :] * factor


def gaussian_noise(shape, loc=0., scale=0.2, shell_radius=0.9, device=None, generator=None):
    """Shell noise g + shell_radius * g/|g|, g ~ N(loc, scale) (reference utils/misc.py:28-36)."""
    g = torch.empty(shape, device=device).normal_(loc, scale, generator=generator)
    return g + g / g.norm(p=2, dim=-1, keepdim=True) * shell_radius


def jitter_points(pc, std=0.01, clip=0.05, generator=None):
    """pc (B,N,3) -> pc + clamp(N(0, std), -clip, clip), a new tensor.  The reference's AdaPoinTr calls misc.jitter_points
    (models/AdaPoinTr.py:864) and its utils/misc.py does not define it; this is an ASSUMPTION: upstream PoinTr's function with its
    constants (std 0.01, clip 0.05), recalled.  The noise is drawn on pc's device and no host value is taken, so it can be captured."""
    if std < 0 or clip < 0:
        raise ValueError("jitter_points: std >= 0 and clip >= 0")
    noise = torch.empty_like(pc).normal_(0.0, std, generator=generator) if std > 0 else torch.zeros_like(pc)
    return pc + noise.clamp_(-clip, clip)


def seprate_point_cloud(xyz, num_points, crop, fixed_points=None, padding_zeros=False, sample_points=1024,
                        incomplete_shape=True, centers=None, generator=None, keep_crop=True):
    """Online cropping of reference utils/misc.py:205-256, batched on the device.

    The reference loops over the batch in Python (randn centre -> distance argsort -> slice -> one single-cloud FPS
    launch for the kept part and one for the cropped part, 2*B launches of up to 1023 rounds each).  All samples have
    the same sizes, so here the whole batch is ONE argsort, two gathers and two batched FPS launches.
    Returns (input_data (B, min(n-crop, sample_points), 3), crop_data (B, min(crop, sample_points), 3)).
    `centers` (B,1,3) overrides the random viewpoints (the reference's `fixed_points`, one per sample).  keep_crop=False: crop_data is
    None and neither its gather nor its FPS is launched (a caller that only uses the kept part)."""
    B, n, c = xyz.shape
    assert n == num_points and c == 3
    if crop == num_points:
        return xyz, None
    if isinstance(crop, (list, tuple)):
        num_crop = int(torch.randint(crop[0], crop[1] + 1, (1,), generator=generator).item())
    else:
        num_crop = crop
    if centers is None:
        if fixed_points is not None:
            fp = fixed_points[torch.randint(0, len(fixed_points), (1,)).item()] if isinstance(fixed_points, list) else fixed_points
            centers = fp.reshape(1, 1, 3).to(xyz.device).expand(B, 1, 3)
        else:
            centers = torch.nn.functional.normalize(torch.randn(B, 1, 3, device=xyz.device, generator=generator), p=2, dim=-1)
    dist = torch.norm(centers - xyz, p=2, dim=-1)                                   # (B, n)
    order = _F.argsort_rows(dist)                     # (rank-counting kernel on the device, torch.argsort on the host)
    take = lambda idx: torch.gather(xyz, 1, idx.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    crop_data = take(order[:, :num_crop]) if keep_crop else None
    if padding_zeros:
        input_data = xyz.clone()
        input_data.scatter_(1, order[:, :num_crop].unsqueeze(-1).expand(-1, -1, 3), 0.0)
    else:
        input_data = take(order[:, num_crop:])
    force = isinstance(crop, (list, tuple))
    if (incomplete_shape or force) and input_data.shape[1] > sample_points:
        input_data = fps(input_data, sample_points)[0]
    if not keep_crop:
        return input_data.contiguous(), None
    if (incomplete_shape or force) and crop_data.shape[1] > sample_points:
        crop_data = fps(crop_data, sample_points)[0]
    return input_data.contiguous(), crop_data.contiguous()


def scale_translate(pc, scale_low=2. / 3., scale_high=3. / 2., translate_range=0.2, generator=None):
    """PointcloudScaleAndTranslate (reference datasets/data_transforms.py:54-68) without the per-sample Python loop and
    host RNG: one anisotropic scale in [2/3, 3/2]^3 and one translation in [-0.2, 0.2]^3 per cloud, on the device."""
    B = pc.shape[0]
    s = torch.empty(B, 1, 3, device=pc.device).uniform_(scale_low, scale_high, generator=generator)
    t = torch.empty(B, 1, 3, device=pc.device).uniform_(-translate_range, translate_range, generator=generator)
    return pc * s + t


def noisy_train_batch(points, npoints=1024, crop_ratio=0.25, lidar=48, gauss=24, generator=None):
    """The per-step input recipe of reference tools/runner_module.py:126-186 for `noisy_train` + `incomplete_cropping`:
    (B, N_full, 3) clean clouds -> cropped + FPS-resampled (B, npoints, 3) -> + lidar outliers + shell noise ->
    scale/translate.  Everything stays on the device."""
    partial, _ = seprate_point_cloud(points, points.shape[1], int(points.shape[1] * crop_ratio), sample_points=npoints,
                                     generator=generator)
    out = [partial]
    if lidar:
        out.append(lidar_noise(partial, lidar, low=1.2, scale=1.5, generator=generator))
    if gauss:
        out.append(gaussian_noise([partial.shape[0], gauss, 3], loc=0., scale=0.1, shell_radius=0.9, device=partial.device,
                                  generator=generator))
    return scale_translate(torch.cat(out, dim=1), generator=generator).contiguous()
