"""Input path for scans of different sizes (the reference's datasets/RealSensorDataset.py:59-78).

The reference normalises every scan on the host (pc_norm: p / (2 max |p|) in float64) and samples it to N_POINTS with one FPS launch per
scan inside __getitem__.  FPS runs `npoints` dependent rounds whatever the batch size, so B scans cost B serial chains.  RaggedBatcher
packs `batch_size` scans back to back, uploads them once and runs the two packed-batch kernels (upp_hip.ops.cloud_norm_ragged,
fps_ragged): one chain per batch, the same bits per scan.  What it yields is what utils.evaluate.validate, validate_captured and
test_vote_captured consume."""
import numpy as np
import torch

from utils import misc


def _as_cloud(c, k):
    if isinstance(c, np.ndarray):
        c = torch.from_numpy(np.ascontiguousarray(c))
    if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 3:
        raise ValueError("RaggedBatcher: item %d is not a (n, 3) cloud" % k)
    if c.dtype not in (torch.float64, torch.float32):
        raise RuntimeError("RaggedBatcher: item %d is %s; scans are float64 or float32" % (k, c.dtype))
    if c.shape[0] < 1:
        raise ValueError("ragged batch: cloud %d is empty (every cloud needs at least one point)" % k)
    return c


class RaggedBatcher:
    """Iterable over `items` = (cloud (n_i,3) float64 or float32 ndarray / tensor, label) -> (points (B,npoints,3) f32, label (B,) int64)
    on `device`, B = batch_size (the last batch: what is left).  Order is kept: cloud i of the output is item i.

    normalize=True: the reference's pc_norm per scan, then FPS to npoints -- per scan the bits of
        misc.fps(torch.from_numpy(scan / (np.max(np.sqrt(np.sum(scan ** 2, axis=1))) * 2)).float().cuda()[None], npoints)[0]
    normalize=False: FPS alone (float64 scans are rounded to float32 first, as the reference's .float()).
    A float32 scan in a batch that also holds float64 scans is upcast (exact)."""

    def __init__(self, items, npoints, batch_size, device, normalize=True):
        if int(batch_size) < 1 or int(npoints) < 1:
            raise ValueError("RaggedBatcher: batch_size and npoints must be positive")
        self.items, self.npoints, self.batch_size = items, int(npoints), int(batch_size)
        self.device, self.normalize = torch.device(device), bool(normalize)

    def _emit(self, clouds, labels):
        lengths = [c.shape[0] for c in clouds]
        if self.normalize:
            dtype = torch.float32 if all(c.dtype == torch.float32 for c in clouds) else torch.float64
        else:
            dtype = torch.float32
        packed = torch.cat([c.to(dtype) for c in clouds]).contiguous()
        label = torch.as_tensor(np.asarray([int(np.asarray(l).reshape(-1)[0]) for l in labels], dtype=np.int64))
        packed, label = packed.to(self.device), label.to(self.device)       # ONE upload of the points per batch
        points, _ = misc.fps_ragged(packed, lengths, self.npoints, normalize=self.normalize)
        return points, label

    def __iter__(self):
        clouds, labels = [], []
        for k, (cloud, label) in enumerate(self.items):
            clouds.append(_as_cloud(cloud, k))
            labels.append(label.cpu() if isinstance(label, torch.Tensor) else label)
            if len(clouds) == self.batch_size:
                yield self._emit(clouds, labels)
                clouds, labels = [], []
        if clouds:
            yield self._emit(clouds, labels)
