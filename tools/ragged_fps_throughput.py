"""Sampling throughput for a batch of scans of DIFFERENT sizes (the reference's datasets/RealSensorDataset.py input path): B seeded scans
with lengths drawn from [--min-len, --max-len], each normalised (pc_norm) and sampled to --npoints.  Three paths over the same scans:
  per_scan_loop : the reference's way -- pc_norm in numpy on the host, one upload and one utils.misc.fps launch per scan,
  ragged        : utils.ingest.RaggedBatcher -- one upload, upp_cloud_norm_ragged + upp_fps_ragged, two launches per batch,
  dense_floor   : upp_fps on B clouds that all have the LONGEST length (the dense kernel at the launch geometry the ragged one is given;
                  no normalisation, points resident) -- what a batch of equal scans would cost.
For the first two both the whole path ("end_to_end": host work, upload, kernels) and the sampling alone on resident, normalised points
("device_only") are timed.  Every path runs in a process of its own under its own time limit; after a path that fails or runs out of
time nothing more is started.  Prints ONE JSON line: per path the first call (warm-up) and the median / min / max ms per batch.
   python tools/ragged_fps_throughput.py [--batch 32] [--min-len 1500] [--max-len 8000] [--npoints 1024] [--repeats 20] [--limit 120]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("per_scan_loop", "ragged", "dense_floor")


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-len", type=int, default=1500)
    ap.add_argument("--max-len", type=int, default=8000)
    ap.add_argument("--npoints", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120, help="seconds per path")
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path in this process")
    return ap.parse_args()


def _one_path(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd")]
    import numpy as np
    import torch
    from upp_hip import ops
    from utils import misc
    from utils.ingest import RaggedBatcher
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    lengths = [int(n) for n in rng.integers(a.min_len, a.max_len + 1, size=a.batch)]
    lengths[0] = a.max_len
    scans = [rng.normal(size=(n, 3)) * rng.uniform(0.5, 3.0) + rng.normal(size=3) for n in lengths]

    def pc_norm(s):
        return s / (np.max(np.sqrt(np.sum(s ** 2, axis=1))) * 2)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(fn):
        first = timed(fn)
        ms = [timed(fn) for _ in range(a.repeats)]
        return {"warmup_ms": round(first, 3), "ms_per_batch": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}

    normed = [torch.from_numpy(pc_norm(s)).float().to(dev) for s in scans]
    out = {}
    if a.path == "per_scan_loop":
        out["end_to_end"] = stats(lambda: [misc.fps(torch.from_numpy(pc_norm(s)).float().to(dev)[None], a.npoints)[0][0] for s in scans])
        resident = [c[None].contiguous() for c in normed]
        out["device_only"] = stats(lambda: [ops.fps(c, a.npoints, want_centers=True) for c in resident])
    elif a.path == "ragged":
        items = [(s, 0) for s in scans]
        out["end_to_end"] = stats(lambda: list(RaggedBatcher(items, a.npoints, a.batch, dev)))
        packed = torch.cat(normed).contiguous()
        offsets, max_len = ops.ragged_layout(lengths, packed.shape[0])
        offsets = offsets.to(dev)
        out["device_only"] = stats(lambda: ops.fps_ragged(packed, offsets, max_len, a.npoints, want_centers=True))
        got = ops.fps_ragged(packed, offsets, max_len, a.npoints)
        same = all(torch.equal(got[b], ops.fps(c[None].contiguous(), a.npoints)[0]) for b, c in enumerate(normed))
        out["indices_equal_per_scan_fps"] = bool(same)
    else:
        g = torch.Generator().manual_seed(0)
        dense = (torch.randn(a.batch, a.max_len, 3, generator=g) * 0.3).to(dev)
        out["device_only"] = stats(lambda: ops.fps(dense, a.npoints, want_centers=True))
    out["lengths"] = {"min": min(lengths), "max": max(lengths), "mean": round(sum(lengths) / len(lengths), 1)}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


def main():
    a = _args()
    if a.path:
        return _one_path(a)
    out = {"B": a.batch, "npoints": a.npoints, "repeats": a.repeats}
    for path in PATHS:
        cmd = [sys.executable, os.path.abspath(__file__), "--path", path, "--batch", str(a.batch), "--min-len", str(a.min_len),
               "--max-len", str(a.max_len), "--npoints", str(a.npoints), "--repeats", str(a.repeats)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            out[path] = {"error": "no result within %d s" % a.limit}
            break
        if r.returncode != 0:
            out[path] = {"error": "exit status %d" % r.returncode, "stderr": r.stderr[-400:]}
            break
        res = json.loads(r.stdout.strip().splitlines()[-1])
        for k in ("lengths", "device"):
            out[k] = res.pop(k)
        out[path] = res
    if all(p in out and "error" not in out[p] for p in PATHS):
        loop, rag = out["per_scan_loop"], out["ragged"]
        out["speedup_device_only"] = round(loop["device_only"]["ms_per_batch"] / rag["device_only"]["ms_per_batch"], 2)
        out["speedup_end_to_end"] = round(loop["end_to_end"]["ms_per_batch"] / rag["end_to_end"]["ms_per_batch"], 2)
    print(json.dumps(out))
    return 0 if all("error" not in out.get(p, {"error": 1}) for p in PATHS) else 1


if __name__ == "__main__":
    sys.exit(main())
