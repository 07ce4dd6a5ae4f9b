"""Throughput of pytorch3d.ops.knn_points on the library's kernels against a torch formulation (differences without cdist, then topk), at
two shapes:
  pretask : the pre-task recipe's call -- 72 noise points against 1,024 partial points, K = 4, D = 3, B = 64, return_nn=True
            (reference models/Point_MAE_pretask_dev.py:680),
  wide    : D = 32, K = 16, 2,048 x 2,048 points, B = 4.
Two paths per shape, `kernels` and `torch`, each in a process of its own under `timeout -k 10`; after a path that fails or runs out of
time nothing more is started.  A window is --calls back-to-back calls between two synchronisations; the figure is the median of 5
windows, in microseconds per call: a host clock around work that ends in a synchronisation, so the call's host cost is
in it.  Writes profiles/knn_points_throughput.json and prints the same JSON line.  Recorded, not gated.
   python tools/knn_points_throughput.py [--calls 500] [--limit 120]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"pretask": dict(B=64, P1=72, P2=1024, D=3, K=4), "wide": dict(B=4, P1=2048, P2=2048, D=32, K=16)}
PATHS = ("kernels", "torch")
WINDOWS = 5


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500, help="calls per timed window")
    ap.add_argument("--limit", type=int, default=120, help="seconds per path and shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_points_throughput.json"))
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path in this process")
    ap.add_argument("--shape", choices=tuple(SHAPES), help="(internal)")
    return ap.parse_args()


def _torch_knn_points(p1, p2, K):
    """Squared distances from the differences (no cdist: its matrix product loses the small distances), then the K smallest."""
    diff = p1.unsqueeze(2) - p2.unsqueeze(1)
    d = (diff * diff).sum(-1)
    dists, idx = d.topk(K, dim=-1, largest=False, sorted=True)
    nn = p2.gather(1, idx.reshape(idx.shape[0], -1, 1).expand(-1, -1, p2.shape[2])).reshape(*idx.shape, p2.shape[2])
    return dists, idx, nn


def _one_path(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd")]
    import torch
    import pytorch3d.ops as P3
    s = SHAPES[a.shape]
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    p1 = (torch.rand(s["B"], s["P1"], s["D"], generator=g) - 0.5).to(dev)
    p2 = (torch.rand(s["B"], s["P2"], s["D"], generator=g) - 0.5).to(dev)
    if a.path == "kernels":
        fn = lambda: P3.knn_points(p1, p2, K=s["K"], return_nn=True)
    else:
        fn = lambda: _torch_knn_points(p1, p2, s["K"])
    with torch.no_grad():
        fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(WINDOWS):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6 / a.calls)
    print(json.dumps({"us_per_call": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2),
                      "device": torch.cuda.get_device_name(dev)}))


def main():
    a = _args()
    if a.path:
        return _one_path(a)
    out = {"calls_per_window": a.calls, "windows": WINDOWS, "shapes": SHAPES}
    ok = True
    for shape in SHAPES:
        out[shape] = {}
        for path in PATHS:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--path", path, "--shape", shape,
                   "--calls", str(a.calls)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                out[shape][path] = {"error": "exit status %d" % r.returncode, "stderr": r.stderr[-400:]}
                ok = False
                break
            res = json.loads(r.stdout.strip().splitlines()[-1])
            out["device"] = res.pop("device")
            out[shape][path] = res
        if not ok:
            break
        out[shape]["torch_over_kernels"] = round(out[shape]["torch"]["us_per_call"] / out[shape]["kernels"]["us_per_call"], 2)
    line = json.dumps(out)
    if ok:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
