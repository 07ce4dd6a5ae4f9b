"""Attention core beyond 160 tokens: ops.attn_fwd / ops.attn_bwd (csrc/attn_stream.hip) against the torch formulation
(q k^T -> * scale -> softmax -> @ v and its autograd, reference models/Point_MAE_pretask_dev.py:186-193), which is what a block runs at
these lengths without the kernels.  L in --lengths, B = --batch, H = --heads, head_dim 64, f32.  Times come from device events around
--iters calls after --warmup calls; each (path, L) runs in a process of its own under its own time limit, and after one that fails or
runs out of time nothing more is started.  FLOPs are the algorithm's: forward 4 B H L^2 64, backward 10 B H L^2 64 (five products; the
kernels' recomputation of S and dP is not counted).  Writes profiles/attn_stream_throughput.json and prints the same JSON line.
   python tools/attn_stream_throughput.py [--lengths 257 513 1025] [--batch 32] [--heads 6] [--iters 50] [--warmup 10] [--limit 120]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("kernels", "torch")


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="+", default=[257, 513, 1025])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--heads", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows of --iters calls; the median is reported")
    ap.add_argument("--limit", type=int, default=120, help="seconds per (path, L)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_stream_throughput.json"))
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path at --lengths[0] in this process")
    return ap.parse_args()


def _one(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd")]
    import torch
    from upp_hip import ops
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not fall back")
    B, L, H, scale = a.batch, a.lengths[0], a.heads, 0.125
    g = torch.Generator(device="cuda").manual_seed(L)
    qkv = torch.randn(B, L, 3 * H * 64, device="cuda", generator=g)
    w = torch.randn(B, L, H * 64, device="cuda", generator=g)

    if a.path == "kernels":
        ctx, lse = ops.attn_fwd(qkv, B, L, H, scale)
        fwd = lambda: ops.attn_fwd(qkv, B, L, H, scale)
        bwd = lambda: ops.attn_bwd(qkv, ctx, w, lse, B, L, H, scale)
    else:
        x = qkv.clone().requires_grad_(True)

        def formulation():
            q, k, v = x.view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
            return (((q @ k.transpose(-2, -1)) * scale).softmax(-1) @ v).transpose(1, 2).reshape(B, L, H * 64)

        def fwd():
            with torch.no_grad():
                return formulation()
        out = formulation()
        bwd = lambda: torch.autograd.grad(out, x, w, retain_graph=True)

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.iters          # us per call

    res = {}
    for name, fn, flops in (("fwd", fwd, 4.0 * B * H * L * L * 64), ("bwd", bwd, 10.0 * B * H * L * L * 64)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        us = [window(fn) for _ in range(a.repeats)]
        med = statistics.median(us)
        res[name] = {"us": round(med, 2), "min": round(min(us), 2), "max": round(max(us), 2), "tflops": round(flops / med * 1e-6, 2)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


def main():
    a = _args()
    if a.path:
        return _one(a)
    out = {"B": a.batch, "H": a.heads, "head_dim": 64, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "lengths": {}}
    ok = True
    for L in a.lengths:
        row = {}
        for path in PATHS:
            cmd = [sys.executable, os.path.abspath(__file__), "--path", path, "--lengths", str(L), "--batch", str(a.batch), "--heads", str(a.heads),
                   "--iters", str(a.iters), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                row[path], ok = {"error": "no result within %d s" % a.limit}, False
                break
            if r.returncode != 0:
                row[path], ok = {"error": "exit status %d" % r.returncode, "stderr": r.stderr[-400:]}, False
                break
            res = json.loads(r.stdout.strip().splitlines()[-1])
            out["device"] = res.pop("device")
            row[path] = res
        if ok:
            row["speedup_fwd"] = round(row["torch"]["fwd"]["us"] / row["kernels"]["fwd"]["us"], 2)
            row["speedup_bwd"] = round(row["torch"]["bwd"]["us"] / row["kernels"]["bwd"]["us"], 2)
        out["lengths"][str(L)] = row
        if not ok:
            break
    line = json.dumps(out)
    if ok:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
