"""Cross-attention core: ops.xattn_fwd / ops.xattn_bwd (csrc/attn_stream.hip) against the torch formulation (q k^T -> * scale -> softmax
-> @ v and its autograd, reference models/Transformer.py:144-152), which is what a decoder block runs without the kernels.  Shapes
(B, H, Lq, Lk) in --shapes: PoinTr's decoder (224 queries over 128 proxies), AdaPoinTr's with its denoising queries (576 over 256) and
64 over 64, the short case that the single streaming family serves worst.  head_dim 64, f32, three separate dense operands.  Times come
from device events around --iters calls after --warmup calls, the median of --repeats windows; each (path, shape) runs in a process of
its own under its own time limit, and after one that fails or runs out of time nothing more is started.  FLOPs are the algorithm's:
forward 4 B H Lq Lk 64, backward 10 B H Lq Lk 64 (five products; the kernels' recomputation of S and dP is not counted).  Writes
profiles/cross_attention_throughput.json and prints the same JSON line.
   python tools/cross_attention_throughput.py [--shapes 32,6,224,128 32,6,576,256 32,6,64,64] [--iters 50] [--warmup 10] [--limit 120]"""
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
    ap.add_argument("--shapes", nargs="+", default=["32,6,224,128", "32,6,576,256", "32,6,64,64"], help="B,H,Lq,Lk")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows of --iters calls; the median is reported")
    ap.add_argument("--limit", type=int, default=120, help="seconds per (path, shape)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_attention_throughput.json"))
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path at --shapes[0] in this process")
    return ap.parse_args()


def _one(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd")]
    import torch
    from upp_hip import ops
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not fall back")
    B, H, Lq, Lk = (int(s) for s in a.shapes[0].split(","))
    scale = 0.125
    g = torch.Generator(device="cuda").manual_seed(1000 * Lq + Lk)
    q, w = (torch.randn(B, Lq, H * 64, device="cuda", generator=g) for _ in range(2))
    k, v = (torch.randn(B, Lk, H * 64, device="cuda", generator=g) for _ in range(2))

    if a.path == "kernels":
        ctx, lse = ops.xattn_fwd(q, k, v, B, Lq, Lk, H, scale)
        fwd = lambda: ops.xattn_fwd(q, k, v, B, Lq, Lk, H, scale)
        bwd = lambda: ops.xattn_bwd(q, k, v, ctx, w, lse, B, Lq, Lk, H, scale)
    else:
        x = [t.clone().requires_grad_(True) for t in (q, k, v)]

        def formulation():
            qh, kh, vh = (t.view(B, L, H, 64).permute(0, 2, 1, 3) for t, L in zip(x, (Lq, Lk, Lk)))
            return (((qh @ kh.transpose(-2, -1)) * scale).softmax(-1) @ vh).transpose(1, 2).reshape(B, Lq, H * 64)

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
    for name, fn, flops in (("fwd", fwd, 4.0 * B * H * Lq * Lk * 64), ("bwd", bwd, 10.0 * B * H * Lq * Lk * 64)):
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
    out = {"head_dim": 64, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "shapes": {}}
    ok = True
    for shape in a.shapes:
        row = {}
        for path in PATHS:
            cmd = [sys.executable, os.path.abspath(__file__), "--path", path, "--shapes", shape, "--iters", str(a.iters), "--warmup", str(a.warmup),
                   "--repeats", str(a.repeats)]
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
        out["shapes"][shape] = row
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
