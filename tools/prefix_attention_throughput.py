"""Denoising-query attention core: ops.xattn_prefix_fwd / xattn_prefix_bwd (csrc/attn_stream.hip) against  (i) the torch masked formulation
(q k^T -> * scale -> masked_fill(mask, -finfo.max) -> softmax -> @ v and its autograd, reference models/Transformer_utils.py:100-120),
which is what AdaPoinTr's decoder runs in training without the kernels, and  (ii) ops.xattn_fwd / xattn_bwd without a mask on the same
operands: the masked call has fewer blocks to walk and should not be slower.  Shapes (B, H, L, D) in --shapes: L tokens of which the last
D are denoising queries, both splits L - D; upstream's 512 + 64 queries and 96 + 64.  head_dim 64, f32; q, k, v are the three views of one
packed (B, L, 3 H 64) product in every path.  Times come from device events around --iters calls after --warmup calls, the median of
--repeats windows; each (path, shape) runs in a process of its own under its own time limit, and after one that fails or runs out of
time nothing more is started.  FLOPs are the algorithm's over the VISIBLE (query, key) pairs P = (L - D)^2 + D L: forward 4 B H P 64,
backward 10 B H P 64 -- the unmasked path is charged the same P, so its figure is comparable, not its own work.  Writes
profiles/prefix_attention_throughput.json and prints the same JSON line.
   python tools/prefix_attention_throughput.py [--shapes 32,6,576,64 32,6,160,64] [--iters 50] [--warmup 10] [--limit 120]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("prefix", "unmasked", "torch")


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32,6,576,64", "32,6,160,64"], help="B,H,L,D")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows of --iters calls; the median is reported")
    ap.add_argument("--limit", type=int, default=120, help="seconds per (path, shape)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_attention_throughput.json"))
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path at --shapes[0] in this process")
    return ap.parse_args()


def _one(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd")]
    import torch
    from upp_hip import ops
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not fall back")
    B, H, L, D = (int(s) for s in a.shapes[0].split(","))
    scale, R = 0.125, L - D
    g = torch.Generator(device="cuda").manual_seed(1000 * L + D)
    qkv = torch.randn(B, L, 3, H * 64, device="cuda", generator=g)
    w = torch.randn(B, L, H * 64, device="cuda", generator=g)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]

    if a.path == "prefix":
        ctx, lse = ops.xattn_prefix_fwd(q, k, v, B, L, L, H, scale, R, R)
        fwd = lambda: ops.xattn_prefix_fwd(q, k, v, B, L, L, H, scale, R, R)
        bwd = lambda: ops.xattn_prefix_bwd(q, k, v, ctx, w, lse, B, L, L, H, scale, R, R)
    elif a.path == "unmasked":
        ctx, lse = ops.xattn_fwd(q, k, v, B, L, L, H, scale)
        fwd = lambda: ops.xattn_fwd(q, k, v, B, L, L, H, scale)
        bwd = lambda: ops.xattn_bwd(q, k, v, ctx, w, lse, B, L, L, H, scale)
    else:
        x = qkv.clone().requires_grad_(True)
        mask = torch.zeros(L, L, device="cuda")
        mask[:-D, -D:] = 1.

        def formulation():
            qh, kh, vh = x.view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
            attn = (qh @ kh.transpose(-2, -1)) * scale
            attn = attn.masked_fill(mask > 0, -torch.finfo(attn.dtype).max).softmax(-1)
            return (attn @ vh).transpose(1, 2).reshape(B, L, H * 64)

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

    res, pairs = {}, R * R + D * L
    for name, fn, flops in (("fwd", fwd, 4.0 * B * H * pairs * 64), ("bwd", bwd, 10.0 * B * H * pairs * 64)):
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
            for other in ("torch", "unmasked"):
                for d in ("fwd", "bwd"):
                    row["%s_over_prefix_%s" % (other, d)] = round(row[other][d]["us"] / row["prefix"][d]["us"], 2)
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
