"""Region-wise deformable attention: the module's fused path (models/Transformer_utils.py DeformableLocalAttention on HF.deform_offset /
HF.three_nn / HF.region_attention, csrc/region_attn.hip) against its torch formulation (the same restatement with the (B,N,k,C) tensors
and the (B,N,H,k,k) scores kept), forward and forward + backward, and the backward operator with the deterministic scatters
(upp_region_attn_bwd_det) against the atomic one.  Shapes (B, N, k, C, H, G) in --shapes: AdaPoinTr's training shape in the encoder's
self position at k = 8 and k = 16.  f32, the neighbour list computed once outside the timed region.  Times come from device events
around --iters calls after --warmup calls, the median of --repeats windows; each (path, shape) runs in a process of its own under its
own time limit, and after one that fails or runs out of time nothing more is started.  Recorded, not gated.  Writes
profiles/rw_deform_throughput.json and prints the same JSON line.
   python tools/rw_deform_throughput.py [--shapes 32,576,8,384,6,2 32,576,16,384,6,2] [--iters 20] [--warmup 5] [--limit 180]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("fused", "torch", "scatter")


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32,576,8,384,6,2", "32,576,16,384,6,2"], help="B,N,k,C,H,G")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows of --iters calls; the median is reported")
    ap.add_argument("--limit", type=int, default=180, help="seconds per (path, shape)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rw_deform_throughput.json"))
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path at --shapes[0] in this process")
    return ap.parse_args()


def _one(a):
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "iccv2025-upp_amd")]
    import torch
    import _seeded
    from models import Transformer_utils
    from upp_hip import ops
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not fall back")
    B, N, k, C, H, G = (int(s) for s in a.shapes[0].split(","))
    g = torch.Generator(device="cuda").manual_seed(1000 * N + k)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.iters          # us per call

    if a.path == "scatter":
        q, PK, PV, bk, bv, w = rnd(B, N, C), rnd(B, G, N, C), rnd(B, G, N, C), rnd(C), rnd(C), rnd(B, N, C)
        idx = torch.randint(0, N, (B, N, k), device="cuda", generator=g)
        idx3 = torch.rand(B, G, N * k, N, device="cuda", generator=g).argsort(-1)[..., :3].int().contiguous()
        w3 = torch.rand(B, G, N * k, 3, device="cuda", generator=g) + 0.05
        w3 = (w3 / w3.sum(-1, keepdim=True)).contiguous()
        scale = 0.125
        out, arg = ops.region_attn_fwd(q, idx, PK, PV, bk, bv, idx3, w3, H, scale)
        rows = torch.empty(3, B, N, k, C, device="cuda")
        calls = [("fwd", lambda: ops.region_attn_fwd(q, idx, PK, PV, bk, bv, idx3, w3, H, scale)),
                 ("bwd_atomic", lambda: ops.region_attn_bwd(q, idx, PK, PV, bk, bv, idx3, w3, arg, w, H, scale, deterministic=False,
                                                            want_krow=True, want_vrow=True)),
                 ("bwd_det", lambda: ops.region_attn_bwd(q, idx, PK, PV, bk, bv, idx3, w3, arg, w, H, scale, deterministic=True,
                                                         want_krow=True, want_vrow=True, rows=rows))]
    else:
        m = _seeded.fill(Transformer_utils.DeformableLocalAttention(C, num_heads=H, qkv_bias=True, k=k, n_group=G)).cuda()
        if a.path == "torch":
            m.fusable = lambda q, v: False
        x, w = rnd(B, N, C).requires_grad_(), rnd(B, N, C)
        pos = _seeded.unit_ball_clouds(B, N, seed=1).cuda()
        idx = Transformer_utils.knn_point(k, pos, pos)
        wrt = [x] + [t for n, t in m.named_parameters() if "proj_v_off." not in n and "linear_offset." not in n]

        def fwd():
            with torch.no_grad():
                return m(x, pos, idx=idx)

        def fwd_bwd():
            return torch.autograd.grad(m(x, pos, idx=idx), wrt, w)
        calls = [("fwd", fwd), ("fwd_bwd", fwd_bwd)]

    res = {}
    for name, fn in calls:
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        us = [window(fn) for _ in range(a.repeats)]
        res[name] = {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


def main():
    a = _args()
    if a.path:
        return _one(a)
    out = {"iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "shapes": {}}
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
            row["speedup_fwd"] = round(row["torch"]["fwd"]["us"] / row["fused"]["fwd"]["us"], 2)
            row["speedup_fwd_bwd"] = round(row["torch"]["fwd_bwd"]["us"] / row["fused"]["fwd_bwd"]["us"], 2)
            row["det_over_atomic"] = round(row["scatter"]["bwd_det"]["us"] / row["scatter"]["bwd_atomic"]["us"], 2)
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
