"""Deformable graph attention: the module's fused path (models/Transformer_utils.py improvedDeformableLocalGraphAttention on
HF.deform_offset(ball=True) / HF.three_nn / HF.interp_edge_max, csrc/interp_max.hip) against its torch formulation (the same restatement
with the (B,N,k,C) tensors kept), forward and forward + backward, and the backward operator with the deterministic scatter
(upp_interp_max_bwd_det) against the atomic one.  Shapes (B, N, NK, k, C) in --shapes: AdaPoinTr's training shape in the self position
(576 over 576) and in the cross position (576 over 256).  f32, neighbour lists computed once outside the timed region.  Times come from
device events around --iters calls after --warmup calls, the median of --repeats windows; each (path, shape) runs in a process of its
own under its own time limit, and after one that fails or runs out of time nothing more is started.  Recorded, not gated.  Writes
profiles/deform_graph_throughput.json and prints the same JSON line.
   python tools/deform_graph_throughput.py [--shapes 32,576,576,8,384 32,576,256,8,384] [--iters 20] [--warmup 5] [--limit 180]"""
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
    ap.add_argument("--shapes", nargs="+", default=["32,576,576,8,384", "32,576,256,8,384"], help="B,N,NK,k,C")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows of --iters calls; the median is reported")
    ap.add_argument("--limit", type=int, default=180, help="seconds per (path, shape)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_graph_throughput.json"))
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
    B, N, NK, k, C = (int(s) for s in a.shapes[0].split(","))
    g = torch.Generator(device="cuda").manual_seed(1000 * N + NK)
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
        PW, Bq, w = rnd(B, NK, C), rnd(B, N, C), rnd(B, N, C)
        idx3 = torch.rand(B, N * k, NK, device="cuda", generator=g).argsort(-1)[..., :3].int().contiguous()
        w3 = torch.rand(B, N * k, 3, device="cuda", generator=g) + 0.05
        w3 = (w3 / w3.sum(-1, keepdim=True)).contiguous()
        out, arg = ops.interp_max_fwd(PW, Bq, idx3, w3, 0.2)
        calls = [("bwd_atomic", lambda: ops.interp_max_bwd(w, out, arg, idx3, w3, NK, 0.2, deterministic=False)),
                 ("bwd_det", lambda: ops.interp_max_bwd(w, out, arg, idx3, w3, NK, 0.2, deterministic=True))]
    else:
        m = _seeded.fill(Transformer_utils.improvedDeformableLocalGraphAttention(C, k=k)).cuda()
        if a.path == "torch":
            m.fusable = lambda q, v: False
        q, v, w = rnd(B, N, C).requires_grad_(), rnd(B, NK, C).requires_grad_(), rnd(B, N, C)
        q_pos, v_pos = _seeded.unit_ball_clouds(B, N, seed=1).cuda(), _seeded.unit_ball_clouds(B, NK, seed=2).cuda()
        idx = Transformer_utils.knn_point(k, v_pos, q_pos)
        wrt = [q, v] + [t for n, t in m.named_parameters() if "proj_v_off." not in n and "linear_offset." not in n]

        def fwd():
            with torch.no_grad():
                return m(q, q_pos, v=v, v_pos=v_pos, idx=idx)

        def fwd_bwd():
            return torch.autograd.grad(m(q, q_pos, v=v, v_pos=v_pos, idx=idx), wrt, w)
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
