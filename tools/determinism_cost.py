"""What the reproducible mode costs: every atomic scatter-add entry point against its `_det` sibling at the recipes' shapes, then the
pre-task and stage-2 steps with the mode off and on.  RECORDED, not gated (the mode is opt-in).

    python tools/determinism_cost.py [--out profiles/deterministic_cost.json] [--steps 30] [--only chamfer,group,gather,emd,three_interpolate,grouping,knn_scatter,steps]

Every measurement is a child process of its own under `timeout -k 10` (a faulting or hanging child ends the run: nothing more is started
on the device after it).  Kernel pairs: bench.time_kernel (the calls captured into a graph, the replay timed with device events), the two
forms ALTERNATED three times in the same child, medians reported.  Steps: `bench.py --workload <recipe>` unedited, once without and once
with UPP_DETERMINISTIC=1 (median of three timings: the JSON line's `value`, point clouds / s, and `ms_per_step`)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = {
    "chamfer": [(32, 32, 1024), (32, 1024, 1024), (32, 2048, 8192)],          # (B, n, m)
    "group": [(32, 1096, 32, 16), (32, 1024, 64, 32), (32, 2048, 128, 32)],   # (B, N, G, K)
    "gather": [(32, 3, 8192, 1024)],                                          # (B, C, N, M)
    "emd": [(32, 1024, 1024)],                                                # (B, n, m)
    # the deformable attention's interpolation, the call the operator serves (csrc/pointnet2.hip's header; no model of this repository
    # calls it yet: 32 clouds x 2 groups, 192 channels a group, 256 tokens x 10 shifted positions), the DGCNN grouper's neighbourhood gather (tools/edge_conv_throughput.py: 512 queries x 16
    # neighbours among 2,048 points, 32 channels), knn_points' g_p2 at the pre-task shape (tools/knn_points_throughput.py) and the edge
    # convolution's g_A at the grouper's widest layer (64 channels)
    "three_interpolate": [(64, 192, 256, 2560)],                              # (B, C, m, n)
    "grouping": [(32, 32, 2048, 512, 16)],                                    # (B, C, N, P, S)
    "knn_scatter": [(64, 72, 4, 3, 1024), (32, 512, 16, 64, 2048)],           # (N, L, K, U, M)
}


def child(kind, shape):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd")]
    import torch
    import bench
    from upp_hip import ops
    assert torch.cuda.is_available(), "determinism_cost.py measures on a GPU; there is no CPU figure"
    g = torch.Generator(device="cuda").manual_seed(0)

    def rand(*s):
        return torch.rand(*s, device="cuda", generator=g)
    if kind == "chamfer":
        B, n, m = shape
        a, b = rand(B, n, 3), rand(B, m, 3)
        _, _, i1, i2 = ops.chamfer_fwd(a, b)
        d1, d2 = rand(B, n), rand(B, m)
        fn = lambda det: ops.chamfer_bwd(a, b, i1, i2, d1, d2, deterministic=det)
    elif kind == "group":
        B, N, G, K = shape
        x = rand(B, N, 3)
        _, idx, _ = ops.knn(x, x[:, :G].contiguous(), K, want_dist=False)         # neighbour lists as the grouping stage sees them
        go = rand(B, G, K, 3)
        fn = lambda det: ops.group_bwd(go, idx, N, deterministic=det)
    elif kind == "gather":
        B, C, N, M = shape
        idx = ops.fps(rand(B, N, 3), M)
        go = rand(B, C, M)
        fn = lambda det: ops.gather_bwd(go, idx, N, deterministic=det)
    elif kind == "three_interpolate":
        B, C, m, n = shape
        dist, idx = ops.three_nn(rand(B, n, 3), rand(B, m, 3))
        w = 1.0 / (dist + 1e-8)
        w = (w / w.sum(2, keepdim=True)).contiguous()
        go = rand(B, C, n)
        fn = lambda det: ops.three_interpolate_bwd(go, idx, w, m, deterministic=det)
    elif kind == "grouping":
        B, C, N, P, S = shape
        x = rand(B, N, 3)
        idx = ops.knn(x, x[:, :P].contiguous(), S, want_dist=False)[1].int()
        go = rand(B, C, P, S)
        fn = lambda det: ops.grouping_bwd(go, idx, N, deterministic=det)
    elif kind == "knn_scatter":
        N, L, K, U, M = shape
        x = rand(N, M, 3)
        idx = ops.knn_points(x[:, :L].contiguous(), x, K=K)[1]
        src = rand(N, L, K, U)
        fn = lambda det: ops.knn_scatter_add(src, idx, M, deterministic=det)
    else:
        B, n, m = shape
        a, b = rand(B, n, 3), rand(B, m, 3)
        match = ops.emd_approxmatch(a, b)
        fn = lambda det: ops.emd_matchcost(a, b, match, deterministic=det)
    ms = {False: [], True: []}
    for _ in range(3):
        for det in (False, True):
            ms[det].append(bench.time_kernel(lambda: fn(det), iters=20))
    at, de = statistics.median(ms[False]), statistics.median(ms[True])
    print(json.dumps({"op": kind, "shape": list(shape), "atomic_us": round(at * 1e3, 2), "det_us": round(de * 1e3, 2), "det_over_atomic": round(de / at, 3),
                      "atomic_us_all": [round(v * 1e3, 2) for v in ms[False]], "det_us_all": [round(v * 1e3, 2) for v in ms[True]]}))


def run(cmd, limit, env=None):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("child %s ended with status %d: nothing more is started on the device" % (" ".join(cmd[-4:]), r.returncode))
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deterministic_cost.json"))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only", default="chamfer,group,gather,emd,three_interpolate,grouping,knn_scatter,steps")
    ap.add_argument("--child", nargs=2)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], tuple(int(v) for v in args.child[1].split(",")))
    only = args.only.split(",")
    out = {"pairs": [], "steps": []}
    for kind, shapes in PAIRS.items():
        if kind in only:
            for shape in shapes:
                out["pairs"].append(run([sys.executable, os.path.abspath(__file__), "--child", kind, ",".join(map(str, shape))], 240))
                print(out["pairs"][-1], flush=True)
    if "steps" in only:
        for recipe in ("pretask", "stage2"):
            row = {"recipe": recipe}
            for mode in ("off", "on"):
                env = {k: v for k, v in os.environ.items() if k != "UPP_DETERMINISTIC"}
                if mode == "on":
                    env["UPP_DETERMINISTIC"] = "1"
                res = run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", recipe, "--steps", str(args.steps), "--warmup", "5", "--repeats", "3",
                           "--no-cpu-baseline", "--no-stage-report"], 600, env)
                row["clouds_per_s_" + mode], row["ms_per_step_" + mode] = res["value"], res["ms_per_step"]
            row["on_over_off_time"] = round(row["clouds_per_s_off"] / row["clouds_per_s_on"], 4)
            out["steps"].append(row)
            print(row, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
