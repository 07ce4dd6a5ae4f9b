"""The expand sites of PoinTr (models/PoinTr.py Fold, models/Transformer.py PCTransformer.query_features) at the model's usual size, on two
paths:
  fused : the modules as shipped -- one per-row Linear product and HF.expand_act (csrc/expand.hip) for the first layer of each folding and
          of mlp_query; the later layers on HF.linear and the BatchNorm-over-rows kernels,
  torch : the same weights through the reference's formulation -- the (R, C + 2 | 3, S) concatenations of Fold and the (B, M, 1027)
          concatenation of mlp_query are built, and the Sequential(Conv1d, BatchNorm1d, ReLU, ...) stacks run on them as torch modules.
Timed: Fold forward and forward + backward at (R, S, C) = (7168, 64, 384) (B = 32, M = 224, hidden 256, training mode), and the mlp_query
site forward and forward + backward at (B, M) = (32, 224).  Each path runs in a process of its own under `timeout -k 10`; after a path
that fails or runs out of time nothing more is started.  A window is --calls back-to-back passes between two synchronisations; the figure is
the median of 5 windows in milliseconds per pass (host clock around work that ends in a synchronisation).  Peak memory is
torch.cuda.max_memory_allocated over one forward + backward, above what was allocated before it.  Writes
profiles/pointr_fold_throughput.json and prints the same JSON line.  Recorded, not gated.
   python tools/pointr_fold_throughput.py [--calls 10] [--limit 240]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(R=7168, S=64, C=384, hidden=256, B=32, M=224)
PATHS = ("fused", "torch")
WINDOWS = 5


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="passes per timed window")
    ap.add_argument("--limit", type=int, default=240, help="seconds per path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointr_fold_throughput.json"))
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path in this process")
    return ap.parse_args()


def _torch_fold(fold, x):
    """reference models/PoinTr.py:47-58"""
    import torch
    S = fold.step * fold.step
    R = x.shape[0]
    features = x.view(R, fold.in_channel, 1).expand(R, fold.in_channel, S)
    seed = fold.folding_seed.to(x.device).view(1, 2, S).expand(R, 2, S)
    fd1 = fold.folding1(torch.cat([seed, features], dim=1))
    return fold.folding2(torch.cat([fd1, features], dim=1))


def _torch_query(tr, gf, coarse):
    """reference models/Transformer.py:413-416"""
    import torch
    feature = torch.cat([gf.unsqueeze(1).expand(-1, coarse.shape[1], -1), coarse], dim=-1)
    return tr.mlp_query(feature.transpose(1, 2)).transpose(1, 2)


def _one_path(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd"), os.path.join(ROOT, "tests")]
    import torch
    import _seeded
    from models.PoinTr import Fold
    from models.Transformer import PCTransformer
    s = SHAPE
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    fold = _seeded.fill(Fold(s["C"], step=int(s["S"] ** 0.5), hidden_dim=s["hidden"])).to(dev).train()
    tr = _seeded.fill(PCTransformer(embed_dim=s["C"], depth=[0, 0], num_query=s["M"], knn_layer=0)).to(dev).train()
    x = torch.randn(s["R"], s["C"], generator=g).to(dev).requires_grad_()
    g_fold = torch.randn(s["R"], 3, s["S"], generator=g).to(dev)
    gf = torch.randn(s["B"], 1024, generator=g).to(dev).requires_grad_()
    coarse = (0.5 * torch.randn(s["B"], s["M"], 3, generator=g)).to(dev).requires_grad_()
    g_q = torch.randn(s["B"], s["M"], s["C"], generator=g).to(dev)
    fused = a.path == "fused"

    def fold_pass(backward):
        out = fold(x) if fused else _torch_fold(fold, x)
        if backward:
            fold.zero_grad(set_to_none=True)
            x.grad = None
            out.backward(g_fold)

    def query_pass(backward):
        out = tr.query_features(gf, coarse) if fused else _torch_query(tr, gf, coarse)
        if backward:
            tr.zero_grad(set_to_none=True)
            gf.grad = coarse.grad = None
            out.backward(g_q)

    res = {}
    for name, fn in (("fold", fold_pass), ("mlp_query", query_pass)):
        for backward in (False, True):
            ctx = torch.enable_grad() if backward else torch.no_grad()
            with ctx:
                fn(backward)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fn(backward)
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - base
                ms = []
                for _ in range(WINDOWS):
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        fn(backward)
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3 / a.calls)
            res["%s_%s" % (name, "fwd_bwd" if backward else "fwd")] = {"ms_per_pass": round(statistics.median(ms), 3), "min": round(min(ms), 3),
                                                                      "max": round(max(ms), 3), "peak_mb": round(peak / 2 ** 20, 1)}
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res))


def main():
    a = _args()
    if a.path:
        return _one_path(a)
    out = {"passes_per_window": a.calls, "windows": WINDOWS, "shape": SHAPE}
    ok = True
    for path in PATHS:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--path", path, "--calls", str(a.calls)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            out[path] = {"error": "exit status %d" % r.returncode, "stderr": r.stderr[-400:]}
            ok = False
            break
        res = json.loads(r.stdout.strip().splitlines()[-1])
        out["device"] = res.pop("device")
        out[path] = res
    if ok:
        out["torch_over_fused_time"] = {k: round(out["torch"][k]["ms_per_pass"] / out["fused"][k]["ms_per_pass"], 2) for k in out["fused"]}
    line = json.dumps(out)
    if ok:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
