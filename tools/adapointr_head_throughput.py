"""The query selection of AdaPoinTr and its three concatenation-Linear sites (models/AdaPoinTr.py) at the stock sizes, on two paths:
  shipped : the selection on HF.query_select (csrc/query_select.hip); the sites as the modules run them -- per-sample and per-token
            products on HF.linear, the broadcast add, the 3-column term and the GELU as torch element-wise operators (no fused kernel),
  torch   : the reference's formulation -- argsort + expand + gather + cat for the selection, and for the sites the concatenations
            [global ; coarse], [global ; q ; coarse] and [max token ; token] built and multiplied by the same weights as torch modules.
Sizes: B 32, 576 queries (512 + 64 denoising), C 384, G 1024, H 512, 16 points per query; the selection picks Q 512 of M 768 candidates and
appends 64 points.  Timed forward and forward + backward.  Each path runs in a process of its own under `timeout -k 10`; after a path
that fails or runs out of time nothing more is started.  A window is --calls back-to-back passes between two synchronisations; the figure
is the median of 5 windows in milliseconds per pass (host clock around work that ends in a synchronisation).  Writes
profiles/adapointr_head_throughput.json and prints the same JSON line.  Recorded, not gated.
   python tools/adapointr_head_throughput.py [--calls 10] [--limit 240]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(B=32, queries=576, C=384, G=1024, H=512, step=16, M=768, Q=512, D=64)
PATHS = ("shipped", "torch")
WINDOWS = 5


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="passes per timed window")
    ap.add_argument("--limit", type=int, default=240, help="seconds per path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapointr_head_throughput.json"))
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path in this process")
    return ap.parse_args()


def _one_path(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd"), os.path.join(ROOT, "tests")]
    import torch
    import torch.nn as nn
    import _seeded
    from models import AdaPoinTr as MA
    from upp_hip import functional as HF
    s = SHAPE
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    shipped = a.path == "shipped"
    B, N, C, G = s["B"], s["queries"], s["C"], s["G"]

    class Sites(nn.Module):
        """the three layers alone, under the model's own names, so that the model's methods run on them"""
        def __init__(self):
            super().__init__()
            self.mlp_query = nn.Sequential(nn.Linear(G + 3, 1024), nn.GELU(), nn.Linear(1024, 1024), nn.GELU(), nn.Linear(1024, C))
            self.reduce_map = nn.Linear(C + G + 3, C)
            self.decode_head = MA.SimpleRebuildFCLayer(2 * C, step=s["step"], hidden_dim=s["H"])

    m = _seeded.fill(Sites()).to(dev).train()
    r = lambda *sh: torch.randn(*sh, generator=g).to(dev)          # noqa: E731
    gf, q, coarse = r(B, G).requires_grad_(), r(B, N, C).requires_grad_(), (0.5 * r(B, N, 3)).requires_grad_()
    score, cand, extra = torch.rand(B, s["M"], generator=g).to(dev), r(B, s["M"], 3).requires_grad_(), r(B, s["D"], 3).requires_grad_()
    cot = {"mlp_query": r(B, N, C), "reduce_map": r(B, N, C), "rebuild_fc": r(B, N, s["step"], 3), "query_select": r(B, s["Q"] + s["D"], 3)}

    def mlp_query():
        if shipped:
            return MA.PCTransformer.query_features(m, gf, coarse)
        return m.mlp_query(torch.cat([gf.unsqueeze(1).expand(-1, N, -1), coarse], dim=-1))

    def reduce_map():
        if shipped:
            return MA.AdaPoinTr.rebuild_feature(m, gf, q, coarse)
        return m.reduce_map(torch.cat([gf.unsqueeze(-2).expand(-1, N, -1), q, coarse], dim=-1))

    def rebuild_fc():
        if shipped:
            return m.decode_head(q)
        h = m.decode_head
        cat = torch.cat([q.max(1)[0].unsqueeze(1).expand(-1, N, -1), q], dim=-1)
        return h.layer.fc2(h.layer.act(h.layer.fc1(cat))).reshape(B, N, h.step, 3)

    def query_select():
        if shipped:
            return HF.query_select(score, cand, s["Q"], extra)[0]
        idx = torch.argsort(score.unsqueeze(-1), dim=1, descending=True)
        picked = torch.gather(cand, 1, idx[:, :s["Q"]].expand(-1, -1, 3))
        return torch.cat([picked, extra], dim=1)

    res = {}
    for name, fn in (("mlp_query", mlp_query), ("reduce_map", reduce_map), ("rebuild_fc", rebuild_fc), ("query_select", query_select)):
        for backward in (False, True):
            def one():
                out = fn()
                if backward:
                    m.zero_grad(set_to_none=True)
                    gf.grad = q.grad = coarse.grad = cand.grad = extra.grad = None
                    out.backward(cot[name])

            with (torch.enable_grad() if backward else torch.no_grad()):
                one()
                torch.cuda.synchronize()
                ms = []
                for _ in range(WINDOWS):
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        one()
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3 / a.calls)
            res["%s_%s" % (name, "fwd_bwd" if backward else "fwd")] = {"ms_per_pass": round(statistics.median(ms), 4), "min": round(min(ms), 4),
                                                                      "max": round(max(ms), 4)}
    res["declined"] = sorted("%s: %s" % k for k in HF._declined)
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
        out["torch_over_shipped_time"] = {k: round(out["torch"][k]["ms_per_pass"] / out["shipped"][k]["ms_per_pass"], 2)
                                          for k in out["shipped"] if k != "declined"}
    line = json.dumps(out)
    if ok:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
