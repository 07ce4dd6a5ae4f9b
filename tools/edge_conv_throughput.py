"""Forward + backward of the DGCNN grouper (models/dgcnn_group.py) at B = 32, N = 2048 (FPS to 512, then 128) on two paths:
  fused : the module as shipped -- upp_knn, two per-point Linear products and the edge-convolution kernels per layer,
  torch : the same weights through torch operators -- the full (B, Nq, Nk) distance matrix and topk, the gathered (B, Nq, 16, 2C)
          neighbourhood tensor, the conv as a matrix product on it, F.group_norm, leaky_relu, max.  (FPS is the library's on both paths:
          torch has none.)
Each path runs in a process of its own under `timeout -k 10`; after a path that fails or runs out of time nothing more is started.  A
window is --calls back-to-back forward + backward passes between two synchronisations; the figure is the median of 5 windows in
milliseconds per pass (host clock around work that ends in a synchronisation).  Peak memory is torch.cuda.max_memory_allocated over one
pass, above what was allocated before it.  Writes profiles/edge_conv_throughput.json and prints the same JSON line.  Recorded, not gated.
   python tools/edge_conv_throughput.py [--calls 10] [--limit 240]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(B=32, N=2048, n1=512, n2=128, k=16)
PATHS = ("fused", "torch")
WINDOWS = 5


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="passes per timed window")
    ap.add_argument("--limit", type=int, default=240, help="seconds per path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_conv_throughput.json"))
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path in this process")
    return ap.parse_args()


def _torch_grouper(model, x, n1, n2, k):
    import torch
    import torch.nn.functional as F
    from upp_hip import functional as HF

    def edge(layer, cq, fq, ck, fk):
        with torch.no_grad():
            d = -2 * cq @ ck.transpose(1, 2) + (cq * cq).sum(-1, keepdim=True) + (ck * ck).sum(-1).unsqueeze(1)
            idx = d.topk(k, dim=-1, largest=False, sorted=False)[1]
        B, Nq, _ = idx.shape
        C = fk.shape[2]
        nb = torch.gather(fk, 1, idx.reshape(B, Nq * k, 1).expand(-1, -1, C)).view(B, Nq, k, C)
        e = torch.cat([nb - fq.unsqueeze(2), fq.unsqueeze(2).expand(-1, -1, k, -1)], -1)
        y = e @ layer[0].weight.view(-1, 2 * C).t()
        y = layer[1](y.permute(0, 3, 1, 2))
        return layer[2](y).max(dim=-1)[0].transpose(1, 2)

    def down(c, f, n):
        cq, i = HF.fps_gather(c, n)
        return cq, torch.gather(f, 1, i.long().unsqueeze(-1).expand(-1, -1, f.shape[2]))

    f = F.linear(x, model.input_trans.weight[:, :, 0], model.input_trans.bias)
    f = edge(model.layer1, x, f, x, f)
    cq, fq = down(x, f, n1)
    f = edge(model.layer2, cq, fq, x, f)
    f = edge(model.layer3, cq, f, cq, f)
    c2, fq = down(cq, f, n2)
    return c2, edge(model.layer4, c2, fq, cq, f)


def _one_path(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd"), os.path.join(ROOT, "tests")]
    import torch
    import _seeded
    from models.dgcnn_group import DGCNN_Grouper
    s = SHAPE
    dev = torch.device("cuda", 0)
    model = _seeded.fill(DGCNN_Grouper(k=s["k"])).to(dev).train()
    x = _seeded.unit_ball_clouds(s["B"], s["N"], seed=0).to(dev)
    g_f = torch.randn(s["B"], s["n2"], 128, generator=torch.Generator().manual_seed(1)).to(dev)

    def step():
        model.zero_grad(set_to_none=True)
        if a.path == "fused":
            _, f = model(x, [s["n1"], s["n2"]])
        else:
            _, f = _torch_grouper(model, x, s["n1"], s["n2"], s["k"])
        f.backward(g_f)

    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / a.calls)
    print(json.dumps({"ms_per_pass": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
                      "peak_mb": round(peak / 2 ** 20, 1), "device": torch.cuda.get_device_name(dev)}))


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
        out["torch_over_fused_time"] = round(out["torch"]["ms_per_pass"] / out["fused"]["ms_per_pass"], 2)
        out["torch_over_fused_peak"] = round(out["torch"]["peak_mb"] / max(out["fused"]["peak_mb"], 1e-9), 2)
    line = json.dumps(out)
    if ok:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
