"""The full fine-tuning steps beside the PEFT steps of bench.py, and HF.tap_pool beside its unfused formulation, on one GPU:
  finetune_cls : PointTransformer (cfgs/finetune_modelnet_cls.yaml), upp_hip.recipes.finetune_cls under TrainStep, B 32, N 1024
  peft_cls     : bench.py's headline step (Point_MAE_unify, noisy-train, PEFT parameter list), one stream and pipelined, B 32
  finetune_seg : PointTransformer_seg (cfgs/finetune_shapenetpart_seg.yaml), upp_hip.recipes.finetune_seg under TrainStep, B 32, N 2048
  peft_seg     : bench.py --workload seg (Point_MAE_unify_seg, PEFT parameter list), B 32
  tap_pool     : HF.tap_pool forward + backward at (32, 128, 384) against three HF.layer_norm, torch.cat, max and mean over the tokens
The steps are captured (HIP-graph replays).  A window is --steps back-to-back steps between two device events; the figure is the median of
3 windows in milliseconds per step, after --warmup steps.  The PEFT steps do other work than the full fine-tuning ones (they run the
prompting front-end and train 1-2 % of the parameters): the pairs say what each recipe costs on this box, not which kernel is faster.
Each path runs in a process of its own under `timeout -k 10`; after a path that fails or runs out of time nothing more is started.
Writes profiles/finetune_throughput.json and prints the same JSON line.  Recorded, not gated.
   python tools/finetune_throughput.py [--steps 30] [--warmup 10] [--limit 240]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("finetune_cls", "peft_cls", "finetune_seg", "peft_seg", "tap_pool")
WINDOWS = 3
TAP_SHAPE = (32, 128, 384)


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--limit", type=int, default=240, help="seconds per path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_throughput.json"))
    ap.add_argument("--path", choices=PATHS, help="(internal) run one path in this process")
    return ap.parse_args()


def _windows(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return {"ms_per_step": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def _one_path(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd"), os.path.join(ROOT, "tests")]
    import torch
    import _seeded
    from upp_hip import functional as HF
    dev = torch.device("cuda", 0)
    B = a.batch
    res = {}
    if a.path in ("finetune_cls", "finetune_seg"):
        from models import build_model_from_cfg
        from upp_hip import recipes
        from upp_hip.train import TrainStep
        from utils.config import cfg_from_yaml_file
        seg = a.path == "finetune_seg"
        cfg = cfg_from_yaml_file(os.path.join(ROOT, "iccv2025-upp_amd", "cfgs", "finetune_shapenetpart_seg.yaml" if seg else "finetune_modelnet_cls.yaml"))
        model = _seeded.fill(build_model_from_cfg(cfg.model)).to(dev).train()
        g = torch.Generator().manual_seed(0)
        pts = _seeded.unit_ball_clouds(B, cfg.npoints, seed=1).to(dev)
        if seg:
            inputs = [pts, torch.nn.functional.one_hot(torch.randint(0, 16, (B,), generator=g), 16).float().to(dev),
                      torch.randint(0, 50, (B * cfg.npoints,), generator=g).to(dev)]
        else:
            inputs = [pts, torch.randint(0, 40, (B,), generator=g).to(dev)]
        ts = TrainStep(model, tuple(pts.shape), loss_fn=recipes.finetune_seg if seg else recipes.finetune_cls, inputs=inputs)
        res["step"] = _windows(torch, lambda: ts.step_inputs(*inputs), a.steps, a.warmup)
        res["loss"] = float(ts.loss)
        res["trainable_parameters"] = sum(p.numel() for p in model.parameters() if p.requires_grad)
    elif a.path in ("peft_cls", "peft_seg"):
        import bench
        forms = (("one_stream", False), ("pipelined", True)) if a.path == "peft_cls" else (("one_stream", False),)
        for name, pipe in forms:
            tr = bench.Trainer(dev, B, False, use_graph=True, pipeline=pipe) if a.path == "peft_cls" else \
                bench.RecipeTrainer("seg", dev, B, use_graph=True, pipeline=pipe)
            res["step" if name == "one_stream" else "step_" + name] = _windows(torch, tr.step, a.steps, a.warmup)
            res["trainable_parameters"] = sum(p.numel() for p in tr.model.parameters() if p.requires_grad)
            del tr
    else:
        Bt, G, C = TAP_SHAPE
        g = torch.Generator().manual_seed(1)
        taps = [torch.randn(Bt, G, C, generator=g).to(dev).requires_grad_() for _ in range(3)]
        ln = torch.nn.LayerNorm(C).to(dev)
        cot = [torch.randn(s, generator=g).to(dev) for s in ((Bt, G, 3 * C), (Bt, 3 * C), (Bt, 3 * C))]

        def fused():
            return HF.tap_pool(taps[0], taps[1], taps[2], ln)

        def unfused():
            x = torch.cat([HF.layer_norm(t, ln) for t in taps], dim=-1)
            return x, x.max(dim=1)[0], torch.mean(x, 1)

        def pass_of(fn):
            def one():
                for t in taps:
                    t.grad = None
                ln.weight.grad = ln.bias.grad = None
                torch.autograd.backward(list(fn()), cot)
            return one
        # alternate the two formulations window by window: other work shares the box
        for name, fn in (("fused", fused), ("unfused", unfused), ("fused_again", fused), ("unfused_again", unfused)):
            res[name + "_fwd_bwd"] = _windows(torch, pass_of(fn), 10 * a.steps, a.warmup)
        with torch.no_grad():
            res["fused_fwd"] = _windows(torch, fused, 10 * a.steps, a.warmup)
            res["unfused_fwd"] = _windows(torch, unfused, 10 * a.steps, a.warmup)
    res["declined"] = sorted("%s: %s" % k for k in HF._declined)
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res))


def main():
    a = _args()
    if a.path:
        return _one_path(a)
    out = {"steps_per_window": a.steps, "windows": WINDOWS, "warmup": a.warmup, "batch": a.batch, "tap_pool_shape": list(TAP_SHAPE)}
    ok = True
    for path in PATHS:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--path", path, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--batch", str(a.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            out[path] = {"error": "exit status %d" % r.returncode, "stderr": r.stderr[-400:]}
            ok = False
            break
        res = json.loads(r.stdout.strip().splitlines()[-1])
        out["device"] = res.pop("device")
        out[path] = res
    if ok:
        out["finetune_over_peft_step_time"] = {"cls": round(out["finetune_cls"]["step"]["ms_per_step"] / out["peft_cls"]["step"]["ms_per_step"], 3),
                                               "seg": round(out["finetune_seg"]["step"]["ms_per_step"] / out["peft_seg"]["step"]["ms_per_step"], 3)}
        t = out["tap_pool"]
        out["unfused_over_fused_time"] = {"fwd_bwd": round(t["unfused_fwd_bwd"]["ms_per_step"] / t["fused_fwd_bwd"]["ms_per_step"], 3),
                                          "fwd": round(t["unfused_fwd"]["ms_per_step"] / t["fused_fwd"]["ms_per_step"], 3)}
    line = json.dumps(out)
    if ok:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
