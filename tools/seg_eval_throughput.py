"""Part-segmentation evaluation throughput on a seeded unify_shapenetpart_seg model at ShapeNetPart shapes (B = 32 shapes of N = 2048
points, 50 parts).  Three paths over the same batches:
  reference_style       : eager forward, the (B, N, 50) log-probabilities copied to the host (.cpu()), the reference's numpy loop
                          (tests/_seg_reference.py restates tools/runner_unify_seg.py:301-367),
  validate_seg          : eager forward, the metric kernels on the device (utils/evaluate.py SegMetric, csrc/seg_eval.hip),
  validate_seg_captured : the forward as one HIP-graph replay (upp_hip/infer.py SegEvalStep), the same metric kernels.
Prints ONE JSON line: per path the first call (warm-up; includes the capture) and the median / min / max ms per batch over the repeats,
plus the device time of the two metric launches alone (bench.time_kernel: replayed from a graph, HIP events).
   python tools/seg_eval_throughput.py [--batch 32] [--points 2048] [--batches 3] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "iccv2025-upp_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import bench
    from _seg_reference import SEG_CLASSES, reference_metrics
    from models import build_model_from_cfg
    from upp_hip import ops
    from utils import evaluate
    from utils.config import builtin_cfg
    from utils.synthetic import unit_ball_clouds
    dev = torch.device("cuda", 0)
    model = build_model_from_cfg(builtin_cfg('unify_shapenetpart_seg').model).to(dev).eval()
    B, N, nb = a.batch, a.points, a.batches
    cats = list(SEG_CLASSES.values())
    names = sorted(SEG_CLASSES)
    batches = []
    for i in range(nb):
        rng = np.random.default_rng(i)
        c = [(i * B + j) % len(cats) for j in range(B)]
        label = torch.tensor([names.index(list(SEG_CLASSES)[k]) for k in c])
        target = torch.from_numpy(np.stack([rng.choice(cats[k], N) for k in c]))
        batches.append((unit_ball_clouds(B, N, seed=i).to(dev), label.to(dev), target.to(dev)))

    @torch.no_grad()
    def reference_style():
        got = []
        for pts, label, target in batches:
            logp = model(pts, evaluate.one_hot(label, 16), completion_prompt=False, denoise=False, point_num=N)
            got.append((logp.cpu().numpy(), target.cpu().numpy()))
        return reference_metrics(got)

    paths = {"reference_style": reference_style,
             "validate_seg": lambda: evaluate.validate_seg(model, batches),
             "validate_seg_captured": lambda: evaluate.validate_seg_captured(model, batches)}
    out = {"B": B, "N": N, "parts": 50, "batches_per_call": nb, "repeats": a.repeats}
    for name, fn in paths.items():
        first = _timed(fn) / nb
        ms = [_timed(fn) / nb for _ in range(a.repeats)]
        med = statistics.median(ms)
        res = fn()
        out[name] = {"warmup_ms_per_batch": round(first, 3), "ms_per_batch": round(med, 3), "min": round(min(ms), 3),
                     "max": round(max(ms), 3), "shapes_per_s": round(B / med * 1e3, 1),
                     "inctance_avg_iou": float(res['inctance_avg_iou'])}
    out["speedup_captured_vs_reference_style"] = round(out["reference_style"]["ms_per_batch"] / out["validate_seg_captured"]["ms_per_batch"], 2)

    with torch.no_grad():
        pts, label, target = batches[0]
        logp = model(pts, evaluate.one_hot(label, 16), completion_prompt=False, denoise=False, point_num=N)
    _, part_cat, cat_range = evaluate.seg_tables()
    part_cat, cat_range = part_cat.to(dev), cat_range.to(dev)
    acc = ops.SegAccumulator(50, 16, dev)
    pred = torch.empty((B, N), dtype=torch.long, device=dev)
    out["metric_kernels_us"] = round(1e3 * bench.time_kernel(lambda: ops.seg_iou_update(logp, target, part_cat, cat_range, acc, pred=pred)), 2)
    out["metric_kernels_no_pred_us"] = round(1e3 * bench.time_kernel(lambda: ops.seg_iou_update(logp, target, part_cat, cat_range, acc)), 2)
    out["logp_mb_per_batch"] = round(logp.numel() * 4 / 1e6, 2)
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
