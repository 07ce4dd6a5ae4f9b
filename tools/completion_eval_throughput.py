"""Point-completion (pre-task) evaluation throughput on a seeded Point_MAE_pretask_dev at ShapeNet-55 test shapes (B = 32 complete clouds
of N = 8192 points, 'easy' crop), for V = 1 (in_detail=False) and V = 8 (in_detail=True, the eight fixed viewpoints).  Three paths over
the same batches:
  reference_style              : the reference's loop (tools/runner_pretask.py:314-426): batch size 1, per (cloud, viewpoint) one crop,
                                 two FPS, one forward, four Chamfer losses read with .item(); with V = 8 also the F-Score on the host
                                 (numpy nearest neighbours of the f32 clouds, as open3d computes them) and the ignore_zeros CDs,
  validate_completion          : every viewpoint of a batch as one V B batch, the metrics on the device (utils/evaluate.py),
  validate_completion_captured : the same as one HIP-graph replay per batch (upp_hip/infer.py CompletionEvalStep).
Prints ONE JSON line: per (V, path) the first call (warm-up; includes the capture) and the median / min / max ms per batch over the
repeats (the reference-style path runs --ref-clouds clouds and is scaled to B).
   python tools/completion_eval_throughput.py [--batch 32] [--points 8192] [--batches 2] [--repeats 3] [--ref-clouds 4]"""
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


def _host_f_score(pred, gt, th=0.01):
    """Metrics._get_f_score on the host: float64 nearest-neighbour distances of the f32 clouds (numpy, chunked)."""
    from _completion_reference import nearest
    d1, d2 = np.sqrt(nearest(pred, gt)[0]), np.sqrt(nearest(gt, pred)[0])
    recall, precision = float((d2 < th).sum()) / len(d2), float((d1 < th).sum()) / len(d1)
    return 2 * recall * precision / (recall + precision) if recall + precision else 0.


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-clouds", type=int, default=4)
    a = ap.parse_args()
    from extensions.chamfer_dist import ChamferDistanceL1, ChamferDistanceL2
    from models import build_model_from_cfg
    from utils import evaluate, misc
    from utils.config import builtin_cfg
    from utils.synthetic import unit_ball_clouds
    import _seeded
    dev = torch.device("cuda", 0)
    model = _seeded.fill(build_model_from_cfg(builtin_cfg('pretask').model)).to(dev).eval()
    B, N, nb = a.batch, a.points, a.batches
    batches = [(unit_ball_clouds(B, N, seed=i).to(dev), (torch.arange(B, device=dev) + i) % 55) for i in range(nb)]
    cd_l1, cd_l2 = ChamferDistanceL1(), ChamferDistanceL2()
    cd_l1z, cd_l2z = ChamferDistanceL1(ignore_zeros=True), ChamferDistanceL2(ignore_zeros=True)

    @torch.no_grad()
    def reference_style(in_detail):
        out = []
        for gt_b, _ in batches:
            for b in range(a.ref_clouds):
                gt = gt_b[b:b + 1]
                for item in evaluate.viewpoints(in_detail):
                    partial, _ = misc.seprate_point_cloud(gt, N, evaluate.crop_count(N, 'easy'), fixed_points=torch.tensor(item))
                    partial, _ = misc.fps(partial, 1024)
                    partial_center, _ = misc.fps(partial, 128)
                    pred_center, rebuild = model(partial, train_with_gaussian=False, predict_center_num=16)
                    coarse = torch.cat([partial_center, pred_center], dim=1)
                    dense = torch.cat([partial, rebuild], dim=1)
                    out.append([cd_l1(coarse, gt).item() * 1000, cd_l2(coarse, gt).item() * 1000, cd_l1(dense, gt).item() * 1000,
                                cd_l2(dense, gt).item() * 1000])
                    if in_detail:
                        out.append([_host_f_score(dense[0].cpu().numpy(), gt[0].cpu().numpy()), cd_l1z(dense, gt).item() * 1000,
                                    cd_l2z(dense, gt).item() * 1000])
        return out

    out = {"B": B, "N": N, "mode": "easy", "batches_per_call": nb, "repeats": a.repeats, "reference_style_clouds": a.ref_clouds}
    for in_detail in (False, True):
        V = len(evaluate.viewpoints(in_detail))
        kw = dict(mode='easy', in_detail=in_detail, num_categories=55)
        paths = {"reference_style": (lambda: reference_style(in_detail), B / a.ref_clouds),
                 "validate_completion": (lambda: evaluate.validate_completion(model, batches, **kw), 1.0),
                 "validate_completion_captured": (lambda: evaluate.validate_completion_captured(model, batches, **kw), 1.0)}
        res = {}
        for name, (fn, scale) in paths.items():
            first = _timed(fn) / nb * scale
            ms = [_timed(fn) / nb * scale for _ in range(a.repeats)]
            med = statistics.median(ms)
            res[name] = {"warmup_ms_per_batch": round(first, 2), "ms_per_batch": round(med, 2), "min": round(min(ms), 2),
                         "max": round(max(ms), 2), "clouds_per_s": round(B / med * 1e3, 1)}
        r = evaluate.validate_completion(model, batches, **kw)
        res["dense_cd_l2"], res["f_score"] = r["dense_cd_l2"], r["f_score"]
        res["speedup_captured_vs_reference_style"] = round(res["reference_style"]["ms_per_batch"] /
                                                           res["validate_completion_captured"]["ms_per_batch"], 2)
        out["V%d" % V] = res
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
