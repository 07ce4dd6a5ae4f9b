"""Fixtures of the reference's own full fine-tuning models -> tests/golden/finetune_cls.npz, finetune_seg.npz, pointtransformer_keys.txt and
pointtransformer_seg_keys.txt (build machine only: needs the reference tree).

The reference classes (models/Point_MAE_cp.py PointTransformer, models/Point_MAE_segment.py PointTransformer_seg) are imported through
oracle/ref_shim.load() as they are (load() imports models.Point_MAE_cp; models.Point_MAE_segment is imported after it, here), built on
the cases below with weights from tests/_seeded.fill, and run in eval mode in float32 and in float64 (model.double()).
    classification  trans_dim 128, 2 heads, depth 4, 16 groups of 16, cls_dim 40; input unit_ball_clouds(2, 128, seed)
    segmentation    trans_dim 384, 6 heads, depth 12 (the class hard-codes 384 channels and taps 3 / 7 / 11), 32 groups of 16, cls_dim 50;
                    input unit_ball_clouds(2, 256, seed), one-hot object labels 3 and 11
Stored -- arrays only; the tests regenerate the inputs from the seed: seed, out_f32, out_f64, err_ref (the reference's own f32 against
f64 error as a fraction of the f64 output's maximum), gap.  The key files list state-dict names and shapes only.

A fixture is only meaningful where the discrete choices do not hang on rounding, so a seed must meet
  (a) the FPS picks of the f32 and the f64 run are equal;
  (b) every neighbour search -- the grouping's k nearest points of every centre and, for segmentation, the propagation's 5 nearest
      centres of every point (the reference's own square_distance, sorted) -- has equal f32 and f64 sets;
  (c) in each search the smallest gap between the k-th and (k+1)-th squared distance (float64) is at least 1e-5 of that search's largest
      squared distance.
Seeds are scanned upward from 0 and the first that passes is the one stored.

    python tools/gen_golden_finetune.py [--check-only]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

GAP = 1e-5
CASES = {
    "cls": dict(cfg=dict(trans_dim=128, depth=4, drop_path_rate=0.1, cls_dim=40, num_heads=2, group_size=16, num_group=16, encoder_dims=128),
                B=2, N=128, seed=0),
    "seg": dict(cfg=dict(trans_dim=384, depth=12, drop_path_rate=0.1, cls_dim=50, num_heads=6, group_size=16, num_group=32, encoder_dims=384),
                B=2, N=256, labels=(3, 11), seed=1),
}


def reference():
    import ref_shim
    ns = ref_shim.load()
    seg = importlib.import_module("models.Point_MAE_segment")
    return ns, {"cls": ns.cp.PointTransformer, "seg": seg.PointTransformer_seg}, seg, sys.modules["pointnet2_ops.pointnet2_utils"]


def one_hot(labels):
    return torch.nn.functional.one_hot(torch.tensor(labels), 16).float()


def _search(d, k):
    """d (B,Q,S) squared distances -> (sorted index sets of the k smallest, smallest relative k-th / (k+1)-th gap)"""
    s, i = d.sort(dim=-1)
    gap = float((s[..., k] - s[..., k - 1]).min() / s.max()) if s.shape[-1] > k else float("inf")
    return np.sort(i[..., :k].numpy(), axis=-1), gap


def run(kind, seed):
    import _seeded
    ns, classes, seg, p2u = reference()
    case = CASES[kind]
    pts = _seeded.unit_ball_clouds(case["B"], case["N"], seed=seed)
    fps_real = p2u.furthest_point_sample
    out, picks = {"seed": np.int64(seed)}, {}
    for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        model = _seeded.fill(classes[kind](ns.EasyDict(case["cfg"]))).to(dtype).eval()
        seen = []

        def fps(xyz, npoint):
            idx = fps_real(xyz, npoint)
            seen.append(idx.clone())
            return idx

        p2u.furthest_point_sample = fps
        try:
            with torch.no_grad():
                ret = model(pts.to(dtype)) if kind == "cls" else model(pts.to(dtype), one_hot(case["labels"]).to(dtype))
        finally:
            p2u.furthest_point_sample = fps_real
        assert len(seen) == 1
        picks[prec] = seen[0].numpy()
        out["out_" + prec] = ret.numpy()
    report = dict(picks=np.array_equal(picks["f32"], picks["f64"]), sets=True, gap=float("inf"), searches=0)
    # the searches, restated on the picked centres in both precisions (the reference's expanded form for the propagation's)
    for dtype in (torch.float32, torch.float64):
        p = pts.to(dtype)
        center = torch.gather(p, 1, torch.from_numpy(picks["f64"]).long().unsqueeze(-1).expand(-1, -1, 3))
        found = [_search(((center.unsqueeze(2) - p.unsqueeze(1)) ** 2).sum(-1), case["cfg"]["group_size"])]
        if kind == "seg":
            found.append(_search(seg.square_distance(p, center), 5))
        if dtype == torch.float32:
            sets32 = [f[0] for f in found]
        else:
            report["sets"] = all(np.array_equal(a, f[0]) for a, f in zip(sets32, found))
            report["gap"] = min(f[1] for f in found)
            report["searches"] = len(found)
    r64 = out["out_f64"]
    out["err_ref"] = np.float64(np.abs(out["out_f32"].astype(np.float64) - r64).max() / np.abs(r64).max())
    out["gap"] = np.float64(report["gap"])
    return out, report


def passes(r):
    return r["picks"] and r["sets"] and r["gap"] >= GAP


def keys(kind):
    ns, classes, _, _ = reference()
    model = classes[kind](ns.EasyDict(CASES[kind]["cfg"]))
    return "".join("%s %s\n" % (k, " ".join(str(s) for s in v.shape)) for k, v in model.state_dict().items())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    for kind, fname, kname in (("cls", "finetune_cls.npz", "pointtransformer_keys.txt"), ("seg", "finetune_seg.npz", "pointtransformer_seg_keys.txt")):
        first = None
        for seed in range(64):
            out, report = run(kind, seed)
            ok = passes(report)
            print("%s seed %d: %d searches, smallest relative gap %.2e, f32 sets %s, FPS picks %s -> %s"
                  % (kind, seed, report["searches"], report["gap"], "equal" if report["sets"] else "DIFFER",
                     "equal" if report["picks"] else "DIFFER", "passes" if ok else "fails"))
            if ok:
                first = seed
                break
        assert first == CASES[kind]["seed"], "%s: the first seed that passes is %s, the fixture's is %d" % (kind, first, CASES[kind]["seed"])
        print("%s: reference f32 against f64 = %.2e of the maximum (max %.4f)" % (kind, out["err_ref"], np.abs(out["out_f64"]).max()))
        if not a.check_only:
            path = os.path.join(ROOT, "tests", "golden", fname)
            np.savez_compressed(path, **out)
            print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
            with open(os.path.join(ROOT, "tests", "golden", kname), "w") as f:
                f.write(keys(kind))
