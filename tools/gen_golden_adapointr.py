"""Fixture of the reference's own AdaPoinTr -> tests/golden/adapointr.npz, adapointr_keys.txt and adapointr_fold_keys.txt (build machine
only: needs the reference tree).

The reference class (models/AdaPoinTr.py with models/Transformer_utils.py under it) is imported through oracle/ref_shim.load() as it is
and built on the case of tests/_adapointr_model_case.py (decoder_type fc; weights from tests/_seeded.fill).  Its training mode calls
misc.jitter_points, which its utils/misc.py does not define: this process sets that name on the reference's utils.misc module, at run
time, to the seeded noise of the case file.  The model runs in eval and in train mode, in float32 and in float64 (model.double()).
Stored -- arrays only; the tests regenerate the inputs from the seed:
    eval_{coarse,rebuild}_{f32,f64}                                       (2, 32, 3), (2, 256, 3)
    train_{pred_coarse,denoised_coarse,denoised_fine,pred_fine}_{f32,f64} (2, 32, 3), (2, 64, 3), (2, 512, 3), (2, 256, 3)
    train_loss_{f32,f64}                                                  (2,)  get_loss(ret, gt): (denoise, reconstruction)
    seed
adapointr_keys.txt lists the reference model's state-dict keys with their shapes, adapointr_fold_keys.txt those of decoder_type fold
(its Fold.__init__ calls .cuda() on the folding seed, so this process makes torch.Tensor.cuda the identity): names only.

The fixture is only meaningful where the reference's discrete choices do not hang on rounding, so a seed must meet, in both modes,
  (a) for every neighbour search (the reference takes topk(sorted=False) of the expanded squared distance; this repository's set is
      upp_knn's): the smallest gap between the k-th and (k+1)-th squared distance (float64) is at least 1e-5 of that search's largest
      squared distance, and the f32 sets equal the float64 sets;
  (b) the FPS picks of the f32 and the f64 run are equal;
  (c) the f32 and f64 rankings of all 48 candidates are the same permutation;
  (d) the smallest gap between adjacent sorted f64 ranking scores is at least 16 times the largest difference between the reference's
      own f32 and f64 scores.
Seeds are scanned upward from 0 to 63 and the first that passes is the one stored.

    python tools/gen_golden_adapointr.py [--check-only]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

SEED, GAP, SCORE_MARGIN = 14, 1e-5, 16.0


def reference():
    import ref_shim
    ns = ref_shim.load()
    torch.Tensor.cuda = lambda self, *a, **k: self                  # Fold.__init__: .cuda() on the folding seed
    return (ns, importlib.import_module("models.AdaPoinTr"), importlib.import_module("models.Transformer_utils"),
            importlib.import_module("utils.misc"), sys.modules["pointnet2_ops.pointnet2_utils"])


def run(seed):
    """-> (arrays, report): report holds the smallest relative k-th/(k+1)-th gap, whether the neighbour sets, the FPS picks and the
    rankings agree between f32 and f64, the smallest f64 score gap and the largest f32-against-f64 score difference, per mode"""
    import _adapointr_model_case as case
    import _seeded
    ns, ref, tu, misc, p2u = reference()
    misc.jitter_points = case.jitter(seed)
    x, gt = case.inputs(seed)
    knn_point, fps_real = tu.knn_point, p2u.furthest_point_sample
    out, report = {"seed": np.int64(seed)}, {}
    for mode in ("eval", "train"):
        seen = {}
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            model = _seeded.fill(ref.AdaPoinTr(ns.EasyDict(case.config()))).to(dtype).train(mode == "train")
            searches, picks, scores = [], [], []

            def traced(nsample, xyz, new_xyz):
                idx = knn_point(nsample, xyz, new_xyz)
                searches.append((xyz.detach().double(), new_xyz.detach().double(), idx.detach().clone()))
                return idx

            def fps(xyz, npoint):
                idx = fps_real(xyz, npoint)
                picks.append(idx.clone())
                return idx

            hook = model.base_model.query_ranking.register_forward_hook(lambda m, i, o: scores.append(o.detach().double().squeeze(-1)))
            tu.knn_point = ref.knn_point = traced            # (models/AdaPoinTr.py holds its own name: `from ... import *`)
            p2u.furthest_point_sample = fps
            try:
                with torch.no_grad():
                    ret = model(x.to(dtype))
                    losses = model.get_loss(ret, gt.to(dtype)) if mode == "train" else None
            finally:
                tu.knn_point = ref.knn_point = knn_point
                p2u.furthest_point_sample = fps_real
                hook.remove()
            names = case.EVAL_OUTPUTS if mode == "eval" else case.TRAIN_OUTPUTS
            assert len(ret) == len(names) and len(scores) == 1 and scores[0].shape == (case.B, case.NUM_QUERY * 3 // 2)
            for name, t in zip(names, ret):
                out["%s_%s_%s" % (mode, name, prec)] = t.numpy()
            if losses is not None:
                out["train_loss_%s" % prec] = np.array([float(v) for v in losses], dtype=np.float64 if prec == "f64" else np.float32)
            seen[prec] = dict(sets=[np.sort(idx.numpy(), axis=-1) for _, _, idx in searches], picks=[p.numpy() for p in picks],
                              scores=scores[0].numpy())
            if prec == "f64":
                rel = []
                for xyz, new_xyz, idx in searches:
                    k = idx.shape[-1]
                    d = ((new_xyz.unsqueeze(2) - xyz.unsqueeze(1)) ** 2).sum(-1).sort(dim=-1)[0]
                    if d.shape[-1] > k:
                        rel.append(float((d[..., k] - d[..., k - 1]).min() / d.max()))
                gap = min(rel)
        a, b = seen["f32"], seen["f64"]
        s64 = np.sort(b["scores"], axis=-1)
        report[mode] = dict(
            gap=gap, searches=len(b["sets"]),
            sets=len(a["sets"]) == len(b["sets"]) and all(np.array_equal(u, v) for u, v in zip(a["sets"], b["sets"])),
            picks=len(a["picks"]) == len(b["picks"]) and all(np.array_equal(u, v) for u, v in zip(a["picks"], b["picks"])),
            ranking=np.array_equal(np.argsort(-a["scores"], axis=-1, kind="stable"), np.argsort(-b["scores"], axis=-1, kind="stable")),
            score_gap=float(np.diff(s64, axis=-1).min()), score_err=float(np.abs(a["scores"] - b["scores"]).max()))
    return out, report


def passes(report):
    return all(r["gap"] >= GAP and r["sets"] and r["picks"] and r["ranking"] and r["score_gap"] >= SCORE_MARGIN * r["score_err"]
               for r in report.values())


def keys(decoder_type):
    import _adapointr_model_case as case
    ns, ref, _, _, _ = reference()
    model = ref.AdaPoinTr(ns.EasyDict(case.config(decoder_type)))
    return "".join("%s %s\n" % (k, " ".join(str(s) for s in v.shape)) for k, v in model.state_dict().items())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    first = None
    for seed in range(64):
        out, report = run(seed)
        ok = passes(report)
        for mode, r in report.items():
            print("seed %d %s: %d searches, smallest relative gap %.2e, f32 sets %s, FPS picks %s, rankings %s, smallest score gap %.2e "
                  "against a score error of %.2e (x %.0f)" % (seed, mode, r["searches"], r["gap"], "equal" if r["sets"] else "DIFFER",
                                                             "equal" if r["picks"] else "DIFFER", "equal" if r["ranking"] else "DIFFER",
                                                             r["score_gap"], r["score_err"], r["score_gap"] / max(r["score_err"], 1e-300)))
        print("seed %d -> %s" % (seed, "passes" if ok else "fails"))
        if ok:
            first = seed
            break
    assert first == SEED, "the first seed that passes is %s, the fixture's is %d" % (first, SEED)
    for name in sorted(out):
        if name.endswith("_f64"):
            r64 = out[name]
            print("%s: reference f32 against f64 = %.2e of the maximum (max %.4f)"
                  % (name[:-4], np.abs(out[name[:-4] + "_f32"].astype(np.float64) - r64).max() / np.abs(r64).max(), np.abs(r64).max()))
    if not a.check_only:
        path = os.path.join(ROOT, "tests", "golden", "adapointr.npz")
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
        for decoder_type, fname in (("fc", "adapointr_keys.txt"), ("fold", "adapointr_fold_keys.txt")):
            with open(os.path.join(ROOT, "tests", "golden", fname), "w") as f:
                f.write(keys(decoder_type))
