"""Fixture of the reference's own PoinTr -> tests/golden/pointr.npz and tests/golden/pointr_keys.txt (build machine only: needs the
reference tree).

The reference class (models/PoinTr.py, with models/Transformer.py and models/dgcnn_group.py under it) is imported through
oracle/ref_shim.load() as it is.  Its Fold.__init__ calls .cuda() on the folding seed, so this process -- and only this process -- makes
torch.Tensor.cuda the identity before the model is constructed; the class then builds and runs on the CPU.  Configuration:
trans_dim = 384, knn_layer = 1, num_pred = 512, num_query = 32 (S = 16; depth [6, 8] and 6 heads are fixed by the class), weights from
tests/_seeded.fill, input unit_ball_clouds(2, 640, seed).  The model runs in eval and in train mode, in float32 and in float64
(model.double()).  Stored -- arrays only; the tests regenerate the inputs from the seed:
    {eval,train}_coarse_{f32,f64}    (2, 64, 3)      the coarse cloud (32 predicted + 32 FPS points of the input)
    {eval,train}_rebuild_{f32,f64}   (2, 1152, 3)    the rebuilt cloud (512 folded points + the input)
    train_loss_{f32,f64}             (2,)            get_loss(ret, input) of the train-mode run: (coarse, fine) Chamfer-L1
    seed
pointr_keys.txt lists the reference model's state-dict keys with their shapes: names only.

The reference takes topk(sorted=False) of the expanded squared distance for its three 8-neighbour searches; this repository's set is
upp_knn's.  The fixture is only meaningful where both pick the same sets whatever the rounding, so for every search, in both modes,
the generator requires  (a) the smallest gap between the 8th and 9th squared distance (float64) to be at least 1e-5 of that search's
largest squared distance and  (b) the f32 topk sets to equal the float64 sets.  Seeds are scanned upward from 0 and the first that
passes is the one stored (4).

    python tools/gen_golden_pointr.py [--check-only]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

CONFIG = dict(NAME="PoinTr", trans_dim=384, knn_layer=1, num_pred=512, num_query=32)
SEED, GAP = 4, 1e-5


def reference():
    import ref_shim
    ns = ref_shim.load()
    torch.Tensor.cuda = lambda self, *a, **k: self                  # Fold.__init__: .cuda() on the folding seed
    return ns, importlib.import_module("models.PoinTr"), importlib.import_module("models.Transformer")


def run(seed):
    """-> (arrays, smallest relative 8th/9th gap per mode, sets equal in f32 and f64?)"""
    import _seeded
    ns, ref, tr = reference()
    x = _seeded.unit_ball_clouds(2, 640, seed=seed)
    out, gaps, same = {"seed": np.int64(seed)}, {}, True
    knn_point = tr.knn_point
    for mode in ("eval", "train"):
        sets = {}
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            model = _seeded.fill(ref.PoinTr(ns.EasyDict(CONFIG))).to(dtype).train(mode == "train")
            searches = []

            def traced(nsample, xyz, new_xyz):
                idx = knn_point(nsample, xyz, new_xyz)
                searches.append((xyz.detach().double(), new_xyz.detach().double(), idx.detach().clone()))
                return idx

            tr.knn_point = traced
            try:
                with torch.no_grad():
                    ret = model(x.to(dtype))
                    losses = model.get_loss(ret, x.to(dtype)) if mode == "train" and prec == "f64" else None
                    if mode == "train" and prec == "f32":
                        losses = model.get_loss(ret, x)
            finally:
                tr.knn_point = knn_point
            assert len(searches) == 3 and ret[0].shape == (2, 64, 3) and ret[1].shape == (2, 1152, 3)
            out["%s_coarse_%s" % (mode, prec)] = ret[0].numpy()
            out["%s_rebuild_%s" % (mode, prec)] = ret[1].numpy()
            if losses is not None:
                out["train_loss_%s" % prec] = np.array([float(v) for v in losses], dtype=np.float64 if prec == "f64" else np.float32)
            sets[prec] = [np.sort(idx.numpy(), axis=-1) for _, _, idx in searches]
            if prec == "f64":
                rel = []
                for xyz, new_xyz, _ in searches:
                    d = ((new_xyz.unsqueeze(2) - xyz.unsqueeze(1)) ** 2).sum(-1).sort(dim=-1)[0]
                    rel.append(float((d[..., 8] - d[..., 7]).min() / d.max()))
                gaps[mode] = min(rel)
        same = same and all(np.array_equal(a, b) for a, b in zip(sets["f32"], sets["f64"]))
    return out, gaps, same


def keys():
    ns, ref, _ = reference()
    model = ref.PoinTr(ns.EasyDict(CONFIG))
    return "".join("%s %s\n" % (k, " ".join(str(s) for s in v.shape)) for k, v in model.state_dict().items())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    first = None
    for seed in range(SEED + 1):
        out, gaps, same = run(seed)
        ok = same and min(gaps.values()) >= GAP
        print("seed %d: smallest relative 8th/9th gap eval %.2e, train %.2e; f32 sets %s the f64 sets -> %s"
              % (seed, gaps["eval"], gaps["train"], "equal" if same else "DIFFER FROM", "passes" if ok else "fails"))
        if ok:
            first = seed
            break
    assert first == SEED, "the first seed that passes is %s, the fixture's is %d" % (first, SEED)
    for mode in ("eval", "train"):
        for name in ("coarse", "rebuild"):
            r64 = out["%s_%s_f64" % (mode, name)]
            print("%s %s: reference f32 against f64 = %.2e of the maximum"
                  % (mode, name, np.abs(out["%s_%s_f32" % (mode, name)] - r64).max() / np.abs(r64).max()))
    print("train losses f32 %s, f64 %s" % (out["train_loss_f32"], out["train_loss_f64"]))
    if not a.check_only:
        path = os.path.join(ROOT, "tests", "golden", "pointr.npz")
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
        with open(os.path.join(ROOT, "tests", "golden", "pointr_keys.txt"), "w") as f:
            f.write(keys())
