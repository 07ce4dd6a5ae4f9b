"""Fixture of the reference's own AdaPoinTr blocks and stacks -> tests/golden/adapointr_blocks.npz and adapointr_blocks_keys.txt (build
machine only: needs the reference tree).

The reference classes (models/AdaPoinTr.py:15-507 with models/Transformer_utils.py under them) are imported through oracle/ref_shim.load()
as they are and run on the cases of tests/_adapointr_case.py (dim 128, 2 heads, k = 8, B = 2, eval mode, weights from
tests/_seeded.fill), in float32 and in float64 (module.double()).  Stored -- arrays only; the tests regenerate the inputs from the seed:
    {a,b,c,d}_{f32,f64}    the output of each case: (2, 40, 128), for c (2, 24, 128)
    seed
adapointr_blocks_keys.txt lists the state-dict keys of the modules of a, c and d with their shapes (`<case> <key> <shape ...>`): names only.

The reference takes topk(sorted=False) of the expanded squared distance for its neighbour searches; this repository's set is upp_knn's.
The fixture is only meaningful where both pick the same sets whatever the rounding, so for every search of every case the generator
requires  (a) the smallest gap between the k-th and (k+1)-th squared distance (float64) to be at least 1e-5 of that search's largest
squared distance and  (b) the f32 topk sets to equal the float64 sets.  Seeds are scanned upward from 0 and the first that passes is the
one stored.

    python tools/gen_golden_adapointr_blocks.py [--check-only]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

SEED, GAP = 0, 1e-5


def reference():
    import ref_shim
    ref_shim.load()
    return importlib.import_module("models.AdaPoinTr"), importlib.import_module("models.Transformer_utils")


def run(seed):
    """-> (arrays, smallest relative k-th/(k+1)-th gap per case, sets equal in f32 and f64?)"""
    import _adapointr_case as case
    ref, tu = reference()
    knn_point = tu.knn_point
    out, gaps, same = {"seed": np.int64(seed)}, {}, True
    x = case.inputs(seed)
    for name in case.CASES:
        sets = {}
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            m = case.module(ref, name).to(dtype)
            searches = []

            def traced(nsample, xyz, new_xyz):
                idx = knn_point(nsample, xyz, new_xyz)
                searches.append((xyz.detach().double(), new_xyz.detach().double(), idx.detach().clone()))
                return idx

            tu.knn_point = ref.knn_point = traced            # (models/AdaPoinTr.py holds its own name: `from ... import *`)
            try:
                with torch.no_grad():
                    y = case.run(m, name, *(t.to(dtype) for t in x))
            finally:
                tu.knn_point = ref.knn_point = knn_point
            assert searches and y.shape == (case.B, case.NK if name == "c" else case.NQ, case.DIM)
            out["%s_%s" % (name, prec)] = y.numpy()
            sets[prec] = [np.sort(idx.numpy(), axis=-1) for _, _, idx in searches]
            if prec == "f64":
                rel = []
                for xyz, new_xyz, _ in searches:
                    d = ((new_xyz.unsqueeze(2) - xyz.unsqueeze(1)) ** 2).sum(-1).sort(dim=-1)[0]
                    rel.append(float((d[..., case.K] - d[..., case.K - 1]).min() / d.max()))
                gaps[name] = min(rel)
        same = same and len(sets["f32"]) == len(sets["f64"]) and all(np.array_equal(a, b) for a, b in zip(sets["f32"], sets["f64"]))
    return out, gaps, same


def keys():
    import _adapointr_case as case
    ref, _ = reference()
    return "".join("%s %s %s\n" % (name, k, " ".join(str(s) for s in v.shape))
                   for name in ("a", "c", "d") for k, v in case.module(ref, name).state_dict().items())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    first = None
    for seed in range(64):
        out, gaps, same = run(seed)
        ok = same and min(gaps.values()) >= GAP
        print("seed %d: smallest relative gap %s; f32 sets %s the f64 sets -> %s"
              % (seed, ", ".join("%s %.2e" % kv for kv in gaps.items()), "equal" if same else "DIFFER FROM", "passes" if ok else "fails"))
        if ok:
            first = seed
            break
    assert first == SEED, "the first seed that passes is %s, the fixture's is %d" % (first, SEED)
    for name in out:
        if name.endswith("_f64"):
            r64 = out[name]
            print("%s: reference f32 against f64 = %.2e of the maximum (max %.3f)"
                  % (name[0], np.abs(out[name[0] + "_f32"] - r64).max() / np.abs(r64).max(), np.abs(r64).max()))
    if not a.check_only:
        path = os.path.join(ROOT, "tests", "golden", "adapointr_blocks.npz")
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
        with open(os.path.join(ROOT, "tests", "golden", "adapointr_blocks_keys.txt"), "w") as f:
            f.write(keys())
