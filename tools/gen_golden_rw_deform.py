"""Fixture of the reference's own region-wise deformable attention -> tests/golden/rw_deform.npz and rw_deform_keys.txt (build machine
only: needs the reference tree).

The reference classes (models/Transformer_utils.py DeformableLocalAttention and RegionWiseBlock, models/AdaPoinTr.py SelfAttnBlockApi)
are imported through oracle/ref_shim.load() as they are and run on the cases of tests/_rw_deform_case.py, in float32 and in float64
(module.double()).  The stand-ins for pointnet2_utils.three_nn / three_interpolate and the way the searches are traced are those of
tools/gen_golden_deform_attn.py, imported from there.  Stored -- arrays only; the tests regenerate the inputs from the seeds:
    {a,b,c,d}_{f32,f64}    the output of each case, (2, 40, 128)
    seed_{a,b,c,d}
rw_deform_keys.txt lists the state-dict keys of the modules of a, b, c and d with their shapes (`<case> <key> <shape ...>`): names only.

Per case the seeds are scanned upward from 0 for the first at which  (a) every k-nearest search has its k-th and (k+1)-th squared
distance (float64) at least 1e-5 of that search's largest squared distance apart,  (b) every three-nearest search likewise between its
3rd and 4th, and  (c) the f32 index sets of every search equal the float64 sets.

    python tools/gen_golden_rw_deform.py [--check-only]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from gen_golden_deform_attn import GAP, reference, three_interpolate, three_nn  # noqa: E402

SEEDS = {"a": 7, "b": 3, "c": 4, "d": 10}


def run(name, seed):
    """-> (arrays, smallest relative gap of the k-nearest and of the three-nearest searches, sets equal in f32 and f64?)"""
    import _rw_deform_case as case
    ref, tu = reference()
    knn_point, p2u = tu.knn_point, tu.pointnet2_utils
    out, sets, gaps = {}, {}, {}
    x = case.inputs(seed)
    for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        m = case.module(ref, tu, name, ours=False).to(dtype)
        knns, threes = [], []

        def traced_knn(nsample, xyz, new_xyz):
            idx = knn_point(nsample, xyz, new_xyz)
            knns.append((xyz.detach().double(), new_xyz.detach().double(), idx.detach().clone()))
            return idx

        def traced_three(unknown, known):
            dist, idx = three_nn(unknown, known)
            threes.append((known.detach().double(), unknown.detach().double(), idx.clone(), float(dist[..., 0].min())))
            return dist, idx

        tu.knn_point = ref.knn_point = traced_knn                # (models/AdaPoinTr.py holds its own name: `from ... import *`)
        p2u.three_nn, p2u.three_interpolate = traced_three, three_interpolate
        try:
            with torch.no_grad():
                y = case.run(m, name, *(t.to(dtype) for t in x))
        finally:
            tu.knn_point = ref.knn_point = knn_point
            del p2u.three_nn, p2u.three_interpolate
        assert knns and threes and y.shape == (case.B, case.N, case.DIM)
        out["%s_%s" % (name, prec)] = y.numpy()
        sets[prec] = [np.sort(s[2].numpy(), axis=-1) for s in knns + threes]
        if prec == "f64":
            for kind, searches in (("knn", knns), ("three", threes)):
                rel = []
                for s in searches:
                    xyz, new_xyz, idx = s[:3]
                    n = idx.shape[-1]
                    d = ((new_xyz.unsqueeze(2) - xyz.unsqueeze(1)) ** 2).sum(-1).sort(dim=-1)[0]
                    rel.append(float((d[..., n] - d[..., n - 1]).min() / d.max()))
                gaps[kind] = min(rel)
            gaps["first"] = min(s[3] for s in threes)
    same = len(sets["f32"]) == len(sets["f64"]) and all(np.array_equal(a, b) for a, b in zip(sets["f32"], sets["f64"]))
    return out, gaps, same


def keys():
    import _rw_deform_case as case
    ref, tu = reference()
    return "".join("%s %s %s\n" % (name, k, " ".join(str(s) for s in v.shape))
                   for name in case.CASES for k, v in case.module(ref, tu, name, ours=False).state_dict().items())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    import _rw_deform_case as case
    stored = {}
    for name in case.CASES:
        first = None
        for seed in range(64):
            out, gaps, same = run(name, seed)
            ok = same and gaps["knn"] >= GAP and gaps["three"] >= GAP
            print("case %s seed %d: smallest relative gap k-nearest %.2e, three-nearest %.2e; smallest first distance %.2e; f32 sets %s the "
                  "f64 sets -> %s" % (name, seed, gaps["knn"], gaps["three"], gaps["first"], "equal" if same else "DIFFER FROM",
                                      "passes" if ok else "fails"))
            if ok:
                first = seed
                break
        assert first == SEEDS[name], "case %s: the first seed that passes is %s, the fixture's is %d" % (name, first, SEEDS[name])
        r64 = out[name + "_f64"]
        print("case %s: reference f32 against f64 = %.2e of the maximum (max %.3f)"
              % (name, np.abs(out[name + "_f32"] - r64).max() / np.abs(r64).max(), np.abs(r64).max()))
        stored.update(out)
        stored["seed_" + name] = np.int64(first)
    if not a.check_only:
        path = os.path.join(ROOT, "tests", "golden", "rw_deform.npz")
        np.savez_compressed(path, **stored)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
        with open(os.path.join(ROOT, "tests", "golden", "rw_deform_keys.txt"), "w") as f:
            f.write(keys())
