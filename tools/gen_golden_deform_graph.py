"""Fixture of the reference's own deformable graph attention -> tests/golden/deform_graph.npz and deform_graph_keys.txt (build machine
only: needs the reference tree).

The reference classes (models/Transformer_utils.py improvedDeformableLocalGraphAttention and improvedDeformableLocalCrossAttention,
models/AdaPoinTr.py CrossAttnBlockApi) are imported through oracle/ref_shim.load() as they are and run on the cases of
tests/_deform_graph_case.py, in float32 and in float64 (module.double()), with the three_nn / three_interpolate stand-ins and the
tracing of tools/gen_golden_deform_attn.py (imported, not copied).  Stored -- arrays only; the tests regenerate the inputs from the seeds:
    {a,b,c,d}_{f32,f64}    the output of each case, (2, 40, 128)
    seed_{a,b,c,d}
deform_graph_keys.txt lists the state-dict keys of the modules of a, c and d with their shapes (`<case> <key> <shape ...>`): names only.

The seed conditions are those of the deformable cross-attention fixture: per case the seeds are scanned upward from 0 for the first at
which  (a) every k-nearest search has its k-th and (k+1)-th squared distance (float64) at least 1e-5 of that search's largest squared
distance apart,  (b) every three-nearest search likewise between its 3rd and 4th, and  (c) the f32 index sets of every search equal the
float64 sets.

    python tools/gen_golden_deform_graph.py [--check-only]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import gen_golden_deform_attn as base  # noqa: E402  (run() looks its case module up by name: it is given this fixture's below)

SEEDS, GAP = {"a": 0, "b": 0, "c": 2, "d": 0}, base.GAP


def _with_cases(fn, *args):
    """fn of the deformable cross-attention generator on THIS fixture's cases: it imports `_deform_attn_case` by name when called"""
    import _deform_graph_case as case
    saved = sys.modules.get("_deform_attn_case")
    sys.modules["_deform_attn_case"] = case
    try:
        return fn(*args)
    finally:
        if saved is None:
            del sys.modules["_deform_attn_case"]
        else:
            sys.modules["_deform_attn_case"] = saved


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    import _deform_graph_case as case
    stored = {}
    for name in case.CASES:
        first = None
        for seed in range(64):
            out, gaps, same = _with_cases(base.run, name, seed)
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
        path = os.path.join(ROOT, "tests", "golden", "deform_graph.npz")
        np.savez_compressed(path, **stored)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
        with open(os.path.join(ROOT, "tests", "golden", "deform_graph_keys.txt"), "w") as f:
            f.write(_with_cases(base.keys))
