"""Fixture of the reference's own DGCNN_Grouper -> tests/golden/dgcnn_grouper.npz (build machine only: needs the reference tree).

The reference class (models/dgcnn_group.py) is imported through oracle/ref_shim.load() as it is, filled with tests/_seeded.fill and run on
unit_ball_clouds(2, 640, seed=0).  Stored: coor (2,3,128), f (2,128,128) and the layer-1 output (2,32,640) -- arrays only; the inputs are
regenerated from the seed by the tests.

The reference takes topk(sorted=False) of the expanded squared distance; this repository's neighbour set is upp_knn's.  The fixture is
only meaningful where both pick the same sets, so the generator asserts, over the four neighbour searches of the run, that the smallest
gap between the 16th and 17th reference distance exceeds 1e-6 and that the oracle's (= the library's) neighbour sets equal the
reference's.

    python tools/gen_golden_dgcnn.py [--seed 0] [--check-only]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def run(seed):
    import ref_shim
    import _seeded
    ref_shim.load()
    import importlib
    import oracle as O
    ref = importlib.import_module("models.dgcnn_group")
    model = _seeded.fill(ref.DGCNN_Grouper()).eval()
    searches = []
    knn_point = ref.knn_point

    def traced(nsample, xyz, new_xyz):
        idx = knn_point(nsample, xyz, new_xyz)
        searches.append((xyz.detach().clone(), new_xyz.detach().clone(), idx.detach().clone()))
        return idx

    ref.knn_point = traced
    kept = {}
    hook = model.layer1.register_forward_hook(lambda m, i, o: kept.__setitem__("l1", o.max(dim=-1)[0].detach()))
    x = _seeded.unit_ball_clouds(2, 640, seed=seed)
    try:
        with torch.no_grad():
            coor, f = model(x.transpose(1, 2).contiguous())
    finally:
        hook.remove()
        ref.knn_point = knn_point
    assert len(searches) == 4
    gaps = []
    for xyz, new_xyz, idx in searches:
        d = ref.square_distance(new_xyz, xyz).sort(dim=-1)[0]
        gaps.append(float((d[..., 16] - d[..., 15]).min()))
        _, want = O.knn(xyz.numpy(), new_xyz.numpy(), 16, want_dist=False)
        same = np.array_equal(np.sort(want, axis=-1), np.sort(idx.numpy(), axis=-1))
        assert same, "the oracle's neighbour sets differ from the reference's (seed %d)" % seed
    assert min(gaps) > 1e-6, gaps
    return {"coor": coor.numpy(), "f": f.numpy(), "l1": kept["l1"].numpy()}, gaps


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    out, gaps = run(a.seed)
    print("seed %d: 16th/17th distance gaps %s; neighbour sets identical" % (a.seed, ", ".join("%.2e" % g for g in gaps)))
    if not a.check_only:
        path = os.path.join(ROOT, "tests", "golden", "dgcnn_grouper.npz")
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
