"""Fixture of the reference's own CrossAttention and DecoderBlock -> tests/golden/decoder_block.npz (build machine only: needs the
reference tree).

The reference classes (models/Transformer.py:120-219) are imported through oracle/ref_shim.load() as they are, at dim = 128,
num_heads = 2, in eval mode, filled with tests/_seeded.fill, and run on the inputs of tests/_decoder_block_case.inputs (B = 2, 40 queries
over 24 proxies, random neighbour lists from the same seeded generator).  The per-sample (B, Nq, 8) lists are converted here to the
reference's flat bs*k*np form with batch offsets (get_knn_index).  Stored -- arrays only; the tests regenerate the inputs from the seed:
    xattn   the CrossAttention output (2, 40, 128)
    plain   the DecoderBlock output without indices
    knn     the DecoderBlock output with both index lists

    python tools/gen_golden_decoder_block.py [--seed 0] [--check-only]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def flat_index(idx, rows):
    """(B, Nq, k) per-sample lists over `rows` key rows -> the reference's (B * k * Nq,) absolute rows, ordered (sample, k, query)"""
    B = idx.shape[0]
    return (idx.long().transpose(1, 2) + torch.arange(B).view(B, 1, 1) * rows).reshape(-1)


def run(seed):
    import ref_shim
    import _seeded
    import _decoder_block_case as case
    ref_shim.load()
    import importlib
    ref = importlib.import_module("models.Transformer")
    q, v, self_idx, cross_idx = case.inputs(seed)
    xattn = _seeded.fill(ref.CrossAttention(case.DIM, case.DIM, num_heads=case.HEADS)).eval()
    block = _seeded.fill(ref.DecoderBlock(case.DIM, case.HEADS)).eval()
    with torch.no_grad():
        out = {"xattn": xattn(q, v), "plain": block(q, v),
               "knn": block(q, v, flat_index(self_idx, case.NQ), flat_index(cross_idx, case.NK))}
    return {k: t.numpy() for k, t in out.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    out = run(a.seed)
    print("seed %d: %s" % (a.seed, ", ".join("%s %s max %.3f" % (k, v.shape, np.abs(v).max()) for k, v in out.items())))
    if not a.check_only:
        path = os.path.join(ROOT, "tests", "golden", "decoder_block.npz")
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
