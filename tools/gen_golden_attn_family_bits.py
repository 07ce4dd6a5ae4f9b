"""Fixture of the streaming attention family's bits -> tests/golden/attn_stream_family_bits.npz (needs an MI355X).

Runs the cases of tests/_attn_family_case.py through ops.attn_fwd / attn_bwd, ops.xattn_fwd / xattn_bwd and ops.xattn_prefix_fwd /
xattn_prefix_bwd of the library that is built in this tree and stores the outputs only, as float32 arrays named `<case>__<array>` (ctx,
lse and d_qkv or d_q, d_k, d_v); the inputs are a closed form that the test computes again.  The fixture pins the kernels of one commit:
run this in a worktree of THAT commit (with this file and tests/_attn_family_case.py copied in), never on the tree under test.
tests/test_gpu_attention_family_bits.py says which commit and when regenerating is legitimate.

    python tools/gen_golden_attn_family_bits.py [--out tests/golden/attn_stream_family_bits.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "iccv2025-upp_amd")]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attn_stream_family_bits.npz"))
    a = ap.parse_args()
    import torch
    import _attn_family_case as case
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the fixture is what the kernels compute")
    out = {}
    for name in case.CASES:
        first, again = case.run(name), case.run(name)
        for arr, t in first.items():
            assert t.dtype == torch.float32 and torch.equal(t.view(torch.int32), again[arr].view(torch.int32)), (name, arr, "two runs differ")
            out["%s__%s" % (name, arr)] = t.cpu().numpy()
            print("%s %s %s max|x| %.4g" % (name, arr, tuple(t.shape), t.abs().max().item()))
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))
