"""The bits of the streaming attention family (csrc/attn_stream.hip: self-attention beyond 160 tokens, cross-attention, prefix-visibility
attention) against tests/golden/attn_stream_family_bits.npz.

The nine kernels are instantiations of three bodies, so the tests that compare one family with another bit for bit
(test_equal_lengths_give_the_bits_of_the_self_attention_kernels, test_split_q_zero_and_split_k_at_lk_give_the_bits_of_the_unmasked_kernels)
cannot see a change of summation order made in a body, and the float64 parity tests pass one.  This file pins every output -- ctx, lse
and d_qkv or d_q, d_k, d_v -- of the five cases of tests/_attn_family_case.py to what the kernels of commit 2d01369 computed, when the
three families were three sets of kernels in files of their own.  The inputs are a closed form (no fixture, no random-number library);
arrays are compared as int32, so -0.0 and NaN patterns count.

The fixture is regenerated with
    python tools/gen_golden_attn_family_bits.py
on an MI355X in a worktree of commit 2d01369 (with that tool and tests/_attn_family_case.py copied in), never from the tree under test.
That is legitimate only after a toolchain change that moves logf or the division of the forward's last step, and only from the same
source: a change of the kernels that moves these bits is a change of the summation order and needs its own argument.

Mutants, built from scratch copies and run once each (never committed): (1) the dQ kernel adding its two key-half accumulators the other
way round (the kh = 0 waves park theirs in the LDS and the kh = 1 waves add and store) passes this file, as it must: IEEE addition of two
finite numbers is commutative, so acc_1 + acc_0 has the bits of acc_0 + acc_1 whatever the inputs are, and no input pattern can tell the
two apart.  (2) The order change that does move bits -- the dQ kernel walking its key blocks in descending order -- fails this file at
the four cases with more than one key block (self_161, cross_70x130, prefix_130_66, prefix_96_32: d_q or the q third of d_qkv) and
passes cross_65x63, whose walk is one block; both mutants pass every float64 parity test of tests/test_gpu_cross_attention.py."""
import os

import numpy as np
import pytest
import torch

import _attn_family_case as case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_stream_family_bits.npz")


@pytest.mark.parametrize("name", list(case.CASES))
def test_every_output_carries_the_bits_of_the_separate_kernel_sets(name):
    want = np.load(GOLDEN)
    got = case.run(name)
    assert sorted(k for k in want.files if k.startswith(name + "__")) == sorted("%s__%s" % (name, a) for a in got)
    for arr, t in got.items():
        g, w = t.cpu().numpy(), want["%s__%s" % (name, arr)]
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, (name, arr, g.dtype, g.shape, w.dtype, w.shape)
        diff = np.flatnonzero(g.view(np.int32).ravel() != w.view(np.int32).ravel())
        if diff.size:
            i = np.unravel_index(diff[0], g.shape)
            pytest.fail("%s %s: %d of %d elements differ, the first at %s: got %r (0x%08x), the fixture holds %r (0x%08x)"
                        % (name, arr, diff.size, g.size, tuple(int(x) for x in i), float(g[i]), g.view(np.uint32)[i], float(w[i]), w.view(np.uint32)[i]))
