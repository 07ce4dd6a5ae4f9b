"""The cases of tests/golden/rw_deform.npz, shared by their generator (tools/gen_golden_rw_deform.py: the reference's own classes) and by
the tests of this repository's classes.  dim 128, 2 heads (head_dim 64), n_group 2, k = 8, qkv_bias=True, B = 2, eval mode, weights from
tests/_seeded.fill, inputs the 40 query tokens and positions of _adapointr_case.inputs(seed), one seed per case:
    a   DeformableLocalAttention, 40 tokens
    b   one SelfAttnBlockApi, 'attn-rw_deform' with concat
    c   the same with onebyone
    d   RegionWiseBlock (its module keeps the default k = 10)
`models` is the module that holds SelfAttnBlockApi (the reference's models.AdaPoinTr or ours) and `utils` the one that holds the
deformable classes (models.Transformer_utils); `ours` adds this repository's opt-in keyword."""
import _adapointr_case as blocks

DIM, HEADS, GROUPS, K, B, N = blocks.DIM, blocks.HEADS, 2, blocks.K, blocks.B, blocks.NQ
CASES = ("a", "b", "c", "d")
bound, check_output = blocks.bound, blocks.check_output


def inputs(seed):
    """-> x (B,N,DIM), pos (B,N,3), f32 CPU"""
    q, _, q_pos, _ = blocks.inputs(seed)
    return q, q_pos


def module(models, utils, case, ours=True):
    """the seeded eval-mode module of a case"""
    import _seeded
    if case == "a":
        m = utils.DeformableLocalAttention(DIM, num_heads=HEADS, qkv_bias=True, k=K, n_group=GROUPS)
    elif case in ("b", "c"):
        extra = dict(region_wise=True) if ours else {}
        m = models.SelfAttnBlockApi(DIM, HEADS, qkv_bias=True, block_style='attn-rw_deform',
                                    combine_style='concat' if case == "b" else 'onebyone', k=K, n_group=GROUPS, **extra)
    else:
        m = utils.RegionWiseBlock(DIM, HEADS, qkv_bias=True)
    return _seeded.fill(m).eval()


def run(m, case, x, pos):
    return m(x, pos)
