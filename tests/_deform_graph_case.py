"""The cases of tests/golden/deform_graph.npz, shared by their generator (tools/gen_golden_deform_graph.py: the reference's own classes)
and by the tests of this repository's classes.  dim 128, 2 heads (head_dim 64), n_group 2, k = 8, qkv_bias=True, B = 2, eval mode,
weights from tests/_seeded.fill, inputs from _adapointr_case.inputs(seed) (40 queries, 24 memory tokens), one seed per case:
    a   improvedDeformableLocalGraphAttention, the cross form: 40 queries over 24 memory tokens
    b   the same module, the self form on the 40 queries with denoise_length = 8
    c   one CrossAttnBlockApi, 'attn-deform_graph' with concat on both sides, denoise_length = 8
    d   improvedDeformableLocalCrossAttention, the cross form
`models` is the module that holds CrossAttnBlockApi (the reference's models.AdaPoinTr or ours) and `utils` the one that holds the
deformable classes (models.Transformer_utils); `ours` adds this repository's opt-in keyword."""
import _adapointr_case as blocks

DIM, HEADS, GROUPS, K, B, NQ, NK, D = blocks.DIM, blocks.HEADS, 2, blocks.K, blocks.B, blocks.NQ, blocks.NK, blocks.D
CASES = ("a", "b", "c", "d")
inputs, bound, check_output = blocks.inputs, blocks.bound, blocks.check_output


def module(models, utils, case, ours=True):
    """the seeded eval-mode module of a case"""
    import _seeded
    if case in ("a", "b"):
        m = utils.improvedDeformableLocalGraphAttention(DIM, k=K)
    elif case == "c":
        extra = dict(deformable=('deform', 'deform_graph')) if ours else {}
        m = models.CrossAttnBlockApi(DIM, HEADS, qkv_bias=True, self_attn_block_style='attn-deform_graph', self_attn_combine_style='concat',
                                     cross_attn_block_style='attn-deform_graph', cross_attn_combine_style='concat', k=K, n_group=GROUPS,
                                     **extra)
    else:
        m = utils.improvedDeformableLocalCrossAttention(DIM, num_heads=HEADS, qkv_bias=True, k=K, n_group=GROUPS)
    return _seeded.fill(m).eval()


def run(m, case, q, v, q_pos, v_pos):
    if case in ("a", "d"):
        return m(q, q_pos, v=v, v_pos=v_pos)
    if case == "b":
        return m(q, q_pos, denoise_length=D)
    return m(q, v, q_pos, v_pos, denoise_length=D)
