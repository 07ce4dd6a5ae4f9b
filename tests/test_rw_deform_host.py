"""The region-wise deformable attention (block token `rw_deform`) on a GPU-less host: the torch formulation
(upp_hip.torch_cpu.region_attention) in float64 against a literal transcription of the reference's forward (interpolate, project over
B N k rows, gather the query rows, a k x k attention per (b, head, n), max over the rows), the modules' state-dict schema, the fixture
cases of tests/golden/rw_deform.npz (tools/gen_golden_rw_deform.py: the reference's own classes) on the CPU formulation, the opt-in
wiring into models.AdaPoinTr, which parameters get a gradient, and the argument checks of the C entry points, which happen before any
launch.

Fixture bound: max(1e-5, 3 x err_ref) of each output's float64 maximum, err_ref the reference's own f32-against-f64 error computed here
from the stored pair (a 6.9e-7, b 4.5e-7, c 3.2e-7, d 3.4e-7: the bound is 1e-5 for all four)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _rw_deform_case as case
from conftest import GOLDEN
from upp_hip import _abi, functional as HF, ops, torch_cpu

BADARG, RANGE = -1, -2
P = ctypes.c_void_p(64)            # non-NULL, 16-byte aligned, never dereferenced
OFFSET_BRANCH = ("proj_v_off.", "linear_offset.")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "rw_deform.npz"))


@pytest.fixture()
def cpu_formulations():
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    yield
    torch_cpu.enable(was)


# ---- the formulation against the reference's own order of operations, float64 -----------------------------------------------------------
@pytest.mark.parametrize("B, N, NK, k, H, G", [(1, 1, 1, 1, 1, 1), (2, 5, 7, 3, 2, 1), (2, 9, 6, 4, 4, 2), (1, 3, 4, 10, 4, 4)])
@pytest.mark.parametrize("bias", [True, False])
def test_formulation_equals_the_materialising_form(B, N, NK, k, H, G, bias):
    g = torch.Generator().manual_seed(B * 100 + N + 11)
    hd = 8
    C = hd * H
    c = C // G
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    qp, v, Wk, Wv = rnd(B, N, C), rnd(B, NK, C), rnd(C, C), rnd(C, C)
    bk, bv = (rnd(C), rnd(C)) if bias else (None, None)
    idx = torch.randint(0, N, (B, N, k), generator=g)
    idx3 = torch.randint(0, NK, (B, G, N * k, 3), generator=g).int()
    w3 = torch.rand(B, G, N * k, 3, generator=g, dtype=torch.float64)
    w3 = w3 / w3.sum(-1, keepdim=True)
    scale = hd ** -0.5
    # the reference (models/Transformer_utils.py:224-258): three_interpolate per group, regroup to (B,N,k,C), index_points(q, idx), proj_k /
    # proj_v over B N k rows, '(b h n) k c' attention with a (BHN, k, k) score tensor, rearranged back, max over dim 2
    vg = v.view(B, NK, G, c).permute(0, 2, 1, 3)
    near = torch.gather(vg, 2, idx3.long().reshape(B, G, N * k * 3, 1).expand(-1, -1, -1, c)).view(B, G, N * k, 3, c)
    interp = (near * w3.unsqueeze(-1)).sum(3).view(B, G, N, k, c).permute(0, 2, 3, 1, 4).reshape(B, N, k, C)
    local_q = torch.gather(qp, 1, idx.reshape(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, C)
    heads = lambda t: t.view(B, N, k, H, hd).permute(0, 3, 1, 2, 4).reshape(B * H * N, k, hd)
    q_, k_, v_ = heads(local_q), heads(F.linear(interp, Wk, bk)), heads(F.linear(interp, Wv, bv))
    attn = torch.einsum('bmc,bnc->bmn', q_, k_).mul(scale).softmax(dim=-1)
    out = torch.einsum('bmn,bnc->bmc', attn, v_).view(B, H, N, k, hd).permute(0, 2, 3, 1, 4).reshape(B, N, k, C)
    want = out.max(dim=2)[0]
    PK = torch.stack([vg[:, i] @ Wk[:, i * c:(i + 1) * c].t() for i in range(G)], 1)
    PV = torch.stack([vg[:, i] @ Wv[:, i * c:(i + 1) * c].t() for i in range(G)], 1)
    got = torch_cpu.region_attention(qp, idx, PK, PV, bk, bv, idx3, w3, H, scale)
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-12 * want.abs().max()


def test_formulation_treats_indices_outside_their_range_as_absent():
    g = torch.Generator().manual_seed(5)
    B, N, NK, k, H, G, C = 1, 4, 5, 3, 2, 1, 16
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    qp, PK, PV = rnd(B, N, C).requires_grad_(), rnd(B, G, NK, C).requires_grad_(), rnd(B, G, NK, C)
    idx = torch.randint(0, N, (B, N, k), generator=g)
    idx3 = torch.randint(0, NK, (B, G, N * k, 3), generator=g).int()
    w3 = torch.rand(B, G, N * k, 3, generator=g, dtype=torch.float64)
    idx[0, 1, 2], idx3[0, 0, 4, 1] = N, -1
    got = torch_cpu.region_attention(qp, idx, PK, PV, None, None, idx3, w3, H, 0.3)
    # the same with the absent entries spelled out: a zero query row appended, a zero weight
    q0 = torch.cat([qp, qp.new_zeros(B, 1, C)], 1)
    w0, i0 = w3.clone(), idx3.clone()
    w0[0, 0, 4, 1], i0[0, 0, 4, 1] = 0.0, 0
    Q = torch.gather(q0, 1, idx.reshape(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, H, C // H)
    rows = lambda Pm: (torch.gather(Pm, 2, i0.long().reshape(B, G, -1, 1).expand(-1, -1, -1, C)).view(B, G, N * k, 3, C)
                       * w0.unsqueeze(-1)).sum(3).sum(1).view(B, N, k, H, C // H)
    p = (torch.einsum('bnthc,bnshc->bnhts', Q, rows(PK)) * 0.3).softmax(-1)
    want = torch.einsum('bnhts,bnshc->bnthc', p, rows(PV)).reshape(B, N, k, C).max(2)[0]
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    got.sum().backward()
    assert torch.isfinite(qp.grad).all() and torch.isfinite(PK.grad).all()


# ---- the modules: schema, fixture, wiring, gradients ----------------------------------------------------------------------------------
def test_state_dict_schema_is_the_references_and_loads_strictly():
    from models import AdaPoinTr, Transformer_utils
    want = {}
    for line in open(os.path.join(GOLDEN, "rw_deform_keys.txt")):
        name, key, *shape = line.split()
        want.setdefault(name, {})[key] = tuple(int(s) for s in shape)
    assert set(want) == set(case.CASES) and len(want["a"]) == 15
    assert {"norm2.weight", "norm2.bias", "deformable_attn.proj_q.weight"} <= set(want["d"])
    for name in want:
        m = case.module(AdaPoinTr, Transformer_utils, name)
        sd = m.state_dict()
        assert {k: tuple(t.shape) for k, t in sd.items()} == want[name], name
        again = case.module(AdaPoinTr, Transformer_utils, name)
        again.load_state_dict({k: t.clone() + 1 for k, t in sd.items()}, strict=True)
        assert all(torch.equal(t, sd[k] + 1) for k, t in again.state_dict().items())


@pytest.mark.parametrize("name", case.CASES)
def test_fixture_cases_on_the_cpu_formulation(fixture, cpu_formulations, name):
    from models import AdaPoinTr, Transformer_utils
    m = case.module(AdaPoinTr, Transformer_utils, name)
    with torch.no_grad():
        y = case.run(m, name, *case.inputs(int(fixture["seed_" + name])))
    case.check_output(fixture, name, y, "torch formulation (CPU)")


def test_the_opt_in_builds_rw_deform_in_both_self_positions_only():
    from models import AdaPoinTr
    from models.Transformer_utils import DeformableLocalAttention as Region
    blk = AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-rw_deform', k=6, n_group=1, region_wise=True)
    assert isinstance(blk.local_attn, Region) and blk.local_attn.k == 6 and blk.local_attn.n_group == 1 and blk.attn is not None
    blk = AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='rw_deform', region_wise=True)
    assert isinstance(blk.local_attn, Region) and blk.attn is None
    blk = AdaPoinTr.CrossAttnBlockApi(128, 2, self_attn_block_style='attn-rw_deform', cross_attn_block_style='attn', k=7, region_wise=True)
    assert isinstance(blk.local_self_attn, Region) and blk.local_self_attn.k == 7 and blk.local_cross_attn is None
    enc = AdaPoinTr.PointTransformerEncoder(embed_dim=128, depth=2, num_heads=2, block_style_list=['attn-rw_deform', 'attn'], region_wise=True)
    assert isinstance(enc.blocks.blocks[0].local_attn, Region) and enc.blocks.blocks[1].local_attn is None
    dec = AdaPoinTr.PointTransformerDecoder(embed_dim=128, depth=1, num_heads=2, self_attn_block_style_list=['attn-rw_deform'],
                                            cross_attn_block_style_list=['attn-graph'], region_wise=True)
    assert isinstance(dec.blocks.blocks[0].local_self_attn, Region)
    for style in ('rw_deform', 'attn-rw_deform'):                                # never in the cross position
        with pytest.raises(ValueError, match="self-attention only"):
            AdaPoinTr.CrossAttnBlockApi(128, 2, self_attn_block_style='attn', cross_attn_block_style=style, region_wise=True)
    with pytest.raises(ValueError, match="'rw_deform'"):                         # the default still raises
        AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-rw_deform')
    with pytest.raises(ValueError, match="'rw_deform'"):                         # `deformable` does not opt it in
        AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-rw_deform', deformable=True)
    with pytest.raises(ValueError, match="'deform'"):                            # ... and region_wise opts nothing else in
        AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-deform', region_wise=True)
    with pytest.raises(ValueError, match="local token"):
        AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='graph-rw_deform', region_wise=True)


def test_the_decoder_self_position_serves_no_denoise_length(cpu_formulations):
    from models import AdaPoinTr
    import _adapointr_case as blocks
    q, v, q_pos, v_pos = blocks.inputs(1)
    for combine in ('concat', 'onebyone'):
        blk = AdaPoinTr.CrossAttnBlockApi(blocks.DIM, blocks.HEADS, self_attn_block_style='attn-rw_deform', self_attn_combine_style=combine,
                                          cross_attn_block_style='attn', k=blocks.K, region_wise=True).eval()
        with torch.no_grad():
            y = blk(q, v, q_pos, v_pos)
            assert y.shape == q.shape and torch.isfinite(y).all()
            with pytest.raises(ValueError, match="no denoising form"):
                blk(q, v, q_pos, v_pos, denoise_length=blocks.D)
    dec = AdaPoinTr.PointTransformerDecoder(embed_dim=blocks.DIM, depth=2, num_heads=blocks.HEADS, self_attn_block_style_list=['attn-rw_deform', 'attn'],
                                            cross_attn_block_style_list=['attn', 'attn'], k=blocks.K, region_wise=True).eval()
    with torch.no_grad():
        assert torch.isfinite(dec(q, v, q_pos, v_pos)).all()
        with pytest.raises(ValueError, match="no denoising form"):
            dec(q, v, q_pos, v_pos, denoise_length=blocks.D)


def test_the_stack_hands_one_list_to_the_module(cpu_formulations, monkeypatch):
    from models import AdaPoinTr
    x, pos = case.inputs(1)
    enc = AdaPoinTr.PointTransformerEncoder(embed_dim=case.DIM, depth=2, num_heads=case.HEADS, block_style_list=['attn-rw_deform', 'rw_deform'],
                                            k=case.K, region_wise=True).eval()
    calls = []
    real = AdaPoinTr.knn_point
    monkeypatch.setattr(AdaPoinTr, "knn_point", lambda *a: calls.append(1) or real(*a))
    from models import Transformer_utils
    monkeypatch.setattr(Transformer_utils, "knn_point", lambda *a: pytest.fail("the module searched for itself"))
    with torch.no_grad():
        assert torch.isfinite(enc(x, pos)).all()
    assert len(calls) == 1


def _cfg(region_wise):
    import _adapointr_model_case as mc
    from utils.config import EasyDict
    cfg = mc.config()
    cfg['encoder_config']['block_style_list'] = ['attn-rw_deform', 'attn']
    cfg['decoder_config']['self_attn_block_style_list'] = ['attn-rw_deform', 'attn']
    if region_wise is not None:
        cfg['region_wise'] = region_wise

    def wrap(d):
        return EasyDict({k: wrap(v) if isinstance(v, dict) else v for k, v in d.items()})
    return wrap(cfg)


def test_from_cfg_passes_the_opt_in_through():
    from models import AdaPoinTr
    from models.Transformer_utils import DeformableLocalAttention as Region
    model = AdaPoinTr.from_cfg(_cfg(True))
    enc, dec = model.base_model.encoder.blocks.blocks[0], model.base_model.decoder.blocks.blocks[0]
    assert isinstance(enc.local_attn, Region) and isinstance(dec.local_self_attn, Region)
    assert enc.local_attn.k == 8 and enc.local_attn.n_group == 2
    for region_wise in (None, False):
        with pytest.raises(ValueError, match="'rw_deform'"):
            AdaPoinTr.from_cfg(_cfg(region_wise))


def test_the_offset_branch_and_norm2_get_no_gradient_and_everything_else_does(cpu_formulations):
    from models import AdaPoinTr, Transformer_utils
    x, pos = (t.requires_grad_() for t in case.inputs(1))
    for name in case.CASES:
        m = case.module(AdaPoinTr, Transformer_utils, name)
        x.grad = pos.grad = None
        case.run(m, name, x, pos).square().sum().backward()
        for pname, prm in m.named_parameters():
            unused = any(o in pname for o in OFFSET_BRANCH) or (name == "d" and pname.startswith("norm2."))
            assert (prm.grad is None) == unused, (name, pname)
            assert unused or torch.isfinite(prm.grad).all()
        assert x.grad is not None and pos.grad is None


def test_region_wise_block_normalises_the_mlp_branch_by_norm1(cpu_formulations):
    """the reference's forward as written: x + mlp(norm1(x)), norm2 unused"""
    from models import Transformer_utils
    m = case.module(None, Transformer_utils, "d")
    x, pos = case.inputs(2)
    with torch.no_grad():
        y = m(x, pos)
        h = x + m.deformable_attn(m.norm1(x), pos)
        assert torch.allclose(y, h + m.mlp(m.norm1(h)), rtol=0, atol=1e-5 * float(y.abs().max()))
        m.norm2.weight.mul_(3.0)
        assert torch.equal(m(x, pos), y)


def test_module_argument_checks_raise(cpu_formulations):
    from models import Transformer_utils
    x, pos = case.inputs(1)
    m = Transformer_utils.DeformableLocalAttention(case.DIM, num_heads=case.HEADS, k=case.K)
    with pytest.raises(ValueError, match=r"\(B, N, 3\)"):
        m(x, pos[:, :, :2])
    with pytest.raises(ValueError, match="channels"):
        m(x[:, :, :64], pos)
    with pytest.raises(ValueError, match=r"\(B, N, k\)"):
        m(x, pos, idx=torch.zeros(case.B, case.N, 4, dtype=torch.long))
    with pytest.raises(TypeError):
        m(x, pos, denoise_length=4)
    with pytest.raises(ValueError, match="n_group"):
        Transformer_utils.DeformableLocalAttention(128, num_heads=2, n_group=4)
    with torch.no_grad():                                          # the list given by a caller and the one searched here are the same
        assert torch.equal(m(x, pos, idx=Transformer_utils.knn_point(case.K, pos, pos)), m(x, pos))


def test_attention_dropout_is_honoured_by_the_formulation(cpu_formulations):
    from models import Transformer_utils
    x, pos = case.inputs(1)
    m = Transformer_utils.DeformableLocalAttention(case.DIM, num_heads=case.HEADS, k=case.K, attn_drop=0.5)
    with torch.no_grad():
        m.eval()
        a, b = m(x, pos), m(x, pos)
        m.train()
        torch.manual_seed(0)
        c = m(x, pos)
        torch.manual_seed(1)
        d = m(x, pos)
    assert torch.equal(a, b) and not torch.equal(c, d) and not torch.equal(a, c)


def test_pool_trace_records_and_replays_idx3_and_the_arg_of_the_max(cpu_formulations, monkeypatch):
    """With upp_layers.POOL_TRACE set the module records the neighbour list, idx3 and the arg of the max; a replay into float64 takes the
    recorded choices, so it lands within f32 rounding of the recording run."""
    from models import Transformer_utils, upp_layers
    x, pos = case.inputs(1)
    m = case.module(None, Transformer_utils, "a")
    trace = {'mode': 'record', 'items': []}
    monkeypatch.setattr(upp_layers, "POOL_TRACE", trace)
    with torch.no_grad():
        want = m(x, pos)
        assert [key[0] for key, _ in trace['items']] == ['transformer_utils.knn_point', 'region_attention.idx3', 'region_attention.max']
        trace['mode'] = 'replay'
        got = m.double()(x.double(), pos.double())
    assert trace['pos'] == 3 and (got - want.double()).abs().max() <= 1e-5 * want.abs().max()


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
NPTR = {"upp_region_attn_fwd": 10, "upp_region_attn_bwd": 15, "upp_region_attn_bwd_det": 16}
OPTIONAL = {"upp_region_attn_fwd": (4, 5), "upp_region_attn_bwd": (4, 5, 13, 14), "upp_region_attn_bwd_det": (4, 5, 13, 14)}


def _call(lib, name, ptrs=None, scale=0.125, B=2, N=5, NK=7, k=3, H=2, G=2):
    return getattr(lib, name)(*((P,) * NPTR[name] if ptrs is None else ptrs), scale, B, N, NK, k, H, G, None)


@pytest.mark.parametrize("name", sorted(NPTR))
def test_entry_points_check_their_arguments_before_any_launch(name):
    lib = _abi.load()
    sizes = [dict(B=0), dict(N=0), dict(NK=0), dict(k=0), dict(H=0), dict(G=0), dict(B=-1)]
    ranges = [dict(H=17, G=1), dict(k=33), dict(H=2, G=3), dict(H=4, G=3), dict(B=65536), dict(B=60000, N=60000),
              dict(B=4096, NK=4096, H=16, G=16), dict(B=1, N=400000, k=32, H=1, G=1)]
    assert all(_call(lib, name, **kw) == BADARG for kw in sizes) and all(_call(lib, name, **kw) == RANGE for kw in ranges)
    assert all(_call(lib, name, scale=s) == BADARG for s in (0.0, -1.0, float("inf"), float("nan")))
    for i in range(NPTR[name]):                                     # bk, bv, d_krow, d_vrow may be NULL: the call then goes on to the size checks
        want = RANGE if i in OPTIONAL[name] else BADARG
        assert _call(lib, name, ptrs=tuple(None if j == i else P for j in range(NPTR[name])), k=33) == want, i


def test_operator_wrappers_refuse_cpu_tensors_and_report_the_range():
    q, PK = torch.zeros(2, 5, 128), torch.zeros(2, 2, 7, 128)
    idx = torch.zeros(2, 5, 3, dtype=torch.int64)
    idx3, w3 = torch.zeros(2, 2, 15, 3, dtype=torch.int32), torch.zeros(2, 2, 15, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.region_attn_fwd(q, idx, PK, PK, None, None, idx3, w3, 2, 0.125)
    assert not HF.region_attention_usable(q, idx, PK, PK, idx3, w3, 2)            # CPU tensors are not the kernels'
    assert ops.region_attn_usable(2, 5, 7, 3, 2, 2) and ops.region_attn_usable(32, 576, 576, 16, 6, 2) and ops.region_attn_usable(1, 1, 1, 32, 16, 16)
    for bad in ((2, 5, 7, 33, 2, 2), (2, 5, 7, 3, 17, 1), (2, 5, 7, 3, 4, 3), (65536, 5, 7, 3, 2, 2), (2, 0, 7, 3, 2, 2), (60000, 60000, 7, 3, 2, 2),
                (1, 400000, 7, 32, 1, 1)):
        assert not ops.region_attn_usable(*bad), bad
    with pytest.raises(RuntimeError, match="torch_cpu|CPU"):
        HF.region_attention(q, idx, PK, PK, None, None, idx3, w3, 2, 0.125)


def test_functional_takes_the_formulation_for_cpu_tensors(cpu_formulations):
    g = torch.Generator().manual_seed(3)
    q, PK, PV = torch.randn(2, 5, 128, generator=g), torch.randn(2, 2, 7, 128, generator=g), torch.randn(2, 2, 7, 128, generator=g)
    idx = torch.randint(0, 5, (2, 5, 3), generator=g)
    idx3, w3 = torch.randint(0, 7, (2, 2, 15, 3), generator=g).int(), torch.rand(2, 2, 15, 3, generator=g)
    assert torch.equal(HF.region_attention(q, idx, PK, PV, None, None, idx3, w3, 2, 0.125),
                       torch_cpu.region_attention(q, idx, PK, PV, None, None, idx3, w3, 2, 0.125))
