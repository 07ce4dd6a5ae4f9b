"""The deformable local cross-attention on a GPU-less host: the torch formulations (upp_hip.torch_cpu.deform_offset / deform_attention)
in float64 against a direct materialising restatement of the reference's forward (concatenate, then the offset MLP; interpolate, then
project), the module's state-dict schema, the fixture cases of tests/golden/deform_attn.npz (tools/gen_golden_deform_attn.py: the
reference's own classes) on the CPU formulation, the opt-in wiring into models.AdaPoinTr, which parameters get a gradient, and the
argument checks of the C entry points, which happen before any launch.

Fixture bound: max(1e-5, 3 x err_ref) of each output's float64 maximum, err_ref the reference's own f32-against-f64 error computed here
from the stored pair.  Measured for the torch formulation on the CPU: a 4.9e-7, b 6.2e-7, c 3.6e-7, d 3.6e-7 (err_ref 6.0e-7, 1.2e-6,
4.4e-7, 2.9e-7; the bound is 1e-5 for all four)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _deform_attn_case as case
from conftest import GOLDEN
from upp_hip import _abi, functional as HF, ops, torch_cpu

BADARG, RANGE = -1, -2
P = ctypes.c_void_p(64)            # non-NULL, 16-byte aligned, never dereferenced
OFFSET_BRANCH = ("proj_v_off.", "linear_offset.")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "deform_attn.npz"))


@pytest.fixture()
def cpu_formulations():
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    yield
    torch_cpu.enable(was)


# ---- the formulations against the reference's own order of operations, float64 -----------------------------------------------------------
@pytest.mark.parametrize("B, N, NK, k, H, G", [(1, 1, 1, 1, 1, 1), (2, 5, 7, 3, 2, 1), (2, 9, 6, 4, 4, 2), (1, 3, 4, 10, 4, 4)])
def test_offset_formulation_equals_the_concatenated_form(B, N, NK, k, H, G):
    g = torch.Generator().manual_seed(B * 100 + N)
    C = 16 * H
    c = C // G
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    v_off, qp, pos = rnd(B, NK, C), rnd(B, N, C), rnd(B, NK, 3)
    W0, b0, gamma, beta, W3 = rnd(C, 2 * c), rnd(C), rnd(C), rnd(C), rnd(3, C)
    idx = torch.randint(0, NK, (B, N, k), generator=g)
    # the reference: gather, split into groups, concatenate with the query's group, the offset MLP, tanh, add the gathered positions
    local = torch.gather(v_off, 1, idx.reshape(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, G, c).permute(0, 3, 1, 2, 4)
    group_q = qp.view(B, N, G, c).permute(0, 2, 1, 3).unsqueeze(3).expand(-1, -1, -1, k, -1)
    h = F.gelu(F.layer_norm(F.linear(torch.cat([local, group_q], -1), W0, b0), (C,), gamma, beta, 1e-5))
    local_pos = torch.gather(pos, 1, idx.reshape(B, N * k, 1).expand(-1, -1, 3)).view(B, 1, N, k, 3)
    want = (local_pos + torch.tanh(F.linear(h, W3))).reshape(B, G, N * k, 3)
    A = torch.matmul(v_off.view(B, NK, G, c).permute(0, 2, 1, 3), W0[:, :c].t())
    Bq = torch.matmul(qp.view(B, N, G, c).permute(0, 2, 1, 3), W0[:, c:].t()) + b0
    got = torch_cpu.deform_offset(A, Bq, idx, pos, gamma, beta, 1e-5, W3)
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize("B, N, NK, k, H, G", [(1, 1, 1, 1, 1, 1), (2, 5, 7, 3, 2, 1), (2, 9, 6, 4, 4, 2), (1, 3, 4, 10, 4, 4)])
@pytest.mark.parametrize("bias", [True, False])
def test_attention_formulation_equals_interpolate_then_project(B, N, NK, k, H, G, bias):
    g = torch.Generator().manual_seed(B * 100 + N + 7)
    hd = 8
    C = hd * H
    c = C // G
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q, v, Wk, Wv = rnd(B, N, C), rnd(B, NK, C), rnd(C, C), rnd(C, C)
    bk, bv = (rnd(C), rnd(C)) if bias else (None, None)
    idx3 = torch.randint(0, NK, (B, G, N * k, 3), generator=g).int()
    w3 = torch.rand(B, G, N * k, 3, generator=g, dtype=torch.float64)
    w3 = w3 / w3.sum(-1, keepdim=True)
    scale = hd ** -0.5
    # the reference: three_interpolate per group, regroup to (B,N,k,C), proj_k / proj_v over B N k rows, attention over the k slots
    vg = v.view(B, NK, G, c).permute(0, 2, 1, 3)
    near = torch.gather(vg, 2, idx3.long().reshape(B, G, N * k * 3, 1).expand(-1, -1, -1, c)).view(B, G, N * k, 3, c)
    interp = (near * w3.unsqueeze(-1)).sum(3).view(B, G, N, k, c).permute(0, 2, 3, 1, 4).reshape(B, N, k, C)
    key = F.linear(interp, Wk, bk).view(B, N, k, H, hd).permute(0, 3, 1, 2, 4)
    val = F.linear(interp, Wv, bv).view(B, N, k, H, hd).permute(0, 3, 1, 2, 4)
    attn = (torch.einsum('bhnc,bhnkc->bhnk', q.view(B, N, H, hd).permute(0, 2, 1, 3), key) * scale).softmax(-1)
    want = torch.einsum('bhnk,bhnkc->bhnc', attn, val).permute(0, 2, 1, 3).reshape(B, N, C)
    PK = torch.stack([vg[:, i] @ Wk[:, i * c:(i + 1) * c].t() for i in range(G)], 1)
    PV = torch.stack([vg[:, i] @ Wv[:, i * c:(i + 1) * c].t() for i in range(G)], 1)
    got = torch_cpu.deform_attention(q, PK, PV, bk, bv, idx3, w3, H, scale)
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-12 * want.abs().max()


def test_formulation_treats_indices_outside_their_range_as_absent():
    """include/upp_hip.h and da_row: an idx3 outside [0, NK) contributes nothing (the twin of the rw_deform test of this name)."""
    g = torch.Generator().manual_seed(11)
    B, N, NK, k, G, H, C = 1, 2, 3, 2, 1, 2, 8
    q, PK, PV, bk, bv = (torch.randn(*s, generator=g) for s in ((B, N, C), (B, G, NK, C), (B, G, NK, C), (C,), (C,)))
    idx3 = torch.randint(0, NK, (B, G, N * k, 3), generator=g).int()
    w3 = torch.rand(B, G, N * k, 3, generator=g) + 0.1
    idx3[0, 0, 1, 0], idx3[0, 0, 2, 2] = -1, NK
    got = torch_cpu.deform_attention(q, PK, PV, bk, bv, idx3, w3, H, 0.35)
    w0, i0 = w3.clone(), idx3.clone()
    w0[0, 0, 1, 0], w0[0, 0, 2, 2] = 0.0, 0.0
    i0[0, 0, 1, 0], i0[0, 0, 2, 2] = 0, 0
    want = torch_cpu.deform_attention(q, PK, PV, bk, bv, i0, w0, H, 0.35)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, torch_cpu.deform_attention(q, PK, PV, bk, bv, i0, w3, H, 0.35))      # (the two entries do carry weight)


# ---- the modules: schema, fixture, wiring, gradients ----------------------------------------------------------------------------------
def test_state_dict_schema_is_the_references_and_loads_strictly():
    from models import AdaPoinTr, Transformer_utils
    want = {}
    for line in open(os.path.join(GOLDEN, "deform_attn_keys.txt")):
        name, key, *shape = line.split()
        want.setdefault(name, {})[key] = tuple(int(s) for s in shape)
    assert set(want) == {"a", "c", "d"} and len(want["a"]) == 15
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


def test_the_opt_in_builds_deform_in_all_three_positions():
    from models import AdaPoinTr
    from models.Transformer_utils import DeformableLocalCrossAttention as Deform
    blk = AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-deform', k=6, n_group=1, deformable=True)
    assert isinstance(blk.local_attn, Deform) and blk.local_attn.k == 6 and blk.local_attn.n_group == 1
    blk = AdaPoinTr.CrossAttnBlockApi(128, 2, self_attn_block_style='deform', cross_attn_block_style='attn-deform', deformable=True)
    assert isinstance(blk.local_self_attn, Deform) and isinstance(blk.local_cross_attn, Deform) and blk.self_attn is None
    enc = AdaPoinTr.PointTransformerEncoder(embed_dim=128, depth=2, num_heads=2, block_style_list=['attn-deform', 'attn'], deformable=True)
    assert isinstance(enc.blocks.blocks[0].local_attn, Deform) and enc.blocks.blocks[1].local_attn is None
    dec = AdaPoinTr.PointTransformerDecoder(embed_dim=128, depth=1, num_heads=2, self_attn_block_style_list=['attn-deform'],
                                            cross_attn_block_style_list=['deform'], deformable=True)
    assert isinstance(dec.blocks.blocks[0].local_self_attn, Deform) and isinstance(dec.blocks.blocks[0].local_cross_attn, Deform)
    for token in ('rw_deform', 'deform_graph'):                                  # still not ported, with or without the keyword
        with pytest.raises(ValueError, match="%r" % token):
            AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-' + token, deformable=True)
        with pytest.raises(ValueError, match="%r" % token):
            AdaPoinTr.CrossAttnBlockApi(128, 2, self_attn_block_style='attn', cross_attn_block_style=token, deformable=True)
    with pytest.raises(ValueError, match="deformable=True"):                     # the default still raises, and names the keyword
        AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-deform')
    with pytest.raises(ValueError, match="'deform'"):
        AdaPoinTr.PointTransformerDecoder(embed_dim=128, depth=1, num_heads=2, self_attn_block_style_list=['attn-deform'],
                                          cross_attn_block_style_list=['attn'])
    with pytest.raises(ValueError, match="local token"):
        AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='graph-deform', deformable=True)


def _deform_cfg(deformable):
    import _adapointr_model_case as mc
    from utils.config import EasyDict
    cfg = mc.config()
    cfg['encoder_config']['block_style_list'] = ['attn-deform', 'attn']
    cfg['decoder_config']['self_attn_block_style_list'] = ['attn-deform', 'attn']
    cfg['decoder_config']['cross_attn_block_style_list'] = ['attn-deform', 'attn']
    if deformable is not None:
        cfg['deformable'] = deformable

    def wrap(d):
        return EasyDict({k: wrap(v) if isinstance(v, dict) else v for k, v in d.items()})
    return wrap(cfg)


def test_from_cfg_passes_the_opt_in_through():
    from models import AdaPoinTr
    from models.Transformer_utils import DeformableLocalCrossAttention as Deform
    model = AdaPoinTr.from_cfg(_deform_cfg(True))
    enc, dec = model.base_model.encoder.blocks.blocks[0], model.base_model.decoder.blocks.blocks[0]
    assert isinstance(enc.local_attn, Deform) and isinstance(dec.local_self_attn, Deform) and isinstance(dec.local_cross_attn, Deform)
    assert enc.local_attn.k == 8 and enc.local_attn.n_group == 2
    for deformable in (None, False):
        with pytest.raises(ValueError, match="'deform'"):
            AdaPoinTr.from_cfg(_deform_cfg(deformable))


def test_the_offset_branch_gets_no_gradient_and_everything_else_does(cpu_formulations):
    from models import AdaPoinTr, Transformer_utils
    q, v, q_pos, v_pos = (t.requires_grad_() for t in case.inputs(1))
    for name in ("a", "b", "c"):
        m = case.module(AdaPoinTr, Transformer_utils, name)
        for t in (q, v, q_pos, v_pos):
            t.grad = None
        case.run(m, name, q, v, q_pos, v_pos).square().sum().backward()
        for pname, prm in m.named_parameters():
            offset = any(o in pname for o in OFFSET_BRANCH)
            assert (prm.grad is None) == offset, (name, pname)
            assert offset or torch.isfinite(prm.grad).all()
        assert q.grad is not None and q_pos.grad is None and v_pos.grad is None and (v.grad is not None) == (name != "b")


def test_denoise_length_restrictions_raise(cpu_formulations):
    from models import Transformer_utils
    q, v, q_pos, v_pos = case.inputs(1)
    m = Transformer_utils.DeformableLocalCrossAttention(case.DIM, num_heads=case.HEADS, k=case.K)
    idx = Transformer_utils.denoise_knn(case.K, q_pos, case.D)
    with pytest.raises(ValueError, match="idx is given"):
        m(q, q_pos, idx=idx, denoise_length=case.D)
    with pytest.raises(ValueError, match="self form"):
        m(q, q_pos, v=v, denoise_length=case.D)
    with pytest.raises(ValueError, match="self form"):
        m(q, q_pos, v_pos=v_pos, denoise_length=case.D)
    with pytest.raises(ValueError, match="real tokens"):
        m(q, q_pos, denoise_length=case.NQ - case.K + 1)
    with pytest.raises(ValueError, match=r"\(B, N, k\)"):
        m(q, q_pos, idx=idx[:, :, :4])
    with torch.no_grad():                                          # the list given by a caller and the one searched here are the same
        assert torch.equal(m(q, q_pos, idx=idx), m(q, q_pos, denoise_length=case.D))
    with pytest.raises(ValueError, match="n_group"):
        Transformer_utils.DeformableLocalCrossAttention(128, num_heads=2, n_group=4)


def test_pool_trace_records_and_replays_the_three_nearest_choice(cpu_formulations, monkeypatch):
    """With upp_layers.POOL_TRACE set the module records idx3 beside the neighbour list; a replay into float64 takes the recorded
    choices and recomputes the distances from them, so it lands within f32 rounding of the recording run."""
    from models import Transformer_utils, upp_layers
    q, v, q_pos, v_pos = case.inputs(1)
    m = case.module(None, Transformer_utils, "a")
    trace = {'mode': 'record', 'items': []}
    monkeypatch.setattr(upp_layers, "POOL_TRACE", trace)
    with torch.no_grad():
        want = m(q, q_pos, v=v, v_pos=v_pos)
        assert [key[0] for key, _ in trace['items']] == ['transformer_utils.knn_point', 'deformable_attention.idx3']
        trace['mode'] = 'replay'
        got = m.double()(q.double(), q_pos.double(), v=v.double(), v_pos=v_pos.double())
    assert trace['pos'] == 2 and (got - want.double()).abs().max() <= 1e-5 * want.abs().max()


def test_no_einops_anywhere_in_the_package():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iccv2025-upp_amd")
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                assert "einops" not in open(os.path.join(d, f)).read(), os.path.join(d, f)


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def _offset(lib, ptrs=(P,) * 8, eps=1e-5, B=2, G=2, N=5, NK=7, k=3, C=128):
    return lib.upp_deform_offset_fwd(*ptrs, eps, B, G, N, NK, k, C, None)


def _fwd(lib, ptrs=(P,) * 9, scale=0.125, B=2, N=5, NK=7, k=3, H=2, G=2):
    return lib.upp_deform_attn_fwd(*ptrs, scale, B, N, NK, k, H, G, None)


def _bwd(lib, name, ptrs=(P,) * 14, scale=0.125, B=2, N=5, NK=7, k=3, H=2, G=2):
    return getattr(lib, name)(*ptrs, scale, B, N, NK, k, H, G, None)


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _abi.load()
    calls = [lambda **kw: _fwd(lib, **kw), lambda **kw: _bwd(lib, "upp_deform_attn_bwd", **kw), lambda **kw: _bwd(lib, "upp_deform_attn_bwd_det", **kw)]
    sizes = [dict(B=0), dict(N=0), dict(NK=0), dict(k=0), dict(H=0), dict(G=0), dict(B=-1)]
    ranges = [dict(H=17, G=1), dict(k=33), dict(H=2, G=3), dict(H=4, G=3), dict(B=65536), dict(B=60000, N=60000),
              dict(B=4096, NK=4096, H=16, G=16), dict(B=30000, N=30000, k=1, H=1, G=1)]
    for call in calls:
        assert all(call(**kw) == BADARG for kw in sizes) and all(call(**kw) == RANGE for kw in ranges)
        assert all(call(scale=s) == BADARG for s in (0.0, -1.0, float("inf"), float("nan")))
    assert all(_offset(lib, **kw) == BADARG for kw in sizes if "H" not in kw) and _offset(lib, C=0) == BADARG
    assert all(_offset(lib, eps=e) == BADARG for e in (0.0, -1e-5, float("inf"), float("nan")))
    assert _offset(lib, C=96) == RANGE and _offset(lib, C=64 * 17, G=1) == RANGE and _offset(lib, k=33) == RANGE
    assert _offset(lib, C=128, G=3) == RANGE and _offset(lib, B=65536) == RANGE
    for i in range(8):                                             # every pointer of the offset head is required
        assert _offset(lib, ptrs=tuple(None if j == i else P for j in range(8))) == BADARG, i
    for i in range(9):                                             # bk (3) and bv (4) may be NULL: the call then goes on to the size checks
        want = RANGE if i in (3, 4) else BADARG
        assert _fwd(lib, ptrs=tuple(None if j == i else P for j in range(9)), k=33) == want, i
    for name in ("upp_deform_attn_bwd", "upp_deform_attn_bwd_det"):
        for i in range(14):                                        # ... and d_krow (12) beside them
            want = RANGE if i in (3, 4, 12) else BADARG
            assert _bwd(lib, name, ptrs=tuple(None if j == i else P for j in range(14)), k=33) == want, (name, i)


def test_operator_wrappers_refuse_cpu_tensors_and_report_the_range():
    q, PK = torch.zeros(2, 5, 128), torch.zeros(2, 2, 7, 128)
    idx3, w3 = torch.zeros(2, 2, 15, 3, dtype=torch.int32), torch.zeros(2, 2, 15, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.deform_attn_fwd(q, PK, PK, None, None, idx3, w3, 2, 0.125)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.deform_offset_fwd(PK, torch.zeros(2, 2, 5, 128), torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(2, 7, 3),
                              torch.ones(128), torch.zeros(128), torch.zeros(3, 128), 1e-5)
    assert not HF.deform_attention_usable(q, PK, PK, idx3, w3, 2)                  # CPU tensors are not the kernels'
    assert ops.deform_attn_usable(2, 5, 7, 3, 2, 2) and ops.deform_attn_usable(65535, 1, 1, 32, 16, 16)
    for bad in ((2, 5, 7, 33, 2, 2), (2, 5, 7, 3, 17, 1), (2, 5, 7, 3, 4, 3), (65536, 5, 7, 3, 2, 2), (2, 0, 7, 3, 2, 2), (60000, 60000, 7, 3, 2, 2)):
        assert not ops.deform_attn_usable(*bad), bad
