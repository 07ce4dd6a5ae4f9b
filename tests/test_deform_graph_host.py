"""The deformable graph attention on a GPU-less host: the float64 restatement identity (W1 f + (W2 - W1) q + b through the gather against
the reference's materialising order), the torch formulations (upp_hip.torch_cpu.interp_edge_max and deform_offset(ball=True)) against
plain numpy / float64 statements, the modules' state-dict schema, the fixture cases of tests/golden/deform_graph.npz
(tools/gen_golden_deform_graph.py: the reference's own classes) on the CPU formulation, the opt-in wiring into models.AdaPoinTr, the
argument checks of the C entry points, which happen before any launch, and that the autograd node follows functional.DETERMINISTIC.

Fixture bound: max(1e-5, 3 x err_ref) of each output's float64 maximum, err_ref the reference's own f32-against-f64 error computed here
from the stored pair (a 7.6e-7, b 7.1e-7, c 3.0e-7, d 5.3e-7: the bound is 1e-5 for all four).  Measured for the torch formulation on
the CPU: a 4.5e-7, b 3.6e-7, c 2.9e-7, d 5.9e-7."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _deform_graph_case as case
import _interp_max_reference as R
from conftest import GOLDEN, ROOT
from upp_hip import _abi, functional as HF, ops, torch_cpu

BADARG, RANGE = -1, -2
P = ctypes.c_void_p(64)            # non-NULL, 16-byte aligned, never dereferenced
OFFSET_BRANCH = ("proj_v_off.", "linear_offset.")
NEW = ("upp_deform_offset_ball_fwd", "upp_interp_max_fwd", "upp_interp_max_bwd", "upp_interp_max_bwd_det")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "deform_graph.npz"))


@pytest.fixture()
def cpu_formulations():
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    yield
    torch_cpu.enable(was)


def _weights(g, *shape, dtype=torch.float64):
    w = torch.rand(*shape, generator=g, dtype=dtype) + 0.05
    return w / w.sum(-1, keepdim=True)


# ---- the restatement, float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, N, NK, k, C", [(1, 1, 1, 1, 1), (2, 5, 7, 3, 16), (2, 9, 6, 4, 24), (1, 3, 2, 10, 8)])
def test_restatement_equals_interpolate_concatenate_project_max(B, N, NK, k, C):
    g = torch.Generator().manual_seed(B * 100 + N)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q, v, W, b = rnd(B, N, C), rnd(B, NK, C), rnd(C, 2 * C), rnd(C)
    idx3 = torch.randint(0, NK, (B, N * k, 3), generator=g).int()
    w3 = _weights(g, B, N * k, 3)
    # the reference: three_interpolate, concatenate [f - q ; q], knn_map (Linear + LeakyReLU), max over the slots
    near = torch.gather(v, 1, idx3.long().reshape(B, N * k * 3, 1).expand(-1, -1, C)).view(B, N * k, 3, C)
    f = (near * w3.unsqueeze(-1)).sum(2).view(B, N, k, C)
    qe = q.unsqueeze(2).expand(-1, -1, k, -1)
    want = F.leaky_relu(F.linear(torch.cat([f - qe, qe], -1), W, b), 0.2).max(-2)[0]
    PW = v @ W[:, :C].t()
    Bq = q @ (W[:, C:] - W[:, :C]).t() + b
    got = torch_cpu.interp_edge_max(PW, Bq, idx3, w3, 0.2)
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize("B, G, N, NK, k, C", [(1, 1, 3, 5, 1, 16), (2, 2, 9, 6, 8, 32), (2, 1, 5, 7, 3, 8)])
def test_ball_offset_formulation_equals_the_concatenated_form(B, G, N, NK, k, C):
    g = torch.Generator().manual_seed(B * 100 + N + 1)
    c = C // G
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    v_off, qp, pos = rnd(B, NK, C), rnd(B, N, C), rnd(B, NK, 3)
    W0, b0, gamma, beta, W3 = rnd(C, 2 * c), rnd(C), rnd(C), rnd(C), rnd(3, C)
    idx = torch.randint(0, NK, (B, N, k), generator=g)
    local = torch.gather(v_off, 1, idx.reshape(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, G, c).permute(0, 3, 1, 2, 4)
    group_q = qp.view(B, N, G, c).permute(0, 2, 1, 3).unsqueeze(3).expand(-1, -1, -1, k, -1)
    h = F.gelu(F.layer_norm(F.linear(torch.cat([local, group_q], -1), W0, b0), (C,), gamma, beta, 1e-5))
    local_pos = torch.gather(pos, 1, idx.reshape(B, N * k, 1).expand(-1, -1, 3)).view(B, 1, N, k, 3)
    scale = (local_pos.max(-2)[0] - local_pos.min(-2)[0]).unsqueeze(-2) * 0.5
    want = (local_pos + torch.tanh(F.linear(h, W3)) * scale).reshape(B, G, N * k, 3)
    A = torch.matmul(v_off.view(B, NK, G, c).permute(0, 2, 1, 3), W0[:, :c].t())
    Bq = torch.matmul(qp.view(B, N, G, c).permute(0, 2, 1, 3), W0[:, c:].t()) + b0
    got = torch_cpu.deform_offset(A, Bq, idx, pos, gamma, beta, 1e-5, W3, ball=True)
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-12 * want.abs().max()
    stated = R.ball_offset(A.numpy(), Bq.numpy(), idx.numpy(), pos.numpy(), gamma.numpy(), beta.numpy(), 1e-5, W3.numpy())
    assert np.abs(got.numpy() - stated).max() <= 1e-12 * np.abs(stated).max()
    plain = torch_cpu.deform_offset(A, Bq, idx, pos, gamma, beta, 1e-5, W3)
    assert torch.equal(plain, torch_cpu.deform_offset(A, Bq, idx, pos, gamma, beta, 1e-5, W3, ball=False))
    if k == 1:                                                        # one slot: the ball has no extent and nothing is shifted
        assert torch.equal(got, local_pos.expand(-1, G, -1, -1, -1).reshape(B, G, N, 3)) and not torch.equal(plain, got)


# ---- the torch formulation against the numpy statement -----------------------------------------------------------------------------------
def _lattice(g, *shape):
    """multiples of 2^-6 in [-4, 4): every fma of the statement is exact in f32, so formulation and statement must agree bit for bit"""
    return torch.randint(-256, 256, shape, generator=g).float() / 64


@pytest.mark.parametrize("B, N, NK, k, O", [(1, 1, 1, 1, 1), (2, 5, 7, 3, 65), (1, 4, 2, 5, 9)])
def test_formulation_equals_the_numpy_statement(B, N, NK, k, O):
    g = torch.Generator().manual_seed(N + O)
    PW, Bq = _lattice(g, B, NK, O), _lattice(g, B, N, O)
    idx3 = torch.randint(0, NK, (B, N * k, 3), generator=g).int()
    w3 = torch.randint(0, 5, (B, N * k, 3), generator=g).float() / 4
    if NK < 3:                                                        # three_nn's padding: index 0 at +inf, weight 0
        idx3[..., NK:] = 0
        w3[..., NK:] = 0
    for slope in (0.2, 0.0, 1.0):
        out, arg, _ = R.forward(PW.numpy(), Bq.numpy(), idx3.numpy(), w3.numpy(), slope)
        assert np.array_equal(torch_cpu.interp_edge_max(PW, Bq, idx3, w3, slope).numpy(), out), slope


def test_ties_take_the_lowest_slot_and_foreign_indices_contribute_nothing():
    g = torch.Generator().manual_seed(5)
    B, N, NK, k, O = 1, 3, 4, 4, 6
    PW, Bq = _lattice(g, B, NK, O), _lattice(g, B, N, O)
    idx3 = torch.randint(0, NK, (B, N * k, 3), generator=g).int()
    w3 = torch.randint(1, 5, (B, N * k, 3), generator=g).float() / 4
    idx3[:, 2::k], w3[:, 2::k] = idx3[:, 1::k], w3[:, 1::k]           # slot 2 repeats slot 1: an exact tie wherever either wins
    out, arg, m = R.forward(PW.numpy(), Bq.numpy(), idx3.numpy(), w3.numpy(), 0.2)
    assert not (arg == 2).any() and (arg == 1).any()
    assert np.array_equal(torch_cpu.interp_edge_max(PW, Bq, idx3, w3, 0.2).numpy(), out)
    bad = idx3.clone()
    bad[:, :, 1] = torch.where(torch.arange(N * k).view(1, -1) % 2 == 0, torch.tensor(-1), torch.tensor(NK)).int()
    zeroed = w3.clone()
    zeroed[:, :, 1] = 0
    want, _, _ = R.forward(PW.numpy(), Bq.numpy(), idx3.numpy(), zeroed.numpy(), 0.2)
    got, _, _ = R.forward(PW.numpy(), Bq.numpy(), bad.numpy(), w3.numpy(), 0.2)
    assert np.array_equal(got, want) and np.array_equal(torch_cpu.interp_edge_max(PW, Bq, bad, w3, 0.2).numpy(), want)


def test_det_statement_is_right_to_rounding_and_sensitive_to_order():
    g = torch.Generator().manual_seed(9)
    B, N, NK, k, O = 2, 40, 5, 3, 7
    PW, Bq, go = torch.randn(B, NK, O, generator=g), torch.randn(B, N, O, generator=g), torch.randn(B, N, O, generator=g)
    idx3 = torch.full((B, N * k, 3), 2, dtype=torch.int32)            # every source on one row
    w3 = _weights(g, B, N * k, 3, dtype=torch.float32)
    out, arg, _ = R.forward(PW.numpy(), Bq.numpy(), idx3.numpy(), w3.numpy(), 0.2)
    d_Bq, d_PW = R.scatter_det(go.numpy(), out, arg, idx3.numpy(), w3.numpy(), 0.2, NK)
    _, rev = R.scatter_det(go.numpy(), out, arg, idx3.numpy(), w3.numpy(), 0.2, NK, reverse=True)
    x = [t.double().requires_grad_() for t in (PW, Bq)]
    (torch_cpu.interp_edge_max(x[0], x[1], idx3, w3.double(), 0.2) * go.double()).sum().backward()
    assert np.abs(d_PW - x[0].grad.numpy()).max() <= 1e-5 * x[0].grad.abs().max().item()
    assert np.abs(d_Bq - x[1].grad.numpy()).max() <= 1e-6 * x[1].grad.abs().max().item()
    assert not np.array_equal(rev, d_PW) and not d_PW[:, :2].any() and not d_PW[:, 3:].any()


# ---- the modules: schema, fixture, wiring, gradients ----------------------------------------------------------------------------------
def test_state_dict_schema_is_the_references_and_loads_strictly():
    from models import AdaPoinTr, Transformer_utils
    want = {}
    for line in open(os.path.join(GOLDEN, "deform_graph_keys.txt")):
        name, key, *shape = line.split()
        want.setdefault(name, {})[key] = tuple(int(s) for s in shape)
    assert set(want) == {"a", "c", "d"} and len(want["a"]) == 9 and len(want["d"]) == 15
    assert set(want["a"]) == {"proj_v_off.weight", "proj_v_off.bias", "linear_offset.0.weight", "linear_offset.0.bias", "linear_offset.1.weight",
                              "linear_offset.1.bias", "linear_offset.3.weight", "knn_map.0.weight", "knn_map.0.bias"}
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
    assert {n: int(fixture["seed_" + n]) for n in case.CASES} == {"a": 0, "b": 0, "c": 2, "d": 0}
    m = case.module(AdaPoinTr, Transformer_utils, name)
    with torch.no_grad():
        y = case.run(m, name, *case.inputs(int(fixture["seed_" + name])))
    case.check_output(fixture, name, y, "torch formulation (CPU)")


def test_a_list_opt_in_builds_deform_graph_in_all_three_positions():
    from models import AdaPoinTr
    from models.Transformer_utils import DeformableLocalCrossAttention as Deform, improvedDeformableLocalGraphAttention as Graph
    both = ['deform', 'deform_graph']
    blk = AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-deform_graph', k=6, deformable=both)
    assert isinstance(blk.local_attn, Graph) and blk.local_attn.k == 6 and blk.attn is not None
    blk = AdaPoinTr.CrossAttnBlockApi(128, 2, self_attn_block_style='deform_graph', cross_attn_block_style='attn-deform_graph', k=7,
                                      deformable=('deform_graph',))
    assert isinstance(blk.local_self_attn, Graph) and isinstance(blk.local_cross_attn, Graph) and blk.self_attn is None
    assert blk.local_self_attn.k == blk.local_cross_attn.k == 7
    enc = AdaPoinTr.PointTransformerEncoder(embed_dim=128, depth=2, num_heads=2, block_style_list=['attn-deform_graph', 'attn-deform'],
                                            deformable=both)
    assert isinstance(enc.blocks.blocks[0].local_attn, Graph) and isinstance(enc.blocks.blocks[1].local_attn, Deform)
    dec = AdaPoinTr.PointTransformerDecoder(embed_dim=128, depth=1, num_heads=2, self_attn_block_style_list=['attn-deform_graph'],
                                            cross_attn_block_style_list=['deform_graph'], deformable={'deform_graph'})
    assert isinstance(dec.blocks.blocks[0].local_self_attn, Graph) and isinstance(dec.blocks.blocks[0].local_cross_attn, Graph)
    for deformable in (True, False, ['deform'], ()):                               # True still means exactly {'deform'}
        with pytest.raises(ValueError, match="'deform_graph'"):
            AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-deform_graph', deformable=deformable)
    with pytest.raises(ValueError, match="deformable=True"):                        # a list without `deform` refuses it with today's message
        AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-deform', deformable=['deform_graph'])
    for deformable in (both, True, ['deform', 'deform_graph', 'rw_deform']):
        with pytest.raises(ValueError, match="'rw_deform'"):
            AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn-rw_deform', deformable=deformable)
    for bad in (['graph'], ['deform', 'attn'], 'deform_graph', 3):
        with pytest.raises(ValueError, match="deformable"):
            AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='attn', deformable=bad)
    with pytest.raises(ValueError, match="local token"):
        AdaPoinTr.SelfAttnBlockApi(128, 2, block_style='graph-deform_graph', deformable=both)


def _graph_cfg(deformable):
    import _adapointr_model_case as mc
    from utils.config import EasyDict
    cfg = mc.config()
    cfg['encoder_config']['block_style_list'] = ['attn-deform_graph', 'attn']
    cfg['decoder_config']['self_attn_block_style_list'] = ['attn-deform_graph', 'attn-deform']
    cfg['decoder_config']['cross_attn_block_style_list'] = ['attn-deform_graph', 'attn']
    if deformable is not None:
        cfg['deformable'] = deformable

    def wrap(d):
        return EasyDict({k: wrap(v) if isinstance(v, dict) else v for k, v in d.items()})
    return wrap(cfg)


def test_from_cfg_passes_a_list_through():
    from models import AdaPoinTr
    from models.Transformer_utils import DeformableLocalCrossAttention as Deform, improvedDeformableLocalGraphAttention as Graph
    model = AdaPoinTr.from_cfg(_graph_cfg(['deform', 'deform_graph']))
    enc, dec = model.base_model.encoder.blocks.blocks[0], model.base_model.decoder.blocks.blocks
    assert isinstance(enc.local_attn, Graph) and isinstance(dec[0].local_self_attn, Graph) and isinstance(dec[0].local_cross_attn, Graph)
    assert isinstance(dec[1].local_self_attn, Deform) and enc.local_attn.k == 8
    sd = {k: t.clone() for k, t in model.state_dict().items()}
    AdaPoinTr.from_cfg(_graph_cfg(['deform', 'deform_graph'])).load_state_dict(sd, strict=True)
    for deformable in (None, False, True, ['deform']):
        with pytest.raises(ValueError, match="'deform_graph'"):
            AdaPoinTr.from_cfg(_graph_cfg(deformable))
    with pytest.raises(ValueError, match="deformable"):
        AdaPoinTr.from_cfg(_graph_cfg(['deform', 'graph']))


def test_the_offset_branch_gets_no_gradient_and_everything_else_does(cpu_formulations):
    from models import AdaPoinTr, Transformer_utils
    q, v, q_pos, v_pos = (t.requires_grad_() for t in case.inputs(1))
    for name in case.CASES:
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
    m = Transformer_utils.improvedDeformableLocalGraphAttention(case.DIM, k=case.K)
    idx = Transformer_utils.denoise_knn(case.K, q_pos, case.D)
    with pytest.raises(ValueError, match="idx is given"):
        m(q, q_pos, idx=idx, denoise_length=case.D)
    with pytest.raises(ValueError, match="self form"):
        m(q, q_pos, v=v, denoise_length=case.D)
    with pytest.raises(ValueError, match="self form"):
        m(q, q_pos, v_pos=v_pos, denoise_length=case.D)
    with pytest.raises(ValueError, match=r"\(B, N, k\)"):
        m(q, q_pos, idx=idx[:, :, :4])
    with torch.no_grad():
        assert torch.equal(m(q, q_pos, idx=idx), m(q, q_pos, denoise_length=case.D))
    improved = Transformer_utils.improvedDeformableLocalCrossAttention(case.DIM, num_heads=case.HEADS, k=case.K)
    with pytest.raises(TypeError, match="denoise_length"):                          # the reference's has no such argument
        improved(q, q_pos, denoise_length=case.D)
    assert improved.ball and not Transformer_utils.DeformableLocalCrossAttention.ball


def test_pool_trace_records_and_replays_idx3_and_the_arg_of_the_max(cpu_formulations, monkeypatch):
    from models import Transformer_utils, upp_layers
    q, v, q_pos, v_pos = case.inputs(1)
    m = case.module(None, Transformer_utils, "a")
    trace = {'mode': 'record', 'items': []}
    monkeypatch.setattr(upp_layers, "POOL_TRACE", trace)
    with torch.no_grad():
        want = m(q, q_pos, v=v, v_pos=v_pos)
        assert [key[0] for key, _ in trace['items']] == ['transformer_utils.knn_point', 'deformable_graph.idx3', 'deformable_graph.max']
        trace['mode'] = 'replay'
        got = m.double()(q.double(), q_pos.double(), v=v.double(), v_pos=v_pos.double())
    assert trace['pos'] == 3 and (got - want.double()).abs().max() <= 1e-5 * want.abs().max()


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "upp_hip.h")).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _abi.SIGNATURES, name
        assert re.search(r" T %s\b" % name, exported), name
    sig = _abi.SIGNATURES
    assert len(sig["upp_deform_offset_ball_fwd"][1]) == len(sig["upp_deform_offset_fwd"][1])
    assert len(sig["upp_interp_max_bwd_det"][1]) == len(sig["upp_interp_max_bwd"][1]) and "#define UPP_ABI_VERSION 5" in hdr


def _fwd(lib, ptrs=(P,) * 6, slope=0.2, B=2, N=5, NK=7, k=3, O=65):
    return lib.upp_interp_max_fwd(*ptrs, slope, B, N, NK, k, O, None)


def _bwd(lib, name, ptrs=(P,) * 7, slope=0.2, B=2, N=5, NK=7, k=3, O=65):
    return getattr(lib, name)(*ptrs, slope, B, N, NK, k, O, None)


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _abi.load()
    calls = [lambda **kw: _fwd(lib, **kw), lambda **kw: _bwd(lib, "upp_interp_max_bwd", **kw), lambda **kw: _bwd(lib, "upp_interp_max_bwd_det", **kw)]
    sizes = [dict(B=0), dict(N=0), dict(NK=0), dict(k=0), dict(O=0), dict(B=-1)]
    ranges = [dict(k=33), dict(O=1025), dict(B=65536), dict(B=60000, N=60000), dict(B=4096, NK=4096, O=1024), dict(B=30000, N=30000, k=1, O=1)]
    for call in calls:
        assert all(call(**kw) == BADARG for kw in sizes) and all(call(**kw) == RANGE for kw in ranges)
        assert all(call(slope=s) == BADARG for s in (-0.1, 1.5, float("inf"), float("-inf"), float("nan")))
        assert call(slope=float("nan"), k=33) == BADARG
    for i in range(6):
        assert _fwd(lib, ptrs=tuple(None if j == i else P for j in range(6)), k=33) == BADARG, i
    for name in ("upp_interp_max_bwd", "upp_interp_max_bwd_det"):
        for i in range(7):
            assert _bwd(lib, name, ptrs=tuple(None if j == i else P for j in range(7)), k=33) == BADARG, (name, i)

    def offset(ptrs=(P,) * 8, eps=1e-5, B=2, G=2, N=5, NK=7, k=3, C=128):
        return lib.upp_deform_offset_ball_fwd(*ptrs, eps, B, G, N, NK, k, C, None)
    assert all(offset(**kw) == BADARG for kw in (dict(B=0), dict(N=0), dict(NK=0), dict(k=0), dict(G=0), dict(C=0)))
    assert all(offset(eps=e) == BADARG for e in (0.0, -1e-5, float("inf"), float("nan")))
    assert offset(C=96) == RANGE and offset(C=64 * 17, G=1) == RANGE and offset(k=33) == RANGE and offset(C=128, G=3) == RANGE
    assert offset(B=65536) == RANGE
    for i in range(8):
        assert offset(ptrs=tuple(None if j == i else P for j in range(8))) == BADARG, i


def test_operator_wrappers_refuse_cpu_tensors_and_report_the_range():
    PW, Bq = torch.zeros(2, 7, 65), torch.zeros(2, 5, 65)
    idx3, w3 = torch.zeros(2, 15, 3, dtype=torch.int32), torch.zeros(2, 15, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.interp_max_fwd(PW, Bq, idx3, w3, 0.2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.interp_max_bwd(Bq, Bq, torch.zeros(2, 5, 65, dtype=torch.uint8), idx3, w3, 7, 0.2)
    with pytest.raises(ValueError, match="slope"):
        HF.interp_edge_max(PW, Bq, idx3, w3, slope=1.5)
    assert not HF.interp_edge_max_usable(PW, Bq, idx3, w3)                         # CPU tensors are not the kernels'
    assert ops.interp_max_usable(2, 5, 7, 3, 65) and ops.interp_max_usable(65535, 1, 1, 32, 1024)
    for bad in ((2, 5, 7, 33, 65), (2, 5, 7, 3, 1025), (65536, 5, 7, 3, 65), (2, 0, 7, 3, 65), (60000, 60000, 7, 3, 65)):
        assert not ops.interp_max_usable(*bad), bad


def test_cpu_tensors_take_the_torch_formulation_when_it_is_enabled(cpu_formulations):
    g = torch.Generator().manual_seed(1)
    PW, Bq = torch.randn(2, 7, 9, generator=g, requires_grad=True), torch.randn(2, 5, 9, generator=g, requires_grad=True)
    idx3 = torch.randint(0, 7, (2, 15, 3), generator=g).int()
    w3 = _weights(g, 2, 15, 3, dtype=torch.float32)
    out = HF.interp_edge_max(PW, Bq, idx3, w3)
    assert torch.equal(out, torch_cpu.interp_edge_max(PW, Bq, idx3, w3, 0.2))
    out.sum().backward()
    assert PW.grad is not None and Bq.grad is not None


# ---- the deterministic mode --------------------------------------------------------------------------------------------------------------
def test_the_node_follows_the_mode_and_the_per_call_override(monkeypatch):
    seen = []

    def fwd(PW, Bq, idx3, w3, slope=0.2):
        return torch.zeros_like(Bq), torch.zeros(Bq.shape, dtype=torch.uint8)

    def bwd(g, out, arg, idx3, w3, NK, slope=0.2, **kw):
        seen.append(kw.get("deterministic", "absent"))
        return torch.zeros_like(g), torch.zeros(g.shape[0], NK, g.shape[2])

    monkeypatch.setattr(ops, "interp_max_fwd", fwd)
    monkeypatch.setattr(ops, "interp_max_bwd", bwd)
    idx3, w3 = torch.zeros(2, 15, 3, dtype=torch.int32), torch.zeros(2, 15, 3)
    for per_call, flag, want in [(None, False, False), (None, True, True), (True, False, True), (False, True, False)]:
        PW, Bq = torch.zeros(2, 7, 9, requires_grad=True), torch.zeros(2, 5, 9, requires_grad=True)
        out = HF._InterpEdgeMax.apply(PW, Bq, idx3, w3, 0.2, per_call)            # forward outside the block, backward inside
        with HF.deterministic(flag):
            out.sum().backward()
        assert seen[-1] is want, (per_call, flag)
        assert PW.grad.shape == PW.shape and Bq.grad.shape == Bq.shape
