"""The AdaPoinTr blocks and stacks (models/AdaPoinTr.py, models/Transformer_utils.py) on the GPU, fused path: the four cases of
tests/golden/adapointr_blocks.npz (the reference's own classes, tools/gen_golden_adapointr_blocks.py) under the fixture bound
max(1e-5, 3 x err_ref) against the reference's float64 run (tests/test_prefix_attention_host.py); the gradients of case a (the decoder
with 8 denoising queries) with respect to q, v and every parameter against the module's float64 torch formulation on the same neighbour
lists, the project's gradient bound (rtol 2e-5, atol 5e-6 max|ref|) through _check_against; the kernels one fused forward + backward
launches; the declined list; and Attention(x, denoise_length=D) against Attention(x, mask=<the reference's mask>).

Measured on MI355X.  Fixture, error over the output's maximum (bound 1e-5 for all four): a 3.1e-7, b 2.7e-7, c 2.0e-7, d 1.9e-7.
Gradients of case a, max|x - f64| / max|f64| of (fused, torch f32): forward 2.8e-7, 3.5e-7; d_q 3.3e-7, 4.7e-7; d_v 4.5e-7, 5.2e-7; the
worst of the 54 parameters with a non-zero gradient 7.5e-7, 8.6e-7 (cross_attn.q_map.weight / norm_q.weight of the two blocks).  The two
cross_attn.k_map.bias gradients are identically zero in exact arithmetic -- a key bias shifts every score of a row by the same amount,
which the softmax does not see; float64 leaves 1e-17 -- so an error relative to their own maximum means nothing there and _check_against
falls through to its float64 arbitration (the fused rounding residue within twice the torch f32 one: 1.2e9 against 6.5e8, and 7.2e8
against 7.4e8, of that 1e-17).  Attention(denoise_length) against Attention(mask): 4.0e-7, 6.3e-7."""
import copy
import os

import numpy as np
import pytest
import torch

import _adapointr_case as case
import _seeded
from _attention_reference import _check_against
from conftest import GOLDEN
from models import AdaPoinTr, Transformer_utils
from upp_hip import functional as HF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "adapointr_blocks.npz"))


@pytest.mark.parametrize("name", case.CASES)
def test_fused_path_meets_the_fixture_bound(fixture, name):
    m = case.module(AdaPoinTr, name).cuda()
    x = [t.cuda() for t in case.inputs(int(fixture["seed"]))]
    HF._declined.clear()
    with torch.no_grad():
        got = case.run(m, name, *x)
    assert not HF._declined, HF._declined
    case.check_output(fixture, name, got, "fused path")


def _grads(m, q, v, q_pos, v_pos, w, lists=None):
    """forward + backward of case a -> (out, {name: gradient}, the neighbour lists it used)"""
    used = []
    own = m.blocks.lists

    def traced(*a):
        used.append(own(*a) if lists is None else lists)
        return used[-1]

    m.blocks.lists = traced
    try:
        m.zero_grad()
        q, v = q.clone().requires_grad_(True), v.clone().requires_grad_(True)
        out = m(q, v, q_pos, v_pos, denoise_length=case.D)
        (out * w).sum().backward()
    finally:
        del m.blocks.lists
    grads = {"d_q": q.grad, "d_v": v.grad}
    grads.update({n: p.grad for n, p in m.named_parameters()})
    return out.detach(), grads, used[0]


def test_decoder_gradients_against_the_float64_torch_formulation(fixture):
    q, v, q_pos, v_pos = case.inputs(int(fixture["seed"]))
    w = torch.randn(q.shape, generator=torch.Generator().manual_seed(3))
    fused = case.module(AdaPoinTr, "a").cuda()
    HF._declined.clear()
    out, g, lists = _grads(fused, q.cuda(), v.cuda(), q_pos.cuda(), v_pos.cuda(), w.cuda())
    assert not HF._declined, HF._declined
    lists = tuple(t.cpu() for t in lists)
    assert lists[0].shape == lists[1].shape == (case.B, case.NQ, case.K) and int(lists[0][:, :case.NQ - case.D].max()) < case.NQ - case.D
    m32 = case.module(AdaPoinTr, "a")
    out32, g32, _ = _grads(m32, q, v, q_pos, v_pos, w, lists)
    m64 = copy.deepcopy(m32).double()
    out64, g64, _ = _grads(m64, q.double(), v.double(), q_pos.double(), v_pos.double(), w.double(), lists)
    assert set(g) == set(g64) and len(g) == 2 + len(list(fused.parameters())) and all(t is not None for t in g.values())
    _check_against("forward", out.cpu(), out32, out64, 1e-5, 2e-6)
    for name in sorted(g):
        _check_against(name, g[name].cpu(), g32[name], g64[name], 2e-5, 5e-6)


def test_fused_decoder_launches_no_library_gemm_softmax_mask_or_topk(fixture):
    x = [t.cuda() for t in case.inputs(int(fixture["seed"]))]
    w = torch.randn(x[0].shape, device='cuda')
    m = case.module(AdaPoinTr, "a").cuda()
    _grads(m, *x, w)                                                    # (warm-up: caches, lazy initialisation)
    HF._declined.clear()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        _grads(m, *x, w)
        torch.cuda.synchronize()
    assert not HF._declined, HF._declined
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    print("\n".join(names))
    for n in names:
        low = n.lower()
        assert "Cijk_" not in n and "gemm" not in low and "softmax" not in low and "topk" not in low, n
        assert "masked_fill" not in low and "where" not in low, n
    for frag in ("xattn_prefix_fwd_kernel", "xattn_prefix_bwd_kv_kernel", "xattn_prefix_bwd_q_kernel", "xattn_fwd_kernel", "ec_"):
        assert any(frag in n for n in names), frag


def _reference_mask(N, D, device):
    mask = torch.zeros(N, N, device=device)
    mask[:-D, -D:] = 1.
    return mask


def test_declined_list_is_empty_when_fused_and_names_the_site_for_a_mask_tensor(fixture):
    q, v, q_pos, v_pos = (t.cuda() for t in case.inputs(int(fixture["seed"])))
    block = case.module(AdaPoinTr, "d").cuda()
    HF._declined.clear()
    with torch.no_grad():
        block(q, v, q_pos, v_pos, denoise_length=case.D)
    assert not HF._declined, HF._declined
    attn = block.self_attn
    with torch.no_grad():
        out = attn(q, mask=_reference_mask(case.NQ, case.D, 'cuda'))
    assert out.shape == q.shape and torch.isfinite(out).all()
    sites = [what for what, why in HF._declined]
    assert len(sites) == 1 and sites[0].startswith("Attention") and "mask tensor" in sites[0], HF._declined
    HF._declined.clear()


def test_attention_with_denoise_length_equals_attention_with_the_references_mask(fixture):
    q = case.inputs(int(fixture["seed"]))[0]
    attn = _seeded.fill(Transformer_utils.Attention(case.DIM, num_heads=case.HEADS)).eval()
    with torch.no_grad():
        f64 = copy.deepcopy(attn).double()(q.double(), mask=_reference_mask(case.NQ, case.D, 'cpu'))
        fused = copy.deepcopy(attn).cuda()
        HF._declined.clear()
        got = fused(q.cuda(), denoise_length=case.D)
        assert not HF._declined, HF._declined
        t32 = fused(q.cuda(), mask=_reference_mask(case.NQ, case.D, 'cuda'))
        plain = fused(q.cuda())
    HF._declined.clear()
    _check_against("Attention(denoise_length) against Attention(mask)", got.cpu(), t32.cpu(), f64, 1e-5, 2e-6)
    assert not torch.equal(got[:, :case.NQ - case.D], plain[:, :case.NQ - case.D])      # the mask does something: the real rows lose 8 keys
