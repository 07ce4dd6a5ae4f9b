"""The streaming attention kernels (csrc/attn_stream.hip, 161 ... ATTN_MAX_L tokens): parity with the torch formulation and float64, the
hazards of an online softmax, isolation of the tail rows, determinism, dispatch below and above the old cap, graph capture, and the
fused block / model paths that the longer range opens.

Parity bounds are those of tests/test_gpu_block.py (forward rtol 1e-5, atol 2e-6 max|ref|; gradient rtol 2e-5, atol 5e-6 max|ref|)
against the torch f32 formulation wherever that formulation itself stays inside them against float64; where it does not, the float64
arbitration of the step-tail tests applies: max|kernel - f64| <= 2 max|torch_f32 - f64| + 2e-6 max|f64|.

Measured on MI355X, max|x - f64| / max|f64| of (kernel, torch f32), forward | gradient | lse (absolute):
    L      forward               gradient              lse
    161    4.9e-7, 5.8e-7        5.5e-7, 5.2e-7        7.2e-7, 6.9e-7
    191    7.9e-7, 8.7e-7        7.8e-7, 7.2e-7        6.9e-7, 6.7e-7
    192    8.0e-7, 9.7e-7        8.5e-7, 9.5e-7        6.5e-7, 7.0e-7
    193    6.2e-7, 6.4e-7        7.8e-7, 6.9e-7        6.9e-7, 7.1e-7
    255    4.4e-7, 6.2e-7        6.8e-7, 6.1e-7        7.1e-7, 7.3e-7
    256    7.7e-7, 6.8e-7        1.25e-6, 1.17e-6      7.4e-7, 7.4e-7
    257    6.2e-7, 7.1e-7        7.1e-7, 5.6e-7        8.1e-7, 7.3e-7
    320    7.8e-7, 1.28e-6       6.8e-7, 7.9e-7        7.5e-7, 7.1e-7
    513    8.1e-7, 6.5e-7        8.7e-7, 6.7e-7        7.4e-7, 8.7e-7
    1025   1.53e-6, 1.00e-6      1.08e-6, 9.1e-7       8.5e-7, 8.0e-7
    2048   1.33e-6, 1.64e-6      1.74e-6, 1.57e-6      1.12e-6, 1.07e-6
The torch f32 formulation stayed inside the project's bounds against float64 at every one of these lengths, 2048 included, so the
project's bounds against it applied everywhere and the float64 arbitration never had to.  Hazard cases (kernel, torch f32): sharp
5.2e-6, 4.4e-6 | 4.3e-6, 5.3e-6; max_last 1.03e-5, 1.06e-5 | 4.6e-6, 6.2e-6; max_first 1.11e-5, 1.01e-5 | 8.7e-6, 8.0e-6; constant_row
8.4e-7, 9.0e-7 | 1.01e-6, 6.9e-7.
"""
import functools

import numpy as np
import pytest
import torch

import _seeded
from _attention_reference import _check_against, _err, _kernels, _memsets, _torch_formulation, close
from models import build_model_from_cfg, upp_layers
from upp_hip import functional as HF, ops
from utils.config import builtin_cfg

pytestmark = pytest.mark.gpu

MAX_L = ops.ATTN_MAX_L
# one past the old cap; both sides of every 64-row block edge that matters (one tail row / one tail key at 193, 257, 513, 1025); many blocks
LENGTHS = [161, 191, 192, 193, 255, 256, 257, 320, 513, 1025, MAX_L]


@functools.lru_cache(maxsize=None)
def _case(L):
    B, H = (3, 2) if L < 1024 else (2, 2)
    g = torch.Generator(device='cuda').manual_seed(L)
    qkv = torch.randn(B, L, 3 * H * 64, device='cuda', generator=g)
    w = torch.randn(B, L, H * 64, device='cuda', generator=g)
    return qkv, w, H, _torch_formulation(qkv, w, H, torch.float32), _torch_formulation(qkv, w, H, torch.float64)


@pytest.mark.parametrize("L", LENGTHS)
def test_parity_with_the_torch_formulation_and_float64(L):
    qkv, w, H, t32, f64 = _case(L)
    out, g, lse = _kernels(qkv, w, H)
    print("L = %d" % L)
    e_lse = (lse.double() - f64[2]).abs().max().item()
    print("lse: kernel %.2e torch_f32 %.2e (absolute)" % (e_lse, (t32[2].double() - f64[2]).abs().max().item()))
    assert torch.isfinite(out).all() and torch.isfinite(g).all() and torch.isfinite(lse).all()
    _check_against("forward", out, t32[0], f64[0], 1e-5, 2e-6)
    _check_against("gradient", g, t32[1], f64[1], 2e-5, 5e-6)
    # lse = m + log l: a few roundings of numbers of size |lse| <= ~10 (f32 epsilon 6e-8) plus the relative error of l (~1e-6)
    np.testing.assert_allclose(lse.cpu().numpy(), f64[2].cpu().numpy(), rtol=2e-6, atol=2e-6)


def _hazard(kind):
    B, L, H = 2, 300, 2                              # key blocks 0-63, ..., 192-255, 256-299
    g = torch.Generator(device='cuda').manual_seed(7)
    x = torch.randn(B, L, 3, H, 64, device='cuda', generator=g)
    if kind == "sharp":                               # q.k * 0.125 with q, k ~ N(0, 16): scores of standard deviation 16, nearly one-hot rows
        x[:, :, 0:2] *= 4.0
    elif kind in ("max_last", "max_first"):          # channel 0 puts +32 on the keys of one block and -32 on every other key
        x[:, :, 0, :, 0] = 16.0
        x[:, :, 1, :, 0] = -16.0
        blk = slice(256, L) if kind == "max_last" else slice(0, 64)
        x[:, blk, 1, :, 0] = 16.0
    else:                                             # one query row of zeros: a constant score row, uniform softmax
        x[0, 5, 0] = 0.0
        x[1, L - 1, 0] = 0.0
    return x.view(B, L, 3 * H * 64).contiguous(), torch.randn(B, L, H * 64, device='cuda', generator=g), H


@pytest.mark.parametrize("kind", ["sharp", "max_last", "max_first", "constant_row"])
def test_online_softmax_hazards_against_float64(kind):
    qkv, w, H = _hazard(kind)
    out, g, lse = _kernels(qkv, w, H)
    assert torch.isfinite(out).all() and torch.isfinite(g).all() and torch.isfinite(lse).all()
    t32, f64 = _torch_formulation(qkv, w, H, torch.float32), _torch_formulation(qkv, w, H, torch.float64)
    # the kernel may be as far from float64 as twice the torch f32 formulation on the same inputs, plus the project's absolute terms
    for name, a, i, atol in (("forward", out, 0, 2e-6), ("gradient", g, 1, 5e-6)):
        e_k, e_t = _err(a, f64[i]), _err(t32[i], f64[i])
        print("%s %s: kernel %.2e torch_f32 %.2e of max|f64|" % (kind, name, e_k, e_t))
        assert e_k <= 2 * e_t + atol, (kind, name, e_k, e_t)
    e_lse = ((lse.double() - f64[2]).abs() / f64[2].abs().clamp_min(1.0)).max().item()
    print("%s lse: %.2e" % (kind, e_lse))
    assert e_lse <= 4e-6                               # relative to |lse| (up to ~100 in the sharp case) where that exceeds 1
    if kind == "constant_row":
        v = qkv.view(2, 300, 3, H, 64)[0, :, 2].double().mean(0).reshape(-1)         # uniform softmax: the mean of V
        assert (out[0, 5].double() - v).abs().max().item() <= 2e-6 * f64[0].abs().max().item()
        assert (lse[0, :, 5].double() - np.log(300.0)).abs().max().item() <= 2e-6


def test_rows_behind_the_last_token_are_never_read():
    B, L, H = 2, 257, 2                               # the last query block holds ONE row, the last key block one key
    g = torch.Generator(device='cuda').manual_seed(11)
    n, nw = B * L * 3 * H * 64, B * L * H * 64
    big = torch.full((n + 64 * 3 * H * 64,), float('nan'), device='cuda')
    bigw = torch.full((nw + 64 * H * 64,), float('nan'), device='cuda')
    big[:n] = torch.randn(n, device='cuda', generator=g)
    bigw[:nw] = torch.randn(nw, device='cuda', generator=g)
    qkv, w = big[:n].view(B, L, 3 * H * 64), bigw[:nw].view(B, L, H * 64)
    assert qkv.is_contiguous() and qkv.data_ptr() == big.data_ptr()
    got = _kernels(qkv, w, H)
    exact = _kernels(qkv.clone(), w.clone(), H)
    for a, b in zip(got, exact):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


@pytest.mark.parametrize("L", [257, 513])
def test_two_runs_give_the_same_bits(L):
    qkv, w, H = _case(L)[:3]
    first = [t.clone() for t in _kernels(qkv, w, H)]
    for a, b in zip(first, _kernels(qkv, w, H)):
        assert torch.equal(a, b)


def _kernel_names(fn):
    fn()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages()]


@pytest.mark.parametrize("L, family, others", [
    (96, ("attn_fwd16_kernel", "attn_bwd16"), ("long_kernel", "attn_stream")),
    (97, ("attn_fwd_long_kernel", "attn_bwd_long_kernel"), ("attn_fwd16", "attn_bwd16", "attn_stream")),
    (160, ("attn_fwd_long_kernel", "attn_bwd_long_kernel"), ("attn_fwd16", "attn_bwd16", "attn_stream")),
    (161, ("attn_stream_fwd_kernel", "attn_stream_bwd_kv_kernel", "attn_stream_bwd_q_kernel"), ("attn_fwd16", "attn_bwd16", "long_kernel")),
])
def test_each_length_launches_its_own_kernel_family(L, family, others):
    qkv = torch.randn(2, L, 3 * 2 * 64, device='cuda')
    w = torch.randn(2, L, 2 * 64, device='cuda')
    names = _kernel_names(lambda: _kernels(qkv, w, 2))
    for k in family:
        assert any(k in n for n in names), (k, names)
    for k in others:
        assert not any(k in n for n in names), (k, names)


def test_captured_forward_and_backward_replay_the_eager_bits_without_a_memset():
    qkv, w, H = _case(257)[:3]
    eager = [t.clone() for t in _kernels(qkv, w, H)]
    assert not _memsets(lambda: _kernels(qkv, w, H))       # (what a capture would turn into memset nodes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _kernels(qkv, w, H)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _kernels(qkv, w, H)
    for _ in range(3):
        for t in captured:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(a, b)


def _no_fused_paths(monkeypatch):
    monkeypatch.setattr(upp_layers.Block, "fusable", lambda self, x: False)
    monkeypatch.setattr(upp_layers.Attention, "fusable", lambda self, x: False)


def test_encoder_blocks_take_the_fused_path_at_257_tokens(monkeypatch):
    torch.manual_seed(3)
    enc = _seeded.fill(upp_layers.TransformerEncoder(embed_dim=384, depth=2, num_heads=6)).cuda().eval()
    params = []
    for n, p in enc.named_parameters():
        p.requires_grad_('.norm1.' in n or '.norm2.' in n)         # (the blocks' two LayerNorms; bnorm belongs to the propagation step)
        if p.requires_grad:
            params.append(p)
    x = torch.randn(2, 257, 384, device='cuda')
    pos = torch.randn(2, 257, 384, device='cuda')
    assert all(b.fusable(x) for b in enc.blocks)

    def run():
        xi = x.clone().requires_grad_(True)
        out = enc(xi, pos, path='downstream')
        wgt = torch.linspace(-1, 1, out.numel(), device='cuda').view_as(out)
        return [out.detach()] + list(torch.autograd.grad((out * wgt).sum(), [xi] + params))

    names = _kernel_names(run)
    assert any("attn_stream" in n for n in names), names
    assert not [n for n in names if n.startswith('Cijk')], [n for n in names if n.startswith('Cijk')]
    fused = run()
    _no_fused_paths(monkeypatch)
    assert not enc.blocks[0].fusable(x)
    unfused = run()
    close(fused[0], unfused[0])
    for a, b in zip(fused[1:], unfused[1:]):
        close(a, b, rtol=2e-5, atol_scale=5e-6)


PEFT_KEYS = ['downstream_adapter', 'downstream_adapter1', 'downstream_prompts', 'bnorm', 'cls_pos', 'cls_token', 'cls_head_finetune']
# (site, reason) pairs that run on torch at 192 groups: the one-launch index build of the prompt propagation serves G2 = num_group / 2 <= 64
# level-2 centres (csrc/prop.hip upp_prop_index); the propagation kernels themselves run.
DOCUMENTED_DECLINES = {("prompt propagation index", "more than 64 level-2 centres / indices not int64")}


def test_a_192_group_model_trains_on_the_fused_path(monkeypatch):
    """One eager forward + loss + backward of Point_MAE_unify with 192 groups on 2048-point clouds (203 tokens in the prompted blocks), as
    tests/test_gpu_model.py::test_train_step_gradients_match_fixture runs it (eval mode: the fused and the unfused path draw their
    dropout masks differently), against the same step with every `fusable` predicate false.

    The propagation step max-pools 8 neighbour rows per (level-2 centre, channel): 6 blocks x 192 x 384 discrete choices, and the two
    runs differ by f32 rounding in what they pool.  Measured on MI355X: ONE of those 442,368 choices falls the other way in the unfused
    run, which re-routes that channel's gradient: 6 of the 102 gradient arrays then leave the bound, by up to 7.5e-5 of their scale (the
    same with only the attention core swapped for the torch formulation; at 64 groups, where no choice flips, 2.2e-6).  So the reference
    run is given the fused run's choices -- what POOL_TRACE does for the float64 comparisons of tests/test_gpu_model.py -- and
    the bounds stay those of that file: with the choices pinned the worst array is 2.8e-6 of its scale away."""
    cfg = builtin_cfg('unify_modelnet_cls').model
    cfg.num_group = 192
    m = _seeded.fill(build_model_from_cfg(cfg)).eval().cuda()
    for n, p in m.named_parameters():
        p.requires_grad_(any(k in n for k in PEFT_KEYS))
    x = _seeded.noisy_clouds(2, 2048, seed=0).cuda()
    y = torch.tensor([1, 2], device='cuda')

    def step():
        for p in m.parameters():
            p.grad = None
        loss, _ = m.get_loss_acc(m(x, completion_prompt=True, denoise=True, point_num=2048), y)
        loss.backward()
        return loss.item(), {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad and p.grad is not None}

    choices, flipped = [], []
    group_max_fwd = ops.group_max_fwd

    def recording(fwd, amax_at):
        def wrapped(*a, **k):
            out = fwd(*a, **k)
            choices.append(out[amax_at].clone())        # arg-max (B * G2, D) of the fused propagation's pool
            return out
        return wrapped

    def replaying_group_max_fwd(xg, *a, **k):
        out, amax = group_max_fwd(xg, *a, **k)
        if choices and tuple(xg.shape) == (choices[0].shape[0], 8, choices[0].shape[1]):      # the same pool on the unfused path
            pinned = choices.pop(0)
            flipped.append((pinned != amax).sum().item())
            amax = pinned
        return out, amax

    HF._declined.clear()
    with monkeypatch.context() as mp:                   # the pool of the fused step, and of its residual / tail form
        mp.setattr(ops, "prop_fwd", recording(ops.prop_fwd, 2))
        mp.setattr(ops, "prop_res_pool_fwd", recording(ops.prop_res_pool_fwd, 1))
        loss, grads = step()
    declined = set(HF._declined)
    assert len(choices) == 6                           # the six prompted blocks
    per_pool = choices[0].numel()
    _no_fused_paths(monkeypatch)
    monkeypatch.setattr(ops, "group_max_fwd", replaying_group_max_fwd)
    ref_loss, ref = step()
    print("pool choices that differ between the runs:", flipped)
    assert not choices and len(flipped) == 6 and max(flipped) <= per_pool // 10000       # (the same pools in the same layout: near-ties only)
    assert np.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())
    assert sorted(grads) == sorted(ref)
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-5)
    names = sorted(grads)
    np.testing.assert_allclose([grads[n].norm().item() for n in names], [ref[n].norm().item() for n in names], rtol=2e-5, atol=1e-7)
    worst = max(((grads[n].double() - ref[n].double()).abs().max() / ref[n].double().abs().max()).item() for n in names)
    print("worst gradient array: %.2e of its scale" % worst)
    for n in names:
        r = ref[n].cpu().numpy()
        np.testing.assert_allclose(grads[n].cpu().numpy(), r, rtol=2e-4, atol=1e-5 * np.abs(r).max(), err_msg=n)
    assert declined == DOCUMENTED_DECLINES, declined
