"""What the attention-core tests share (tests/test_gpu_attention_short.py: 1 ... 160 tokens, tests/test_gpu_attention_stream.py: 161 ...
ATTN_MAX_L): the torch formulation in f32 / f64, the kernels' forward + backward, and the project's bounds with their float64 arbitration."""
import numpy as np
import torch

from upp_hip import ops

SCALE = 0.125


def close(a, b, rtol=1e-5, atol_scale=2e-6):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol_scale * max(np.abs(b).max(), 1e-30))


def _inside(a, ref, rtol, atol_scale):
    ref = ref.double()
    return bool(((a.double() - ref).abs() <= atol_scale * ref.abs().max() + rtol * ref.abs()).all())


def _err(a, ref):
    return ((a.double() - ref.double()).abs().max() / ref.double().abs().max()).item()


def _torch_formulation(qkv, w, H, dtype):
    """reference models/Point_MAE_pretask_dev.py:186-193 and its autograd -> out, d_qkv, lse"""
    B, L, _ = qkv.shape
    x = qkv.detach().to(dtype).requires_grad_(True)
    q, k, v = x.view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * SCALE
    out = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, L, H * 64)
    (out * w.to(dtype)).sum().backward()
    return out.detach(), x.grad, torch.logsumexp(s.detach(), -1)


def _kernels(qkv, w, H):
    B, L, _ = qkv.shape
    out, lse = ops.attn_fwd(qkv, B, L, H, SCALE)
    return out, ops.attn_bwd(qkv, out, w, lse, B, L, H, SCALE), lse


def _check_against(name, got, t32, f64, rtol, atol_scale):
    """the project's bound against the torch formulation where that is itself inside it against float64; else the float64 arbitration"""
    e_k, e_t = _err(got, f64), _err(t32, f64)
    own = _inside(t32, f64, rtol, atol_scale)
    print("%s: kernel %.2e torch_f32 %.2e of max|f64| (%s)" % (name, e_k, e_t, "project bound against torch" if own else "float64 arbitration"))
    if own:
        close(got, t32, rtol=rtol, atol_scale=atol_scale)
    else:
        scale = f64.abs().max().item()
        assert e_k * scale <= 2 * e_t * scale + 2e-6 * scale, (name, e_k, e_t)


def _memsets(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if "memset" in e.name.lower()]
