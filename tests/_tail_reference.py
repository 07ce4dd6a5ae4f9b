"""Plain torch reference of the block tail: the row kernels of csrc/block.hip (row map + residual + LayerNorm), the bottleneck adapter of
csrc/adapter.hip and their composition (the fused tail), forward AND backward, with the gradients written out -- no autograd, none of
the project's kernels.  One set of functions evaluates the formulation in any dtype on any device, so the same code is the float64
arbiter and the float32 yardstick of tests/test_gpu_tail.py; tests/test_tail_host.py checks it against torch autograd of the plain
formulation (torch.cat, F.layer_norm, F.linear, F.gelu) on the CPU.

    rows = map(x + add, prompts) + f_b * (y + ybias)          f_b = floor(keep + u_b) / keep; prompt rows take no residual
    ha   = LayerNorm(rows) = (rows - mean) * rstd * gamma + beta,   rstd = 1 / sqrt(var + eps), biased variance
    out  = x + s * (W2 . (gelu(W1 . ha + b1) * m) + b2)       m = (ud >= p) / (1 - p); GELU in its erf form
    tail = the adapter applied to (ha, x = rows)

Three rules keep a float64 run faithful to what the kernels see: floor(keep + u) and ud >= p are SELECTIONS taken on the float32
values with keep and p rounded to float32 first (drop_select, dropout_select), shared by every dtype; keep and p enter the arithmetic
as those float32 values.
"""
import numpy as np
import torch

IDENTITY, INSERT_CLS, INSERT, STRIP_CLS, STRIP = 0, 1, 2, 3, 4
H = 32          # bottleneck width of the adapter


def f32(v):
    """A scalar as the kernels receive it (a C float), as a Python float."""
    return float(np.float32(v))


def lout(mode, Lin, P):
    return Lin + P if mode in (INSERT_CLS, INSERT) else (Lin - P if mode in (STRIP_CLS, STRIP) else Lin)


def row_sources(mode, P, Lout):
    """For every output row t its source: -> (t_tok, s_tok, t_pr, p_pr), output rows that copy token row s, and those that copy prompt p.
    Layouts [cls | prompts | tokens] (INSERT_CLS / STRIP_CLS) or [prompts | tokens] (INSERT / STRIP)."""
    t_tok, s_tok, t_pr, p_pr = [], [], [], []
    for t in range(Lout):
        if mode == INSERT_CLS:
            s = 0 if t == 0 else (-t if t <= P else t - P)
        elif mode == INSERT:
            s = -(t + 1) if t < P else t - P
        elif mode == STRIP_CLS:
            s = 0 if t == 0 else t + P
        elif mode == STRIP:
            s = t + P
        else:
            s = t
        if s >= 0:
            t_tok.append(t); s_tok.append(s)
        else:
            t_pr.append(t); p_pr.append(-s - 1)
    return t_tok, s_tok, t_pr, p_pr


def drop_select(u, keep):
    """floor(keep + u) in float32 (0 or 1 per sample): the kernel's arithmetic, a selection."""
    return np.floor(np.float32(keep) + np.asarray(u, dtype=np.float32)).astype(np.float32)


def drop_factor(u, keep, B, dtype, device):
    """f (B,) in `dtype`; ones without u."""
    if u is None:
        return torch.ones(B, dtype=dtype, device=device)
    s = torch.from_numpy(drop_select(u.detach().cpu().numpy(), keep)).to(device=device, dtype=dtype)
    return s / f32(keep)


def dropout_select(ud, p):
    """ud >= p on the float32 values (1 keeps the element; ud == float32(p) keeps it)."""
    return (np.asarray(ud, dtype=np.float32) >= np.float32(p)).astype(np.float32)


def dropout_mask(ud, p, dtype, device):
    """m (R, H) in `dtype`, or None without uniforms."""
    if ud is None:
        return None
    s = torch.from_numpy(dropout_select(ud.detach().cpu().numpy(), p)).to(device=device, dtype=dtype)
    return s / (1.0 - f32(p))


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gelu_grad(x):
    """d/dx [x Phi(x)] = Phi(x) + x phi(x)"""
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


def _idx(v, device):
    return torch.tensor(v, dtype=torch.long, device=device)


# ---------------------------------------------------------------------------------------------- rows
def rows_fwd(x, add, prompts, y, ybias, f, mode, P):
    """-> rows (B, Lout, D)."""
    B, Lin, D = x.shape
    Lo = lout(mode, Lin, P)
    t_tok, s_tok, t_pr, p_pr = row_sources(mode, P, Lo)
    src = x if add is None else x + add
    if y is not None:
        src = src + f.view(B, 1, 1) * (y if ybias is None else y + ybias)
    rows = torch.zeros(B, Lo, D, dtype=x.dtype, device=x.device)
    rows[:, _idx(t_tok, x.device)] = src[:, _idx(s_tok, x.device)]
    if t_pr:
        rows[:, _idx(t_pr, x.device)] = prompts[_idx(p_pr, x.device)].unsqueeze(0).expand(B, -1, -1)
    return rows


def rows_bwd(g_rows, f, mode, P, Lin, has_y):
    """Gradient of rows_fwd: g_x (= g_add) and g_y (B, Lin, D) -- exact zeros in the rows a strip map drops --, the per-sample prompt
    gradient (B, P, D) and its batch sum."""
    B, Lo, D = g_rows.shape
    t_tok, s_tok, t_pr, p_pr = row_sources(mode, P, Lo)
    dev = g_rows.device
    g_x = torch.zeros(B, Lin, D, dtype=g_rows.dtype, device=dev)
    g_x[:, _idx(s_tok, dev)] = g_rows[:, _idx(t_tok, dev)]
    res = dict(g_x=g_x, g_y=(g_x * f.view(B, 1, 1)) if has_y else None, g_prompt_b=None, g_prompt=None)
    if t_pr:
        gp = torch.zeros(B, P, D, dtype=g_rows.dtype, device=dev)
        gp[:, _idx(p_pr, dev)] = g_rows[:, _idx(t_pr, dev)]
        res.update(g_prompt_b=gp, g_prompt=gp.sum(dim=0))
    return res


def ln_fwd(rows, gamma, beta, eps):
    """-> (h, mean, rstd) over the last dimension."""
    mean = rows.mean(dim=-1, keepdim=True)
    var = ((rows - mean) ** 2).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (rows - mean) * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def ln_bwd(g_h, rows, mean, rstd, gamma):
    """-> (g_rows, g_gamma, g_beta):  dx = rstd (dy - mean(dy) - xhat mean(dy xhat)),  dy = g_h gamma."""
    xh = (rows - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    dy = g_h * gamma
    dx = rstd.unsqueeze(-1) * (dy - dy.mean(dim=-1, keepdim=True) - xh * (dy * xh).mean(dim=-1, keepdim=True))
    D = rows.shape[-1]
    return dx, (g_h * xh).reshape(-1, D).sum(dim=0), g_h.reshape(-1, D).sum(dim=0)


# ---------------------------------------------------------------------------------------------- adapter
def adapter_fwd(ha, x, W1, b1, W2, b2, m, s):
    """ha, x (R, D) -> (out (R, D), s1 (R, H))."""
    s1 = ha @ W1.t() + b1
    gq = gelu(s1) if m is None else gelu(s1) * m
    return x + s * (gq @ W2.t() + b2), s1


def adapter_bwd(g_out, ha, s1, W1, W2, m, s):
    """The per-row factors ga = gd * m * gelu'(s1), d = s * gelu(s1) * m, and from them every gradient."""
    one = torch.ones_like(s1) if m is None else m
    gd = (s * g_out) @ W2
    ga = gd * one * gelu_grad(s1)
    d = s * gelu(s1) * one
    return dict(g_ha=ga @ W1, g_x=g_out, g_W1=ga.t() @ ha, g_b1=ga.sum(dim=0), g_W2=g_out.t() @ d, g_b2=s * g_out.sum(dim=0), ga=ga, d=d)


# ---------------------------------------------------------------------------------------------- whole operators, converted inputs
def _cv(t, dtype, device):
    return None if t is None else t.detach().to(device=device, dtype=dtype)


def _f64(res):
    return {k: (None if v is None else v.detach().double()) for k, v in res.items()}


def rowln(x, add, prompts, y, ybias, u, keep, gamma, beta, eps, mode, P, g_xo, g_h, dtype, device=None):
    """The row kernel pair in `dtype`: rows, LayerNorm (gamma None: rows only) and the gradients of sum(rows * g_xo) + sum(h * g_h)
    (either may be None).  -> dict of float64 tensors: xo, h, mean, rstd, g_x, g_y, g_prompt_b, g_prompt, g_gamma, g_beta."""
    device = device or x.device
    x_, add_, pr_, y_, yb_, gm_, bt_, gxo, gh = (_cv(t, dtype, device) for t in (x, add, prompts, y, ybias, gamma, beta, g_xo, g_h))
    B, Lin, D = x_.shape
    f = drop_factor(u if y is not None else None, keep, B, dtype, device)
    rows = rows_fwd(x_, add_, pr_, y_, yb_, f, mode, P)
    res = dict(xo=rows, h=None, mean=None, rstd=None, g_gamma=None, g_beta=None)
    g_rows = torch.zeros_like(rows) if gxo is None else gxo.clone()
    if gm_ is not None:
        h, mean, rstd = ln_fwd(rows, gm_, bt_, eps)
        res.update(h=h, mean=mean, rstd=rstd)
        if gh is not None:
            dx, gg, gb = ln_bwd(gh, rows, mean, rstd, gm_)
            g_rows = g_rows + dx
            res.update(g_gamma=gg, g_beta=gb)
    res.update(rows_bwd(g_rows, f, mode, P, Lin, y is not None))
    return _f64(res)


def adapter(ha, x, W1, b1, W2, b2, ud, p, s, g_out, dtype, device=None):
    """The adapter pair in `dtype` -> dict of float64 tensors: out, s1, g_ha, g_x, g_W1, g_b1, g_W2, g_b2, ga, d."""
    device = device or ha.device
    ha_, x_, W1_, b1_, W2_, b2_, go = (_cv(t, dtype, device) for t in (ha, x, W1, b1, W2, b2, g_out))
    m = dropout_mask(ud, p, dtype, device)
    out, s1 = adapter_fwd(ha_, x_, W1_, b1_, W2_, b2_, m, f32(s))
    res = adapter_bwd(go, ha_, s1, W1_, W2_, m, f32(s))
    res.update(out=out, s1=s1)
    return _f64(res)


def tail(x, y, ybias, u, keep, mode, P, gamma, beta, eps, W1, b1, W2, b2, ud, p, s, g_out, dtype, device=None):
    """The fused tail in `dtype` (ha is never an output) -> dict of float64 tensors: out, xo, mean, rstd, s1, g_x, g_y, g_gamma, g_beta,
    g_W1, g_b1, g_W2, g_b2, fac (R, 2 H) = [ga | d]."""
    device = device or x.device
    x_, y_, yb_, gm_, bt_, W1_, b1_, W2_, b2_, go = (_cv(t, dtype, device) for t in (x, y, ybias, gamma, beta, W1, b1, W2, b2, g_out))
    B, Lin, D = x_.shape
    f = drop_factor(u if y is not None else None, keep, B, dtype, device)
    rows = rows_fwd(x_, None, None, y_, yb_, f, mode, P)
    Lo = rows.shape[1]
    ha, mean, rstd = ln_fwd(rows, gm_, bt_, eps)
    m = dropout_mask(ud, p, dtype, device)
    out, s1 = adapter_fwd(ha.reshape(-1, D), rows.reshape(-1, D), W1_, b1_, W2_, b2_, m, f32(s))
    a = adapter_bwd(go.reshape(-1, D), ha.reshape(-1, D), s1, W1_, W2_, m, f32(s))
    dx, gg, gb = ln_bwd(a['g_ha'].view(B, Lo, D), rows, mean, rstd, gm_)
    r = rows_bwd(go.view(B, Lo, D) + dx, f, mode, P, Lin, y is not None)
    return _f64(dict(out=out.view(B, Lo, D), xo=rows, mean=mean, rstd=rstd, s1=s1, g_x=r['g_x'], g_y=r['g_y'], g_gamma=gg, g_beta=gb,
                     g_W1=a['g_W1'], g_b1=a['g_b1'], g_W2=a['g_W2'], g_b2=a['g_b2'], fac=torch.cat([a['ga'], a['d']], dim=1)))
