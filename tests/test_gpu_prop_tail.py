"""A prompted block's MLP residual + prompt propagation + tail in 7 launches (HF.prop_tail: upp_prop_res_pool_fwd,
upp_ln_adapter_prop_fwd, upp_prop_res_bwd) against the 10 launches it replaces, bit for bit.

The replaced composition is  rowln (x3 = x2 + dp (m + mb))  ->  propagate (pool + statistics | finalize | interpolate)  ->
ln_adapter (strip + LayerNorm + adapter)  and, backward,  ln_adapter_bwd_fused -> prop_bwd -> rowln_bwd.  The new kernels perform the
same operations in the same order (the library is built without floating-point contraction), so every comparison here is torch.equal:
pooled, amax, the (sum, M2) partials, the BatchNorm statistics and running statistics, the tail's rows / mean / rstd / s1 / output;
the gradients of x2, m, the BatchNorm, the adapter's LayerNorm and the adapter.  The composition itself is judged against float64 in
test_gpu_prop.py / test_gpu_tail.py / test_gpu_rows.py.

Shapes are the smallest at which the kernels take each of their paths: B = 2 and 3; T = 8 / G2 = 4 and T = 64 / G2 = 32; P = 1 and 10, with
and without the cls row; B * Lout = 24 and 39 (no multiple of the tail's 16-row workgroup) and 130; groups = 8, 12 (a multiple of 4) and
64; D = 384 and, for the two kernels that are not tied to it, D = 64.  The lists are random over ALL rows of a sample (prompt rows and the
cls row included, a row several times in one group) or come from build_prop_index in both index conventions (flat: rows of other samples).
"""
import types

import pytest
import torch

from models import upp_layers
from test_gpu_prop import EPS, MOM
from upp_hip import _abi, ops
from upp_hip import functional as HF

pytestmark = pytest.mark.gpu

KEEP_DP, KEEP_G = 0.8, 0.9


def make_case(B, cls, P, T, G2, D, training, dp, bias, pd, seed, lists="random"):
    """dp: None (no drop path) | 'u' (uniforms; sample 0 dropped: factor 0, the last sample kept: factor 1 / keep)."""
    g = torch.Generator().manual_seed(seed)
    lead = (1 if cls else 0) + P
    Lp = lead + T
    c = types.SimpleNamespace(B=B, cls=cls, P=P, T=T, G2=G2, D=D, Lp=Lp, Lout=Lp - P, rows=B * Lp, groups=B * G2, training=training, pd=pd,
                              mode=HF.ROW_STRIP_CLS if cls else HF.ROW_STRIP)
    c.x2 = torch.randn(B, Lp, D, generator=g) * 0.7 + 0.3
    c.m = torch.randn(B, Lp, D, generator=g) * 0.5
    c.mb = torch.randn(D, generator=g) * 0.1 if bias else None
    if dp:
        c.u_dp = torch.rand(B, generator=g)
        c.u_dp[0], c.u_dp[B - 1] = 0.05, 0.95                    # floor(0.8 + 0.05) = 0: the sample's branch is dropped
        c.keep_dp = KEEP_DP
        c.u_g, c.keep_g = torch.rand(B * G2, generator=g), KEEP_G
    else:
        c.u_dp, c.keep_dp, c.u_g, c.keep_g = None, 1.0, None, 1.0
    if lists == "random":
        base = (torch.arange(B) * Lp).view(B, 1)
        i1 = base + torch.randint(0, Lp, (B, G2 * 8), generator=g)
        i1[:, 1] = i1[:, 0]                                      # group 0 of every sample lists one row twice ...
        i1[:, 8:16] = i1[:, 8:9]                                 # ... and group 1 one row eight times
        i1[0, 17], i1[B - 1, 18] = 0, (B - 1) * Lp + lead - 1    # the first row of all (cls or a prompt) and a prompt row, for certain
        c.i1 = i1.reshape(-1).int()
        c.i2 = (base + torch.randint(0, Lp, (B, G2), generator=g)).reshape(-1).int()
        c.i2[1] = lead - 1                                       # a level-2 centre whose own token is a prompt row
        c.idx8 = torch.randint(0, G2, (B, T, 8), generator=g).int()
        w8 = torch.rand(B, T, 8, generator=g) + 0.05
        c.w8 = w8 / w8.sum(-1, keepdim=True)
    else:                                                        # the model's lists: 'flat' (batch offsets b * T into rows of stride Lp - off) | 'gather'
        c1 = torch.rand(B, T, 3, generator=g).cuda() * 2 - 1
        _, c2, i1, i2 = upp_layers.Group(G2, 8)(c1, require_index=True, gather_idx=lists == "gather")
        index = upp_layers.build_prop_index(c1, c2, i1, i2, lists == "gather", B, Lp, 1 if cls else 0)
        c.i1, c.i2, c.idx8, c.w8 = index.i1, index.i2, index.idx8, index.w8
        if lists == "flat" and B > 1:
            assert bool((c.i1.long() // Lp != torch.arange(B, device="cuda").repeat_interleave(G2 * 8)).any())   # rows of other samples
            assert bool((c.i1.long() % Lp < lead).any())                                                         # and prompt rows
    c.gamma, c.beta = torch.linspace(0.5, 1.5, D), torch.linspace(-0.2, 0.2, D)
    c.rm, c.rv = torch.linspace(-0.1, 0.4, D), torch.linspace(0.6, 1.7, D)
    c.lng, c.lnb = torch.linspace(0.8, 1.2, D), torch.linspace(-0.1, 0.1, D)
    c.W1, c.b1 = torch.randn(32, D, generator=g) * 0.05, torch.randn(32, generator=g) * 0.1
    c.W2, c.b2 = torch.randn(D, 32, generator=g) * 0.05, torch.randn(D, generator=g) * 0.1
    c.ud = torch.rand(B * c.Lout, 32, generator=g) if pd > 0 else None
    c.g_tail = torch.randn(B, c.Lout, D, generator=g)            # gradient of the adapter output
    c.g_rows = torch.randn(B, Lp, D, generator=g)                # gradient of the propagated rows (kernel-level backward)
    for k, v in list(vars(c).items()):
        if isinstance(v, torch.Tensor):
            setattr(c, k, v.contiguous().cuda())
    assert int(c.i1.min()) >= 0 and int(c.i1.max()) < c.rows and int(c.i2.min()) >= 0 and int(c.i2.max()) < c.rows   # never a row outside x2
    assert int(c.idx8.min()) >= 0 and int(c.idx8.max()) < G2
    c.index = HF.PropIndex(c.i1, c.i2, c.idx8, c.w8, c.rows)
    return c


#        B  cls    P   T   G2  training dp    bias   pd   lists
CASES = [(2, True, 10, 64, 32, True, "u", True, 0.1, "random"),      # the headline layout
         (3, False, 1, 8, 4, False, None, False, 0.0, "random"),     # smallest lists, eval BatchNorm, 24 rows out
         (3, True, 10, 12, 4, True, "u", False, 0.0, "random"),      # Lout = 13: 39 rows out
         (2, False, 10, 8, 4, True, None, True, 0.1, "random"),      # every output row a centre row
         (3, True, 10, 64, 32, True, "u", True, 0.1, "flat"),        # the reference's stride-64-into-74 lists
         (2, False, 1, 64, 32, False, "u", True, 0.0, "gather")]
IDS = ["B%d-cls%d-P%d-T%d-G%d-%s-dp%s-b%d-pd%s-%s" % (c[0], c[1], c[2], c[3], c[4], "train" if c[5] else "eval", c[6], c[7], c[8], c[9]) for c in CASES]


def _old_forward_kernels(c, with_tail):
    """The launches that are replaced, through the library's entry points (upp_prop_fwd itself: its partials are compared too)."""
    lib, p = _abi.load(), _abi.ptr
    x3 = ops.rowln_fwd(c.x2, None, None, 0, 0, c.m, c.u_dp, c.keep_dp, None, None, 1e-5, c.Lp, ybias=c.mb)[0]
    o = types.SimpleNamespace(rm=c.rm.clone(), rv=c.rv.clone(), pooled=torch.empty(c.groups, c.D, device="cuda"),
                              amax=torch.empty(c.groups, c.D, dtype=torch.uint8, device="cuda"),
                              part=torch.empty(lib.upp_prop_part_floats(c.groups, c.D), device="cuda"), mean=torch.empty(c.D, device="cuda"),
                              rstd=torch.empty(c.D, device="cuda"), rows=torch.empty_like(x3))
    assert lib.upp_prop_fwd(p(x3), p(c.i1), p(c.u_g), c.keep_g, p(c.i2), p(c.idx8), p(c.w8), p(c.gamma), p(c.beta), p(o.rm), p(o.rv), MOM, EPS,
                            int(c.training), p(o.pooled), p(o.amax), p(o.part), p(o.mean), p(o.rstd), p(o.rows), c.B, c.Lp, c.T, c.G2, c.D,
                            _abi.stream()) == 0
    if with_tail:
        o.tail = ops.ln_adapter_fwd(o.rows, None, None, None, 1.0, c.mode, c.P, c.lng, c.lnb, 1e-5, c.W1, c.b1, c.W2, c.b2, c.ud, c.pd, 0.7, c.Lout)
    return o


def _check_pool_and_backward(c):
    old = _old_forward_kernels(c, c.D == 384)
    rm, rv = c.rm.clone(), c.rv.clone()
    pooled, amax, part, mean, rstd = ops.prop_res_pool_fwd(c.x2, c.m, c.mb, c.u_dp, c.keep_dp, c.i1, c.u_g, c.keep_g, rm, rv, MOM, EPS,
                                                           c.training, c.G2)
    for name, a, b in (("pooled", pooled, old.pooled), ("amax", amax, old.amax), ("part", part, old.part), ("mean", mean, old.mean),
                       ("rstd", rstd, old.rstd), ("running_mean", rm, old.rm), ("running_var", rv, old.rv)):
        assert torch.equal(a, b), name
    # backward: prop_bwd -> rowln_bwd of the plain residual  |  prop_res_bwd
    ix = c.index
    gX, gg, gb = ops.prop_bwd(c.g_rows, pooled, amax, mean, rstd, c.gamma, c.u_g, c.keep_g, c.w8, ix.csr1, ix.csr2, ix.csr8, c.training,
                              c.B, c.Lp, c.T, c.G2)
    g_x2, _, g_m, _ = ops.rowln_bwd(gX, None, None, None, None, None, 0, c.u_dp, c.keep_dp, c.B, c.Lp, c.Lp, c.D, 0, need_x=True,
                                    need_prompt=False, need_y=True)
    n_x2, n_m, n_gg, n_gb = ops.prop_res_bwd(c.g_rows, pooled, amax, mean, rstd, c.gamma, c.u_g, c.keep_g, c.w8, ix.csr1, ix.csr2, ix.csr8,
                                             c.training, c.u_dp, c.keep_dp, c.B, c.Lp, c.T, c.G2)
    for name, a, b in (("g_x2", n_x2, g_x2), ("g_m", n_m, g_m), ("g_gamma", n_gg, gg), ("g_beta", n_gb, gb)):
        assert torch.equal(a, b), name
    if c.u_dp is not None:
        assert float(n_m[0].abs().max()) == 0.0 and torch.equal(n_x2[0], gX[0])      # the dropped sample: no gradient into its branch
    return old, (pooled, mean, rstd)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernels_equal_the_launches_they_replace(case):
    """upp_prop_res_pool_fwd, upp_ln_adapter_prop_fwd and upp_prop_res_bwd against rowln_fwd + upp_prop_fwd + ln_adapter_fwd and prop_bwd +
    rowln_bwd: every intermediate the backward reads, and the results."""
    c = make_case(*case[:4], case[4], 384, *case[5:9], seed=11 + case[0] * 7 + case[3], lists=case[9])
    old, (pooled, mean, rstd) = _check_pool_and_backward(c)
    new = ops.ln_adapter_prop_fwd(c.x2, c.m, c.mb, c.u_dp, c.keep_dp, c.mode, c.P, pooled, mean, rstd, c.gamma, c.beta, c.i2, c.idx8, c.w8,
                                  c.lng, c.lnb, 1e-5, c.W1, c.b1, c.W2, c.b2, c.ud, c.pd, 0.7, c.Lout)
    for name, a, b in zip(("out", "xo", "mean", "rstd", "s1"), new, old.tail):
        assert a.shape == b.shape and torch.equal(a, b), name
    # the rows the tail normalised ARE the propagated rows without their prompts
    keep_rows = [0] + list(range(1 + c.P, c.Lp)) if c.cls else list(range(c.P, c.Lp))
    assert torch.equal(new[1], old.rows[:, keep_rows])


@pytest.mark.parametrize("B,T,G2,training,dp,bias,lists", [(2, 8, 4, True, "u", True, "random"), (3, 64, 32, False, None, False, "random"),
                                                           (3, 64, 32, True, "u", True, "flat")])
def test_pool_and_gradient_kernels_at_64_columns(B, T, G2, training, dp, bias, lists):
    """The pool and g_X variants take any D <= 512 (one column slot of eight live at D = 64, seven clamped)."""
    _check_pool_and_backward(make_case(B, True, 10, T, G2, 64, training, dp, bias, 0.0, seed=5 + B + T, lists=lists))


def _bn(c):
    bn = torch.nn.BatchNorm1d(c.D, eps=EPS, momentum=MOM).cuda().train(c.training)
    with torch.no_grad():
        bn.weight.copy_(c.gamma); bn.bias.copy_(c.beta); bn.running_mean.copy_(c.rm); bn.running_var.copy_(c.rv)
    return bn


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_node_equals_the_three_nodes_it_replaces(case):
    """HF.prop_tail against HF.rowln -> HF.propagate -> HF.ln_adapter under autograd: output, running statistics and the gradients of x2, m,
    the BatchNorm, the adapter's LayerNorm and the adapter."""
    c = make_case(*case[:4], case[4], 384, *case[5:9], seed=23 + case[0] * 7 + case[3], lists=case[9])

    def run(fused):
        bn = _bn(c)
        ln = torch.nn.LayerNorm(c.D).cuda()
        with torch.no_grad():
            ln.weight.copy_(c.lng); ln.bias.copy_(c.lnb)
        leaves = [t.clone().requires_grad_(True) for t in (c.x2, c.m, c.W1, c.b1, c.W2, c.b2)]
        x2, m, W1, b1, W2, b2 = leaves
        if fused:
            assert HF.prop_tail_usable(x2, bn, c.T, c.P, c.mode)
            out = HF.prop_tail(x2, m, c.mb, c.u_dp, c.keep_dp, c.mode, c.P, bn, c.index, c.u_g, c.keep_g, c.training, ln, W1, b1, W2, b2, c.ud,
                               c.pd, 0.7)
        else:
            x3, _ = HF.rowln(x2, y=m, ybias=c.mb, u=c.u_dp, keep=c.keep_dp)
            x3 = HF.propagate(x3, bn, c.index, c.u_g, c.keep_g, c.training)
            out = HF.ln_adapter(x3, None, None, None, 1.0, c.mode, c.P, ln, W1, b1, W2, b2, c.ud, c.pd, 0.7)
        grads = torch.autograd.grad((out * c.g_tail).sum(), leaves + [bn.weight, bn.bias, ln.weight, ln.bias])
        return [out.detach(), bn.running_mean.clone(), bn.running_var.clone()] + list(grads)

    names = ("out", "running_mean", "running_var", "g_x2", "g_m", "g_W1", "g_b1", "g_W2", "g_b2", "g_bn_weight", "g_bn_bias", "g_ln_weight",
             "g_ln_bias")
    for name, a, b in zip(names, run(True), run(False)):
        assert a.shape == b.shape and torch.equal(a, b), name


# ---------------------------------------------------------------------------------------------- the block
@pytest.fixture(scope="module")
def blocks():
    """Blocks 0 and 1 of the classification model's encoder with the recipe's trainable set: prompts, adapters, the propagation BatchNorm."""
    import _seeded
    from models import build_model_from_cfg
    from utils.config import builtin_cfg
    model = _seeded.fill(build_model_from_cfg(builtin_cfg('unify_modelnet_cls').model)).cuda()
    blks = list(model.blocks.blocks[:2])
    for b in blks:
        for n, p in b.named_parameters():
            p.requires_grad_(any(k in n for k in ("downstream_adapter", "downstream_prompts", "bnorm")))
    pts = _seeded.unit_ball_clouds(2, 1024, seed=2).cuda()
    with torch.no_grad():
        _, center = model.group_divider(pts)
        _, c2, i1, i2 = upp_layers.Group(32, 8)(center, require_index=True, gather_idx=False)
    kw = dict(path='downstream', downstream_adapter=True, downstream_prompts=True, classification=True, center1=center, center1_idx=i1,
              center2=c2, center2_idx=i2, gather_idx=False, prompt_propagation_after=True)
    return blks, kw


def _run_blocks(blks, kw, training, switch):
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randn(2, 65, 384, device='cuda', generator=g).requires_grad_(True)
    pos = torch.randn(2, 65, 384, device='cuda', generator=g)
    state = [{k: v.clone() for k, v in b.bnorm.state_dict().items()} for b in blks]
    was = upp_layers.FUSE_PROP_TAIL
    upp_layers.FUSE_PROP_TAIL = switch
    try:
        upp_layers.UNIFORMS.buf = None                           # no model forward around the blocks: every site draws directly ...
        torch.manual_seed(17)                                    # ... from the default generator, in the same order in both runs
        h = x
        kw = dict(kw, _prop_cache={})
        for b in blks:
            b.train(training)
            assert b.fusable(h)
            h = b.forward_fused(h, pos, **kw)
        params = [p for b in blks for p in b.parameters() if p.requires_grad]
        w = torch.linspace(-1, 1, h.numel(), device='cuda').view_as(h)
        grads = torch.autograd.grad((h * w).sum(), [x] + params)
        stats = [t.clone() for b in blks for t in (b.bnorm.running_mean, b.bnorm.running_var)]
        return h.grad_fn.name(), [h.detach()] + stats + list(grads)
    finally:
        upp_layers.FUSE_PROP_TAIL = was
        for b, s in zip(blks, state):
            b.bnorm.load_state_dict(s)
            b.eval()


@pytest.mark.parametrize("training", [True, False])
def test_two_blocks_with_the_switch_on_and_off(blocks, training):
    """Block.forward_fused over two prompted blocks at B = 2: output, BatchNorm running statistics, the input gradient and every parameter
    gradient are the same bits with FUSE_PROP_TAIL on (one node per block) and off (the three nodes)."""
    blks, kw = blocks
    node_on, on = _run_blocks(blks, kw, training, True)
    node_off, off = _run_blocks(blks, kw, training, False)
    assert node_on == "_PropTailBackward" and node_off == "_LnAdapterBackward"
    assert len(on) == len(off) > 10
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and torch.equal(a, b), i


def test_stage_two_keeps_the_stored_rows(blocks, monkeypatch):
    """Centres with a gradient (stage 2 of the recipe): the interpolation weights carry one, upp_prop_w8_grad reads the stored x3, so the
    block takes rowln -> propagate -> ln_adapter and not prop_tail (and the other way round without that gradient); the gradient
    reaches the centres."""
    blks, kw = blocks
    blk = blks[0]
    calls = []
    for name in ("prop_tail", "propagate", "ln_adapter"):
        real = getattr(HF, name)
        monkeypatch.setattr(HF, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    g = torch.Generator(device='cuda').manual_seed(4)
    x, pos = torch.randn(2, 65, 384, device='cuda', generator=g), torch.randn(2, 65, 384, device='cuda', generator=g)
    c1 = kw['center1'].clone().requires_grad_(True)
    out = blk.forward_fused(x, pos, **dict(kw, _prop_cache={}, center1=c1))
    assert calls == ["propagate", "ln_adapter"]
    g_c1 = torch.autograd.grad(out.sum(), c1)[0]
    assert bool(torch.isfinite(g_c1).all()) and float(g_c1.abs().max()) > 0
    del calls[:]
    blk.forward_fused(x, pos, **dict(kw, _prop_cache={}))
    assert calls == ["prop_tail"]


def test_wrappers_refuse_what_the_kernels_cannot_take():
    c = make_case(2, True, 10, 8, 4, 384, True, "u", True, 0.0, seed=3)
    pooled, amax, part, mean, rstd = ops.prop_res_pool_fwd(c.x2, c.m, c.mb, c.u_dp, c.keep_dp, c.i1, c.u_g, c.keep_g, c.rm.clone(), c.rv.clone(),
                                                           MOM, EPS, True, c.G2)
    with pytest.raises(RuntimeError):
        ops.prop_res_pool_fwd(c.x2, c.m[:, :-1].contiguous(), c.mb, c.u_dp, c.keep_dp, c.i1, c.u_g, c.keep_g, c.rm, c.rv, MOM, EPS, True, c.G2)
    with pytest.raises(RuntimeError):
        ops.prop_res_pool_fwd(c.x2, c.m, c.mb, c.u_dp[:1].contiguous(), c.keep_dp, c.i1, c.u_g, c.keep_g, c.rm, c.rv, MOM, EPS, True, c.G2)
    with pytest.raises(RuntimeError):
        ops.prop_res_pool_fwd(c.x2, c.m, c.mb, c.u_dp, c.keep_dp, c.i1[:-8].contiguous(), c.u_g, c.keep_g, c.rm, c.rv, MOM, EPS, True, c.G2)
    args = [c.x2, c.m, c.mb, c.u_dp, c.keep_dp, c.mode, c.P, pooled, mean, rstd, c.gamma, c.beta, c.i2, c.idx8, c.w8, c.lng, c.lnb, 1e-5, c.W1,
            c.b1, c.W2, c.b2, None, 0.0, 0.7, c.Lout]
    for pos, bad in ((7, pooled[:-1].contiguous()), (14, c.w8[:, :-1].contiguous()), (25, c.Lout + 1), (5, HF.ROW_INSERT)):
        a = list(args)
        a[pos] = bad
        with pytest.raises(RuntimeError):
            ops.ln_adapter_prop_fwd(*a)
    x64 = torch.randn(2, c.Lp, 64, device="cuda")
    assert not HF.prop_tail_usable(x64, torch.nn.BatchNorm1d(64).cuda(), c.T, c.P, c.mode)
    assert not HF.prop_tail_usable(c.x2, torch.nn.BatchNorm1d(384, affine=False).cuda(), c.T, c.P, c.mode)
    assert not HF.prop_tail_usable(c.x2, torch.nn.BatchNorm1d(384).cuda(), c.T, c.P, HF.ROW_IDENTITY)
    assert HF.prop_tail_usable(c.x2, torch.nn.BatchNorm1d(384).cuda(), c.T, c.P, c.mode)
