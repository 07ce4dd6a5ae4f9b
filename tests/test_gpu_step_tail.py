"""The step-tail kernels of csrc/optim.hip (fused clip + AdamW, batched column sums, batched copies, column-sum partials) at the sizes,
alignments and job mixes at which they take another path: block caps, two-load and remainder loops, scalar tails, unaligned buffers,
the tall / wide / narrow classes of upp_batched_sum and its window destinations, the copy kernel's byte branch and second launch, chunks
without rows.  Every layout check is exact (integer data, torch.equal against a float64 sum); every output sits between guard elements
that must keep their sentinel.  The one toleranced assertion is the AdamW comparison, bounded by torch's own f32 error."""
import ctypes
import math

import numpy as np
import pytest
import torch

from upp_hip import _abi, ops

pytestmark = pytest.mark.gpu

F32 = torch.float32
PAD = 64                     # guard elements on either side of a view (a multiple of 16 bytes for every dtype used here)


def guarded(n, dtype, offset_elems=0):
    """-> (view of n elements inside a larger sentinel-filled buffer, shifted `offset_elems` off the 16-byte aligned start; checker that
    asserts every element outside the view still holds the sentinel: NaN for floats, 0xA5 bytes for everything else)."""
    item = torch.empty(0, dtype=dtype).element_size()
    start = PAD + offset_elems
    if dtype.is_floating_point:
        buf = torch.full((start + n + PAD,), float('nan'), dtype=dtype, device='cuda')
        view = buf[start:start + n]

        def check():
            assert bool(torch.isnan(buf[:start]).all()) and bool(torch.isnan(buf[start + n:]).all()), "guard elements overwritten"
    else:
        buf = torch.full(((start + n + PAD) * item,), 0xA5, dtype=torch.uint8, device='cuda')
        view = buf[start * item:(start + n) * item].view(dtype)

        def check():
            assert bool((buf[:start * item] == 0xA5).all()) and bool((buf[(start + n) * item:] == 0xA5).all()), "guard bytes overwritten"
    assert buf.data_ptr() % 16 == 0
    assert n == 0 or view.data_ptr() == buf.data_ptr() + start * item
    return view, check


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _ints(shape, k, gen):
    return torch.randint(-k, k + 1, tuple(shape), device='cuda', generator=gen).float()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ clip + AdamW
def _f(x):
    return float(np.float32(x))            # every implementation below gets the same (f32-representable) hyper-parameters


LR, B1, B2, EPS, WD = _f(5e-4), _f(0.9), _f(0.999), _f(1e-8), _f(0.05)
# 262144 / 262145: below / above the 1,024-block cap of the norm; 524289: first n above the update's 2,048-block cap;
# 3195111 = 3 * 1048576 + 4 * 12345 + 3: the two-load loop runs twice for the low threads, the single-load remainder runs, and three
# scalar tail elements remain
EXACT_N = [1, 3, 5, 255, 257, 1027, 262144, 262145, 524289, 3195111]


def _adam_buffers(n, g_off=0):
    b = {}
    checks = []
    for name, k, off in (("p", n, 0), ("g", n, g_off), ("m", n, 0), ("v", n, 0), ("state", 8, 0), ("scratch", 1024, 0)):
        b[name], chk = guarded(k, F32, off)
        checks.append(chk)
    b["state"].zero_()                       # (the scratch stays NaN: the prepare kernel may read only the partials this call wrote)
    return b, checks


@pytest.mark.parametrize("g_off", [0, 1])                  # 1: g is 4 bytes off alignment -> the norm's n4 = 0 (all-scalar) path
@pytest.mark.parametrize("max_norm", [1.0, -1.0])          # -1: no clipping
@pytest.mark.parametrize("n", EXACT_N)
def test_adamw_norm_clip_and_gradient_are_exact_on_integer_gradients(n, max_norm, g_off):
    """Gradients in {-2..2}: every partial sum of squares is an integer <= 4 * 3,195,111 < 2^24, exact in f32 in any order."""
    gen = _gen(n)
    b, checks = _adam_buffers(n, g_off)
    g0 = _ints((n,), 2, gen)
    g0[0] = 2.0                                            # never an all-zero gradient
    b["g"].copy_(g0)
    b["p"].copy_(torch.randn(n, device='cuda', generator=gen) * 0.1)
    b["m"].zero_(); b["v"].zero_()
    assert (b["g"].data_ptr() % 16 == 0) == (g_off == 0)
    ops.adamw_flat(b["p"], b["g"], b["m"], b["v"], n, n // 3, b["state"], b["scratch"], LR, B1, B2, EPS, WD, max_norm)
    st = b["state"].cpu().numpy()
    sumsq = int(g0.double().square().sum().item())
    want_norm = np.float32(np.sqrt(np.float64(sumsq)))
    assert abs(np.float64(st[1]) - np.float64(want_norm)) <= np.spacing(want_norm), (st[1], want_norm)
    one = np.float32(1.0)
    want_clip = min(np.float32(max_norm) / (st[1] + np.float32(1e-6)), one) if max_norm > 0 else one      # the kernel's formula, in f32
    assert st[2].dtype == np.float32 and st[2] == want_clip, (st[2], want_clip)
    assert st[0] == 1.0
    g0c = g0.cpu().numpy()
    if max_norm > 0:
        want_g = g0c * st[2]                               # one f32 multiply
        assert want_g.dtype == np.float32 and st[2] < 1.0          # (|g[0]| = 2 > max_norm: always clipped)
    else:
        want_g = g0c
        assert st[2] == 1.0
    assert np.array_equal(b["g"].cpu().numpy(), want_g)
    # first step from zero moments: m = g (1 - beta1), v = (g g)(1 - beta2), one rounding per operation
    assert np.array_equal(b["m"].cpu().numpy(), want_g * (one - np.float32(B1)))
    assert np.array_equal(b["v"].cpu().numpy(), (want_g * want_g) * (one - np.float32(B2)))
    assert bool(torch.isfinite(b["p"]).all())
    for chk in checks:
        chk()


def _ref64_step(p, m, v, g, step, split, max_norm):
    """clip_grad_norm_ + AdamW (decoupled decay, lerp first moment, eps after the bias-corrected sqrt) in float64, in place."""
    norm = g.square().sum().sqrt()
    if max_norm > 0:
        g = g * torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    bc1, sbc2 = 1.0 - B1 ** step, math.sqrt(1.0 - B2 ** step)
    p[split:] *= 1.0 - LR * WD
    m += (g - m) * (1.0 - B1)
    v.mul_(B2).add_(g * g * (1.0 - B2))
    p -= (LR / bc1) * (m / (v.sqrt() / sbc2 + EPS))


def _adam_inputs(n, seed):
    gen = _gen(seed)
    p0 = torch.randn(n, device='cuda', generator=gen) * 0.1
    # norms of 50 sqrt(n) and 1e-3 sqrt(n) (1.8 at n = 3,195,111) against max_norm = 10: clipping active, idle, active
    grads = [torch.randn(n, device='cuda', generator=gen) * s for s in (50.0, 1e-3, 50.0)]
    return p0, grads


def _run_kernel(n, split, p0, grads, max_norm, by_argument=False):
    b, checks = _adam_buffers(n)
    b["p"].copy_(p0); b["m"].zero_(); b["v"].zero_()
    if not by_argument:
        b["state"][5:7] = torch.tensor([LR, WD], device='cuda')
    gs = []
    for g in grads:
        b["g"].copy_(g)
        if by_argument:
            ops.adamw_flat(b["p"], b["g"], b["m"], b["v"], n, split, b["state"], b["scratch"], LR, B1, B2, EPS, WD, max_norm)
        else:                                              # lr < 0: lr / weight decay from state[5:7]; the by-value weight decay is ignored
            ops.adamw_flat(b["p"], b["g"], b["m"], b["v"], n, split, b["state"], b["scratch"], -1.0, B1, B2, EPS, 0.3, max_norm)
        gs.append(b["g"].clone())
    for chk in checks:
        chk()
    return b, gs


@pytest.mark.parametrize("n,splits", [(1027, (0, 1, 515, 1027)), (3195111, (0, 1, 1234567, 3195111))])
def test_adamw_three_steps_against_float64_within_twice_torchs_own_error(n, splits):
    """Three implementations of the same three steps: a float64 restatement, torch.optim.AdamW in f32 on two flat parameters after
    clip_grad_norm_, and the kernel.  e_x = max |x_impl - x_f64|; the kernel may be off by twice torch's own error (the second moment's
    fmaf contracts differently) plus one f32 ulp of the value scale.
    Measured on MI355X (e_hip / e_torch, worst split): see the comment beside the assertion."""
    p0, grads = _adam_inputs(n, n)
    for split in splits:
        assert split in (0, 1, n) or (split % 4 and split % 256)
        p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64, device='cuda'), torch.zeros(n, dtype=torch.float64, device='cuda')
        for it, g in enumerate(grads):
            _ref64_step(p64, m64, v64, g.double(), it + 1, split, 10.0)
        parts = [(p0[:split], 0.0), (p0[split:], WD)]
        groups = [{'params': [torch.nn.Parameter(t.clone())], 'weight_decay': wd} for t, wd in parts if t.numel()]
        params = [g_['params'][0] for g_ in groups]
        opt = torch.optim.AdamW(groups, lr=LR, betas=(B1, B2), eps=EPS)
        for g in grads:
            for q, gq in zip(params, (g[:split], g[split:]) if len(params) == 2 else (g,)):
                q.grad = gq.clone()
            torch.nn.utils.clip_grad_norm_(params, 10.0)
            opt.step()
        torch_p = torch.cat([q.detach() for q in params])
        torch_m = torch.cat([opt.state[q]['exp_avg'] for q in params])
        torch_v = torch.cat([opt.state[q]['exp_avg_sq'] for q in params])
        b, gs = _run_kernel(n, split, p0, grads, 10.0)
        assert b["state"][0].item() == 3.0                                             # the step count, exactly
        assert float(b["state"][2]) < 1.0 and not torch.equal(gs[0], grads[0]) and torch.equal(gs[1], grads[1])     # clipped, idle, clipped
        for name, hip, tor, r64 in (("p", b["p"], torch_p, p64), ("m", b["m"], torch_m, m64), ("v", b["v"], torch_v, v64)):
            e_hip, e_torch = float((hip.double() - r64).abs().max()), float((tor.double() - r64).abs().max())
            scale = float(r64.abs().max())
            print("adamw n=%d split=%d %s: e_hip %.3e e_torch %.3e scale %.3e" % (n, split, name, e_hip, e_torch, scale))
            # measured on MI355X, worst split, e_hip / e_torch / scale:
            #   n = 1027:    p 4.03e-08 / 4.70e-08 / 0.386   m 1.14e-08 / 1.43e-08 / 0.169    v 1.85e-10 / 1.85e-10 / 1.80e-03
            #   n = 3195111: p 8.32e-08 / 8.32e-08 / 0.504   m 3.89e-10 / 4.48e-10 / 3.71e-03 v 1.53e-13 / 2.04e-13 / 1.09e-06
            # (the one case with e_hip above e_torch: n = 3195111, split = n, p: 4.32e-08 against 4.17e-08)
            assert e_hip <= 2.0 * e_torch + 6e-8 * scale, (name, split, e_hip, e_torch, scale)


@pytest.mark.parametrize("n,split", [(1027, 515), (3195111, 1234567)])
def test_adamw_lr_by_argument_equals_lr_from_device_state_bit_for_bit(n, split):
    p0, grads = _adam_inputs(n, n + 1)
    a, ga = _run_kernel(n, split, p0, grads, 10.0, by_argument=False)
    b, gb = _run_kernel(n, split, p0, grads, 10.0, by_argument=True)
    assert float(b["state"][5]) == 0.0 and float(b["state"][6]) == 0.0                 # nothing on the device to read them from
    for name in ("p", "m", "v"):
        assert torch.equal(_bits(a[name]), _bits(b[name])), name
    for x, y in zip(ga, gb):
        assert torch.equal(_bits(x), _bits(y))
    assert torch.equal(_bits(a["state"][:5]), _bits(b["state"][:5])) and a["state"][0].item() == 3.0
    assert not torch.equal(a["p"][split:], p0[split:]) and not torch.equal(a["p"][:split], p0[:split])


# ------------------------------------------------------------------------------------------------ batched column sums
class Group:
    """One destination of upp_batched_sum and the jobs that land on it.  rows: one entry per job; every source is columns
    [off, off + length) of an (rows, off + length + extra) matrix; window = (w, pitch, c0): the destination is columns [c0, c0 + w) of a
    guarded (length / w, pitch) matrix."""

    def __init__(self, gen, rows, length, acc, off=3, extra=7, dst_off=0, window=None, values=None):
        values = values or (lambda shape: _ints(shape, 8, gen))
        self.off, self.length, self.acc, self.window = off, length, acc, window
        self.parts = [values((r, off + length + extra)) for r in rows]
        if window:
            w, pitch, c0 = window
            assert length % w == 0 and c0 + w <= pitch
            flat, self.check = guarded((length // w) * pitch, F32, dst_off)
            self.matrix = flat.view(length // w, pitch)
            self.dst = self.matrix[:, c0:c0 + w]
        else:
            self.dst, self.check = guarded(length, F32, dst_off)
        if acc:
            self.dst.copy_(values(tuple(self.dst.shape)))
        self.dst0 = self.dst.clone()
        self.jobs = [(p, off, p.shape[0], length, p.stride(0), self.dst, acc) for p in self.parts]

    def cols(self, p):
        return p[:, self.off:self.off + self.length]

    def reset(self):
        self.dst.copy_(self.dst0)

    def guards(self):
        self.check()
        if self.window:
            w, pitch, c0 = self.window
            outside = torch.ones(pitch, dtype=torch.bool, device='cuda')
            outside[c0:c0 + w] = False
            assert bool(torch.isnan(self.matrix[:, outside]).all()), "columns outside the window overwritten"

    def verify_exact(self):
        want = torch.zeros(self.length, dtype=torch.float64, device='cuda')
        for p in self.parts:
            want += self.cols(p).double().sum(0)
        if self.acc:
            want += self.dst0.double().reshape(-1)
        assert torch.equal(self.dst.double().reshape(-1), want), (self.length, [p.shape[0] for p in self.parts], self.acc, self.window)
        self.guards()

    def wide_eligible(self):
        ok = self.length >= 4096 and self.length % 4 == 0 and self.dst.data_ptr() % 16 == 0 and max(p.shape[0] for p in self.parts) <= 512
        if self.window:
            ok = ok and self.window[0] % 4 == 0 and self.window[1] % 4 == 0
        return ok and all(p.stride(0) % 4 == 0 and (p.data_ptr() + 4 * self.off) % 16 == 0 for p in self.parts)


def _run(groups):
    ops.batched_sum([j for g in groups for j in g.jobs])


def test_batched_sum_tall_jobs_exact():
    """More than 512 rows: 64 columns per workgroup, the four waves split 16-row chunks.  Rows at and around the chunk (16) and the
    wave-round (64) edges, lengths around the 64-column workgroup, strided sources with a column offset."""
    gen = _gen(11)
    groups = [Group(gen, [rows], length, acc) for rows in (513, 528, 529, 577, 2049) for length in (1, 63, 64, 65, 200) for acc in (False, True)]
    groups += [Group(gen, [577, 40], 65, acc) for acc in (False, True)]         # a tall and a short job on one destination: a tall group
    groups += [Group(gen, [3, 513, 1], 130, True)]
    _run(groups)
    for g in groups:
        g.verify_exact()


def test_batched_sum_wide_jobs_and_their_near_misses_exact():
    """Long 16-byte aligned rows: 1,024 columns per workgroup, 16 bytes per lane.  One float of misalignment anywhere, a row stride or a
    length that is no multiple of 4 must take the narrow kernel and give the same sums."""
    gen = _gen(12)
    wide = [Group(gen, [rows], length, acc, off=4, extra=8) for length in (4096, 4100, 8192 + 4) for rows in (1, 2, 3, 8, 9, 75)
            for acc in (False, True)]
    wide += [Group(gen, [9, 1, 17], 4100, acc, off=4, extra=8) for acc in (False, True)]
    near = []
    for rows in (3, 9):
        for acc in (False, True):
            near += [Group(gen, [rows], 4098, acc, off=4, extra=10),              # length % 4
                     Group(gen, [rows], 4100, acc, off=5, extra=7),               # source one float off
                     Group(gen, [rows], 4100, acc, off=4, extra=9),               # row stride % 4
                     Group(gen, [rows], 4100, acc, off=4, extra=8, dst_off=1),    # destination one float off
                     Group(gen, [rows, rows], 4100, acc, off=4, extra=8)]
            near[-1].parts[1] = _ints((rows, 4100 + 13), 8, gen)                  # the group's SECOND source has a row stride % 4
            near[-1].jobs[1] = (near[-1].parts[1], 4, rows, 4100, 4113, near[-1].dst, acc)
    assert all(g.wide_eligible() for g in wide) and not any(g.wide_eligible() for g in near)
    _run(wide + near)
    for g in wide + near:
        g.verify_exact()


def test_batched_sum_window_destinations_exact():
    """(rows, w) column ranges of a wider matrix: element c lives at (c / w) * pitch + c % w.  w 4 / 128 are wide-eligible with an aligned
    pitch when rows * w >= 4096; w 3 / 130 and the odd pitch never are.  All three kernels compute window addresses."""
    gen = _gen(13)
    groups, eligible = [], 0
    for w, wrows_list in ((4, (5, 1024)), (128, (3, 32)), (3, (5, 1366)), (130, (3, 32))):
        for wrows in wrows_list:
            for pitch, c0 in ((w + 4, 4), (w + 5, 2)):
                for n in (3, 513):
                    for acc in (False, True):
                        groups.append(Group(gen, [n], wrows * w, acc, off=4, extra=8, window=(w, pitch, c0)))
                        eligible += groups[-1].wide_eligible()
                        assert groups[-1].wide_eligible() == (w % 4 == 0 and pitch % 4 == 0 and wrows * w >= 4096 and n <= 512)
    assert eligible == 4
    groups.append(Group(gen, [2, 5], 1024 * 4, True, off=4, extra=8, window=(4, 8, 0)))        # wide, two jobs, window at column 0
    groups.append(Group(gen, [2, 600], 32 * 130, True, window=(130, 135, 5)))                   # tall, two jobs, window flush right
    _run(groups)
    for g in groups:
        g.verify_exact()


def test_batched_sum_one_call_mixing_the_three_classes_exact():
    """About 150 short, 70 tall and 70 wide groups interleaved in one call: each pass skips the other classes' groups and needs more
    than one launch (64 groups / 64 jobs each); the jobs of a shared destination are submitted apart from each other."""
    gen = _gen(14)
    groups = []
    for i in range(70):
        groups.append(Group(gen, [1 + i % 20], 1 + (37 * i) % 300, i % 2 == 1))
        groups.append(Group(gen, [513 + i % 18], 1 + (29 * i) % 130, i % 3 == 1))
        groups.append(Group(gen, [2, 7] if i % 9 == 0 else [5 + i % 16], 17 + i, i % 2 == 0))
        groups.append(Group(gen, [1 + i % 3, 2] if i % 10 == 0 else [1 + i % 3], 4096 + 4 * (i % 2), i % 2 == 0, off=4, extra=8))
        if i % 7 == 0:
            groups.append(Group(gen, [3, 2, 1], 257, True))
    assert sum(g.wide_eligible() for g in groups) == 70
    first = [g.jobs[0] for g in groups]
    rest = [j for g in groups for j in g.jobs[1:]]
    assert len(first) == 290 and len(rest) >= 20
    ops.batched_sum(first + rest)
    for g in groups:
        g.verify_exact()


def test_batched_sum_sixty_four_jobs_on_one_destination_exact():
    gen = _gen(15)
    groups = [Group(gen, [2], 100, False), Group(gen, [1 + i % 3 for i in range(64)], 100, True), Group(gen, [4], 9, True)]
    _run(groups)
    for g in groups:
        g.verify_exact()


def _tall_reference(parts, dst0, acc):
    """The tall kernel's documented order in f32: wave w adds the rows of the 16-row chunks w, w + 4, ... in ascending order into ONE
    accumulator that carries across the jobs of the group; the partials combine as ((p0 + p1) + p2) + p3; then the destination."""
    length = parts[0].shape[1]
    partial = []
    for w in range(4):
        a = np.zeros(length, np.float32)
        for part in parts:
            n = part.shape[0]
            for i0 in range(16 * w, n, 64):
                for i in range(i0, min(i0 + 16, n)):
                    a = a + part[i]
        partial.append(a)
    s = ((partial[0] + partial[1]) + partial[2]) + partial[3]
    assert s.dtype == np.float32
    return dst0 + s if acc else s


def _sequential_reference(parts, dst0, acc):
    """The short and wide kernels: destination first, then the rows in ascending order, job after job."""
    a = dst0.copy() if acc else np.zeros(parts[0].shape[1], np.float32)
    for part in parts:
        for i in range(part.shape[0]):
            a = a + part[i]
    assert a.dtype == np.float32
    return a


def test_batched_sum_orders_on_random_floats_bit_exact():
    gen = _gen(16)
    rnd = lambda shape: torch.randn(tuple(shape), device='cuda', generator=gen)
    tall, seq = [], []
    for acc in (False, True):
        tall += [Group(gen, [513], 65, acc, values=rnd), Group(gen, [2049], 200, acc, values=rnd), Group(gen, [577, 40], 63, acc, values=rnd)]
        seq += [Group(gen, [75], 4100, acc, off=4, extra=8, values=rnd), Group(gen, [9, 3], 8196, acc, off=4, extra=8, values=rnd),
                Group(gen, [75], 4098, acc, off=4, extra=10, values=rnd), Group(gen, [17], 300, acc, values=rnd),
                Group(gen, [4, 64, 1], 129, acc, values=rnd)]
    assert [g.wide_eligible() for g in seq[:5]] == [True, True, False, False, False]
    _run(tall + seq)
    first = [g.dst.clone() for g in tall + seq]
    for g in tall + seq:
        g.reset()
    _run(tall + seq)
    for g, was in zip(tall + seq, first):                    # run to run
        assert torch.equal(_bits(g.dst), _bits(was))
    for g, ref in [(g, _tall_reference) for g in tall] + [(g, _sequential_reference) for g in seq]:
        want = ref([g.cols(p).cpu().numpy() for p in g.parts], g.dst0.cpu().numpy(), g.acc)
        assert np.array_equal(g.dst.cpu().numpy(), want), (ref.__name__, g.length, [p.shape[0] for p in g.parts], g.acc)
        g.guards()


# ------------------------------------------------------------------------------------------------ batched copies
COPY_LENGTHS = (0, 1, 15, 16, 17, 65535, 65536, 65537, 131072 + 15)       # the 16-byte piece and the 65,536-byte chunk edges
# (source, destination) byte offsets: both aligned / one of them / both unaligned, by different amounts and by the same one
COPY_OFFSETS = ((0, 0), (0, 1), (5, 0), (3, 7), (8, 8), (0, 15), (12, 0), (1, 2), (15, 15), (0, 0), (4, 0), (0, 8), (9, 6))


def _copy_pairs(gen):
    pairs = []
    for s_off, d_off in COPY_OFFSETS:
        for n in COPY_LENGTHS:
            src, _ = guarded(n, torch.uint8, s_off)
            src.copy_(torch.randint(0, 256, (n,), device='cuda', generator=gen, dtype=torch.uint8))
            dst, chk = guarded(n, torch.uint8, d_off)
            pairs.append((src, dst, chk))
    for k, (shape, dtype) in enumerate([((3, 5), F32), ((16384,), F32), ((16385,), F32), ((7,), torch.int64), ((8192, 2), torch.int64),
                                        ((1,), F32), ((33, 3), torch.int64), ((4097,), F32), ((2, 2, 2), F32), ((5,), torch.int64),
                                        ((65536 // 4 + 1,), F32), ((11,), F32), ((1,), torch.int64)]):
        n = int(np.prod(shape))
        src, _ = guarded(n, dtype, k % 2)
        if dtype == F32:
            src.copy_(torch.randn(n, device='cuda', generator=gen))
        else:
            src.copy_(torch.randint(-2 ** 40, 2 ** 40, (n,), device='cuda', generator=gen))
        dst, chk = guarded(n, dtype, (k // 2) % 2)
        pairs.append((src.view(shape), dst.view(shape), chk))
    return pairs


def test_copy_batched_130_jobs_every_alignment_mix_and_chunk_edge():
    """117 non-empty jobs, so two launches (64 + 53): the 16-byte branch, the byte branch (either pointer unaligned), lengths at the piece and chunk
    edges, empty tensors among the others (the wrapper leaves them out: their data pointer is NULL), f32 and int64 tensors."""
    pairs = _copy_pairs(_gen(17))
    assert len(pairs) == 130
    ops.copy_batched([d for _, d, _ in pairs], [s for s, _, _ in pairs])
    for src, dst, chk in pairs:
        assert torch.equal(dst, src), (tuple(src.shape), src.dtype)
        chk()
    ops.copy_batched([pairs[0][1]], [pairs[0][0]])            # nothing but an empty pair: no launch, no error


def test_copy_batched_zero_length_jobs_through_the_c_abi():
    """The library itself takes a zero-byte job (non-NULL pointers) in either launch of a call and touches nothing for it."""
    gen = _gen(18)
    jobs = []
    for j in range(70):
        n = (0, 17, 65537, 0, 5)[j % 5]
        src, _ = guarded(max(n, 1), torch.uint8, j % 3)
        src.copy_(torch.randint(0, 256, (max(n, 1),), device='cuda', generator=gen, dtype=torch.uint8))
        dst, chk = guarded(max(n, 1), torch.uint8, j % 4)
        jobs.append((src, dst, n, chk))
    k = len(jobs)
    S = (ctypes.c_void_p * k)(*[s.data_ptr() for s, _, _, _ in jobs])
    D = (ctypes.c_void_p * k)(*[d.data_ptr() for _, d, _, _ in jobs])
    B = (ctypes.c_longlong * k)(*[n for _, _, n, _ in jobs])
    ops._call(jobs[0][0].device, "upp_copy_batched", S, D, B, k)
    for src, dst, n, chk in jobs:
        assert torch.equal(dst[:n], src[:n]) and bool((dst[n:] == 0xA5).all())
        chk()


# ------------------------------------------------------------------------------------------------ column-sum partials
def _chunk_rows(n, chunks):
    per = (n + chunks - 1) // chunks
    return [(min(n, c * per), min(n, (c + 1) * per)) for c in range(chunks)]


@pytest.mark.parametrize("n,chunks", [(5, 8), (100, 64), (1000, 7)])
def test_colsum_partials_exact_and_chunks_without_rows_are_zero(n, chunks):
    gen = _gen(19)
    off, length = 3, 70                                     # two 64-column workgroups, the second partly filled
    part = _ints((n, off + length + 6), 8, gen)
    dst, chk = guarded(chunks * length, F32)                # NaN everywhere: an empty chunk must WRITE its zeros
    ops._call(part.device, "upp_colsum_partials", _abi.ptr(part[:, off:]), part.stride(0), n, length, chunks, _abi.ptr(dst))
    got = dst.view(chunks, length)
    rows = _chunk_rows(n, chunks)
    assert (n, chunks) == (1000, 7) or any(r0 >= r1 for r0, r1 in rows)
    for c, (r0, r1) in enumerate(rows):
        want = part[r0:r1, off:off + length].double().sum(0)
        assert torch.equal(got[c].double(), want), c
        if r0 >= r1:
            assert bool((got[c] == 0.0).all()), c
    assert torch.equal(got.double().sum(0), part[:, off:off + length].double().sum(0))
    chk()
    assert torch.equal(ops.colsum_partials(part, off, length, chunks), got)


@pytest.mark.parametrize("W", [1, 3, 4])
@pytest.mark.parametrize("n,chunks", [(5, 8), (100, 64), (1000, 7)])
def test_wcolsum_partials_exact_and_chunks_without_rows_are_zero(n, chunks, W):
    gen = _gen(20 + W)
    length = 260                                            # two 256-column workgroups, the second with one 16-byte piece
    src = _ints((n, length + 8), 8, gen)[:, :length]       # row stride 268
    wts = _ints((n, W + 2), 4, gen)[:, 1:1 + W]
    dst, chk = guarded(chunks * W * length, F32)
    ops._call(src.device, "upp_wcolsum_partials", _abi.ptr(src), src.stride(0), _abi.ptr(wts), wts.stride(0), W, n, length, chunks, _abi.ptr(dst))
    got = dst.view(chunks, W, length)
    for c, (r0, r1) in enumerate(_chunk_rows(n, chunks)):
        want = wts[r0:r1].double().t() @ src[r0:r1].double()
        assert torch.equal(got[c].double(), want), c
        if r0 >= r1:
            assert bool((got[c] == 0.0).all()), c
    assert torch.equal(got.double().sum(0), wts.double().t() @ src.double())
    chk()
    assert torch.equal(ops.wcolsum_partials(src, wts, chunks), got)
