"""The step-tail entry points of csrc/optim.hip, host side (no GPU): every argument check that returns before the first launch or
runtime call.  The pointers are fake non-NULL values that are never dereferenced (device pointers) or small host arrays (the job
tables).  No call here has a zero job count: that path ends in a runtime status query."""
import ctypes

import pytest

from upp_hip import _abi

BADARG, RANGE = -1, -2
P = ctypes.c_void_p(64)            # non-NULL, 16-byte aligned, never dereferenced
P4 = ctypes.c_void_p(68)           # ... and one float off alignment


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def test_adamw_flat_refuses_bad_arguments(lib):
    hyper = (5e-4, 0.9, 0.999, 1e-8, 0.05, 10.0)
    for k in range(4):                                     # p, g, m, v
        assert lib.upp_adamw_flat(*[None if i == k else P for i in range(4)], 8, 4, P, P, *hyper, None) == BADARG, k
    assert lib.upp_adamw_flat(P, P, P, P, 8, 4, None, P, *hyper, None) == BADARG          # state
    assert lib.upp_adamw_flat(P, P, P, P, 8, 4, P, None, *hyper, None) == BADARG          # scratch
    for n, split in ((0, 0), (-1, 0), (-2 ** 40, 0), (8, -1), (8, 9), (1, 2), (2 ** 33, 2 ** 33 + 1)):
        assert lib.upp_adamw_flat(P, P, P, P, n, split, P, P, *hyper, None) == BADARG, (n, split)
    assert lib.upp_adamw_scratch_floats() == 1024


def _sum(lib, src, dst, n, ln, ld, acc, dw=None, dp=None, jobs=None):
    k = len(n) if jobs is None else jobs
    return lib.upp_batched_sum(_ptrs(src), _ptrs(dst), _ints(n), _ints(ln), _ints(ld), _ints(acc),
                               None if dw is None else _ints(dw), None if dp is None else _ints(dp), k, None)


def test_batched_sum_refuses_bad_arguments(lib):
    one = dict(src=[64], dst=[128], n=[3], ln=[8], ld=[8], acc=[0])
    arrays = (_ptrs([64]), _ptrs([128]), _ints([3]), _ints([8]), _ints([8]), _ints([0]))
    for k in range(6):                                     # each NULL array with jobs > 0
        assert lib.upp_batched_sum(*[None if i == k else a for i, a in enumerate(arrays)], None, None, 1, None) == BADARG, k
    assert lib.upp_batched_sum(*arrays, None, None, -1, None) == BADARG
    for key, bad in (("src", [None]), ("dst", [None]), ("n", [0]), ("n", [-4]), ("ln", [0]), ("ln", [-1]), ("ld", [7])):
        assert _sum(lib, **dict(one, **{key: bad})) == BADARG, (key, bad)
    # windows: both tables or neither; the width divides the length; rows do not overlap
    assert _sum(lib, dw=[4], **one) == BADARG and _sum(lib, dp=[8], **one) == BADARG
    for dw, dp in ((3, 8), (5, 8), (16, 16), (-4, 8), (4, 3), (8, 7), (4, 0), (4, -8)):
        assert _sum(lib, dw=[dw], dp=[dp], **one) == BADARG, (dw, dp)
    # two jobs, one destination: one length, one accumulate flag, one window
    two = dict(src=[64, 256], dst=[128, 128], n=[3, 5], ln=[8, 8], ld=[8, 12], acc=[1, 1])
    assert _sum(lib, **dict(two, ln=[8, 4], ld=[8, 8])) == BADARG
    assert _sum(lib, **dict(two, acc=[1, 0])) == BADARG
    assert _sum(lib, dw=[4, 2], dp=[8, 8], **two) == BADARG and _sum(lib, dw=[4, 4], dp=[8, 12], **two) == BADARG
    # the limits: 4,096 jobs in a call, 64 jobs on one destination
    k = 4097
    assert _sum(lib, [64] * k, [128 + 4 * j for j in range(k)], [1] * k, [1] * k, [1] * k, [0] * k) == RANGE
    k = 65
    assert _sum(lib, [64 + 4 * j for j in range(k)], [128] * k, [1] * k, [1] * k, [1] * k, [1] * k) == RANGE
    assert _sum(lib, [64 + 4 * j for j in range(k)], [128] * k, [600] * k, [1] * k, [1] * k, [1] * k) == RANGE         # tall
    assert _sum(lib, [64 + 16 * j for j in range(k)], [128] * k, [2] * k, [4096] * k, [4096] * k, [1] * k) == RANGE    # wide


def test_copy_batched_refuses_bad_arguments(lib):
    src, dst = _ptrs([64, 128]), _ptrs([256, 512])
    nbytes = (ctypes.c_longlong * 2)(16, 5)
    assert lib.upp_copy_batched(None, dst, nbytes, 2, None) == BADARG
    assert lib.upp_copy_batched(src, None, nbytes, 2, None) == BADARG
    assert lib.upp_copy_batched(src, dst, None, 2, None) == BADARG
    assert lib.upp_copy_batched(src, dst, nbytes, -1, None) == BADARG
    assert lib.upp_copy_batched(src, dst, (ctypes.c_longlong * 2)(16, -1), 2, None) == BADARG
    assert lib.upp_copy_batched(src, dst, (ctypes.c_longlong * 2)(-2 ** 40, 0), 2, None) == BADARG
    assert lib.upp_copy_batched(_ptrs([64, None]), dst, nbytes, 2, None) == BADARG
    assert lib.upp_copy_batched(src, _ptrs([None, 512]), nbytes, 2, None) == BADARG
    assert lib.upp_copy_batched(src, dst, (ctypes.c_longlong * 2)(5, 65536 * 65535 + 1), 2, None) == RANGE    # more chunks than a grid holds


def test_colsum_partials_refuse_bad_arguments(lib):
    # (src, ld, n, len, chunks, dst, stream)
    assert lib.upp_colsum_partials(None, 8, 4, 8, 2, P, None) == BADARG
    assert lib.upp_colsum_partials(P, 8, 4, 8, 2, None, None) == BADARG
    for ld, n, ln, chunks in ((8, 0, 8, 2), (8, -1, 8, 2), (8, 4, 0, 2), (8, 4, 8, 0), (8, 4, 8, -1), (7, 4, 8, 2)):
        assert lib.upp_colsum_partials(P, ld, n, ln, chunks, P, None) == BADARG, (ld, n, ln, chunks)
    assert lib.upp_colsum_partials(P, 8, 4, 8, 65536, P, None) == RANGE
    # (src, ld, wts, ldw, W, n, len, chunks, dst, stream)
    ok = dict(src=P, ld=8, wts=P, ldw=3, W=3, n=4, ln=8, chunks=2, dst=P)

    def w(**kw):
        a = dict(ok, **kw)
        return lib.upp_wcolsum_partials(a["src"], a["ld"], a["wts"], a["ldw"], a["W"], a["n"], a["ln"], a["chunks"], a["dst"], None)

    for bad in (dict(src=None), dict(wts=None), dict(dst=None), dict(n=0), dict(ln=0), dict(chunks=0), dict(ld=4), dict(W=0), dict(ldw=2)):
        assert w(**bad) == BADARG, bad
    for bad in (dict(chunks=65536), dict(W=5, ldw=5), dict(ln=6), dict(ln=8, ld=9), dict(src=P4), dict(dst=P4)):
        assert w(**bad) == RANGE, bad
