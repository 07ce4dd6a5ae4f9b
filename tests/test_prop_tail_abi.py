"""upp_prop_res_pool_fwd / upp_prop_res_bwd / upp_ln_adapter_prop_fwd check their arguments on the host, before any launch: the error
codes come back on a machine without a GPU."""
import ctypes

from upp_hip import _abi

P = ctypes.c_void_p(4096)        # a non-null pointer that is never dereferenced: every call below is refused before its launch


def test_null_pointers_and_bad_sizes_are_refused_before_any_launch():
    lib = _abi.load()
    ok_pool = [P, P, None, None, 1.0, P, None, 1.0, P, P, 0.1, 1e-5, 1, P, P, P, P, P, 2, 19, 4, 384, None]
    for pos in (0, 1, 5, 13, 14, 15, 16, 17):
        a = list(ok_pool); a[pos] = None
        assert lib.upp_prop_res_pool_fwd(*a) == -1, pos
    for pos, bad in ((18, 0), (19, 0), (20, 0), (21, 0), (4, 0.0), (7, 0.0)):
        a = list(ok_pool); a[pos] = bad
        assert lib.upp_prop_res_pool_fwd(*a) == -1, pos
    a = list(ok_pool); a[12] = 0; a[8] = None                    # eval mode needs the running statistics
    assert lib.upp_prop_res_pool_fwd(*a) == -1
    a = list(ok_pool); a[21] = 513
    assert lib.upp_prop_res_pool_fwd(*a) == -2

    ok_bwd = [P] * 7 + [1.0] + [P] * 7 + [1, None, 1.0] + [P] * 6 + [2, 19, 8, 4, 384, None]
    for pos in list(range(7)) + list(range(8, 15)) + list(range(18, 24)):
        if pos == 6:
            continue                                             # u: optional
        a = list(ok_bwd); a[pos] = None
        assert lib.upp_prop_res_bwd(*a) == -1, pos
    for pos, bad in ((24, 0), (25, 7), (26, 0), (27, 0), (28, 0), (17, 0.0)):
        a = list(ok_bwd); a[pos] = bad
        assert lib.upp_prop_res_bwd(*a) == -1, pos
    a = list(ok_bwd); a[28] = 513
    assert lib.upp_prop_res_bwd(*a) == -2

    ok_tail = [P, P, None, None, 1.0, 3, 10] + [P] * 8 + [8, 4, P, P, 1e-5, P, P, P, P, None, 0.0, 0.7] + [P] * 5 + [2, 19, 9, 384, 32, None]
    for pos in [0, 1] + list(range(7, 15)) + [17, 18, 20, 21, 22, 23] + list(range(27, 32)):
        a = list(ok_tail); a[pos] = None
        assert lib.upp_ln_adapter_prop_fwd(*a) == -1, pos
    for pos, bad in ((15, 0), (15, 20), (16, 0), (5, 1), (5, 2), (6, -1), (34, 10), (4, 0.0)):      # T, G2, mode, P, Lout, keep
        a = list(ok_tail); a[pos] = bad
        assert lib.upp_ln_adapter_prop_fwd(*a) == -1, (pos, bad)
    for pos, bad in ((35, 64), (36, 16)):                        # D, H: the one shape the tail kernel is built for
        a = list(ok_tail); a[pos] = bad
        assert lib.upp_ln_adapter_prop_fwd(*a) == -2, (pos, bad)
