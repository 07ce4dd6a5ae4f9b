"""The edge-convolution entry points and the DGCNN grouper on a GPU-less host: argument checks of the library (before any launch), the
reference's state dict, and the module's torch formulation against the fixture of the reference's own class
(tests/golden/dgcnn_grouper.npz, written by tools/gen_golden_dgcnn.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _seeded
from conftest import GOLDEN
from upp_hip import _abi, torch_cpu
from upp_hip import functional as HF

P = ctypes.c_void_p(64)          # a non-null pointer: every call below must be refused before anything reads it


def _fwd(lib, A=P, Bq=P, idx=P, gamma=P, beta=P, eps=1e-5, slope=0.2, G=4, out=P, arg=P, mean=P, rstd=P, work=P, B=1, Nk=8, Nq=8, K=16, O=32):
    return lib.upp_edge_conv_fwd(A, Bq, idx, gamma, beta, eps, slope, G, out, arg, mean, rstd, work, B, Nk, Nq, K, O, None)


def _bwd(lib, g_out=P, A=P, Bq=P, idx=P, arg=P, gamma=P, beta=P, mean=P, rstd=P, slope=0.2, G=4, g_A=P, g_Bq=P, g_gamma=P, g_beta=P, work=P,
         g_y=None, B=1, Nk=8, Nq=8, K=16, O=32):
    return lib.upp_edge_conv_bwd(g_out, A, Bq, idx, arg, gamma, beta, mean, rstd, slope, G, g_A, g_Bq, g_gamma, g_beta, work, g_y,
                                 B, Nk, Nq, K, O, None)


def test_the_library_refuses_bad_arguments_before_any_launch():
    lib = _abi.load()
    BADARG, RANGE = -1, -2
    for call in (_fwd, _bwd):
        for name in ("A", "Bq", "idx", "arg", "gamma", "beta", "mean", "rstd", "work"):
            assert call(lib, **{name: None}) == BADARG, (call.__name__, name)
        assert call(lib, K=0) == BADARG and call(lib, K=65) == RANGE
        assert call(lib, O=513) == RANGE and call(lib, O=0) == BADARG
        assert call(lib, G=5) == RANGE and call(lib, G=3) == RANGE and call(lib, G=-1) == BADARG
        for slope in (-0.01, 1.01, float("nan"), float("inf")):
            assert call(lib, slope=slope) == BADARG, slope
        assert call(lib, Nq=0) == BADARG and call(lib, Nk=0) == BADARG and call(lib, B=-1) == BADARG
        assert call(lib, B=65536) == RANGE and call(lib, Nq=2 ** 27, K=64) == RANGE and call(lib, Nk=2 ** 26, O=32) == RANGE
        assert call(lib, B=0) == 0                                   # an empty batch: nothing to do, nothing launched
    assert _fwd(lib, out=None) == BADARG and _fwd(lib, eps=-1.0) == BADARG
    for name in ("g_out", "g_A", "g_Bq", "g_gamma", "g_beta"):
        assert _bwd(lib, **{name: None}) == BADARG, name
    # without a norm the norm's operands may be absent -- the size checks still come first
    none = dict(gamma=None, beta=None, mean=None, rstd=None, work=None, G=0)
    assert _fwd(lib, K=65, **none) == RANGE and _bwd(lib, O=513, g_gamma=None, g_beta=None, **none) == RANGE
    assert _fwd(lib, B=0, **none) == 0
    slabs = (100 + 7) // 8
    assert lib.upp_edge_conv_work_floats(3, 100, 32) == 3 * slabs * 2 * 32 + 2 * 3 * 32
    assert lib.upp_edge_conv_work_floats(3, 0, 32) == 0 and lib.upp_edge_conv_work_floats(-1, 8, 32) == 0


def test_cpu_tensors_are_served_only_by_the_opt_in_torch_formulation():
    A, Bq, idx = torch.randn(1, 6, 8), torch.randn(1, 5, 8), torch.randint(0, 6, (1, 5, 4))
    was = torch_cpu.enabled()
    try:
        torch_cpu.enable(False)
        with pytest.raises(RuntimeError, match="no CPU path"):
            HF.edge_conv_max(A, Bq, idx)
        torch_cpu.enable(True)
        out = HF.edge_conv_max(A, Bq, idx, norm=(2, torch.ones(8), torch.zeros(8), 1e-5), slope=0.1)
        assert out.shape == (1, 5, 8)
        with pytest.raises(ValueError):
            HF.edge_conv_max(A, Bq, idx, slope=1.5)
    finally:
        torch_cpu.enable(was)


KEYS = [("input_trans.weight", (8, 3, 1)), ("input_trans.bias", (8,))]
for _i, (_c, _o) in enumerate(((8, 32), (32, 64), (64, 64), (64, 128)), 1):
    KEYS += [("layer%d.0.weight" % _i, (_o, 2 * _c, 1, 1)), ("layer%d.1.weight" % _i, (_o,)), ("layer%d.1.bias" % _i, (_o,))]


def test_state_dict_is_the_references():
    from models.dgcnn_group import DGCNN_Grouper
    sd = DGCNN_Grouper().state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == KEYS and len(KEYS) == 14
    assert DGCNN_Grouper(k=16).k == 16 and DGCNN_Grouper().num_features == 128


@pytest.fixture(scope="module")
def cpu_run():
    from models.dgcnn_group import DGCNN_Grouper
    was = torch_cpu.enabled()
    torch_cpu.enable(True)
    try:
        model = _seeded.fill(DGCNN_Grouper()).eval()
        x = _seeded.unit_ball_clouds(2, 640, seed=0)
        with torch.no_grad():
            coor, f = model(x.transpose(1, 2).contiguous())
            l1 = model.edge_layer(model.layer1, x, torch.nn.functional.linear(x, model.input_trans.weight[:, :, 0], model.input_trans.bias),
                                  x, torch.nn.functional.linear(x, model.input_trans.weight[:, :, 0], model.input_trans.bias))
            coor2, f2 = model(x, [512, 128])
    finally:
        torch_cpu.enable(was)
    return coor, f, l1, coor2, f2


def test_module_on_cpu_equals_the_reference_fixture(cpu_run):
    """The project's parity bar: 1e-5 of the output's scale (measured for this formulation: 8e-7 on f, the decomposed conv
    W1 f_j + (W2 - W1) f_i against the reference's W [f_j - f_i ; f_i])."""
    g = np.load(os.path.join(GOLDEN, "dgcnn_grouper.npz"))
    coor, f, l1, _, _ = cpu_run
    assert coor.shape == (2, 3, 128) and f.shape == (2, 128, 128)
    assert np.array_equal(coor.numpy(), g["coor"])                  # FPS picks are points of the input: exact
    for name, got in (("l1", l1.transpose(1, 2).numpy()), ("f", f.numpy())):
        err = np.abs(got - g[name]).max() / np.abs(g[name]).max()
        print("%s: max error / scale = %.3g" % (name, err))
        assert err < 1e-5, (name, err)


def test_both_call_forms_agree(cpu_run):
    coor, f, _, coor2, f2 = cpu_run
    assert coor2.shape == (2, 128, 3) and f2.shape == (2, 128, 128)
    assert torch.equal(coor2.transpose(1, 2), coor) and torch.equal(f2.transpose(1, 2), f)
