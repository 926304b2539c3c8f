"""Host-side checks of the layered-training entries (include/l2hmc_hip.h, layered Dynamics training): bad arguments
are refused before any launch, rows = 0 is accepted, workspace queries are consistent.  No GPU needed."""
import ctypes as C

import pytest

from l2hmc_amd import _lib, build as lbuild

ADDR = 256          # any non-NULL address: these calls never reach a launch


@pytest.fixture(scope="module")
def L():
    lbuild.build()
    return _lib.lib()


def _net(D=50, H=100, Ka=None, Kb=None):
    n = _lib.DenseNet(D=D, H=H, Ka=D if Ka is None else Ka, Kb=D if Kb is None else Kb, q_tanh=1)
    for f in ("w1_t", "wt", "b1", "wh_t", "bh", "whd_t", "bhd", "coeff_s", "coeff_q"):
        setattr(n, f, ADDR)
    return n


def _grads():
    return _lib.DenseGrads(**{f[0]: ADDR for f in _lib.DenseGrads._fields_})


def _err(L):
    return L.l2hmc_last_error().decode()


def test_new_entries_are_declared_and_bound(L):
    for name in ("l2hmc_stq_dense_taped", "l2hmc_lf_update_v_vjp", "l2hmc_lf_update_x_vjp",
                 "l2hmc_dense_backward_data_ws_bytes", "l2hmc_dense_backward_data",
                 "l2hmc_dense_weight_grads_ws_bytes", "l2hmc_dense_weight_grads", "l2hmc_mog_energy_hvp"):
        assert name in _lib.declared_symbols() and name in _lib._PROTOS and hasattr(L, name)


def test_taped_forward_checks_arguments(L):
    P = [ADDR] * 7
    for bad in (_net(D=0), _net(H=0), _net(Ka=-1), _net(Kb=0)):
        assert L.l2hmc_stq_dense_taped(C.byref(bad), ADDR, ADDR, None, 1., 0., 4, *P[:5], None) == 1
        assert "must be positive" in _err(L)
    assert L.l2hmc_stq_dense_taped(None, ADDR, ADDR, None, 1., 0., 4, *P[:5], None) == 1
    assert L.l2hmc_stq_dense_taped(C.byref(_net()), ADDR, ADDR, None, 1., 0., -1, *P[:5], None) == 1
    assert "rows" in _err(L)
    assert L.l2hmc_stq_dense_taped(C.byref(_net()), ADDR, ADDR, None, 1., 0., 4, ADDR, ADDR, ADDR, ADDR, None,
                                   None) == 1
    assert "NULL" in _err(L)
    assert L.l2hmc_stq_dense_taped(C.byref(_net()), None, None, None, 1., 0., 0, None, None, None, None, None,
                                   None) == 0


@pytest.mark.parametrize("fn,nhead", [("l2hmc_lf_update_v_vjp", 5), ("l2hmc_lf_update_x_vjp", 6)])
def test_update_vjps_check_arguments(L, fn, nhead):
    f = getattr(L, fn)
    head = [ADDR] * nhead
    outs = [ADDR] * 6
    assert f(*head, 0.1, 0, -1, 50, ADDR, ADDR, *outs, None) == 1 and "bad arguments" in _err(L)
    assert f(*head, 0.1, 0, 4, 0, ADDR, ADDR, *outs, None) == 1
    assert f(*head, 0.1, 2, 4, 50, ADDR, ADDR, *outs, None) == 1
    assert f(*head, 0.1, 1, 4, 50, ADDR, ADDR, *outs[:5], None, None) == 1 and "NULL" in _err(L)
    assert f(*head[:-1], None, 0.1, 0, 4, 50, ADDR, None, *outs, None) == 1 and "NULL" in _err(L)
    assert f(*[None] * nhead, 0.1, 0, 0, 50, None, None, *[None] * 6, None) == 0


def test_backward_data_checks_arguments_and_workspace(L):
    n = _net(D=50, H=100)
    need = L.l2hmc_dense_backward_data_ws_bytes(C.byref(n))
    assert need >= 4 * (3 * 50 * 100 + 100 * 100 + 100 * 100)
    assert L.l2hmc_dense_backward_data_ws_bytes(C.byref(_net(H=0))) == 0
    assert L.l2hmc_dense_backward_data_ws_bytes(None) == 0
    P = [ADDR] * 7
    outs = [ADDR] * 5
    assert L.l2hmc_dense_backward_data(C.byref(_net(D=0)), *P, 4, *outs, ADDR, need, None) == 1
    assert "must be positive" in _err(L)
    assert L.l2hmc_dense_backward_data(C.byref(n), *P, -3, *outs, ADDR, need, None) == 1 and "rows" in _err(L)
    assert L.l2hmc_dense_backward_data(C.byref(n), *P, 4, ADDR, ADDR, None, ADDR, ADDR, ADDR, need, None) == 1
    assert "NULL" in _err(L)
    assert L.l2hmc_dense_backward_data(C.byref(n), *P, 4, *outs, ADDR, need - 1, None) == 3
    assert "workspace" in _err(L)
    assert L.l2hmc_dense_backward_data(C.byref(n), *[None] * 7, 0, *[None] * 5, None, 0, None) == 0


def test_weight_grads_check_arguments_and_workspace(L):
    n = _net(D=50, H=100)
    R = 163840
    need = L.l2hmc_dense_weight_grads_ws_bytes(C.byref(n), R)
    assert need >= 4 * 100 * 100 * 2                 # split-k partials of at least two splits
    assert L.l2hmc_dense_weight_grads_ws_bytes(C.byref(n), 37) < need
    assert L.l2hmc_dense_weight_grads_ws_bytes(C.byref(n), -1) == 0
    assert L.l2hmc_dense_weight_grads_ws_bytes(C.byref(_net(D=-2)), 16) == 0
    P = [ADDR] * 8
    g = _grads()
    assert L.l2hmc_dense_weight_grads(C.byref(_net(Kb=0)), R, *P, C.byref(g), ADDR, need, None) == 1
    assert L.l2hmc_dense_weight_grads(C.byref(n), -1, *P, C.byref(g), ADDR, need, None) == 1
    assert L.l2hmc_dense_weight_grads(C.byref(n), R, *P, None, ADDR, need, None) == 1 and "NULL" in _err(L)
    g.bhd = None
    assert L.l2hmc_dense_weight_grads(C.byref(n), R, *P, C.byref(g), ADDR, need, None) == 1 and "NULL" in _err(L)
    g = _grads()
    assert L.l2hmc_dense_weight_grads(C.byref(n), R, *P[:7], None, C.byref(g), ADDR, need, None) == 1
    assert L.l2hmc_dense_weight_grads(C.byref(n), R, *P, C.byref(g), ADDR, need - 256, None) == 3
    assert "workspace" in _err(L)


def test_energy_hvp_checks_arguments(L):
    t = _lib.MogTarget(dim=2, K=2, is_gaussian=0, temperature=1.0, mu=ADDR, prec=ADDR, log_const=ADDR)
    assert L.l2hmc_mog_energy_hvp(None, ADDR, ADDR, 4, ADDR, None) == 1
    assert L.l2hmc_mog_energy_hvp(C.byref(t), ADDR, ADDR, -1, ADDR, None) == 1 and "rows" in _err(L)
    assert L.l2hmc_mog_energy_hvp(C.byref(t), ADDR, None, 4, ADDR, None) == 1 and "NULL" in _err(L)
    assert L.l2hmc_mog_energy_hvp(C.byref(t), None, None, 0, None, None) == 0
    for bad in (dict(dim=9), dict(dim=0), dict(K=9), dict(temperature=0.0)):
        b = _lib.MogTarget(**{**dict(dim=2, K=2, is_gaussian=0, temperature=1.0, mu=ADDR, prec=ADDR,
                                     log_const=ADDR), **bad})
        assert L.l2hmc_mog_energy_hvp(C.byref(b), ADDR, ADDR, 4, ADDR, None) == 1
