"""Host-side checks of torus-exact training on the tiled entries (`GaugeDynamics(periodic=True, tiled_train=True)`,
L2HMC_PLAN_PERIODIC_TRAIN), no GPU: the flag's value and rules, what `check_train_plan` lets through on fake non-NULL
addresses (host checks only, as tests/test_periodic_host.py does), the workspace formula of the header, the trainer's
path selection and the Python refusals."""
import ctypes as C
import types

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from l2hmc_amd import _lib, build as lbuild
    lbuild.build()
    return _lib.lib()


FAKE = 16                                              # any non-NULL address: host checks only
W = ("w1_t", "wt", "b1", "wh_t", "bh", "whd_t", "bhd", "coeff_s", "coeff_q")


def _nets(D, hidden=None):
    """(XNet, VNet, a reference-mode net) of a periodic plan at x_dim D."""
    from l2hmc_amd import _lib
    Hn = 4 * D if hidden is None else hidden
    w = {k: FAKE for k in W}
    return (_lib.DenseNet(D=D, H=Hn, Ka=D, Kb=2 * D, **w), _lib.DenseNet(D=D, H=Hn, Ka=2 * D, Kb=D, **w),
            _lib.DenseNet(D=D, H=Hn, Ka=D, Kb=D, **w))


def _plan(flags, T=4, X=4, N=3, hmc=0, nets=None, **kw):
    from l2hmc_amd import _lib
    xnet, vnet, _ = _nets(2 * T * X) if nets is None else nets
    return _lib.GaugePlan(T=T, X=X, num_steps=N, hmc=hmc, flags=flags, masks=FAKE, xnet=xnet, vnet=vnet, **kw)


def _forward(L, plan, rows=4):
    return L.l2hmc_gauge_train_forward(C.byref(plan), 1.0, None, None, None, rows, None, None, None, None, None, 0,
                                       None)


def test_flag_is_declared_with_the_same_value_on_both_sides():
    from l2hmc_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        assert "#define L2HMC_PLAN_PERIODIC_TRAIN 1024" in f.read()
    assert _lib.PLAN_PERIODIC_TRAIN == 1024


@pytest.mark.parametrize("T,X", [(4, 4), (2, 8), (4, 8), (8, 8), (16, 16)])
def test_flagged_periodic_plan_gets_past_the_plan_check(L, T, X):
    from l2hmc_amd import _lib
    both = _lib.PLAN_PERIODIC | _lib.PLAN_PERIODIC_TRAIN
    # past check_train_plan: the entry then fails on its NULL pointers, not with the refusal of the mode
    for flags in (both, both | _lib.PLAN_PERIODIC_STEP):
        assert _forward(L, _plan(flags, T, X)) == 1
        msg = L.l2hmc_last_error()
        assert b"NULL pointer" in msg and b"L2HMC_PLAN_PERIODIC" not in msg, msg
    # ... and the reverse entries likewise (bad arguments, not the mode)
    plan = _plan(both, T, X)
    assert L.l2hmc_gauge_train_backward(C.byref(plan), 1.0, None, 4, None, None, None, None, None, None, None, None,
                                        None, 0, None) == 1
    assert b"bad arguments" in L.l2hmc_last_error()
    # the unflagged plan keeps today's refusal, message included; 8x8 does not take the fused training kernels
    assert _forward(L, _plan(_lib.PLAN_PERIODIC, T, X)) == 1
    msg = L.l2hmc_last_error()
    assert b"L2HMC_PLAN_PERIODIC plans train through the layered-training entries" in msg and b"tiled" in msg


def test_flag_rules(L):
    from l2hmc_amd import _lib
    both = _lib.PLAN_PERIODIC | _lib.PLAN_PERIODIC_TRAIN
    xnet, vnet, old = _nets(32)
    # alone on an hmc = 0 plan: refused by the plan check of the sampling entries and by the training entries
    alone = _plan(_lib.PLAN_PERIODIC_TRAIN, nets=(old, old, old))
    assert L.l2hmc_gauge_plan_fused(C.byref(alone)) == -1
    msg = L.l2hmc_last_error()
    assert b"L2HMC_PLAN_PERIODIC_TRAIN" in msg and b"L2HMC_PLAN_PERIODIC" in msg.replace(b"L2HMC_PLAN_PERIODIC_TRAIN", b"")
    assert _forward(L, alone) == 1
    msg = L.l2hmc_last_error()
    assert b"L2HMC_PLAN_PERIODIC_TRAIN" in msg and b"L2HMC_PLAN_PERIODIC" in msg.replace(b"L2HMC_PLAN_PERIODIC_TRAIN", b"")
    # plain HMC ignores it
    from l2hmc_amd._lib import GaugePlan
    for flags in (_lib.PLAN_PERIODIC_TRAIN, both):
        assert L.l2hmc_gauge_plan_fused(C.byref(GaugePlan(T=8, X=8, num_steps=3, hmc=1, flags=flags, masks=FAKE))) == 1
    # the sampling entries take the flagged plan as they take the unflagged one
    assert L.l2hmc_gauge_plan_fused(C.byref(_plan(both))) == 0
    x8, v8, _ = _nets(128)
    for d in x8, v8:
        d.packed = FAKE
    assert L.l2hmc_gauge_plan_fused(C.byref(_plan(both | _lib.PLAN_PERIODIC_STEP, 8, 8, nets=(x8, v8, None)))) == 1
    # ConvNet3D under it is refused
    conv = _plan(both | _lib.PLAN_CONV3D)
    assert _forward(L, conv) == 1 and b"GenericNet" in L.l2hmc_last_error()
    # widths that are no multiples of 32 are refused with the widths named
    assert _forward(L, _plan(both, 3, 5)) == 1
    msg = L.l2hmc_last_error()
    assert b"D=30" in msg and b"Ka=30" in msg and b"Kb=60" in msg and b"H=120" in msg and b"multiples of 32" in msg
    # ... and so is a hidden width that does not tile, or the reference mode's Ka = Kb = D
    assert _forward(L, _plan(both, nets=_nets(32, hidden=100))) == 1 and b"H=100" in L.l2hmc_last_error()
    assert _forward(L, _plan(both, nets=(old, old, old))) == 1
    assert b"periodic XNet" in L.l2hmc_last_error() and b"Kb = 64" in L.l2hmc_last_error()
    assert _forward(L, _plan(both, nets=(xnet, xnet, old))) == 1 and b"periodic VNet" in L.l2hmc_last_error()
    # an hmc plan has nothing to train, flag or not
    assert _forward(L, _plan(both, hmc=1)) == 1 and b"hmc" in L.l2hmc_last_error()


@pytest.mark.parametrize("T,X,N", [(4, 4, 3), (2, 8, 1), (8, 8, 10), (16, 16, 5)])
def test_workspace_grows_by_the_documented_formula_only(L, T, X, N):
    from l2hmc_amd import _lib
    D = 2 * T * X
    flagged = _plan(_lib.PLAN_PERIODIC | _lib.PLAN_PERIODIC_TRAIN, T, X, N)
    plain = _plan(_lib.PLAN_PERIODIC, T, X, N)
    up = lambda n: (n + 255) // 256 * 256            # noqa: E731
    for rows in (5, 19, 2048):
        extra = L.l2hmc_gauge_train_ws_bytes(C.byref(flagged), rows) - L.l2hmc_gauge_train_ws_bytes(C.byref(plain), rows)
        assert extra == 2 * (2 * N * rows * D * 4) + up(rows * 3 * D * 4) - rows * 2 * D * 4
        # the sampling workspaces do not depend on the flag
        assert L.l2hmc_gauge_ws_bytes(C.byref(flagged), rows) == L.l2hmc_gauge_ws_bytes(C.byref(plain), rows)
        assert L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(flagged), rows) == \
            L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plain), rows)
    # a reference-mode plan: the flag (meaningless there, and refused by the entries) moves no byte
    _, _, old = _nets(D)
    for rows in (5, 2048):
        a = L.l2hmc_gauge_train_ws_bytes(C.byref(_plan(0, T, X, N, nets=(old, old, old))), rows)
        b = L.l2hmc_gauge_train_ws_bytes(C.byref(_plan(_lib.PLAN_PERIODIC_TRAIN, T, X, N, nets=(old, old, old))), rows)
        assert a == b > 0


# ---- Python --------------------------------------------------------------------------------------------------------
def _trainer_ns(D, layered=None, **dyn):
    from l2hmc_amd import _lib
    xnet, vnet, _ = _nets(D)
    nets = [types.SimpleNamespace(pack=lambda st=st: st) for st in (xnet, vnet)]
    return types.SimpleNamespace(dynamics=types.SimpleNamespace(network_arch='generic', **dyn), layered=layered,
                                 _nets=nets)


def test_use_layered_truth_table():
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    use = GaugeTrainer._use_layered
    for D in (32, 64, 128, 512):                                    # 4x4, 4x8, 8x8, 16x16
        assert use(_trainer_ns(D, periodic=True, tiled_train=True)) is False
        assert use(_trainer_ns(D, layered=False, periodic=True, tiled_train=True)) is False
        assert use(_trainer_ns(D, layered=True, periodic=True, tiled_train=True)) is True      # the cross-check
    for D in (72, 30):                                              # 6x6, 3x5: the flag is carried, the walk trains
        assert use(_trainer_ns(D, periodic=True, tiled_train=True)) is True
        assert use(_trainer_ns(D, layered=True, periodic=True, tiled_train=True)) is True
        with pytest.raises(NotImplementedError, match=rf"tiled.*\({D}, {4 * D}, {D}, {2 * D}\)"):
            use(_trainer_ns(D, layered=False, periodic=True, tiled_train=True))
    # without the flag: today's answers
    for kw in (dict(periodic=True), dict(periodic=True, tiled_train=False), dict(periodic=True, whole_step=True)):
        assert use(_trainer_ns(32, **kw)) is True
        with pytest.raises(NotImplementedError, match="tiled"):
            use(_trainer_ns(32, layered=False, **kw))
    # the reference mode does not read the attribute
    ref = _trainer_ns(32, periodic=False)
    ref._nets = [types.SimpleNamespace(pack=lambda: _nets(32)[2])] * 2
    assert use(ref) is False
    ref.layered = True
    assert use(ref) is True


def _dyn(T=3, X=5, **kw):
    from l2hmc_amd import GaugeLattice, GaugeDynamics
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=4, rand=False)
    return GaugeDynamics(lat, lat.get_energy_function(), eps=0.2, num_steps=2, device=torch.device("cpu"), **kw)


def test_tiled_train_needs_periodic_and_is_refused_before_any_library_call(monkeypatch):
    from l2hmc_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the refusal must not reach the library or torch.cuda")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "stream_ptr", boom)
    with pytest.raises(ValueError, match="tiled_train=True.*periodic=True"):
        _dyn(tiled_train=True)
    with pytest.raises(ValueError, match="tiled_train=True.*periodic=True"):
        _dyn(periodic=False, tiled_train=True, whole_step=False)
    assert _dyn().tiled_train is False and _dyn(periodic=True).tiled_train is False        # opt-in
    dyn = _dyn(periodic=True, tiled_train=1)
    assert dyn.tiled_train is True and dyn.periodic is True and dyn.whole_step is False     # coerced with bool
    both = _dyn(periodic=True, tiled_train=True, whole_step=True)
    assert both.tiled_train is True and both.whole_step is True                             # they compose
    assert _dyn(hmc=True, tiled_train=True).tiled_train is True      # no networks: carried, changes nothing


def test_plan_carries_the_flag_only_where_it_means_something(monkeypatch):
    from l2hmc_amd import _lib
    monkeypatch.setattr(_lib, "dev_ptr", lambda t, dtype=torch.float32, name="tensor": 16)   # (host tensors: no address)
    hmc = _dyn(periodic=True, tiled_train=True, hmc=True)
    assert not hmc._plan().flags & (_lib.PLAN_PERIODIC | _lib.PLAN_PERIODIC_TRAIN)
    for tt, ws in ((True, False), (False, False), (True, True), (False, True)):
        dyn = _dyn(periodic=True, tiled_train=tt, whole_step=ws)
        st = _lib.DenseNet(D=30, H=120, Ka=30, Kb=60)
        dyn.position_fn = types.SimpleNamespace(pack=lambda: st)
        dyn.momentum_fn = types.SimpleNamespace(pack=lambda: st)
        monkeypatch.setattr(dyn, "_heads_image", lambda plan: None)
        flags = dyn._plan().flags
        assert flags & _lib.PLAN_PERIODIC
        assert bool(flags & _lib.PLAN_PERIODIC_TRAIN) is tt and bool(flags & _lib.PLAN_PERIODIC_STEP) is ws


def test_check_differentiable_lets_the_flagged_mode_through_where_the_widths_tile():
    from l2hmc_amd import autograd
    autograd.check_differentiable(_dyn(4, 4, periodic=True, tiled_train=True))               # D = 32, H = 128
    autograd.check_differentiable(_dyn(2, 8, periodic=True, tiled_train=True, whole_step=True))
    # widths that do not tile: the existing ValueError, with the widths
    with pytest.raises(ValueError, match="widths .*'D': 30.*multiples of 32"):
        autograd.check_differentiable(_dyn(3, 5, periodic=True, tiled_train=True))
    # without the flag: the existing refusal of the mode, at any widths
    for T, X in ((4, 4), (3, 5)):
        with pytest.raises(NotImplementedError, match="periodic=True.*layered reverse walk"):
            autograd.check_differentiable(_dyn(T, X, periodic=True))
    with pytest.raises(NotImplementedError, match="hmc=True"):
        autograd.check_differentiable(_dyn(4, 4, periodic=True, tiled_train=True, hmc=True))
