"""Host-side checks of the one-launch training forward of the torus-exact mode (`GaugeDynamics(periodic=True,
tiled_train=True, fused_forward=True)`, L2HMC_PLAN_PERIODIC_TAPE), no GPU: the flag's value and rules, what
`l2hmc_gauge_plan_train_fused` answers on fake non-NULL addresses (host logic only, as tests/run_cases.py::PTR), that
no workspace size depends on the flag, and the constructor's refusals."""
import ctypes as C
import types

import pytest
import torch

from tests.test_periodic_train_host import FAKE, _dyn, _nets, _plan


@pytest.fixture(scope="module")
def L():
    from l2hmc_amd import _lib, build as lbuild
    lbuild.build()
    return _lib.lib()


def _flags():
    from l2hmc_amd import _lib
    both = _lib.PLAN_PERIODIC | _lib.PLAN_PERIODIC_TRAIN
    return both, both | _lib.PLAN_PERIODIC_TAPE


def _nets128(packed=True, hidden=512):
    x, v, old = _nets(128, hidden=hidden)
    for d in (x, v, old):
        d.packed = FAKE if packed else None
    return x, v, old


def _q(L, plan):
    return L.l2hmc_gauge_plan_train_fused(C.byref(plan))


def test_flag_and_query_are_declared_with_the_same_value_on_both_sides(L):
    from l2hmc_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "#define L2HMC_PLAN_PERIODIC_TAPE 2048" in header
    assert "int l2hmc_gauge_plan_train_fused(const l2hmc_gauge_plan* plan);" in header
    assert "gate" in header.split("#define L2HMC_PLAN_PERIODIC_TAPE 2048")[1].split("typedef struct")[0]
    assert _lib.PLAN_PERIODIC_TAPE == 2048
    assert hasattr(L, "l2hmc_gauge_plan_train_fused")


@pytest.mark.parametrize("T,X", [(8, 8), (4, 16), (16, 4)])
def test_query_is_one_for_the_flagged_plans_with_the_kernel(L, T, X):
    from l2hmc_amd import _lib
    both, tape = _flags()
    nets = _nets128()
    for extra in (0, _lib.PLAN_PERIODIC_STEP, _lib.PLAN_RECOMPUTE, _lib.PLAN_SELECTED_ONLY):
        assert _q(L, _plan(tape | extra, T, X, nets=nets)) == 1
    # the same plans without the flag, and the flagged ones under L2HMC_PLAN_LAYERED: layer by layer
    for extra in (0, _lib.PLAN_PERIODIC_STEP):
        assert _q(L, _plan(both | extra, T, X, nets=nets)) == 0
        assert _q(L, _plan(tape | extra | _lib.PLAN_LAYERED, T, X, nets=nets)) == 0
    # a flagged plan without the packed image of either network
    for drop in (0, 1):
        nets_np = list(_nets128())
        nets_np[drop].packed = None
        assert _q(L, _plan(tape, T, X, nets=tuple(nets_np))) == 0
    assert _q(L, _plan(tape, T, X, nets=_nets128(packed=False))) == 0


def test_query_is_zero_where_the_flag_is_only_carried(L):
    both, tape = _flags()

    def packed(D):
        nets = _nets(D)
        for d in nets:
            d.packed = FAKE
        return nets
    for T, X in ((4, 4), (16, 16), (2, 8), (4, 8)):
        assert _q(L, _plan(tape, T, X, nets=packed(2 * T * X))) == 0
        assert _q(L, _plan(both, T, X, nets=packed(2 * T * X))) == 0
    # D = 128 at another hidden width
    assert _q(L, _plan(tape, 8, 8, nets=_nets128(hidden=256))) == 0


def test_query_answers_for_the_reference_mode_as_the_forward_branches(L):
    from l2hmc_amd import _lib
    _, _, old = _nets128()
    assert _q(L, _plan(0, 8, 8, nets=(old, old, old))) == 1
    assert _q(L, _plan(_lib.PLAN_LAYERED, 8, 8, nets=(old, old, old))) == 0
    _, _, bare = _nets128(packed=False)
    assert _q(L, _plan(0, 8, 8, nets=(bare, bare, bare))) == 0
    _, _, small = _nets(32)
    assert _q(L, _plan(0, 4, 4, nets=(small, small, small))) == 0
    # plans the training entries refuse: negative, with the reason
    assert _q(L, _plan(0, 8, 8, hmc=1, nets=(old, old, old))) < 0 and b"hmc" in L.l2hmc_last_error()
    assert _q(L, _plan(_lib.PLAN_PERIODIC, 8, 8, nets=_nets128())) < 0
    assert b"layered-training entries" in L.l2hmc_last_error()
    assert L.l2hmc_gauge_plan_train_fused(None) < 0


def test_flag_rules(L):
    from l2hmc_amd import _lib
    from l2hmc_amd._lib import GaugePlan
    both, tape = _flags()
    x, v, old = _nets128()
    for flags, nets in ((_lib.PLAN_PERIODIC_TAPE, (old, old, old)),                                 # alone
                        (_lib.PLAN_PERIODIC_TAPE | _lib.PLAN_PERIODIC, (x, v, old)),               # without _TRAIN
                        (_lib.PLAN_PERIODIC_TAPE | _lib.PLAN_PERIODIC_TRAIN, (old, old, old))):    # without _PERIODIC
        plan = _plan(flags, 8, 8, nets=nets)
        # refused by the training entries, by the query and by the plan check of the sampling entries, naming the flag
        for call in (lambda: _q(L, plan), lambda: L.l2hmc_gauge_plan_fused(C.byref(plan))):
            assert call() < 0
            msg = L.l2hmc_last_error()
            assert b"L2HMC_PLAN_PERIODIC_TAPE" in msg, msg
            assert b"L2HMC_PLAN_PERIODIC_TRAIN" in msg.replace(b"L2HMC_PLAN_PERIODIC_TAPE", b""), msg
        assert L.l2hmc_gauge_train_forward(C.byref(plan), 1.0, None, None, None, 4, None, None, None, None, None, 0,
                                           None) == 1
        assert b"L2HMC_PLAN_PERIODIC_TAPE" in L.l2hmc_last_error()
    # plain HMC ignores it
    for flags in (_lib.PLAN_PERIODIC_TAPE, tape, _lib.PLAN_PERIODIC_TAPE | _lib.PLAN_PERIODIC):
        assert L.l2hmc_gauge_plan_fused(C.byref(GaugePlan(T=8, X=8, num_steps=3, hmc=1, flags=flags, masks=FAKE))) == 1
    # the sampling entries take the flagged plan as they take the unflagged one: the flag alone selects no sampling kernel
    assert L.l2hmc_gauge_plan_fused(C.byref(_plan(tape, 8, 8, nets=(x, v, old)))) == 0
    assert L.l2hmc_gauge_plan_fused(C.byref(_plan(tape | _lib.PLAN_PERIODIC_STEP, 8, 8, nets=(x, v, old)))) == 1
    # ConvNet3D under it is refused as under L2HMC_PLAN_PERIODIC_TRAIN
    assert _q(L, _plan(tape | _lib.PLAN_CONV3D, 8, 8, nets=(x, v, old))) < 0 and b"GenericNet" in L.l2hmc_last_error()


@pytest.mark.parametrize("T,X,N", [(8, 8, 10), (4, 16, 2), (4, 4, 3), (16, 16, 5)])
def test_no_workspace_size_depends_on_the_flag(L, T, X, N):
    from l2hmc_amd import _lib
    both, tape = _flags()
    nets = _nets(2 * T * X)
    for d in nets:
        d.packed = FAKE
    for extra in (0, _lib.PLAN_PERIODIC_STEP):
        a, b = _plan(both | extra, T, X, N, nets=nets), _plan(tape | extra, T, X, N, nets=nets)
        for rows in (1, 5, 18, 19, 4096):
            assert L.l2hmc_gauge_train_ws_bytes(C.byref(a), rows) == L.l2hmc_gauge_train_ws_bytes(C.byref(b), rows) > 0
            assert L.l2hmc_gauge_ws_bytes(C.byref(a), rows) == L.l2hmc_gauge_ws_bytes(C.byref(b), rows) > 0
            assert L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(a), rows) == L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(b), rows)


# ---- Python --------------------------------------------------------------------------------------------------------
def test_fused_forward_needs_both_and_is_refused_before_any_library_call(monkeypatch):
    from l2hmc_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the refusal must not reach the library or torch.cuda")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "stream_ptr", boom)
    with pytest.raises(ValueError, match=r"fused_forward=True.*needs periodic=True and tiled_train=True"):
        _dyn(fused_forward=True)
    with pytest.raises(ValueError, match=r"fused_forward=True.*needs tiled_train=True with"):
        _dyn(periodic=True, fused_forward=True)
    with pytest.raises(ValueError, match=r"fused_forward=True.*needs tiled_train=True with"):
        _dyn(periodic=True, whole_step=True, fused_forward=True)
    with pytest.raises(ValueError, match=r"fused_forward=True.*needs periodic=True with"):
        _dyn(tiled_train=True, fused_forward=True)
    assert _dyn().fused_forward is False and _dyn(periodic=True, tiled_train=True).fused_forward is False   # opt-in
    dyn = _dyn(periodic=True, tiled_train=True, fused_forward=1)
    assert dyn.fused_forward is True and dyn.whole_step is False                              # coerced with bool
    assert _dyn(periodic=True, tiled_train=True, fused_forward=0).fused_forward is False
    assert _dyn(periodic=True, tiled_train=True, whole_step=True, fused_forward=True).whole_step is True   # they compose
    assert _dyn(hmc=True, fused_forward=True).fused_forward is True           # no networks: carried, changes nothing


def test_plan_carries_the_flag_only_where_it_means_something(monkeypatch):
    from l2hmc_amd import _lib
    monkeypatch.setattr(_lib, "dev_ptr", lambda t, dtype=torch.float32, name="tensor": 16)   # (host tensors: no address)
    hmc = _dyn(periodic=True, tiled_train=True, fused_forward=True, hmc=True)
    assert not hmc._plan().flags & (_lib.PLAN_PERIODIC | _lib.PLAN_PERIODIC_TRAIN | _lib.PLAN_PERIODIC_TAPE)
    for ff, ws in ((True, False), (False, False), (True, True), (False, True)):
        dyn = _dyn(periodic=True, tiled_train=True, fused_forward=ff, whole_step=ws)      # 3x5: no kernel, flag carried
        st = _lib.DenseNet(D=30, H=120, Ka=30, Kb=60)
        dyn.position_fn = types.SimpleNamespace(pack=lambda: st)
        dyn.momentum_fn = types.SimpleNamespace(pack=lambda: st)
        monkeypatch.setattr(dyn, "_heads_image", lambda plan: None)
        flags = dyn._plan().flags
        assert flags & _lib.PLAN_PERIODIC and flags & _lib.PLAN_PERIODIC_TRAIN
        assert bool(flags & _lib.PLAN_PERIODIC_TAPE) is ff and bool(flags & _lib.PLAN_PERIODIC_STEP) is ws
