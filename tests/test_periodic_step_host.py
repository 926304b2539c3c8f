"""Host-side checks of the torus-exact mode's whole-step kernel selection (`GaugeDynamics(periodic=True,
whole_step=True)`, L2HMC_PLAN_PERIODIC_STEP), no GPU: the flag's value, what `l2hmc_gauge_plan_fused` answers for it on
fake non-NULL addresses (host checks only, as tests/test_periodic_host.py does), the packed image's size for the two
network shapes of a periodic plan at D = 128, and the constructor's refusal."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from l2hmc_amd import _lib, build as lbuild
    lbuild.build()
    return _lib.lib()


FAKE = 16                                              # any non-NULL address: host checks only
D, HN = 128, 512


def _nets(packed=FAKE):
    from l2hmc_amd import _lib
    w = dict(w1_t=FAKE, wt=FAKE, b1=FAKE, wh_t=FAKE, bh=FAKE, whd_t=FAKE, bhd=FAKE, coeff_s=FAKE, coeff_q=FAKE)
    xnet = _lib.DenseNet(D=D, H=HN, Ka=D, Kb=2 * D, packed=packed, **w)
    vnet = _lib.DenseNet(D=D, H=HN, Ka=2 * D, Kb=D, packed=packed, **w)
    old = _lib.DenseNet(D=D, H=HN, Ka=D, Kb=D, packed=packed, **w)
    return xnet, vnet, old


def test_flag_is_declared_with_the_same_value_on_both_sides():
    from l2hmc_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        assert "#define L2HMC_PLAN_PERIODIC_STEP 512" in f.read()
    assert _lib.PLAN_PERIODIC_STEP == 512


def test_plan_check_selects_the_whole_step_kernel_only_with_both_flags(L):
    from l2hmc_amd import _lib
    xnet, vnet, old = _nets()
    both = _lib.PLAN_PERIODIC | _lib.PLAN_PERIODIC_STEP

    def fused(flags, T=8, X=8, hmc=0, xn=xnet, vn=vnet):
        plan = _lib.GaugePlan(T=T, X=X, num_steps=3, hmc=hmc, flags=flags, masks=FAKE, xnet=xn, vnet=vn)
        return L.l2hmc_gauge_plan_fused(C.byref(plan))
    assert fused(both) == 1
    assert fused(both, T=4, X=16) == 1 and fused(both, T=16, X=4) == 1      # D = 128 with a power-of-two X
    assert fused(_lib.PLAN_PERIODIC) == 0                                    # opt-in: the unflagged plan is unchanged
    assert fused(both | _lib.PLAN_LAYERED) == 0
    # another lattice carries the flag and runs layer by layer
    x6 = _lib.DenseNet(D=72, H=288, Ka=72, Kb=144, packed=FAKE, **{k: FAKE for k in (
        "w1_t", "wt", "b1", "wh_t", "bh", "whd_t", "bhd", "coeff_s", "coeff_q")})
    v6 = _lib.DenseNet(D=72, H=288, Ka=144, Kb=72, packed=FAKE, **{k: FAKE for k in (
        "w1_t", "wt", "b1", "wh_t", "bh", "whd_t", "bhd", "coeff_s", "coeff_q")})
    assert fused(both, T=6, X=6, xn=x6, vn=v6) == 0
    # no packed image, no kernel
    xu, vu, _ = _nets(packed=None)
    assert fused(both, xn=xu, vn=vu) == 0
    # the step flag alone is refused by the plan check, which names both flags
    assert fused(_lib.PLAN_PERIODIC_STEP, xn=old, vn=old) == -1
    msg = L.l2hmc_last_error()
    assert b"L2HMC_PLAN_PERIODIC_STEP" in msg and b"L2HMC_PLAN_PERIODIC" in msg.replace(b"L2HMC_PLAN_PERIODIC_STEP", b"")
    # plain HMC ignores both
    hmc = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=1, flags=both, masks=FAKE)
    assert L.l2hmc_gauge_plan_fused(C.byref(hmc)) == 1
    hmc1 = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=1, flags=_lib.PLAN_PERIODIC_STEP, masks=FAKE)
    assert L.l2hmc_gauge_plan_fused(C.byref(hmc1)) == 1
    # the tiled training entries refuse the flagged plan as they refuse the unflagged one
    plan = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=0, flags=both, masks=FAKE, xnet=xnet, vnet=vnet)
    assert L.l2hmc_gauge_train_forward(C.byref(plan), 1.0, None, None, None, 4, None, None, None, None, None, 0,
                                       None) == 1
    assert b"L2HMC_PLAN_PERIODIC" in L.l2hmc_last_error() and b"layered" in L.l2hmc_last_error()
    # the workspace does not depend on the step flag
    base = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=0, flags=_lib.PLAN_PERIODIC, masks=FAKE, xnet=xnet, vnet=vnet)
    for B in (5, 19, 2048):
        assert L.l2hmc_gauge_ws_bytes(C.byref(plan), B) == L.l2hmc_gauge_ws_bytes(C.byref(base), B)
        assert L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B) == L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(base), B)


def test_pack_bytes_of_the_periodic_network_shapes(L):
    from l2hmc_amd import _lib
    xnet, vnet, _ = _nets()
    want = 4 * (384 * 512 + 512 * 512 + 384 * 512)          # the 4-wave image alone: no sub-tile image behind it
    assert L.l2hmc_dense_pack_bytes(C.byref(xnet)) == want
    assert L.l2hmc_dense_pack_bytes(C.byref(vnet)) == want
    assert L.l2hmc_dense_pack_bytes(C.byref(_lib.DenseNet(D=72, H=288, Ka=72, Kb=144))) == 0
    assert L.l2hmc_dense_pack_bytes(C.byref(_lib.DenseNet(D=72, H=288, Ka=72, Kb=72))) == 0
    assert L.l2hmc_dense_pack_bytes(C.byref(_lib.DenseNet(D=128, H=512, Ka=256, Kb=256))) == 0
    # the pack itself refuses NULL weights on the host
    bare = _lib.DenseNet(D=128, H=512, Ka=128, Kb=256)
    assert L.l2hmc_dense_pack(C.byref(bare), FAKE, None) == 1 and b"NULL weight" in L.l2hmc_last_error()


def _dyn(T=3, X=5, **kw):
    from l2hmc_amd import GaugeLattice, GaugeDynamics
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=4, rand=False)
    return GaugeDynamics(lat, lat.get_energy_function(), eps=0.2, num_steps=2, device=torch.device("cpu"), **kw)


def test_whole_step_needs_periodic_and_is_refused_before_any_library_call(monkeypatch):
    from l2hmc_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the refusal must not reach the library or torch.cuda")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "stream_ptr", boom)
    with pytest.raises(ValueError, match="whole_step=True.*periodic=True"):
        _dyn(whole_step=True)
    with pytest.raises(ValueError, match="whole_step=True.*periodic=True"):
        _dyn(periodic=False, whole_step=True)
    assert _dyn().whole_step is False and _dyn(periodic=True).whole_step is False      # opt-in
    dyn = _dyn(periodic=True, whole_step=True)
    assert dyn.whole_step is True and dyn.periodic is True
    assert _dyn(hmc=True, whole_step=True).whole_step is True       # no networks: carried, changes nothing


def test_plan_carries_the_flag_only_where_it_means_something(monkeypatch):
    from l2hmc_amd import _lib
    import types
    monkeypatch.setattr(_lib, "dev_ptr", lambda t, dtype=torch.float32, name="tensor": 16)   # (host tensors: no address)
    hmc = _dyn(periodic=True, whole_step=True, hmc=True)
    assert not hmc._plan().flags & (_lib.PLAN_PERIODIC | _lib.PLAN_PERIODIC_STEP)
    # an L2HMC plan needs packed networks: stand-ins, and no heads image (host only)
    for ws in (True, False):
        dyn = _dyn(periodic=True, whole_step=ws)
        st = _lib.DenseNet(D=30, H=120, Ka=30, Kb=60)
        dyn.position_fn = types.SimpleNamespace(pack=lambda: st)
        dyn.momentum_fn = types.SimpleNamespace(pack=lambda: st)
        monkeypatch.setattr(dyn, "_heads_image", lambda plan: None)
        flags = dyn._plan().flags
        assert flags & _lib.PLAN_PERIODIC
        assert bool(flags & _lib.PLAN_PERIODIC_STEP) is ws


def test_trainer_takes_the_layered_walk_whatever_the_flag():
    import types
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    tr = types.SimpleNamespace(dynamics=types.SimpleNamespace(periodic=True, whole_step=True, network_arch='generic'),
                               layered=None)
    assert GaugeTrainer._use_layered(tr) is True
