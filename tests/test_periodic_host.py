"""Host-side checks of the torus-exact L2HMC mode (`GaugeDynamics(periodic=True)`), no GPU:

- the float64 reference of tests/periodic_ref.py has the properties the mode exists for -- its log-determinant is the
  Jacobian's, the trajectory commutes with 2 pi shifts of any link, and backward(wrap(forward(x))) returns to x --, so
  the GPU tests compare against a reference that is itself checked;
- construction: refusals, network widths, the plan flag, state loading across modes, the wrappers' argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import periodic_ref as PR

TWO_PI = 2 * np.pi


def _model(T, X, N, eps, regime="stress", cls=PR.NumpyPeriodic, **kw):
    xp, vp = PR.periodic_weights(T, X, regime=regime)
    return cls(T, X, N, eps, PR.masks_for(N, 2 * T * X), xp, vp, **kw)


@pytest.mark.parametrize("bwd", [False, True])
def test_reference_logdet_is_the_jacobians(bwd):
    """2 x 2 lattice (D = 8): sumlogdet = log |det d(x', v') / d(x, v)| from torch.autograd, to 1e-10."""
    T = X = 2
    D = 8
    tm = _model(T, X, 2, 0.25, cls=PR.TorchPeriodic)
    rng = np.random.default_rng(3)
    z0 = torch.tensor(np.concatenate([rng.uniform(0, TWO_PI, D), rng.standard_normal(D)]), dtype=torch.float64)

    def f(z):
        x, v, _, _ = tm.trajectory(z[None, :D], z[None, D:], 2.5, bwd)
        return torch.cat([x[0], v[0]])
    J = torch.autograd.functional.jacobian(f, z0)
    _, logabs = torch.linalg.slogdet(J)
    with torch.no_grad():
        ld = tm.trajectory(z0[None, :D], z0[None, D:], 2.5, bwd)[3]
    assert abs(float(ld)) > 1e-3, "a net that does nothing proves nothing"
    assert abs(float(logabs) - float(ld)) <= 1e-10


@pytest.mark.parametrize("T,X", [(2, 2), (3, 5)])
def test_reference_commutes_with_two_pi_shifts(T, X):
    D, B = 2 * T * X, 5
    m = _model(T, X, 3, 0.2)
    rng = np.random.default_rng(11)
    x, v = rng.uniform(0, TWO_PI, (B, D)), rng.standard_normal((B, D))
    k = rng.integers(-3, 4, (B, D))
    for bwd in (False, True):
        x1, v1, p1, l1 = m.trajectory(x, v, 2.0, bwd)
        x2, v2, p2, l2 = m.trajectory(x + TWO_PI * k, v, 2.0, bwd)
        assert PR.angdist(x1, x2).max() <= 1e-9
        assert np.abs(v1 - v2).max() <= 1e-9 and np.abs(l1 - l2).max() <= 1e-9 and np.abs(p1 - p2).max() <= 1e-9
        assert np.abs(l1).mean() > 1e-3


@pytest.mark.parametrize("T,X", [(2, 2), (3, 5)])
def test_reference_is_reversible_on_the_torus(T, X):
    D, B = 2 * T * X, 5
    m = _model(T, X, 3, 0.2)
    rng = np.random.default_rng(12)
    x, v = rng.uniform(0, TWO_PI, (B, D)), rng.standard_normal((B, D))
    x1, v1, _, l1 = m.trajectory(x, v, 2.0, False)
    x2, v2, _, l2 = m.trajectory(np.mod(x1, TWO_PI), v1, 2.0, True)
    assert PR.angdist(x2, x).max() <= 1e-9 and np.abs(v2 - v).max() <= 1e-9
    assert np.abs(l1 + l2).max() <= 1e-9              # the inverse map's log-determinant


# ---- construction --------------------------------------------------------------------------------------------------
def _dyn(T=3, X=5, **kw):
    from l2hmc_amd import GaugeLattice, GaugeDynamics
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=4, rand=False)
    return GaugeDynamics(lat, lat.get_energy_function(), eps=0.2, num_steps=2, device=torch.device("cpu"), **kw)


def test_periodic_networks_have_the_documented_widths():
    dyn = _dyn(periodic=True)
    D, Hn = 30, 120
    assert dyn.periodic is True
    assert tuple(dyn.position_fn.x_layer.kernel.shape) == (2 * D, Hn)      # XNet([v, m x, t]): x is the second input
    assert tuple(dyn.position_fn.v_layer.kernel.shape) == (D, Hn)
    assert tuple(dyn.momentum_fn.v_layer.kernel.shape) == (2 * D, Hn)      # VNet([x, force, t]): x is the first input
    assert tuple(dyn.momentum_fn.x_layer.kernel.shape) == (D, Hn)
    plain = _dyn()
    assert plain.periodic is False
    for net in (plain.position_fn, plain.momentum_fn):
        assert tuple(net.x_layer.kernel.shape) == (D, Hn) and tuple(net.v_layer.kernel.shape) == (D, Hn)
    # the packed first layer is [Ka + Kb] = 3 D wide, Ka from the first-input layer
    xs, vs = dyn.position_fn.state_dict(), dyn.momentum_fn.state_dict()
    assert xs["v_layer/W"].shape[0] + xs["x_layer/W"].shape[0] == 3 * D
    assert vs["v_layer/W"].shape[0] == 2 * D and vs["x_layer/W"].shape[0] == D


def test_periodic_same_seed_keeps_the_draw_order_and_factors():
    """The layers are created in the reference's order; only the fan-in of the layer that reads x changes, and with
    it that layer's scale sqrt(1.3 * 2 * factor / fan_in)."""
    from l2hmc_amd.network import GenericNet
    kw = dict(device=torch.device("cpu"), x_dim=8, num_hidden=4096, factor=2., links_shape=(2, 2, 2))
    a = GenericNet(model_name='XNet', rng=np.random.RandomState(5), **kw)
    b = GenericNet(model_name='XNet', rng=np.random.RandomState(5), angle_input='second', **kw)
    assert float(b.x_layer.kernel.std() / a.x_layer.kernel.std()) == pytest.approx(np.sqrt(0.5), rel=0.03)
    assert float(b.v_layer.kernel.std() / a.v_layer.kernel.std()) == pytest.approx(1.0, rel=0.03)
    with pytest.raises(ValueError, match="angle_input"):
        GenericNet(model_name='XNet', angle_input='both', **kw)


def test_periodic_refusals_at_construction(monkeypatch):
    from l2hmc_amd import _lib
    with pytest.raises(NotImplementedError, match="generic"):
        _dyn(T=4, X=4, periodic=True, network_arch='conv3D')
    dyn = _dyn(periodic=True, hmc=True)               # no networks: accepted, changes nothing
    assert dyn.periodic is True
    monkeypatch.setattr(_lib, "dev_ptr", lambda t, dtype=torch.float32, name="tensor": 16)   # (host tensors: no address)
    assert not dyn._plan().flags & _lib.PLAN_PERIODIC


def test_loading_a_state_of_the_other_mode_names_the_mode():
    per, plain = _dyn(periodic=True), _dyn()
    with pytest.raises(ValueError, match="x_layer: shape .*other `periodic` mode"):
        per.position_fn.load_state({k: v.numpy() for k, v in plain.position_fn.state_dict().items()})
    with pytest.raises(ValueError, match="v_layer: shape .*other `periodic` mode"):
        plain.momentum_fn.load_state({k: v.numpy() for k, v in per.momentum_fn.state_dict().items()})
    xp, vp = PR.periodic_weights(3, 5)
    per.position_fn.load_state(xp)
    per.momentum_fn.load_state(vp)
    got = per.position_fn.state_dict()
    assert all(np.allclose(got[k].numpy().reshape(np.shape(v)), v, rtol=1e-6, atol=1e-7) for k, v in xp.items())


def test_autograd_on_a_periodic_dynamics_is_refused():
    from l2hmc_amd import autograd
    dyn = _dyn(periodic=True)
    with pytest.raises(NotImplementedError, match="periodic=True.*layered reverse walk"):
        autograd.check_differentiable(dyn)


def test_trainer_takes_the_layered_walk_on_a_periodic_dynamics():
    import types
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    tr = types.SimpleNamespace(dynamics=types.SimpleNamespace(periodic=True, network_arch='generic'), layered=None)
    assert GaugeTrainer._use_layered(tr) is True
    tr.layered = False
    with pytest.raises(NotImplementedError, match="tiled"):
        GaugeTrainer._use_layered(tr)


# ---- the C boundary ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from l2hmc_amd import _lib, build as lbuild
    lbuild.build()
    return _lib.lib()


def test_new_entries_are_declared_and_check_their_arguments(L):
    from l2hmc_amd import _lib
    names = ("l2hmc_lf_update_x_ncp", "l2hmc_lf_update_x_ncp_vjp", "l2hmc_u1_angle_features",
             "l2hmc_u1_angle_features_vjp")
    for n in names:
        assert n in _lib.declared_symbols() and n in _lib._PROTOS and hasattr(L, n)
    with open(_lib.HEADER_PATH) as f:
        assert "#define L2HMC_PLAN_PERIODIC 256" in f.read()
    assert _lib.PLAN_PERIODIC == 256
    assert L.l2hmc_lf_update_x_ncp(None, None, None, None, None, None, 0.1, 0, 0, 8, None, None, None) == 0
    assert L.l2hmc_lf_update_x_ncp(None, None, None, None, None, None, 0.1, 2, 4, 8, None, None, None) == 1
    assert L.l2hmc_lf_update_x_ncp(None, None, None, None, None, None, 0.1, 0, 4, 8, None, None, None) == 1
    assert b"NULL" in L.l2hmc_last_error()
    assert L.l2hmc_lf_update_x_ncp_vjp(*([None] * 6), 0.1, 1, 4, 8, *([None] * 8), None) == 1
    assert L.l2hmc_u1_angle_features(None, 0, 8, None, None) == 0
    assert L.l2hmc_u1_angle_features(None, 3, 0, None, None) == 1
    assert L.l2hmc_u1_angle_features_vjp(None, None, 15, 3, 8, None, None) == 1       # ldf < 2 D
    assert b"ldf" in L.l2hmc_last_error()


def test_plan_flag_sets_the_widths_and_switches_the_whole_step_kernels_off(L):
    from l2hmc_amd import _lib
    D, Hn = 128, 512
    fake = 16                                          # any non-NULL address: host checks only
    w = dict(w1_t=fake, wt=fake, b1=fake, wh_t=fake, bh=fake, whd_t=fake, bhd=fake, coeff_s=fake, coeff_q=fake)
    xnet = _lib.DenseNet(D=D, H=Hn, Ka=D, Kb=2 * D, **w)
    vnet = _lib.DenseNet(D=D, H=Hn, Ka=2 * D, Kb=D, **w)
    plan = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=0, flags=_lib.PLAN_PERIODIC, masks=fake, xnet=xnet, vnet=vnet)
    assert L.l2hmc_gauge_plan_fused(C.byref(plan)) == 0
    old = _lib.DenseNet(D=D, H=Hn, Ka=D, Kb=D, **w)
    bad = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=0, flags=_lib.PLAN_PERIODIC, masks=fake, xnet=old, vnet=old)
    assert L.l2hmc_gauge_plan_fused(C.byref(bad)) == -1
    assert b"periodic XNet expects Ka=128, Kb=256" in L.l2hmc_last_error()
    unflagged = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=0, flags=0, masks=fake, xnet=xnet, vnet=vnet)
    assert L.l2hmc_gauge_plan_fused(C.byref(unflagged)) == -1
    # the workspace grows by the features and the doubled masks only under the flag
    base = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=0, flags=_lib.PLAN_LAYERED | _lib.PLAN_RECOMPUTE, masks=fake,
                          xnet=old, vnet=old)
    rows = 64
    extra = L.l2hmc_gauge_ws_bytes(C.byref(plan), rows) - L.l2hmc_gauge_ws_bytes(C.byref(base), rows)
    assert extra == 4 * (rows * 2 * D + 2 * 3 * 2 * D)
    # plain HMC ignores the flag
    hmc = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=1, flags=_lib.PLAN_PERIODIC, masks=fake)
    assert L.l2hmc_gauge_plan_fused(C.byref(hmc)) == 1
    # the tiled training entries refuse the plan, and say where it trains
    assert L.l2hmc_gauge_train_forward(C.byref(plan), 1.0, None, None, None, 4, None, None, None, None, None, 0,
                                       None) == 1
    assert b"L2HMC_PLAN_PERIODIC" in L.l2hmc_last_error() and b"layered" in L.l2hmc_last_error()
    conv = _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=0, flags=_lib.PLAN_PERIODIC | _lib.PLAN_CONV3D, masks=fake,
                          xnet=xnet, vnet=vnet)
    assert L.l2hmc_gauge_plan_fused(C.byref(conv)) == -1 and b"GenericNet" in L.l2hmc_last_error()


def test_wrappers_check_their_tensors_before_the_library(monkeypatch):
    from l2hmc_amd import _lib, ops_periodic

    def boom(*a, **k):
        raise AssertionError("validation must not reach the library or torch.cuda")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "stream_ptr", boom)
    B, D = 3, 8
    z = lambda *s: torch.zeros(*s)        # noqa: E731
    with pytest.raises(RuntimeError, match="^x: .*no CPU fallback"):
        ops_periodic.lf_update_x_ncp(z(B, D), z(B, D), z(D), z(B, D), z(B, D), z(B, D), 0.1, 0)
    with pytest.raises(RuntimeError, match="^x: .*no CPU fallback"):
        ops_periodic.u1_angle_features(z(B, D))
    with pytest.raises(RuntimeError, match="^x: .*no CPU fallback"):
        ops_periodic.u1_angle_features_vjp(z(B, D), z(B, 2 * D), z(B, D))
    with pytest.raises(RuntimeError, match="^x: .*no CPU fallback"):
        ops_periodic.lf_update_x_ncp_vjp(z(B, D), z(B, D), z(D), z(B, D), z(B, D), z(B, D), 0.1, 1, z(B, D), z(B))
    # one offender among stand-ins for good GPU tensors: the error names it
    real = _lib.dev_ptr
    monkeypatch.setattr(_lib, "dev_ptr", lambda t, dtype=torch.float32, name="tensor":
                        1 if isinstance(t, torch.Tensor) else real(t, dtype, name))
    with pytest.raises(TypeError, match="^keep: expected a torch.Tensor, got ndarray"):
        ops_periodic.lf_update_x_ncp(z(B, D), z(B, D), np.zeros(D, np.float32), z(B, D), z(B, D), z(B, D), 0.1, 0)
    with pytest.raises(TypeError, match="^dlogdet: expected a torch.Tensor, got ndarray"):
        ops_periodic.lf_update_x_ncp_vjp(z(B, D), z(B, D), z(D), z(B, D), z(B, D), z(B, D), 0.1, 1, z(B, D),
                                         np.zeros(B, np.float32))
    with pytest.raises(ValueError, match="dfeat"):
        ops_periodic.u1_angle_features_vjp(z(B, D), z(B, D), z(B, D))
