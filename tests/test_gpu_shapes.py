"""The Python boundary on the GPU, positive cases only: every accepted FORM of a caller tensor (a position as
[B, T, X, 2], numpy float64 draws) gives the bits of the canonical [B, D] float32 device tensors, and the stateless
sub-updates may write their state IN PLACE ("out may alias in", include/l2hmc_hip.h), which no other test does.

No test here passes a wrongly shaped tensor to anything: if a check were missing, that call would be the out-of-bounds
access the checks exist to prevent.  The refusals are proved on the host (tests/test_shapes_host.py), where the
backend is a stub.  Every buffer below has exactly the size its kernel reads or writes."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_ops import _raw

pytestmark = pytest.mark.gpu

N_STEPS, EPS, BETA = 2, 0.1, 2.5


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    return l2hmc_amd


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda")


def _gauge(T, X, B):
    xp, vp = H.gauge_weights(T, X, regime="mild")
    orc = H.gauge_oracle(T, X, N_STEPS, EPS, xp, vp)
    dyn = H.gauge_hip(T, X, N_STEPS, EPS, xp, vp, orc.mask, B)
    x, v0f, v0b, coin, u = H.gauge_inputs(B, 2 * T * X)
    z = np.random.default_rng(11).standard_normal(x.shape)
    return dyn, dict(x=x, v0f=v0f, v0b=v0b, coin=coin, u=u, z=z)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)


# ------------------------------------------------------------------------------------------------ accepted forms
@pytest.mark.parametrize("T,X,B", [(4, 6, 9), (2, 2, 5)])
def test_gauge_dynamics_forms_give_the_bits_of_device_tensors(la, T, X, B):
    dyn, i = _gauge(T, X, B)
    lattice = (B, T, X, 2)
    draws = lambda f: dict(momentum_f=f(i["v0f"]), momentum_b=f(i["v0b"]), coin=f(i["coin"]), u=f(i["u"]))  # noqa: E731
    want = dyn.apply_transition(_dev(i["x"]), BETA, **draws(_dev))
    assert all(tuple(t.shape) == s for t, s in zip(want, [(B, 2 * T * X)] * 2 + [(B,), (B, 2 * T * X)]))
    _same(dyn.apply_transition(i["x"].reshape(lattice), BETA, **draws(np.asarray)), want)      # numpy float64
    _same(dyn.apply_transition(_dev(i["x"]).reshape(lattice), BETA, momentum_f=i["v0f"].reshape(lattice),
                               momentum_b=_dev(i["v0b"], torch.float64), coin=list(i["coin"]), u=_dev(i["u"])), want)
    ladder = np.full(B, BETA)                          # the layer-by-layer ladder branch, checked among its own forms
    want = dyn.apply_transition(_dev(i["x"]), ladder, **draws(_dev))
    _same(dyn.apply_transition(i["x"].reshape(lattice), ladder, **draws(np.asarray)), want)
    for forward in (True, False):
        want = dyn.transition_kernel(_dev(i["x"]), BETA, forward=forward, momentum=_dev(i["v0f"]), return_logdet=True)
        got = dyn.transition_kernel(i["x"].reshape(lattice), BETA, forward=forward,
                                    momentum=i["v0f"].reshape(lattice), return_logdet=True)
        _same(got, want)


@pytest.mark.parametrize("T,X,B", [(4, 6, 9), (2, 2, 5)])
def test_gauge_trainer_forms_give_the_bits_of_device_tensors(la, T, X, B):
    dyn, i = _gauge(T, X, B)
    tr = la.GaugeTrainer(dyn)
    rng = np.random.default_rng(12)
    dz = (rng.standard_normal(i["x"].shape), rng.standard_normal(i["x"].shape), rng.uniform(size=B),
          rng.uniform(size=B))
    dx = (i["v0f"], i["v0b"], i["coin"], i["u"])
    want = tr.calc_loss_and_grads(_dev(i["x"]), BETA, z=_dev(i["z"]), draws_x=tuple(_dev(a) for a in dx),
                                  draws_z=tuple(_dev(a) for a in dz))
    want_grads, draws = tr.grads.clone(), dyn._draws
    got = tr.calc_loss_and_grads(i["x"].reshape(B, T, X, 2), BETA, z=i["z"].reshape(B, T, X, 2), draws_x=dx,
                                 draws_z=list(dz))
    _same(got, want)
    assert torch.equal(tr.grads, want_grads)
    assert bool(torch.isfinite(want_grads).all()) and float(want_grads.abs().max()) > 0
    assert dyn._draws == draws, "every draw was injected"


def test_toy_propose_forms_give_the_bits_of_device_tensors(la):
    dim, B, nodes, N = 2, 5, 10, 3
    m = H.mog_target_oracle()
    xp, vp = H.mlp_weights(dim, nodes, regime="mild")
    dyn = la.Dynamics(dim, la.GMM(m.mus, m.sigmas, m.pis).get_energy_function(), trajectory_length=N, eps=0.1,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes), seed=7)
    dyn.XNet.load_state(xp)
    dyn.VNet.load_state(vp)
    rng = np.random.default_rng(13)
    x, vf, vb = (rng.standard_normal((B, dim)) for _ in range(3))
    bits, u = rng.integers(0, 2, B).astype(np.float64), rng.uniform(size=B)
    assert 0 < bits.sum() < B
    with torch.no_grad():
        want = la.propose(_dev(x), dyn, init_v=_dev(vf), init_v_backward=_dev(vb), dir_bits=_dev(bits), u=_dev(u),
                          do_mh_step=True)
        got = la.propose(x, dyn, init_v=vf, init_v_backward=vb, dir_bits=bits, u=u, do_mh_step=True)
        _same((*got[:3], *got[3]), (*want[:3], *want[3]))
        for fn in (dyn.forward, dyn.backward):
            _same(fn(x, init_v=vf, log_jac=True), fn(_dev(x), init_v=_dev(vf), log_jac=True))
        _same([t for pair in dyn.both(x, vf, vb) for t in pair],
              [t for pair in dyn.both(_dev(x), _dev(vf), _dev(vb)) for t in pair])
    assert dyn._draws == 0, "every draw was injected"


# ------------------------------------------------------------------------------------------------ in-place operators
def _sub_update_inputs(D, rows):
    rng = np.random.default_rng(100 * D + rows)
    t = {k: _dev(rng.standard_normal((rows, D))) for k in ("v", "grad")}
    t["x"] = _dev(rng.uniform(-7, 13, (rows, D)))
    t.update({k: _dev(0.3 * rng.standard_normal((rows, D))) for k in ("S", "T", "Q")})
    t["keep"] = _dev(rng.uniform(size=D) < 0.5)
    return t


@pytest.mark.parametrize("D,rows", [(8, 5), (48, 9), (30, 70)])
@pytest.mark.parametrize("direction", [0, 1])
def test_sub_updates_in_place_equal_out_of_place(la, D, rows, direction):
    """The output pointer IS the state's: state and log-det must be the out-of-place call's, bit for bit.  D = 30: no
    multiple of a wave's 64 lanes or of 4; 70 rows: more than one workgroup, the last one partial."""
    t = _sub_update_inputs(D, rows)
    p = lambda k: t[k].data_ptr()                 # noqa: E731
    stq = (p("S"), p("T"), p("Q"))
    calls = {"l2hmc_lf_update_v": ("v", lambda s: (s, p("grad"), *stq)),
             "l2hmc_lf_update_x": ("x", lambda s: (s, p("v"), p("keep"), *stq)),
             "l2hmc_lf_update_x_ncp": ("x", lambda s: (s, p("v"), p("keep"), *stq))}
    for entry, (state, front) in calls.items():
        out, ld = torch.empty(rows, D, device="cuda"), torch.empty(rows, device="cuda")
        _raw(entry, *front(p(state)), EPS, direction, rows, D, out.data_ptr(), ld.data_ptr())
        assert bool(torch.isfinite(out).all()) and not torch.equal(out, t[state]), entry
        own, ld_own = t[state].clone(), torch.empty(rows, device="cuda")
        _raw(entry, *front(own.data_ptr()), EPS, direction, rows, D, own.data_ptr(), ld_own.data_ptr())
        assert torch.equal(own, out) and torch.equal(ld_own, ld), entry


@pytest.mark.parametrize("D,rows", [(8, 5), (48, 9), (30, 70)])
def test_wrap_angle_in_place_equals_out_of_place(la, D, rows):
    from l2hmc_amd import ops
    x = _sub_update_inputs(D, rows)["x"]
    want = ops.wrap_angle(x)
    assert float(want.min()) >= 0.0 and float(want.max()) < 2 * np.pi + 1e-6 and not torch.equal(want, x)
    raw = x.clone()
    _raw("l2hmc_wrap_angle", raw.data_ptr(), rows * D, raw.data_ptr())
    assert torch.equal(raw, want)
    own = x.clone()
    assert ops.wrap_angle(own, out=own) is own and torch.equal(own, want)
