"""The torus-exact L2HMC mode (`GaugeDynamics(periodic=True)`, L2HMC_PLAN_PERIODIC) on the device, against the float64
reference of tests/periodic_ref.py (itself checked in tests/test_periodic_host.py).

Tolerances of the operator and trajectory comparisons are not fixed numbers.  The yardstick of a case is the error of
the SAME reference evaluated in float32 (NumPy; torch float32 autograd for the reverse operators) against its float64
form on the case's inputs; the gate is four times that (the kernels' summation order, atan2f, logf, sincosf and the
hardware exp2 differ from NumPy's float32).  Positions are defined modulo 2 pi (the update returns the principal value
of atan2) and are compared by angular distance.  The operator cases of one (D, direction) share one input set of 131
rows -- the 1- and 37-row cases are its leading rows -- and its yardstick.  Measured on the MI355X, worst case of each
group as error / yardstick (gate 4), at the end of this docstring.

Properties on the device (4x4 and 3x5, stress weights, angular distance below 1e-3, the gate of
test_gpu_parity.py::test_reference_quirk_wrap_breaks_torus_reversibility): the trajectory is invertible, commutes with
2 pi shifts of any link, and backward(wrap(forward(x))) returns to x.  The reference mode with the same seed misses
the last two by about 1 rad, which the test asserts too: without the feature `periodic=True` was silently set as an
attribute and this test fails.

Training gradients: float64 autograd of the same loss, per tensor at 2e-4 of the tensor's max (the rule of
tests/test_gpu_gauge_train_layered.py), on draws for which the float64 reference has no relu pre-activation within
1e-5 of 0 and no accept exponent within 1e-5 of its clamp.

lf_update_x_ncp 2.83 (D = 72, backward, 1 row, log-det: 1.19e-6 against a yardstick of 4.2e-7), its reverse 3.17
(D = 30, backward, 1 row, d/d eps: 4.2e-7 against 1.3e-7), angle features and their reverse 1.05; transition_kernel 2.88
(6x6 mild forward, sumlogdet: 1.7e-6 against 5.9e-7), apply_transition 1.34 (3x5, p), on the ladder 1.25 (4x4, p).  The
trajectory yardsticks lie between 9.8e-8 and 2.45e-5, so the loosest gate is 9.8e-5: none is looser than the 1e-4 of
the existing trajectory tests.  Properties: invertibility, shift and wrap round trips at 2.4e-6 to 3.3e-6 rad (v, the
log-det and p within 9e-6); the reference mode with the same seed: shift 3.13 rad, wrap 3.13 rad.  Gradients: every
tensor within 1.5e-5 of its max (3x5 3.5e-6, 4x4 1.5e-5, 6x6 7.6e-6, ladder 5.0e-6)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import periodic_ref as PR
from tests.test_gpu_train import _compare, _ref_grads

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi
GATE = 4.0


def _dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device="cuda")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _err(got, want, angular=False):
    """H.relerr, with angular distance for positions."""
    if angular:
        return float(PR.angdist(got, want).max() / max(1.0, np.abs(want).max()))
    return H.relerr(got, want)


def _yard(f32, f64, angular=()):
    """The yardstick per output: the float32 reference's error against the float64 one."""
    return {k: _err(f32[k], want, k in angular) for k, want in f64.items()}


def _gate(name, got, f64, yard, angular=()):
    """got / f64: dicts of the device's and the float64 reference's outputs; every output within GATE yardsticks."""
    worst = 0.0
    for k, want in f64.items():
        err = _err(got[k], want, k in angular)
        print(f"[periodic] {name} {k}: error {err:.3e} yardstick {yard[k]:.3e} ratio {err / max(yard[k], 1e-300):.2f}")
        # (a yardstick of 0 -- dT of the forward update is u (1 - keep) eps, exact in float32 at eps = 1/4 -- asks for 0)
        assert err <= GATE * yard[k], (name, k, err, yard[k])
        worst = max(worst, err / yard[k]) if yard[k] > 0 else worst
    return worst


def _hip(T, X, N, eps, B, regime="stress", periodic=True, **kw):
    """(periodic dynamics on the device, float64 reference, float32 reference) with the same weights and masks."""
    from l2hmc_amd import GaugeLattice, GaugeDynamics
    D = 2 * T * X
    masks = PR.masks_for(N, D)
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=eps, num_steps=N, eps_trainable=True, periodic=periodic,
                        **kw)
    dyn.set_masks(masks)
    if not periodic:
        xp, vp = H.gauge_weights(T, X, regime=regime)
        dyn.position_fn.load_state(xp)
        dyn.momentum_fn.load_state(vp)
        return dyn, None, None
    xp, vp = PR.periodic_weights(T, X, regime=regime)
    dyn.position_fn.load_state(xp)
    dyn.momentum_fn.load_state(vp)
    # the device holds the float32 roundings of the weights: so do both references
    xp = {k: np.asarray(v, dtype=np.float32) for k, v in xp.items()}
    vp = {k: np.asarray(v, dtype=np.float32) for k, v in vp.items()}
    f32eps = float(np.float32(eps))
    return (dyn, PR.NumpyPeriodic(T, X, N, f32eps, masks, xp, vp, np.float64),
            PR.NumpyPeriodic(T, X, N, f32eps, masks, xp, vp, np.float32))


# ---- operators -----------------------------------------------------------------------------------------------------
ROWS = (1, 37, 131)
WIDTHS = (8, 30, 32, 72)
_OP_INPUTS = {}


def _op_inputs(D):
    """131 rows of float32 inputs: angles over several turns, with columns of every row within 1e-3 of 0, pi and
    2 pi on either side; |eps S| up to 0.5 (eps = 0.25, |S| <= 2)."""
    if D not in _OP_INPUTS:
        rng = np.random.default_rng(100 + D)
        R = max(ROWS)
        x = rng.uniform(-TWO_PI, 2 * TWO_PI, (R, D))
        edge = np.array([0.0, np.pi, TWO_PI])[rng.integers(0, 3, (R, D))] + rng.uniform(-1e-3, 1e-3, (R, D))
        x = np.where(rng.uniform(size=(R, D)) < 0.3, edge, x)
        S = rng.uniform(-2, 2, (R, D))
        S[:, 0] = 2.0 * np.sign(S[:, 0])                        # the full |eps S| = 0.5
        a = dict(x=x, v=rng.standard_normal((R, D)), keep=(rng.uniform(size=D) < 0.5).astype(np.float64), S=S,
                 T=rng.standard_normal((R, D)), Q=rng.uniform(-1, 1, (R, D)), u=rng.standard_normal((R, D)),
                 dl=rng.standard_normal(R))
        _OP_INPUTS[D] = {k: np.asarray(v, dtype=np.float32) for k, v in a.items()}
    return _OP_INPUTS[D]


EPS = 0.25


def _ncp_ref(a, d, dt):
    """The position sub-update's formulas in NumPy at dtype dt."""
    x, v, keep, S, T, Q = (a[k].astype(dt) for k in ("x", "v", "keep", "S", "T", "Q"))
    eps, half, two = dt(np.float32(EPS)), dt(0.5), dt(2)
    drift = eps * (np.exp(eps * Q) * v + T)
    s = (-eps if d else eps) * S
    es = np.exp(s)
    w = x - drift if d else x
    sh, ch = np.sin(half * w), np.cos(half * w)
    y = two * np.arctan2(es * sh, ch)
    if not d:
        y = y + drift
    omk = 1 - keep
    return dict(x=keep * x + omk * y, logdet=(omk * (s - np.log(ch * ch + es * es * sh * sh))).sum(1))


def _ncp_vjp_ref(a, d, dt):
    """Reverse of the same formulas by torch autograd at dtype dt -> dx, dv, dS, dT, dQ, deps [rows]."""
    t = {k: torch.tensor(a[k], dtype=dt, requires_grad=k in ("x", "v", "S", "T", "Q")) for k in a}
    rows = a["x"].shape[0]
    eps = torch.full((rows, 1), float(np.float32(EPS)), dtype=dt, requires_grad=True)
    x, v, keep, S, T, Q = (t[k] for k in ("x", "v", "keep", "S", "T", "Q"))
    drift = eps * (torch.exp(eps * Q) * v + T)
    s = (-eps if d else eps) * S
    es = torch.exp(s)
    w = x - drift if d else x
    sh, ch = torch.sin(0.5 * w), torch.cos(0.5 * w)
    y = 2 * torch.atan2(es * sh, ch)
    if not d:
        y = y + drift
    omk = 1 - keep
    out = ((keep * x + omk * y) * t["u"]).sum() + ((omk * (s - torch.log(ch * ch + es * es * sh * sh))).sum(1) * t["dl"]).sum()
    g = torch.autograd.grad(out, [x, v, S, T, Q, eps])
    return {k: gi.numpy().astype(np.float64).reshape(-1) if k == "deps" else gi.numpy().astype(np.float64)
            for k, gi in zip(("dx", "dv", "dS", "dT", "dQ", "deps"), g)}


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("D", WIDTHS)
def test_position_update_operator_and_its_reverse_match_float64(D, d):
    from l2hmc_amd import ops_periodic
    a = _op_inputs(D)
    f64, f32 = _ncp_ref(a, d, np.float64), _ncp_ref(a, d, np.float32)
    g64, g32 = _ncp_vjp_ref(a, d, torch.float64), _ncp_vjp_ref(a, d, torch.float32)
    assert np.abs(EPS * a["S"]).max() == 0.5
    # (the yardstick is the shared input set's: a single row's own can be an accident of rounding)
    yard, gyard = _yard(f32, f64, angular=("x",)), _yard(g32, g64)
    for rows in ROWS:
        t = {k: _dev(v if k == "keep" else v[:rows]) for k, v in a.items()}
        x1, ld = ops_periodic.lf_update_x_ncp(t["x"], t["v"], t["keep"], t["S"], t["T"], t["Q"], EPS, d)
        cut = lambda r: {k: v[:rows] for k, v in r.items()}     # noqa: E731
        _gate(f"lf_update_x_ncp D={D} d={d} rows={rows}", dict(x=_np(x1), logdet=_np(ld)), cut(f64), yard,
              angular=("x",))
        outs = ops_periodic.lf_update_x_ncp_vjp(t["x"], t["v"], t["keep"], t["S"], t["T"], t["Q"], EPS, d, t["u"],
                                                t["dl"])
        _gate(f"lf_update_x_ncp_vjp D={D} d={d} rows={rows}",
              dict(zip(("dx", "dv", "dS", "dT", "dQ", "deps"), map(_np, outs))), cut(g64), gyard)


@pytest.mark.parametrize("D", WIDTHS)
def test_angle_features_and_their_reverse_match_float64(D):
    from l2hmc_amd import ops_periodic
    a = _op_inputs(D)
    rng = np.random.default_rng(7 + D)
    df = rng.standard_normal((max(ROWS), 2 * D)).astype(np.float32)
    dx0 = rng.standard_normal((max(ROWS), D)).astype(np.float32)

    def ref(dt):
        x, g, base = a["x"].astype(dt), df.astype(dt), dx0.astype(dt)
        return dict(feat=np.concatenate([np.cos(x), np.sin(x)], axis=1),
                    dx=base + (-np.sin(x) * g[:, :D] + np.cos(x) * g[:, D:]))
    f64, yard = ref(np.float64), _yard(ref(np.float32), ref(np.float64))
    for rows in ROWS:
        x = _dev(a["x"][:rows])
        feat = ops_periodic.u1_angle_features(x)
        assert feat.shape == (rows, 2 * D)
        dx = ops_periodic.u1_angle_features_vjp(x, _dev(df[:rows]), _dev(dx0[:rows]))
        _gate(f"u1_angle_features D={D} rows={rows}", dict(feat=_np(feat), dx=_np(dx)),
              {k: v[:rows] for k, v in f64.items()}, yard)
    # an unaligned view takes the scalar form: same values
    if D % 4 == 0:
        buf = torch.zeros(max(ROWS) * D + 1, device="cuda")
        xs = buf[1:].view(max(ROWS), D)
        xs.copy_(_dev(a["x"]))
        assert torch.equal(ops_periodic.u1_angle_features(xs), ops_periodic.u1_angle_features(_dev(a["x"])))


# ---- trajectory parity ---------------------------------------------------------------------------------------------
# (T, X, N, eps, B): 3x5 the bounds-checked kernel instances, 4x4 (D = 32, H = 128) the tiled ones, 6x6 D = 72
SHAPES = [(3, 5, 3, 0.2, 37), (4, 4, 3, 0.2, 64), (6, 6, 2, 0.15, 9)]


@pytest.mark.parametrize("regime", ["mild", "stress"])
@pytest.mark.parametrize("T,X,N,eps,B", SHAPES)
def test_transition_kernel_matches_float64(T, X, N, eps, B, regime):
    dyn, r64, r32 = _hip(T, X, N, eps, B, regime)
    x, v0f, v0b, _, _ = H.gauge_inputs(B, 2 * T * X, seed=103 + T)
    x, v0f, v0b = (np.asarray(a, dtype=np.float32) for a in (x, v0f, v0b))
    beta = 2.5
    for bwd, v0 in ((False, v0f), (True, v0b)):
        xo, vo, p, sld = dyn.transition_kernel(_dev(x), beta, forward=not bwd, momentum=_dev(v0), return_logdet=True)
        names = ("x", "v", "p", "sumlogdet")
        f64, f32 = (dict(zip(names, r.trajectory(x, v0, beta, bwd))) for r in (r64, r32))
        assert np.abs(f64["sumlogdet"]).mean() > 1e-3
        _gate(f"transition_kernel {T}x{X} {regime} bwd={bwd}", dict(zip(names, map(_np, (xo, vo, p, sld)))), f64,
              _yard(f32, f64, angular=("x",)), angular=("x",))


@pytest.mark.parametrize("ladder", [False, True])
@pytest.mark.parametrize("T,X,N,eps,B", SHAPES)
def test_apply_transition_with_injected_draws_matches_float64(T, X, N, eps, B, ladder):
    dyn, r64, r32 = _hip(T, X, N, eps, B, "stress")
    x, v0f, v0b, coin, u = (np.asarray(a, dtype=np.float32) for a in H.gauge_inputs(B, 2 * T * X, seed=211 + X))
    beta = np.linspace(1.0, 4.0, B).astype(np.float32) if ladder else 2.5
    got = dyn.apply_transition(_dev(x), _dev(beta) if ladder else beta, momentum_f=_dev(v0f), momentum_b=_dev(v0b),
                               coin=_dev(coin), u=_dev(u))
    names = ("x_prop", "v_prop", "p", "x_out")
    f64, f32 = (dict(zip(names, r.apply_transition(x, beta, v0f, v0b, coin, u))) for r in (r64, r32))
    got = dict(zip(names, map(_np, got)))
    # a chain whose p sits within rounding of its uniform may accept on one side and reject on the other
    clear = np.abs(f64["p"] - u) > 1e-4
    assert clear.mean() > 0.9 and 0 < (f64["p"] > u).mean() < 1
    for d in (got, f32, f64):
        d["x_out"] = d["x_out"][clear]
    ang = ("x_prop", "x_out")
    _gate(f"apply_transition {T}x{X} ladder={ladder}", got, f64, _yard(f32, f64, angular=ang), angular=ang)


def test_sampler_step_runs_the_periodic_plan_layer_by_layer():
    """GaugeSampler.step (l2hmc_gauge_mcmc_step) and the ladder step at 8x8, where the reference mode has a whole-step
    kernel: the periodic plan has none, takes the same draws as apply_transition, and keeps the state wrapped."""
    import ctypes as C
    from l2hmc_amd import GaugeSampler, _lib
    dyn, r64, _ = _hip(8, 8, 2, 0.1, 16, "mild", seed=11)
    assert _lib.lib().l2hmc_gauge_plan_fused(C.byref(dyn._plan())) == 0
    x = _dev(H.gauge_inputs(16, 128, seed=5)[0])
    sampler = GaugeSampler(dyn)
    x1, px, _, _ = sampler.step(x, 2.0)
    assert float(x1.min()) >= 0 and float(x1.max()) <= TWO_PI and bool(torch.isfinite(px).all())
    dyn2, _, _ = _hip(8, 8, 2, 0.1, 16, "mild", seed=11)
    _, _, p2, xo2 = dyn2(x, 2.0)
    assert torch.equal(px, p2) and torch.equal(x1, sampler.wrap(xo2))
    dyn3, _, _ = _hip(8, 8, 2, 0.1, 16, "mild", seed=11)
    x3, p3, _, _ = GaugeSampler(dyn3).step(x, torch.full((16,), 2.0, device="cuda"))
    assert torch.equal(p3, px) and torch.equal(x3, x1)


# ---- properties on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,X,B", [(4, 4, 64), (3, 5, 37)])
def test_periodic_trajectory_is_invertible_shift_equivariant_and_reversible_on_the_torus(T, X, B):
    D, N, eps, beta = 2 * T * X, 3, 0.2, 2.0
    rng = np.random.default_rng(31 + T)
    x = _dev(rng.uniform(0, TWO_PI, (B, D)))
    v = _dev(rng.standard_normal((B, D)))
    k = _dev(rng.integers(-3, 4, (B, D)))
    ang = lambda a, b: torch.remainder(a - b + np.pi, TWO_PI) - np.pi   # noqa: E731

    def measure(dyn):
        x1, v1, p1, s1 = dyn.transition_kernel(x, beta, forward=True, momentum=v, return_logdet=True)
        x2, v2, _ = dyn.transition_kernel(x1, beta, forward=False, momentum=v1)
        xs, vs, ps, ss = dyn.transition_kernel(x + TWO_PI * k, beta, forward=True, momentum=v, return_logdet=True)
        x3, v3, _ = dyn.transition_kernel(torch.remainder(x1, TWO_PI), beta, forward=False, momentum=v1)
        assert float(s1.abs().mean()) > 0.05, "a net that does nothing proves nothing"
        return dict(invert=float(ang(x2, x).abs().max()), invert_v=float((v2 - v).abs().max()),
                    shift=float(ang(xs, x1).abs().max()), shift_v=float((vs - v1).abs().max()),
                    shift_ld=float((ss - s1).abs().max()), shift_p=float((ps - p1).abs().max()),
                    wrap=float(ang(x3, x).abs().max()), wrap_v=float((v3 - v).abs().max()),
                    left=float((x1 < 0).float().mean() + (x1 >= TWO_PI).float().mean()))
    per = measure(_hip(T, X, N, eps, B, "stress")[0])
    print(f"[periodic] properties {T}x{X} periodic=True: {per}")
    assert per["left"] > 0.01                       # some links left [0, 2 pi): the wrap does something
    for name in ("invert", "invert_v", "shift", "shift_v", "shift_ld", "shift_p", "wrap", "wrap_v"):
        assert per[name] < 1e-3, (name, per)
    ref = measure(_hip(T, X, N, eps, B, "stress", periodic=False)[0])
    print(f"[periodic] properties {T}x{X} periodic=False: {ref}")
    assert ref["invert"] < 1e-3                     # the reference mode is invertible too ...
    assert ref["shift"] > 1e-2 and ref["wrap"] > 1e-2, ref      # ... but neither equivariant nor reversible (Q10)


# ---- training gradients --------------------------------------------------------------------------------------------
def _trainer(T, X, N, eps, B, regime, seed):
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    D = 2 * T * X
    dyn, _, _ = _hip(T, X, N, eps, B, regime)
    tr = GaugeTrainer(dyn, metric='cos_diff', lr_init=1e-3)
    xp, vp = PR.periodic_weights(T, X, regime=regime)
    tm = PR.TorchPeriodic(T, X, N, eps, PR.masks_for(N, D), xp, vp)
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, TWO_PI, (B, D))
    z = rng.standard_normal((B, D))
    dx = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    dz = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    return tr, tm, x, z, dx, dz


# seeds for which the float64 reference is flip-free (PR.TorchPeriodic.flip_free), found on the CPU
GRAD_CASES = [(3, 5, 2, 0.15, 37, "stress", 21),(4, 4, 3, 0.2, 6, "mild", 7), (6, 6, 2, 0.2, 9, "mild", 7)]


@pytest.mark.parametrize("T,X,N,eps,B,regime,seed", GRAD_CASES)
def test_periodic_training_gradients_match_autograd(T, X, N, eps, B, regime, seed):
    tr, tm, x, z, dx, dz = _trainer(T, X, N, eps, B, regime, seed)
    beta = 2.5
    loss, _, _, _ = tr.calc_loss_and_grads(x, beta, z=z, draws_x=dx, draws_z=dz)
    assert tr._walk is not None                  # the layered walk, whatever the widths (4x4 has tiled ones)
    want_loss, want_terms = _ref_grads(tm, x, z, dx, dz, beta, 'cos_diff')
    assert tm.flip_free(), (tm.min_preact, tm.min_clamp)
    np.testing.assert_allclose(tr.last_loss_terms.cpu().numpy(), want_terms, rtol=2e-4,
                               atol=1e-5 * max(1., np.abs(want_terms).max()))
    assert abs(float(loss) - want_loss) <= 2e-4 * max(1., abs(want_loss))
    print(f"[periodic] gradients {T}x{X}: {_compare(tr, tm)}")


def test_periodic_training_on_a_ladder_of_betas():
    T, X, N, eps, B, regime, seed = GRAD_CASES[0]
    tr, tm, x, z, dx, dz = _trainer(T, X, N, eps, B, regime, seed)
    betas = np.linspace(1.5, 3.5, B).astype(np.float32)
    loss, _, _, _ = tr.calc_loss_and_grads(x, betas, z=z, draws_x=dx, draws_z=dz)
    want_loss, want_terms = _ref_grads(tm, x, z, dx, dz, torch.tensor(betas, dtype=torch.float64), 'cos_diff')
    assert tm.flip_free(), (tm.min_preact, tm.min_clamp)
    np.testing.assert_allclose(tr.last_loss_terms.cpu().numpy(), want_terms, rtol=2e-4,
                               atol=1e-5 * max(1., np.abs(want_terms).max()))
    assert abs(float(loss) - want_loss) <= 2e-4 * max(1., abs(want_loss))
    print(f"[periodic] ladder gradients: {_compare(tr, tm)}")
    # a ladder of equal betas is the scalar step, bit for bit
    tr.calc_loss_and_grads(x, np.full(B, 2.5, dtype=np.float32), z=z, draws_x=dx, draws_z=dz)
    g_ladder, terms_ladder = tr.grads.clone(), tr.last_loss_terms.clone()
    tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    assert torch.equal(tr.grads, g_ladder) and torch.equal(tr.last_loss_terms, terms_ladder)


def test_autograd_is_refused_on_the_device():
    dyn, _, _ = _hip(3, 5, 2, 0.2, 4)
    x = torch.rand(4, 30, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="periodic=True"):
        dyn(x, 2.0)
