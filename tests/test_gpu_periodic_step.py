"""The torus-exact mode's whole-step kernel (`GaugeDynamics(periodic=True, whole_step=True)`,
L2HMC_PLAN_PERIODIC | L2HMC_PLAN_PERIODIC_STEP; l2hmc_amd/csrc/fused_traj_ncp.hip) on the device.

Only D = 128 has the kernel: every case is 8x8 (one 4x16 case for the non-square index arithmetic of the force pass),
N = 3 leapfrog steps (two step boundaries for the kept VNet product; the backward mask and time index N - 1 - step
differ from the forward ones), batches of 5 (one partial workgroup), 8 and 19 (three paired workgroups, the last
partial; two in selected-only, the second partial).

Parity against the float64 reference of tests/periodic_ref.py is gated as tests/test_gpu_periodic.py gates it, with
one more yardstick: per output, the LARGER of the float32 NumPy reference's error against float64 and the error of the
layered device path (whole_step=False: same weights, masks and inputs) against float64; the gate is GATE = 4 of those
(the kernel's fast_sincos force and its summation orders differ from both).  Every case prints error / yardstick.

Observables and sums of the one-launch step (test 5): compared with l2hmc_u1_action_force on the step's own x_in /
x_out under the tolerances of tests/test_gpu_parity.py::test_native_mcmc_step_matches_oracle_on_its_own_draws (1e-5
action and plaquette, 1e-4 charge, 1e-3 |dQ|) and of tests/test_gpu_step_active_heads.py (4 float32 eps on the sums).
The tolerance rule is the one in force, not bit equality: the kernel's chain sums run over 16 lanes with fast_sincos,
and on the MI355X none of the four was bit-equal (errors 1.1e-7, 1.5e-8, 8.9e-8, 1.3e-7); the test prints both.

Without the feature `whole_step=True` was silently set as an attribute: test_the_flag_selects_the_kernel fails on the
parent commit (l2hmc_gauge_plan_fused == 0).

Measured on the MI355X, worst error / yardstick (gate 4): transition_kernel 1.80 (8x8, 19 rows, mild, backward, p:
2.2e-5 against 1.2e-5; 4x16 at most 1.58), apply_transition 1.80 (p, both layouts), the whole step 1.01 (x_out).  The
yardsticks lie between 5.4e-8 and 1.8e-5.  Round trips 2.4e-6 rad (v, log-det, p within 6.5e-6); invariance max |z|
1.91 (accept 0.395, mean |sumlogdet| 0.515).  The file runs in about 6 s.  More in profiles/periodic_step.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import invariance as I
from tests import periodic_ref as PR
from tests.test_gpu_periodic import _dev, _gate, _hip, _np, _yard

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi
N, EPS = 3, 0.15


def _pair(T, X, B, regime, **kw):
    """(whole-step dynamics, layered dynamics, float64 reference, float32 reference): same weights, masks, seed."""
    ws, r64, r32 = _hip(T, X, N, EPS, B, regime, whole_step=True, **kw)
    lay, _, _ = _hip(T, X, N, EPS, B, regime, **kw)
    return ws, lay, r64, r32


def _yard2(f32, lay, f64, angular=()):
    """Per output, the larger of the float32 reference's and the layered device path's error against float64."""
    a, b = _yard(f32, f64, angular), _yard(lay, f64, angular)
    return {k: max(a[k], b[k]) for k in f64}


def _fused(dyn):
    from l2hmc_amd import _lib
    return _lib.lib().l2hmc_gauge_plan_fused(C.byref(dyn._plan()))


# ---- 1. the flag does something ------------------------------------------------------------------------------------
def test_the_flag_selects_the_kernel():
    from l2hmc_amd import GaugeSampler
    ws, lay, _, _ = _pair(8, 8, 8, "mild")
    assert _fused(ws) == 1
    assert _fused(lay) == 0                           # opt-in: the default periodic plan runs layer by layer
    ws.fused = False
    assert _fused(ws) == 0                            # L2HMC_PLAN_LAYERED wins
    ws.fused = True
    assert _fused(_hip(4, 16, N, EPS, 5, "mild", whole_step=True)[0]) == 1
    dyn6, _, _ = _hip(6, 6, N, EPS, 8, "mild", whole_step=True)
    assert dyn6.whole_step is True and _fused(dyn6) == 0
    x = _dev(H.gauge_inputs(8, 72, seed=5)[0])
    x1, px, _, _ = GaugeSampler(dyn6).step(x, 2.0)    # the flag is carried; the step runs layer by layer
    assert float(x1.min()) >= 0 and float(x1.max()) <= TWO_PI and bool(torch.isfinite(px).all())


# ---- 2. trajectory parity against float64 --------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["mild", "stress"])
@pytest.mark.parametrize("T,X,B", [(8, 8, 5), (8, 8, 19), (4, 16, 5)])
def test_transition_kernel_matches_float64(T, X, B, regime):
    ws, lay, r64, r32 = _pair(T, X, B, regime)
    assert _fused(ws) == 1
    x, v0f, v0b, _, _ = (np.asarray(a, dtype=np.float32) for a in H.gauge_inputs(B, 2 * T * X, seed=211))
    beta = 2.5
    names = ("x", "v", "p", "sumlogdet")
    for bwd, v0 in ((False, v0f), (True, v0b)):
        run = lambda d: dict(zip(names, map(_np, d.transition_kernel(   # noqa: E731
            _dev(x), beta, forward=not bwd, momentum=_dev(v0), return_logdet=True))))
        got, layered = run(ws), run(lay)
        f64, f32 = (dict(zip(names, r.trajectory(x, v0, beta, bwd))) for r in (r64, r32))
        assert np.abs(f64["sumlogdet"]).mean() > 1e-3
        _gate(f"whole-step transition_kernel {T}x{X} B={B} {regime} bwd={bwd}", got, f64,
              _yard2(f32, layered, f64, angular=("x",)), angular=("x",))


# ---- 3. apply_transition with injected draws -----------------------------------------------------------------------
@pytest.mark.parametrize("both", [True, False])
def test_apply_transition_with_injected_draws_matches_float64(both):
    T = X = 8
    B = 19
    ws, lay, r64, r32 = _pair(T, X, B, "mild", both_directions=both)
    x, v0f, v0b, coin, u = (np.asarray(a, dtype=np.float32) for a in H.gauge_inputs(B, 2 * T * X, seed=211))
    beta = 2.5
    names = ("x_prop", "v_prop", "p", "x_out")
    run = lambda d: dict(zip(names, map(_np, d.apply_transition(   # noqa: E731
        _dev(x), beta, momentum_f=_dev(v0f), momentum_b=_dev(v0b), coin=_dev(coin), u=_dev(u)))))
    got, layered = run(ws), run(lay)
    f64, f32 = (dict(zip(names, r.apply_transition(x, beta, v0f, v0b, coin, u))) for r in (r64, r32))
    # a chain whose p sits within rounding of its uniform may accept on one side and reject on the other
    clear = np.abs(f64["p"] - u) > 1e-4
    assert clear.mean() > 0.9 and 0 < (f64["p"] > u).mean() < 1
    for d in (got, layered, f32, f64):
        d["x_out"] = d["x_out"][clear]
    ang = ("x_prop", "x_out")
    _gate(f"whole-step apply_transition both={both}", got, f64, _yard2(f32, layered, f64, angular=ang), angular=ang)


# ---- 4. - 7. the whole step ----------------------------------------------------------------------------------------
B19 = 19
DRAWS = 40                                             # the dynamics' draw counter: the step takes the pair (40, 41)


def _x19():
    return _dev(H.gauge_inputs(B19, 128, seed=211)[0])


def _step(dyn, x, beta):
    """One GaugeSampler.step from draw counter DRAWS -> dict of x_next, px, the observables, dq and the step sums."""
    from l2hmc_amd import GaugeSampler
    dyn._draws = DRAWS
    smp = GaugeSampler(dyn)
    ring, slot = smp._sums_ring, smp._sums_next
    xn, px, obs, dq = smp.step(x, beta)
    torch.cuda.synchronize()
    return dict(x_next=xn, px=px, action=obs["action"], avg_plaq=obs["avg_plaq"], top_charge=obs["top_charge"], dq=dq,
                sums=ring[slot].clone())


def _equal(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


def test_whole_step_takes_the_layered_steps_draws():
    from l2hmc_amd import ops
    ws, lay, r64, r32 = _pair(8, 8, B19, "mild", seed=11)
    x, beta = _x19(), 2.0
    got, layered = _step(ws, x, beta), _step(lay, x, beta)
    # the step's draws, reproduced: streams 2 draw (momenta of both directions) and 2 draw + 1 (coin | u)
    draw = DRAWS // 2
    V = _np(ops.fill_normal((2 * B19, 128), ws._seed, 2 * draw, x.device))
    cu = _np(ops.fill_uniform((2 * B19,), ws._seed, 2 * draw + 1, x.device))
    x32 = x.cpu().numpy()
    names = ("x_prop", "v_prop", "p", "x_out")
    f64, f32 = (dict(zip(names, r.apply_transition(x32, beta, V[:B19], V[B19:], cu[:B19], cu[B19:]))) for r in (r64, r32))
    # (a chain whose p sits within rounding of its uniform may accept on one side and reject on the other)
    clear = np.abs(f64["p"] - cu[B19:]) > 1e-4
    assert clear.mean() > 0.5
    acc_ws = _np(got["px"]) > cu[B19:]
    acc_lay = _np(layered["px"]) > cu[B19:]
    assert np.array_equal(acc_ws[clear], acc_lay[clear]) and np.array_equal(acc_ws[clear], (f64["p"] > cu[B19:])[clear])
    # px and, on the clear chains, the new state (by angular distance: it is wrapped) within the gate of the
    # trajectory tests above
    pick = lambda p, xo: dict(p=p, x_out=xo[clear])   # noqa: E731
    want = pick(f64["p"], f64["x_out"])
    _gate("whole step", pick(_np(got["px"]), _np(got["x_next"])), want,
          _yard2(pick(f32["p"], f32["x_out"]), pick(_np(layered["px"]), _np(layered["x_next"])), want,
                 angular=("x_out",)), angular=("x_out",))
    xn = _np(got["x_next"])
    assert xn.min() >= 0 and xn.max() <= TWO_PI
    # dyn(x, beta) under no_grad takes the same kernel and the same draws: bit for bit
    from l2hmc_amd import GaugeSampler
    ws2, _, _ = _hip(8, 8, N, EPS, B19, "mild", whole_step=True, seed=11)
    ws2._draws = DRAWS
    with torch.no_grad():
        _, _, p2, xo2 = ws2(x, beta)
    assert torch.equal(p2, got["px"]) and torch.equal(GaugeSampler(ws2).wrap(xo2), got["x_next"])


def test_step_observables_and_sums():
    """actions, plaqs, charges, |dQ| and the sums of the one-launch step against the standalone operators on the
    step's own x_in / x_out (tolerances: module docstring)."""
    from l2hmc_amd.lattice import u1_observables
    ws = _hip(8, 8, N, EPS, B19, "mild", whole_step=True, seed=11)[0]
    x, beta = _x19(), 2.0
    got = _step(ws, x, beta)
    ws._draws = DRAWS
    with torch.no_grad():
        _, _, _, x_out = ws(x, beta)                   # the step's own x_out, unwrapped (same kernel, same draws)
    obs_in, obs_out = u1_observables(x, 8, 8), u1_observables(x_out, 8, 8)      # l2hmc_u1_action_force
    want = dict(action=obs_in["action"], avg_plaq=obs_in["avg_plaq"], top_charge=obs_in["top_charge"],
                dq=(obs_in["top_charge"] - obs_out["top_charge"]).abs())
    tol = dict(action=1e-5, avg_plaq=1e-5, top_charge=1e-4, dq=1e-3)
    for k, w in want.items():
        err = H.relerr(_np(got[k]), _np(w))
        print(f"[periodic step] {k}: bit-equal {torch.equal(got[k], w)} error {err:.3e} (tolerance {tol[k]:.0e})")
        assert err < tol[k], (k, err)
    sums = _np(got["sums"])
    f32eps = np.finfo(np.float32).eps
    for i, k in enumerate(("px", "dq")):
        s64 = float(got[k].double().sum())
        print(f"[periodic step] sum {k}: {sums[i]!r} float64 sum of the step's own outputs {s64!r}")
        assert abs(sums[i] - s64) <= 4 * f32eps * max(1., abs(s64))
    assert sums[2] == B19 and sums[3] == 0             # the chain count, and the ticket left at 0


def test_ladder_step_equals_the_uniform_step_column_by_column():
    x = _x19()
    rungs = (1.0, 2.5, 4.0)
    betas = torch.tensor([rungs[c % 3] for c in range(B19)], dtype=torch.float32, device="cuda")
    for both in (True, False):
        mk = lambda: _hip(8, 8, N, EPS, B19, "mild", whole_step=True, seed=11, both_directions=both)[0]   # noqa: E731
        ladder = _step(mk(), x, betas)
        for b in rungs:
            uni = _step(mk(), x, b)
            cols = (betas == b).cpu()
            for k in ("x_next", "px", "action", "avg_plaq", "top_charge", "dq"):
                assert torch.equal(ladder[k].cpu()[cols], uni[k].cpu()[cols]), (both, b, k)
        flat = _step(mk(), x, torch.full((B19,), 2.5, device="cuda"))
        _equal(flat, _step(mk(), x, 2.5), f"a ladder of equal values, both={both}")


def test_kept_first_layer_products_are_bit_neutral():
    x = _x19()
    v = _dev(H.gauge_inputs(B19, 128, seed=211)[1])
    for both in (True, False):
        outs = []
        for rec in (False, True):
            dyn = _hip(8, 8, N, EPS, B19, "mild", whole_step=True, seed=11, both_directions=both, recompute=rec)[0]
            assert _fused(dyn) == 1
            step = _step(dyn, x, 2.0)
            traj = {f"{d}{i}": t for d in (True, False)
                    for i, t in enumerate(dyn.transition_kernel(x, 2.5, forward=d, momentum=v, return_logdet=True))}
            outs.append({**step, **traj})
        _equal(outs[0], outs[1], f"recompute, both={both}")


def test_leapfrog_steps_compose_to_the_trajectory():
    """l2hmc_gauge_leapfrog_steps through the kernel (step_begin .. step_end, the log-det accumulated): all steps in
    one call give the trajectory's bits; step by step -- no kept VNet product across the launches, which is
    bit-neutral -- x and v keep them, and the log-det is the same terms summed in another grouping."""
    x = _x19()
    v = _dev(H.gauge_inputs(B19, 128, seed=211)[2])
    dyn = _hip(8, 8, N, EPS, B19, "stress", whole_step=True)[0]
    for bwd in (False, True):
        xt, vt, _, st = dyn.transition_kernel(x, 2.5, forward=not bwd, momentum=v, return_logdet=True)
        x1, v1, s1 = dyn._lf(x, v, 2.5, 0, bwd, step_end=N)
        assert torch.equal(x1, xt) and torch.equal(v1, vt) and torch.equal(s1, st)
        xs, vs, ss = x, v, torch.zeros_like(st)
        for step in range(N):
            xs, vs, ld = dyn._lf(xs, vs, 2.5, step, bwd)
            ss = ss + ld
        assert torch.equal(xs, xt) and torch.equal(vs, vt)
        # (the same float32 terms in N partial sums instead of one: a regrouping moves the result by a few float32
        #  eps, 6e-8, of the partial sums' magnitudes; 1e-5 of the largest log-det leaves two orders of room)
        assert float((ss - st).abs().max()) <= 1e-5 * max(1., float(st.abs().max()))


# ---- 8. torus properties through the new kernel --------------------------------------------------------------------
def test_whole_step_trajectory_is_invertible_shift_equivariant_and_reversible_on_the_torus():
    D, beta, B = 128, 2.0, B19
    rng = np.random.default_rng(31)
    x = _dev(rng.uniform(0, TWO_PI, (B, D)))
    v = _dev(rng.standard_normal((B, D)))
    k = _dev(rng.integers(-3, 4, (B, D)))
    ang = lambda a, b: torch.remainder(a - b + np.pi, TWO_PI) - np.pi   # noqa: E731
    dyn = _hip(8, 8, N, EPS, B, "stress", whole_step=True)[0]
    assert _fused(dyn) == 1
    x1, v1, p1, s1 = dyn.transition_kernel(x, beta, forward=True, momentum=v, return_logdet=True)
    x2, v2, _ = dyn.transition_kernel(x1, beta, forward=False, momentum=v1)
    xs, vs, ps, ss = dyn.transition_kernel(x + TWO_PI * k, beta, forward=True, momentum=v, return_logdet=True)
    x3, v3, _ = dyn.transition_kernel(torch.remainder(x1, TWO_PI), beta, forward=False, momentum=v1)
    assert float(s1.abs().mean()) > 0.05, "a net that does nothing proves nothing"
    per = dict(invert=float(ang(x2, x).abs().max()), invert_v=float((v2 - v).abs().max()),
               shift=float(ang(xs, x1).abs().max()), shift_v=float((vs - v1).abs().max()),
               shift_ld=float((ss - s1).abs().max()), shift_p=float((ps - p1).abs().max()),
               wrap=float(ang(x3, x).abs().max()), wrap_v=float((v3 - v).abs().max()),
               left=float((x1 < 0).float().mean() + (x1 >= TWO_PI).float().mean()))
    print(f"[periodic step] properties 8x8: {per}")
    assert per["left"] > 0.01                       # some links left [0, 2 pi): the wrap does something
    for name in ("invert", "invert_v", "shift", "shift_v", "shift_ld", "shift_p", "wrap", "wrap_v"):
        assert per[name] < 1e-3, (name, per)


# ---- 9. invariance --------------------------------------------------------------------------------------------------
def test_whole_step_leaves_the_finite_volume_distribution_invariant():
    from l2hmc_amd import GaugeLattice, GaugeDynamics, GaugeSampler
    from tests.test_gpu_invariance import CHECKPOINTS, Z_PASS, _action64, _report
    T, X, beta, B, eps = 8, 8, 2.0, 1 << 13, 0.15
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=eps, num_steps=N, eps_trainable=False,
                        network_arch='generic', periodic=True, whole_step=True, seed=5)
    dyn.set_masks(PR.masks_for(N, 2 * T * X, seed=3))
    xp, vp = PR.periodic_weights(T, X, regime="mild")
    dyn.position_fn.load_state(xp)
    dyn.momentum_fn.load_state(vp)
    assert _fused(dyn) == 1
    sampler = GaugeSampler(dyn)
    x = torch.as_tensor(I.u1_samples(B, T, X, beta, np.random.default_rng(17)), dtype=torch.float32, device="cuda")
    want = I.u1_exact_vector(T, X, beta)
    ld = 0.5 * sum(float(dyn.transition_kernel(x, beta, forward=f, return_logdet=True)[3].abs().mean())
                   for f in (True, False))
    zs, acc = [], None
    for k in range(1, max(CHECKPOINTS) + 1):
        x, px, _, _ = sampler.step(x, beta)
        if acc is None:
            acc = float(px.double().mean())
        if k in CHECKPOINTS:
            a, p, q = _action64(x, T, X)
            zs.append(I.zscores(I.u1_features(p.cpu().numpy(), a.cpu().numpy(), q.cpu().numpy()), want))
    assert float(x.min()) >= 0 and float(x.max()) <= TWO_PI
    m = _report("U(1) periodic L2HMC 8x8 whole step", np.array(zs), f"accept {acc:.3f} |logdet| {ld:.3f}")
    assert acc > 0.2 and ld > 0.05, (acc, ld)          # the chain does something
    assert m < Z_PASS, zs


# ---- 10. graph capture ----------------------------------------------------------------------------------------------
def test_whole_step_is_hip_graph_capturable():
    """One kernel node and no memset: captured once, replayed twice, every output of the second replay equal to the
    eager step with the same draw."""
    from l2hmc_amd import _lib
    B = B19
    dyn = _hip(8, 8, N, EPS, B, "mild", whole_step=True)[0]
    plan, L = dyn._plan(), _lib.lib()
    assert L.l2hmc_gauge_plan_fused(C.byref(plan)) == 1
    nb = L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    x0 = _x19()

    def bufs():
        return [torch.zeros(B, 128, device="cuda")] + [torch.zeros(B, device="cuda") for _ in range(5)] + \
               [torch.zeros(4, device="cuda")]

    def step(o):
        _lib.check(L.l2hmc_gauge_mcmc_step_ex(C.byref(plan), 2.0, x0.data_ptr(), o[0].data_ptr(), B, 42, 7,
                                              *(t.data_ptr() for t in o[1:6]), o[6].data_ptr(), ws.data_ptr(), nb,
                                              _lib.stream_ptr()))
    eager = bufs()
    step(eager)                                   # also the warm-up (one-time function attributes are set here)
    torch.cuda.synchronize()
    out = bufs()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(out)
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(2):
        for t in out[:6]:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(out, eager)):
            assert torch.equal(a, b), (rep, i)
    assert float(eager[6][2]) == B and float(eager[6][3]) == 0


# ---- 11. training ignores the flag ----------------------------------------------------------------------------------
def test_training_ignores_the_flag():
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    T = X = 8
    B, D = 8, 128
    rng = np.random.default_rng(7)
    x = rng.uniform(0, TWO_PI, (B, D))
    z = rng.standard_normal((B, D))
    dx = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    dz = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    res = []
    for flag in (True, False):
        dyn = _hip(T, X, 2, EPS, B, "mild", whole_step=flag)[0]
        tr = GaugeTrainer(dyn, metric='cos_diff', lr_init=1e-3)
        loss, _, px, _ = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
        assert tr._walk is not None                   # the layered walk
        res.append((loss.clone(), px.clone(), tr.grads.clone()))
    assert float(res[0][2].abs().max()) > 0
    for a, b in zip(*res):
        assert torch.equal(a, b)
