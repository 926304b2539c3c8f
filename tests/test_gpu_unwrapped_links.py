"""Links far outside [0, 2 pi): both sides of the switch of `fast_sincos` (csrc/common.h: the polynomial below
|x| = 8192, libm's sincosf from there on) in the kernels that compile it in (what is not reached is named at the end).
Negative links and links many windings
from 0 are legal input to every entry that takes x; before this file no test fed any kernel an argument outside
[-4 pi, 4 pi].  Inputs, float64 references and bars are tests/unwrapped_cases.py (links on a grid of 2^-10, so that every
plaquette is exact in float32 and the only error left is the sine's and the float32 operations'), proven on the CPU by
tests/test_nonfinite_host.py, which also shows that a sine that is wrong on either side of the switch alone misses the
bars used here by a factor of 100 or more.

a. the standalone entries with a free x: action, force, average plaquette and charge (l2hmc_u1_action_force), the
   force's Hessian-vector product (l2hmc_u1_force_hvp) and the energies and swap probabilities of a replica-exchange
   round (l2hmc_gauge_replica_swap, gauge_swap.h), at 8x8, 6x6 and 3x5, against float64 on the same float32 inputs, each
   output under a bar derived from 2e-7 per sine and its own float32 operations (tests/unwrapped_cases.py::bars).
b. the one-launch kernels, an N = 1 transition from a grid start with every draw injected: plain HMC (hmc_step.hip; one
   lattice per sites-per-thread class; 8x8 is also what `hmc=True` runs where the whole-step kernels live) and the
   torus-exact whole-step kernel (fused_traj_ncp.hip: fast_sincos of the links themselves and of the plaquettes).
   v_prop and p under `assert_fp32_equivalent` and the accept-probability rule of tests/test_gpu_parity.py, x_prop within
   half an ulp of max |x| plus what v' may be off by.  Both also run a whole step (GaugeSampler.step) from the same
   start, and the observables of its input are held to the bars of a.: for plain HMC the stencil of hmc_step.hip, for the
   torus-exact kernel `plaq_sums` of fused_step.h, the observables stage that every whole-step kernel shares.

c. the same observables stage as compiled into the reference mode's whole-step kernels (GenericNet in its sub-tile and
   16-row split forms, ConvNet3D): a whole step from the grid start, the observables of its input under the bars of a.
   (Their proposals are not compared here: behind a network at |x| = 4096 the float32 oracle is off by the rounding of x.)

Not reached by this file: the 32-row form's copy of the observables stage, and fused_train.hip's use of the switch.

Every test prints figure / bar."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import toy_cases as tc
from tests import unwrapped_cases as U

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device="cuda")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _hold(what, k, got, want, bar):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    err = err.reshape(err.shape[0], -1).max(axis=1)
    ratio = float(np.max(err / bar))
    print(f"[unwrapped] {what} {k}: error {err.max():.3e}, worst error / bar {ratio:.3f} (bar {np.max(bar):.3e})")
    assert ratio <= 1.0, (what, k, float(err.max()), float(np.max(bar)))


# ---- a. standalone entries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,X", U.LATTICES)
@pytest.mark.parametrize("cls", list(U.CLASSES))
def test_standalone_entries_on_unwrapped_links(cls, T, X):
    from l2hmc_amd import ops
    from l2hmc_amd.lattice import replica_swap
    x, u = U.links(T, X, cls), U.tangent(T, X)
    want, bar = U.reference(x, u, T, X), U.bars(x, u, T, X)
    what = f"{T}x{X} |x| <= {U.CLASSES[cls]:g}"
    action, force, plaq, charge = ops.u1_action_force(_dev(x), T, X, U.BETA)
    hvp = ops.u1_force_hvp(_dev(x), _dev(u), T, X, U.BETA)
    for k, g in (("action", action), ("force", force), ("avg_plaq", plaq), ("top_charge", charge), ("hvp", hvp)):
        _hold(what, k, _np(g), want[k], bar[k])
    # one exchange round in pairs (a, a + 1): the energies of gauge_swap.h and p = min(1, exp((beta_a - beta_b)(S_a - S_b)))
    B = x.shape[0]
    betas = np.where(np.arange(B) % 2 == 0, 2.0, 3.0).astype(np.float32)
    xs = _dev(x).clone()
    swap_p, swapped, act = replica_swap(xs, T, X, 2, 0, _dev(betas), 11, 5)
    _hold(what, "swap energy", _np(act), want["action"], bar["action"])
    a = np.arange(0, B, 2)
    dh = (betas[a].astype(np.float64) - betas[a + 1]) * (want["action"][a] - want["action"][a + 1])
    p64 = np.exp(np.minimum(dh, 0.0))
    # |d exp(min(dh, 0))| <= |d dh| <= |beta_a - beta_b| (two energies' bars); one rounding of p to float32
    _hold(what, "swap p", _np(swap_p)[a], p64, 2 * bar["action"] * 1.0 + 2 * U.E)
    perm = np.arange(B)
    sw = swapped.cpu().numpy()[a]
    perm[a[sw]], perm[a[sw] + 1] = a[sw] + 1, a[sw]
    assert np.array_equal(xs.cpu().numpy(), x[perm])                       # a round moves rows, bit for bit


# ---- b. one-launch kernels ------------------------------------------------------------------------------------------
def _transition_bars(what, got, w64, w32):
    fails, fig = tc.fp32_equivalent(got[1], w64[1], w32[1])
    print(f"[unwrapped] {what} v_prop: max {fig['max']:.3e} rms {fig['rms']:.3e} (fp32 oracle {fig['fp32_max']:.3e} / "
          f"{fig['fp32_rms']:.3e})")
    assert not fails, (what, fails)
    ep, bp = float(np.abs(got[2] - w64[2]).max()), tc.p_bar(w64[2], w32[2])
    print(f"[unwrapped] {what} p: {ep:.3e} / {bp:.3e}; p in [{w64[2].min():.3f}, {w64[2].max():.3f}]")
    assert ep < bp, (what, ep, bp)


@pytest.mark.parametrize("T,X", U.HMC_LATTICES)
@pytest.mark.parametrize("cls", list(U.CLASSES))
def test_plain_hmc_step_from_unwrapped_links(cls, T, X):
    from l2hmc_amd import GaugeSampler
    x, v0f, v0b, coin, u = U.hmc_inputs(T, X, cls)
    o64 = H.gauge_oracle(T, X, 1, U.HMC_EPS, None, None, hmc=True)
    o32 = H.gauge_oracle(T, X, 1, U.HMC_EPS, None, None, hmc=True, dtype=np.float32)
    dyn = H.gauge_hip(T, X, 1, U.HMC_EPS, None, None, o64.mask, x.shape[0], hmc=True)
    o64.eps = float(dyn.eps)                                               # the float32 rounding the device holds
    what = f"hmc {T}x{X} |x| <= {U.CLASSES[cls]:g}"
    got = [_np(t) for t in dyn.apply_transition(_dev(x), U.HMC_BETA, momentum_f=_dev(v0f), momentum_b=_dev(v0b),
                                                coin=_dev(coin), u=_dev(u))]
    w64 = o64.apply_transition(x.astype(np.float64), U.HMC_BETA, v0f.astype(np.float64), v0b.astype(np.float64), coin,
                               u.astype(np.float64))
    w32 = o32.apply_transition(x, U.HMC_BETA, v0f, v0b, coin, u)
    _transition_bars(what, got, w64, w32)
    bar_x = U.bar_x_prop(w64[0], np.concatenate([v0f, v0b]))
    ex = float(np.abs(got[0] - w64[0]).max())
    print(f"[unwrapped] {what} x_prop: {ex:.3e} = {ex / U.ulp(w64[0]):.3f} ulp(max |x|) / bar {bar_x / U.ulp(w64[0]):.3f} ulp")
    assert ex <= bar_x, (what, ex, bar_x)
    # the observables of the step's input (the step's own draws; what it measures does not depend on them)
    xn, px, obs, dq = GaugeSampler(dyn).step(_dev(x), U.HMC_BETA)
    zero = np.zeros_like(x)
    want, bar = U.reference(x, zero, T, X, U.HMC_BETA), U.bars(x, zero, T, X, U.HMC_BETA)
    for k in ("action", "avg_plaq", "top_charge"):
        _hold(what + " step", k, _np(obs[k]), want[k], bar[k])
    assert float(xn.min()) >= 0 and float(xn.max()) <= 2 * np.pi and bool(((px >= 0) & (px <= 1)).all())


@pytest.mark.parametrize("cls", list(U.CLASSES))
def test_torus_exact_whole_step_from_unwrapped_links(cls):
    """The network of this mode sees only cos x and sin x (fast_sincos of the links: the polynomial path up to 4096) and
    the force takes fast_sincos of the plaquettes (both paths).  Positions by angular distance, as in the mode's own tests."""
    from tests import periodic_ref as PR
    from tests.test_gpu_periodic import _hip
    from tests.test_gpu_periodic_step import _fused
    T = X = 8
    x, v0f, v0b, coin, u = U.hmc_inputs(T, X, cls)
    dyn, r64, r32 = _hip(T, X, 1, U.HMC_EPS, x.shape[0], "mild", both_directions=True, whole_step=True)
    assert _fused(dyn) == 1
    what = f"torus-exact whole step 8x8 |x| <= {U.CLASSES[cls]:g}"
    got = [_np(t) for t in dyn.apply_transition(_dev(x), U.HMC_BETA, momentum_f=_dev(v0f), momentum_b=_dev(v0b),
                                                coin=_dev(coin), u=_dev(u))]
    w64 = r64.apply_transition(x, U.HMC_BETA, v0f, v0b, coin, u)
    w32 = r32.apply_transition(x, U.HMC_BETA, v0f, v0b, coin, u)
    w64, w32 = [np.asarray(a, dtype=np.float64) for a in w64], [np.asarray(a, dtype=np.float64) for a in w32]
    _transition_bars(what, got, w64, w32)
    # x_prop by angle: tests/unwrapped_cases.py::bar_x_angle (no absolute floor)
    ex, e32 = float(PR.angdist(got[0], w64[0]).max()), float(PR.angdist(w32[0], w64[0]).max())
    ulp_x = max(U.ulp(x), U.ulp(got[0]))                                   # (the references may return another winding)
    bar_x = U.bar_x_angle(x, got[0], e32, tc.MAX_RATIO)
    print(f"[unwrapped] {what} x_prop: angular distance {ex:.3e} = {ex / ulp_x:.3f} ulp(max |x|) / bar {bar_x / ulp_x:.3f} ulp "
          f"(float32 reference {e32:.3e})")
    assert ex <= bar_x, (what, ex, bar_x)
    # the whole step: step_observables -> plaq_sums of fused_step.h (the second fast_sincos of every whole-step kernel and
    # the charge's projection) on the step's unwrapped INPUT; what it measures does not depend on the step's own draws
    from l2hmc_amd import GaugeSampler
    xn, px, obs, dq = GaugeSampler(dyn).step(_dev(x), U.HMC_BETA)
    zero = np.zeros_like(x)
    want, bar = U.reference(x, zero, T, X, U.HMC_BETA), U.bars(x, zero, T, X, U.HMC_BETA)
    for k in ("action", "avg_plaq", "top_charge"):
        _hold(what + " step", k, _np(obs[k]), want[k], bar[k])
    assert float(xn.min()) >= 0 and float(xn.max()) <= 2 * np.pi and bool(((px >= 0) & (px <= 1)).all())
    assert bool(torch.isfinite(dq).all())


# ---- c. the observables stage of the reference mode's whole-step kernels ---------------------------------------------
@pytest.mark.parametrize("form", ["sub-tile", "split-16", "conv3d"])
@pytest.mark.parametrize("cls", list(U.CLASSES))
def test_whole_step_observables_on_unwrapped_links(cls, form):
    import ctypes as C
    from l2hmc_amd import GaugeSampler, _lib
    T = X = 8
    x = U.hmc_inputs(T, X, cls)[0]
    conv = form == "conv3d"
    xp, vp = (H.conv_weights if conv else H.gauge_weights)(T, X, regime="mild")
    orc = H.gauge_oracle(T, X, 1, U.HMC_EPS, xp, vp, arch="conv3D" if conv else "generic")
    dyn = H.gauge_hip(T, X, 1, U.HMC_EPS, xp, vp, orc.mask, x.shape[0], arch="conv3D" if conv else "generic")
    dyn.tiles16_only = form == "split-16"
    plan = dyn._plan()
    assert _lib.lib().l2hmc_gauge_plan_fused(C.byref(plan)) == 1
    assert bool(plan.flags & _lib.PLAN_CONV3D) == conv and bool(plan.flags & _lib.PLAN_TILES16_ONLY) == (form == "split-16")
    xn, px, obs, dq = GaugeSampler(dyn).step(_dev(x), U.HMC_BETA)
    zero = np.zeros_like(x)
    want, bar = U.reference(x, zero, T, X, U.HMC_BETA), U.bars(x, zero, T, X, U.HMC_BETA)
    what = f"whole step ({form}) 8x8 |x| <= {U.CLASSES[cls]:g}"
    for k in ("action", "avg_plaq", "top_charge"):
        _hold(what, k, _np(obs[k]), want[k], bar[k])
    # (nothing is asked of x_next: generic_net.py puts no tanh on the transformation head, so behind |x| = 4096 the
    # proposal may overflow, which the accept probability answers with 0)
    assert bool(((px >= 0) & (px <= 1)).all())
