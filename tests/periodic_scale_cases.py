"""Case table of tests/test_gpu_periodic_scale.py and tests/test_gpu_periodic_train_scale.py: the torus-exact mode's
one-launch kernels (l2hmc_amd/csrc/fused_traj_ncp.hip) at the benchmark's trajectory length (N = 10) and at batches that
fill the chip more than once.  Importable without a GPU; tests/test_periodic_scale_host.py proves the conditions below
on the float64 / float32 references of tests/periodic_ref.py alone.

Sizes follow the device: a workgroup of the kernel holds 16 rows (8 chains in both directions, or 16 selected-only
chains) and its LDS use allows one workgroup per compute unit, so with CUS compute units
    8 CUS + 1 paired chains, 16 CUS + 1 selected-only chains and 16 CUS + 2 trajectory rows
are CUS + 1 workgroups: one full round of the chip and a last workgroup of one chain (two rows).  The host test uses
CUS = 256 (the MI355X).

Starts are thermal (`tests.invariance.u1_samples` at the case's beta): from the uniform start of the N = 3 tests a
trajectory of ten steps accepts nothing (mean p 0.004), and a comparison of p = 0 with p = 0 gates nothing.  eps was
picked on the CPU until, for every case that gates p or x_out, the float64 reference has
    at least 90 % of the chains with |p - u| > 1e-4,   an accepted fraction in (0.1, 0.9),   mean |sumlogdet| > 1e-3
and, at N = 10, every yardstick (float32 reference against float64) is finite and at most 2.5e-5."""
from collections import namedtuple

import numpy as np

from tests import invariance as I
from tests import periodic_ref as PR

HOST_CUS = 256
GATE = 4.0
YARD_CAP = 2.5e-5                  # N = 10: with GATE = 4 no gate is looser than the 1e-4 of the trajectory tests
CLEAR = 1e-4                       # |p - u| of a chain whose accept / reject decision rounding cannot move
BITES = 10.0                       # a perturbed reference misses its gate by at least this factor
WG_ROWS = 16                       # rows of one workgroup of gauge_traj_ncp_kernel

# name, lattice, leapfrog steps, eps, beta, weights, chains = per_cu * CUS + extra, both directions, input seed,
# gates_p: p and x_out are gated (False: "stress" at N = 10, where p is 0 to forty digits: x, v, sumlogdet only)
Case = namedtuple("Case", "name T X N eps beta regime per_cu extra both seed gates_p")

N10_CASES = [
    Case("n10-8x8-mild-paired", 8, 8, 10, 0.04, 2.5, "mild", 0, 19, True, 301, True),
    Case("n10-8x8-mild-selected", 8, 8, 10, 0.04, 2.5, "mild", 0, 19, False, 302, True),
    Case("n10-4x16-mild-paired", 4, 16, 10, 0.04, 2.5, "mild", 0, 19, True, 303, True),
    Case("n10-8x8-stress-paired", 8, 8, 10, 0.1, 2.5, "stress", 0, 19, True, 304, False),
]
BIG_CASES = [
    Case("big-paired", 8, 8, 3, 0.15, 2.5, "mild", 8, 1, True, 311, True),
    Case("big-selected", 8, 8, 3, 0.15, 2.5, "mild", 16, 1, False, 312, True),
]
# the whole step (GaugeSampler.step): draws of the dynamics' own Philox streams (seed STEP_SEED, draw counter STEP_DRAWS)
STEP_SEED, STEP_DRAWS, STEP_BETA = 11, 40, 2.5
STEP_CASES = [
    Case("step-n10", 8, 8, 10, 0.04, STEP_BETA, "mild", 0, 19, True, 324, True),
    Case("step-big-paired", 8, 8, 3, 0.15, STEP_BETA, "mild", 8, 1, True, 322, True),
    Case("step-big-selected", 8, 8, 3, 0.15, STEP_BETA, "mild", 16, 1, False, 323, True),
]
BY_NAME = {c.name: c for c in N10_CASES + BIG_CASES + STEP_CASES}
TRAJ_ROWS_PER_CU, TRAJ_ROWS_EXTRA = 16, 2            # the big trajectory entry: 16 CUS + 2 rows


def chains(case, cus=HOST_CUS):
    return case.per_cu * cus + case.extra


def workgroups(case, cus=HOST_CUS):
    per = WG_ROWS // 2 if case.both else WG_ROWS
    return -(-chains(case, cus) // per)


def start(case, B):
    """[B, D] float32 thermal start of the case."""
    return I.u1_samples(B, case.T, case.X, case.beta, np.random.default_rng(case.seed)).astype(np.float32)


def inputs(case, cus=HOST_CUS):
    """(x, v0_f, v0_b, coin, u) in float32: a thermal start and injected draws."""
    B, D = chains(case, cus), 2 * case.T * case.X
    rng = np.random.default_rng(case.seed + 5000)
    v0f, v0b = rng.standard_normal((B, D)), rng.standard_normal((B, D))
    coin, u = rng.uniform(size=B), rng.uniform(size=B)
    return (start(case, B), *(np.asarray(a, dtype=np.float32) for a in (v0f, v0b, coin, u)))


def step_draws_host(case, cus=HOST_CUS):
    """The draws the whole step takes, restated on the host (tests/philox_ref.py; the normals in float64 from the
    device's float32 uniforms).  The GPU test takes them from ops.fill_normal / fill_uniform."""
    from tests import philox_ref
    B = chains(case, cus)
    return philox_ref.lattice_step(STEP_SEED, STEP_DRAWS // 2, B, 2 * case.T * case.X)


def refs(case, cls=PR.NumpyPeriodic, **kw):
    """(float64 reference, float32 reference) on the float32 roundings of the weights and of eps, as the device holds
    them (tests/test_gpu_periodic.py::_hip builds the same pair)."""
    D = 2 * case.T * case.X
    masks = PR.masks_for(case.N, D)
    xp, vp = PR.periodic_weights(case.T, case.X, regime=case.regime)
    xp = {k: np.asarray(v, dtype=np.float32) for k, v in xp.items()}
    vp = {k: np.asarray(v, dtype=np.float32) for k, v in vp.items()}
    eps = float(np.float32(case.eps))
    return (cls(case.T, case.X, case.N, eps, masks, xp, vp, np.float64, **kw),
            cls(case.T, case.X, case.N, eps, masks, xp, vp, np.float32, **kw))


TRAJ_NAMES = ("x", "v", "p", "sumlogdet")
APPLY_NAMES = ("x_prop", "v_prop", "p", "x_out")


def traj(ref, x, v0, beta, bwd):
    return dict(zip(TRAJ_NAMES, ref.trajectory(x, v0, beta, bwd)))


def apply(ref, x, beta, v0f, v0b, coin, u, both=True):
    """apply_transition as a dict.  A selected-only dynamics runs each chain in its coin's direction alone: the same
    outputs (the reference mixes by the coin)."""
    return dict(zip(APPLY_NAMES, ref.apply_transition(x, beta, v0f, v0b, coin, u)))


def mix(tf, tb, x, coin, u):
    """apply_transition from the two trajectories' outputs (NumpyPeriodic.apply_transition on finite values: its 0 / 1
    weights select exactly)."""
    fwd = np.asarray(coin) > 0.5
    xp = np.where(fwd[:, None], tf["x"], tb["x"])
    vp = np.where(fwd[:, None], tf["v"], tb["v"])
    p = np.where(fwd, tf["p"], tb["p"])
    acc = p > np.asarray(u).astype(p.dtype)
    return dict(x_prop=xp, v_prop=vp, p=p, x_out=np.where(acc[:, None], xp, np.asarray(x).astype(xp.dtype)),
                sumlogdet=np.where(fwd, tf["sumlogdet"], tb["sumlogdet"]))


def apply_selected(ref, x, beta, v0f, v0b, coin, u):
    """apply_transition with every chain run in its coin's direction alone (half the work at the big batches; the
    outputs of a transition depend on nothing else) -> the dict of `mix`."""
    fwd = np.asarray(coin) > 0.5
    x = np.asarray(x)
    beta = np.asarray(beta)
    sel = lambda a, rows: a[rows] if a.ndim else a          # noqa: E731
    out = {k: None for k in TRAJ_NAMES}
    parts = [(rows, traj(ref, x[rows], (v0b if bwd else v0f)[rows], sel(beta, rows), bwd))
             for bwd, rows in ((False, fwd), (True, ~fwd)) if rows.any()]
    for k in TRAJ_NAMES:
        first = parts[0][1][k]
        full = np.empty((x.shape[0],) + first.shape[1:], dtype=first.dtype)
        for rows, t in parts:
            full[rows] = t[k]
        out[k] = full
    acc = out["p"] > np.asarray(u).astype(out["p"].dtype)
    return dict(x_prop=out["x"], v_prop=out["v"], p=out["p"],
                x_out=np.where(acc[:, None], out["x"], x.astype(out["x"].dtype)), sumlogdet=out["sumlogdet"])


def clear_chains(p64, u):
    return np.abs(np.asarray(p64, dtype=np.float64) - np.asarray(u, dtype=np.float64)) > CLEAR


def conditions(f64, u, sumlogdet):
    """(clear fraction, accepted fraction, mean |sumlogdet|) of a float64 apply_transition."""
    return (float(clear_chains(f64["p"], u).mean()), float((f64["p"] > u).mean()), float(np.abs(sumlogdet).mean()))


def conditions_hold(cond):
    clear, acc, sld = cond
    return clear >= 0.9 and 0.1 < acc < 0.9 and sld > 1e-3


# ---- perturbed references -------------------------------------------------------------------------------------------
class Perturbed(PR.NumpyPeriodic):
    """The reference with one index wrong: `mask` takes the mask row of step s at s % 3, `time` gives backward rows the
    time feature of `step` instead of N - 1 - step.  What the N = 3 tests cannot tell from the right code."""

    def __init__(self, *a, fault=None):
        super().__init__(*a)
        assert fault in ("mask", "time")
        self.fault = fault

    def leapfrog(self, x, v, beta, step, bwd):
        i = self.N - step - 1 if bwd else step
        t = self._time(step if self.fault == "time" else i, x.shape[0])
        m = self.mask[i % 3 if self.fault == "mask" else i]
        mi = 1 - m
        v, l1 = self.upd_v(x, v, beta, t, bwd)
        x, l2 = self.upd_x(x, v, t, mi if bwd else m, bwd)
        x, l3 = self.upd_x(x, v, t, m if bwd else mi, bwd)
        v, l4 = self.upd_v(x, v, beta, t, bwd)
        return x, v, l1 + l2 + l3 + l4


def neighbour_swap(out, axis_len):
    """The outputs with the last chain replaced by its neighbour (the references are chain-local: this is what a
    workgroup that read the wrong row base for its one chain would return)."""
    res = {}
    for k, a in out.items():
        a = np.array(a, copy=True)
        if a.shape[0] == axis_len:
            a[-1] = a[-2]
        res[k] = a
    return res


def err(got, want, angular=False):
    """tests/test_gpu_periodic.py::_err."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if angular:
        return float(PR.angdist(got, want).max() / max(1.0, np.abs(want).max()))
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) if want.size else 0.0


def yard(f32, f64, angular=()):
    return {k: err(f32[k], w, k in angular) for k, w in f64.items()}


def margin(perturbed, f64, yardstick, angular=(), keys=None):
    """The largest error / gate over the outputs: how far the perturbed reference misses the gate."""
    return max(err(perturbed[k], f64[k], k in angular) / (GATE * max(yardstick[k], 1e-300))
               for k in (keys or f64))
