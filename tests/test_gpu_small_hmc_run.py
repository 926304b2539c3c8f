"""A run of plain-HMC toy-target steps in one launch (l2hmc_small_hmc_run, small_hmc_run_kernel in
l2hmc_amd/csrc/small_hmc.hip) and `DynamicsSampler.run_hmc` around it.

The yardstick is `DynamicsSampler.run` on the same `hmc=True` dynamics: the loop over `propose(x, dynamics,
do_mh_step=True)` -- fill_normal, l2hmc_small_trajectory, fill_uniform, l2hmc_mix_accept per step --, which
tests/test_gpu_invariance.py holds to the exact target distributions.  The run has to give ITS bits, so every comparison
here is an equality.  Chains never interact and a chain's draws depend on (seed, stream, chain index) only, so the
columns of a ladder (of temperatures, of step sizes) equal the same columns of uniform runs of all chains."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.run_cases import assert_same_run, count_launches

pytestmark = pytest.mark.gpu

GMM3 = ([np.array([1., 0., 0.5]), np.array([0., 1., -0.5]), np.array([-1., -1., 0.])],
        [np.diag([0.05, 0.08, 0.1]), 0.07 * np.eye(3) + 0.02, np.diag([0.1, 0.05, 0.06])], [0.3, 0.5, 0.2])
SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])
GAUSS8_VAR = np.array([0.3, 0.5, 0.8, 1.0, 1.3, 1.7, 2.0, 2.5])
# kind: (x_dim, leapfrog steps, temperature).  The first four are tests/test_gpu_small_run.py's TOYS; "gmm3" is the
# MD = 8 instance with dim < MD, "gauss8" the one with dim = MD, "rw" / "funnel" / "rw8" the analytic instances
TOYS = {"scg": (2, 5, 1.0), "scg_T3": (2, 5, 3.0), "mog": (2, 10, 1.0), "gmm3": (3, 5, 1.0), "gauss8": (8, 5, 1.0),
        "rw": (2, 5, 1.0), "funnel": (2, 5, 1.0), "rw8": (8, 5, 1.0)}
BATCHES = [1, 63, 64, 65, 130]          # a partial wave, an exact one, a wave plus one chain, several workgroups
STEPS = 5


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _energy_function(la, kind):
    if kind.startswith("scg"):
        return la.Gaussian(np.zeros(2), SCG_SIGMA).get_energy_function()
    if kind == "mog":
        m = H.mog_target_oracle()
        return la.GMM(m.mus, m.sigmas, m.pis).get_energy_function()
    if kind == "gmm3":
        return la.GMM(*GMM3).get_energy_function()
    if kind == "gauss8":
        return la.Gaussian(np.linspace(-0.4, 0.4, 8), np.diag(GAUSS8_VAR)).get_energy_function()
    if kind == "rw":
        return la.RoughWell(2, 0.5, easy=True).get_energy_function()
    if kind == "rw8":
        return la.RoughWell(8, 0.5, easy=True).get_energy_function()
    return la.GaussianFunnel(2).get_energy_function()


def _toy(la, kind, eps=0.1, temperature=None):
    """Built as tests/test_gpu_small_run.py::_toy(hmc=True): oracle masks, seed 7, draws at 4."""
    from oracle import dynamics as od
    dim, N, temp = TOYS[kind]
    dyn = la.Dynamics(dim, _energy_function(la, kind), trajectory_length=N, eps=eps, hmc=True, use_temperature=True,
                      seed=7)
    dyn.temperature = temp if temperature is None else temperature
    dyn.set_masks(od.make_masks(N, dim, np.random.RandomState(3)))
    dyn._draws = 4
    assert dyn.hmc and not dyn.layered
    return dyn


def _sampler(la, kind, spl=256, **kw):
    smp = la.DynamicsSampler(_toy(la, kind, **kw))
    assert smp.steps_per_launch == 256
    smp.steps_per_launch = spl
    return smp


def _x0(B, dim):
    g = torch.Generator(device="cpu").manual_seed(1234 + B)
    return (0.7 * torch.randn(B, dim, generator=g)).to("cuda")


_REFS = {}


def _loop(la, kind, B, steps=STEPS, eps=0.1, temperature=None, schedule=None):
    """`run` on the hmc dynamics -- the loop over `propose` --: computed once per key, never modified.  Returns the
    result and the draw counter it left."""
    key = (kind, B, steps, eps, temperature, None if schedule is None else tuple(schedule))
    if key not in _REFS:
        smp = _sampler(la, kind, eps=eps, temperature=temperature)
        x0 = _x0(B, smp.dynamics.x_dim)
        out = smp.run(steps, x0, keep_samples=True) if schedule is None else \
            smp.run(steps, x0, keep_samples=True, temperature=schedule)
        _REFS[key] = (out, smp.dynamics._draws)
    return _REFS[key]


def _assert_same_run(a, b, what):
    assert set(a) == set(b) == {"px", "samples", "samples_out", "mean_accept"}, what
    assert_same_run(a, b, ("px", "samples"), what)


def _run_hmc(la, kind, B, steps=STEPS, spl=256, dyn_eps=0.1, dyn_temperature=None, **kw):
    """One `run_hmc` from the case's start, seed and draw counter; checks what every run must leave alone."""
    smp = _sampler(la, kind, spl, eps=dyn_eps, temperature=dyn_temperature)
    dyn = smp.dynamics
    dim, alpha, temp = dyn.x_dim, dyn.alpha.clone(), dyn.temperature
    x0 = _x0(B, dim)
    keep = x0.clone()
    out = smp.run_hmc(steps, x0, keep_samples=True, **kw)
    assert torch.equal(x0, keep)                                     # the caller's x is not advanced in place
    assert torch.equal(dyn.alpha, alpha) and dyn.temperature == temp
    assert dyn._draws == 4 + 2 * steps
    assert out["px"].shape == (steps, B) and out["samples"].shape == (steps, B, dim)
    assert np.array_equal(out["samples"][-1], out["samples_out"].cpu().numpy())
    assert np.isfinite(out["samples"]).all() and (out["px"] >= 0).all() and (out["px"] <= 1).all()
    return out


# ----------------------------------------------------------------- 1. the run against the loop, bit for bit
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", list(TOYS))
def test_run_hmc_equals_the_loop(la, kind, B):
    a = _run_hmc(la, kind, B)
    b, draws = _loop(la, kind, B)
    _assert_same_run(a, b, f"{kind} B={B}")
    assert draws == 4 + 2 * STEPS


def test_runs_move_and_reject(la):
    """The equalities above are not those of frozen or of always-accepting chains (MoG, 130 chains, eps = 0.1)."""
    a = _run_hmc(la, "mog", 130)
    x0 = _x0(130, 2).cpu().numpy()
    path = np.concatenate([x0[None], a["samples"]])
    moved = (path[1:] != path[:-1]).any(axis=2)
    print(f"mean_accept={a['mean_accept']:.4f} moved={moved.mean():.4f}")
    assert 0.0 < a["mean_accept"] < 1.0, a["mean_accept"]
    assert moved.any() and not moved.all(), (moved.mean(), a["mean_accept"])


# ----------------------------------------------------------------- 2. chunks and launches
def test_run_in_chunks_with_a_shorter_last_one(la):
    a = _run_hmc(la, "mog", 130, steps=7, spl=3)
    b, draws = _loop(la, "mog", 130, steps=7)
    _assert_same_run(a, b, "7 steps, 3 per launch")
    assert draws == 4 + 2 * 7


def test_run_hmc_is_one_launch_per_chunk(la):
    x = _x0(64, 2)
    for spl in (8, 3):
        smp = _sampler(la, "mog", spl)
        smp.run_hmc(8, x)                                            # warm-up
        assert count_launches(7, lambda: smp.run_hmc(8, x)) == math.ceil(8 / spl)


# ----------------------------------------------------------------- 3. the C entry on its own
@pytest.mark.parametrize("kind,B", [("mog", 70), ("gmm3", 33), ("rw", 65)])
def test_c_entry_outputs_are_optional_and_it_runs_in_place(la, kind, B):
    from l2hmc_amd import _lib
    L, n = _lib.lib(), 4
    dyn = _toy(la, kind)
    D, seed, draw0 = dyn.x_dim, 77, 5
    plan = dyn._plan()
    x0 = _x0(B, D)

    def call(x_in, x_next, full):
        px = torch.empty(n, B, device="cuda") if full else None
        samples = torch.empty(n, B, D, device="cuda") if full else None
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(L.l2hmc_small_hmc_run(C.byref(plan), x_in.data_ptr(), x_next.data_ptr(), B, seed, draw0, n, None, 0,
                                         0, None, ptr(px), ptr(samples), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return px, samples

    full, again, bare, inplace = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0), x0.clone()
    px, samples = call(x0, full, True)
    px2, samples2 = call(x0, again, True)
    call(x0, bare, False)
    call(inplace, inplace, False)
    assert torch.equal(full, again) and torch.equal(px, px2) and torch.equal(samples, samples2)
    assert torch.equal(full, bare) and torch.equal(full, inplace) and torch.equal(samples[-1], full)
    assert not torch.equal(full, x0)
    # the steps chain: two calls of two steps, the second on the streams after the first's
    half = torch.empty_like(x0)
    _lib.check(L.l2hmc_small_hmc_run(C.byref(plan), x0.data_ptr(), half.data_ptr(), B, seed, draw0, 2, None, 0, 0, None,
                                     None, None, _lib.stream_ptr()))
    _lib.check(L.l2hmc_small_hmc_run(C.byref(plan), half.data_ptr(), half.data_ptr(), B, seed, draw0 + 4, 2, None, 0, 0,
                                     None, None, None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(half, full)


# ----------------------------------------------------------------- 4. temperature
SCHEDULE = np.array([2.5, 0.7, 1.0, 3.25, 1.3], dtype=np.float32)      # five distinct values, 1 / t inexact for most
LADDER = np.array([0.7, 1.0, 2.5], dtype=np.float32)                    # chain c at LADDER[c % 3]: mixed within a wave
TEMPERED = [("mog", 70), ("gmm3", 65), ("rw", 70)]


@pytest.mark.parametrize("kind,B", TEMPERED)
def test_a_schedule_equals_the_loop(la, kind, B):
    a = _run_hmc(la, kind, B, spl=2, temperature=SCHEDULE)              # three launches: 2 + 2 + 1 steps
    b, _ = _loop(la, kind, B, schedule=SCHEDULE)
    _assert_same_run(a, b, f"schedule {kind} B={B}")


@pytest.mark.parametrize("kind,B", TEMPERED)
def test_a_ladder_equals_uniform_runs_column_by_column(la, kind, B):
    temps = LADDER[np.arange(B) % 3]
    lad = _run_hmc(la, kind, B, temperature=temps[None])
    both = _run_hmc(la, kind, B, spl=2, temperature=np.broadcast_to(temps, (STEPS, B)))
    _assert_same_run(lad, both, f"[n, B] with constant columns, {kind}")
    unis = []
    for k, T in enumerate(LADDER):
        uni = _run_hmc(la, kind, B, dyn_temperature=float(T))           # the untempered instance at temperature T
        unis.append(uni)
        scalar = _run_hmc(la, kind, B, temperature=float(T))
        _assert_same_run(uni, scalar, f"scalar temperature {T}, {kind}")
        cols = np.arange(B) % 3 == k
        assert np.array_equal(lad["px"][:, cols], uni["px"][:, cols]), (kind, T)
        assert np.array_equal(lad["samples"][:, cols], uni["samples"][:, cols]), (kind, T)
    hot = np.arange(B) % 3 == 2                                         # the temperature does matter
    assert not np.array_equal(lad["px"][:, hot], unis[0]["px"][:, hot])


# ----------------------------------------------------------------- 5. a step size per chain
EPS = (0.05, 0.1, 0.25)


@pytest.mark.parametrize("kind,B", [("mog", 130), ("gauss8", 65), ("funnel", 63)])
def test_an_eps_ladder_equals_uniform_runs_column_by_column(la, kind, B):
    """The uniform run at e is `run_hmc` on a dynamics BUILT with eps = e (which stores exp(log e) in float32, not
    necessarily the literal); the ladder is given that dynamics' own float(eps)."""
    stored = [float(_toy(la, kind, eps=e).eps) for e in EPS]
    ladder = np.array(stored, dtype=np.float32)[np.arange(B) % 3]
    smp = _sampler(la, kind)
    x0 = _x0(B, smp.dynamics.x_dim)
    lad = smp.run_hmc(STEPS, x0, eps=ladder)
    assert smp.dynamics._draws == 4 + 2 * STEPS and float(smp.dynamics.eps) == stored[1]
    unis = []
    for k, e in enumerate(EPS):
        uni = _run_hmc(la, kind, B, dyn_eps=e)
        unis.append(uni)
        cols = np.arange(B) % 3 == k
        assert np.array_equal(lad["px"][:, cols], uni["px"][:, cols]), (kind, e)
        assert np.array_equal(lad["samples"][:, cols], uni["samples"][:, cols]), (kind, e)
        assert torch.equal(lad["samples_out"][torch.from_numpy(cols).to("cuda")],
                           uni["samples_out"][torch.from_numpy(cols).to("cuda")]), (kind, e)
        # a scalar eps on the eps = 0.1 dynamics is the uniform run as well
        sc = _sampler(la, kind)
        _assert_same_run(sc.run_hmc(STEPS, x0, eps=stored[k]), uni, f"scalar eps {e}, {kind}")
    big = np.arange(B) % 3 == 2                                         # the step size does matter
    assert not np.array_equal(lad["px"][:, big], unis[0]["px"][:, big])


def test_no_eps_is_the_dynamics_own(la):
    smp, ref = _sampler(la, "mog"), _sampler(la, "mog")
    x0 = _x0(70, 2)
    _assert_same_run(smp.run_hmc(STEPS, x0, eps=float(smp.dynamics.eps)), ref.run_hmc(STEPS, x0), "eps=None")
    assert smp.dynamics._draws == ref.dynamics._draws == 4 + 2 * STEPS
