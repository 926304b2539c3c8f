"""A temperature per step, per chain, or both inside a one-launch toy-target run (l2hmc_small_run_tempered, the TEMPERED
instances of small_traj_mfma_kernel in l2hmc_amd/csrc/small_mlp.hip) and `DynamicsSampler.run(..., temperature=)`.

Every reference is exact.  Chains never interact and a chain's draws depend on (seed, draw, chain index) only, so
  * a schedule equals the loop over `propose` with `dynamics.temperature` set before each step (`steps_per_launch = 1`),
  * the columns of a ladder equal the same columns of uniform runs at their temperatures, and
  * a run whose temperatures all equal T equals today's `run` on a dynamics with `temperature = T`,
bit for bit: every comparison is an equality.  The loop and the untempered run are themselves held to the float64 oracle
and to the exact target distributions by tests/test_gpu_parity.py, test_gpu_small_run.py and test_gpu_invariance.py.

The last test asks the target itself what a ladder means: two temperature groups of a Gaussian target, each started
from exact draws of N(0, T Sigma), must each stay there (the statistic and threshold of tests/test_gpu_invariance.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import invariance as I

pytestmark = pytest.mark.gpu

SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])
STEPS, SPL = 5, 2                                   # three launches: 2 + 2 + 1 steps
SCHEDULE = np.array([2.5, 0.7, 1.0, 3.25, 1.3], dtype=np.float32)      # five distinct values, 1 / t inexact for most
LADDER = np.array([0.7, 1.0, 2.5], dtype=np.float32)                    # chain c at LADDER[c % 3]: mixed within a wave
T_CONST = 0.7

# (target, hidden units, first_layer_form, chains, leapfrog steps): every target kind at every width and form (form 3,
# two waves per group, exists above 16 hidden units), B = 13 (a ragged last wave of eight-chain groups) and 24 with each
CASES = [(t, nodes, form, (13, 24)[(i + j) % 2], 3 + (i + j) % 3)
         for i, t in enumerate(("mog", "scg", "rw", "funnel"))
         for j, (nodes, form) in enumerate(((10, 1), (10, 2), (50, 1), (50, 2), (50, 3)))]
IDS = [f"{t}-H{n}-form{f}-B{b}-N{N}" for t, n, f, b, N in CASES]
# the instances of x_dim > 2 (chain state of up to 8 components): a 3-D mixture at 64 hidden units
CASES_3D = [("gmm3", 64, 1, 13, 3), ("gmm3", 64, 3, 24, 4)]
GMM3 = ([np.array([1., 0., 0.5]), np.array([0., 1., -0.5]), np.array([-1., -1., 0.])],
        [np.diag([0.05, 0.08, 0.1]), 0.07 * np.eye(3) + 0.02, np.diag([0.1, 0.05, 0.06])], [0.3, 0.5, 0.2])


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _energy_function(la, target):
    if target == "gmm3":
        return la.GMM(*GMM3).get_energy_function()
    if target == "mog":
        m = H.mog_target_oracle()
        return la.GMM(m.mus, m.sigmas, m.pis).get_energy_function()
    if target == "scg":
        return la.Gaussian(np.zeros(2), SCG_SIGMA).get_energy_function()
    if target == "rw":
        return la.RoughWell(2, 0.5, True).get_energy_function()
    return la.GaussianFunnel(2).get_energy_function()


def _dim(case):
    return 3 if case[0] == "gmm3" else 2


def _sampler(la, case, spl=SPL, temperature=1.0):
    """Stress-regime nets, oracle masks, seed 7, draws at 4 (as tests/test_gpu_small_run.py::_toy)."""
    from oracle import dynamics as od
    target, nodes, form, _, N = case
    dim = _dim(case)
    xp, vp = H.mlp_weights(dim, nodes, seed=106, regime="stress")
    dyn = la.Dynamics(dim, _energy_function(la, target), trajectory_length=N, eps=0.1,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes),
                      use_temperature=True, seed=7)
    dyn.temperature = temperature
    dyn.set_masks(od.make_masks(N, dim, np.random.RandomState(3)))
    dyn.XNet.load_state(xp)
    dyn.VNet.load_state(vp)
    dyn.first_layer_form = form
    dyn._draws = 4
    assert not dyn.layered
    smp = la.DynamicsSampler(dyn)
    smp.steps_per_launch = spl
    return smp


def _x0(B, dim=2):
    g = torch.Generator(device="cpu").manual_seed(1234 + B)
    return (0.7 * torch.randn(B, dim, generator=g)).to("cuda")


def _run(la, case, temperature=None, spl=SPL, dyn_temperature=1.0):
    """One run of STEPS steps from the case's start, seed and draw counter; checks what every run must leave alone."""
    smp = _sampler(la, case, spl, dyn_temperature)
    x0 = _x0(case[3], _dim(case))
    keep = x0.clone()
    out = smp.run(STEPS, x0, keep_samples=True) if temperature is None else \
        smp.run(STEPS, x0, keep_samples=True, temperature=temperature)
    assert torch.equal(x0, keep)                                   # the caller's x is not advanced in place
    assert smp.dynamics.temperature == dyn_temperature             # nor is the dynamics' temperature touched
    assert smp.dynamics._draws == 4 + 4 * STEPS
    assert out["px"].shape == (STEPS, case[3]) and out["samples"].shape == (STEPS, case[3], _dim(case))
    assert out["px"].dtype == out["samples"].dtype == np.float32
    assert np.isfinite(out["px"]).all() and np.isfinite(out["samples"]).all()
    assert np.array_equal(out["samples"][-1], out["samples_out"].cpu().numpy())
    return out


_REFS = {}


def _uniform(la, case, T):
    """Today's run (l2hmc_small_run) at `dynamics.temperature = T`: computed once per (case, T), never modified."""
    T = float(np.float32(T))
    key = ("uniform", case, T)
    if key not in _REFS:
        _REFS[key] = _run(la, case, dyn_temperature=T)
    return _REFS[key]


def _loop(la, case, scale):
    """The loop over `propose` (`steps_per_launch = 1`) with `dynamics.temperature` = fl32(SCHEDULE[s] * scale) before
    step s: once per (case, scale)."""
    key = ("loop", case, float(np.float32(scale)))
    if key not in _REFS:
        _REFS[key] = _run(la, case, temperature=SCHEDULE * np.float32(scale), spl=1)
    return _REFS[key]


def _assert_same(a, b, what, cols=slice(None)):
    for k in ("px", "samples"):
        assert np.array_equal(a[k][:, cols], b[k][:, cols]), (what, k, float(np.abs(a[k][:, cols] - b[k][:, cols]).max()))
    assert torch.equal(a["samples_out"][cols], b["samples_out"][cols]), what


def _differ(a, b, cols=slice(None)):
    return not np.array_equal(a["px"][:, cols], b["px"][:, cols])


# ----------------------------------------------------------------- 1. a schedule against the loop
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_schedule_equals_the_loop_that_sets_the_temperature_per_step(la, case):
    got = _run(la, case, temperature=SCHEDULE)
    want = _loop(la, case, 1.0)
    _assert_same(got, want, "schedule")
    assert got["mean_accept"] == want["mean_accept"]
    # the comparison has something to see: the temperature matters to this case, and its chains move
    assert _differ(got, _uniform(la, case, 1.0))
    assert (got["samples"][1:] != got["samples"][:-1]).any()


# ----------------------------------------------------------------- 2. constant temperatures against today's run
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_constant_temperatures_equal_the_untempered_run_at_that_temperature(la, case):
    B = case[3]
    want = _uniform(la, case, T_CONST)
    assert _differ(want, _uniform(la, case, 1.0))
    for name, t in (("scalar", T_CONST), ("schedule", np.full(STEPS, T_CONST)), ("ladder", np.full((1, B), T_CONST)),
                    ("both", np.full((STEPS, B), T_CONST))):
        # the dynamics' own temperature is not what the tempered entry runs at
        got = _run(la, case, temperature=t, dyn_temperature=1.0 if name != "both" else 4.0)
        _assert_same(got, want, name)
        assert got["mean_accept"] == want["mean_accept"]


# ----------------------------------------------------------------- 3. a ladder against uniform runs
def _groups(B):
    return [np.arange(g, B, 3) for g in range(3)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ladder_columns_equal_uniform_runs_at_their_temperatures(la, case):
    B = case[3]
    got = _run(la, case, temperature=LADDER[np.arange(B) % 3][None])
    for g, cols in enumerate(_groups(B)):
        _assert_same(got, _uniform(la, case, LADDER[g]), f"ladder group {g}", cols)
        other = _uniform(la, case, LADDER[(g + 1) % 3])
        assert _differ(got, other, cols), g                         # and not the neighbouring temperature's


# ----------------------------------------------------------------- 4. both: a schedule per chain group
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_schedule_times_ladder_equals_the_loops_at_the_matching_temperatures(la, case):
    B = case[3]
    temps = SCHEDULE[:, None] * LADDER[np.arange(B) % 3][None, :]             # float32 products, as _loop forms them
    assert temps.dtype == np.float32 and temps.shape == (STEPS, B)
    got = _run(la, case, temperature=temps)
    for g, cols in enumerate(_groups(B)):
        _assert_same(got, _loop(la, case, LADDER[g]), f"both, group {g}", cols)
        assert _differ(got, _loop(la, case, LADDER[(g + 1) % 3]), cols), g


@pytest.mark.parametrize("case", CASES_3D, ids=["gmm3-H64-form1-B13-N3", "gmm3-H64-form3-B24-N4"])
def test_three_dimensions_schedule_ladder_and_both(la, case):
    B = case[3]
    _assert_same(_run(la, case, temperature=SCHEDULE), _loop(la, case, 1.0), "schedule")
    _assert_same(_run(la, case, temperature=np.full((1, B), T_CONST)), _uniform(la, case, T_CONST), "constant")
    ladder = _run(la, case, temperature=LADDER[np.arange(B) % 3][None])
    both = _run(la, case, temperature=SCHEDULE[:, None] * LADDER[np.arange(B) % 3][None, :])
    for g, cols in enumerate(_groups(B)):
        _assert_same(ladder, _uniform(la, case, LADDER[g]), f"ladder group {g}", cols)
        _assert_same(both, _loop(la, case, LADDER[g]), f"both, group {g}", cols)
        assert _differ(ladder, _uniform(la, case, LADDER[(g + 1) % 3]), cols), g


# ----------------------------------------------------------------- 5. bookkeeping (the rest is asserted by every _run)
BOOK = [CASES[0], CASES[9], CASES[12], CASES[18]]     # mog H10 form 1, scg H50 form 3, rw H50 form 1, funnel H50 form 2


@pytest.mark.parametrize("case", BOOK, ids=[IDS[CASES.index(c)] for c in BOOK])
def test_keep_samples_false_and_the_c_entry_in_place(la, case):
    from l2hmc_amd import _lib
    L, B = _lib.lib(), case[3]
    temps = SCHEDULE[:, None] * LADDER[np.arange(B) % 3][None, :]
    want = _run(la, case, temperature=temps, spl=256)                # one launch of five steps
    smp = _sampler(la, case, 256)
    out = smp.run(STEPS, _x0(B), keep_samples=False, temperature=temps)
    assert set(out) == {"px", "samples_out", "mean_accept"} and smp.dynamics._draws == 4 + 4 * STEPS
    assert np.array_equal(out["px"], want["px"]) and torch.equal(out["samples_out"], want["samples_out"])
    # the C entry: x_next aliasing x_in, the optional outputs left out, each stride pair
    dyn = _sampler(la, case).dynamics
    plan = dyn._plan()
    tdev = torch.as_tensor(temps, device="cuda").contiguous()

    def call(x_in, x_next, t, ss, cs, full=False):
        px = torch.empty(STEPS, B, device="cuda") if full else None
        samples = torch.empty(STEPS, B, 2, device="cuda") if full else None
        ptr = lambda a: None if a is None else a.data_ptr()       # noqa: E731
        _lib.check(L.l2hmc_small_run_tempered(C.byref(plan), x_in.data_ptr(), x_next.data_ptr(), B, 7, 4, STEPS,
                                              t.data_ptr(), ss, cs, ptr(px), ptr(samples), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return px, samples
    x0 = _x0(B)
    apart, inplace = torch.empty_like(x0), x0.clone()
    px, samples = call(x0, apart, tdev, B, 1, full=True)
    call(inplace, inplace, tdev, B, 1)
    assert torch.equal(apart, want["samples_out"]) and torch.equal(inplace, apart)
    assert np.array_equal(px.cpu().numpy(), want["px"]) and np.array_equal(samples.cpu().numpy(), want["samples"])
    for t, ss, cs, ref in ((torch.as_tensor(SCHEDULE, device="cuda"), 1, 0, _loop(la, case, 1.0)),
                           (torch.full((1,), T_CONST, device="cuda"), 0, 0, _uniform(la, case, T_CONST))):
        x_next = torch.empty_like(x0)
        call(x0, x_next, t, ss, cs)
        assert torch.equal(x_next, ref["samples_out"]), (ss, cs)


def test_the_host_loop_on_the_device_refuses_a_ladder_and_restores_the_temperature(la):
    case = CASES[0]
    smp = _sampler(la, case, spl=1, temperature=1.75)
    with pytest.raises(NotImplementedError, match="one-launch"):
        smp.run(STEPS, _x0(13), temperature=np.full((1, 13), 2.0))
    assert smp.dynamics._draws == 4 and smp.dynamics.temperature == 1.75
    with pytest.raises(ValueError, match="finite and > 0"):
        _sampler(la, case).run(STEPS, _x0(13), temperature=[1.0, 2.0, 0.0, 1.0, 1.0])


# ----------------------------------------------------------------- 6. a ladder means what it says
CHECKPOINTS = (1, 4, 16)                # tests/test_gpu_invariance.py: the checkpoints, bars and the Gaussian case's
Z_PASS, Z_DEFECT = 5.0, 8.0             # shape (2-D, 5 leapfrog steps, eps 0.1, 32 hidden units, 2^20 chains)
ACCEPT_RANGE = (0.2, 0.95)
LADDER2 = (1.0, 3.0)


@pytest.mark.parametrize("form", [1, 2])
def test_each_temperature_group_of_a_ladder_leaves_its_own_target_invariant(la, form):
    """Chain c runs at LADDER2[c % 2] and starts as an exact float64 draw of N(0, T_c Sigma).  If the step of chain c
    leaves exp(-E / T_c) invariant, group g is an exact sample of its target after every step, and
    z = (mean f - E f) / (sd f / sqrt(n)) is N(0, 1) for every test function: max |z| < 5 per group at steps 1, 4, 16.
    Against the OTHER group's target the same statistic must exceed 8: the groups are told apart."""
    B = 1 << 20
    smp = _sampler(la, ("scg", 32, form, B, 5), spl=256)
    exact = [I.ExactGMM.of_library_gaussian(np.zeros(2), SCG_SIGMA, temperature=T) for T in LADDER2]
    x0 = np.empty((B, 2))
    for g, ex in enumerate(exact):
        x0[g::2] = ex.sample(B // 2, np.random.default_rng(1 + g))
    x = torch.as_tensor(x0, dtype=torch.float32, device="cuda")
    temps = np.asarray(LADDER2, dtype=np.float32)[np.arange(B) % 2][None]
    halves = [ex.halfspaces(np.random.default_rng(5)) for ex in exact]
    zs, zs_swapped, done, acc = [[], []], [[], []], 0, None
    for k in CHECKPOINTS:                                            # runs of 1, 3 and 12 steps
        out = smp.run(k - done, x, keep_samples=False, temperature=temps)
        x, done = out["samples_out"], k
        acc = out["mean_accept"] if acc is None else acc
        xs = x.double().cpu().numpy()
        for g in range(2):
            for into, ex, (W, c) in ((zs, exact[g], halves[g]), (zs_swapped, exact[1 - g], halves[1 - g])):
                into[g].append(I.zscores(ex.features(xs[g::2], W, c), ex.expectations(W, c)))
    worst = [float(np.abs(np.array(z)).max()) for z in zs]
    swapped = [float(np.abs(np.array(z)).max()) for z in zs_swapped]
    print(f"\n[tempered ladder] form {form}: max|z| per group {worst[0]:.2f}, {worst[1]:.2f}; against the other "
          f"group's target {swapped[0]:.1f}, {swapped[1]:.1f}; accept {acc:.3f}")
    assert smp.dynamics._draws == 4 + 4 * 16
    assert ACCEPT_RANGE[0] < acc < ACCEPT_RANGE[1], acc
    assert max(worst) < Z_PASS, zs
    assert min(swapped) > Z_DEFECT, zs_swapped
