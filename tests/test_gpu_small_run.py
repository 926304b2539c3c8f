"""A run of toy-target L2HMC steps in one launch (l2hmc_small_run, the RUN instance of small_traj_mfma_kernel in
l2hmc_amd/csrc/small_mlp.hip) and `DynamicsSampler` around it.

The yardstick is the loop over `propose(x, dynamics, do_mh_step=True)` (`steps_per_launch = 1`), which
tests/test_gpu_invariance.py holds to the exact target distributions and tests/test_gpu_parity.py to the piecewise path:
the run has to give ITS bits, so every comparison here is an equality."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.helpers import _graph_shape, _hip            # noqa: F401  (tests/test_gpu_small_run_exchange.py imports them from here)
from tests.run_cases import assert_same_run, count_launches

pytestmark = pytest.mark.gpu

GMM3 = ([np.array([1., 0., 0.5]), np.array([0., 1., -0.5]), np.array([-1., -1., 0.])],
        [np.diag([0.05, 0.08, 0.1]), 0.07 * np.eye(3) + 0.02, np.diag([0.1, 0.05, 0.06])], [0.3, 0.5, 0.2])
SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])
# kind: (x_dim, leapfrog steps, hidden units, temperature)
TOYS = {"scg": (2, 5, 10, 1.0), "scg_T3": (2, 5, 10, 3.0), "mog": (2, 10, 50, 1.0), "gmm3": (3, 5, 64, 1.0),
        "mog_wide": (2, 5, 96, 1.0)}


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _toy(la, kind, form=0, hmc=False, temperature=None):
    """Built as tests/test_gpu_invariance.py::_toy: stress-regime nets, oracle masks, seed 7, draws at 4."""
    from oracle import dynamics as od
    dim, N, nodes, temp = TOYS[kind]
    if kind.startswith("scg"):
        fn = la.Gaussian(np.zeros(2), SCG_SIGMA).get_energy_function()
    elif kind.startswith("mog"):
        m = H.mog_target_oracle()
        fn = la.GMM(m.mus, m.sigmas, m.pis).get_energy_function()
    else:
        fn = la.GMM(*GMM3).get_energy_function()
    xp, vp = H.mlp_weights(dim, nodes, seed=106, regime="stress")
    dyn = la.Dynamics(dim, fn, trajectory_length=N, eps=0.1, hmc=hmc,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes),
                      use_temperature=True, seed=7)
    dyn.temperature = temp if temperature is None else temperature
    dyn.set_masks(od.make_masks(N, dim, np.random.RandomState(3)))
    if not hmc:
        dyn.XNet.load_state(xp)
        dyn.VNet.load_state(vp)
    dyn.first_layer_form = form
    dyn._draws = 4
    return dyn


def _sampler(la, kind, form=0, spl=256, **kw):
    smp = la.DynamicsSampler(_toy(la, kind, form, **kw))
    assert smp.steps_per_launch == 256
    smp.steps_per_launch = spl
    return smp


def _x0(B, dim):
    g = torch.Generator(device="cpu").manual_seed(1234 + B)
    return (0.7 * torch.randn(B, dim, generator=g)).to("cuda")


def _assert_same_run(a, b, sa, sb, what):
    assert set(a) == set(b) == {"px", "samples", "samples_out", "mean_accept"}, what
    assert_same_run(a, b, ("px", "samples"), what)
    assert sa.dynamics._draws == sb.dynamics._draws, what


def _compare(la, kind, form, B, steps, spl=256):
    new, old = _sampler(la, kind, form, spl), _sampler(la, kind, form, 1)
    dim = new.dynamics.x_dim
    x0 = _x0(B, dim)
    keep = x0.clone()
    a = new.run(steps, x0, keep_samples=True)
    b = old.run(steps, x0, keep_samples=True)
    assert torch.equal(x0, keep)                                     # the caller's x is not advanced in place
    _assert_same_run(a, b, new, old, f"{kind} form={form} B={B} steps={steps} per launch={spl}")
    assert a["px"].shape == (steps, B) and a["samples"].shape == (steps, B, dim)
    assert np.array_equal(a["samples"][-1], a["samples_out"].cpu().numpy())
    assert new.dynamics._draws == 4 + 4 * steps
    assert (a["px"] >= 0).all() and (a["px"] <= 1).all()
    return a


# ----------------------------------------------------------------- 1. the run against the loop, bit for bit
CASES = [(k, f) for k in ("scg", "scg_T3", "mog", "gmm3") for f in (1, 2, 3)
         if not (f == 3 and TOYS[k][2] <= 16)]                      # no twin instance at 16 hidden units or fewer


@pytest.mark.parametrize("B", [1, 7, 8, 9, 33, 70])
@pytest.mark.parametrize("kind,form", CASES)
def test_run_equals_the_loop(la, kind, form, B):
    _compare(la, kind, form, B, steps=5)


def test_runs_move_and_reject(la):
    """The equalities above are not those of frozen or of always-accepting chains."""
    a = _compare(la, "mog", 0, 70, steps=5)
    moved = (a["samples"][1:] != a["samples"][:-1]).any(axis=2)
    assert moved.any() and not moved.all(), (moved.mean(), a["mean_accept"])
    assert 0.0 < a["mean_accept"] < 1.0, a["mean_accept"]


@pytest.mark.parametrize("B,steps", [(4096, 5), (4097, 5), (8200, 2)])
def test_run_equals_the_loop_where_the_automatic_form_changes(la, B, steps):
    """first_layer_form = 0: 2 B rows in groups of 16 -- two waves per group up to 512 groups (B = 4096), the
    matrix-pipe first layer up to 1024 (B = 4097), the VALU one beyond (B = 8200)."""
    _compare(la, "mog", 0, B, steps)


# ----------------------------------------------------------------- 2. chunks
@pytest.mark.parametrize("form", [1, 3])
def test_run_in_chunks_with_a_shorter_last_one(la, form):
    _compare(la, "mog", form, 70, steps=7, spl=3)


# ----------------------------------------------------------------- 3. the C entry on its own
@pytest.mark.parametrize("kind,form,B", [("mog", 3, 70), ("mog", 2, 9), ("scg", 1, 1), ("gmm3", 1, 33)])
def test_c_entry_equals_chained_proposes_and_its_outputs_are_optional(la, kind, form, B):
    from l2hmc_amd import _lib
    L, n = _lib.lib(), 4
    dyn = _toy(la, kind, form)
    D, seed, draw0 = dyn.x_dim, 77, 5
    plan = dyn._plan()
    x0 = _x0(B, D)

    def call(x_in, x_next, full):
        px = torch.empty(n, B, device="cuda") if full else None
        samples = torch.empty(n, B, D, device="cuda") if full else None
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(L.l2hmc_small_run(C.byref(plan), x_in.data_ptr(), x_next.data_ptr(), B, seed, draw0, n, ptr(px),
                                     ptr(samples), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return px, samples

    full, again, bare, inplace = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0), x0.clone()
    px, samples = call(x0, full, True)
    px2, samples2 = call(x0, again, True)
    call(x0, bare, False)
    call(inplace, inplace, False)
    assert torch.equal(full, again) and torch.equal(px, px2) and torch.equal(samples, samples2)
    assert torch.equal(full, bare) and torch.equal(full, inplace) and torch.equal(samples[-1], full)
    x = x0
    for s in range(n):
        xn, p = torch.empty_like(x), torch.empty(B, device="cuda")
        _lib.check(L.l2hmc_small_propose(C.byref(plan), x.data_ptr(), B, seed, draw0 + 4 * s, None, None, p.data_ptr(),
                                         xn.data_ptr(), _lib.stream_ptr()))
        assert torch.equal(p, px[s]) and torch.equal(xn, samples[s]), s
        x = xn
    assert torch.equal(x, full)


# ----------------------------------------------------------------- 4. launches
def test_run_is_one_launch_per_chunk(la):
    x = _x0(64, 2)
    for spl in (8, 3, 1):
        smp = _sampler(la, "mog", 0, spl)
        smp.run(8, x)                                                # warm-up
        assert count_launches(7, lambda: smp.run(8, x)) == (math.ceil(8 / spl) if spl > 1 else 8)


# ----------------------------------------------------------------- 5. dynamics the kernel does not hold
@pytest.mark.parametrize("kind,hmc", [("mog", True), ("mog_wide", False)])
def test_other_dynamics_run_the_loop_over_propose(la, kind, hmc):
    B, n = 9, 4
    smp = _sampler(la, kind, hmc=hmc)
    ref = _toy(la, kind, hmc=hmc)
    assert smp.dynamics.layered == (kind == "mog_wide") and smp.steps_per_launch == 256
    x0 = _x0(B, 2)
    out = smp.run(n, x0, keep_samples=True)
    x = x0
    for s in range(n):
        _, _, px, (x,) = la.propose(x, ref, do_mh_step=True)
        assert np.array_equal(out["px"][s], px.cpu().numpy()) and np.array_equal(out["samples"][s], x.cpu().numpy()), s
    assert torch.equal(out["samples_out"], x) and smp.dynamics._draws == ref._draws
    assert out["mean_accept"] == float(out["px"].mean(dtype=np.float64))


# ----------------------------------------------------------------- 6. generate_trajectories
def test_generate_trajectories_has_the_reference_layout(la):
    B, n = 33, 6
    dyn = _toy(la, "mog")
    m = H.mog_target_oracle()
    smp = la.DynamicsSampler(dyn, distribution=la.GMM(m.mus, m.sigmas, m.pis))
    x0 = _x0(B, 2)
    traj, px = smp.generate_trajectories(temp=1., num_samples=B, num_steps=n, x=x0)
    assert dyn.temperature == 1.0 and dyn._draws == 4 + 4 * n
    run = _sampler(la, "mog").run(n, x0)
    assert traj.shape == (n, B, 2) and px.shape == (n, B) and traj.dtype == px.dtype == np.float32
    assert np.array_equal(traj[0], x0.cpu().numpy())
    assert np.array_equal(traj[1:], run["samples"][:-1]) and np.array_equal(px, run["px"])
    # the start drawn from the distribution (NumPy's global stream, as the reference)
    np.random.seed(5)
    want0 = la.GMM(m.mus, m.sigmas, m.pis).get_samples(12).astype(np.float32)
    np.random.seed(5)
    traj, px = smp.generate_trajectories(num_samples=12, num_steps=3)
    assert traj.shape == (3, 12, 2) and px.shape == (3, 12) and np.array_equal(traj[0], want0)
    rates = la.stats.calc_tunneling_rate(traj, np.stack(m.mus))
    assert rates.shape == (12,) and (rates >= 0).all() and (rates <= 1).all()


def test_generate_trajectories_sets_and_restores_the_temperature(la):
    B, n = 33, 5
    x0 = _x0(B, 2)
    smp = _sampler(la, "scg")
    assert smp.dynamics.temperature == 1.0
    traj, px = smp.generate_trajectories(temp=3., num_samples=B, num_steps=n, x=x0)
    assert smp.dynamics.temperature == 1.0
    hot = _sampler(la, "scg", temperature=3.0).run(n, x0)
    cold = _sampler(la, "scg").run(n, x0)
    assert np.array_equal(px, hot["px"]) and np.array_equal(traj[1:], hot["samples"][:-1])
    assert not np.array_equal(px, cold["px"])


# ----------------------------------------------------------------- 7. graph capture
def test_a_run_is_captured_as_one_kernel_node_and_replays_the_eager_bits(la):
    from l2hmc_amd import _lib
    L, n, B = _lib.lib(), 4, 70
    dyn = _toy(la, "mog")
    plan = dyn._plan()
    x0 = _x0(B, 2)
    px, samples = torch.empty(n, B, device="cuda"), torch.empty(n, B, 2, device="cuda")

    def run(x_in, x_next):
        _lib.check(L.l2hmc_small_run(C.byref(plan), x_in.data_ptr(), x_next.data_ptr(), B, 77, 5, n, px.data_ptr(),
                                     samples.data_ptr(), _lib.stream_ptr()))
    eager = torch.empty_like(x0)
    run(x0, eager)
    torch.cuda.synchronize()
    want = (eager.clone(), px.clone(), samples.clone())
    hip = _hip()
    xin, xg = x0.clone(), torch.empty_like(x0)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            before = _graph_shape(hip, side.cuda_stream)
            run(xin, xg)
            after = _graph_shape(hip, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    assert before == (0, 0, 0) and after == (1, 0, 0), (before, after)
    for _ in range(2):
        xg.zero_(), px.zero_(), samples.zero_()
        xin.copy_(x0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, want[0]) and torch.equal(px, want[1]) and torch.equal(samples, want[2])
