"""Replica exchange inside a plain-HMC toy-target run: `DynamicsSampler.run_hmc_exchange(..., replicas=G, swap_every=k)`
(l2hmc_small_hmc_run_exchange: the rounds between two steps of ONE launch of small_hmc_run_kernel's EXCHANGE instances)
and, for an L2HMC dynamics, `DynamicsSampler.run_exchange` (l2hmc_small_replica_swap between launches of
l2hmc_small_run_tempered).

The round itself is held to float64 in tests/test_gpu_small_replica_swap.py and the run without exchange in
tests/test_gpu_small_hmc_run.py; what is new here is how they are put together, so the yardstick is the loop a caller
would write -- `run_hmc(k, ...)`, then `swap_replicas(...)` with the right parity, on a second dynamics of the same seed
-- and every comparison with it is an equality.  The target is the other yardstick: 4096 groups of exact samples of the
tempered Gaussians at every rung stay exact under HMC steps with a round after each.

Measured on the MI355X (max |z| over rungs, checkpoints and test functions; `_report`'s lines):
  exchange run, swap_every = 1:  3.84  (HMC accept 0.993, 0.670 exchanges per proposed pair and round);
  round replaced by the torch restatement of a defect:  exponent sign flipped 93.60, always accept 68.91.
  The three cases take 0.5 s together, the 25 tests of the file 4 s."""
import math
import time

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import toy_cases as tc
from tests import toy_replica_ref as TR
from tests.replica_ref import lower_chains
from tests.run_cases import count_launches

pytestmark = pytest.mark.gpu

STEPS = 12
# kind: (x_dim, leapfrog steps): the register-held 2-D mixture, a mixture read from LDS, an analytic target
TOYS = {"mog": (2, 10), "gmm5": (5, 4), "rw": (2, 5)}
HIST = ("px",)
ROUNDS = ("swap_p", "swapped", "replica")
EPSS = (0.05, 0.1, 0.2)
Z_PASS, Z_DEFECT = 5.0, 8.0          # tests/test_gpu_invariance.py


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _energy_function(la, kind):
    if kind == "mog":
        m = H.mog_target_oracle()
        return la.GMM(m.mus, m.sigmas, m.pis).get_energy_function()
    if kind == "gmm5":
        return tc.target(5, 8, tc.M)[1].get_energy_function()
    return la.RoughWell(2, 0.5, easy=True).get_energy_function()


def _sampler(la, kind, spl=256, draws=4, hmc=True, nodes=10):
    """Oracle masks, seed 7, draws at 4 (as tests/test_gpu_small_hmc_run.py::_toy); hmc=False: an L2HMC dynamics with
    stress-regime nets (as tests/test_gpu_small_run_tempered.py::_sampler)."""
    from oracle import dynamics as od
    dim, N = TOYS[kind]
    kw = dict(hmc=True) if hmc else dict(
        net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes))
    dyn = la.Dynamics(dim, _energy_function(la, kind), trajectory_length=N, eps=0.1, use_temperature=True, seed=7, **kw)
    dyn.set_masks(od.make_masks(N, dim, np.random.RandomState(3)))
    if not hmc:
        xp, vp = H.mlp_weights(dim, nodes, seed=106, regime="stress")
        dyn.XNet.load_state(xp)
        dyn.VNet.load_state(vp)
    dyn._draws = draws
    assert dyn.hmc == hmc and not dyn.layered
    smp = la.DynamicsSampler(dyn)
    smp.steps_per_launch = spl
    return smp


def _x0(B, dim):
    g = torch.Generator(device="cpu").manual_seed(1234 + B)
    return (0.7 * torch.randn(B, dim, generator=g)).to("cuda")


def _temps(B, G, n=None):
    """[1, B] ladder from 1 to 4 over the rungs of every group, or [n, B]: the ladder scaled a little from step to step"""
    lad = np.tile(np.linspace(1.0, 4.0, G), B // G)[None, :]
    return lad if n is None else lad * (1.0 + 0.02 * np.arange(n))[:, None]


def _loop(smp, n, temps, x, G, k, first_parity=0, **kw):
    """What `run_hmc_exchange(n, x, True, temps, eps, G, k, first_parity)` has to be: run_hmc(k), swap_replicas, ...;
    on an L2HMC dynamics (no eps) what `run_exchange` has to be: run(k, temperature=), swap_replicas, ..."""
    B = x.shape[0]
    temps = np.asarray(temps)
    run = smp.run_hmc if smp.dynamics.hmc else smp.run
    smp.replica = torch.arange(B, dtype=torch.int32, device="cuda")
    parts, rounds, s = [], {r: [] for r in ROUNDS}, 0
    while s < n:
        m = min(k, n - s)
        o = run(m, x, keep_samples=True, temperature=temps if temps.shape[0] == 1 else temps[s:s + m], **kw)
        parts.append(o)
        x = o["samples_out"]
        s += m
        if s % k == 0:
            p, sw, _ = smp.swap_replicas(x, temps[0 if temps.shape[0] == 1 else s - 1], G, (first_parity + s // k - 1) % 2)
            rounds["swap_p"].append(p.cpu().numpy())
            rounds["swapped"].append(sw.cpu().numpy())
            rounds["replica"].append(smp.replica.cpu().numpy().copy())
    out = {key: np.concatenate([o[key] for o in parts]) for key in HIST + ("samples",)}
    out.update({r: np.stack(v) if v else np.empty((0, B)) for r, v in rounds.items()})
    out["samples_out"] = x
    return out


def _assert_same(a, b, sa, sb, what, rounds=True):
    for key in HIST + ("samples",) + (ROUNDS if rounds else ()):
        assert a[key].shape == b[key].shape, (what, key)
        assert np.array_equal(a[key], b[key], equal_nan=(key == "swap_p")), (what, key)
    assert torch.equal(a["samples_out"], b["samples_out"]), what
    assert sa.dynamics._draws == sb.dynamics._draws, what


# ----------------------------------------------------------------- 1. the run is the loop a caller would write
@pytest.mark.parametrize("G", [2, 3, 8])
@pytest.mark.parametrize("kind", list(TOYS))
def test_exchange_run_is_run_hmc_then_swap_replicas(la, kind, G):
    dim = TOYS[kind][0]
    exchanged = 0
    for B in (72, G):                                                # a second, partial workgroup; one group
        x0 = _x0(B, dim)
        keep = x0.clone()
        eps = np.array(EPSS)[np.arange(B) % 3]
        for k in (1, 5):
            temps = _temps(B, G) if k == 1 else _temps(B, G, STEPS)      # a ladder; a ladder with a schedule
            ref_smp = _sampler(la, kind)
            ref = _loop(ref_smp, STEPS, temps, x0, G, k, eps=eps)
            assert ref_smp.dynamics._draws == 4 + 2 * STEPS + STEPS // k
            for spl in (256, 3, 7):                                  # (3, 7: a chunk ends inside a swap period of 5)
                what = f"{kind} B={B} G={G} swap_every={k} steps_per_launch={spl}"
                smp = _sampler(la, kind, spl)
                out = smp.run_hmc_exchange(STEPS, x0, keep_samples=True, temperature=temps, eps=eps, replicas=G,
                                           swap_every=k)
                assert out["swap_p"].shape == (STEPS // k, B) and out["swap_p"].dtype == np.float32, what
                assert out["swapped"].dtype == np.bool_ and out["replica"].dtype == np.int32, what
                assert out["px"].shape == (STEPS, B) and out["samples"].shape == (STEPS, B, dim), what
                _assert_same(out, ref, smp, ref_smp, what)
                assert out["mean_accept"] == float(out["px"].mean(dtype=np.float64)), what
                assert np.array_equal(smp.replica.cpu().numpy(), out["replica"][-1]), what
                exchanged += int(out["swapped"].sum())
        assert torch.equal(x0, keep)                                 # the caller's x is not advanced in place
    assert exchanged > 0


# ----------------------------------------------------------------- 2. a run continues
@pytest.mark.parametrize("kind,B,G", [("mog", 72, 3), ("gmm5", 8, 4), ("rw", 72, 2)])
def test_two_halves_are_the_whole(la, kind, B, G):
    x0, temps = _x0(B, TOYS[kind][0]), _temps(B, G)
    for k, n in ((1, 3), (2, 6), (5, 5)):
        for fp in (0, 1):
            whole_smp, smp = _sampler(la, kind), _sampler(la, kind, spl=4)
            whole = whole_smp.run_hmc_exchange(2 * n, x0, temperature=temps, replicas=G, swap_every=k, first_parity=fp)
            a = smp.run_hmc_exchange(n, x0, temperature=temps, replicas=G, swap_every=k, first_parity=fp)
            b = smp.run_hmc_exchange(n, a["samples_out"], temperature=temps, replicas=G, swap_every=k,
                                     first_parity=(fp + n // k) % 2, replica0=a["replica"][-1])
            both = {key: np.concatenate([a[key], b[key]]) for key in HIST + ("samples",) + ROUNDS}
            both["samples_out"] = b["samples_out"]
            _assert_same(whole, both, whole_smp, smp, f"{kind} G={G} swap_every={k} first_parity={fp}")


# ----------------------------------------------------------------- 3. no exchange asked for
@pytest.mark.parametrize("kind,B", [("mog", 72), ("rw", 65)])
def test_without_replicas_it_is_run_hmc(la, kind, B):
    x0, temps = _x0(B, TOYS[kind][0]), _temps(B, 1, STEPS) * np.linspace(1.0, 2.0, B)[None, :]
    eps = np.array(EPSS)[np.arange(B) % 3]
    for spl in (256, 5):
        sa, sb = _sampler(la, kind, spl), _sampler(la, kind, spl)
        a = sa.run_hmc(STEPS, x0, temperature=temps, eps=eps)
        b = sb.run_hmc_exchange(STEPS, x0, temperature=temps, eps=eps, replicas=None, swap_every=0, first_parity=5,
                                replica0="ignored")
        assert set(a) == set(b) and "swap_p" not in b and sb.replica is None
        _assert_same(a, b, sa, sb, f"{kind} steps_per_launch={spl}", rounds=False)
        assert a["mean_accept"] == b["mean_accept"]


# ----------------------------------------------------------------- 4. labels and rates
@pytest.mark.parametrize("kind,B,G", [("mog", 72, 3), ("gmm5", 8, 4), ("rw", 72, 2), ("mog", 128, 64)])
def test_labels_are_permutations_and_the_rate_is_the_mean(la, kind, B, G):
    smp = _sampler(la, kind)
    start = np.arange(B, dtype=np.int32).reshape(-1, G)[:, ::-1].reshape(-1).copy()       # every group reversed
    out = smp.run_hmc_exchange(STEPS, _x0(B, TOYS[kind][0]), temperature=_temps(B, G), replicas=G, replica0=start)
    rep, sw = out["replica"], out["swapped"]
    assert rep.shape == (STEPS, B)
    prev = start
    for t in range(STEPS):
        assert np.array_equal(np.sort(rep[t].reshape(-1, G), axis=1), np.arange(B).reshape(-1, G)), t
        low = lower_chains(B, G, t % 2)
        lower = np.zeros(B, dtype=bool)
        lower[low] = True
        assert not sw[t][~lower].any() and np.isnan(out["swap_p"][t][~lower]).all()
        assert np.isfinite(out["swap_p"][t][lower]).all()
        perm = np.arange(B)
        a = low[sw[t][low]]
        perm[a], perm[a + 1] = a + 1, a
        assert np.array_equal(rep[t], prev[perm]), t
        prev = rep[t]
    assert out["swap_rate"].shape == (G - 1,)
    assert np.array_equal(out["swap_rate"], sw.reshape(STEPS, B // G, G)[:, :, :G - 1].mean(axis=(0, 1)))
    assert sw.any()
    from l2hmc_amd import stats
    trips, per_group = stats.replica_round_trips(np.vstack([start[None], rep]), G)
    assert trips.shape == (B,) and per_group.shape == (B // G,) and per_group.sum() == trips.sum()


# ----------------------------------------------------------------- 5. launches
@pytest.mark.parametrize("kind,B", [("mog", 72), ("gmm5", 8)])
def test_the_exchange_run_is_one_launch_per_chunk_and_no_launch_per_round(la, kind, B):
    """Class 7: the toy-target run kernels, class 8: a round on its own."""
    x, n = _x0(B, TOYS[kind][0]), STEPS
    for G in (2, 4):
        temps = _temps(B, G)
        for k in (1, 5):
            for spl in (256, 3, 7):
                smp = _sampler(la, kind, spl)
                run = lambda: smp.run_hmc_exchange(n, x, temperature=temps, replicas=G, swap_every=k, first_parity=1)
                run()                                                # warm-up
                assert count_launches(7, run) == math.ceil(n / spl), (G, k, spl)
                assert count_launches(8, run) == 0, (G, k, spl)


@pytest.mark.parametrize("kind,B", [("mog", 72), ("gmm5", 8)])
def test_run_exchange_of_an_l2hmc_dynamics_is_the_loop_with_its_launches(la, kind, B):
    """`run_exchange`: values and draws of the loop `run(k, temperature=)`, `swap_replicas`; no launch of the run
    kernel spans a round or exceeds steps_per_launch, and every round with a pair is one launch."""
    x0, n = _x0(B, TOYS[kind][0]), STEPS
    exchanged = 0
    for G in (2, 4):
        for k in (1, 5):
            temps = _temps(B, G) if k == 1 else _temps(B, G, n)
            ref_smp = _sampler(la, kind, hmc=False)
            ref = _loop(ref_smp, n, temps, x0, G, k, first_parity=1)
            assert ref_smp.dynamics._draws == 4 + 4 * n + n // k
            for spl in (256, 3):
                what = f"{kind} B={B} G={G} swap_every={k} steps_per_launch={spl}"
                smp = _sampler(la, kind, spl, hmc=False)
                run = lambda: smp.run_exchange(n, x0, temperature=temps, replicas=G, swap_every=k, first_parity=1)
                out = run()
                _assert_same(out, ref, smp, ref_smp, what)
                assert np.array_equal(smp.replica.cpu().numpy(), out["replica"][-1]), what
                exchanged += int(out["swapped"].sum())
                want = (n // k) * math.ceil(k / spl) + math.ceil((n % k) / spl)
                assert count_launches(7, run) == want, what
                # parities 1, 0, 1, ...: with two rungs only the rounds of parity 0 have a pair
                parities = [(1 + r) % 2 for r in range(n // k)]
                assert count_launches(8, run) == sum(1 for p in parities if G > 2 or p == 0), what
    assert exchanged > 0


# ----------------------------------------------------------------- 6. the target stays invariant
def _report(name, zs, extra=""):
    zs = np.asarray(zs)
    k = np.unravel_index(np.argmax(np.abs(zs)), zs.shape)
    print(f"\n[invariance] {name}: max|z| = {np.abs(zs).max():.2f} (checkpoint {TR.CHECKPOINTS[k[0]]}, rung {k[1]}, "
          f"f{k[2]}) {extra}")
    return float(np.abs(zs).max())


def _ladder_sampler(la):
    dyn = la.Dynamics(2, la.Gaussian(TR.MU, TR.COV).get_energy_function(), trajectory_length=TR.HMC_N, eps=TR.HMC_EPS,
                      hmc=True, use_temperature=True, seed=5)
    assert not dyn.layered
    return la.DynamicsSampler(dyn)


def test_exchange_run_leaves_every_rung_invariant(la):
    t0 = time.time()
    G = len(TR.LADDER)
    x0, temps, exact = TR.ladder_start()
    smp = _ladder_sampler(la)
    x = torch.as_tensor(x0, dtype=torch.float32, device="cuda")
    zs, done, labels, rate, acc = [], 0, None, [], []
    for cp in TR.CHECKPOINTS:                                        # the run, continued from checkpoint to checkpoint
        out = smp.run_hmc_exchange(cp - done, x, keep_samples=False, temperature=temps[None, :], replicas=G,
                                   swap_every=1, first_parity=done % 2, replica0=labels)
        x, labels, done = out["samples_out"], out["replica"][-1], cp
        rate.append(out["swapped"].sum() / np.isfinite(out["swap_p"]).sum())        # per proposed pair
        acc.append(out["px"].mean())
        zs.append(TR.rung_zscores(x, exact))
    m = _report("toy HMC + replica exchange in the launch", zs,
                f"accept {np.mean(acc):.3f}, exchanges per pair and round {np.mean(rate):.3f}, {time.time() - t0:.1f} s")
    assert np.mean(rate) > 0.1
    assert m < Z_PASS, zs


@pytest.mark.parametrize("rule", ["sign_flipped", "always_accept"])
def test_exchange_power_controls(la, rule):
    """The same run with the round replaced by the torch restatement of a defect: the checks above can see one."""
    t0 = time.time()
    G = len(TR.LADDER)
    x0, temps, exact = TR.ladder_start()
    smp = _ladder_sampler(la)
    x = torch.as_tensor(x0, dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(31)
    zs = []
    for s in range(1, max(TR.CHECKPOINTS) + 1):
        x = smp.run_hmc(1, x, keep_samples=False, temperature=temps[None, :])["samples_out"]
        u = torch.rand(x.shape[0], dtype=torch.float64, device="cuda", generator=gen)
        x = TR.swap_round(x, temps, G, (s - 1) % 2, u, TR.energy64, rule)[0]
        if s in TR.CHECKPOINTS:
            zs.append(TR.rung_zscores(x, exact))
    m = _report(f"toy HMC + replica exchange defect={rule}", zs, f"{time.time() - t0:.1f} s")
    assert m > Z_DEFECT, zs
