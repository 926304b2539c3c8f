"""Replica exchange inside a plain-HMC ladder run: `GaugeSampler.run_hmc_exchange(..., replicas=G, swap_every=k)` and
`GaugeSampler.swap_replicas` (l2hmc_gauge_replica_swap between launches of l2hmc_gauge_hmc_run_ladder).

The round itself is held to float64 in tests/test_gpu_replica_swap.py and the run without exchange in
tests/test_gpu_hmc_run_ladder.py; what is new here is how they are put together, so the yardstick is the loop a caller
would write -- `run_hmc(k, ...)`, then `swap_replicas(...)` with the right parity, on a second dynamics of the same seed
-- and every comparison with it is an equality.  The target is the other yardstick: 4096 groups of exact samples at
every rung stay exact under HMC steps with a round after each.

Measured on the MI355X (max |z| over rungs, checkpoints and test functions; `_report`'s lines):
  exchange run, swap_every = 1:  4x4 2.47, 8x8 1.75  (HMC accept 0.97 / 0.92, 0.55 / 0.64 exchanges per group and
  round);  0.3 s per case.
  round replaced by the torch restatement of a defect (4x4 / 8x8):  exponent sign flipped 234 / 142, always accept
  208 / 121."""
import math
import time

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import replica_ref as R
from tests.run_cases import count_launches

pytestmark = pytest.mark.gpu

N_LF, EPS, STEPS = 3, 0.1, 12
SHAPES = [(3, 5, 8), (8, 8, 72), (16, 16, 6), (32, 32, 4)]
HIST = ("px", "actions", "plaqs", "charges", "charge_diff")
ROUNDS = ("swap_p", "swapped", "replica")
EPSS = (0.05, 0.1, 0.2)
Z_PASS, Z_DEFECT = 5.0, 8.0          # tests/test_gpu_invariance.py


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _sampler(la, T, X, B, both=True, spl=256, draws=4):
    orc = H.gauge_oracle(T, X, N_LF, EPS, None, None, hmc=True)
    dyn = H.gauge_hip(T, X, N_LF, EPS, None, None, orc.mask, B, hmc=True, both_directions=both)
    dyn._draws = draws
    smp = la.GaugeSampler(dyn)
    smp.steps_per_launch = spl
    return smp


def _x0(T, X, B):
    torch.manual_seed(1234)
    return torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)


def _groups(B):
    return [G for G in (2, 3, 4) if B % G == 0]


def _betas(B, G, n=None):
    """[1, B] ladder from 1 to 4 over the rungs of every group, or [n, B]: the ladder scaled a little from step to step"""
    lad = np.tile(np.linspace(1.0, 4.0, G), B // G)[None, :]
    return lad if n is None else lad * (1.0 + 0.02 * np.arange(n))[:, None]


def _loop(smp, n, beta, x, eps, G, k, first_parity=0):
    """What `run_hmc_exchange(n, beta, x, eps, True, G, k, first_parity)` has to be: run_hmc(k), swap_replicas, ..."""
    B = x.shape[0]
    beta = np.asarray(beta)
    smp.replica = torch.arange(B, dtype=torch.int32, device="cuda")
    parts, rounds, s = [], {r: [] for r in ROUNDS}, 0
    while s < n:
        m = min(k, n - s)
        o = smp.run_hmc(m, beta if beta.shape[0] == 1 else beta[s:s + m], x, eps=eps, keep_samples=True)
        parts.append(o)
        x = o["samples_out"]
        s += m
        if s % k == 0:
            p, sw, _ = smp.swap_replicas(x, beta[0 if beta.shape[0] == 1 else s - 1], G, (first_parity + s // k - 1) % 2)
            rounds["swap_p"].append(p.cpu().numpy())
            rounds["swapped"].append(sw.cpu().numpy())
            rounds["replica"].append(smp.replica.cpu().numpy().copy())
    out = {key: np.concatenate([o[key] for o in parts]) for key in HIST + ("samples",)}
    out.update({r: np.stack(v) if v else np.empty((0, B)) for r, v in rounds.items()})
    out["samples_out"], out["mean_accept"] = x, parts[-1]["mean_accept"]
    return out


def _assert_same(a, b, sa, sb, what, rounds=True):
    for key in HIST + ("samples",) + (ROUNDS if rounds else ()):
        assert a[key].shape == b[key].shape, (what, key)
        assert np.array_equal(a[key], b[key], equal_nan=(key == "swap_p")), (what, key)
    assert torch.equal(a["samples_out"], b["samples_out"]), what
    assert a["mean_accept"] == b["mean_accept"], what
    assert torch.equal(sa.stats.total, sb.stats.total), what
    assert sa.dynamics._draws == sb.dynamics._draws, what


# ----------------------------------------------------------------- 1. the run is the loop a caller would write
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", SHAPES)
def test_exchange_run_is_run_hmc_then_swap_replicas(la, T, X, B, both):
    x0 = _x0(T, X, B)
    keep = x0.clone()
    eps = np.array(EPSS)[np.arange(B) % 3]
    exchanged = 0
    for G in _groups(B):
        for k in (1, 5):
            beta = _betas(B, G) if k == 1 else _betas(B, G, STEPS)       # a ladder; a ladder with a schedule
            ref_smp = _sampler(la, T, X, B, both)
            ref = _loop(ref_smp, STEPS, beta, x0, eps, G, k)
            for spl in (256, 3):
                what = f"{T}x{X} B={B} both={both} G={G} swap_every={k} steps_per_launch={spl}"
                smp = _sampler(la, T, X, B, both, spl)
                out = smp.run_hmc_exchange(STEPS, beta, x0, eps=eps, keep_samples=True, replicas=G, swap_every=k)
                assert out["swap_p"].shape == (STEPS // k, B) and out["swap_p"].dtype == np.float32, what
                assert out["swapped"].dtype == np.bool_ and out["replica"].dtype == np.int32, what
                _assert_same(out, ref, smp, ref_smp, what)
                assert np.array_equal(smp.replica.cpu().numpy(), out["replica"][-1]), what
                exchanged += int(out["swapped"].sum())
    assert torch.equal(x0, keep)                                     # the caller's x is not advanced in place
    assert exchanged > 0


# ----------------------------------------------------------------- 2. a run continues
@pytest.mark.parametrize("T,X,B,G", [(3, 5, 8, 4), (8, 8, 72, 3), (32, 32, 4, 2)])
def test_two_halves_are_the_whole(la, T, X, B, G):
    x0, beta = _x0(T, X, B), _betas(B, G)
    for k, n in ((1, 3), (2, 6), (5, 5)):
        for fp in (0, 1):
            whole_smp, smp = _sampler(la, T, X, B), _sampler(la, T, X, B)
            whole = whole_smp.run_hmc_exchange(2 * n, beta, x0, keep_samples=True, replicas=G, swap_every=k,
                                               first_parity=fp)
            a = smp.run_hmc_exchange(n, beta, x0, keep_samples=True, replicas=G, swap_every=k, first_parity=fp)
            b = smp.run_hmc_exchange(n, beta, a["samples_out"], keep_samples=True, replicas=G, swap_every=k,
                                     first_parity=(fp + n // k) % 2, replica0=a["replica"][-1])
            both = {key: np.concatenate([a[key], b[key]]) for key in HIST + ("samples",) + ROUNDS}
            both["samples_out"], both["mean_accept"] = b["samples_out"], b["mean_accept"]
            _assert_same(whole, both, whole_smp, smp, f"{T}x{X} G={G} swap_every={k} first_parity={fp}")


# ----------------------------------------------------------------- 3. no exchange asked for
@pytest.mark.parametrize("T,X,B", [(8, 8, 72), (32, 32, 4)])
def test_without_replicas_it_is_run_hmc(la, T, X, B):
    x0, beta = _x0(T, X, B), _betas(B, 2, STEPS)
    eps = np.array(EPSS)[np.arange(B) % 3]
    for spl in (256, 5):
        sa, sb = _sampler(la, T, X, B, spl=spl), _sampler(la, T, X, B, spl=spl)
        a = sa.run_hmc(STEPS, beta, x0, eps=eps, keep_samples=True)
        b = sb.run_hmc_exchange(STEPS, beta, x0, eps=eps, keep_samples=True, replicas=None, swap_every=0,
                                first_parity=5, replica0="ignored")
        assert set(a) == set(b) and "swap_p" not in b and sb.replica is None
        _assert_same(a, b, sa, sb, f"{T}x{X} steps_per_launch={spl}", rounds=False)


# ----------------------------------------------------------------- 4. labels and rates
@pytest.mark.parametrize("T,X,B,G", [(3, 5, 8, 4), (8, 8, 72, 3), (8, 8, 72, 2)])
def test_labels_are_permutations_and_the_rate_is_the_mean(la, T, X, B, G):
    smp = _sampler(la, T, X, B)
    start = np.arange(B, dtype=np.int32).reshape(-1, G)[:, ::-1].reshape(-1).copy()       # every group reversed
    out = smp.run_hmc_exchange(STEPS, _betas(B, G), _x0(T, X, B), replicas=G, replica0=start)
    rep, sw = out["replica"], out["swapped"]
    assert rep.shape == (STEPS, B)
    prev = start
    for t in range(STEPS):
        assert np.array_equal(np.sort(rep[t].reshape(-1, G), axis=1), np.arange(B).reshape(-1, G)), t
        low = R.lower_chains(B, G, t % 2)
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
@pytest.mark.parametrize("T,X,B", [(8, 8, 72), (32, 32, 4)])
def test_one_run_launch_per_chunk_and_one_swap_launch_per_round_with_a_pair(la, T, X, B):
    """No launch of the run kernel spans a round or exceeds steps_per_launch: between two rounds (k steps, and the
    n % k steps after the last) that is ceil(steps / steps_per_launch) launches.  Class 5: the run kernel, class 8: the
    round."""
    x, n = _x0(T, X, B), STEPS
    for G in (2, 4):
        beta = _betas(B, G)
        for k in (1, 5):
            for spl in (256, 3):
                smp = _sampler(la, T, X, B, spl=spl)
                run = lambda: smp.run_hmc_exchange(n, beta, x, replicas=G, swap_every=k, first_parity=1)
                run()                                                # warm-up
                want = (n // k) * math.ceil(k / spl) + math.ceil((n % k) / spl)
                assert count_launches(5, run) == want, (G, k, spl)
                # parities 1, 0, 1, ...: with two rungs only the rounds of parity 0 have a pair
                parities = [(1 + r) % 2 for r in range(n // k)]
                assert count_launches(8, run) == sum(1 for p in parities if G > 2 or p == 0), (G, k, spl)
                assert count_launches(4, run) == 0
                assert count_launches(8, lambda: smp.run_hmc(n, beta, x)) == 0


# ----------------------------------------------------------------- 6. the target stays invariant
def _report(name, zs, extra=""):
    zs = np.asarray(zs)
    k = np.unravel_index(np.argmax(np.abs(zs)), zs.shape)
    print(f"\n[invariance] {name}: max|z| = {np.abs(zs).max():.2f} (checkpoint {R.CHECKPOINTS[k[0]]}, rung {k[1]}, "
          f"f{k[2]}) {extra}")
    return float(np.abs(zs).max())


def _ladder_sampler(la, name):
    """HMC with eps 0.1 and 5 leapfrog steps, the dynamics built as tests/test_gpu_invariance.py builds its own"""
    T, X, ladder = R.LADDERS[name]
    B = R.GROUPS * len(ladder)
    lat = la.GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    dyn = la.GaugeDynamics(lat, lat.get_energy_function(), eps=0.1, hmc=True, num_steps=5, eps_trainable=False,
                           network_arch='generic', both_directions=True, seed=5)
    return la.GaugeSampler(dyn)


@pytest.mark.parametrize("name", ["4x4", "8x8"])
def test_exchange_run_leaves_every_rung_invariant(la, name):
    t0 = time.time()
    T, X, ladder = R.LADDERS[name]
    G = len(ladder)
    x0, betas, exact = R.ladder_start(name)
    smp = _ladder_sampler(la, name)
    x = torch.as_tensor(x0, dtype=torch.float32, device="cuda")
    zs, done, labels, rate, acc = [], 0, None, [], []
    for cp in R.CHECKPOINTS:                                         # the run, continued from checkpoint to checkpoint
        out = smp.run_hmc_exchange(cp - done, betas[None, :], x, replicas=G, swap_every=1, first_parity=done % 2,
                                   replica0=labels)
        x, labels, done = out["samples_out"], out["replica"][-1], cp
        rate.append(out["swapped"].sum() / (out["swapped"].shape[0] * R.GROUPS))
        acc.append(out["px"].mean())
        zs.append(R.rung_zscores(x, T, X, G, exact))
    assert float(x.min()) >= 0 and float(x.max()) <= 2 * np.pi
    m = _report(f"U(1) HMC + replica exchange {name}", zs,
                f"accept {np.mean(acc):.3f}, exchanges per group and round {np.mean(rate):.3f}, {time.time() - t0:.1f} s")
    assert np.mean(rate) > 0.1
    assert m < Z_PASS, zs


@pytest.mark.parametrize("rule", ["sign_flipped", "always_accept"])
@pytest.mark.parametrize("name", ["4x4", "8x8"])
def test_exchange_power_controls(la, name, rule):
    """The same run with the round replaced by the torch restatement of a defect: the checks above can see one."""
    t0 = time.time()
    T, X, ladder = R.LADDERS[name]
    G = len(ladder)
    x0, betas, exact = R.ladder_start(name)
    smp = _ladder_sampler(la, name)
    x = torch.as_tensor(x0, dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(31)
    zs = []
    for s in range(1, max(R.CHECKPOINTS) + 1):
        x = smp.run_hmc(1, betas[None, :], x)["samples_out"]
        u = torch.rand(x.shape[0], dtype=torch.float64, device="cuda", generator=gen)
        x = R.swap_round(x, betas, G, (s - 1) % 2, u, T, X, rule)[0]
        if s in R.CHECKPOINTS:
            zs.append(R.rung_zscores(x, T, X, G, exact))
    m = _report(f"U(1) HMC + replica exchange {name} defect={rule}", zs, f"{time.time() - t0:.1f} s")
    assert m > Z_DEFECT, zs
