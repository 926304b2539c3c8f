"""`GaugeSampler.run_exchange`: the trained L2HMC sampler with replica exchange between the rungs of a beta ladder.
It must be the hand-written loop `run(swap_every, ...)`, `swap_replicas(...)` on the dynamics' one draw counter, bit
for bit.  No statistical test here: a round is `swap_replicas`, whose invariance tests/test_gpu_replica_exchange.py
holds, and a step of a ladder is the uniform step bit for bit (tests/test_gpu_gauge_step_ladder.py)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.run_cases import assert_same_run

pytestmark = pytest.mark.gpu

HIST = ("px", "actions", "plaqs", "charges", "charge_diff")
TWO_PI = 2 * np.pi


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    return l2hmc_amd


_WEIGHTS = {}


def _dyn(T, X, N, eps, B, both=True):
    from oracle.gauge_dynamics import make_masks
    if (T, X) not in _WEIGHTS:
        _WEIGHTS[(T, X)] = H.gauge_weights(T, X, regime="init")
    xp, vp = _WEIGHTS[(T, X)]
    masks = make_masks(N, 2 * T * X, np.random.RandomState(42))
    return H.gauge_hip(T, X, N, eps, xp, vp, masks, B, both_directions=both)


def _x0(B, D, seed=33):
    # near-cold chains: neighbouring rungs then exchange with probabilities strictly between 0 and 1
    return torch.as_tensor(np.random.default_rng(seed).normal(0, 0.6, (B, D)) % TWO_PI, dtype=torch.float32,
                           device="cuda")


def _ladder(B, G, lo=1.0, hi=3.0):
    return np.tile(np.linspace(lo, hi, G), B // G)[None, :]                    # [1, B]


def _hand_loop(la, dyn, n, beta, x0, G, k, parity0=0, replica0=None):
    """run(k), swap_replicas, run(k), ... by hand on one sampler: the dictionary `run_exchange` must return."""
    smp = la.GaugeSampler(dyn)
    B = x0.shape[0]
    smp.replica = torch.as_tensor(np.arange(B, dtype=np.int32) if replica0 is None else replica0, device="cuda")
    beta = np.asarray(beta, dtype=np.float64)
    x, s, j = x0, 0, 0
    parts, rounds = [], {"swap_p": [], "swapped": [], "replica": []}
    while s < n:
        m = min(k, n - s)
        o = smp.run(m, beta if beta.shape[0] == 1 else beta[s:s + m], x, keep_samples=True)
        parts.append(o)
        x, s = o["samples_out"], s + m
        if s % k == 0:
            p, sw, _ = smp.swap_replicas(x, beta[0] if beta.shape[0] == 1 else beta[s - 1], G, (parity0 + j) % 2)
            j += 1
            rounds["swap_p"].append(p.cpu().numpy())
            rounds["swapped"].append(sw.cpu().numpy().astype(np.bool_))
            rounds["replica"].append(smp.replica.cpu().numpy())
    out = {key: np.concatenate([o[key] for o in parts]) for key in HIST + ("samples",)}
    out["samples_out"], out["mean_accept"] = x, parts[-1]["mean_accept"]
    for key, dtype in (("swap_p", np.float32), ("swapped", np.bool_), ("replica", np.int32)):
        out[key] = np.stack(rounds[key]).astype(dtype) if rounds[key] else np.empty((0, B), dtype=dtype)
    return out, smp


def _assert_same_exchange(got, want, what):
    assert_same_run(got, want, HIST + ("samples",), what)
    assert got["swap_p"].dtype == np.float32 and got["swapped"].dtype == np.bool_ and got["replica"].dtype == np.int32
    assert np.array_equal(got["swap_p"], want["swap_p"], equal_nan=True), what
    assert np.array_equal(got["swapped"], want["swapped"]) and np.array_equal(got["replica"], want["replica"]), what


def _check_rounds(out, B, G, n_r):
    assert out["swap_p"].shape == out["swapped"].shape == out["replica"].shape == (n_r, B)
    for row in out["replica"]:                             # labels are permutations within groups
        assert np.array_equal(np.sort(row.reshape(B // G, G), axis=1), np.arange(B).reshape(B // G, G))
    sw = out["swapped"].reshape(n_r, B // G, G)[:, :, :G - 1]
    assert out["swap_rate"].shape == (G - 1,)
    assert np.array_equal(out["swap_rate"], sw.mean(axis=(0, 1)))
    assert not out["swapped"].reshape(n_r, B // G, G)[:, :, G - 1].any()
    p = out["swap_p"][np.isfinite(out["swap_p"])]
    assert p.size and (p >= 0).all() and (p <= 1).all()


@pytest.mark.parametrize("both", [True, False], ids=["both", "selected"])
@pytest.mark.parametrize("k", [1, 3])
def test_run_exchange_is_the_hand_written_loop_on_a_whole_step_plan(la, both, k):
    B, G, n = 72, 4, 7                                     # n is no multiple of k = 3: the run ends on plain steps
    dyn = _dyn(8, 8, 2, 0.2, B, both=both)
    x0, beta = _x0(B, 128), _ladder(B, G)
    dyn._draws = 40
    want, hand = _hand_loop(la, dyn, n, beta, x0, G, k, parity0=1)
    draws = dyn._draws
    dyn._draws = 40
    smp = la.GaugeSampler(dyn)
    got = smp.run_exchange(n, beta, x0, keep_samples=True, replicas=G, swap_every=k, first_parity=1)
    assert dyn._draws == draws
    _assert_same_exchange(got, want, (both, k))
    assert torch.equal(smp.replica, hand.replica)
    _check_rounds(got, B, G, n // k)
    assert got["swapped"].any() and not got["swapped"].all()          # rounds that exchange and rounds that do not
    assert got["plaq_exact"].shape == (B,)


def test_a_schedule_with_a_chain_axis_and_the_layer_by_layer_plan(la):
    """6 x 6 has no whole-step kernel; beta [n, B]: a round runs at the betas of the step before it."""
    B, G, n, k = 24, 3, 5, 2
    dyn = _dyn(6, 6, 2, 0.2, B)
    x0 = _x0(B, 72)
    beta = np.linspace(1.0, 1.5, n)[:, None] * _ladder(B, G)                   # [n, B]
    dyn._draws = 40
    want, hand = _hand_loop(la, dyn, n, beta, x0, G, k)
    draws = dyn._draws
    dyn._draws = 40
    smp = la.GaugeSampler(dyn)
    got = smp.run_exchange(n, beta, x0, keep_samples=True, replicas=G, swap_every=k)
    assert dyn._draws == draws
    _assert_same_exchange(got, want, "6x6")
    assert torch.equal(smp.replica, hand.replica)
    _check_rounds(got, B, G, n // k)


def test_two_halves_continue_to_the_whole_run(la):
    B, G, k, n1, n2 = 72, 4, 3, 6, 5
    dyn = _dyn(8, 8, 2, 0.2, B)
    x0, beta = _x0(B, 128), _ladder(B, G)
    dyn._draws = 40
    whole = la.GaugeSampler(dyn).run_exchange(n1 + n2, beta, x0, keep_samples=True, replicas=G, swap_every=k,
                                              first_parity=1)
    draws = dyn._draws
    dyn._draws = 40
    smp = la.GaugeSampler(dyn)
    a = smp.run_exchange(n1, beta, x0, keep_samples=True, replicas=G, swap_every=k, first_parity=1)
    b = smp.run_exchange(n2, beta, a["samples_out"], keep_samples=True, replicas=G, swap_every=k,
                         first_parity=(1 + n1 // k) % 2, replica0=a["replica"][-1])
    assert dyn._draws == draws
    for key in HIST + ("samples", "swap_p", "swapped", "replica"):
        assert np.array_equal(np.concatenate([a[key], b[key]]), whole[key], equal_nan=True), key
    assert torch.equal(b["samples_out"], whole["samples_out"])
    assert b["mean_accept"] == whole["mean_accept"]


@pytest.mark.parametrize("both", [True, False], ids=["both", "selected"])
def test_without_replicas_it_is_run(la, both):
    B, n = 36, 3
    dyn = _dyn(8, 8, 2, 0.2, B, both=both)
    x0 = _x0(B, 128)
    for beta in (_ladder(B, 4), 2.0, [1.0, 2.0, 3.0]):
        dyn._draws = 40
        want = la.GaugeSampler(dyn).run(n, beta, x0, keep_samples=True)
        draws = dyn._draws
        dyn._draws = 40
        got = la.GaugeSampler(dyn).run_exchange(n, beta, x0, keep_samples=True, swap_every=2, first_parity=1)
        assert dyn._draws == draws
        assert_same_run(got, want, HIST + ("samples",), "replicas=None")
        assert "swap_p" not in got and np.array_equal(got["plaq_exact"], want["plaq_exact"])


def _bits(values):
    """The tensors of a tuple (dictionaries of tensors among them), in order, as integer arrays: NaN equals itself."""
    flat = []
    for v in values:
        for t in ([v[key] for key in sorted(v)] if isinstance(v, dict) else [v]):
            flat.append((t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().numpy())
    return flat


def _assert_device_ladders_are_the_host_ladder(call, ladder, what):
    """`call(ladder)` -> tensors; as a float32 device tensor [B] and [1, B] the ladder stays where it is and gives the
    bits the NumPy array gives; [B, 1] has B elements too and is none of the documented shapes."""
    want = _bits(call(ladder))
    on_device = torch.as_tensor(ladder, dtype=torch.float32, device="cuda")
    for shaped in (on_device, on_device[None, :]):
        got = _bits(call(shaped))
        assert len(got) == len(want) >= 4
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (what, tuple(shaped.shape))
    with pytest.raises(ValueError, match=f"{what}: .* of shape \\({ladder.size}, 1\\): expected"):
        call(on_device[:, None])


def test_a_ladder_on_the_device_is_the_same_ladder_from_the_host(la):
    """`step` and the `swap_replicas` of both samplers, 8 chains in groups of 4 rungs: a 4 x 4 lattice and a mixture of
    two Gaussians in 2 dimensions."""
    from oracle import dynamics as od
    from tests import toy_cases as tc
    B, G = 8, 4
    dyn = _dyn(4, 4, 2, 0.2, B)
    smp, x0, beta = la.GaugeSampler(dyn), _x0(B, 32), _ladder(B, G)[0]
    labels = torch.arange(B, dtype=torch.int32, device="cuda")

    def step(b):
        dyn._draws = 40
        return smp.step(x0, b)

    def swap(sampler, start):
        def call(values):
            sampler.dynamics._draws, sampler.replica, x = 40, labels.clone(), start.clone()
            return (x, sampler.replica, *sampler.swap_replicas(x, values, G, 0))
        return call

    _assert_device_ladders_are_the_host_ladder(step, beta, "step")
    _assert_device_ladders_are_the_host_ladder(swap(smp, x0), beta, "swap_replicas")
    assert swap(smp, x0)(beta)[3].any()                    # (a round that exchanges something)

    toy = la.Dynamics(2, tc.target(2, 2, tc.M)[1].get_energy_function(), trajectory_length=3, eps=0.1,
                      use_temperature=True, seed=7, hmc=True)
    toy.set_masks(od.make_masks(3, 2, np.random.RandomState(3)))
    points = torch.as_tensor(tc.target_points(2, 2, tc.M, B)[0], dtype=torch.float32, device="cuda")
    temps = np.tile(np.linspace(0.5, 4.0, G), B // G)
    _assert_device_ladders_are_the_host_ladder(swap(la.DynamicsSampler(toy), points), temps, "swap_replicas")
