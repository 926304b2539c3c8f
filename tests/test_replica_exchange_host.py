"""Host side of replica exchange between the rungs of a plain-HMC lattice ladder: the C entry
l2hmc_gauge_replica_swap (l2hmc_amd/csrc/replica_swap.hip) and its binding, the argument checks that fail before any
device call, what `GaugeSampler.run_hmc_exchange` / `swap_replicas` refuse, `stats.replica_round_trips` on hand-made
label histories, and the float64 restatement of the round (tests/replica_ref.py) against the exact finite-volume
distribution.  No GPU: arguments carry any non-NULL address where a pointer is checked and the sampler runs on stub
dynamics that must not be asked for a plan.

Invariance of the restatement: 4096 groups start as exact samples at each rung's beta (tests/invariance.py), 16 rounds
of alternating parity and no HMC in between; if the rule leaves the joint distribution invariant every rung still
holds exact samples, so the z-scores of I.U1_FEATURES per rung at rounds 1, 4 and 16 are N(0, 1).  Bars: max |z| < 5
for the correct rule, > 8 for each defect (Z_PASS / Z_DEFECT of tests/test_gpu_invariance.py).  Measured (seed 1),
4x4 / 2x4 / 8x8: correct 2.31 / 2.40 / 2.63; exponent sign flipped 1746 / 715 / 560; always accept 1284 / 1039 / 457;
mean swap rate of the proposed pairs 0.34 / 0.60 / 0.40.  About 2 s per ladder."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib, stats
from tests import replica_ref as R
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
Z_PASS, Z_DEFECT = 5.0, 8.0


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _swap(L, T=8, X=8, x=PTR, B=8, group=4, parity=0, betas=PTR, chain_stride=1):
    return L.l2hmc_gauge_replica_swap(T, X, x, B, group, parity, betas, chain_stride, 42, 3, None, None, None, None,
                                      None)


# ------------------------------------------------------------------------------------------------ the C entry
def test_header_declares_and_binding_matches():
    assert "l2hmc_gauge_replica_swap" in _lib.declared_symbols()
    # T, X, x, B, group, parity, betas, chain_stride, seed, stream_index, replica, action, swap_p, swapped, stream
    assert _lib._PROTOS["l2hmc_gauge_replica_swap"] == (
        C.c_int, [_I32, _I32, _P, _I64, _I32, _I32, _P, _I64, _U64, _U64, _P, _P, _P, _P, _P])
    text = header_text()
    assert ("int l2hmc_gauge_replica_swap(int32_t T, int32_t X, float* x, int64_t B, int32_t group, int32_t parity, "
            "const float* betas, int64_t chain_stride, uint64_t seed, uint64_t stream_index, int32_t* replica, "
            "float* action, float* swap_p, uint8_t* swapped, l2hmc_stream_t stream);") in text
    assert "#define L2HMC_ABI_VERSION 1" in text


def test_library_exports_the_entry(L):
    assert L.l2hmc_gauge_replica_swap is not None
    assert L.l2hmc_abi_version() == 1


def test_bad_arguments_fail_with_a_message_before_any_device_call(L):
    cases = [(dict(T=0), "bad lattice"), (dict(X=0), "bad lattice"), (dict(T=-2), "bad lattice"),
             (dict(X=-1), "bad lattice"), (dict(group=1), "group = 1"), (dict(group=0), "group = 0"),
             (dict(group=-4), "group = -4"), (dict(B=7), "not a multiple"), (dict(B=6, group=4), "not a multiple"),
             (dict(B=-8), "B < 0"), (dict(parity=2), "parity = 2"), (dict(parity=-1), "parity = -1"),
             (dict(chain_stride=-1), "negative stride"), (dict(x=None), "NULL x / betas"),
             (dict(betas=None), "NULL x / betas")]
    for kw, word in cases:
        rc = _swap(L, **kw)
        msg = L.l2hmc_last_error().decode()
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        assert msg.startswith("gauge_replica_swap: ") and word in msg, (kw, msg)
    with pytest.raises(ValueError, match="gauge_replica_swap: parity = 3"):
        _lib.check(_swap(L, parity=3))


def test_an_empty_batch_is_a_no_op(L):
    assert _swap(L, B=0) == 0
    assert _swap(L, B=0, x=None, betas=None) == 0
    assert _swap(L, B=0, group=2, parity=1, chain_stride=0) == 0
    assert _swap(L, B=0, T=33, X=32, group=5) == 0       # any lattice size: nothing caps the entry at 1024 sites
    assert _swap(L, B=0, group=1) == 1                    # checked before the batch size is looked at
    assert _swap(L, B=0, parity=2) == 1


# ------------------------------------------------------------------------------------------------ the sampler on stubs
T_, X_, B_ = 3, 5, 8
D_ = 2 * T_ * X_


def _stub(hmc=True):
    def _plan_():
        raise AssertionError("a refused call must not build a plan")
    lat = types.SimpleNamespace(time_size=T_, space_size=X_)
    return types.SimpleNamespace(hmc=hmc, lattice=lat, x_dim=D_, batch_size=B_, num_steps=3, eps=torch.tensor(0.1),
                                 _draws=4, _seed=7, _device=torch.device("cpu"), _plan=_plan_)


def _sampler(dyn):
    import l2hmc_amd as la
    return la.GaugeSampler(dyn)


def test_signatures():
    import l2hmc_amd as la
    assert (str(inspect.signature(la.GaugeSampler.run_hmc_exchange))
            == "(self, run_steps, beta, x=None, eps=None, keep_samples=False, replicas=None, swap_every=1, "
               "first_parity=0, replica0=None)")
    assert str(inspect.signature(la.GaugeSampler.swap_replicas)) == "(self, x, beta, replicas, parity)"
    assert str(inspect.signature(stats.replica_round_trips)) == "(replica, replicas)"


BETA = np.linspace(1.0, 4.5, B_)[None, :]


@pytest.mark.parametrize("kw", [dict(replicas=1), dict(replicas=0), dict(replicas=-2), dict(replicas=3),
                                dict(replicas=5), dict(replicas=16), dict(replicas=2.5),
                                dict(replicas=4, swap_every=0), dict(replicas=4, swap_every=-1),
                                dict(replicas=4, first_parity=2), dict(replicas=4, first_parity=-1),
                                dict(replicas=4, replica0=np.arange(B_)),                       # int64
                                dict(replicas=4, replica0=np.arange(B_, dtype=np.float32)),
                                dict(replicas=4, replica0=np.arange(B_ - 1, dtype=np.int32)),
                                dict(replicas=4, replica0=np.zeros((1, B_), dtype=np.int32)),
                                dict(replicas=4, replica0=torch.arange(B_))])                     # int64
def test_run_hmc_exchange_refuses(kw):
    dyn = _stub()
    with pytest.raises(ValueError, match="run_hmc_exchange: "):
        _sampler(dyn).run_hmc_exchange(5, BETA, torch.zeros(B_, D_), **kw)
    assert dyn._draws == 4


def test_run_hmc_exchange_refuses_an_l2hmc_dynamics():
    dyn = _stub(hmc=False)
    with pytest.raises(ValueError, match="`run`"):
        _sampler(dyn).run_hmc_exchange(5, BETA, torch.zeros(B_, D_), replicas=4)
    assert dyn._draws == 4


def test_run_hmc_exchange_accepts_good_arguments_up_to_the_plan():
    x0 = torch.zeros(B_, D_)
    for kw in (dict(), dict(replicas=None, swap_every=0, first_parity=7, replica0="ignored"), dict(replicas=2),
               dict(replicas=4, swap_every=3, first_parity=1), dict(replicas=8, replica0=np.arange(B_, dtype=np.int32)),
               dict(replicas=4, replica0=torch.arange(B_, dtype=torch.int32)), dict(replicas=np.int64(4))):
        dyn = _stub()
        with pytest.raises(AssertionError, match="must not build a plan"):
            _sampler(dyn).run_hmc_exchange(5, BETA, x0, **kw)
        assert dyn._draws == 4


def test_an_empty_exchange_run_returns_empty_histories():
    dyn = _stub()
    x0 = torch.ones(B_, D_)
    out = _sampler(dyn).run_hmc_exchange(0, BETA, x0, replicas=4)
    assert out["swap_p"].shape == (0, B_) and out["swap_p"].dtype == np.float32
    assert out["swapped"].shape == (0, B_) and out["swapped"].dtype == np.bool_
    assert out["replica"].shape == (0, B_) and out["replica"].dtype == np.int32
    assert out["swap_rate"].shape == (3,) and np.isnan(out["swap_rate"]).all()
    assert out["px"].shape == (0, B_) and torch.equal(out["samples_out"], x0) and dyn._draws == 4
    assert "swap_p" not in _sampler(dyn).run_hmc_exchange(0, BETA, x0)


@pytest.mark.parametrize("kw", [dict(replicas=1), dict(replicas=3), dict(parity=2), dict(parity=-1),
                                dict(beta=np.ones(B_ + 1)), dict(beta=2.0), dict(x=torch.zeros(B_, D_ + 1)),
                                dict(x=np.zeros((B_, D_)))])
def test_swap_replicas_refuses(kw):
    dyn = _stub()
    args = dict(x=torch.zeros(B_, D_), beta=BETA, replicas=4, parity=0)
    args.update(kw)
    with pytest.raises(ValueError, match="swap_replicas: "):
        _sampler(dyn).swap_replicas(**args)
    assert dyn._draws == 4


# ------------------------------------------------------------------------------------------------ round trips
def _history(G, paths):
    """paths[label] = the rung of the label after every round (one group) -> [n_r, G] label history."""
    n_r = len(paths[0])
    rep = np.empty((n_r, G), dtype=np.int32)
    for t in range(n_r):
        rungs = [p[t] for p in paths]
        assert sorted(rungs) == list(range(G))
        for label, r in enumerate(rungs):
            rep[t, r] = label
    return rep


def test_round_trips_on_hand_made_histories():
    # nobody moves: none
    rep = np.tile(np.arange(6, dtype=np.int32), (5, 1))
    trips, groups = stats.replica_round_trips(rep, 3)
    assert trips.tolist() == [0] * 6 and groups.tolist() == [0, 0] and trips.dtype == np.int64
    # G = 2: the two labels trade places every round.  Label 0: rungs 1 0 1 0 1 0 -> at the bottom after round 2, up,
    # down (1 trip), up, down (2 trips).  Label 1: rungs 0 1 0 1 0 1 -> up, down (1), up, down (2), up
    rep = _history(2, [[1, 0, 1, 0, 1, 0], [0, 1, 0, 1, 0, 1]])
    trips, groups = stats.replica_round_trips(rep, 2)
    assert trips.tolist() == [2, 2] and groups.tolist() == [4]
    # with the starting labels stacked on top label 0 is seen at the bottom from the start: one trip more
    trips, _ = stats.replica_round_trips(np.vstack([np.arange(2, dtype=np.int32)[None], rep]), 2)
    assert trips.tolist() == [3, 2]
    # a group of 3: label 0 walks 0 1 2 1 0 (one trip); label 1 is at the bottom after round 2, at the top after
    # round 4 and back after round 7 (one trip); label 2 starts at the top, which does not count without a visit to
    # the bottom before it, then goes down and up and never returns: none
    p0 = [0, 1, 2, 1, 0, 0, 1]
    p1 = [1, 0, 0, 2, 2, 1, 0]
    p2 = [2, 2, 1, 0, 1, 2, 2]
    trips, groups = stats.replica_round_trips(_history(3, [p0, p1, p2]), 3)
    assert trips.tolist() == [1, 1, 0] and groups.tolist() == [2]
    # two groups side by side count on their own: labels 3..5 of the second group stay put
    rep = np.hstack([_history(3, [p0, p1, p2]), np.tile(np.arange(3, 6, dtype=np.int32), (7, 1))])
    trips, groups = stats.replica_round_trips(rep, 3)
    assert trips.tolist() == [1, 1, 0, 0, 0, 0] and groups.tolist() == [2, 0]
    # two trips in a group of 3
    p0 = [0, 1, 2, 1, 0, 1, 2, 2, 1, 0]
    p1 = [1, 0, 0, 0, 1, 0, 0, 1, 2, 2]
    p2 = [2, 2, 1, 2, 2, 2, 1, 0, 0, 1]
    trips, groups = stats.replica_round_trips(_history(3, [p0, p1, p2]), 3)
    assert trips.tolist() == [2, 0, 0] and groups.tolist() == [2]
    # an empty history
    trips, groups = stats.replica_round_trips(np.empty((0, 6), dtype=np.int32), 3)
    assert trips.tolist() == [0] * 6 and groups.tolist() == [0, 0]


def test_round_trips_refuses_what_is_no_label_history():
    with pytest.raises(ValueError):
        stats.replica_round_trips(np.zeros((4, 6), dtype=np.int32), 3)        # no permutation
    with pytest.raises(ValueError):
        stats.replica_round_trips(np.array([[0, 3, 2, 1, 4, 5]], dtype=np.int32), 3)     # a label left its group
    with pytest.raises(ValueError):
        stats.replica_round_trips(np.arange(6, dtype=np.int32)[None], 4)
    with pytest.raises(ValueError):
        stats.replica_round_trips(np.arange(6, dtype=np.int32), 3)
    with pytest.raises(ValueError):
        stats.replica_round_trips(np.arange(6, dtype=np.int32)[None], 1)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_exchanges_exactly_the_accepted_pairs():
    T, X, G, B = 3, 5, 5, 10
    rng = np.random.default_rng(3)
    x = torch.as_tensor(rng.uniform(-7, 7, (B, 2 * T * X)))
    betas = rng.uniform(0.5, 5, B)
    for parity in (0, 1):
        u = rng.uniform(size=B)
        xn, p, sw, perm = R.swap_round(x, betas, G, parity, u, T, X)
        low = R.lower_chains(B, G, parity)
        assert low.tolist() == ([0, 2, 5, 7] if parity == 0 else [1, 3, 6, 8])
        off = np.setdiff1d(np.arange(B), low)
        assert np.isnan(p[off].numpy()).all() and not sw[off].any() and np.isfinite(p[low].numpy()).all()
        S = R.action64(x, T, X)[0].numpy()
        want = np.minimum(1.0, np.exp((betas[low] - betas[low + 1]) * (S[low] - S[low + 1])))
        assert np.allclose(p[low].numpy(), want, rtol=1e-14)
        assert np.array_equal(sw[low].numpy(), want > u[low])
        for a in low:
            if sw[a]:
                assert torch.equal(xn[a], x[a + 1]) and torch.equal(xn[a + 1], x[a])
            else:
                assert torch.equal(xn[a], x[a]) and torch.equal(xn[a + 1], x[a + 1])
        assert torch.equal(xn, x[perm]) and sorted(perm.tolist()) == list(range(B))


def _max_z(name, rule):
    T, X, ladder = R.LADDERS[name]
    G = len(ladder)
    x0, betas, exact = R.ladder_start(name)
    x = torch.as_tensor(x0)
    rng = np.random.default_rng(11)
    zs, rates = [], []
    for t in range(1, max(R.CHECKPOINTS) + 1):
        x, _, sw, _ = R.swap_round(x, betas, G, (t - 1) % 2, rng.uniform(size=x.shape[0]), T, X, rule)
        rates.append(float(sw[R.lower_chains(x.shape[0], G, (t - 1) % 2)].double().mean()))
        if t in R.CHECKPOINTS:
            zs.append(R.rung_zscores(x, T, X, G, exact))
    m = float(np.abs(np.array(zs)).max())
    print(f"\n[invariance] replica exchange restatement {name} rule={rule}: max|z| = {m:.2f}, "
          f"swap rate {np.mean(rates):.3f}")
    return m


@pytest.mark.parametrize("name", list(R.LADDERS))
def test_restatement_leaves_the_target_invariant_and_defects_do_not(name):
    assert _max_z(name, "correct") < Z_PASS
    assert _max_z(name, "sign_flipped") > Z_DEFECT
    assert _max_z(name, "always_accept") > Z_DEFECT
