"""Host side of replica exchange between the rungs of a toy-target temperature ladder: the C entries
l2hmc_small_replica_swap and l2hmc_small_hmc_run_exchange (l2hmc_amd/csrc/small_hmc.hip, small_swap.h) and their
bindings, the argument checks that fail before any device call, what `DynamicsSampler.run_hmc_exchange`,
`swap_replicas` and `run_exchange` refuse, and the float64 restatement of the round (tests/toy_replica_ref.py) against
the exact tempered Gaussians.  No GPU: arguments carry any non-NULL address where a pointer is checked and the sampler
runs on stub dynamics that must not be asked for a plan.

Invariance of the restatement: 4096 groups start as exact samples of N(0, T [[1, .6], [.6, 1]]) at T = 1, 2, 4, 8;
every step is one float64 HMC step (eps 0.3, 5 leapfrog steps) at the column's temperature and then one round, parities
alternating; if the rule leaves the joint distribution invariant every rung still holds exact samples, so the z-scores
per rung (means, second moments, half-space indicators, U) at steps 1, 4 and 16 are N(0, 1).  Bars: max |z| < 5 for the
correct rule, > 8 for each defect (Z_PASS / Z_DEFECT of tests/test_gpu_invariance.py).  Measured here (seed 1):
correct 3.46, exponent sign flipped 108.75, always accept 78.16, swap rate of the proposed pairs 0.667.  About 1 s."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib, stats
from tests import toy_replica_ref as TR
from tests.replica_ref import lower_chains
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
Z_PASS, Z_DEFECT = 5.0, 8.0


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _target(dim=2, K=1, kind=1, temperature=1.0, mu=PTR):
    return _lib.MogTarget(dim=dim, K=K, is_gaussian=kind, temperature=temperature, mu=mu, prec=PTR, log_const=PTR)


def _plan(x_dim=2, hmc=1, N=5, masks=PTR, target=None):
    return _lib.SmallPlan(x_dim=x_dim, num_nodes=0, trajectory_length=N, hmc=hmc, eps=0.1, first_layer_form=0,
                          masks=masks, target=target if target is not None else _target())


def _swap(L, plan, x=PTR, B=8, group=4, parity=0, temps=PTR, chain_stride=1):
    return L.l2hmc_small_replica_swap(None if plan is None else C.byref(plan), x, B, group, parity, temps, chain_stride,
                                      42, 3, None, None, None, None, None)


def _run(L, plan, x_in=PTR, x_next=PTR, B=8, draw0=0, n_steps=3, temps=PTR, step_stride=0, chain_stride=1,
         eps_chain=None, group=4, swap_every=1, swap_phase=0, first_parity=0):
    return L.l2hmc_small_hmc_run_exchange(None if plan is None else C.byref(plan), x_in, x_next, B, 42, draw0, n_steps,
                                          temps, step_stride, chain_stride, eps_chain, group, swap_every, swap_phase,
                                          first_parity, None, None, None, None, None, None, None)


# ------------------------------------------------------------------------------------------------ the C entries
def test_header_declares_and_bindings_match():
    assert {"l2hmc_small_replica_swap", "l2hmc_small_hmc_run_exchange"} <= set(_lib.declared_symbols())
    # plan, x, B, group, parity, temps, chain_stride, seed, stream_index, replica, energy, swap_p, swapped, stream
    assert _lib._PROTOS["l2hmc_small_replica_swap"] == (
        C.c_int, [C.POINTER(_lib.SmallPlan), _P, _I64, _I32, _I32, _P, _I64, _U64, _U64, _P, _P, _P, _P, _P])
    # plan, x_in, x_next, B, seed, draw0, n_steps, temps, step_stride, chain_stride, eps_chain, group, swap_every,
    # swap_phase, first_parity, replica, px, samples, swap_p, swapped, replica_hist, stream
    assert _lib._PROTOS["l2hmc_small_hmc_run_exchange"] == (
        C.c_int, [C.POINTER(_lib.SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _I64, _I64, _P, _I32, _I32, _I32, _I32,
                  _P, _P, _P, _P, _P, _P, _P])
    text = header_text()
    assert ("int l2hmc_small_replica_swap(const l2hmc_small_plan* plan, float* x, int64_t B, int32_t group, "
            "int32_t parity, const float* temps, int64_t chain_stride, uint64_t seed, uint64_t stream_index, "
            "int32_t* replica, float* energy, float* swap_p, uint8_t* swapped, l2hmc_stream_t stream);") in text
    assert ("int l2hmc_small_hmc_run_exchange(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B, "
            "uint64_t seed, uint64_t draw0, int32_t n_steps, const float* temps, int64_t step_stride, "
            "int64_t chain_stride, const float* eps_chain, int32_t group, int32_t swap_every, int32_t swap_phase, "
            "int32_t first_parity, int32_t* replica, float* px, float* samples, float* swap_p, uint8_t* swapped, "
            "int32_t* replica_hist, l2hmc_stream_t stream);") in text
    assert "#define L2HMC_ABI_VERSION 1" in text
    assert "l2hmc_small_replica_swap" in header_text(comments=True).split("int l2hmc_profile_begin")[0].rsplit("8 =", 1)[1]


def test_library_exports_the_entries(L):
    assert L.l2hmc_small_replica_swap is not None and L.l2hmc_small_hmc_run_exchange is not None
    assert L.l2hmc_abi_version() == 1


TARGET_REFUSALS = [(dict(x_dim=3), "x_dim=3 != target dim=2"),
                   (dict(x_dim=9, target=_target(dim=9)), "target dim=9 (max 8)"),
                   (dict(target=_target(K=9)), "K=9 (max 8)"),
                   (dict(target=_target(kind=4)), "target kind 4 unknown"),
                   (dict(target=_target(temperature=0.0)), "temperature must be > 0"),
                   (dict(target=_target(mu=None)), "NULL parameter pointer"),
                   (dict(target=_target(kind=3, dim=1), x_dim=1), "funnel target needs dim >= 2")]


def test_the_round_refuses_bad_arguments_before_any_device_call(L):
    ok = _plan()
    cases = [(dict(plan=None), "plan is NULL"), (dict(x=None), "NULL x / temps"), (dict(temps=None), "NULL x / temps"),
             (dict(group=1), "group = 1"), (dict(group=0), "group = 0"), (dict(group=-4), "group = -4"),
             (dict(group=65, B=130), "group = 65"), (dict(B=7), "not a multiple"),
             (dict(B=6, group=4), "not a multiple"), (dict(B=-8), "B < 0"), (dict(parity=2), "parity = 2"),
             (dict(parity=-1), "parity = -1"), (dict(chain_stride=-1), "negative stride")]
    cases += [(dict(plan=_plan(**kw)), word) for kw, word in TARGET_REFUSALS]
    for kw, word in cases:
        plan = kw.pop("plan", ok)
        rc = _swap(L, plan, **kw)
        msg = L.l2hmc_last_error().decode()
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        assert msg.startswith("small_replica_swap: ") and word in msg, (kw, msg)
    with pytest.raises(ValueError, match="small_replica_swap: parity = 3"):
        _lib.check(_swap(L, ok, parity=3))


def test_the_round_serves_any_plan_with_a_packed_target_and_an_empty_batch_is_a_no_op(L):
    # of the plan only x_dim and the target are read: an L2HMC plan, no masks, no trajectory
    for plan in (_plan(), _plan(hmc=0), _plan(masks=None, N=0)):
        assert _swap(L, plan, B=0) == 0
        assert _swap(L, plan, B=0, x=None, temps=None) == 0
        assert _swap(L, plan, B=0, group=2, parity=1, chain_stride=0) == 0
        assert _swap(L, plan, B=0, group=64) == 0
    assert _swap(L, _plan(), B=0, group=1) == 1            # checked before the batch size is looked at
    assert _swap(L, _plan(), B=0, parity=2) == 1
    assert _swap(L, _plan(target=_target(K=9)), B=0) == 1


def test_the_run_refuses_bad_arguments_before_any_device_call(L):
    ok = _plan()
    cases = [(dict(plan=None), "plan is NULL"), (dict(x_in=None), "x_in / x_next is NULL"),
             (dict(x_next=None), "x_in / x_next is NULL"), (dict(B=-8), "B < 0"),
             (dict(n_steps=0), "n_steps=0"), (dict(n_steps=-1), "n_steps=-1"),
             (dict(plan=_plan(hmc=0)), "L2HMC sampler"),
             (dict(step_stride=-1), "negative stride"), (dict(chain_stride=-1), "negative stride"),
             (dict(plan=_plan(N=0)), "bad trajectory_length / masks"),
             (dict(plan=_plan(masks=None)), "bad trajectory_length / masks"),
             (dict(temps=None), "temps is NULL"),
             (dict(group=1), "group = 1"), (dict(group=0), "group = 0"), (dict(group=65, B=130), "group = 65"),
             (dict(B=7), "not a multiple"), (dict(B=6), "not a multiple"),
             (dict(swap_every=0), "swap_every = 0"), (dict(swap_every=-2), "swap_every = -2"),
             (dict(swap_phase=-1), "swap_phase = -1"), (dict(swap_phase=1), "swap_phase = 1"),
             (dict(swap_every=3, swap_phase=3), "swap_phase = 3"),
             (dict(first_parity=2), "first_parity = 2"), (dict(first_parity=-1), "first_parity = -1"),
             (dict(draw0=2 ** 64 - 4, n_steps=2), "overflows 64 bits"),
             # 2 * 3 steps fit below 2^64 - 1, their three rounds do not
             (dict(draw0=2 ** 64 - 9, n_steps=3), "draw0 + 2 * n_steps + rounds overflows")]
    cases += [(dict(plan=_plan(**kw)), word) for kw, word in TARGET_REFUSALS]
    for kw, word in cases:
        plan = kw.pop("plan", ok)
        rc = _run(L, plan, **kw)
        msg = L.l2hmc_last_error().decode()
        assert rc == 1, (kw, rc)
        assert msg.startswith("small_hmc_run_exchange: ") and word in msg, (kw, msg)


def test_a_round_takes_its_stream_whatever_the_group(L):
    """3 steps with a round after each take streams draw0 .. draw0 + 8, group 2 (a round without a pair) included;
    with swap_every = 4 and phase 0 the launch has no round and needs 6."""
    for group in (2, 4):
        assert _run(L, _plan(), B=0, draw0=2 ** 64 - 10, n_steps=3, group=group) == 0       # streams up to 2^64 - 2
        assert _run(L, _plan(), B=0, draw0=2 ** 64 - 9, n_steps=3, group=group) == 1
        assert _run(L, _plan(), B=0, draw0=2 ** 64 - 7, n_steps=3, group=group, swap_every=4) == 0
        assert _run(L, _plan(), B=0, draw0=2 ** 64 - 7, n_steps=3, group=group, swap_every=4, swap_phase=1) == 1
    assert _run(L, _plan(hmc=0), B=0) == 1                                # checked before the batch size is looked at


# ------------------------------------------------------------------------------------------------ the sampler on stubs
B_, D_ = 8, 2


def _stub(hmc=True, layered=False, use_temperature=True):
    def _plan_():
        raise AssertionError("a refused call must not build a plan")
    return types.SimpleNamespace(hmc=hmc, layered=layered, x_dim=D_, trajectory_length=5, temperature=1.0,
                                 use_temperature=use_temperature, _draws=4, _seed=7, _device=torch.device("cpu"),
                                 _plan=_plan_)


def _sampler(dyn):
    import l2hmc_amd as la
    return la.DynamicsSampler(dyn)


def test_signatures():
    import l2hmc_amd as la
    assert (str(inspect.signature(la.DynamicsSampler.run_hmc_exchange))
            == "(self, run_steps, x=None, keep_samples=True, temperature=None, eps=None, replicas=None, swap_every=1, "
               "first_parity=0, replica0=None)")
    assert (str(inspect.signature(la.DynamicsSampler.run_exchange))
            == "(self, run_steps, x=None, keep_samples=True, temperature=None, replicas=None, swap_every=1, "
               "first_parity=0, replica0=None)")
    assert str(inspect.signature(la.DynamicsSampler.swap_replicas)) == "(self, x, temperature, replicas, parity)"


TEMPS = np.linspace(1.0, 4.5, B_)[None, :]
BAD = [dict(replicas=1), dict(replicas=0), dict(replicas=-2), dict(replicas=3), dict(replicas=5), dict(replicas=16),
       dict(replicas=2.5), dict(replicas=4, swap_every=0), dict(replicas=4, swap_every=-1),
       dict(replicas=4, first_parity=2), dict(replicas=4, first_parity=-1),
       dict(replicas=4, replica0=np.arange(B_)),                       # int64
       dict(replicas=4, replica0=np.arange(B_, dtype=np.float32)),
       dict(replicas=4, replica0=np.arange(B_ - 1, dtype=np.int32)),
       dict(replicas=4, replica0=np.zeros((1, B_), dtype=np.int32)),
       dict(replicas=4, replica0=torch.arange(B_)),                     # int64
       dict(replicas=4, temperature=None), dict(replicas=4, temperature=[1.0, 2.0]),
       dict(replicas=4, temperature=0.0)]


@pytest.mark.parametrize("kw", BAD)
@pytest.mark.parametrize("method,hmc", [("run_hmc_exchange", True), ("run_exchange", False)])
def test_the_exchange_runs_refuse(method, hmc, kw):
    dyn = _stub(hmc=hmc)
    args = dict(temperature=TEMPS)
    args.update(kw)
    with pytest.raises(ValueError):
        getattr(_sampler(dyn), method)(5, torch.zeros(B_, D_), **args)
    assert dyn._draws == 4


def test_a_group_of_more_than_64_rungs_is_refused():
    x0, temps = torch.zeros(130, D_), np.linspace(1.0, 4.0, 130)[None, :]
    for method, hmc in (("run_hmc_exchange", True), ("run_exchange", False)):
        dyn = _stub(hmc=hmc)
        with pytest.raises(ValueError, match=f"{method}: replicas=65"):
            getattr(_sampler(dyn), method)(5, x0, temperature=temps, replicas=65)
        with pytest.raises(AssertionError, match="must not build a plan"):
            getattr(_sampler(dyn), method)(5, torch.zeros(128, D_), temperature=temps[:, :128], replicas=64)
    with pytest.raises(ValueError, match="swap_replicas: replicas=65"):
        _sampler(_stub()).swap_replicas(x0, temps, 65, 0)


def test_the_exchange_runs_refuse_the_other_kind_of_dynamics_and_a_layered_one():
    x0 = torch.zeros(B_, D_)
    dyn = _stub(hmc=False)
    with pytest.raises(ValueError, match="`run`"):
        _sampler(dyn).run_hmc_exchange(5, x0, temperature=TEMPS, replicas=4)
    dyn = _stub(hmc=True)
    with pytest.raises(ValueError, match="`run_hmc_exchange`"):
        _sampler(dyn).run_exchange(5, x0, temperature=TEMPS, replicas=4)
    for hmc, method in ((True, "run_hmc_exchange"), (False, "run_exchange")):
        dyn = _stub(hmc=hmc, layered=True)
        with pytest.raises(NotImplementedError):
            getattr(_sampler(dyn), method)(5, x0, temperature=TEMPS, replicas=4)
        with pytest.raises(NotImplementedError, match="swap_replicas: "):
            _sampler(dyn).swap_replicas(x0, TEMPS, 4, 0)
        assert dyn._draws == 4
    smp = _sampler(_stub(hmc=False))
    smp.steps_per_launch = 1
    with pytest.raises(NotImplementedError, match="run_exchange: "):
        smp.run_exchange(5, x0, temperature=TEMPS, replicas=4)
    dyn = _stub(use_temperature=False)
    with pytest.raises(ValueError, match="use_temperature=False"):
        _sampler(dyn).run_hmc_exchange(5, x0, temperature=TEMPS, replicas=4)


def test_the_exchange_runs_accept_good_arguments_up_to_the_plan():
    x0 = torch.zeros(B_, D_)
    for kw in (dict(replicas=2), dict(replicas=4, swap_every=3, first_parity=1),
               dict(replicas=8, replica0=np.arange(B_, dtype=np.int32)),
               dict(replicas=4, replica0=torch.arange(B_, dtype=torch.int32)), dict(replicas=np.int64(4)),
               dict(replicas=4, temperature=2.0), dict(replicas=4, temperature=np.ones((5, B_)))):
        for method, hmc in (("run_hmc_exchange", True), ("run_exchange", False)):
            dyn = _stub(hmc=hmc)
            args = dict(temperature=TEMPS)
            args.update(kw)
            with pytest.raises(AssertionError, match="must not build a plan"):
                getattr(_sampler(dyn), method)(5, x0, **args)
            assert dyn._draws == 4


def test_an_empty_exchange_run_returns_empty_histories():
    x0 = torch.ones(B_, D_)
    for method, hmc in (("run_hmc_exchange", True), ("run_exchange", False)):
        dyn = _stub(hmc=hmc)
        out = getattr(_sampler(dyn), method)(0, x0, temperature=TEMPS, replicas=4)
        assert out["swap_p"].shape == (0, B_) and out["swap_p"].dtype == np.float32
        assert out["swapped"].shape == (0, B_) and out["swapped"].dtype == np.bool_
        assert out["replica"].shape == (0, B_) and out["replica"].dtype == np.int32
        assert out["swap_rate"].shape == (3,) and np.isnan(out["swap_rate"]).all()
        assert out["px"].shape == (0, B_) and torch.equal(out["samples_out"], x0) and dyn._draws == 4
        assert np.isnan(out["mean_accept"])
        trips, groups = stats.replica_round_trips(out["replica"], 4)
        assert trips.tolist() == [0] * B_ and groups.tolist() == [0, 0]


@pytest.mark.parametrize("kw", [dict(replicas=1), dict(replicas=3), dict(parity=2), dict(parity=-1),
                                dict(temperature=np.ones(B_ + 1)), dict(temperature=np.ones((2, B_))),
                                dict(temperature=0.0), dict(temperature=[1.0] * (B_ - 1) + [float("nan")]),
                                dict(x=torch.zeros(B_, D_ + 1)), dict(x=np.zeros((B_, D_)))])
def test_swap_replicas_refuses(kw):
    for hmc in (True, False):
        dyn = _stub(hmc=hmc)
        args = dict(x=torch.zeros(B_, D_), temperature=TEMPS, replicas=4, parity=0)
        args.update(kw)
        with pytest.raises(ValueError, match="swap_replicas: "):
            _sampler(dyn).swap_replicas(**args)
        assert dyn._draws == 4


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_exchanges_exactly_the_accepted_pairs():
    G, B = 5, 10
    rng = np.random.default_rng(3)
    x = torch.as_tensor(rng.standard_normal((B, 2)) * 2)
    temps = rng.uniform(0.5, 5, B)
    for parity in (0, 1):
        u = rng.uniform(size=B)
        xn, p, sw, perm = TR.swap_round(x, temps, G, parity, u, TR.energy64)
        low = lower_chains(B, G, parity)
        assert low.tolist() == ([0, 2, 5, 7] if parity == 0 else [1, 3, 6, 8])
        off = np.setdiff1d(np.arange(B), low)
        assert np.isnan(p[off].numpy()).all() and not sw[off].any() and np.isfinite(p[low].numpy()).all()
        U = TR.energy64(x).numpy()
        want = np.minimum(1.0, np.exp((1 / temps[low] - 1 / temps[low + 1]) * (U[low] - U[low + 1])))
        assert np.allclose(p[low].numpy(), want, rtol=1e-14)
        assert np.array_equal(sw[low].numpy(), want > u[low])
        for a in low:
            if sw[a]:
                assert torch.equal(xn[a], x[a + 1]) and torch.equal(xn[a + 1], x[a])
            else:
                assert torch.equal(xn[a], x[a]) and torch.equal(xn[a + 1], x[a + 1])
        assert torch.equal(xn, x[perm]) and sorted(perm.tolist()) == list(range(B))


def _max_z(rule):
    G = len(TR.LADDER)
    x0, temps, exact = TR.ladder_start()
    x = x0.copy()
    rng = np.random.default_rng(11)
    zs, rates = [], []
    for t in range(1, max(TR.CHECKPOINTS) + 1):
        x = TR.hmc_step64(x, temps, rng)
        xt, _, sw, _ = TR.swap_round(torch.as_tensor(x), temps, G, (t - 1) % 2, rng.uniform(size=x.shape[0]),
                                     TR.energy64, rule)
        x = xt.numpy()
        rates.append(float(sw[lower_chains(x.shape[0], G, (t - 1) % 2)].double().mean()))
        if t in TR.CHECKPOINTS:
            zs.append(TR.rung_zscores(x, exact, with_energy=True))
    m = float(np.abs(np.array(zs)).max())
    print(f"\n[invariance] toy replica exchange restatement rule={rule}: max|z| = {m:.2f}, "
          f"swap rate {np.mean(rates):.3f}")
    return m


def test_restatement_leaves_the_target_invariant_and_defects_do_not():
    assert _max_z("correct") < Z_PASS
    assert _max_z("sign_flipped") > Z_DEFECT
    assert _max_z("always_accept") > Z_DEFECT
