"""Host side of the toy-target run entry (l2hmc_small_run in l2hmc_amd/csrc/small_mlp.hip): its declaration and binding,
the argument checks that must fail before any device call, the tunnelling rate of stats.py, and the path
`DynamicsSampler` picks.  No GPU: plans and arguments carry any non-NULL address where a pointer is checked, and the
sampler runs on a stub dynamics with `propose` replaced."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _net(dim, H):
    return _lib.DenseNet(D=dim, H=H, Ka=dim, Kb=dim, w1_t=PTR, wt=PTR, b1=PTR, wh_t=PTR, bh=PTR, whd_t=PTR, bhd=PTR,
                         coeff_s=PTR, coeff_q=PTR, q_tanh=1)


def _plan(x_dim=2, nodes=10, hmc=0, target_dim=2):
    tgt = _lib.MogTarget(dim=target_dim, K=1, is_gaussian=1, temperature=1.0, mu=PTR, prec=PTR, log_const=PTR)
    return _lib.SmallPlan(x_dim=x_dim, num_nodes=nodes, trajectory_length=5, hmc=hmc, eps=0.1, first_layer_form=0,
                          masks=PTR, xnet=_net(x_dim, nodes), vnet=_net(x_dim, nodes), target=tgt)


def _run(L, plan, x_in=PTR, x_next=PTR, B=4, draw0=0, n_steps=3):
    return L.l2hmc_small_run(None if plan is None else C.byref(plan), x_in, x_next, B, 42, draw0, n_steps, None, None,
                             None)


def test_header_declares_and_binding_matches():
    assert "l2hmc_small_run" in _lib.declared_symbols()
    # plan, x_in, x_next, B, seed, draw0, n_steps, px, samples, stream
    assert _lib._PROTOS["l2hmc_small_run"] == (
        C.c_int, [C.POINTER(_lib.SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _P, _P])
    text = header_text(comments=True)
    assert ("int l2hmc_small_run(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B, "
            "uint64_t seed, uint64_t draw0, int32_t n_steps, float* px, float* samples, "
            "l2hmc_stream_t stream);") in text
    assert "#define L2HMC_ABI_VERSION 1" in text


def test_library_exports_the_entry(L):
    assert L.l2hmc_small_run is not None and L.l2hmc_abi_version() == 1


def test_bad_arguments_fail_with_a_message_before_any_device_call(L):
    ok = _plan()
    cases = [(dict(plan=None), "plan is NULL"), (dict(x_in=None), "x_in"), (dict(x_next=None), "x_next"),
             (dict(n_steps=0), "n_steps"), (dict(n_steps=-1), "n_steps"),
             (dict(plan=_plan(hmc=1)), "the hmc sampler proposes with the forward trajectory only"),
             (dict(draw0=2 ** 64 - 4, n_steps=2), "overflows 64 bits"),
             (dict(plan=_plan(x_dim=3)), "x_dim=3 != target dim=2"),
             (dict(plan=_plan(nodes=65)), "num_nodes=65")]
    for kw, word in cases:
        plan = kw.pop("plan", ok)
        rc = _run(L, plan, **kw)
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        assert word in L.l2hmc_last_error().decode(), (kw, L.l2hmc_last_error().decode())
    with pytest.raises(ValueError):
        _lib.check(_run(L, ok, n_steps=0))


def test_the_hmc_refusal_is_worded_as_small_proposes(L):
    assert _run(L, _plan(hmc=1)) == 1
    run_msg = L.l2hmc_last_error().decode()
    assert L.l2hmc_small_propose(C.byref(_plan(hmc=1)), PTR, 4, 42, 0, None, None, None, None, None) == 1
    prop_msg = L.l2hmc_last_error().decode()
    assert run_msg.split(": ", 1)[1] == prop_msg.split(": ", 1)[1]


def test_an_empty_batch_is_a_no_op(L):
    assert _run(L, _plan(), B=0) == 0
    assert _run(L, _plan(), B=0, draw0=2 ** 64 - 13, n_steps=3) == 0      # the last stream index is 2^64 - 1
    assert _run(L, _plan(), B=-1) == 1


# ------------------------------------------------------------------------------------------------ tunnelling rate
def _rate_by_loops(trajectory, means):
    """utils/trajectories.py:63-95 as a literal double loop."""
    events = 0
    member = []
    for pt in trajectory:
        best, best_d = None, None
        for k, mu in enumerate(means):
            d = float(np.sqrt(np.sum((np.asarray(pt, dtype=np.float64) - mu) ** 2)))
            if best is None or d < best_d:
                best, best_d = k, d
        member.append(best)
    for i in range(len(member) - 1):
        if member[i + 1] != member[i]:
            events += 1
    return events / (len(trajectory) - 1)


def test_tunneling_rate_equals_the_double_loop_for_both_ranks():
    from l2hmc_amd import stats
    rng = np.random.default_rng(11)
    means = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, -1.0]])
    walk = np.cumsum(rng.normal(0, 0.35, (60, 5, 2)), axis=0) * 0.5 + means[rng.integers(0, 3, 5)]
    walk = np.clip(walk, -2, 2)
    rates = stats.calc_tunneling_rate(walk, means)
    assert rates.shape == (5,)
    want = [_rate_by_loops(walk[:, c], means) for c in range(5)]
    assert np.array_equal(rates, np.array(want))
    assert 0 < max(want) < 1                             # the walk does move among the modes
    for c in range(5):
        one = stats.calc_tunneling_rate(walk[:, c], means)
        assert isinstance(one, float) and one == want[c]
    assert np.array_equal(stats.calc_tunneling_rate(walk.astype(np.float32), [m for m in means]), rates)


def test_tunneling_rate_of_a_stuck_and_of_an_alternating_trajectory():
    from l2hmc_amd import stats
    means = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, -1.0]])
    stuck = means[1] + 0.1 * np.random.default_rng(3).normal(size=(20, 2))
    assert stats.calc_tunneling_rate(stuck, means) == 0.0
    alt = np.stack([means[i % 2] for i in range(21)])
    assert stats.calc_tunneling_rate(alt, means) == 1.0
    both = np.stack([stuck[:20], alt[:20]], axis=1)
    assert np.array_equal(stats.calc_tunneling_rate(both, means), np.array([0.0, 1.0]))
    with pytest.raises(ValueError):
        stats.calc_tunneling_rate(alt[:1], means)


# ------------------------------------------------------------------------------------------------ the sampler's path
def _stub(hmc=False, layered=False):
    def _plan():
        raise AssertionError("the host loop must not build a plan")
    return types.SimpleNamespace(hmc=hmc, layered=layered, x_dim=2, trajectory_length=5, temperature=1.0, _draws=4,
                                 _seed=7, _device=torch.device("cpu"), _plan=_plan)


@pytest.fixture()
def fake_propose(monkeypatch):
    """Stands in for sampler.propose: x + 1, px = step count, and the four streams a step with the
    Metropolis-Hastings uniform takes (sampler.py: `_draws += 4`)."""
    from l2hmc_amd import dynamics_sampler as ds
    calls = []

    def propose(x, dynamics, init_v=None, aux=None, do_mh_step=False, **kw):
        assert do_mh_step and init_v is None and not kw
        calls.append(dynamics._draws)
        dynamics._draws += 4
        px = torch.full((x.shape[0],), float(len(calls)))
        return x + 1, None, px, [x + 1]
    monkeypatch.setattr(ds, "propose", propose)
    return calls


@pytest.mark.parametrize("hmc,layered,spl", [(True, False, 256), (False, True, 256), (False, False, 1)])
def test_sampler_takes_the_host_loop(fake_propose, hmc, layered, spl):
    import l2hmc_amd as la
    dyn = _stub(hmc, layered)
    smp = la.DynamicsSampler(dyn)
    assert smp.steps_per_launch == 256
    smp.steps_per_launch = spl
    x0 = torch.zeros(3, 2)
    out = smp.run(5, x0)
    assert len(fake_propose) == 5 and fake_propose == [4, 8, 12, 16, 20]
    assert dyn._draws == 4 + 4 * 5                       # 4 n further
    assert out["px"].shape == (5, 3) and out["samples"].shape == (5, 3, 2)
    assert np.array_equal(out["px"][:, 0], np.arange(1, 6, dtype=np.float32))
    assert np.array_equal(out["samples"][:, 0, 0], np.arange(1, 6, dtype=np.float32))
    assert torch.equal(out["samples_out"], torch.full((3, 2), 5.0)) and torch.equal(x0, torch.zeros(3, 2))
    assert out["mean_accept"] == 3.0
    assert "samples" not in smp.run(2, x0, keep_samples=False)


def test_sampler_takes_the_launches_for_an_l2hmc_dynamics_the_kernel_holds(fake_propose):
    import l2hmc_amd as la
    smp = la.DynamicsSampler(_stub())
    with pytest.raises(AssertionError, match="must not build a plan"):
        smp.run(2, torch.zeros(3, 2))                    # the one-launch path asks for the plan first
    assert fake_propose == []


def test_an_empty_run_and_the_trajectory_layout(fake_propose):
    import l2hmc_amd as la
    dyn = _stub(hmc=True)
    dist = types.SimpleNamespace(get_samples=lambda n: np.full((n, 2), 0.5))
    smp = la.DynamicsSampler(dyn, distribution=dist)
    x0 = torch.ones(3, 2)
    out = smp.run(0, x0)
    assert out["px"].shape == (0, 3) and out["samples"].shape == (0, 3, 2) and torch.equal(out["samples_out"], x0)
    assert np.isnan(out["mean_accept"]) and dyn._draws == 4 and fake_propose == []
    dyn.temperature = 2.0
    traj, px = smp.generate_trajectories(temp=3.0, num_samples=6, num_steps=4)
    assert traj.shape == (4, 6, 2) and px.shape == (4, 6) and dyn.temperature == 2.0
    assert np.array_equal(traj[:, 0, 0], 0.5 + np.arange(4))          # trajectories[s] is the input of step s
    with pytest.raises(ValueError):
        la.DynamicsSampler(dyn).generate_trajectories(num_steps=2)
    with pytest.raises(ValueError):
        la.DynamicsSampler(dyn).run(2)
