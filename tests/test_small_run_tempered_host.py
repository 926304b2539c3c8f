"""Host side of the tempered toy-target run (l2hmc_small_run_tempered in l2hmc_amd/csrc/small_mlp.hip, and
`DynamicsSampler.run(..., temperature=)`): the declaration and binding, the argument checks that must fail before any
device call, the validation of the temperatures in Python, and the host loop's handling of a schedule.  No GPU: plans and
arguments carry any non-NULL address where a pointer is checked (as tests/test_small_run_host.py), and the sampler runs
on a stub dynamics with `propose` replaced."""
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


def _plan(x_dim=2, nodes=10, hmc=0, target_dim=2, temperature=1.0):
    tgt = _lib.MogTarget(dim=target_dim, K=1, is_gaussian=1, temperature=temperature, mu=PTR, prec=PTR, log_const=PTR)
    return _lib.SmallPlan(x_dim=x_dim, num_nodes=nodes, trajectory_length=5, hmc=hmc, eps=0.1, first_layer_form=0,
                          masks=PTR, xnet=_net(x_dim, nodes), vnet=_net(x_dim, nodes), target=tgt)


def _run(L, plan, x_in=PTR, x_next=PTR, B=4, draw0=0, n_steps=3, temps=PTR, step_stride=1, chain_stride=0):
    return L.l2hmc_small_run_tempered(None if plan is None else C.byref(plan), x_in, x_next, B, 42, draw0, n_steps,
                                      temps, step_stride, chain_stride, None, None, None)


# ------------------------------------------------------------------------------------------------ the C entry
def test_header_declares_and_binding_matches():
    assert "l2hmc_small_run_tempered" in _lib.declared_symbols()
    # plan, x_in, x_next, B, seed, draw0, n_steps, temps, step_stride, chain_stride, px, samples, stream
    assert _lib._PROTOS["l2hmc_small_run_tempered"] == (
        C.c_int, [C.POINTER(_lib.SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _I64, _I64, _P, _P, _P])
    text = header_text(comments=True)
    assert ("int l2hmc_small_run_tempered(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B, "
            "uint64_t seed, uint64_t draw0, int32_t n_steps, const float* temps, int64_t step_stride, "
            "int64_t chain_stride, float* px, float* samples, l2hmc_stream_t stream);") in text
    assert "#define L2HMC_ABI_VERSION 1" in text


def test_library_exports_the_entry_and_the_abi_version_stays(L):
    assert L.l2hmc_small_run_tempered is not None and L.l2hmc_abi_version() == 1


def test_bad_arguments_fail_with_a_message_before_any_device_call(L):
    ok = _plan()
    cases = [(dict(plan=None), "plan is NULL"), (dict(x_in=None), "x_in"), (dict(x_next=None), "x_next"),
             (dict(n_steps=0), "n_steps"), (dict(n_steps=-1), "n_steps"),
             (dict(plan=_plan(hmc=1)), "the hmc sampler proposes with the forward trajectory only"),
             (dict(draw0=2 ** 64 - 4, n_steps=2), "overflows 64 bits"),
             (dict(temps=None), "temps is NULL"),
             (dict(step_stride=-1), "negative stride"), (dict(chain_stride=-1), "negative stride"),
             (dict(step_stride=-4, chain_stride=1), "negative stride"),
             (dict(B=-1), "B < 0"),
             (dict(plan=_plan(x_dim=3)), "x_dim=3 != target dim=2"),
             (dict(plan=_plan(nodes=65)), "num_nodes=65"),
             (dict(plan=_plan(temperature=0.0)), "temperature")]       # unused by this entry, still checked
    for kw, word in cases:
        plan = kw.pop("plan", ok)
        rc = _run(L, plan, **kw)
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        msg = L.l2hmc_last_error().decode()
        assert word in msg, (kw, msg)
    with pytest.raises(ValueError):
        _lib.check(_run(L, ok, temps=None))


def test_the_messages_name_the_entry_and_the_hmc_refusal_is_small_proposes(L):
    assert _run(L, _plan(hmc=1)) == 1
    run_msg = L.l2hmc_last_error().decode()
    assert run_msg.startswith("small_run_tempered: ")
    assert L.l2hmc_small_propose(C.byref(_plan(hmc=1)), PTR, 4, 42, 0, None, None, None, None, None) == 1
    prop_msg = L.l2hmc_last_error().decode()
    assert run_msg.split(": ", 1)[1] == prop_msg.split(": ", 1)[1]
    # the untempered entry keeps its own name in what it shares with this one
    assert L.l2hmc_small_run(C.byref(_plan()), PTR, PTR, 4, 42, 0, 0, None, None, None) == 1
    assert L.l2hmc_last_error().decode().startswith("small_run: n_steps=0")


def test_an_empty_batch_is_a_no_op_and_zero_strides_are_allowed(L):
    assert _run(L, _plan(), B=0) == 0
    assert _run(L, _plan(), B=0, step_stride=0, chain_stride=0) == 0
    assert _run(L, _plan(), B=0, step_stride=0, chain_stride=1) == 0
    assert _run(L, _plan(), B=0, draw0=2 ** 64 - 13, n_steps=3) == 0      # the last stream index is 2^64 - 1
    assert _run(L, _plan(), B=0, temps=None) == 1                         # checked before the batch size is looked at


# ------------------------------------------------------------------------------------------------ the sampler
def _stub(hmc=False, layered=False, use_temperature=True):
    def _plan():
        raise AssertionError("the host loop must not build a plan")
    return types.SimpleNamespace(hmc=hmc, layered=layered, x_dim=2, trajectory_length=5, temperature=1.5, _draws=4,
                                 _seed=7, _device=torch.device("cpu"), _plan=_plan, use_temperature=use_temperature)


@pytest.fixture()
def fake_propose(monkeypatch):
    """Stands in for sampler.propose: x + 1, px = the temperature the step sees, four streams per step; raises at the
    step number in `fail_at`."""
    from l2hmc_amd import dynamics_sampler as ds
    seen = types.SimpleNamespace(temps=[], fail_at=None)

    def propose(x, dynamics, init_v=None, aux=None, do_mh_step=False, **kw):
        assert do_mh_step and init_v is None and not kw
        if seen.fail_at == len(seen.temps):
            raise RuntimeError("propose failed")
        seen.temps.append(dynamics.temperature)
        dynamics._draws += 4
        return x + 1, None, torch.full((x.shape[0],), float(dynamics.temperature)), [x + 1]
    monkeypatch.setattr(ds, "propose", propose)
    return seen


LOOPS = [(True, False, 256), (False, True, 256), (False, False, 1)]


@pytest.mark.parametrize("hmc,layered,spl", LOOPS)
def test_host_loop_sets_the_scheduled_temperature_and_restores(fake_propose, hmc, layered, spl):
    import l2hmc_amd as la
    dyn = _stub(hmc, layered)
    smp = la.DynamicsSampler(dyn)
    smp.steps_per_launch = spl
    x0 = torch.zeros(3, 2)
    sched = [2.0, 0.5, 3.25, 1.0, 7.0]
    out = smp.run(5, x0, temperature=sched)
    assert fake_propose.temps == sched and all(type(t) is float for t in fake_propose.temps)
    assert dyn.temperature == 1.5 and dyn._draws == 4 + 4 * 5
    assert np.array_equal(out["px"], np.repeat(np.float32(sched)[:, None], 3, axis=1))
    assert out["samples"].shape == (5, 3, 2) and torch.equal(out["samples_out"], torch.full((3, 2), 5.0))
    assert torch.equal(x0, torch.zeros(3, 2))
    # a scalar, in each of the forms a caller may hold it in
    for scalar in (2.5, np.float32(2.5), np.array(2.5), torch.tensor(2.5)):
        fake_propose.temps.clear()
        smp.run(3, x0, temperature=scalar, keep_samples=False)
        assert fake_propose.temps == [2.5] * 3 and dyn.temperature == 1.5
    # a schedule as an array and as a tensor; float64 entries are rounded to the float32 the kernels take
    for arr in (np.array(sched[:2]), torch.tensor(sched[:2], dtype=torch.float64)):
        fake_propose.temps.clear()
        smp.run(2, x0, temperature=arr)
        assert fake_propose.temps == sched[:2]
    fake_propose.temps.clear()
    smp.run(1, x0, temperature=[0.1])
    assert fake_propose.temps == [float(np.float32(0.1))]
    # no keyword: the loop leaves the temperature alone
    fake_propose.temps.clear()
    smp.run(2, x0)
    assert fake_propose.temps == [1.5, 1.5] and dyn.temperature == 1.5


def test_host_loop_restores_the_temperature_when_propose_raises(fake_propose):
    import l2hmc_amd as la
    dyn = _stub(hmc=True)
    smp = la.DynamicsSampler(dyn)
    fake_propose.fail_at = 2
    with pytest.raises(RuntimeError, match="propose failed"):
        smp.run(4, torch.zeros(3, 2), temperature=[2.0, 3.0, 4.0, 5.0])
    assert fake_propose.temps == [2.0, 3.0] and dyn.temperature == 1.5
    assert dyn._draws == 4 + 4 * 2                       # the counter stands where the completed steps left it


@pytest.mark.parametrize("hmc,layered,spl", LOOPS)
def test_host_loop_refuses_temperatures_per_chain(fake_propose, hmc, layered, spl):
    import l2hmc_amd as la
    dyn = _stub(hmc, layered)
    smp = la.DynamicsSampler(dyn)
    smp.steps_per_launch = spl
    for t in (np.full((1, 3), 2.0), np.full((4, 3), 2.0)):
        with pytest.raises(NotImplementedError, match="one-launch"):
            smp.run(4, torch.zeros(3, 2), temperature=t)
    assert fake_propose.temps == [] and dyn._draws == 4 and dyn.temperature == 1.5


def test_the_one_launch_path_is_taken_with_a_temperature(fake_propose):
    import l2hmc_amd as la
    for t in (2.0, [2.0, 3.0], np.full((1, 3), 2.0), np.full((2, 3), 2.0)):
        smp = la.DynamicsSampler(_stub())
        with pytest.raises(AssertionError, match="must not build a plan"):
            smp.run(2, torch.zeros(3, 2), temperature=t)     # the one-launch path asks for the plan first
    assert fake_propose.temps == []


@pytest.mark.parametrize("one_launch", [True, False])
def test_bad_temperatures_are_refused(fake_propose, one_launch):
    import l2hmc_amd as la
    dyn = _stub(hmc=not one_launch)
    smp = la.DynamicsSampler(dyn)
    x0, steps, B = torch.zeros(3, 2), 4, 3
    shapes = [(3,), (5,), (1,), (0,), (4, 1), (3, 4), (4, 2), (2, 3), (1, 4), (1, 1), (4, 3, 1), (1, 1, 3)]
    for shape in shapes:
        with pytest.raises(ValueError, match="shape"):
            smp.run(steps, x0, temperature=np.ones(shape))
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-50, 1e39):   # the last two: 0 / inf in float32
        for t in (bad, [1.0, bad, 1.0, 1.0], np.array([[1.0, 1.0, bad]]), np.where(np.eye(4, 3) > 0, bad, 1.0)):
            with pytest.raises(ValueError, match="finite and > 0"):
                smp.run(steps, x0, temperature=t)
    with pytest.raises(ValueError, match="shape"):           # also for an empty run
        smp.run(0, x0, temperature=[1.0])
    with pytest.raises(ValueError):
        smp.run(steps, x0, temperature="hot")
    assert fake_propose.temps == [] and dyn._draws == 4 and dyn.temperature == 1.5


@pytest.mark.parametrize("one_launch", [True, False])
def test_a_dynamics_that_ignores_temperatures_is_refused(fake_propose, one_launch):
    import l2hmc_amd as la
    dyn = _stub(hmc=not one_launch, use_temperature=False)
    smp = la.DynamicsSampler(dyn)
    for t in (2.0, [2.0, 3.0], np.full((1, 3), 2.0)):
        with pytest.raises(ValueError, match="use_temperature"):
            smp.run(2, torch.zeros(3, 2), temperature=t)
    assert fake_propose.temps == [] and dyn._draws == 4
    if not one_launch:
        smp.run(2, torch.zeros(3, 2))                        # without the keyword it runs as before
        assert fake_propose.temps == [1.5, 1.5]


def test_an_empty_run_with_a_temperature(fake_propose):
    import l2hmc_amd as la
    dyn = _stub(hmc=True)
    smp = la.DynamicsSampler(dyn)
    x0 = torch.ones(3, 2)
    for t in (2.0, np.ones((0,))):
        out = smp.run(0, x0, temperature=t)
        assert out["px"].shape == (0, 3) and torch.equal(out["samples_out"], x0) and dyn._draws == 4
    assert fake_propose.temps == []


def test_generate_trajectories_keeps_its_signature():
    import inspect
    import l2hmc_amd as la
    assert list(inspect.signature(la.DynamicsSampler.generate_trajectories).parameters) == [
        "self", "temp", "num_samples", "num_steps", "x"]
    assert list(inspect.signature(la.DynamicsSampler.run).parameters) == [
        "self", "run_steps", "x", "keep_samples", "temperature"]
