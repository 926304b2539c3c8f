"""Host side of the plain-HMC run entry (l2hmc_small_hmc_run in l2hmc_amd/csrc/small_hmc.hip) and of
`DynamicsSampler.run_hmc`: the declaration and its binding, the argument checks that must fail before any device call,
and what `run_hmc` refuses.  No GPU: plans and arguments carry any non-NULL address where a pointer is checked, and the
sampler runs on stub dynamics that must not be asked for a plan."""
import ctypes as C
import inspect
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


def _target(dim=2, K=1, kind=1, temperature=1.0, mu=PTR):
    return _lib.MogTarget(dim=dim, K=K, is_gaussian=kind, temperature=temperature, mu=mu, prec=PTR, log_const=PTR)


def _plan(x_dim=2, hmc=1, N=5, masks=PTR, target=None):
    return _lib.SmallPlan(x_dim=x_dim, num_nodes=0, trajectory_length=N, hmc=hmc, eps=0.1, first_layer_form=0,
                          masks=masks, target=target if target is not None else _target())


def _run(L, plan, x_in=PTR, x_next=PTR, B=4, draw0=0, n_steps=3, temps=None, step_stride=0, chain_stride=0,
         eps_chain=None):
    return L.l2hmc_small_hmc_run(None if plan is None else C.byref(plan), x_in, x_next, B, 42, draw0, n_steps, temps,
                                 step_stride, chain_stride, eps_chain, None, None, None)


def test_header_declares_and_binding_matches():
    assert "l2hmc_small_hmc_run" in _lib.declared_symbols()
    # plan, x_in, x_next, B, seed, draw0, n_steps, temps, step_stride, chain_stride, eps_chain, px, samples, stream
    assert _lib._PROTOS["l2hmc_small_hmc_run"] == (
        C.c_int, [C.POINTER(_lib.SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _I64, _I64, _P, _P, _P, _P])
    text = header_text()
    assert ("int l2hmc_small_hmc_run(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B, "
            "uint64_t seed, uint64_t draw0, int32_t n_steps, const float* temps, int64_t step_stride, "
            "int64_t chain_stride, const float* eps_chain, float* px, float* samples, l2hmc_stream_t stream);") in text
    assert "#define L2HMC_ABI_VERSION 1" in text


def test_library_exports_the_entry(L):
    assert L.l2hmc_small_hmc_run is not None and L.l2hmc_abi_version() == 1


def test_bad_arguments_fail_with_a_message_before_any_device_call(L):
    ok = _plan()
    cases = [(dict(plan=None), "plan is NULL"), (dict(x_in=None), "x_in / x_next is NULL"),
             (dict(x_next=None), "x_in / x_next is NULL"), (dict(B=-1), "B < 0"),
             (dict(n_steps=0), "n_steps=0"), (dict(n_steps=-1), "n_steps=-1"),
             (dict(plan=_plan(hmc=0)), "use l2hmc_small_run"),
             (dict(draw0=2 ** 64 - 4, n_steps=2), "draw0 + 2 * n_steps overflows 64 bits"),
             (dict(temps=PTR, step_stride=-1), "negative stride"), (dict(temps=PTR, chain_stride=-1), "negative stride"),
             (dict(step_stride=-1), "negative stride"),
             (dict(plan=_plan(x_dim=3)), "x_dim=3 != target dim=2"),
             (dict(plan=_plan(N=0)), "bad trajectory_length / masks"),
             (dict(plan=_plan(masks=None)), "bad trajectory_length / masks"),
             (dict(plan=_plan(x_dim=9, target=_target(dim=9))), "target dim=9 (max 8)"),
             (dict(plan=_plan(target=_target(K=9))), "K=9 (max 8)"),
             (dict(plan=_plan(target=_target(kind=4))), "target kind 4 unknown"),
             (dict(plan=_plan(target=_target(temperature=0.0))), "temperature must be > 0"),
             (dict(plan=_plan(target=_target(mu=None))), "NULL parameter pointer"),
             (dict(plan=_plan(target=_target(kind=3, dim=1), x_dim=1)), "funnel target needs dim >= 2")]
    for kw, word in cases:
        plan = kw.pop("plan", ok)
        rc = _run(L, plan, **kw)
        msg = L.l2hmc_last_error().decode()
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        assert msg.startswith("small_hmc_run: ") and word in msg, (kw, msg)
    with pytest.raises(ValueError, match="small_hmc_run: n_steps=0 must be positive"):
        _lib.check(_run(L, ok, n_steps=0))


def test_the_last_stream_index_may_be_the_largest(L):
    assert _run(L, _plan(), B=0, draw0=2 ** 64 - 7, n_steps=3) == 0       # streams up to 2^64 - 2
    assert _run(L, _plan(), B=0, draw0=2 ** 64 - 6, n_steps=3) == 1


def test_an_empty_batch_is_a_no_op(L):
    assert _run(L, _plan(), B=0) == 0
    assert _run(L, _plan(), B=0, temps=PTR, step_stride=0, chain_stride=1, eps_chain=PTR) == 0
    assert _run(L, _plan(hmc=0), B=0) == 1                                # checked before the batch size is looked at


def test_the_l2hmc_run_entries_still_refuse_an_hmc_plan(L):
    plan = _plan(hmc=1)
    assert L.l2hmc_small_run(C.byref(plan), PTR, PTR, 4, 42, 0, 3, None, None, None) == 1
    assert "small_run: the hmc sampler proposes with the forward trajectory only" in L.l2hmc_last_error().decode()
    assert L.l2hmc_small_run_tempered(C.byref(plan), PTR, PTR, 4, 42, 0, 3, PTR, 0, 0, None, None, None) == 1
    assert "small_run_tempered: the hmc sampler" in L.l2hmc_last_error().decode()
    assert L.l2hmc_small_propose(C.byref(plan), PTR, 4, 42, 0, None, None, None, None, None) == 1
    assert "small_propose: the hmc sampler" in L.l2hmc_last_error().decode()


# ------------------------------------------------------------------------------------------------ run_hmc on stubs
def _stub(hmc=True, layered=False, use_temperature=True):
    def _plan():
        raise AssertionError("a refused call must not build a plan")
    return types.SimpleNamespace(hmc=hmc, layered=layered, x_dim=2, trajectory_length=5, temperature=1.0,
                                 use_temperature=use_temperature, _draws=4, _seed=7, _device=torch.device("cpu"),
                                 _plan=_plan)


def test_run_hmc_has_the_signature_of_run_plus_eps():
    import l2hmc_amd as la
    sig = inspect.signature(la.DynamicsSampler.run_hmc)
    assert str(sig) == "(self, run_steps, x=None, keep_samples=True, temperature=None, eps=None)"
    assert str(inspect.signature(la.DynamicsSampler.run)) == "(self, run_steps, x=None, keep_samples=True, temperature=None)"


def test_run_hmc_refuses_other_dynamics_without_a_draw():
    import l2hmc_amd as la
    x0 = torch.zeros(3, 2)
    dyn = _stub(hmc=False)
    with pytest.raises(ValueError, match="`run`"):
        la.DynamicsSampler(dyn).run_hmc(5, x0)
    assert dyn._draws == 4
    dyn = _stub(hmc=True, layered=True)
    with pytest.raises(NotImplementedError, match="`run`"):
        la.DynamicsSampler(dyn).run_hmc(5, x0)
    assert dyn._draws == 4


@pytest.mark.parametrize("eps", [0, 0.0, -0.1, float("inf"), float("nan"), 1e-60, 1e60, [0.1, 0.1, 0.0],
                                 [0.1, float("nan"), 0.1], [0.1, 0.2, 0.3, 0.4], [[0.1, 0.2, 0.3]], [[0.1], [0.2], [0.3]],
                                 [0.1]])
def test_run_hmc_refuses_bad_step_sizes(eps):
    import l2hmc_amd as la
    dyn = _stub()
    with pytest.raises(ValueError, match="run_hmc: e"):
        la.DynamicsSampler(dyn).run_hmc(5, torch.zeros(3, 2), eps=eps)
    with pytest.raises(ValueError, match="run_hmc: e"):
        la.DynamicsSampler(dyn).run_hmc(5, torch.zeros(3, 2), eps=torch.tensor(eps, dtype=torch.float64))
    assert dyn._draws == 4


def test_run_hmc_accepts_good_step_sizes_up_to_the_plan():
    """A scalar and a [B] array pass the check: the call gets as far as the plan (which the stub refuses)."""
    import l2hmc_amd as la
    for eps in (0.25, np.float32(0.25), [0.1, 0.2, 0.3], np.array([0.1, 0.2, 0.3]), torch.tensor([0.1, 0.2, 0.3])):
        dyn = _stub()
        with pytest.raises(AssertionError, match="must not build a plan"):
            la.DynamicsSampler(dyn).run_hmc(5, torch.zeros(3, 2), eps=eps)
        assert dyn._draws == 4


def test_run_hmc_refuses_a_temperature_the_dynamics_would_ignore():
    import l2hmc_amd as la
    dyn = _stub(use_temperature=False)
    with pytest.raises(ValueError, match="use_temperature=False"):
        la.DynamicsSampler(dyn).run_hmc(5, torch.zeros(3, 2), temperature=2.0)
    dyn = _stub()
    for bad in ([1.0, 2.0], np.ones((5, 2)), 0.0, [[1.0, float("inf"), 1.0]]):
        with pytest.raises(ValueError):
            la.DynamicsSampler(dyn).run_hmc(5, torch.zeros(3, 2), temperature=bad)
    assert dyn._draws == 4


def test_an_empty_run_and_a_missing_start():
    import l2hmc_amd as la
    dyn = _stub()
    x0 = torch.ones(3, 2)
    out = la.DynamicsSampler(dyn).run_hmc(0, x0, eps=[0.1, 0.2, 0.3])
    assert out["px"].shape == (0, 3) and out["samples"].shape == (0, 3, 2) and torch.equal(out["samples_out"], x0)
    assert np.isnan(out["mean_accept"]) and dyn._draws == 4
    assert "samples" not in la.DynamicsSampler(dyn).run_hmc(0, x0, keep_samples=False)
    with pytest.raises(ValueError):
        la.DynamicsSampler(dyn).run_hmc(2)
    with pytest.raises(ValueError):
        la.DynamicsSampler(dyn).run_hmc(-1, x0)
