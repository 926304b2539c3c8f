"""Host side of the ladder form of the plain-HMC lattice run (l2hmc_gauge_hmc_run_ladder in
l2hmc_amd/csrc/mcmc_step.hip, its kernel in hmc_step.hip) and of `GaugeSampler.run_hmc`: the declarations and their binding, the workspace query, the
argument checks that must fail before any device call, and what `run_hmc` refuses.  No GPU: plans and arguments carry
any non-NULL address where a pointer is checked, and the sampler runs on stub dynamics that must not be asked for a
plan."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _SZ, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_uint64


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _plan(T=8, X=8, N=10, hmc=1, flags=0):
    return _lib.GaugePlan(T=T, X=X, num_steps=N, hmc=hmc, flags=flags, masks=PTR)


def _run(L, plan, betas=PTR, step_stride=1, chain_stride=0, eps_chain=None, x_in=PTR, x_next=PTR, B=4, n_steps=3,
         sums=None, ws=None, ws_bytes=0, draw0=0):
    return L.l2hmc_gauge_hmc_run_ladder(None if plan is None else C.byref(plan), betas, step_stride, chain_stride,
                                        eps_chain, x_in, x_next, B, 42, draw0, n_steps, None, None, None, None, None,
                                        sums, None, ws, ws_bytes, None)


# ------------------------------------------------------------------------------------------------ the C entries
def test_header_declares_and_binding_matches():
    assert {"l2hmc_gauge_hmc_run_ladder", "l2hmc_gauge_hmc_run_ladder_ws_bytes"} <= set(_lib.declared_symbols())
    assert _lib._PROTOS["l2hmc_gauge_hmc_run_ladder_ws_bytes"] == (_SZ, [C.POINTER(_lib.GaugePlan), _I64, _I32])
    # plan, betas, step_stride, chain_stride, eps_chain, x_in, x_next, B, seed, draw0, n_steps, five histories,
    # step_sums, samples, ws, ws_bytes, stream
    assert _lib._PROTOS["l2hmc_gauge_hmc_run_ladder"] == (
        C.c_int, [C.POINTER(_lib.GaugePlan), _P, _I64, _I64, _P, _P, _P, _I64, _U64, _U64, _I32] + [_P] * 5
        + [_P, _P, _P, _SZ, _P])
    text = header_text()
    assert ("size_t l2hmc_gauge_hmc_run_ladder_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps);"
            in text)
    assert ("int l2hmc_gauge_hmc_run_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t step_stride, "
            "int64_t chain_stride, const float* eps_chain, const float* x_in, float* x_next, int64_t B, uint64_t seed, "
            "uint64_t draw0, int32_t n_steps, float* px, float* actions, float* plaqs, float* charges, "
            "float* charge_diff, float* step_sums, float* samples, void* ws, size_t ws_bytes, "
            "l2hmc_stream_t stream);") in text
    assert "#define L2HMC_ABI_VERSION 1" in text


def test_library_exports_the_entries(L):
    assert L.l2hmc_gauge_hmc_run_ladder is not None and L.l2hmc_gauge_hmc_run_ladder_ws_bytes is not None
    assert L.l2hmc_abi_version() == 1


BIG = dict(T=2, X=513)                                   # 1026 sites: no one-launch kernel


def test_bad_arguments_fail_with_a_message_before_any_device_call(L):
    ok = _plan()
    cases = [(dict(plan=None), "plan is NULL"), (dict(betas=None), "NULL betas"),
             (dict(x_in=None), "NULL x_in / x_next"), (dict(x_next=None), "NULL x_in / x_next"), (dict(plan=_plan(hmc=0)), "hmc = 0"),
             (dict(plan=_plan(**BIG)), "no one-launch kernel"),
             (dict(plan=_plan(flags=_lib.PLAN_LAYERED)), "no one-launch kernel"),
             (dict(n_steps=0), "n_steps = 0"), (dict(n_steps=-3), "n_steps = -3"), (dict(B=-1), "B < 0"),
             (dict(step_stride=-1), "negative stride"), (dict(chain_stride=-1), "negative stride"),
             (dict(step_stride=0, chain_stride=-4, eps_chain=PTR), "negative stride"),
             (dict(draw0=2 ** 63, n_steps=1), "2^63"), (dict(draw0=2 ** 63 - 2, n_steps=3), "2^63"),
             (dict(draw0=2 ** 64 - 1, n_steps=1), "2^63"), (dict(sums=PTR), "step_sums needs the workspace")]
    for kw, word in cases:
        plan = kw.pop("plan", ok)
        rc = _run(L, plan, **kw)
        msg = L.l2hmc_last_error().decode()
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        assert msg.startswith("gauge_hmc_run_ladder: ") and word in msg, (kw, msg)
    # step_sums with a workspace that is too small: the workspace error, still before any launch
    assert _run(L, ok, sums=PTR, ws=PTR, ws_bytes=8) == 3
    assert L.l2hmc_last_error().decode().startswith("gauge_hmc_run_ladder: workspace")
    with pytest.raises(ValueError, match="gauge_hmc_run_ladder: n_steps = 0"):
        _lib.check(_run(L, ok, n_steps=0))


def test_ws_bytes_is_zero_with_the_error_set_for_the_same_arguments(L):
    q = L.l2hmc_gauge_hmc_run_ladder_ws_bytes
    for plan, B, n, word in [(None, 64, 8, "plan is NULL"), (_plan(hmc=0), 64, 8, "hmc = 0"),
                             (_plan(**BIG), 64, 8, "no one-launch kernel"),
                             (_plan(flags=_lib.PLAN_LAYERED), 64, 8, "no one-launch kernel"),
                             (_plan(), 64, 0, "n_steps = 0"), (_plan(), 64, -1, "n_steps = -1"),
                             (_plan(), -1, 8, "B < 0")]:
        _run(L, _plan(), B=0)                          # (a call that succeeds in between)
        assert q(None if plan is None else C.byref(plan), B, n) == 0
        msg = L.l2hmc_last_error().decode()
        assert msg.startswith("gauge_hmc_run_ladder_ws_bytes: ") and word in msg, msg


@pytest.mark.parametrize("T,X", [(3, 5), (8, 8), (16, 20), (32, 32)])
@pytest.mark.parametrize("flags", [0, _lib.PLAN_SELECTED_ONLY])
def test_ws_bytes_of_a_served_plan_is_the_uniform_runs(L, T, X, flags):
    plan = _plan(T, X, flags=flags)
    assert L.l2hmc_gauge_plan_fused(C.byref(plan)) == 1
    for B in (0, 1, 70, 2048, 4097):
        for n in (1, 3, 256):
            got = L.l2hmc_gauge_hmc_run_ladder_ws_bytes(C.byref(plan), B, n)
            assert got == L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(plan), B, n) and got > 0


def test_an_empty_batch_is_a_no_op(L):
    assert _run(L, _plan(), B=0) == 0
    assert _run(L, _plan(), B=0, step_stride=0, chain_stride=1, eps_chain=PTR) == 0
    assert _run(L, _plan(), B=0, draw0=2 ** 63 - 3, n_steps=3) == 0          # the largest draw index accepted
    assert _run(L, _plan(hmc=0), B=0) == 1                # checked before the batch size is looked at
    assert _run(L, _plan(**BIG), B=0) == 1


# ------------------------------------------------------------------------------------------------ run_hmc on stubs
T_, X_, B_ = 3, 5, 4
D_ = 2 * T_ * X_


def _stub(hmc=True, plan=None):
    def _plan_():
        if plan is None:
            raise AssertionError("a refused call must not build a plan")
        return plan
    lat = types.SimpleNamespace(time_size=T_, space_size=X_)
    return types.SimpleNamespace(hmc=hmc, lattice=lat, x_dim=D_, batch_size=B_, num_steps=3, eps=torch.tensor(0.1),
                                 _draws=4, _seed=7, _device=torch.device("cpu"), _plan=_plan_)


def _sampler(dyn):
    import l2hmc_amd as la
    return la.GaugeSampler(dyn)


def test_run_hmc_signature_and_run_unchanged():
    import l2hmc_amd as la
    assert (str(inspect.signature(la.GaugeSampler.run_hmc))
            == "(self, run_steps, beta, x=None, eps=None, keep_samples=False)")
    assert str(inspect.signature(la.GaugeSampler.run)) == "(self, run_steps, beta, x=None, keep_samples=False)"


def test_run_hmc_refuses_an_l2hmc_dynamics_without_a_draw():
    dyn = _stub(hmc=False)
    with pytest.raises(ValueError, match="`run`"):
        _sampler(dyn).run_hmc(5, 2.0, torch.zeros(B_, D_))
    assert dyn._draws == 4


def test_run_hmc_names_run_for_a_plan_without_the_kernel():
    """The plan is looked at on the host alone (l2hmc_gauge_plan_fused): no launch, no draw."""
    dyn = _stub(plan=_plan(T_, X_, 3, flags=_lib.PLAN_LAYERED))
    with pytest.raises(NotImplementedError, match="`run`"):
        _sampler(dyn).run_hmc(5, 2.0, torch.zeros(B_, D_))
    assert dyn._draws == 4


@pytest.mark.parametrize("beta", [[1.0, 2.0], np.ones((5, 3)), np.ones((2, B_)), np.ones((B_,)), np.ones((1, 1, B_)),
                                  np.ones((B_, 1)), -0.5, float("nan"), float("inf"), 1e60, [[1.0, -1.0, 1.0, 1.0]],
                                  [1.0, 2.0, float("nan"), 1.0, 1.0], np.full((5, B_), -1e-3)])
def test_run_hmc_refuses_bad_betas(beta):
    dyn = _stub()
    with pytest.raises(ValueError, match="run_hmc: (beta of shape|every beta)"):
        _sampler(dyn).run_hmc(5, beta, torch.zeros(B_, D_))
    with pytest.raises(ValueError, match="run_hmc: (beta of shape|every beta)"):
        _sampler(dyn).run_hmc(5, torch.tensor(beta, dtype=torch.float64), torch.zeros(B_, D_))
    assert dyn._draws == 4


@pytest.mark.parametrize("eps", [0, 0.0, -0.1, float("inf"), float("nan"), 1e-60, 1e60, [0.1, 0.1, 0.0, 0.1],
                                 [0.1, float("nan"), 0.1, 0.1], [0.1, 0.2, 0.3], [[0.1, 0.2, 0.3, 0.4]],
                                 [[0.1], [0.2], [0.3], [0.4]], [0.1]])
def test_run_hmc_refuses_bad_step_sizes(eps):
    dyn = _stub()
    with pytest.raises(ValueError, match="run_hmc: e"):
        _sampler(dyn).run_hmc(5, 2.0, torch.zeros(B_, D_), eps=eps)
    with pytest.raises(ValueError, match="run_hmc: e"):
        _sampler(dyn).run_hmc(5, 2.0, torch.zeros(B_, D_), eps=torch.tensor(eps, dtype=torch.float64))
    assert dyn._draws == 4


def test_run_hmc_refuses_a_start_of_the_wrong_shape_and_negative_steps():
    dyn = _stub()
    with pytest.raises(ValueError, match="run_hmc: x of shape"):
        _sampler(dyn).run_hmc(5, 2.0, torch.zeros(B_, D_ + 1))
    with pytest.raises(ValueError):
        _sampler(dyn).run_hmc(-1, 2.0, torch.zeros(B_, D_))
    assert dyn._draws == 4


def test_run_hmc_accepts_good_arguments_up_to_the_plan():
    """Every accepted form passes the checks: the call gets as far as the plan (which the stub refuses)."""
    x0 = torch.zeros(B_, D_)
    for beta in (2.0, np.float32(2.0), 0.0, [1.0] * 5, np.ones((1, B_)), np.ones((5, B_)), torch.ones(5, B_)):
        for eps in (None, 0.25, np.float32(0.25), [0.1, 0.2, 0.3, 0.4], torch.tensor([0.1, 0.2, 0.3, 0.4])):
            dyn = _stub()
            with pytest.raises(AssertionError, match="must not build a plan"):
                _sampler(dyn).run_hmc(5, beta, x0, eps=eps)
            assert dyn._draws == 4


def test_beta_shapes_map_to_the_stride_pairs():
    from l2hmc_amd import _runs

    def f(beta, run_steps, B):
        b, flat, (step_stride, chain_stride) = _runs.chain_axis(beta, run_steps, B, who="run_hmc", name="beta",
                                                                positive=False)
        return b, flat, step_stride, chain_stride
    n, B = 5, 3
    b, flat, ss, cs = f(2.5, n, B)
    assert (ss, cs) == (0, 0) and flat.dtype == np.float32 and flat.tolist() == [2.5]
    sched = np.arange(1, n + 1, dtype=np.float64)
    b, flat, ss, cs = f(sched, n, B)
    assert (ss, cs) == (1, 0) and flat.tolist() == sched.tolist()
    lad = np.array([[1.0, 2.5, 4.0]])
    b, flat, ss, cs = f(lad, n, B)
    assert (ss, cs) == (0, 1) and flat.tolist() == [1.0, 2.5, 4.0]
    both = sched[:, None] + 10 * np.arange(B)[None, :]
    b, flat, ss, cs = f(both, n, B)
    assert (ss, cs) == (B, 1) and flat.shape == (n * B,)
    # step s of chain c reads flat[s * step_stride + c * chain_stride]
    assert all(flat[s * ss + c * cs] == both[s, c] for s in range(n) for c in range(B))
    assert b.dtype == np.float64 and np.array_equal(b, both)
    # [1, B] of a one-step run and [n, B] with n = 1 are the same array and the same reads
    assert f(lad, 1, B)[2:] in ((0, 1), (B, 1))
    # a transposed (non-contiguous) view is laid out anew
    b, flat, ss, cs = f(np.asfortranarray(both), n, B)
    assert all(flat[s * ss + c * cs] == both[s, c] for s in range(n) for c in range(B))
    # float32 rounding is the device's: 0.1 goes over as float32(0.1)
    assert f(0.1, n, B)[1][0] == np.float32(0.1)


def test_an_empty_run_returns_empty_histories():
    dyn = _stub()
    x0 = torch.ones(B_, D_)
    out = _sampler(dyn).run_hmc(0, [[1.0, 2.0, 3.0, 4.0]], x0, eps=[0.1, 0.2, 0.3, 0.4], keep_samples=True)
    for k in ("px", "actions", "plaqs", "charges", "charge_diff"):
        assert out[k].shape == (0, B_) and out[k].dtype == np.float32
    assert out["samples"].shape == (0, B_, D_) and torch.equal(out["samples_out"], x0)
    assert out["samples_out"] is not x0 and dyn._draws == 4
    from l2hmc_amd.lattice import u1_plaq_exact
    assert out["plaq_exact"].shape == (B_,) and np.allclose(out["plaq_exact"], u1_plaq_exact(np.arange(1.0, 5.0)))
    out = _sampler(dyn).run_hmc(0, 2.0, x0)
    assert "samples" not in out and isinstance(float(out["plaq_exact"]), float) and np.ndim(out["plaq_exact"]) == 0
    out = _sampler(dyn).run_hmc(0, [], x0)
    assert out["px"].shape == (0, B_)
