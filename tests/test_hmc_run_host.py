"""Host side of the plain-HMC run entry (l2hmc_gauge_hmc_run in l2hmc_amd/csrc/mcmc_step.hip, its kernel in hmc_step.hip): its declaration and
binding, its workspace query, the argument checks that must fail before any device call, and the draw counter of a
run.  No GPU: the plans and arguments carry any non-NULL address where a pointer is checked."""
import ctypes as C

import pytest

from l2hmc_amd import _lib
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _SZ, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_uint64


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _plan(T=8, X=8, N=10, hmc=1, flags=0):
    return _lib.GaugePlan(T=T, X=X, num_steps=N, hmc=hmc, flags=flags, masks=PTR)


def _run(L, plan, betas=PTR, x_in=PTR, x_next=PTR, B=4, n_steps=3, sums=None, ws=None, ws_bytes=0, draw0=0):
    return L.l2hmc_gauge_hmc_run(C.byref(plan), betas, x_in, x_next, B, 42, draw0, n_steps, None, None, None, None, None,
                                 sums, None, ws, ws_bytes, None)


def test_header_declares_and_binding_matches():
    assert {"l2hmc_gauge_hmc_run", "l2hmc_gauge_hmc_run_ws_bytes"} <= set(_lib.declared_symbols())
    assert _lib._PROTOS["l2hmc_gauge_hmc_run_ws_bytes"] == (_SZ, [C.POINTER(_lib.GaugePlan), _I64, _I32])
    # plan, betas, x_in, x_next, B, seed, draw0, n_steps, five histories, step_sums, samples, ws, ws_bytes, stream
    assert _lib._PROTOS["l2hmc_gauge_hmc_run"] == (
        C.c_int, [C.POINTER(_lib.GaugePlan), _P, _P, _P, _I64, _U64, _U64, _I32] + [_P] * 5 + [_P, _P, _P, _SZ, _P])
    text = header_text(comments=True)
    assert ("int l2hmc_gauge_hmc_run(const l2hmc_gauge_plan* plan, const float* betas, const float* x_in, "
            "float* x_next, int64_t B, uint64_t seed, uint64_t draw0, int32_t n_steps, float* px, float* actions, "
            "float* plaqs, float* charges, float* charge_diff, float* step_sums, float* samples, void* ws, "
            "size_t ws_bytes, l2hmc_stream_t stream);") in text
    assert "size_t l2hmc_gauge_hmc_run_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps);" in text


def test_library_exports_the_entries(L):
    assert L.l2hmc_gauge_hmc_run is not None and L.l2hmc_gauge_hmc_run_ws_bytes is not None


@pytest.mark.parametrize("T,X", [(3, 5), (8, 8), (16, 16), (32, 32)])
@pytest.mark.parametrize("flags", [0, _lib.PLAN_SELECTED_ONLY])
def test_ws_bytes_of_a_fused_plan_is_positive_and_monotone(L, T, X, flags):
    plan = _plan(T, X, flags=flags)
    assert L.l2hmc_gauge_plan_fused(C.byref(plan)) == 1
    q = lambda B, n: L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(plan), B, n)
    for B in (1, 70, 2048):
        sizes = [q(B, n) for n in (1, 2, 16, 256)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == 4
        # per step: 2 floats for each of at most B workgroups
        assert sizes[0] >= 8 * B and sizes[3] == 256 * sizes[0]
    for n in (1, 16):
        sizes = [q(B, n) for B in (1, 70, 2048, 4097)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[1] < sizes[2] < sizes[3]


def test_ws_bytes_of_an_unfused_hmc_plan_is_the_loops(L):
    plan = _plan(6, 6, flags=_lib.PLAN_LAYERED)
    assert L.l2hmc_gauge_plan_fused(C.byref(plan)) == 0
    step = L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), 9)
    assert L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(plan), 9, 1) >= step
    assert L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(plan), 9, 1) == L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(plan), 9, 50)


def test_ws_bytes_is_zero_with_a_message_for_network_plans(L):
    """Documented in the header: 0, and l2hmc_last_error says that the plan is not plain HMC."""
    assert L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(_plan(hmc=0)), 64, 8) == 0
    assert "hmc = 0" in L.l2hmc_last_error().decode()
    assert L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(_plan()), 64, 0) == 0
    assert L.l2hmc_gauge_hmc_run_ws_bytes(None, 64, 8) == 0


def test_bad_arguments_fail_with_a_message_before_any_device_call(L):
    ok = _plan()
    cases = [(dict(plan=_plan(hmc=0)), "hmc = 0"), (dict(n_steps=0), "n_steps"), (dict(n_steps=-3), "n_steps"),
             (dict(betas=None), "betas"), (dict(x_in=None), "x_in"), (dict(x_next=None), "x_in"),
             (dict(sums=PTR), "workspace")]
    for kw, word in cases:
        plan = kw.pop("plan", ok)
        rc = _run(L, plan, **kw)
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        assert word in L.l2hmc_last_error().decode(), (kw, L.l2hmc_last_error().decode())
    # step_sums with a workspace that is too small: the workspace error, still before any launch
    assert _run(L, ok, sums=PTR, ws=PTR, ws_bytes=8) == 3
    assert "workspace" in L.l2hmc_last_error().decode()
    with pytest.raises(ValueError):
        _lib.check(_run(L, ok, n_steps=0))


@pytest.mark.parametrize("start", [0, 1, 4, 7])
@pytest.mark.parametrize("n", [1, 5])
def test_run_draw_counter_is_that_of_n_steps(start, n):
    draws, idx = start, []
    for _ in range(n):
        d, draws = _lib.step_draw_index(draws)
        idx.append(d)
    d0, after = _lib.run_draw_index(start, n)
    assert idx == list(range(d0, d0 + n))
    assert after == draws == 2 * (d0 + n - 1) + 2


def test_draw_indices_must_stay_below_2_to_the_63(L):
    """The run kernel uses bit 63 of a step's draw index as a zero; the host refuses, before any launch, a run whose
    last draw index draw0 + n_steps - 1 would reach 2^63.  B = 0 makes the largest accepted value a host-only call."""
    for plan in (_plan(), _plan(flags=_lib.PLAN_LAYERED)):
        for draw0, n in ((2 ** 63, 1), (2 ** 63 - 2, 3), (2 ** 64 - 1, 1), (2 ** 63 - 255, 256)):
            assert _run(L, plan, draw0=draw0, n_steps=n) == 1, (draw0, n)
            assert "2^63" in L.l2hmc_last_error().decode()
        assert _run(L, plan, draw0=2 ** 63 - 3, n_steps=3, B=0) == 0
        assert _run(L, plan, draw0=2 ** 63 - 256, n_steps=256, B=0) == 0
