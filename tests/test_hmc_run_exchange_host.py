"""Host side of the plain-HMC lattice run with the replica-exchange rounds inside the launch
(l2hmc_gauge_hmc_run_exchange, _served and _ws_bytes in l2hmc_amd/csrc/mcmc_step.hip; the kernel and the served rule in
hmc_step.hip) and of `GaugeSampler.run_hmc_exchange` with `sampler.in_launch = True`: the declarations and their binding, the
served rule on a table of (lattice, directions, group), the argument checks that must fail before any device call, and
the draw accounting against a literal replay of the loop it stands for.  No GPU: plans and arguments carry any non-NULL
address where a pointer is checked."""
import ctypes as C
import inspect
import math
import types

import pytest
import torch

from l2hmc_amd import _lib
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _SZ, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_uint64
NAMES = ("l2hmc_gauge_hmc_run_exchange_served", "l2hmc_gauge_hmc_run_exchange_ws_bytes", "l2hmc_gauge_hmc_run_exchange")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _plan(T=8, X=8, N=10, hmc=1, flags=0):
    return _lib.GaugePlan(T=T, X=X, num_steps=N, hmc=hmc, flags=flags, masks=PTR)


def _run(L, plan, betas=PTR, step_stride=0, chain_stride=1, eps_chain=None, x_in=PTR, x_next=PTR, B=8, n_steps=3,
         group=4, swap_every=1, swap_phase=0, first_parity=0, sums=None, ws=None, ws_bytes=0, draw0=0):
    return L.l2hmc_gauge_hmc_run_exchange(None if plan is None else C.byref(plan), betas, step_stride, chain_stride,
                                          eps_chain, x_in, x_next, B, 42, draw0, n_steps, group, swap_every, swap_phase,
                                          first_parity, None, None, None, None, None, None, sums, None, None, None,
                                          None, ws, ws_bytes, None)


# ------------------------------------------------------------------------------------------------ the C entries
def test_header_declares_and_binding_matches():
    assert set(NAMES) <= set(_lib.declared_symbols())
    plan_p = C.POINTER(_lib.GaugePlan)
    assert _lib._PROTOS[NAMES[0]] == (C.c_int, [plan_p, _I32])
    assert _lib._PROTOS[NAMES[1]] == (_SZ, [plan_p, _I64, _I32])
    # plan, betas, step_stride, chain_stride, eps_chain, x_in, x_next, B, seed, draw0, n_steps, group, swap_every,
    # swap_phase, first_parity, replica, five histories, step_sums, samples, three round histories, ws, ws_bytes, stream
    assert _lib._PROTOS[NAMES[2]] == (
        C.c_int, [plan_p, _P, _I64, _I64, _P, _P, _P, _I64, _U64, _U64, _I32] + [_I32] * 4 + [_P] + [_P] * 5
        + [_P, _P] + [_P] * 3 + [_P, _SZ, _P])
    text = header_text()
    assert "int l2hmc_gauge_hmc_run_exchange_served(const l2hmc_gauge_plan* plan, int32_t group);" in text
    assert ("size_t l2hmc_gauge_hmc_run_exchange_ws_bytes(const l2hmc_gauge_plan* plan, int64_t B, int32_t n_steps);"
            in text)
    assert ("int l2hmc_gauge_hmc_run_exchange(const l2hmc_gauge_plan* plan, const float* betas, int64_t step_stride, "
            "int64_t chain_stride, const float* eps_chain, const float* x_in, float* x_next, int64_t B, uint64_t seed, "
            "uint64_t draw0, int32_t n_steps, int32_t group, int32_t swap_every, int32_t swap_phase, "
            "int32_t first_parity, int32_t* replica, float* px, float* actions, float* plaqs, float* charges, "
            "float* charge_diff, float* step_sums, float* samples, float* swap_p, uint8_t* swapped, "
            "int32_t* replica_hist, void* ws, size_t ws_bytes, l2hmc_stream_t stream);") in text
    assert "#define L2HMC_ABI_VERSION 1" in text
    # the header states the served rule and the stream accounting
    doc = header_text(comments=True)
    assert "lcm(group, cpw0) * rpc * tpc <= 1024" in doc and "stream 2 d + 3 is skipped" in doc


def test_library_exports_the_entries(L):
    for name in NAMES:
        assert getattr(L, name) is not None


# ------------------------------------------------------------------------------------------------ the served rule
SEL = _lib.PLAN_SELECTED_ONLY
SERVED = ([(8, 8, 0, G) for G in (2, 3, 4, 8)] + [(8, 8, SEL, G) for G in (2, 3, 4, 8, 16)]
          + [(3, 5, 0, 4), (6, 6, 0, 3), (8, 16, 0, 2), (8, 16, 0, 4), (16, 16, 0, 2), (16, 32, 0, 2),
             (16, 16, SEL, 4), (16, 32, SEL, 4)])
BIG = dict(T=2, X=513)                                   # 1026 sites: no one-launch kernel
UNSERVED = [(dict(T=1, X=1), 3, "of LDS"), (dict(T=0, X=8), 2, "bad lattice"),
            (dict(T=8, X=8), 16, "more than 1024"), (dict(T=8, X=8), 5, "more than 1024"),
            (BIG, 2, "more than 1024 sites"), (dict(hmc=0), 2, "hmc = 0"),
            (dict(flags=_lib.PLAN_LAYERED), 2, "L2HMC_PLAN_LAYERED"), (dict(T=8, X=8), 1, "2 rungs or more"),
            (dict(T=16, X=16), 3, "more than 1024"), (dict(T=16, X=16), 4, "more than 1024")]


def _rule(T, X, flags, G):
    """The served rule restated: lcm(G, cpw0) * rpc * tpc <= 1024 on a lattice of at most 512 sites, in 64 KiB of LDS."""
    sites = T * X
    if sites > 512:
        return False
    spt = 1 if sites <= 256 else 2
    tpc = 1 << max(0, math.ceil(math.log2(-(-sites // spt))))
    rpc = 1 if flags & SEL else 2
    cpw0 = (512 if tpc == 256 else 256) // tpc // rpc
    rows = math.lcm(G, cpw0) * rpc
    # per row: x and v planes and sin P (5 floats per site), 18 words of scratch; the sum tree [2][256]
    return rows * tpc <= 1024 and 4 * (rows * (5 * sites + 18) + 512) <= 64 * 1024


@pytest.mark.parametrize("T,X,flags,G", SERVED)
def test_served_shapes(L, T, X, flags, G):
    assert L.l2hmc_gauge_hmc_run_exchange_served(C.byref(_plan(T, X, flags=flags)), G) == 1
    assert _rule(T, X, flags, G)
    assert _run(L, _plan(T, X, flags=flags), B=0, group=G) == 0           # the entry agrees (an empty batch: no launch)


@pytest.mark.parametrize("kw,G,word", UNSERVED)
def test_unserved_shapes_say_why(L, kw, G, word):
    plan = _plan(**kw)
    assert L.l2hmc_gauge_hmc_run_exchange_served(C.byref(plan), G) == 0
    msg = L.l2hmc_last_error().decode()
    assert msg.startswith("gauge_hmc_run_exchange_served: ") and word in msg, msg
    assert _run(L, plan, B=0, group=G) == 1                               # checked before the batch size is looked at


def test_served_follows_the_rule_on_a_grid(L):
    assert L.l2hmc_gauge_hmc_run_exchange_served(None, 2) == 0
    for T, X in [(1, 1), (1, 2), (2, 2), (2, 4), (3, 5), (4, 4), (6, 6), (8, 8), (5, 13), (8, 16), (10, 20), (16, 16), (16, 20), (16, 32),
                 (20, 30), (32, 32)]:
        for flags in (0, SEL):
            for G in range(2, 40):
                got = L.l2hmc_gauge_hmc_run_exchange_served(C.byref(_plan(T, X, flags=flags)), G)
                assert got == int(_rule(T, X, flags, G)), (T, X, flags, G)
    # 32x32, four sites per thread: the instance is not shipped
    assert L.l2hmc_gauge_hmc_run_exchange_served(C.byref(_plan(32, 32)), 2) == 0
    assert "sites per thread" in L.l2hmc_last_error().decode()


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_fail_with_a_message_before_any_device_call(L):
    ok = _plan()
    cases = [(dict(plan=None), "plan is NULL"), (dict(betas=None), "NULL betas"),
             (dict(x_in=None), "NULL x_in / x_next"), (dict(x_next=None), "NULL x_in / x_next"),
             (dict(plan=_plan(hmc=0)), "hmc = 0"), (dict(plan=_plan(**BIG)), "no one-launch kernel"),
             (dict(plan=_plan(flags=_lib.PLAN_LAYERED)), "no one-launch kernel"),
             (dict(n_steps=0), "n_steps = 0"), (dict(n_steps=-3), "n_steps = -3"), (dict(B=-1), "B < 0"),
             (dict(step_stride=-1), "negative stride"), (dict(chain_stride=-1), "negative stride"),
             (dict(group=1), "2 rungs or more"), (dict(group=0), "2 rungs or more"), (dict(group=-4), "2 rungs or more"),
             (dict(B=10, group=4), "not a multiple of group"), (dict(B=9, group=2), "not a multiple of group"),
             (dict(swap_every=0), "swap_every = 0"), (dict(swap_every=-1), "swap_every = -1"),
             (dict(swap_every=3, swap_phase=3), "swap_phase = 3"), (dict(swap_phase=-1), "swap_phase = -1"),
             (dict(swap_phase=1), "swap_phase = 1"),
             (dict(first_parity=2), "first_parity = 2"), (dict(first_parity=-1), "first_parity = -1"),
             (dict(B=16, group=16), "not served"), (dict(B=10, group=5), "not served"),
             (dict(plan=_plan(32, 32), group=2), "not served"),
             (dict(draw0=2 ** 63, n_steps=1), "2^63"), (dict(draw0=2 ** 63 - 5, n_steps=3), "2^63"),
             (dict(draw0=2 ** 63 - 3, n_steps=3, swap_every=3), "2^63"),
             (dict(draw0=2 ** 63 - 2, n_steps=2, swap_every=2, swap_phase=1), "2^63"),
             (dict(draw0=2 ** 64 - 1, n_steps=1), "2^63"), (dict(sums=PTR), "step_sums needs the workspace")]
    for kw, word in cases:
        plan = kw.pop("plan", ok)
        rc = _run(L, plan, **kw)
        msg = L.l2hmc_last_error().decode()
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        assert msg.startswith("gauge_hmc_run_exchange: ") and word in msg, (kw, msg)
    assert _run(L, ok, sums=PTR, ws=PTR, ws_bytes=8) == 3
    assert L.l2hmc_last_error().decode().startswith("gauge_hmc_run_exchange: workspace")


def test_an_empty_batch_is_a_no_op_and_the_draw_bound_counts_the_rounds(L):
    assert _run(L, _plan(), B=0) == 0
    # 3 steps and 3 rounds from draw0: draw0 + 6 <= 2^63
    assert _run(L, _plan(), B=0, draw0=2 ** 63 - 6, n_steps=3) == 0
    assert _run(L, _plan(), B=0, draw0=2 ** 63 - 5, n_steps=3) == 1
    # 3 steps, one round every 4 steps, phase 0: no round
    assert _run(L, _plan(), B=0, draw0=2 ** 63 - 3, n_steps=3, swap_every=4) == 0
    assert _run(L, _plan(), B=0, draw0=2 ** 63 - 3, n_steps=3, swap_every=4, swap_phase=1) == 1      # one round


def test_ws_bytes_is_the_ladder_runs(L):
    for T, X in [(3, 5), (8, 8), (16, 32)]:
        plan = _plan(T, X)
        for B in (0, 8, 72, 2048):
            for n in (1, 5, 256):
                got = L.l2hmc_gauge_hmc_run_exchange_ws_bytes(C.byref(plan), B, n)
                assert got == L.l2hmc_gauge_hmc_run_ladder_ws_bytes(C.byref(plan), B, n) and got > 0
    assert L.l2hmc_gauge_hmc_run_exchange_ws_bytes(C.byref(_plan(hmc=0)), 8, 4) == 0
    assert L.l2hmc_last_error().decode().startswith("gauge_hmc_run_exchange_ws_bytes: ")


# ------------------------------------------------------------------------------------------------ the draw accounting
def _replay(draws, n, k, phase):
    """The loop itself: `step_draw_index` per step, `_draws += 1` per round."""
    first, rounds = None, 0
    for s in range(n):
        d, draws = _lib.step_draw_index(draws)
        first = d if first is None else first
        if (phase + s + 1) % k == 0:
            draws += 1
            rounds += 1
    return first, rounds, draws


def test_draw_helper_is_the_replay_of_the_loop():
    for k in range(1, 6):
        for n in range(1, 8):
            for phase in range(k):
                for draws in (0, 1, 4, 7, 1001):
                    assert _lib.exchange_run_draw_index(draws, n, k, phase) == _replay(draws, n, k, phase), (k, n, phase)


def test_chunks_of_a_run_chain_as_the_uncut_loop():
    """Chunks of any length, each starting at phase s0 % k from where the last one left the counter."""
    for k in range(1, 6):
        for chunk in range(1, 8):
            for total in (12, 13):
                draws, s0, starts = 4, 0, []
                while s0 < total:
                    n = min(chunk, total - s0)
                    d0, _, draws = _lib.exchange_run_draw_index(draws, n, k, s0 % k)
                    starts.append(d0)
                    s0 += n
                # the uncut loop, step by step
                ref, want, s0 = 4, [], 0
                for s in range(total):
                    d, ref = _lib.step_draw_index(ref)
                    if s % chunk == 0:
                        want.append(d)
                    if (s + 1) % k == 0:
                        ref += 1
                assert (starts, draws) == (want, ref), (k, chunk, total)


# ------------------------------------------------------------------------------------------------ the sampler
def test_signatures():
    import l2hmc_amd as la
    assert (str(inspect.signature(la.GaugeSampler.run_hmc_exchange))
            == "(self, run_steps, beta, x=None, eps=None, keep_samples=False, replicas=None, swap_every=1, "
               "first_parity=0, replica0=None)")            # unchanged: the switch is an attribute of the sampler
    assert str(inspect.signature(la.GaugeSampler.exchange_in_launch)) == "(self, replicas)"
    assert la.GaugeSampler(_stub(8, 8, 16)).in_launch is False        # the default stays the round between launches


def _stub(T, X, B, flags=0):
    lat = types.SimpleNamespace(time_size=T, space_size=X)
    return types.SimpleNamespace(hmc=True, lattice=lat, x_dim=2 * T * X, batch_size=B, num_steps=3,
                                 eps=torch.tensor(0.1), _draws=4, _seed=7, _device=torch.device("cpu"),
                                 _plan=lambda: _plan(T, X, 3, flags=flags))


def test_sampler_query_and_refusal_without_a_launch():
    import l2hmc_amd as la
    smp = la.GaugeSampler(_stub(8, 8, 16))
    assert smp.exchange_in_launch(8) is True and smp.exchange_in_launch(16) is False
    assert smp.exchange_in_launch(1) is False and smp.exchange_in_launch(2.5) is False
    assert la.GaugeSampler(_stub(8, 8, 16, SEL)).exchange_in_launch(16) is True
    assert la.GaugeSampler(_stub(32, 32, 4)).exchange_in_launch(2) is False
    for T, X, B, G in [(8, 8, 16, 16), (32, 32, 4, 2)]:
        dyn = _stub(T, X, B)
        smp = la.GaugeSampler(dyn)
        smp.in_launch = True
        with pytest.raises(NotImplementedError, match="exceed 1024"):
            smp.run_hmc_exchange(4, [[1.0 + c for c in range(B)]], torch.zeros(B, 2 * T * X), replicas=G)
        assert dyn._draws == 4 and smp.replica is None
