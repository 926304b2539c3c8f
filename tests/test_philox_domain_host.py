"""Host side of the (seed, stream) domain tests (tests/test_gpu_philox_domain.py): the reference generator of
tests/philox_ref.py against Random123's known answers, the proof that every corner of tests/philox_cases.py can tell a
generator that keeps a high word from one that drops it, the refusals of draw indices whose streams would wrap, and the
accept condition of every lattice case the GPU test compares with the float64 oracle.  No GPU: plans and arguments carry
any non-NULL address where a pointer is checked."""
import ctypes as C

import numpy as np
import pytest

from l2hmc_amd import _lib
from tests import philox_cases as PC
from tests import philox_ref as R
from tests.run_cases import PTR


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the reference
def test_random123_known_answers():
    """kat_vectors of Random123 (philox4x32 10): counter and key zero, all ones, and the digits of pi."""
    ones = 0xFFFFFFFF
    assert R.philox_raw([0] * 4, [0] * 2) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert R.philox_raw([ones] * 4, [ones] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert R.philox_raw([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # the (block, stream, seed) form places the words as the kernels do
    assert R.philox(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert R.philox(0x85a308d3243f6a88, 0x0370734413198a2e, 0x299f31d0a4093822) == [
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_array_form_equals_the_integer_form():
    for seed in PC.SEEDS:
        for stream in PC.FILL_STREAMS + (0, 77):
            idx = np.array([0, 1, 2, 3, 4, 5, 1001, PC.FILL_N - 1])
            w = R.word(seed, stream, idx)
            assert [int(v) for v in w] == [R.philox(int(i) >> 2, stream, seed)[int(i) & 3] for i in idx]
            u = R.uniform(seed, stream, idx)
            assert u.dtype == np.float32
            assert all(u[k] == np.float32((int(w[k]) >> 8) * 2.0 ** -24) for k in range(len(idx)))
    with pytest.raises(ValueError):
        R.uniform(2 ** 64, 0, 0)
    with pytest.raises(ValueError):
        R.uniform(0, -1, 0)
    with pytest.raises(ValueError):
        R.lattice_step_streams(2 ** 63)


def test_normal_is_box_muller_on_the_devices_float32_uniforms():
    """Words whose upper 24 bits are 2^23 or more: the sum with 0.5 rounds to even, the top word gives u = 1.0 exactly.
    The reference keeps that (u1 = 1 -> radius 0; u2 = 1 -> angle 2 pi)."""
    w = np.array([0, 1 << 8, (2 ** 23 - 1) << 8, 2 ** 23 << 8, (2 ** 23 + 1) << 8, 0xFFFFFFFF], dtype=np.uint64)
    u = R._u01_open(w)
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -25) and u[1] == np.float32(1.5 * 2.0 ** -24)
    assert u[2] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)              # the last word whose + 0.5 is exact
    assert u[3] == np.float32(0.5) and u[4] == np.float32((2 ** 23 + 2) * 2.0 ** -24) and u[5] == np.float32(1.0)
    seed, stream = PC.SEED_HIGH, 2 ** 63
    z = R.normals(seed, stream, 64)
    for i in (0, 1, 2, 3, 37, 62):
        c = R.philox(i >> 2, stream, seed)
        h = (i & 3) >> 1
        u1, u2 = (float(R._u01_open(np.array([c[2 * h + k]], dtype=np.uint64))[0]) for k in (0, 1))
        rad = np.sqrt(-2.0 * np.log(u1))
        want = rad * np.sin(2 * np.pi * u2) if i & 1 else rad * np.cos(2 * np.pi * u2)
        assert abs(z[i] - want) <= 1e-14 * max(1.0, abs(want))             # (array and scalar libm may differ by an ulp)
    assert np.abs(R.normals(seed, stream, PC.FILL_N)).max() <= 5.9      # u1 >= 2^-25
    assert z.dtype == np.float64


def test_layouts():
    seed, B, D = PC.SEED_HIGH, 3, 8
    vf, vb, coin, u = R.lattice_step(seed, 2 ** 31, B, D)
    assert vf.shape == vb.shape == (B, D) and coin.shape == u.shape == (B,)
    assert vb[1, 2] == R.normal(seed, 2 ** 32, (B + 1) * D + 2) and u[2] == R.uniform(seed, 2 ** 32 + 1, B + 2)
    assert coin[0] == R.uniform(seed, 2 ** 32 + 1, 0)
    bits, wf, wb, mh = R.toy_step(seed, 2 ** 32 - 6, 1, B, 3)
    assert bits[2] == R.uniform(seed, 2 ** 32 - 2, 2) and wf[1, 2] == R.normal(seed, 2 ** 32 - 1, 5)
    assert wb[2, 0] == R.normal(seed, 2 ** 32, 6) and mh[1] == R.uniform(seed, 2 ** 32 + 1, 1)
    v, mh = R.toy_hmc_step(seed, 2 ** 64 - 7, 2, B, 3)
    assert v[2, 2] == R.normal(seed, 2 ** 64 - 3, 8) and mh[0] == R.uniform(seed, 2 ** 64 - 2, 0)
    # one stream counter: a step the next even-aligned pair, a round the next stream (include/l2hmc_hip.h)
    steps, rounds = R.lattice_run_draws(10, 4, swap_every=2)
    assert steps == [10, 11, 13, 14] and rounds == [24, 30]
    for draw0, k, phase, n in ((5, 3, 1, 7), (2 ** 31 - 3, 2, 0, 4)):
        steps, rounds = R.lattice_run_draws(draw0, n, k, phase)
        d0, n_rounds, after = _lib.exchange_run_draw_index(2 * draw0, n, k, phase)
        assert d0 == steps[0] and n_rounds == len(rounds)
        assert after == (rounds[-1] + 1 if (phase + n) % k == 0 else 2 * steps[-1] + 2)
    assert R.lattice_run_draws(7, 3) == ([7, 8, 9], [])
    steps, rounds = R.toy_hmc_run_streams(100, 4, swap_every=2)
    assert steps == [(100, 101), (102, 103), (105, 106), (107, 108)] and rounds == [104, 109]
    # the largest permitted values stay inside 64 bits, one more does not
    R.lattice_run_draws(PC.EXCHANGE_DRAW0[1], PC.RUN_STEPS, PC.EXCHANGE_EVERY)
    R.toy_hmc_run_streams(PC.TOY_EXCHANGE_DRAW0[1], PC.TOY_EXCHANGE_STEPS, PC.TOY_EXCHANGE_EVERY)
    for fn, args in ((R.lattice_run_draws, (PC.EXCHANGE_DRAW0[1] + 1, PC.RUN_STEPS, PC.EXCHANGE_EVERY)),
                     (R.toy_hmc_run_streams, (PC.TOY_EXCHANGE_DRAW0[1] + 2, PC.TOY_EXCHANGE_STEPS,
                                              PC.TOY_EXCHANGE_EVERY)),
                     (R.toy_step, (seed, 2 ** 64 - 3, 0, B, 2))):
        with pytest.raises(ValueError):
            fn(*args)


# ------------------------------------------------------------------------------------------------ truncated twins
def _differ(a, b):
    """Two sets of draws have nothing to do with each other: no element in common but by chance (8 or more uniforms of
    24 bits: at most one coincidence is allowed for)."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.shape == b.shape and a.size >= 8 and (a == b).sum() <= 1


def test_fill_corners_differ_from_their_truncated_twins():
    idx = np.arange(16)
    twins = 0
    for seed in PC.SEEDS:
        for stream in PC.FILL_STREAMS:
            u, z = R.uniform(seed, stream, idx), R.normal(seed, stream, idx)
            for s2 in PC.truncated_seeds(seed):
                assert _differ(u, R.uniform(s2, stream, idx)) and _differ(z, R.normal(s2, stream, idx)), (seed, stream)
                twins += 1
            for t2 in PC.truncated_streams(stream):
                assert _differ(u, R.uniform(seed, t2, idx)) and _differ(z, R.normal(seed, t2, idx)), (seed, stream)
                twins += 1
            # the high stream word in the block's high word instead (counter words 1 and 3 exchanged)
            if stream >> 32:
                moved = [R.philox((stream >> 32) << 32 | b, stream & R.M32, seed) for b in range(4)]
                assert _differ(R.word(seed, stream, idx), np.array(moved).reshape(-1)), (seed, stream)
    assert twins == 2 * 5 + 3 * 4          # two seeds with a high word, four streams with one
    assert PC.truncated_seeds(PC.SEED_SMALL) == [] and PC.truncated_streams(2 ** 32 - 1) == []


def test_step_corners_differ_from_their_truncated_twins():
    seed, B, D = PC.SEED_HIGH, 3, 8
    flat = lambda draws: np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in draws])
    for draw in PC.STEP_DRAWS + PC.RUN_DRAW0 + PC.EXCHANGE_DRAW0:
        for s in range(PC.RUN_STEPS if draw in PC.RUN_DRAW0 else 1):
            d = draw + s
            got = flat(R.lattice_step(seed, d, B, D))
            assert _differ(got, flat(R.lattice_step(seed & R.M32, d, B, D))), d
            for d2 in PC.truncated_draws(d):
                assert _differ(got, flat(R.lattice_step(seed, d2, B, D))), d
            for k, st in enumerate(R.lattice_step_streams(d)):
                for t2 in PC.truncated_streams(st):
                    fn = (R.normal, R.uniform)[k]
                    assert _differ(fn(seed, st, np.arange(16)), fn(seed, t2, np.arange(16))), d
    # 2^31 - 1 is the last draw whose streams fit 32 bits, 2^31 the first one whose twin exists
    assert PC.truncated_draws(2 ** 31 - 1) == [] and PC.truncated_draws(2 ** 31) == [0]
    assert PC.truncated_draws(2 ** 63 - 1) == [2 ** 31 - 1]
    steps, rounds = R.lattice_run_draws(PC.RUN_DRAW0[0], PC.RUN_STEPS)
    assert [R.lattice_step_streams(d)[0] >> 32 for d in steps] == [0, 0, 1, 1]       # the carry inside one launch
    steps, rounds = R.lattice_run_draws(PC.EXCHANGE_DRAW0[0], PC.RUN_STEPS, PC.EXCHANGE_EVERY)
    assert [2 * d >> 32 for d in steps] == [0, 0, 1, 1] and [r >> 32 for r in rounds] == [0, 1]
    steps, rounds = R.lattice_run_draws(PC.EXCHANGE_DRAW0[1], PC.RUN_STEPS, PC.EXCHANGE_EVERY)
    assert rounds[-1] == 2 ** 64 - 2 and steps[-1] == 2 ** 63 - 2


def test_toy_corners_differ_from_their_truncated_twins():
    seed, B = PC.SEED_HIGH, 5
    flat = lambda draws: np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in draws])
    starts = [(d, 1) for d in PC.TOY_PROPOSE_DRAW0] + list(PC.TOY_RUN)
    for draw0, n in starts:
        for s in range(n):
            got = R.toy_step(seed, draw0, s, B, 3)
            twin = R.toy_step(seed & R.M32, draw0, s, B, 3)
            assert all(_differ(flat([g]), flat([t])) for g, t in zip(got[1:3], twin[1:3])), (draw0, s)
            assert _differ(flat(got), flat(twin))
            for k in range(4):
                st = draw0 + 4 * s + k
                for t2 in PC.truncated_streams(st):
                    assert _differ(R.normal(seed, st, np.arange(16)), R.normal(seed, t2, np.arange(16)))
                    assert _differ(R.uniform(seed, st, np.arange(16)), R.uniform(seed, t2, np.arange(16)))
    # each start has streams on both sides of 2^32, or ends on the last stream there is
    assert [(d + k) >> 32 for d in PC.TOY_PROPOSE_DRAW0[:1] for k in range(4)] == [0, 0, 1, 1]
    assert PC.TOY_PROPOSE_DRAW0[1] + 3 == 2 ** 64 - 1
    assert PC.TOY_RUN[1][0] + 4 * PC.TOY_RUN[1][1] == 2 ** 64 - 1          # l2hmc_small_run's own limit
    assert [(PC.TOY_RUN[0][0] + k) >> 32 for k in (0, 5, 6, 11)] == [0, 0, 1, 1]
    for (draw0, n), last in zip(PC.TOY_HMC_RUN, (2 ** 32 + 2, 2 ** 64 - 2)):
        steps, _ = R.toy_hmc_run_streams(draw0, n)
        assert steps[-1][1] == last
        for s in range(n):
            got, twin = R.toy_hmc_step(seed, draw0, s, B, 3), R.toy_hmc_step(seed & R.M32, draw0, s, B, 3)
            assert _differ(flat(got), flat(twin))
    steps, rounds = R.toy_hmc_run_streams(PC.TOY_EXCHANGE_DRAW0[1], PC.TOY_EXCHANGE_STEPS, PC.TOY_EXCHANGE_EVERY)
    assert rounds[-1] == 2 ** 64 - 2          # draw0 + 2 n_steps + rounds = 2^64 - 1 is the entry's own limit
    steps, rounds = R.toy_hmc_run_streams(PC.TOY_EXCHANGE_DRAW0[0], PC.TOY_EXCHANGE_STEPS, PC.TOY_EXCHANGE_EVERY)
    assert rounds == [2 ** 32 - 1, 2 ** 32 + 4] and steps[0][0] == 2 ** 32 - 5 and steps[-1][1] == 2 ** 32 + 3
    for st in PC.SWAP_STREAMS:
        assert _differ(R.uniform(seed, st, np.arange(16)), R.uniform(seed, st & R.M32, np.arange(16)))
        assert _differ(R.uniform(seed, st, np.arange(16)), R.uniform(seed & R.M32, st, np.arange(16)))


# ------------------------------------------------------------------------------------------------ refusals
def _gauge_plan(T=8, X=8, hmc=0, flags=0):
    return _lib.GaugePlan(T=T, X=X, num_steps=3, hmc=hmc, flags=flags, masks=PTR)


def _step(L, plan, B, draw):
    return L.l2hmc_gauge_mcmc_step(C.byref(plan), 2.0, PTR, B, 42, draw, None, None, None, None, None, PTR, 0, None)


def _step_ex(L, plan, B, draw):
    return L.l2hmc_gauge_mcmc_step_ex(C.byref(plan), 2.0, PTR, PTR, B, 42, draw, None, None, None, None, None, None, PTR,
                                      0, None)


def _step_ladder(L, plan, B, draw):
    return L.l2hmc_gauge_mcmc_step_ladder(C.byref(plan), PTR, 1, PTR, PTR, B, 42, draw, None, None, None, None, None,
                                          None, PTR, 0, None)


def _transition_draw(L, plan, B, draw):
    return L.l2hmc_gauge_transition_draw(C.byref(plan), 2.0, PTR, B, 42, draw, PTR, PTR, PTR, PTR, PTR, 0, None)


@pytest.mark.parametrize("entry,name", [(_step, "gauge_mcmc_step"), (_step_ex, "gauge_mcmc_step"),
                                        (_step_ladder, "gauge_mcmc_step_ladder"),
                                        (_transition_draw, "gauge_transition_draw")])
def test_lattice_step_entries_refuse_a_draw_of_2_to_the_63_or_more(L, entry, name):
    """2 * draw would wrap and the step would replay the streams of draw - 2^63.  Refused before any device call and
    before the B == 0 return, as the run entries refuse it; the message names the entry and the value.  The largest
    permitted draw passes the check: B == 0 is then a no-op, and with B > 0 the call gets as far as the workspace check
    (0 bytes given), which still precedes every launch."""
    plans = [_gauge_plan(), _gauge_plan(flags=_lib.PLAN_LAYERED), _gauge_plan(6, 6)]
    if entry is not _step_ladder:
        plans.append(_gauge_plan(hmc=1))
    for plan in plans:
        for B in (0, 4):
            for draw in (2 ** 63, 2 ** 63 + 5, 2 ** 64 - 1):
                assert entry(L, plan, B, draw) == 1, (B, draw)             # L2HMC_ERR_ARG
                msg = L.l2hmc_last_error().decode()
                assert msg.startswith(name + ": ") and str(draw) in msg and "2^63" in msg, msg
        assert entry(L, plan, 0, 2 ** 63 - 1) == 0
        assert entry(L, plan, 4, 2 ** 63 - 1) == 3                         # L2HMC_ERR_WORKSPACE
        assert "workspace" in L.l2hmc_last_error().decode()
    with pytest.raises(ValueError, match="2\\^63"):
        _lib.check(entry(L, plans[0], 0, 2 ** 63))


def _small_plan(hmc=0):
    net = _lib.DenseNet(D=2, H=10, Ka=2, Kb=2, w1_t=PTR, wt=PTR, b1=PTR, wh_t=PTR, bh=PTR, whd_t=PTR, bhd=PTR,
                        coeff_s=PTR, coeff_q=PTR, q_tanh=1)
    tgt = _lib.MogTarget(dim=2, K=1, is_gaussian=1, temperature=1.0, mu=PTR, prec=PTR, log_const=PTR)
    return _lib.SmallPlan(x_dim=2, num_nodes=10, trajectory_length=5, hmc=hmc, eps=0.1, first_layer_form=0, masks=PTR,
                          xnet=net, vnet=net, target=tgt)


def test_small_propose_refuses_a_draw0_whose_four_streams_would_wrap(L):
    """draw0 .. draw0 + 3 must stay below 2^64.  With B > 0 the accepted value is shown on a plain-HMC plan, which the
    entry refuses AFTER the draw check with another message and before any device call."""
    propose = lambda plan, B, d: L.l2hmc_small_propose(C.byref(plan), PTR, B, 42, d, None, None, None, None, None)
    for plan in (_small_plan(), _small_plan(hmc=1)):
        for B in (0, 4):
            for d in (2 ** 64 - 3, 2 ** 64 - 1):
                assert propose(plan, B, d) == 1, (B, d)
                msg = L.l2hmc_last_error().decode()
                assert msg.startswith("small_propose: ") and "overflows 64 bits" in msg and str(d) in msg, msg
        assert propose(plan, 0, 2 ** 64 - 4) == 0
    assert propose(_small_plan(hmc=1), 4, 2 ** 64 - 4) == 1
    assert "hmc sampler" in L.l2hmc_last_error().decode()


def test_header_states_both_rules():
    from tests.run_cases import header_text
    text = header_text(comments=True)
    assert "draw must be below 2^63" in text and "draw0 must not exceed 2^64 - 4" in text


# ------------------------------------------------------------------------------------------------ accept condition
@pytest.mark.parametrize("case", [c for c in PC.LATTICE_CASES if c.both], ids=lambda c: c.name)
def test_reference_draws_keep_every_accept_decision_clear_of_its_uniform(case):
    """The GPU test feeds the float64 oracle the draws the library wrote and leaves out chains whose accept decision
    lies within 1e-4 of the uniform (none allowed where B < 64, 2 % elsewhere).  Here the oracle is fed the REFERENCE
    draws of the same (seed, draw): no chain of any committed case lies within 2e-4, twice the GPU margin, because the
    device's normals differ from the reference ones at the 1e-6 level.  (A selected-only case has the draws, the start
    and therefore the margins of its both-directions twin.)"""
    orc = PC.lattice_oracle(case)
    x64 = PC.lattice_x0(case).astype(np.float64)
    for draw in PC.STEP_DRAWS:
        vf, vb, coin, u = R.lattice_step(PC.SEED_HIGH, draw, case.B, 2 * case.T * case.X)
        want = orc.apply_transition(x64, PC.BETA, vf, vb, coin.astype(np.float64), u.astype(np.float64))
        margin = np.abs(want[2] - u)
        print(f"{case.name} draw={draw}: min |p - u| = {margin.min():.3e}, mean p = {want[2].mean():.3f}, "
              f"{int((want[2] > u).sum())} of {case.B} accepted")
        assert np.isfinite(want[2]).all()
        assert (margin > PC.MARGIN_HOST).all(), (case.name, draw, margin.min())
        assert PC.excluded_cap(case.B) in (0, 1)
