"""A run of plain-HMC steps in one launch (l2hmc_gauge_hmc_run, hmc_run_kernel in l2hmc_amd/csrc/hmc_step.hip).

The yardstick is the loop over `GaugeSampler.step` (`steps_per_launch = 1`), which tests/test_gpu_hmc_step.py and the
invariance tests hold to the float64 oracle: the run has to give ITS bits, so every comparison here is an equality."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.run_cases import assert_same_run, count_launches

pytestmark = pytest.mark.gpu

N_LF, EPS = 3, 0.1
SHAPES = [(8, 8, 70), (3, 5, 1), (6, 6, 33), (4, 16, 257), (16, 16, 5), (32, 32, 3)]
HIST = ("px", "actions", "plaqs", "charges", "charge_diff")


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _sampler(la, T, X, B, both=True, fused=True, spl=256, N=N_LF, draws=4):
    orc = H.gauge_oracle(T, X, N, EPS, None, None, hmc=True)
    dyn = H.gauge_hip(T, X, N, EPS, None, None, orc.mask, B, hmc=True, both_directions=both)
    dyn.fused = fused
    dyn._draws = draws
    smp = la.GaugeSampler(dyn)
    smp.steps_per_launch = spl
    return smp


def _x0(T, X, B):
    torch.manual_seed(1234)
    return torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)


def _plan_fused(dyn):
    from l2hmc_amd import _lib
    plan = dyn._plan()
    return _lib.lib().l2hmc_gauge_plan_fused(C.byref(plan))


def _assert_same_run(a, b, sa, sb, what):
    assert set(a) == set(b), what
    assert_same_run(a, b, HIST + ("samples",), what)
    assert a["plaq_exact"] == b["plaq_exact"], what
    assert torch.equal(sa.stats.total, sb.stats.total), (what, sa.stats.total, sb.stats.total)
    assert sa.dynamics._draws == sb.dynamics._draws, what


def _compare(la, T, X, B, both, steps, spl, fused=True, N=N_LF, beta=2.0):
    new, old = (_sampler(la, T, X, B, both, fused, s, N) for s in (spl, 1))
    x0 = _x0(T, X, B)
    keep = x0.clone()
    a = new.run(steps, beta, x0, keep_samples=True)
    b = old.run(steps, beta, x0, keep_samples=True)
    assert torch.equal(x0, keep)                                     # the caller's x is not advanced in place
    _assert_same_run(a, b, new, old, f"{T}x{X} B={B} both={both} steps={steps} per launch={spl}")
    assert a["px"].shape == (steps, B) and a["samples"].shape == (steps, B, 2 * T * X)
    assert np.array_equal(a["samples"][-1], a["samples_out"].cpu().numpy())
    assert a["samples"].min() >= 0 and a["samples"].max() <= 2 * np.pi
    return new, old


# ----------------------------------------------------------------- 1. the run against the loop, bit for bit
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", SHAPES)
def test_run_equals_the_loop(la, T, X, B, both):
    new, _ = _compare(la, T, X, B, both, steps=5, spl=256)
    assert _plan_fused(new.dynamics) == 1


@pytest.mark.parametrize("T,X,B", [(8, 8, 70), (32, 32, 3)])
def test_run_in_chunks_with_a_shorter_last_one(la, T, X, B):
    _compare(la, T, X, B, True, steps=7, spl=3)


def test_run_with_one_beta_per_step_equals_steps_at_those_betas(la):
    T, X, B = 6, 6, 33
    betas = [1.0, 1.5, 2.0, 2.5, 3.0]
    new, old = _sampler(la, T, X, B), _sampler(la, T, X, B)
    x0 = _x0(T, X, B)
    a = new.run(5, betas, x0, keep_samples=True)
    x = x0
    for i, beta in enumerate(betas):
        x, px, obs, dq = old.step(x, beta)
        got = (a["px"][i], a["actions"][i], a["plaqs"][i], a["charges"][i], a["charge_diff"][i], a["samples"][i])
        want = (px, obs["action"], obs["avg_plaq"], obs["top_charge"], dq, x)
        for g, w in zip(got, want):
            assert np.array_equal(g, w.cpu().numpy()), i
    assert torch.equal(a["samples_out"], x)
    assert a["mean_accept"] == old.stats.mean_accept() and torch.equal(new.stats.total, old.stats.total)
    assert new.dynamics._draws == old.dynamics._draws
    assert a["plaq_exact"] == la.lattice.u1_plaq_exact(3.0)
    # the loop takes the same sequence
    b = _sampler(la, T, X, B, spl=1).run(5, betas, x0, keep_samples=True)
    assert all(np.array_equal(a[k], b[k]) for k in HIST + ("samples",))


# ----------------------------------------------------------------- 2. launches
@pytest.mark.parametrize("T,X,B", [(8, 8, 64), (32, 32, 4)])
def test_run_is_one_launch_per_chunk(la, T, X, B):
    x = _x0(T, X, B)
    for spl in (8, 3, 1):
        smp = _sampler(la, T, X, B, spl=spl)
        smp.run(8, 2.0, x)                                           # warm-up
        assert count_launches(5, lambda: smp.run(8, 2.0, x)) == math.ceil(8 / spl)
        assert count_launches(4, lambda: smp.run(8, 2.0, x)) == 0


# ----------------------------------------------------------------- 3. the C entry on its own
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", [(8, 8, 70), (32, 32, 3), (3, 5, 1)])
def test_c_entry_outputs_are_optional_in_place_works_and_tickets_stay_zero(la, T, X, B, both):
    from l2hmc_amd import _lib
    L, n, D = _lib.lib(), 4, 2 * T * X
    dyn = _sampler(la, T, X, B, both).dynamics
    plan = dyn._plan()
    x0 = _x0(T, X, B)
    betas = torch.full((n,), 2.0, device="cuda")
    nb = L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(plan), B, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

    def call(x_in, x_next, full):
        hist = [torch.empty(n, B, device="cuda") for _ in range(5)] if full else [None] * 5
        sums = torch.zeros(n, 4, device="cuda") if full else None
        samples = torch.empty(n, B, D, device="cuda") if full else None
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(L.l2hmc_gauge_hmc_run(C.byref(plan), betas.data_ptr(), x_in.data_ptr(), x_next.data_ptr(), B, 77, 5,
                                         n, *(ptr(h) for h in hist), ptr(sums), ptr(samples),
                                         ws.data_ptr() if full else None, nb if full else 0, _lib.stream_ptr()))
        torch.cuda.synchronize()
        return hist, sums, samples

    full, again, bare, inplace = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0), x0.clone()
    hist, sums, samples = call(x0, full, True)
    hist2, sums2, samples2 = call(x0, again, True)
    call(x0, bare, False)
    call(inplace, inplace, False)
    assert torch.equal(full, again) and torch.equal(samples, samples2) and torch.equal(sums, sums2)
    assert all(torch.equal(a, b) for a, b in zip(hist, hist2))
    assert torch.equal(full, bare) and torch.equal(full, inplace)
    assert torch.equal(samples[-1], full)
    assert torch.all(sums.view(torch.int32)[:, 3] == 0)               # every ticket word is left at 0
    assert torch.all(sums[:, 2] == B)
    # row s of step_sums is the step's own: l2hmc_gauge_mcmc_step_ex from the same state and draw
    one = torch.zeros(4, device="cuda")
    wsb = L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B)
    ws1 = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    x = x0
    for s in range(n):
        xn = torch.empty_like(x)
        px = torch.empty(B, device="cuda")
        _lib.check(L.l2hmc_gauge_mcmc_step_ex(C.byref(plan), 2.0, x.data_ptr(), xn.data_ptr(), B, 77, 5 + s,
                                              px.data_ptr(), None, None, None, None, one.data_ptr(), ws1.data_ptr(),
                                              wsb, _lib.stream_ptr()))
        assert torch.equal(one, sums[s]) and torch.equal(px, hist[0][s]) and torch.equal(xn, samples[s]), s
        x = xn


# ----------------------------------------------------------------- 4. plans without the kernel, and L2HMC dynamics
@pytest.mark.parametrize("T,X,B,N,layered", [(6, 6, 9, 3, True), (2, 513, 2, 2, False)])
def test_unfused_hmc_plans_run_the_loop(la, T, X, B, N, layered):
    from l2hmc_amd import _lib
    L, n, D = _lib.lib(), 3, 2 * T * X
    new, old = _compare(la, T, X, B, True, steps=n, spl=256, fused=not layered, N=N)
    assert _plan_fused(new.dynamics) == 0
    # the C entry is total: the same run as a host loop over the step
    dyn = old.dynamics
    plan = dyn._plan()
    x0 = _x0(T, X, B)
    dyn._draws = 4
    want = old.run(n, 2.0, x0, keep_samples=True)
    betas = torch.full((n,), 2.0, device="cuda")
    nb = L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(plan), B, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    hist = [torch.empty(n, B, device="cuda") for _ in range(5)]
    sums, samples, xn = torch.zeros(n, 4, device="cuda"), torch.empty(n, B, D, device="cuda"), torch.empty_like(x0)
    _lib.check(L.l2hmc_gauge_hmc_run(C.byref(plan), betas.data_ptr(), x0.data_ptr(), xn.data_ptr(), B, dyn._seed,
                                     _lib.step_draw_index(4)[0], n, *(h.data_ptr() for h in hist), sums.data_ptr(),
                                     samples.data_ptr(), ws.data_ptr(), nb, _lib.stream_ptr()))
    for k, h in zip(HIST, hist):
        assert np.array_equal(h.cpu().numpy(), want[k]), k
    assert np.array_equal(samples.cpu().numpy(), want["samples"]) and torch.equal(xn, want["samples_out"])


def test_l2hmc_dynamics_keep_the_loop(la):
    T = X = 4
    B, N = 6, 3
    xp, vp = H.gauge_weights(T, X, regime="mild")
    orc = H.gauge_oracle(T, X, N, EPS, xp, vp)
    outs = []
    for spl in (None, 1):
        dyn = H.gauge_hip(T, X, N, EPS, xp, vp, orc.mask, B)
        dyn._draws = 4
        smp = la.GaugeSampler(dyn)
        assert smp.steps_per_launch == 256
        if spl is not None:
            smp.steps_per_launch = spl
        outs.append((smp.run(4, 2.0, _x0(T, X, B), keep_samples=True), smp))
    (a, sa), (b, sb) = outs
    _assert_same_run(a, b, sa, sb, "GenericNet 4x4")
