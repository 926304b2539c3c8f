"""The ladder form of the plain-HMC lattice run: beta per step and chain, a step size per chain, in one launch
(l2hmc_gauge_hmc_run_ladder, hmc_run_kernel<SPT, true> in l2hmc_amd/csrc/hmc_step.hip, `GaugeSampler.run_hmc`).

The yardstick is the uniform run (l2hmc_gauge_hmc_run / `GaugeSampler.run`), which tests/test_gpu_hmc_run.py and
tests/test_gpu_hmc_step.py hold to the loop over the step and to the float64 oracle.  Chains never interact and the
ladder kernel runs the step's own fp32 operations on per-chain values, so a column of a ladder has to be the column of
the uniform run of the whole batch at that column's beta and eps: every comparison here is an equality.  (The one
bound, on the step sums of a true ladder, is the rounding of an fp32 sum of B terms against float64.)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.run_cases import assert_same_run, count_launches

pytestmark = pytest.mark.gpu

N_LF, EPS, STEPS = 3, 0.1, 5
# one shape per way the kernel lays rows onto waves: 16 threads per row (rows of different beta inside one wave, dead
# rows); one wave per row, B no multiple of the chains per workgroup; 36 sites on 64 threads; a row over 4 waves;
# SPT = 2; SPT = 4 (the pair in LDS), one chain per workgroup when paired
SHAPES = [(3, 5, 7), (8, 8, 70), (6, 6, 33), (16, 16, 5), (16, 20, 3), (32, 32, 3)]
HIST = ("px", "actions", "plaqs", "charges", "charge_diff")
BETAS = (1.0, 2.5, 4.0)
EPSS = (0.05, 0.1, 0.2)


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _sampler(la, T, X, B, both=True, spl=256, eps=EPS, draws=4):
    orc = H.gauge_oracle(T, X, N_LF, eps, None, None, hmc=True)
    dyn = H.gauge_hip(T, X, N_LF, eps, None, None, orc.mask, B, hmc=True, both_directions=both)
    dyn._draws = draws
    smp = la.GaugeSampler(dyn)
    smp.steps_per_launch = spl
    return smp


def _x0(T, X, B, sigma=None):
    """the shared start: uniform in [0, 2 pi), or (sigma) links N(0, sigma^2) around the ordered state, wrapped"""
    torch.manual_seed(1234)
    if sigma is not None:
        return torch.remainder(torch.randn(B, 2 * T * X, device="cuda") * sigma, 2 * np.pi)
    return torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)


_UNIFORM = {}


def _uniform(la, T, X, B, both, beta, eps=EPS, steps=STEPS, sigma=None):
    """`run` of the whole batch at one beta (a float, or a tuple: one per step) and one eps, from the shared start, seed
    and draw counter: computed once, shared by the tests, never written to."""
    key = (T, X, B, both, beta, eps, steps, sigma)
    if key not in _UNIFORM:
        smp = _sampler(la, T, X, B, both, eps=eps)
        out = smp.run(steps, list(beta) if isinstance(beta, tuple) else beta, _x0(T, X, B, sigma), keep_samples=True)
        _UNIFORM[key] = (out, smp)
    return _UNIFORM[key]


def _assert_columns(a, u, cols, what):
    """columns `cols` of every history, of the samples and of the final state of ladder run `a` are those of run `u`"""
    assert len(cols) > 0
    for k in HIST:
        assert a[k].shape == u[k].shape and a[k].dtype == u[k].dtype, (what, k)
        assert np.array_equal(a[k][:, cols], u[k][:, cols]), (what, k)
    assert np.array_equal(a["samples"][:, cols], u["samples"][:, cols]), (what, "samples")
    assert torch.equal(a["samples_out"][cols], u["samples_out"][cols]), (what, "samples_out")


def _assert_same_run(a, b, sa, sb, what):
    assert_same_run(a, b, HIST + ("samples",), what)
    assert torch.equal(sa.stats.total, sb.stats.total), (what, sa.stats.total, sb.stats.total)
    assert sa.dynamics._draws == sb.dynamics._draws, what


# ----------------------------------------------------------------- 1. the columns of a ladder are uniform runs
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", SHAPES)
def test_ladder_columns_are_uniform_runs(la, T, X, B, both):
    x0 = _x0(T, X, B)
    keep = x0.clone()
    c = np.arange(B)
    # a ladder of beta
    smp = _sampler(la, T, X, B, both)
    a = smp.run_hmc(STEPS, np.array(BETAS)[c % 3][None, :], x0, keep_samples=True)
    assert torch.equal(x0, keep)                                     # the caller's x is not advanced in place
    assert a["px"].shape == (STEPS, B) and a["samples"].shape == (STEPS, B, 2 * T * X)
    assert np.array_equal(a["samples"][-1], a["samples_out"].cpu().numpy())
    assert np.array_equal(a["plaq_exact"], la.lattice.u1_plaq_exact(np.array(BETAS)[c % 3]))
    for g, beta in enumerate(BETAS):
        u, us = _uniform(la, T, X, B, both, beta)
        _assert_columns(a, u, c[g::3], f"{T}x{X} B={B} both={both} beta={beta}")
        assert smp.dynamics._draws == us.dynamics._draws
    # a ladder of step sizes; the dynamics' own eps and plan are left alone
    smp = _sampler(la, T, X, B, both)
    a = smp.run_hmc(STEPS, 2.0, x0, eps=np.array(EPSS)[c % 3], keep_samples=True)
    assert float(smp.dynamics.eps) == np.float32(EPS) and smp.dynamics._plan().eps == np.float32(EPS)
    assert a["plaq_exact"] == la.lattice.u1_plaq_exact(2.0)
    for g, eps in enumerate(EPSS):
        u, _ = _uniform(la, T, X, B, both, 2.0, eps)
        _assert_columns(a, u, c[g::3], f"{T}x{X} B={B} both={both} eps={eps}")
    # a 2 x 2 grid of both: chain c at (beta[c % 2], eps[(c // 2) % 2])
    gb, ge = np.array([1.0, 4.0]), np.array([0.05, 0.2])
    smp = _sampler(la, T, X, B, both)
    a = smp.run_hmc(STEPS, gb[c % 2][None, :], x0, eps=ge[(c // 2) % 2], keep_samples=True)
    seen = 0
    for i in range(2):
        for j in range(2):
            cols = c[(c % 2 == i) & ((c // 2) % 2 == j)]
            if len(cols):
                u, _ = _uniform(la, T, X, B, both, float(gb[i]), float(ge[j]))
                _assert_columns(a, u, cols, f"{T}x{X} B={B} both={both} grid {i}{j}")
                seen += len(cols)
    assert seen == B


# ----------------------------------------------------------------- 2. beta per step equals `run`
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", SHAPES)
def test_step_indexed_beta_equals_run(la, T, X, B, both):
    s1, s2 = (1.0, 1.5, 2.0, 2.5, 3.0), (4.0, 3.0, 2.0, 1.0, 0.5)
    x0 = _x0(T, X, B)
    u1, us1 = _uniform(la, T, X, B, both, s1)
    u2, _ = _uniform(la, T, X, B, both, s2)
    smp = _sampler(la, T, X, B, both)
    a = smp.run_hmc(STEPS, list(s1), x0, keep_samples=True)
    _assert_same_run(a, u1, smp, us1, "schedule")
    assert a["plaq_exact"] == u1["plaq_exact"]
    # [n, B]: even chains on the first schedule, odd chains on the second
    c = np.arange(B)
    grid = np.where((c % 2 == 0)[None, :], np.array(s1)[:, None], np.array(s2)[:, None])
    a = _sampler(la, T, X, B, both).run_hmc(STEPS, grid, x0, keep_samples=True)
    _assert_columns(a, u1, c[0::2], "grid, first schedule")
    _assert_columns(a, u2, c[1::2], "grid, second schedule")
    assert np.array_equal(a["plaq_exact"], la.lattice.u1_plaq_exact(grid[-1]))


# ----------------------------------------------------------------- 3. all-equal entries equal the uniform entry
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", SHAPES)
def test_all_equal_entries_equal_the_uniform_entry(la, T, X, B, both):
    x0 = _x0(T, X, B)
    u, us = _uniform(la, T, X, B, both, 2.0)
    want_sums = us._run_sums[:STEPS].clone()
    forms = [(2.0, None), (np.full(STEPS, 2.0), EPS), (np.full((1, B), 2.0), np.full(B, EPS)),
             (np.full((STEPS, B), 2.0), None), (torch.full((STEPS, B), 2.0), torch.full((B,), EPS))]
    for beta, eps in forms:
        smp = _sampler(la, T, X, B, both)
        a = smp.run_hmc(STEPS, beta, x0, eps=eps, keep_samples=True)
        what = f"{T}x{X} B={B} both={both} beta {np.shape(beta)} eps {np.shape(eps) if eps is not None else None}"
        _assert_same_run(a, u, smp, us, what)
        assert np.all(a["plaq_exact"] == u["plaq_exact"]), what
        assert np.shape(a["plaq_exact"]) == ((B,) if np.ndim(beta) == 2 else ()), what
        assert torch.equal(smp._run_sums[:STEPS], want_sums), what       # the step_sums rows, tickets at 0 included


# ----------------------------------------------------------------- 4. chunks
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", SHAPES)
def test_chunks_with_a_shorter_last_one_equal_one_chunk(la, T, X, B, both):
    n, c = 7, np.arange(B)
    x0 = _x0(T, X, B)
    grid = np.linspace(1.0, 3.0, n)[:, None] + 0.5 * (c % 3)[None, :]          # every step and every rung its own beta
    eps = np.array(EPSS)[(c // 3) % 3]
    outs = []
    for spl in (256, 3):
        smp = _sampler(la, T, X, B, both, spl=spl)
        outs.append((smp.run_hmc(n, grid, x0, eps=eps, keep_samples=True), smp))
    (a, sa), (b, sb) = outs
    _assert_same_run(a, b, sa, sb, f"{T}x{X} both={both} chunks")
    assert torch.equal(sa._run_sums[:n], sb._run_sums[:n])
    # ... and a [1, B] ladder, whose chunks all start at the same row
    a, b = (_sampler(la, T, X, B, both, spl=spl).run_hmc(n, grid[:1], x0, keep_samples=True) for spl in (256, 3))
    assert all(np.array_equal(a[k], b[k]) for k in HIST + ("samples",))


# ----------------------------------------------------------------- 5. launches
@pytest.mark.parametrize("T,X,B", [(8, 8, 64), (32, 32, 4)])
def test_run_hmc_is_one_launch_per_chunk(la, T, X, B):
    x = _x0(T, X, B)
    beta = np.array(BETAS)[np.arange(B) % 3][None, :]
    eps = np.array(EPSS)[np.arange(B) % 3]
    for spl in (8, 3, 1):
        smp = _sampler(la, T, X, B, spl=spl)
        smp.run_hmc(8, beta, x, eps=eps)                             # warm-up
        assert count_launches(5, lambda: smp.run_hmc(8, beta, x, eps=eps)) == math.ceil(8 / spl)
        assert count_launches(4, lambda: smp.run_hmc(8, beta, x, eps=eps)) == 0


# ----------------------------------------------------------------- 6. the C entry on its own
def _c_run(plan, B, D, n, x_in, x_next, betas, ss=1, cs=0, eps=None, full=True, ladder=True, ws=None):
    """One call of l2hmc_gauge_hmc_run_ladder (or of the uniform entry); returns (histories, step_sums, samples)."""
    from l2hmc_amd import _lib
    L = _lib.lib()
    hist = [torch.empty(n, B, device="cuda") for _ in range(5)] if full else [None] * 5
    sums = torch.zeros(n, 4, device="cuda") if full else None
    samples = torch.empty(n, B, D, device="cuda") if full else None
    ptr = lambda t: None if t is None else t.data_ptr()
    tail = (B, 77, 5, n, *(ptr(h) for h in hist), ptr(sums), ptr(samples), ws.data_ptr() if full else None,
            ws.numel() if full else 0, _lib.stream_ptr())
    if ladder:
        _lib.check(L.l2hmc_gauge_hmc_run_ladder(C.byref(plan), betas.data_ptr(), ss, cs, ptr(eps), x_in.data_ptr(),
                                                x_next.data_ptr(), *tail))
    else:
        _lib.check(L.l2hmc_gauge_hmc_run(C.byref(plan), betas.data_ptr(), x_in.data_ptr(), x_next.data_ptr(), *tail))
    torch.cuda.synchronize()
    return hist, sums, samples


def _same(a, b, cols=None):
    """(histories, sums, samples) of two calls are equal, on the columns `cols` (then without the sums) or on all"""
    (ha, sa, xa), (hb, sb, xb) = a, b
    if cols is None:
        return all(torch.equal(p, q) for p, q in zip(ha, hb)) and torch.equal(sa, sb) and torch.equal(xa, xb)
    return all(torch.equal(p[:, cols], q[:, cols]) for p, q in zip(ha, hb)) and torch.equal(xa[:, cols], xb[:, cols])


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", [(8, 8, 70), (32, 32, 3), (3, 5, 7)])
def test_c_entry(la, T, X, B, both):
    from l2hmc_amd import _lib
    L, n, D = _lib.lib(), 4, 2 * T * X
    dyn = _sampler(la, T, X, B, both).dynamics                       # (kept: it owns the masks the plan points to)
    plan = dyn._plan()
    x0 = _x0(T, X, B)
    nb = L.l2hmc_gauge_hmc_run_ladder_ws_bytes(C.byref(plan), B, n)
    assert nb == L.l2hmc_gauge_hmc_run_ws_bytes(C.byref(plan), B, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dev = lambda v: torch.tensor(np.asarray(v, dtype=np.float32).reshape(-1), device="cuda")
    c = torch.arange(B, device="cuda")
    rung = np.arange(B) % 3
    sched = np.array([1.0, 2.0, 3.0, 4.0])
    lad_b, lad_e = dev(np.array(BETAS)[rung]), dev(np.array(EPSS)[rung])
    run = lambda x_in, x_next, betas, **kw: _c_run(plan, B, D, n, x_in, x_next, betas, ws=ws, **kw)

    # a true ladder of both: outputs are optional, in place works, twice the same, tickets stay 0, sums are the rows'
    full, again, bare, inplace = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0), x0.clone()
    out = run(x0, full, lad_b, ss=0, cs=1, eps=lad_e)
    out2 = run(x0, again, lad_b, ss=0, cs=1, eps=lad_e)
    run(x0, bare, lad_b, ss=0, cs=1, eps=lad_e, full=False)
    run(inplace, inplace, lad_b, ss=0, cs=1, eps=lad_e, full=False)
    hist, sums, samples = out
    assert _same(out, out2) and torch.equal(full, again)
    assert torch.equal(full, bare) and torch.equal(full, inplace) and torch.equal(samples[-1], full)
    assert torch.all(sums.view(torch.int32)[:, 3] == 0)               # every ticket word is left at 0
    assert torch.all(sums[:, 2] == B)
    for col, h in ((0, hist[0]), (1, hist[4])):                       # sum p_accept, sum |dQ|
        for s in range(n):
            want = float(h[s].double().sum())
            got = float(sums[s, col])
            print(f"step_sums[{s}][{col}] = {got!r}, float64 sum of the row = {want!r}")
            assert abs(got - want) <= B * 2.0 ** -23 * max(1.0, want), (s, col, got, want)
    assert float(samples.min()) >= 0 and float(samples.max()) <= 2 * np.pi

    def uniform(betas, eps=None):
        """the uniform entry on the same batch: betas [n], plan.eps = eps"""
        p = dyn._plan()
        if eps is not None:
            p.eps = float(np.float32(eps))
        xn = torch.empty_like(x0)
        return _c_run(p, B, D, n, x0, xn, dev(betas), ladder=False, ws=ws), xn

    # columns of the ladder against the uniform entry at the rung's (beta, eps)
    for g in range(3):
        ref, xn = uniform(np.full(n, BETAS[g]), EPSS[g])
        assert _same(out, ref, c[g::3]) and torch.equal(full[g::3], xn[g::3]), g
    # the four stride pairs with NULL eps_chain
    xn = torch.empty_like(x0)
    ref, xr = uniform(sched)
    assert _same(run(x0, xn, dev(sched), ss=1, cs=0), ref) and torch.equal(xn, xr)                  # a schedule
    ref, xr = uniform(np.full(n, 2.5))
    assert _same(run(x0, xn, dev([2.5]), ss=0, cs=0), ref) and torch.equal(xn, xr)                  # one value
    lad = run(x0, xn, lad_b, ss=0, cs=1)                                                            # a ladder
    xl = xn.clone()
    grid = sched[:, None] * np.array([1.0, 0.5, 0.25])[rung][None, :]
    both_ = run(x0, xn, dev(grid), ss=B, cs=1)                                                      # both
    for g, f in enumerate((1.0, 0.5, 0.25)):
        ref, xr = uniform(np.full(n, BETAS[g]))
        assert _same(lad, ref, c[g::3]) and torch.equal(xl[g::3], xr[g::3]), g
        ref, xr = uniform(sched * f)
        assert _same(both_, ref, c[g::3]) and torch.equal(xn[g::3], xr[g::3]), g
    # a ladder of step sizes under one beta, and equal step sizes against the plan's own
    eps_only = run(x0, xn, dev([2.0]), ss=0, cs=0, eps=lad_e)
    for g in range(3):
        ref, xr = uniform(np.full(n, 2.0), EPSS[g])
        assert _same(eps_only, ref, c[g::3]) and torch.equal(xn[g::3], xr[g::3]), g
    ref, xr = uniform(np.full(n, 2.0))
    assert _same(run(x0, xn, dev([2.0]), ss=0, cs=0, eps=dev(np.full(B, EPS))), ref) and torch.equal(xn, xr)


# ----------------------------------------------------------------- 7. sensible values
# An accept probability is min(1, exp(-dH)).  From the uniform-random start of the other tests the energy error of a
# trajectory has one sign and every chain of the small batches has p = 1 at every beta, which says nothing about beta.
# This test starts near the ordered state instead (links N(0, 0.3^2): <cos P> = exp(-2 * 0.09) = 0.84, between the
# equilibria of beta 2.5 and 4), where dH takes both signs, p < 1 for about half of the entries and p depends on beta.
SIGMA = 0.3


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", SHAPES)
def test_values_are_sensible_and_the_rungs_differ(la, T, X, B, both):
    c = np.arange(B)
    a = _sampler(la, T, X, B, both).run_hmc(STEPS, np.array(BETAS)[c % 3][None, :], _x0(T, X, B, SIGMA),
                                            keep_samples=True)
    assert a["samples"].min() >= 0 and a["samples"].max() <= 2 * np.pi
    assert np.isfinite(a["px"]).all() and a["px"].min() >= 0 and a["px"].max() <= 1
    # the same chains at beta = 4 and at beta = 1 (a ladder that read one value would give them one probability):
    # the uniform runs of the whole batch give every chain both, and the ladder has each rung's own
    lo, hi = (_uniform(la, T, X, B, both, beta, sigma=SIGMA)[0]["px"] for beta in (1.0, 4.0))
    print(f"{T}x{X} B={B} both={both}: px of the chains of rung 2 at beta 4 {a['px'][:, 2::3].ravel()[:6]}, "
          f"at beta 1 {lo[:, 2::3].ravel()[:6]}")
    assert not np.array_equal(lo, hi)
    assert np.array_equal(a["px"][:, 0::3], lo[:, 0::3]) and np.array_equal(a["px"][:, 2::3], hi[:, 2::3])
    assert not np.array_equal(a["px"][:, 2::3], lo[:, 2::3])
    assert not np.array_equal(a["px"][:, 0::3], hi[:, 0::3])
    # the beta = 4 rung against the beta = 1 rung of the ladder itself: other chains, so compare what a column shows
    assert not np.array_equal(np.sort(a["px"][:, 0]), np.sort(a["px"][:, 2]))
