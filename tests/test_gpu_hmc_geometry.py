"""The one-launch plain-HMC kernels (l2hmc_amd/csrc/hmc_step.hip) in every thread-geometry class.

Every entry of the family (the MCMC step, the trajectory and single leapfrog steps, the runs, the ladder runs, the runs
with the exchange rounds inside) shares one copy of the step and one host rule, `hmc_geom`, that maps a row onto threads:
`spt` sites per thread, `2^tsh` threads per row, `R` rows per workgroup, `ragged` where lanes own no site.  The cases of
tests/hmc_geometry_cases.py take one lattice per reachable class and a few per edge (extents of 1 and 2, T > X, slices of
a thread with no live lane), each at a batch that fills a workgroup and leaves the last one partial, with both
directions and with the selected one only, at inputs on which the float64 oracle accepts some chains and rejects others
with no chain within 1e-3 of its uniform (tests/test_hmc_geometry_host.py): NO chain is left out of any comparison.

1, 2: the step and the trajectory against the float64 NumPy oracle on the device's own draws, at the project's
tolerances (tests/test_gpu_parity.py) with the float32 oracle's own error as the allowance where it exceeds them.
3 - 5: the equalities that tie the run, the ladder run and the exchange run to the step, bit for bit, through the
helpers of the files that own them, on the full and the ragged class of every (spt, tsh).  6: the layered path.

What the file found.  With the row sums of the action and the kinetic energy taken as two fp32 totals of O(sites) that
were subtracted afterwards, px of the step at 24x24 missed its bar (2.49e-5 against 2.0e-5, the float32 oracle 2.8e-6),
and p of the forward trajectory at 20x20 missed its own (6.55e-5 against 4.30e-5): an fp32 total of 1000 carries 6e-5
of rounding, and p = exp(dH) takes all of it once p lies inside (0, 1), which the older cases (p clipped to 1) never
showed.  hmc_trajectory now sums the differences of the threads' own shares; every figure below is with that.

Measured on the MI355X, the worst case of each class as figure / bar (classes: spt, tsh, f full or r ragged):
  the step: px 1.5e-5 / 9.0e-5 at (1, 8, f), 1.2e-5 / 2.0e-5 at (2, 8, r), 1.1e-5 / 4.2e-5 at (1, 7, r), 9.2e-6 / 4.1e-5
  at (1, 8, r), 6.4e-6 / 2.0e-5 or less in every other class (3.3e-6 at (4, 8, r), 0 at 1x1); action 3.4e-7 and plaquette
  4.8e-7 / 1e-5 (both at two and three sites, 1.1e-7 or less from 32 sites on); charge 8.7e-7 / 1e-4; |dQ| 1.5e-6 / 1e-3;
  x_next 2.7e-6 / 5e-5 (the float32 oracle's own error never lifts that bar).  Every accept decision is the float64
  reference's, 1x1 accepts all 129 and 130 chains, and the reference accepts / rejects 63 / 2 and 127 / 2 at 1x2,
  31 / 2 and 59 / 6 at 2x2, 31 / 2 and 63 / 2 at 1x3, 14 / 3 and 29 / 4 at 2x4 and 2x3, 15 / 2 and 31 / 2 at 1x7, 7 / 2 and
  14 / 3 at 5x3 and 4x4, and of 9 chains 5 / 4 at 7x9, 3x11 and 17x17, 6 / 3 at 8x16 and 32x32, 4 / 5 at 16x32 and 20x20,
  7 / 2 at the other sixteen lattices.
  trajectory, single steps and the round trip: x 3.8e-7 / 1e-5 (rms 3.7e-8 / 3.3e-6), v 2.2e-6 / 1e-5 (rms 2.1e-7 / 3.3e-6);
  p 1.9e-5 / 7.8e-5 at (1, 7, f), 1.5e-5 / 6.5e-5 at (1, 6, r), 1.3e-5 / 3.7e-5 at (1, 8, r), 1.2e-5 / 6.5e-5 at (2, 8, r),
  8.6e-6 / 2.7e-5 or less elsewhere.
The equalities (3 - 5) hold bit for bit in every class; the exchange run's workgroups reach 768 threads at 2x2 and 10x10
(groups of 3) and 1024 at 17x17 (groups of 2)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import tests.test_gpu_hmc_run as run_tests
import tests.test_gpu_hmc_run_exchange as exchange_tests
import tests.test_gpu_hmc_run_ladder as ladder_tests
from oracle import lattice as olat
from tests import helpers as H
from tests import hmc_geometry_cases as G
from tests.run_cases import count_launches
from tests.test_gpu_hmc_step import (MAX_RATIO, TOL_OP, _compare_paths, _plan_fused, assert_fp32_equivalent, circle,
                                     np_)
from tests.toy_cases import p_bar

pytestmark = pytest.mark.gpu

X_NEXT_TOL = 5e-5
EQ = G.equality_cases()


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _dyn(c, B, both):
    orc = G.oracle(c)
    dyn = H.gauge_hip(c.T, c.X, G.N_LF, c.eps, None, None, orc.mask, B, hmc=True, both_directions=both)
    assert _plan_fused(dyn) == 1
    return orc, G.oracle(c, np.float32), dyn


def _what(c, B, both):
    return f"{c.T}x{c.X} class {G.class_of(c)} B={B} both={both}"


# ----------------------------------------------------------------- 1. the step on its own draws
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_step_matches_oracle_on_its_own_draws(la, c, both):
    """l2hmc_gauge_mcmc_step against the float64 oracle fed the device's own l2hmc_fill_* draws: the accept decision of
    EVERY chain, px, the observables, |dQ| and x_next of every chain; a rejected chain returns its input's bits."""
    from l2hmc_amd import _lib
    B, D = G.batch(c, both), 2 * c.T * c.X
    orc, orc32, dyn = _dyn(c, B, both)
    x0 = G.start(c, B)
    x = torch.as_tensor(x0, device="cuda").clone()
    outs = [torch.empty(B, device="cuda") for _ in range(5)]
    plan, Lh = dyn._plan(), _lib.lib()
    ws, nb = dyn._ws.get(Lh.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B), x.device)
    _lib.check(Lh.l2hmc_gauge_mcmc_step(C.byref(plan), c.beta, x.data_ptr(), B, G.SEED, c.draw,
                                         *[o.data_ptr() for o in outs], ws, nb, _lib.stream_ptr()))
    V = torch.empty(2 * B, D, device="cuda")
    cu = torch.empty(2 * B, device="cuda")
    _lib.check(Lh.l2hmc_fill_normal(V.data_ptr(), V.numel(), G.SEED, 2 * c.draw, None))
    _lib.check(Lh.l2hmc_fill_uniform(cu.data_ptr(), cu.numel(), G.SEED, 2 * c.draw + 1, None))
    V32, cu32 = V.cpu().numpy(), cu.cpu().numpy()
    V, cu = V32.astype(np.float64), cu32.astype(np.float64)
    x64 = x0.astype(np.float64)
    want = orc.apply_transition(x64, c.beta, V[:B], V[B:], cu[:B], cu[B:])
    w32 = orc32.apply_transition(x0, c.beta, V32[:B], V32[B:], cu32[:B], cu32[B:])
    px, actions, plaqs, charges, dq = [np_(o) for o in outs]
    got = np_(x)
    u = cu[B:]
    f = G.figures(want[2], u)
    assert G.conditions_hold(c, f), f                                # the conditions, on the device's draws
    acc = want[2] > u
    xw = np.mod(want[3], 2 * np.pi)
    bar_p = p_bar(want[2], w32[2])
    bar_x = max(X_NEXT_TOL, MAX_RATIO * float(circle(w32[0], want[0])[acc].max())) if acc.any() else X_NEXT_TOL
    figs = dict(px=np.abs(px - want[2]).max(), action=H.relerr(actions, olat.total_action(x64, c.T, c.X)),
                plaq=H.relerr(plaqs, olat.avg_plaq(x64, c.T, c.X)), charge=H.relerr(charges, olat.top_charge(x64, c.T, c.X)),
                dq=H.relerr(dq, olat.top_charge_diff(x64, want[3], c.T, c.X)), x_next=circle(got, xw).max())
    print(f"hmc geometry step {_what(c, B, both)} eps={c.eps}: accepted {f['accepted']} rejected {f['rejected']} "
          f"interior {f['interior']} margin {f['margin']:.2e} | px {figs['px']:.3e} (bar {bar_p:.3e}) "
          f"action {figs['action']:.3e} plaq {figs['plaq']:.3e} (bar {TOL_OP:.0e}) charge {figs['charge']:.3e} (bar 1e-4) "
          f"dq {figs['dq']:.3e} (bar 1e-3) x_next {figs['x_next']:.3e} (bar {bar_x:.3e})")
    assert np.array_equal(px > u, acc), (px, want[2], u)             # every decision is the reference's
    assert figs["px"] < bar_p
    assert figs["action"] < TOL_OP and figs["plaq"] < TOL_OP and figs["charge"] < 1e-4
    assert figs["dq"] < 1e-3
    assert figs["x_next"] < bar_x
    assert got.min() >= 0 and got.max() <= 2 * np.pi
    # the reject branch: the input's own bits (every start value is its own wrap), and no charge moved
    rej = ~acc
    assert np.array_equal(x.cpu().numpy()[rej], x0[rej])
    assert np.all(dq[rej] == 0)
    if acc.any():
        assert not np.array_equal(x.cpu().numpy()[acc], x0[acc])


# ----------------------------------------------------------------- 2. trajectory and single leapfrog steps
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_trajectory_and_single_steps_match_oracle(la, c, both):
    """transition_kernel forward / backward, `_lf` single steps at the first and the last step, and backward after
    forward, from the case's start at the case's eps (the trajectory launch lays rows [0, B) onto workgroups of R)."""
    B, D, N = G.batch(c, both), 2 * c.T * c.X, G.N_LF
    orc, orc32, dyn = _dyn(c, B, both)
    x = G.start(c, B)
    rng = np.random.default_rng(5)
    v0f, v0b = (rng.standard_normal((B, D)).astype(np.float32) for _ in range(2))
    x64 = x.astype(np.float64)
    what = _what(c, B, both)
    for forward, v0 in ((True, v0f), (False, v0b)):
        xo, vo, p, sld = dyn.transition_kernel(x, c.beta, forward=forward, momentum=v0, return_logdet=True)
        w64 = orc.transition_kernel(x64, c.beta, v0.astype(np.float64), forward=forward)
        w32 = orc32.transition_kernel(x, c.beta, v0, forward=forward)
        assert_fp32_equivalent(np_(xo), w64[0], w32[0], f"hmc geometry trajectory {what} forward={forward} x")
        assert_fp32_equivalent(np_(vo), w64[1], w32[1], f"hmc geometry trajectory {what} forward={forward} v")
        ep, bar = np.abs(np_(p) - w64[2]).max(), p_bar(w64[2], w32[2])
        print(f"hmc geometry trajectory {what} forward={forward}: p {ep:.3e} (bar {bar:.3e}), p in "
              f"[{w64[2].min():.3f}, {w64[2].max():.3f}]")
        assert ep < bar
        assert torch.all(sld == 0)
    for step in sorted({0, N - 1}):
        for fn, ofn, ofn32 in ((dyn._forward_lf, orc._forward_lf, orc32._forward_lf),
                               (dyn._backward_lf, orc._backward_lf, orc32._backward_lf)):
            x1, v1, ld = fn(x, v0f, c.beta, step)
            ox, ov, _ = ofn(x64, v0f.astype(np.float64), c.beta, step)
            sx, sv, _ = ofn32(x, v0f, c.beta, step)
            assert_fp32_equivalent(np_(x1), ox, sx, f"hmc geometry {fn.__name__} {what} step {step} x")
            assert_fp32_equivalent(np_(v1), ov, sv, f"hmc geometry {fn.__name__} {what} step {step} v")
            assert torch.all(ld == 0)
    # backward after forward with the returned momentum gives x back: against the oracles' own round trip
    xf, vf, _ = dyn.transition_kernel(x, c.beta, forward=True, momentum=v0f)
    xb, vb, _ = dyn.transition_kernel(xf, c.beta, forward=False, momentum=vf)
    rt = []
    for o, xx, vv in ((orc, x64, v0f.astype(np.float64)), (orc32, x, v0f)):
        a = o.transition_kernel(xx, c.beta, vv, forward=True)
        rt.append(o.transition_kernel(a[0], c.beta, a[1], forward=False))
    assert np.abs(rt[0][0] - x64).max() < 1e-12 and np.abs(rt[0][1] - v0f).max() < 1e-12
    assert_fp32_equivalent(np_(xb), rt[0][0], rt[1][0], f"hmc geometry round trip {what} x")
    assert_fp32_equivalent(np_(vb), rt[0][1], rt[1][1], f"hmc geometry round trip {what} v")


# ----------------------------------------------------------------- 3. the run is the loop of steps
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("c", EQ, ids=G.case_id)
def test_run_equals_the_loop_of_steps(la, c, both):
    B = G.batch(c, both)
    new, _ = run_tests._compare(la, c.T, c.X, B, both, steps=5, spl=256)
    assert _plan_fused(new.dynamics) == 1
    run_tests._compare(la, c.T, c.X, B, both, steps=7, spl=3)        # chunks of 3 with a shorter last one


# ----------------------------------------------------------------- 4. the columns of a ladder are uniform runs
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("c", EQ, ids=G.case_id)
def test_ladder_columns_are_uniform_runs(la, c, both):
    """beta per chain, eps per chain and a grid of both (the four-sites-per-thread instance keeps the pair in LDS)."""
    ladder_tests.test_ladder_columns_are_uniform_runs(la, c.T, c.X, G.batch(c, both), both)


# ----------------------------------------------------------------- 5. the exchange rounds inside the launch
# the workgroups of the exchange run that are no power of two, and the full 1024: (T, X, both) -> (group, threads)
NAMED = {(10, 10, True): (3, 768), (2, 2, True): (3, 768), (17, 17, True): (2, 1024)}
assert all(any((c.T, c.X) == k[:2] for c in EQ) for k in NAMED)


def _exchange_batch(c, both, grp):
    """whole replica groups: a full workgroup of the exchange run (lcm(group, cpw0) chains) and one group more; where
    that exceeds 130 chains, the groups that 130 hold (the only workgroup is then partial)"""
    cpw = math.lcm(grp, G.chains_per_workgroup(c.T, c.X, both))
    return cpw + grp if cpw + grp <= G.TINY_BATCH else (G.TINY_BATCH // grp) * grp


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("c", EQ, ids=G.case_id)
def test_exchange_in_launch_is_the_round_between_launches(la, c, both):
    """tests/test_gpu_hmc_run_exchange.py::test_in_launch_is_between_launches with its helpers: a round after every
    step in one launch, and a round every 5 steps in chunks of 5 from the other parity, on a ladder with a schedule."""
    E = exchange_tests
    grp = G.exchange_group(c.T, c.X, both)
    if grp is None:
        # not served (four sites per thread: no instance): the refusal on the host, and nothing is launched
        B = 4
        smp = E._sampler(la, c.T, c.X, B, both, in_launch=True)
        assert not any(smp.exchange_in_launch(g) for g in (2, 3, 4))
        x0, beta = E._x0(c.T, c.X, B), E._betas(B, 2)

        def refused():
            with pytest.raises(NotImplementedError):
                smp.run_hmc_exchange(E.STEPS, beta, x0, replicas=2)
        assert count_launches(5, refused) == 0 and count_launches(8, refused) == 0
        assert smp.dynamics._draws == 4 and smp.replica is None
        return
    B = _exchange_batch(c, both, grp)
    cpw = math.lcm(grp, G.chains_per_workgroup(c.T, c.X, both))
    threads = (cpw * (2 if both else 1)) << G.geom(c.T, c.X)[1]
    assert threads <= 1024 and NAMED.get((c.T, c.X, both), (grp, threads)) == (grp, threads)
    x0 = E._x0(c.T, c.X, B)
    eps = np.array(E.EPSS)[np.arange(B) % 3]
    assert E._sampler(la, c.T, c.X, B, both).exchange_in_launch(grp) is True
    exchanged = 0
    for k, fp, spl in ((1, 0, 256), (5, 1, 5)):
        beta = E._betas(B, grp) if k == 1 else E._betas(B, grp, E.STEPS)
        what = f"{_what(c, B, both)} G={grp} swap_every={k} first_parity={fp} steps_per_launch={spl}"
        ref_smp = E._sampler(la, c.T, c.X, B, both)
        ref = ref_smp.run_hmc_exchange(E.STEPS, beta, x0, eps=eps, keep_samples=True, replicas=grp, swap_every=k,
                                       first_parity=fp)
        smp = E._sampler(la, c.T, c.X, B, both, spl, in_launch=True)
        got = {}

        def run():
            got["out"] = smp.run_hmc_exchange(E.STEPS, beta, x0, eps=eps, keep_samples=True, replicas=grp,
                                              swap_every=k, first_parity=fp)
        assert count_launches(8, run) == 0, what                     # no launch of the round on its own
        E._assert_same(got["out"], ref, smp, ref_smp, what)
        exchanged += int(ref["swapped"].sum())
    print(f"hmc geometry exchange {_what(c, B, both)} G={grp}: workgroups of {cpw} chains, {threads} threads; "
          f"{exchanged} exchanges")
    if B >= 72:                                                      # 18 groups or more, as in the file that owns it
        assert exchanged > 0


# ----------------------------------------------------------------- 6. the layered cross-check
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X", [(8, 16), (10, 10), (17, 17), (19, 27)])
def test_kernel_matches_layered_path(la, T, X, both):
    """tsh 7 (full and ragged), spt 2 ragged and spt 4 ragged with a slice of one live lane"""
    c = next(k for k in G.CASES if (k.T, k.X) == (T, X))
    _compare_paths(T, X, G.batch(c, both), both)
