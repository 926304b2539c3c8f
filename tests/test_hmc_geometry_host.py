"""Host side of tests/test_gpu_hmc_geometry.py: the case table of tests/hmc_geometry_cases.py covers every
thread-geometry class of the one-launch plain-HMC kernels (l2hmc_amd/csrc/hmc_step.hip), its restatement of the host rule
agrees with the library, every case meets the conditions on its inputs on the float64 oracle, and a perturbed oracle
misses every gate of the GPU test by more than ten times.  No GPU."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from l2hmc_amd import _lib
from oracle import lattice as olat
from tests import hmc_geometry_cases as G
from tests import philox_ref
from tests.test_hmc_run_exchange_host import SEL, _plan, _rule
from tests.toy_cases import MAX_RATIO, TOL_OP, p_bar

X_NEXT_TOL = 5e-5                                        # tests/test_gpu_hmc_step.py
BITES = 10.0


def _reachable():
    """every (spt, tsh, ragged) of a lattice of 1 .. 1024 sites (the rule takes T and X through their product alone)"""
    return {(g[0], g[1], g[4]) for g in (G.geom(1, s) for s in range(1, G.MAX_SITES + 1))}


# ------------------------------------------------------------------------------------------------ the table
def test_the_rule_depends_on_the_product_alone_and_has_the_stated_classes():
    for T, X in [(3, 5), (5, 3), (8, 16), (16, 8), (1, 257), (257, 1), (19, 27), (27, 19)]:
        assert G.geom(T, X) == G.geom(1, T * X)
    classes = _reachable()
    # tsh 0 .. 8 at one site per thread, 8 alone at two and four; a row of 1 or 2 sites is never ragged
    assert {(s, t) for s, t, _ in classes} == {(1, t) for t in range(9)} | {(2, 8), (4, 8)}
    assert {k for k in classes if k[2]} == {(1, t, True) for t in range(2, 9)} | {(2, 8, True), (4, 8, True)}
    assert all((s, t, False) in classes for s, t, _ in classes)
    for bad in [(0, 8), (8, 0), (2, 513), (33, 32)]:
        with pytest.raises(ValueError):
            G.geom(*bad)


def test_table_covers_every_reachable_class_and_the_stated_lattices():
    have = {G.class_of(c) for c in G.CASES}
    assert have == _reachable()
    lattices = {(c.T, c.X) for c in G.CASES}
    assert len(lattices) == len(G.CASES)
    stated = [(1, 1), (1, 2), (2, 2), (1, 3), (2, 4), (2, 3), (1, 7), (5, 3), (4, 8), (5, 5), (7, 9), (3, 11), (11, 3),
              (64, 1), (2, 32), (8, 16), (16, 8), (10, 10), (9, 9), (12, 12), (15, 17), (16, 32), (17, 17), (20, 20),
              (1, 257), (257, 1), (19, 27), (24, 24), (31, 33)]
    assert set(stated) <= lattices
    # the slices of a thread that own no site at all: 513 sites on 256 lanes leave one live lane in slice 2, none in 3
    assert G.geom(19, 27) == (4, 8, 512, 2, True) and 19 * 27 - 2 * 256 == 1
    # the equality cases: the full and the ragged class of every (spt, tsh)
    assert {G.class_of(c) for c in G.equality_cases()} == _reachable()
    assert len(G.equality_cases()) == len(_reachable())
    # exactly one case is exempt from the accept / reject conditions, and it is the one-site lattice
    assert [(c.T, c.X) for c in G.CASES if not c.mixed] == [(1, 1)]


def test_batches_fill_a_workgroup_and_leave_the_last_one_partial():
    for c in G.CASES:
        tiny = c.T * c.X <= G.TINY_SITES
        for both in (True, False):
            B, cpw = G.batch(c, both), G.chains_per_workgroup(c.T, c.X, both)
            assert 1 <= B <= (G.TINY_BATCH if tiny else G.BATCH), (c, both)
            if cpw == 1:
                assert both and G.batch(c, False) % 2 == 1, c        # the selected-only launch gets the half-filled one
            else:
                assert B % cpw != 0, (c, both)                       # the last workgroup is partial
                if tiny:
                    assert B == min(cpw + 1, G.TINY_BATCH), (c, both)
                assert B > cpw or B == G.TINY_BATCH, (c, both)       # ... and one ahead of it is full
        # a full workgroup exists in at least one of the two launches of every case
        assert any(G.batch(c, b) > G.chains_per_workgroup(c.T, c.X, b) for b in (True, False)), c


# ------------------------------------------------------------------------------------------------ geom and the library
def _served_by_geom(T, X, flags, grp):
    spt, tsh, _, R, _ = G.geom(T, X)
    rpc = 1 if flags & SEL else 2
    rows = math.lcm(grp, R // rpc) * rpc
    return spt <= 2 and rows << tsh <= 1024 and 4 * (rows * (5 * T * X + 18) + 512) <= 64 * 1024


def test_geom_agrees_with_the_library():
    """The exchange run's served rule is a function of the threads per row and the rows per workgroup, and the text of
    its refusal names both: the grid of tests/test_hmc_run_exchange_host.py, on the lattices of the table."""
    L = _lib.lib()
    for c in G.CASES:
        spt, tsh, threads, R, _ = G.geom(c.T, c.X)
        for flags in (0, SEL):
            plan = _plan(c.T, c.X, flags=flags)
            for grp in range(2, 40):
                got = L.l2hmc_gauge_hmc_run_exchange_served(C.byref(plan), grp)
                assert got == int(_served_by_geom(c.T, c.X, flags, grp)) == int(_rule(c.T, c.X, flags, grp)), (c, grp)
            # a prime group beyond 1024: lcm(group, cpw0) = group * cpw0, refused by the thread count on every lattice
            assert L.l2hmc_gauge_hmc_run_exchange_served(C.byref(plan), 1031) == 0
            msg = L.l2hmc_last_error().decode()
            m = re.search(r"takes (\d+) threads per row and (\d+) row\(s\) per chain.*ladder-run workgroups of (\d+) "
                          r"chains", msg)
            assert m, msg
            rpc = 1 if flags & SEL else 2
            assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (1 << tsh, rpc, R // rpc), (c, msg)
            assert R << tsh == threads
        for both in (True, False):
            grp = G.exchange_group(c.T, c.X, both)
            plan = _plan(c.T, c.X, flags=0 if both else SEL)
            if grp is None:
                assert spt == 4 or c.T * c.X == 1, c
                assert not any(L.l2hmc_gauge_hmc_run_exchange_served(C.byref(plan), g) for g in (2, 3, 4))
            else:
                assert L.l2hmc_gauge_hmc_run_exchange_served(C.byref(plan), grp) == 1
    # the three workgroups of the exchange test that are no power of two, or the full 1024
    for (T, X, both, grp), want in {(10, 10, True, 3): 768, (2, 2, True, 3): 768, (17, 17, True, 2): 1024}.items():
        _, tsh, _, R, _ = G.geom(T, X)
        rpc = 2 if both else 1
        assert (math.lcm(grp, R // rpc) * rpc) << tsh == want


# ------------------------------------------------------------------------------------------------ the conditions
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_case_meets_the_conditions_on_the_float64_oracle(c):
    """At the committed (eps, draw), on the reference Philox draws, at both batches of the case."""
    for B in sorted({c.B, c.B_sel}):
        f = G.reference_figures(c, B)
        print(f"{c.T}x{c.X} B={B} eps={c.eps} draw={c.draw}: {f}")
        assert f["margin"] >= G.MARGIN, (c, B, f)
        if c.mixed:
            assert f["accepted"] >= 2 and f["rejected"] >= 2, (c, B, f)
            assert f["interior"] >= (1 if c.T * c.X > 512 else 2), (c, B, f)
        else:
            assert f["rejected"] == 0 and f["interior"] == 0, (c, B, f)
        assert G.conditions_hold(c, f)
    x = G.start(c, c.B)
    assert x.dtype == np.float32 and x.min() >= 0 and x.max() <= np.float32(6.283)


# ------------------------------------------------------------------------------------------------ the tests bite
def _circle(a, b):
    d = np.mod(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)), 2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def _wrong_force(axis):
    """the force with the FORWARD neighbour's sin P in place of the backward one's along `axis` (nr for nl, nu for nd)"""
    def grad(x, T, X):
        sp = np.sin(olat.plaq_sums(x, T, X))
        g = np.empty(sp.shape + (2,), dtype=sp.dtype)
        g[..., 0] = sp - np.roll(sp, -1 if axis == 2 else 1, axis=2)
        g[..., 1] = -sp + np.roll(sp, -1 if axis == 1 else 1, axis=1)
        return g.reshape(g.shape[0], -1)
    return grad


def _action_without_the_last_site(x, T, X):
    p = olat.plaq_sums(x, T, X)
    return np.sum(1.0 - np.cos(p), axis=(1, 2)) - (1.0 - np.cos(p[:, T - 1, X - 1]))


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_a_perturbed_oracle_misses_every_gate_tenfold(c, monkeypatch):
    """What the GPU test would see of a kernel with a wrong neighbour in the force, or one that left the last site of a
    row out of the action: the outputs of such an oracle against the true one, in units of the gates."""
    B, D = c.B, 2 * c.T * c.X
    x = G.start(c, B).astype(np.float64)
    draws = philox_ref.lattice_step(G.SEED, c.draw, B, D)
    want = G.oracle(c).apply_transition(x, c.beta, *draws)
    w32 = G.oracle(c, np.float32).apply_transition(x.astype(np.float32), c.beta, *(d.astype(np.float32) for d in draws))
    acc = want[2] > draws[3]
    gate_p = p_bar(want[2], w32[2])
    gate_x = max(X_NEXT_TOL, MAX_RATIO * float(_circle(w32[0], want[0])[acc].max())) if acc.any() else X_NEXT_TOL
    print(f"{c.T}x{c.X}: gates p {gate_p:.2e} x_next {gate_x:.2e}")
    assert gate_p < 1e-3 and gate_x < 1e-3                           # the gates themselves stay tight
    seen = 0
    # -- a wrong neighbour in the force: visible along an extent of 3 or more (at 1 and 2 both neighbours coincide)
    for axis, extent in ((2, c.X), (1, c.T)):
        if extent < 3:
            continue
        monkeypatch.setattr(olat, "grad_action", _wrong_force(axis))
        bad = G.oracle(c).apply_transition(x, c.beta, *draws)
        monkeypatch.undo()
        dp, dx = np.abs(bad[2] - want[2]).max(), _circle(bad[0], want[0])[acc].max()
        print(f"  wrong force neighbour along axis {axis}: p {dp:.2e} ({dp / gate_p:.0f} gates), proposal {dx:.2e} "
              f"({dx / gate_x:.0f} gates)")
        assert dx > BITES * gate_x, (c, axis)
        assert dp > BITES * gate_p, (c, axis)
        seen += 1
    # -- the last site left out of the action (the last lane of a ragged row): the accept probability and the
    #    observables of the input; invisible only where P = 0 identically
    if c.mixed:
        monkeypatch.setattr(olat, "total_action", _action_without_the_last_site)
        bad = G.oracle(c).apply_transition(x, c.beta, *draws)
        da = np.abs(olat.total_action(x, c.T, c.X) - want_action(x, c)).max() / max(1.0, want_action(x, c).max())
        monkeypatch.undo()
        dp = np.abs(bad[2] - want[2]).max()
        print(f"  last site left out of the action: p {dp:.2e} ({dp / gate_p:.0f} gates), action {da:.2e} "
              f"({da / TOL_OP:.0f} gates)")
        assert dp > BITES * gate_p and da > BITES * TOL_OP, c
        seen += 1
    assert seen > 0 or not c.mixed


def want_action(x, c):
    return np.sum(1.0 - np.cos(olat.plaq_sums(x, c.T, c.X)), axis=(1, 2))
