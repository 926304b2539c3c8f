"""Host side of tests/test_gpu_nonfinite.py: the case table of tests/nonfinite_cases.py meets its conditions on the NumPy
oracle alone.  No GPU; sizes that follow the device are taken at 256 compute units.

For every case and every kind of poison it takes:
  - the oracle is chain-local: every other chain has the same bits in the poisoned and in the benign call, and is finite;
  - the bad chain has p = 0, in float32 and in float64, and both precisions have the same NaN / inf pattern (the GPU
    test gates the finite entries of a poisoned chain against float64 under the entry's parity bar);
  - a network case: x_prop, v_prop and x_out are NaN in EVERY link, and the oracle with a NaN-dropping relu
    (`relu_drops_nan`: fmaxf) gives a DIFFERENT pattern, with the counts measured when the cases were chosen (8x8
    GenericNet at N = 3: 47 of 128 links for a poisoned link, 23 for a poisoned momentum; N = 1: 7 and 1; 4x4: 31 and
    22 of 32; ConvNet3D at N = 2: 23 and 7): a device relu that drops a NaN fails exactly these cases;
  - a plain-HMC case: the pattern is the stencil's reach, a strict subset of the links from 32 sites on;
  - every kernel family of the table has a case, the 32-row case is a 32-row launch whose bad chains sit in the first and
    in the last workgroup, and every threads-per-row class of tests/hmc_geometry_cases.py has a lattice.
The unwrapped-links half (tests/unwrapped_cases.py) is described where it begins.  The file runs in 14 s."""
import numpy as np
import pytest

from tests import hmc_geometry_cases as G
from tests import nonfinite_cases as NF

NETWORK = [c for c in NF.LATTICE_CASES if c.arch != "hmc"]
HMC = [c for c in NF.LATTICE_CASES if c.arch == "hmc"]
# NaN links of x_prop under the NaN-dropping relu: (lattice or arch, N) -> (poisoned link, poisoned momentum)
DROPPED = {("generic", 8, 8, 3): (47, 23), ("generic", 8, 8, 1): (7, 1), ("generic", 4, 16, 3): (38, 22),
           ("generic", 4, 4, 3): (31, 22), ("generic", 6, 6, 3): (46, 23), ("conv3D", 8, 8, 2): (23, 7),
           ("conv3D", 4, 16, 2): (22, 7)}


def _rows(c):
    """The chains the oracle is run on: all of a small batch; of a big one the bad chains and their neighbours."""
    B = NF.chains(c)
    if B <= 21:
        return np.arange(B)
    bad = NF.bad_chains(c)
    return np.unique(np.clip([b + d for b in bad for d in (-1, 0, 1)], 0, B - 1))


def _runs(c, kind, dtype=np.float32):
    rows = _rows(c)
    clean = NF.clean_inputs(c, draws=NF.host_step_draws(rows))
    bad, benign = NF.poison(c, kind, clean)
    at = [int(np.flatnonzero(rows == b)[0]) for b in NF.bad_chains(c)]
    return NF.reference(c, bad, rows, dtype), NF.reference(c, benign, rows, dtype), at, bad, rows


@pytest.mark.parametrize("c", NF.LATTICE_CASES, ids=lambda c: c.name)
def test_the_oracle_is_chain_local_and_rejects_the_poisoned_chain(c):
    for kind in NF.kinds(c):
        got, ok, at, bad, rows = _runs(c, kind)
        others = np.ones(len(rows), bool)
        others[at] = False
        for k in got:
            assert np.array_equal(got[k][others], ok[k][others]), (kind, k)
            assert np.isfinite(ok[k]).all(), (kind, k)
        g64 = NF.reference(c, bad, rows[at], np.float64)
        for j, i in enumerate(at):
            assert got["p"][i] == 0 and g64["p"][j] == 0
            for k in got:
                assert NF.same_pattern(got[k][i], g64[k][j]), (kind, k)
            if c.entry == "step":
                for k in ("action", "avg_plaq", "top_charge", "dq"):
                    assert np.isnan(got[k][i]), (kind, k)
                assert np.array_equal(np.isnan(got["x_next"][i]), np.isnan(got["x_out"][i]))
                assert not np.isinf(got["x_next"][i]).any()


@pytest.mark.parametrize("c", NETWORK, ids=lambda c: c.name)
def test_a_nan_dropping_relu_gives_another_pattern(c):
    assert c.pattern
    D = NF.dim(c)
    for kind in NF.kinds(c):
        got, _, at, bad, rows = _runs(c, kind)
        with NF.relu_drops_nan():
            dropped = NF.reference(c, bad, rows)
        for i in at:
            for k in ("x_prop", "v_prop", "x_out"):
                assert np.isnan(got[k][i]).all(), (kind, k)
            n = int(np.isnan(dropped["x_prop"][i]).sum())
            want = DROPPED[(c.arch, c.T, c.X, c.N)][kind == "nanv"]
            print(f"[nonfinite host] {c.name} {kind}: x_prop NaN in {D} of {D} links, with a NaN-dropping relu in {n}")
            assert n == want < D, (kind, n, want)
            assert not NF.same_pattern(got["x_prop"][i], dropped["x_prop"][i])
            assert not NF.same_pattern(got["x_out"][i], dropped["x_out"][i])
            assert dropped["p"][i] == 0


@pytest.mark.parametrize("c", HMC, ids=lambda c: c.name)
def test_plain_hmc_spreads_a_nan_by_the_stencil_alone(c):
    assert not c.pattern
    D = NF.dim(c)
    for kind in NF.kinds(c):
        got, _, at, bad, rows = _runs(c, kind)
        with NF.relu_drops_nan():
            dropped = NF.reference(c, bad, rows)
        for i in at:
            n = int(np.isnan(got["x_prop"][i]).sum())
            print(f"[nonfinite host] {c.name} {kind}: x_prop NaN in {n} of {D} links")
            assert 0 < n <= D and (n < D or c.T * c.X < 32), (kind, n)
            assert np.array_equal(np.isnan(got["x_out"][i]), np.isnan(got["x_prop"][i]))
            for k in got:
                assert NF.same_pattern(got[k][i], dropped[k][i]), (kind, k)      # no network, no relu


def test_every_family_and_every_geometry_class_has_a_case():
    have = {c.family for c in NF.LATTICE_CASES} | {"toy"}
    assert have == set(NF.FAMILIES)
    for fam in ("16-row", "sub-tile", "32-row", "split", "ladder", "conv3d whole-step", "conv3d layered", "layered"):
        assert any(c.family == fam and c.pattern for c in NF.LATTICE_CASES), fam
    assert {G.geom(T, X)[1] for T, X in NF.HMC_LATTICES} == {G.geom(c.T, c.X)[1] for c in G.CASES}
    assert all(c.N in (1, 2, 3) for c in NETWORK)
    assert len(NF.TOY_CASES) >= 2 and NF.TOY_BATCHES == (37, 1)


def test_the_32_row_case_is_a_32_row_launch_with_a_bad_chain_in_its_first_and_last_workgroup():
    c = NF.BY_NAME["step-rows32"]
    for cus in (NF.HOST_CUS, 64, 304):
        B = NF.chains(c, cus)
        parts = NF.step_plan(2 * B, cus)
        assert not any(w == 32 for _, w in NF.step_plan(2 * (B - 1), cus)), (cus, B)
        assert parts[0][1] == 32 and all(w == 32 for _, w in parts), (cus, parts)     # one form: nothing but 32-row tiles
        first, last = NF.bad_chains(c, cus)
        assert first < 16 and last == B - 1 and last // 16 == -(-B // 16) - 1, (cus, B, first, last)
    assert NF.chains(c) == 3073


def test_small_cases_take_the_form_they_name():
    for c in NF.LATTICE_CASES:
        if c.arch == "generic" and c.family == "sub-tile":
            rows = NF.chains(c) * (2 if c.both else 1)
            assert [w for _, w in NF.step_plan(rows, NF.HOST_CUS)] == [4], c.name
        if c.family in ("16-row", "split"):
            assert dict(c.flags).get("tiles16_only"), c.name


# ---- toy targets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", NF.TOY_BATCHES)
@pytest.mark.parametrize("c", NF.TOY_CASES, ids=NF.toy_id)
def test_toy_oracle_is_chain_local_and_the_relu_decides_the_pattern(c, B):
    clean = NF.toy_inputs(c, B)
    b = NF.toy_bad(B)
    others = np.arange(B) != b
    for kind in NF.KINDS_APPLY:
        bad, benign = NF.toy_poison(c, kind, clean)
        got, ok = NF.toy_reference(c, bad), NF.toy_reference(c, benign)
        g64 = NF.toy_reference(c, bad, np.float64)
        with NF.relu_drops_nan():
            dropped = NF.toy_reference(c, bad)
        for k in NF.TOY_NAMES:
            assert np.array_equal(got[k][others], ok[k][others]) and np.isfinite(ok[k]).all(), (kind, k)
            assert NF.same_pattern(got[k][b], g64[k][b]), (kind, k)
        assert got["px"][b] == 0 and got["pf"][b] == 0 and got["pb"][b] == 0
        for k in ("Xf", "Vf", "Xb", "Vb", "Lx", "Lv"):
            assert np.isnan(got[k][b]).all(), (kind, k)
        # a rejected chain keeps its state: sampler.py:57-59 selects, it does not multiply
        assert np.array_equal(got["x_out"][b], bad["x"][b].astype(np.float32), equal_nan=True)
        n = int(np.isnan(dropped["Lx"][b]).sum())
        print(f"[nonfinite host] toy {NF.toy_id(c)} B={B} {kind}: Lx NaN in {c.dim} of {c.dim}, NaN-dropping relu {n}")
        # a poisoned coordinate reaches the others through the force's matrix product (0 x NaN) whatever the relu does: the
        # x kinds are isolation cases; the poisoned momentum is the pattern case (1 coordinate of dim with fmaxf)
        if kind == "nanv":
            assert n == 1 < c.dim and not NF.same_pattern(got["Lx"][b], dropped["Lx"][b]), n
        else:
            assert n == c.dim


@pytest.mark.parametrize("B", NF.TOY_BATCHES)
@pytest.mark.parametrize("c", NF.TOY_CASES, ids=NF.toy_id)
def test_toy_oracle_run_keeps_the_poisoned_chain_rejected_and_alone(c, B):
    """The run of tests/test_gpu_nonfinite.py::test_a_poisoned_chain_in_the_toy_run on the oracle, with the run's draws
    restated on the host: in each of the 3 steps the other chains have the bits of the benign run, the bad chain has
    px = 0 and keeps its input's bits; the NaN-dropping relu gives the same, so these are isolation cases; and the benign
    run accepts most proposals, so the other chains' states do move."""
    clean = NF.toy_inputs(c, B)
    b = NF.toy_bad(B)
    others = np.arange(B) != b
    draws = NF.toy_host_draws(B, c.dim)
    assert len({float(draws(s)[3][0]) for s in range(NF.TOY_RUN_STEPS)}) == NF.TOY_RUN_STEPS      # a stream per step
    for kind in NF.KINDS_STEP:
        bad, benign = NF.toy_poison(c, kind, clean)
        px, xs = NF.toy_run_reference(c, bad["x"], draws)
        ok_px, ok_xs = NF.toy_run_reference(c, benign["x"], draws)
        px64, xs64 = NF.toy_run_reference(c, bad["x"], draws, dtype=np.float64)
        with NF.relu_drops_nan():
            dpx, dxs = NF.toy_run_reference(c, bad["x"], draws)
        assert px.shape == (NF.TOY_RUN_STEPS, B) and xs.shape == (NF.TOY_RUN_STEPS, B, c.dim)
        assert np.isfinite(ok_px).all() and np.isfinite(ok_xs).all()
        assert np.array_equal(px[:, others], ok_px[:, others]) and np.array_equal(xs[:, others], ok_xs[:, others])
        x_in = bad["x"][b].astype(np.float32)
        for s in range(NF.TOY_RUN_STEPS):
            assert px[s, b] == 0 and px64[s, b] == 0 and dpx[s, b] == 0, (kind, s)
            assert np.array_equal(xs[s, b], x_in, equal_nan=True) and np.array_equal(dxs[s, b], x_in, equal_nan=True)
            assert NF.same_pattern(xs[s, b], xs64[s, b])
        if B > 1:
            assert (ok_xs[0] != benign["x"].astype(np.float32)).any(axis=1).sum() > B // 2, kind     # chains do move


# ---- unwrapped links (tests/unwrapped_cases.py) -------------------------------------------------------------------------
# Host side of tests/test_gpu_unwrapped_links.py.  The links lie on the grid and within their class, every plaquette is
# exact in float32 in three groupings of its four terms, none lies within 1e-2 of the charge's branch cut, the |x| <= 4096
# class has at least 5 % of its plaquettes on either path of fast_sincos (measured: 0.92 / 0.08) and the constructed chain
# holds +-8192 and the last float32 below it.  A float64 reference whose sine and cosine are 0 from |P| = 8192 on, or
# on 4096 <= |P| < 8192 only, misses the bars of the GPU test by the factor SEES = 100 of tests/toy_cases.py or more:
# measured 5.6e3 ... 3.1e6 for action, force, plaquette and HVP, 400 ... 825 for v_prop and 162 for x_prop of the one-launch step.
from oracle import lattice as olat                     # noqa: E402
from tests import helpers as H                         # noqa: E402
from tests import toy_cases as tc                      # noqa: E402
from tests import unwrapped_cases as U                 # noqa: E402


@pytest.mark.parametrize("T,X,standalone", [(T, X, True) for T, X in U.LATTICES] + [(T, X, False) for T, X in U.HMC_LATTICES])
@pytest.mark.parametrize("cls", list(U.CLASSES))
def test_unwrapped_links_meet_their_conditions(cls, T, X, standalone):
    """`standalone`: the batch of the standalone entries; otherwise the start of the one-launch kernels, whose whole steps
    (plain HMC, the torus-exact kernel and the reference mode's whole-step kernels at 8x8) measure the charge of it."""
    x = U.links(T, X, cls) if standalone else U.hmc_inputs(T, X, cls)[0]
    M = U.CLASSES[cls]
    body = x[:-1] if standalone and cls == "both" else x
    assert np.abs(x).max() <= M and np.array_equal(body / U.GRID, np.round(body / U.GRID))
    s = x.reshape(-1, T, X, 2)
    x0, x1, x0r, x1r = s[..., 0], s[..., 1], np.roll(s[..., 0], -1, axis=2), np.roll(s[..., 1], -1, axis=1)
    P64 = olat.plaq_sums(x.astype(np.float64), T, X)
    for P32 in (((x0 - x1) - x0r) + x1r, (x0 + x1r) - (x1 + x0r), (x0 - x0r) + (x1r - x1)):
        assert P32.dtype == np.float32 and np.array_equal(P32.astype(np.float64), P64)     # exact in any grouping
    assert U.cut_distance(P64).min() >= U.CUT_MARGIN
    poly, libm = U.path_fractions(x, T, X)
    print(f"[unwrapped host] {T}x{X} |x| <= {M:g}: {poly:.3f} of the plaquettes on the polynomial path, {libm:.3f} on libm's; "
          f"max |P| {np.abs(P64).max():.1f}")
    if cls == "both":
        assert poly >= 0.05 and libm >= 0.05
    else:
        assert libm == 0
    if cls == "small":
        assert (x < 0).mean() > 0.3 and (x > 2 * np.pi).mean() > 0.05
    if cls == "poly":
        assert np.abs(P64).max() / (np.pi / 2) > 1000                                     # quadrant counts in the thousands
    if standalone and cls == "both":
        edge = olat.plaq_sums(x[-1:].astype(np.float64), T, X).reshape(-1)
        for want in U.EDGE_PLAQUETTES:
            assert (edge == want).any(), want
        assert np.float32(U.SWITCH - 2.0 ** -11) < np.float32(U.SWITCH) == np.nextafter(np.float32(U.SWITCH - 2.0 ** -11),
                                                                                           np.float32(1e9))


@pytest.mark.parametrize("T,X", U.LATTICES)
def test_a_wrong_sine_on_either_side_of_the_switch_misses_the_standalone_bars(T, X):
    x, u = U.links(T, X, "both"), U.tangent(T, X)
    want, bar = U.reference(x, u, T, X), U.bars(x, u, T, X)
    for wrong in (U.wrong_from_the_switch_on, U.wrong_below_the_switch):
        got = U.reference(x, u, T, X, sincos=wrong)
        for k in ("action", "force", "avg_plaq", "hvp"):
            err = np.abs(got[k] - want[k])
            err = err.reshape(err.shape[0], -1).max(axis=1)
            miss = float(np.max(err / bar[k]))
            print(f"[unwrapped host] {T}x{X} {wrong.__name__} {k}: misses its bar by {miss:.3g}")
            assert miss >= tc.SEES, (wrong.__name__, k, miss)
        assert np.array_equal(got["top_charge"], want["top_charge"])                      # no sine in the charge
    for k, b in bar.items():
        assert np.all(np.asarray(b) > 0) and np.all(np.asarray(b) < 1e-2), (k, b)
    # the same float64 numbers as the oracle's own functions
    x64 = np.asarray(x, dtype=np.float64)
    assert np.allclose(want["action"], olat.total_action(x64, T, X), rtol=0, atol=1e-9)
    assert np.allclose(want["force"], U.BETA * olat.grad_action(x64, T, X), rtol=0, atol=1e-12)
    assert np.allclose(want["top_charge"], olat.top_charge(x64, T, X), rtol=0, atol=1e-9)
    h = 2.0 ** -20                                                                         # hvp: a central difference
    fd = U.BETA * (olat.grad_action(x64 + h * u, T, X) - olat.grad_action(x64 - h * u, T, X)) / (2 * h)
    assert np.abs(fd - want["hvp"]).max() < 1e-4


@pytest.mark.parametrize("T,X", U.HMC_LATTICES)
def test_a_wrong_sine_misses_the_bars_of_the_one_launch_step(T, X):
    x, v0f, _, _, _ = U.hmc_inputs(T, X, "both")
    o64 = H.gauge_oracle(T, X, 1, U.HMC_EPS, None, None, hmc=True)
    o32 = H.gauge_oracle(T, X, 1, U.HMC_EPS, None, None, hmc=True, dtype=np.float32)
    o64.eps = float(np.float32(U.HMC_EPS))
    w64 = o64.transition_kernel(x.astype(np.float64), U.HMC_BETA, v0f.astype(np.float64), forward=True)
    w32 = o32.transition_kernel(x, U.HMC_BETA, v0f, forward=True)
    own = U.hmc_n1(x, v0f, T, X)
    assert np.abs(own[0] - w64[0]).max() < 1e-9 and np.abs(own[1] - w64[1]).max() < 1e-9
    assert np.abs(own[2] - w64[2]).max() < 1e-9
    bar_v, bar_p = tc.max_bar(w64[1], w32[1]), tc.p_bar(w64[2], w32[2])
    bar_x = U.bar_x_prop(w64[0], v0f)
    for wrong in (U.wrong_from_the_switch_on, U.wrong_below_the_switch):
        got = U.hmc_n1(x, v0f, T, X, sincos=wrong)
        miss = dict(v_prop=H.relerr(got[1], w64[1]) / bar_v, p=np.abs(got[2] - w64[2]).max() / bar_p,
                    x_prop=np.abs(got[0] - w64[0]).max() / bar_x)
        print(f"[unwrapped host] hmc {T}x{X} {wrong.__name__}: misses the bars by "
              + ", ".join(f"{k} {m:.3g}" for k, m in miss.items()) + f" (bars v {bar_v:.2e} p {bar_p:.2e} x {bar_x:.2e})")
        # p does not tell at this magnitude, under its own rule: x' = x + eps v' is rounded to ulp(4096) = 4.9e-4 in float32,
        # so the float32 oracle's dH, and with it the bar on p, is off by more than the wrong sine moves it (figures above;
        # at 32x32 every p is clipped to 1).  v' and x' do tell.
        assert miss["v_prop"] >= tc.SEES and miss["x_prop"] >= tc.SEES, miss


def test_a_wrong_sine_misses_the_bars_of_the_torus_exact_step():
    """The same for tests/test_gpu_unwrapped_links.py::test_torus_exact_whole_step_from_unwrapped_links at |x| <= 4096: the
    float64 reference of tests/periodic_ref.py with a sine of the plaquettes that is wrong on one side of the switch."""
    from tests import periodic_ref as PR
    T = X = 8
    x, v0f, v0b, coin, u = U.hmc_inputs(T, X, "both")
    r64, r32 = U.torus_references()
    w64 = [np.asarray(a, dtype=np.float64) for a in r64.apply_transition(x, U.HMC_BETA, v0f, v0b, coin, u)]
    w32 = [np.asarray(a, dtype=np.float64) for a in r32.apply_transition(x, U.HMC_BETA, v0f, v0b, coin, u)]
    bar_v, bar_p = tc.max_bar(w64[1], w32[1]), tc.p_bar(w64[2], w32[2])
    bar_x = U.bar_x_angle(x, w64[0], float(PR.angdist(w32[0], w64[0]).max()), tc.MAX_RATIO)
    for wrong in (U.wrong_from_the_switch_on, U.wrong_below_the_switch):
        got = [np.asarray(a, dtype=np.float64)
               for a in U.torus_references(wrong)[0].apply_transition(x, U.HMC_BETA, v0f, v0b, coin, u)]
        miss = dict(v_prop=H.relerr(got[1], w64[1]) / bar_v, p=np.abs(got[2] - w64[2]).max() / bar_p,
                    x_prop=float(PR.angdist(got[0], w64[0]).max()) / bar_x)
        print(f"[unwrapped host] torus-exact 8x8 {wrong.__name__}: misses the bars by "
              + ", ".join(f"{k} {m:.3g}" for k, m in miss.items()) + f" (bars v {bar_v:.2e} p {bar_p:.2e} x {bar_x:.2e})")
        # (here p tells as well: the proposal of this mode is rounded on the circle, not at ulp(4096))
        assert miss["v_prop"] >= tc.SEES and miss["p"] >= tc.SEES and miss["x_prop"] >= 10, miss
