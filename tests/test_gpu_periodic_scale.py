"""The torus-exact mode's one-launch kernels (`GaugeDynamics(periodic=True, whole_step=True)`,
l2hmc_amd/csrc/fused_traj_ncp.hip) at the benchmark's trajectory length and at batches that fill the chip more than once:
what tests/test_gpu_periodic_step.py (N = 3, at most 19 chains and three workgroups) cannot see.  The cases, their
inputs and the conditions on them are tests/periodic_scale_cases.py, proven on the CPU by
tests/test_periodic_scale_host.py.

a. N = 10 (step indices 3 .. 9: the mask row, the time feature of backward rows N - 1 - step, the kept VNet product
   across nine step boundaries), 19 chains paired and selected-only, 8x8 and 4x16.
b. N = 3 at CUS + 1 workgroups (CUS = the device's compute units; the kernel's LDS use allows one workgroup per CU, so
   the last workgroup runs in a second round): the rows of workgroups 0, CUS - 1 and CUS (the last: two rows / one
   chain) have the bits of a launch of exactly those rows -- a workgroup's arithmetic has no business depending on
   blockIdx -- and every row is gated against float64.
c. the whole step at those batches: observables, the sums' last-arriver tree over CUS + 1 partials, the ticket.
d. the ladder's per-chain beta at thousands of rows: every column bit equal to the uniform step at its rung.
e. a chain holding inf or NaN does not reach the other fifteen rows of its tile.

Gates are those of tests/test_gpu_periodic_step.py: against the float64 reference, per output GATE = 4 times the larger
of the float32 NumPy reference's error and the layered device path's (`whole_step=False`) error; positions by angular
distance.  At N = 10 the yardstick is also capped at 2.5e-5, so no gate is looser than the 1e-4 of the existing
trajectory tests.  Nothing is compared with the kernel under test except where bit equality of two launches of it is
the claim.  Every case prints error / yardstick or figure / bar.

Measured on the MI355X (256 CUs), worst error / yardstick (gate 4): a. transition_kernel 1.75 (4x16, backward, p: 4.4e-5
against the capped 2.5e-5), apply_transition 1.75 (the same chain), GaugeSampler.step 0.94; stress: max p 3.2e-13; log-det
regrouping 3.0e-7 / 1.5e-5.  b. trajectory entry at 4098 rows 1.04, apply_transition 1.16 (2049 paired) and 1.01 (4097
selected-only); every tile bit equal to its own launch; a neighbour's chain in the last workgroup misses the gate by 4e5.
c. whole step 0.99 / 0.97; action 3.1e-7, plaquette 1.2e-7, charge 1.6e-7, |dQ| 2.4e-7; sums within 0.20 (px) and 0.52 (dq)
of their bars; ticket 0 after each of three steps.  d. 683 / 1366 columns per rung bit equal.  e. tile-mates bit equal on
both paths, and the chain itself NaN in all 128 links as in the reference (47 and 23 of 128 before the kernels' relu
handed a NaN on: see test_a_poisoned_chain_shows_the_references_nan_pattern).
The file runs in 10 s, no test over 1.0 s.  More in profiles/periodic_scale.txt."""
import numpy as np
import pytest
import torch

from tests import periodic_ref as PR
from tests import periodic_scale_cases as S
from tests.test_gpu_periodic import _dev, _gate, _hip, _np
from tests.test_gpu_periodic_step import _equal, _fused, _yard2
from tests.test_gpu_periodic_train_forward import _trajectory

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi
ANG_T, ANG_A = ("x",), ("x_prop", "x_out")
WORST = {}                                             # group -> worst error / yardstick, printed by the last test


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dyn(c, B, whole_step=True, **kw):
    """(dynamics of the case, float64 reference, float32 reference)."""
    flags = dict(whole_step=True) if whole_step else {}
    return _hip(c.T, c.X, c.N, c.eps, B, c.regime, both_directions=c.both, **flags, **kw)


def _yards(c, f32, layered, f64, angular):
    """The yardstick rule in force; at N = 10 no yardstick above YARD_CAP."""
    y = _yard2(f32, layered, f64, angular)
    for k, v in y.items():
        assert np.isfinite(v), (c.name, k)
    return {k: min(v, S.YARD_CAP) for k, v in y.items()} if c.N == 10 else y


def _note(group, ratio):
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print(f"[periodic scale] {group}: worst error / yardstick {ratio:.2f} (gate {S.GATE:.0f})")


def _cut(d, keys):
    return {k: d[k] for k in keys}


# ---- a. benchmark length -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in S.N10_CASES])
def test_transition_kernel_at_benchmark_length(name):
    c = S.BY_NAME[name]
    B = S.chains(c)
    ws, r64, r32 = _dyn(c, B)
    lay, _, _ = _dyn(c, B, whole_step=False)
    assert _fused(ws) == 1 and _fused(lay) == 0
    x, v0f, v0b, _, _ = S.inputs(c)
    keys = S.TRAJ_NAMES if c.gates_p else ("x", "v", "sumlogdet")
    for bwd, v0 in ((False, v0f), (True, v0b)):
        run = lambda d: dict(zip(S.TRAJ_NAMES, map(_np, d.transition_kernel(   # noqa: E731
            _dev(x), c.beta, forward=not bwd, momentum=_dev(v0), return_logdet=True))))
        got, layered = run(ws), run(lay)
        f64, f32 = S.traj(r64, x, v0, c.beta, bwd), S.traj(r32, x, v0, c.beta, bwd)
        assert np.abs(f64["sumlogdet"]).mean() > 1e-3
        if c.gates_p:
            assert 0.05 < f64["p"].mean() < 0.95
        else:
            print(f"[periodic scale] {name} bwd={bwd}: max p {got['p'].max():.3e} (bar 1e-6)")
            assert got["p"].max() <= 1e-6 and f64["p"].max() <= 1e-6
        w = _gate(f"N=10 transition_kernel {name} bwd={bwd}", _cut(got, keys), _cut(f64, keys),
                  _yards(c, _cut(f32, keys), _cut(layered, keys), _cut(f64, keys), ANG_T), angular=ANG_T)
        _note("a. transition_kernel N=10", w)


def _apply_case(c, B, x, v0f, v0b, coin, u, ref=S.apply_selected):
    """apply_transition with injected draws: the kernel, the layered path and both references, x_out on the clear chains."""
    ws, r64, r32 = _dyn(c, B)
    lay, _, _ = _dyn(c, B, whole_step=False)
    assert _fused(ws) == 1
    run = lambda d: dict(zip(S.APPLY_NAMES, map(_np, d.apply_transition(   # noqa: E731
        _dev(x), c.beta, momentum_f=_dev(v0f), momentum_b=_dev(v0b), coin=_dev(coin), u=_dev(u)))))
    got, layered = run(ws), run(lay)
    f64, f32 = (ref(r, x, c.beta, v0f, v0b, coin, u) for r in (r64, r32))
    cond = S.conditions(f64, u, f64.pop("sumlogdet"))
    f32.pop("sumlogdet")
    print(f"[periodic scale] {c.name}: clear {cond[0]:.4f} accepted {cond[1]:.3f} mean |sumlogdet| {cond[2]:.3f}")
    assert S.conditions_hold(cond), cond
    clear = S.clear_chains(f64["p"], u)
    for d in (got, layered, f32, f64):
        d["x_out"] = d["x_out"][clear]
    return ws, got, layered, f64, f32, clear


@pytest.mark.parametrize("name", [c.name for c in S.N10_CASES if c.gates_p])
def test_apply_transition_at_benchmark_length(name):
    c = S.BY_NAME[name]
    _, got, layered, f64, f32, _ = _apply_case(c, S.chains(c), *S.inputs(c))
    w = _gate(f"N=10 apply_transition {name}", got, f64, _yards(c, f32, layered, f64, ANG_A), angular=ANG_A)
    _note("a. apply_transition N=10", w)


def _whole_step(dyn, x, beta, steps=1):
    """`steps` GaugeSampler.step calls from draw counter STEP_DRAWS on one sampler (one workspace, successive rows of
    the sums ring) -> the dict of tests/test_gpu_periodic_step.py::_step per call."""
    from l2hmc_amd import GaugeSampler
    dyn._draws = S.STEP_DRAWS
    smp = GaugeSampler(dyn)
    out = []
    for _ in range(steps):
        ring, slot = smp._sums_ring, smp._sums_next
        xn, px, obs, dq = smp.step(x, beta)
        torch.cuda.synchronize()
        out.append(dict(x_next=xn, px=px, action=obs["action"], avg_plaq=obs["avg_plaq"], top_charge=obs["top_charge"],
                        dq=dq, sums=ring[slot].clone()))
    return out


def _step_draws(dyn, B, D, draw):
    """The draws of the step with draw index `draw`: streams 2 draw (momenta of both directions) and 2 draw + 1
    (coin | u), through the library's own generators."""
    from l2hmc_amd import ops
    V = _np(ops.fill_normal((2 * B, D), dyn._seed, 2 * draw, "cuda")).astype(np.float32)
    cu = _np(ops.fill_uniform((2 * B,), dyn._seed, 2 * draw + 1, "cuda")).astype(np.float32)
    return V[:B], V[B:], cu[:B], cu[B:]


def _step_against_float64(c, B):
    """One whole step of case c at B chains: px and, on the clear chains, x_next within the gate.  Returns what the
    other checks of the step need."""
    ws, r64, r32 = _dyn(c, B, seed=S.STEP_SEED)
    lay, _, _ = _dyn(c, B, whole_step=False, seed=S.STEP_SEED)
    assert _fused(ws) == 1 and ws._seed == lay._seed
    x32 = S.start(c, B)
    x = _dev(x32)
    got3 = _whole_step(ws, x, c.beta, steps=3)
    got, layered = got3[0], _whole_step(lay, x, c.beta)[0]
    v0f, v0b, coin, u = _step_draws(ws, B, 2 * c.T * c.X, S.STEP_DRAWS // 2)
    f64, f32 = (S.apply_selected(r, x32, c.beta, v0f, v0b, coin, u) for r in (r64, r32))
    cond = S.conditions(f64, u, f64["sumlogdet"])
    print(f"[periodic scale] {c.name}: clear {cond[0]:.4f} accepted {cond[1]:.3f} mean |sumlogdet| {cond[2]:.3f}")
    assert S.conditions_hold(cond), cond
    clear = S.clear_chains(f64["p"], u)
    acc = _np(got["px"]) > u
    assert np.array_equal(acc[clear], (f64["p"] > u)[clear]) and np.array_equal(acc[clear], (_np(layered["px"]) > u)[clear])
    pick = lambda p, xo: dict(p=np.asarray(p, dtype=np.float64), x_out=np.asarray(xo, dtype=np.float64)[clear])   # noqa: E731
    want = pick(f64["p"], f64["x_out"])
    w = _gate(f"whole step {c.name}", pick(_np(got["px"]), _np(got["x_next"])), want,
              _yards(c, pick(f32["p"], f32["x_out"]), pick(_np(layered["px"]), _np(layered["x_next"])), want, ("x_out",)),
              angular=("x_out",))
    xn = _np(got["x_next"])
    assert xn.min() >= 0 and xn.max() <= TWO_PI
    return ws, x, got3, w


def test_sampler_step_at_benchmark_length():
    c = S.BY_NAME["step-n10"]
    _, _, _, w = _step_against_float64(c, S.chains(c))
    _note("a. GaugeSampler.step N=10", w)


def test_leapfrog_steps_compose_to_the_trajectory_at_benchmark_length():
    """tests/test_gpu_periodic_step.py::test_leapfrog_steps_compose_to_the_trajectory at N = 10: all steps in one call
    give the trajectory's bits; step by step x and v keep them and the log-det is the same terms in another grouping
    (its 1e-5 bound)."""
    c = S.BY_NAME["n10-8x8-mild-paired"]
    B = S.chains(c)
    x32, v0f, v0b, _, _ = S.inputs(c)
    x = _dev(x32)
    dyn = _dyn(c, B)[0]
    for bwd, v0 in ((False, _dev(v0f)), (True, _dev(v0b))):
        xt, vt, _, st = dyn.transition_kernel(x, c.beta, forward=not bwd, momentum=v0, return_logdet=True)
        x1, v1, s1 = dyn._lf(x, v0, c.beta, 0, bwd, step_end=c.N)
        assert torch.equal(x1, xt) and torch.equal(v1, vt) and torch.equal(s1, st)
        xs, vs, ss = x, v0, torch.zeros_like(st)
        for step in range(c.N):
            xs, vs, ld = dyn._lf(xs, vs, c.beta, step, bwd)
            ss = ss + ld
        assert torch.equal(xs, xt) and torch.equal(vs, vt), (bwd, float((xs - xt).abs().max()))
        fig, bar = float((ss - st).abs().max()), 1e-5 * max(1., float(st.abs().max()))
        print(f"[periodic scale] leapfrog steps N=10 bwd={bwd}: log-det regrouping {fig:.3e} / {bar:.3e}")
        assert fig <= bar
        # two halves: the kept VNet product is dropped at one launch boundary, at step 5
        xh, vh, sh = dyn._lf(x, v0, c.beta, 0, bwd, step_end=5)
        xh, vh, sh2 = dyn._lf(xh, vh, c.beta, 5, bwd, step_end=c.N)
        assert torch.equal(xh, xt) and torch.equal(vh, vt)
        assert float((sh + sh2 - st).abs().max()) <= bar


@pytest.mark.parametrize("name", ["n10-8x8-mild-paired", "n10-8x8-mild-selected"])
def test_kept_first_layer_products_are_bit_neutral_at_benchmark_length(name):
    c = S.BY_NAME[name]
    B = S.chains(c)
    x32, v0f, v0b, coin, u = S.inputs(c)
    x = _dev(x32)
    outs = []
    for rec in (False, True):
        dyn = _dyn(c, B, seed=S.STEP_SEED, recompute=rec)[0]
        assert _fused(dyn) == 1
        res = dict(_whole_step(dyn, x, c.beta)[0])
        for fwd, v0 in ((True, v0f), (False, v0b)):
            for i, t in enumerate(dyn.transition_kernel(x, c.beta, forward=fwd, momentum=_dev(v0), return_logdet=True)):
                res[f"traj{fwd}{i}"] = t
        for i, t in enumerate(dyn.apply_transition(x, c.beta, momentum_f=_dev(v0f), momentum_b=_dev(v0b),
                                                   coin=_dev(coin), u=_dev(u))):
            res[f"apply{i}"] = t
        outs.append(res)
    _equal(outs[0], outs[1], f"recompute at N = 10, {name}")


# ---- b. chip-filling grids -----------------------------------------------------------------------------------------
def _tiles(n, per):
    """Indices of the rows (chains) of workgroups 0, CUS - 1 and the last of n items at `per` per workgroup."""
    cus = _cus()
    assert -(-n // per) == cus + 1
    return np.concatenate([np.arange(0, per), np.arange((cus - 1) * per, cus * per), np.arange(cus * per, n)])


def test_trajectory_rows_do_not_depend_on_the_grid():
    """l2hmc_gauge_trajectory at 16 CUS + 2 rows of mixed directions: bits of the tiles alone, and float64."""
    c = S.BY_NAME["big-selected"]                       # its lattice, weights, N, eps and beta
    R = S.TRAJ_ROWS_PER_CU * _cus() + S.TRAJ_ROWS_EXTRA
    rng = np.random.default_rng(401)
    x32 = S.start(c._replace(seed=402), R)
    v32 = rng.standard_normal((R, 128)).astype(np.float32)
    d32 = rng.integers(0, 2, R).astype(np.int32)
    ws, r64, r32 = _dyn(c, R)
    lay, _, _ = _dyn(c, R, whole_step=False)
    assert _fused(ws) == 1
    run = lambda d, rows: _trajectory(d, _dev(x32[rows]), _dev(v32[rows]),   # noqa: E731
                                      torch.as_tensor(d32[rows], device="cuda"), c.beta)
    every = np.arange(R)
    full = run(ws, every)
    tiles = _tiles(R, S.WG_ROWS)
    assert len(tiles) == 2 * S.WG_ROWS + 2 and 0 < d32[tiles[-2:]].sum() + d32[tiles[:16]].sum() < 18
    alone = run(ws, tiles)
    for k, a, b in zip(("x", "v", "sumlogdet", "p"), full, alone):
        same = torch.equal(a[torch.as_tensor(tiles, device="cuda")], b)
        print(f"[periodic scale] trajectory {R} rows, {k}: tiles 0, CUS - 1, last bit equal to their own launch: {same}")
        assert same, (k, float((a[torch.as_tensor(tiles, device="cuda")] - b).abs().max()))
    # every row against float64 (the reference is row-local: each direction's rows in one pass)
    layered = run(lay, every)
    names = ("x", "v", "sumlogdet", "p")
    for bwd in (False, True):
        sel = d32 == int(bwd)
        f64, f32 = S.traj(r64, x32[sel], v32[sel], c.beta, bwd), S.traj(r32, x32[sel], v32[sel], c.beta, bwd)
        got = {k: _np(t)[sel] for k, t in zip(names, full)}
        lay_o = {k: _np(t)[sel] for k, t in zip(names, layered)}
        assert np.abs(f64["sumlogdet"]).mean() > 1e-3 and 0.1 < f64["p"].mean() < 0.9
        yard = _yards(c, f32, lay_o, f64, ANG_T)
        w = _gate(f"trajectory {R} rows bwd={bwd}", got, f64, yard, angular=ANG_T)
        _note("b. trajectory entry, 16 CUS + 2 rows", w)
        m = S.margin(S.neighbour_swap(f64, int(sel.sum())), f64, yard, ANG_T)
        print(f"[periodic scale] trajectory bwd={bwd}: a neighbour's row in the last place misses the gate by {m:.3g}")
        assert m >= S.BITES


@pytest.mark.parametrize("name", [c.name for c in S.BIG_CASES])
def test_apply_transition_does_not_depend_on_the_grid(name):
    c = S.BY_NAME[name]
    B = S.chains(c, _cus())
    x, v0f, v0b, coin, u = S.inputs(c, _cus())
    ws, got, layered, f64, f32, clear = _apply_case(c, B, x, v0f, v0b, coin, u)
    yard = _yards(c, f32, layered, f64, ANG_A)
    w = _gate(f"apply_transition {name} B={B}", got, f64, yard, angular=ANG_A)
    _note(f"b. apply_transition, {name}", w)
    keys = ("x_prop", "v_prop", "p")
    m = S.margin(S.neighbour_swap(_cut(f64, keys), B), _cut(f64, keys), yard, ANG_A, keys=keys)
    print(f"[periodic scale] {name}: a neighbour's chain in the last workgroup misses the gate by {m:.3g}")
    assert m >= S.BITES
    # the chains of workgroups 0, CUS - 1 and the last (one chain), launched alone: the same bits
    tiles = _tiles(B, S.WG_ROWS // 2 if c.both else S.WG_ROWS)
    run = lambda rows: ws.apply_transition(_dev(x[rows]), c.beta, momentum_f=_dev(v0f[rows]),   # noqa: E731
                                           momentum_b=_dev(v0b[rows]), coin=_dev(coin[rows]), u=_dev(u[rows]))
    full, alone = run(np.arange(B)), run(tiles)
    assert 0 < (coin[tiles] > 0.5).sum() < len(tiles)
    for k, a, b in zip(S.APPLY_NAMES, full, alone):
        same = torch.equal(a[torch.as_tensor(tiles, device="cuda")], b)
        print(f"[periodic scale] {name} {k}: workgroups 0, CUS - 1, last bit equal to their own launch: {same}")
        assert same, k


# ---- c. step mode at the big batches -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in S.STEP_CASES if c.per_cu])
def test_step_observables_and_sums_at_a_chip_filling_batch(name):
    from l2hmc_amd.lattice import u1_observables
    from tests import helpers as H
    c = S.BY_NAME[name]
    B = S.chains(c, _cus())
    ws, x, got3, w = _step_against_float64(c, B)
    _note(f"c. whole step, {name}", w)
    got = got3[0]
    ws._draws = S.STEP_DRAWS
    with torch.no_grad():
        _, _, _, x_out = ws(x, c.beta)                 # the step's own x_out, unwrapped (same kernel, same draws)
    obs_in, obs_out = u1_observables(x, c.T, c.X), u1_observables(x_out, c.T, c.X)      # l2hmc_u1_action_force
    want = dict(action=obs_in["action"], avg_plaq=obs_in["avg_plaq"], top_charge=obs_in["top_charge"],
                dq=(obs_in["top_charge"] - obs_out["top_charge"]).abs())
    tol = dict(action=1e-5, avg_plaq=1e-5, top_charge=1e-4, dq=1e-3)      # tests/test_gpu_periodic_step.py
    for k, wk in want.items():
        err = H.relerr(_np(got[k]), _np(wk))
        print(f"[periodic scale] {name} {k}: error {err:.3e} / {tol[k]:.0e}")
        assert err < tol[k], (k, err)
    # ... and against float64 arithmetic on the step's input
    a64 = PR.NumpyPeriodic(c.T, c.X, c.N, c.eps, PR.masks_for(c.N, 128), {}, {}).action(_np(x))
    err = H.relerr(_np(got["action"]), a64)
    print(f"[periodic scale] {name} action against float64: error {err:.3e} / 1e-05")
    assert err < 1e-5
    f32eps = np.finfo(np.float32).eps
    for n, step in enumerate(got3):
        sums = _np(step["sums"])
        for i, k in enumerate(("px", "dq")):
            s64 = float(step[k].double().sum())
            fig, bar = abs(sums[i] - s64), 4 * f32eps * max(1., abs(s64))
            print(f"[periodic scale] {name} step {n} sum {k}: {sums[i]!r} against {s64!r}: {fig:.3e} / {bar:.3e}")
            assert fig <= bar, (n, k)
        assert sums[2] == B and sums[3] == 0, (n, sums)      # the chain count, and the ticket left at 0
    assert float(got3[0]["dq"].sum()) > 0 and not torch.equal(got3[0]["px"], got3[1]["px"])


# ---- d. the ladder at the big batches ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in S.STEP_CASES if c.per_cu])
def test_ladder_step_equals_the_uniform_step_column_by_column(name):
    c = S.BY_NAME[name]
    B = S.chains(c, _cus())
    x = _dev(S.start(c, B))
    rungs = (1.0, 2.5, 4.0)
    betas = torch.tensor([rungs[i % 3] for i in range(B)], dtype=torch.float32, device="cuda")
    mk = lambda: _dyn(c, B, seed=S.STEP_SEED)[0]        # noqa: E731
    ladder = _whole_step(mk(), x, betas)[0]
    for b in rungs:
        uni = _whole_step(mk(), x, b)[0]
        cols = betas == b
        for k in ("x_next", "px", "action", "avg_plaq", "top_charge", "dq"):
            same = torch.equal(ladder[k][cols], uni[k][cols])
            assert same, (name, b, k)
        assert not torch.equal(ladder["px"][~cols], uni["px"][~cols])     # the rung matters
        print(f"[periodic scale] {name} ladder rung {b}: {int(cols.sum())} columns bit equal to the uniform step")
    assert float(ladder["sums"][2]) == B and float(ladder["sums"][3]) == 0


# ---- e. one chain cannot reach its tile-mates ----------------------------------------------------------------------
BAD = 3                                                # the chain that holds the inf / NaN; 19 paired chains, N = 3


def _poisoned(kind):
    """(case, clean inputs, inputs with chain BAD poisoned, inputs with chain BAD replaced by a benign chain)."""
    c = S.BY_NAME["big-paired"]._replace(name="isolation", per_cu=0, extra=19, seed=331)
    x, v0f, v0b, coin, u = S.inputs(c)
    masks = PR.masks_for(c.N, 128)
    moved = int(np.flatnonzero(masks[0] == 0)[0])      # a link the first position sub-update of a forward row moves
    bad = [a.copy() for a in (x, v0f, v0b, coin, u)]
    if kind == "inf":
        bad[0][BAD, moved] = np.inf
    else:
        bad[1][BAD, 5] = np.nan
        bad[2][BAD, 5] = np.nan
    benign = [a.copy() for a in (x, v0f, v0b, coin, u)]
    for a in benign:
        a[BAD] = a[BAD + 1]
    return c, bad, benign


def _isolation_runs(kind):
    """The float32 reference's and both device paths' apply_transition on the poisoned and on the benign inputs."""
    c, bad, benign = _poisoned(kind)
    B = 19
    ws, _, r32 = _dyn(c, B)
    lay, _, _ = _dyn(c, B, whole_step=False)
    with np.errstate(all="ignore"):
        want_bad = dict(zip(S.APPLY_NAMES, r32.apply_transition(bad[0], c.beta, *bad[1:])))
        want_ok = dict(zip(S.APPLY_NAMES, r32.apply_transition(benign[0], c.beta, *benign[1:])))
    run = lambda d, a: dict(zip(S.APPLY_NAMES, (t.cpu().numpy() for t in d.apply_transition(   # noqa: E731
        _dev(a[0]), c.beta, momentum_f=_dev(a[1]), momentum_b=_dev(a[2]), coin=_dev(a[3]), u=_dev(a[4])))))
    got = {what: (run(dyn, bad), run(dyn, benign)) for what, dyn in (("whole step kernel", ws), ("layered path", lay))}
    return want_bad, want_ok, got


@pytest.mark.parametrize("kind", ["inf", "nan"])
def test_a_poisoned_chain_does_not_reach_its_tile_mates(kind):
    """Ordinary arithmetic on NaN data: nothing here addresses anything a clean call does not.  The float32 reference
    defines the outcome: p = 0 for the chain, its proposal and its new state not finite, every other chain unchanged
    bit for bit; so it is on the device, against the same call with the chain replaced by a benign one."""
    want_bad, want_ok, got = _isolation_runs(kind)
    others = np.arange(19) != BAD
    assert want_bad["p"][BAD] == 0 and np.isnan(want_bad["x_prop"][BAD]).all()
    assert not np.isfinite(want_bad["x_out"][BAD]).all()
    for k in S.APPLY_NAMES:
        assert np.array_equal(want_bad[k][others], want_ok[k][others]) and np.isfinite(want_ok[k]).all(), k
    for what, (got_bad, got_ok) in got.items():
        assert got_bad["p"][BAD] == 0, (what, got_bad["p"][BAD])
        assert not np.isfinite(got_bad["x_prop"][BAD]).all() and not np.isfinite(got_bad["x_out"][BAD]).all(), what
        for k in S.APPLY_NAMES:
            assert np.isfinite(got_ok[k]).all(), (what, k)
            same = np.array_equal(got_bad[k][others], got_ok[k][others])
            print(f"[periodic scale] {kind} in chain {BAD}, {what}, {k}: the other 18 chains keep their bits: {same}")
            assert same, (what, k)


@pytest.mark.parametrize("kind", ["inf", "nan"])
def test_a_poisoned_chain_shows_the_references_nan_pattern(kind):
    """The poisoned chain's own x_prop and x_out, element by element: NaN where the float32 reference has NaN, inf where
    it has inf (all 128 links NaN: one NaN in the force or in v makes every S, T and Q of the row NaN).

    This is what made the relu of the torus-exact whole-step kernel and of the layered dense kernels `relu_nan`
    (csrc/common.h): with fmaxf(h, 0), which returns 0 for a NaN, S, T and Q stayed finite and only 47 (inf) and 23
    (NaN) of the 128 links came back NaN, on both paths."""
    want_bad, _, got = _isolation_runs(kind)
    for what, (got_bad, _) in got.items():
        for k in ("x_prop", "x_out"):
            n_dev, n_ref = int(np.isnan(got_bad[k][BAD]).sum()), int(np.isnan(want_bad[k][BAD]).sum())
            print(f"[periodic scale] {kind} in chain {BAD}, {what}, {k}: NaN in {n_dev} links, the reference in {n_ref}")
    for what, (got_bad, _) in got.items():
        for k in ("x_prop", "x_out"):
            assert np.array_equal(np.isnan(got_bad[k][BAD]), np.isnan(want_bad[k][BAD])), (what, k)
            assert np.array_equal(np.isinf(got_bad[k][BAD]), np.isinf(want_bad[k][BAD])), (what, k)


def test_report():
    """The worst error / yardstick of every group run in this session (for profiles/periodic_scale.txt)."""
    for group, w in sorted(WORST.items()):
        print(f"[periodic scale] worst {group}: {w:.2f}")
        assert w <= S.GATE
