"""A chain that holds an inf or a NaN, in every reference-mode sampling kernel, against the oracle.

The cases, their inputs and the float32 oracle's outputs are tests/nonfinite_cases.py, proven on the CPU by
tests/test_nonfinite_host.py.  Every case runs its entry twice with every random draw fixed (injected, or the library's
own Philox streams at the same seed and draw counter): on the poisoned inputs and on the same inputs with the bad chain
replaced by a benign one.  Asserted for every output of the entry:

1. isolation: every other chain has the bits of the benign call and is finite there.  Chains share workgroups, waves
   and the butterflies of the chain sums (`chain_sum` of fused_step.h: 16 lanes of a wave per chain; `__shfl_xor` over
   the rows of a wave in hmc_step.hip), so a sum that reached one lane too far would fail here.
2. pattern: the bad chain's outputs are NaN exactly where the float32 oracle has NaN and inf where it has inf, its p is
   0, and its finite entries (plain HMC only: a network makes every link NaN) meet the bar of the entry's parity test
   against the float64 oracle.  x_next is np.mod(x_out, 2 pi) of the oracle.  The step sums are NaN exactly where a
   NumPy sum of the per-chain outputs is.
3. the form that ran: from `dyn._plan()`, l2hmc_gauge_plan_fused and l2hmc_gauge_step_plan on the device's CU count.

The toy kernels: l2hmc_small_trajectory and l2hmc_small_propose in every first-layer form with all three kinds of poison
(pattern cases), and l2hmc_small_run over 3 steps with a poisoned coordinate (isolation and a chain that stays rejected:
the run draws its own momenta, and behind a poisoned coordinate no relu decides the outcome).

What the file found.  The relu of the reference mode's one-launch kernels and the relu and max-pool of the ConvNet3D
front-ends were fmaxf, which returns 0 for a NaN where the oracle's np.maximum hands it on: a poisoned chain came back
NaN in 47 / 23 (8x8, N = 3: poisoned link / momentum), 7 / 1 (N = 1) and 23 / 7 (ConvNet3D, N = 2) of 128 links instead
of all 128, and in 1 of 4 and 1 of 8 toy coordinates, while the layered path (relu_nan since the torus-exact mode's
tests) returned 128: `fused = True` and `fused = False` disagreed.  They are `relu_nan` / `max_nan` of csrc/common.h
now; figures before and after in profiles/offdomain_inputs.txt.

What was read before the first run: NaN and inf are ordinary float data in every kernel under test.  The only
float-to-int conversion on data is `(int)n` of fast_sincos (csrc/common.h), behind `!(fabsf(x) < 8192)`, which sends NaN
and inf to libm's sincosf; project_angle and the wrap to [0, 2 pi) use floorf and compares only; masks, directions, chain
and row indices, loop bounds and every address come from integers, the plan and the Philox streams, never from x or v;
the accept test `p > u` with p = 0 rejects, and accept_from_delta maps NaN to 0 ahead of expf."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import nonfinite_cases as NF
from tests import replica_ref as R
from tests import toy_cases as tc

pytestmark = pytest.mark.gpu

X_NEXT_TOL = 5e-5                                      # tests/test_gpu_hmc_geometry.py
OBS_TOL = dict(action=1e-5, avg_plaq=1e-5, top_charge=1e-4, dq=1e-3)


def _count(line):
    """A line of profiles/offdomain_inputs.txt: the NaN count of the device next to the reference's."""
    print("[nonfinite] " + line)


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dynamics(c, B):
    xp, vp = NF.weights(c)
    hmc = c.arch == "hmc"
    dyn = H.gauge_hip(c.T, c.X, c.N, c.eps, xp, vp, NF.masks(c), B, hmc=hmc, both_directions=c.both,
                      arch="generic" if hmc else c.arch)
    dyn._seed = NF.SEED
    for k, v in c.flags:
        setattr(dyn, k, v)
    return dyn


def _assert_form(c, dyn, B):
    """3.: the kernel the case names is the one its plan selects."""
    from l2hmc_amd import _lib
    plan = dyn._plan()
    fused = _lib.lib().l2hmc_gauge_plan_fused(C.byref(plan))
    flags = dict(c.flags)
    if c.family in ("layered", "conv3d layered"):
        assert fused == 0, c.name
        assert bool(plan.flags & _lib.PLAN_ALL_COLUMNS) == bool(flags.get("all_columns")), c.name
        return
    assert fused == 1, c.name
    if c.arch == "hmc":
        assert plan.hmc == 1
        return
    if c.arch == "conv3D":
        assert plan.flags & _lib.PLAN_CONV3D
        return
    rows = B * (2 if c.both else 1)
    parts = NF.step_plan(rows, _cus())
    assert bool(plan.flags & _lib.PLAN_TILES16_ONLY) == (c.family in ("16-row", "split") or bool(flags.get("tiles16_only")))
    assert bool(plan.flags & _lib.PLAN_SINGLE_KICKS) == bool(flags.get("single_kicks"))
    assert bool(plan.flags & _lib.PLAN_FULL_L1) == bool(flags.get("full_l1"))
    assert bool(plan.flags & _lib.PLAN_ALL_COLUMNS) == bool(flags.get("all_columns"))
    assert bool(plan.flags & _lib.PLAN_SELECTED_ONLY) == (not c.both)
    if c.family == "sub-tile" or (c.family == "ladder" and not flags.get("tiles16_only")):
        assert len(parts) == 1 and parts[0][1] in (4, 8, 12), (c.name, parts)     # what the launcher asks without the flag
    if c.family == "32-row":
        assert all(w == 32 for _, w in parts) and sum(r for r, _ in parts) == rows, (c.name, parts)
    if c.family in ("16-row", "split"):
        # L2HMC_PLAN_TILES16_ONLY (asserted above) is what keeps launch_fused_trajectory and launch_fused_step off the
        # sub-tile and 32-row forms; l2hmc_gauge_step_plan answers for a plan without it, so it has nothing to say here
        assert plan.flags & _lib.PLAN_TILES16_ONLY
    if c.family == "split":
        # launch_fused_step splits a GenericNet step of both directions; the heads image in the plan is what its
        # active-column form reads (tests/test_gpu_step_active_heads.py asserts the same)
        assert plan.heads and not plan.flags & _lib.PLAN_SELECTED_ONLY and not plan.flags & _lib.PLAN_CONV3D


def _device_draws(dyn):
    """The draws of the step with draw counter NF.DRAWS, through the library's own generators."""
    from l2hmc_amd import ops

    def draws(B, D):
        d = NF.DRAWS // 2
        V = _np(ops.fill_normal((2 * B, D), dyn._seed, 2 * d, "cuda"))
        cu = _np(ops.fill_uniform((2 * B,), dyn._seed, 2 * d + 1, "cuda"))
        return V[:B], V[B:], cu[:B], cu[B:]
    return draws


def _run(c, dyn, inp):
    """The case's entry on `inp` -> dict of NumPy outputs."""
    from l2hmc_amd import GaugeSampler
    x = _dev(inp[0])
    if c.entry == "apply":
        out = dyn.apply_transition(x, c.beta, momentum_f=_dev(inp[1]), momentum_b=_dev(inp[2]), coin=_dev(inp[3]),
                                   u=_dev(inp[4]))
        torch.cuda.synchronize()
        return dict(zip(NF.APPLY_NAMES, map(_np, out)))
    ladder = NF.betas(c, x.shape[0])
    dyn._draws = NF.DRAWS
    smp = GaugeSampler(dyn)
    ring, slot = smp._sums_ring, smp._sums_next
    xn, px, obs, dq = smp.step(x, c.beta if ladder is None else _dev(ladder))
    out = dict(x_next=xn, p=px, action=obs["action"], avg_plaq=obs["avg_plaq"], top_charge=obs["top_charge"], dq=dq,
               sums=ring[slot].clone())
    if ladder is None:                                  # the same kernel and draws with apply_transition's own outputs
        dyn._draws = NF.DRAWS
        out["x_prop"], out["v_prop"], out["p_apply"], out["x_out"] = dyn.apply_transition(x, c.beta)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _circle(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % NF.TWO_PI
    return np.minimum(d, NF.TWO_PI - d)


def _finite_entries_meet_the_parity_bar(what, k, got, w64, w32):
    """The finite entries of a poisoned chain's output against float64, under the rule of the entry's parity test."""
    fin = np.isfinite(w32)
    if not fin.any():
        return
    g, a, b = np.asarray(got)[fin], np.asarray(w64)[fin], np.asarray(w32)[fin]
    if k == "x_next":
        fig = float(_circle(g, a).max())
        print(f"[nonfinite] {what} {k}: {int(fin.sum())} finite entries, circle distance {fig:.3e} / {X_NEXT_TOL:.0e}")
        assert fig < X_NEXT_TOL, (what, k, fig)
    elif k in ("p", "p_apply"):
        assert np.abs(g - a).max() < tc.p_bar(a, b), (what, k)
    elif k in OBS_TOL:
        assert H.relerr(g, a) < OBS_TOL[k], (what, k)
    else:
        fails, fig = tc.fp32_equivalent(g, a, b)
        print(f"[nonfinite] {what} {k}: {int(fin.sum())} finite entries, max {fig['max']:.2e} (fp32 oracle {fig['fp32_max']:.2e})")
        assert not fails, (what, k, fails)


def _check(c, kind, got_bad, got_ok, bad_inp, B):
    bad_rows = list(NF.bad_chains(c, _cus()))
    others = np.ones(B, bool)
    others[bad_rows] = False
    # 1. isolation
    for k in got_bad:
        if k == "sums":
            continue
        assert np.isfinite(got_ok[k]).all(), (c.name, kind, k)
        same = np.array_equal(got_bad[k][others], got_ok[k][others])
        assert same, (c.name, kind, k, "another chain's bits moved")
    # 2. the oracle's pattern
    w32 = NF.reference(c, bad_inp, bad_rows)
    w64 = NF.reference(c, bad_inp, bad_rows, np.float64)
    w32["p_apply"], w64["p_apply"] = w32["p"], w64["p"]
    for j, b in enumerate(bad_rows):
        for k in got_bad:
            if k == "sums":
                continue
            g, w = got_bad[k][b], w32[k][j]
            n_dev, n_ref = int(np.isnan(g).sum()), int(np.isnan(w).sum())
            _count(f"{c.name:26s} {kind:5s} chain {b:5d} {k:10s} NaN: device {n_dev:4d} reference {n_ref:4d}"
                          f" of {np.size(w)}")
    wrong = []
    for j, b in enumerate(bad_rows):
        assert got_bad["p"][b] == 0, (c.name, kind, got_bad["p"][b])
        for k in got_bad:
            if k == "sums":
                continue
            g, w = got_bad[k][b], w32[k][j]
            if not NF.same_pattern(g, w):
                wrong.append(f"{k} of chain {b}: NaN in {int(np.isnan(g).sum())}, the reference in "
                             f"{int(np.isnan(w).sum())} of {np.size(w)}")
                continue
            _finite_entries_meet_the_parity_bar(f"{c.name} {kind} chain {b}", k, g, w64[k][j], w)
    if "sums" in got_bad:
        sums, eps32 = got_bad["sums"], np.finfo(np.float32).eps
        for i, k in enumerate(("p", "dq")):
            s64 = float(np.sum(got_bad[k].astype(np.float64)))
            assert np.isnan(sums[i]) == np.isnan(s64), (c.name, kind, k, sums[i], s64)
            if not np.isnan(s64):
                assert abs(sums[i] - s64) <= 4 * eps32 * max(1., abs(s64)), (c.name, kind, k)
        assert np.isnan(sums[1]) and not np.isnan(sums[0])          # |dQ| of the bad chain is NaN, its p is 0
        assert sums[2] == B and sums[3] == 0, (c.name, kind, sums)
        ok = got_ok["sums"]
        assert np.isfinite(ok).all() and ok[2] == B and ok[3] == 0
    return wrong


@pytest.mark.parametrize("name", [c.name for c in NF.LATTICE_CASES])
def test_a_poisoned_chain_stays_alone_and_shows_the_oracles_pattern(name):
    c = NF.BY_NAME[name]
    B = NF.chains(c, _cus())
    dyn = _dynamics(c, B)
    _assert_form(c, dyn, B)
    clean = NF.clean_inputs(c, _cus(), draws=_device_draws(dyn))
    wrong = []
    for kind in NF.kinds(c):
        bad, benign = NF.poison(c, kind, clean, _cus())
        wrong += [f"{kind}: {w}" for w in _check(c, kind, _run(c, dyn, bad), _run(c, dyn, benign), bad, B)]
    assert not wrong, (c.name, "not the oracle's pattern", wrong)       # (every kind is run before the case fails)


# ---- plain-HMC runs: the chain stays poisoned, the others stay bit equal, in every step ----------------------------------
HIST = ("px", "actions", "plaqs", "charges", "charge_diff")


def _group(T, X):
    """The replica group of a lattice: the first of 3, 2, 4 that the in-launch exchange serves (tests/hmc_geometry_cases.py)."""
    from tests import hmc_geometry_cases as G
    return G.exchange_group(T, X, True)


def _run_case(T, X):
    """Three groups of G rungs; the bad chain is rung G // 2 of the middle group."""
    g = _group(T, X)
    return NF.case(f"hmc-run-{T}x{X}", "plain HMC", "step", arch="hmc", T=T, X=X, B=3 * g, bad=(g + g // 2,), eps=0.1,
                 pattern=False)


def _sampler(c, in_launch=False):
    from l2hmc_amd import GaugeSampler
    dyn = _dynamics(c, c.B)
    dyn._draws = NF.DRAWS
    smp = GaugeSampler(dyn)
    smp.in_launch = in_launch
    return smp


def _run_reference(c, x0, beta, draw_indices, seed, dtype=np.float32):
    """The oracle's run of the bad chain alone: per step the dict of NF.reference, from the library's own draws."""
    from l2hmc_amd import ops
    B, D, bad = c.B, NF.dim(c), c.bad[0]
    x = np.asarray(x0[bad:bad + 1], dtype=dtype)
    out = []
    for d in draw_indices:
        V = _np(ops.fill_normal((2 * B, D), seed, 2 * d, "cuda"))
        cu = _np(ops.fill_uniform((2 * B,), seed, 2 * d + 1, "cuda"))
        rows = [a[bad:bad + 1] for a in (V[:B], V[B:], cu[:B], cu[B:])]
        ref = NF.reference(c._replace(beta=float(beta)), [x, *rows], [0], dtype)
        out.append(ref)
        x = ref["x_next"]
    return out


@pytest.mark.parametrize("entry", ["run", "run_ladder", "run_exchange", "run_exchange_in_launch"])
@pytest.mark.parametrize("T,X", NF.HMC_RUN_LATTICES)
def test_a_poisoned_chain_in_a_plain_hmc_run(T, X, entry):
    """l2hmc_gauge_hmc_run, _run_ladder and _run_exchange (rounds between the launches and inside them), 3 steps: in every
    step the other chains keep the bits of the benign run, the bad chain has the oracle's pattern (the stencil's reach
    grows from step to step) with p = 0, and a swap with the poisoned replica is refused: its action is NaN, and
    tests/replica_ref.py::swap_round gives p = 0 for it whatever the uniform."""
    from tests import philox_ref
    from l2hmc_amd import _lib
    c = _run_case(T, X)
    B, grp, bad_chain = c.B, _group(T, X), c.bad[0]
    ladder = np.tile(np.linspace(1.0, 3.0, grp), 3)[None, :]
    clean = NF.clean_inputs(c, draws=lambda B_, D: (np.zeros((B_, D)),) * 2 + (np.zeros(B_),) * 2)
    n = NF.HMC_RUN_STEPS
    exchange = entry.startswith("run_exchange")
    in_launch = entry == "run_exchange_in_launch"
    if in_launch:
        assert _sampler(c, True).exchange_in_launch(grp) is True
    beta_bad = 2.0 if entry == "run" else float(ladder[0, bad_chain])

    def run(x):
        smp = _sampler(c, in_launch)
        assert _lib.lib().l2hmc_gauge_plan_fused(C.byref(smp.dynamics._plan())) == 1
        if entry == "run":
            return smp.run(n, 2.0, _dev(x), keep_samples=True)
        if entry == "run_ladder":
            return smp.run_hmc(n, ladder, _dev(x), keep_samples=True)
        return smp.run_hmc_exchange(n, ladder, _dev(x), keep_samples=True, replicas=grp, swap_every=1)

    d0 = _lib.step_draw_index(NF.DRAWS)[0]
    draw_indices = philox_ref.lattice_run_draws(d0, n, swap_every=1 if exchange else None)[0]
    others = np.arange(B) != bad_chain
    if exchange:                                        # the bad chain's group decides differently: the other groups
        others = np.arange(B) // grp != bad_chain // grp
    names = dict(px="p", actions="action", plaqs="avg_plaq", charges="top_charge", charge_diff="dq", samples="x_next")
    for kind in NF.KINDS_STEP:
        bad, benign = NF.poison(c, kind, clean)
        got, ok = run(bad[0]), run(benign[0])
        for k in HIST + ("samples",):
            assert np.isfinite(ok[k]).all(), (kind, k)
            assert np.array_equal(got[k][:, others], ok[k][:, others]), (entry, kind, k)
        assert np.array_equal(_np(got["samples_out"])[others], _np(ok["samples_out"])[others])
        w32 = _run_reference(c, bad[0], beta_bad, draw_indices, NF.SEED)
        w64 = _run_reference(c, bad[0], beta_bad, draw_indices, NF.SEED, np.float64)
        reach = []
        for s in range(n):
            for k, rk in names.items():
                g, w = got[k][s, bad_chain], w32[s][rk][0]
                assert NF.same_pattern(g, w), (entry, kind, s, k, int(np.isnan(g).sum()), int(np.isnan(w).sum()))
                _finite_entries_meet_the_parity_bar(f"{entry} {T}x{X} {kind} step {s}", rk, g, w64[s][rk][0], w)
            assert got["px"][s, bad_chain] == 0
            reach.append(int(np.isnan(got["samples"][s, bad_chain]).sum()))
        _count(f"{entry:22s} {T}x{X} {kind:5s} NaN links of the bad chain after steps 1..{n}: {reach} of {NF.dim(c)}")
        assert reach == sorted(reach) and reach[0] > 0
        if exchange:
            g0 = bad_chain // grp * grp
            pairs = [a for a in (bad_chain - 1, bad_chain) if g0 <= a and a + 1 < g0 + grp]    # lower chains of its pairs
            proposed = 0
            for r in range(got["swap_p"].shape[0]):
                # the reference round on the state the step left: p = 0 for a pair that holds the poisoned replica
                _, ref_p, ref_sw, _ = R.swap_round(torch.as_tensor(got["samples"][r]), ladder[0], grp, r % 2,
                                                   np.zeros(B), T, X)
                for a in pairs:
                    assert np.isnan(got["swap_p"][r, a]) == bool(torch.isnan(ref_p[a])), (entry, kind, r, a)
                    if not np.isnan(got["swap_p"][r, a]):               # the pair was proposed in this round
                        proposed += 1
                        assert float(ref_p[a]) == 0 and not bool(ref_sw[a])
                        assert got["swap_p"][r, a] == 0 and not got["swapped"][r, a], (entry, kind, r, a)
                assert got["replica"][r, bad_chain] == bad_chain
            assert proposed > 0
            assert np.array_equal(got["swap_p"][:, others], ok["swap_p"][:, others], equal_nan=True)
            assert np.array_equal(got["swapped"][:, others], ok["swapped"][:, others])


# ---- toy targets ----------------------------------------------------------------------------------------------------
def _toy_dynamics(c):
    import l2hmc_amd as la
    mu, cov = NF.toy_arrays(c)
    xp, vp = NF.toy_nets(c)
    dyn = la.Dynamics(c.dim, la.Gaussian(mu, cov).get_energy_function(), trajectory_length=c.N, eps=NF.TOY_EPS,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=c.H),
                      use_temperature=True)
    dyn.set_masks(NF.toy_masks(c))
    dyn.XNet.load_state(xp)
    dyn.VNet.load_state(vp)
    assert not dyn.layered
    return dyn


def _toy_run(la, dyn, i):
    got = {}
    got["Xf"], got["Vf"], got["pf"] = dyn.forward(i["x"], init_v=i["v0f"])
    got["Xb"], got["Vb"], got["pb"] = dyn.backward(i["x"], init_v=i["v0b"])
    got["Lx"], got["Lv"], got["px"], (got["x_out"],) = la.propose(
        i["x"], dyn, init_v=i["v0f"], do_mh_step=True, init_v_backward=i["v0b"], dir_bits=i["bits"], u=i["u"])
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in got.items()}


@pytest.mark.parametrize("B", NF.TOY_BATCHES)
@pytest.mark.parametrize("c", NF.TOY_CASES, ids=NF.toy_id)
def test_a_poisoned_chain_in_the_toy_kernels(c, B):
    """l2hmc_small_trajectory and the one-launch propose in every first-layer form (small_mlp.hip; the shared net of
    small_mlp.h): isolation, and the oracle's pattern -- all coordinates of the proposal NaN; with fmaxf a poisoned
    momentum left dim - 1 of them finite.  A rejected chain keeps its state's bits (sampler.py:57-59 selects)."""
    import l2hmc_amd as la
    dyn = _toy_dynamics(c)
    clean = NF.toy_inputs(c, B)
    b = NF.toy_bad(B)
    others = np.arange(B) != b
    wrong = []
    for form in tc.forms(c.H):
        dyn.first_layer_form = form
        for kind in NF.KINDS_APPLY:
            bad, benign = NF.toy_poison(c, kind, clean)
            got, ok = _toy_run(la, dyn, bad), _toy_run(la, dyn, benign)
            w32 = NF.toy_reference(c, bad)
            for k in NF.TOY_NAMES:
                assert np.isfinite(ok[k]).all(), (form, kind, k)
                assert np.array_equal(got[k][others], ok[k][others]), (form, kind, k)
                _count(f"toy {NF.toy_id(c)} B={B:2d} form {form} {kind:5s} {k:6s} NaN: device "
                              f"{int(np.isnan(got[k][b]).sum())} reference {int(np.isnan(w32[k][b]).sum())} of {np.size(w32[k][b])}")
            wrong += [f"form {form} {kind} {k}: NaN in {int(np.isnan(got[k][b]).sum())}, the reference in "
                      f"{int(np.isnan(w32[k][b]).sum())} of {np.size(w32[k][b])}"
                      for k in NF.TOY_NAMES if not NF.same_pattern(got[k][b], w32[k][b])]
            assert got["px"][b] == 0 and got["pf"][b] == 0 and got["pb"][b] == 0
            assert np.array_equal(got["x_out"][b], bad["x"][b].astype(np.float32), equal_nan=True)
    assert not wrong, (NF.toy_id(c), B, "not the oracle's pattern", wrong)


@pytest.mark.parametrize("B", NF.TOY_BATCHES)
@pytest.mark.parametrize("c", NF.TOY_CASES, ids=NF.toy_id)
def test_a_poisoned_chain_in_the_toy_run(c, B):
    """l2hmc_small_run (`DynamicsSampler.run`: the chains stay in registers over the steps of ONE launch), 3 steps at the
    same draw counter for the poisoned and the benign call.  In every step the other chains' px and samples keep their
    bits; the bad chain has px = 0 and keeps its input's bits, as a rejected chain does, which is also what the float32
    oracle stepped on the library's own draws returns.  The run draws its momenta itself, so only a coordinate can be
    poisoned, and then no relu decides the pattern (tests/nonfinite_cases.py): an isolation case."""
    import l2hmc_amd as la
    from l2hmc_amd import ops
    dyn = _toy_dynamics(c)
    dyn._seed = NF.SEED
    clean = NF.toy_inputs(c, B)
    b = NF.toy_bad(B)
    others = np.arange(B) != b
    n = NF.TOY_RUN_STEPS

    def draws(s):
        d = NF.TOY_RUN_DRAWS + 4 * s
        return (_np(ops.fill_uniform((B,), NF.SEED, d, "cuda")), _np(ops.fill_normal((B, c.dim), NF.SEED, d + 1, "cuda")),
                _np(ops.fill_normal((B, c.dim), NF.SEED, d + 2, "cuda")), _np(ops.fill_uniform((B,), NF.SEED, d + 3, "cuda")))

    def run(x):
        smp = la.DynamicsSampler(dyn)
        assert smp._one_launch() and smp.steps_per_launch >= n
        dyn._draws = NF.TOY_RUN_DRAWS
        out = smp.run(n, _dev(x), keep_samples=True)
        assert dyn._draws == NF.TOY_RUN_DRAWS + 4 * n
        return out

    for form in tc.forms(c.H):
        dyn.first_layer_form = form
        for kind in NF.KINDS_STEP:
            bad, benign = NF.toy_poison(c, kind, clean)
            got, ok = run(bad["x"]), run(benign["x"])
            want_px, want_x = NF.toy_run_reference(c, bad["x"], draws)
            x_in = bad["x"][b].astype(np.float32)
            assert got["px"].shape == (n, B) and got["samples"].shape == (n, B, c.dim)
            for k in ("px", "samples"):
                assert np.isfinite(ok[k]).all(), (form, kind, k)
                assert np.array_equal(got[k][:, others], ok[k][:, others]), (form, kind, k, "another chain's bits moved")
            assert np.array_equal(_np(got["samples_out"])[others], _np(ok["samples_out"])[others])
            for s in range(n):
                assert got["px"][s, b] == 0 and want_px[s, b] == 0, (form, kind, s)
                assert NF.same_pattern(got["samples"][s, b], want_x[s, b]), (form, kind, s)
                assert np.array_equal(got["samples"][s, b], x_in, equal_nan=True), (form, kind, s)
            assert np.array_equal(_np(got["samples_out"])[b], x_in, equal_nan=True)
            # the restated draws are the run's own: px of the benign run's first step (no accept decision behind it yet)
            # against the oracle on them, under the accept-probability rule of tests/test_gpu_parity.py
            p64 = NF.toy_run_reference(c, benign["x"], draws, steps=1, dtype=np.float64)[0][0]
            p32 = NF.toy_run_reference(c, benign["x"], draws, steps=1)[0][0]
            assert np.abs(ok["px"][0] - p64).max() < tc.p_bar(p64, p32), (form, kind)
            _count(f"toy run {NF.toy_id(c)} B={B:2d} form {form} {kind:5s}: px of the bad chain {got['px'][:, b].tolist()}, its "
                   f"state keeps the input's bits in all {n} steps; {int(others.sum())} other chains bit equal")
