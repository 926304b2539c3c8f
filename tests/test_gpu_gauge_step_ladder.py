"""The L2HMC lattice step with a beta per chain (l2hmc_gauge_mcmc_step_ladder; `GaugeSampler.step` / `run` with a chain
axis on beta) on the GPU.  The yardstick is that of tests/test_gpu_hmc_run_ladder.py: chains never interact and the
kernels run the uniform step's own fp32 operations on the chain's value, so a column of a ladder EQUALS the uniform step
of the whole batch at that column's beta, bit for bit -- in every form of the whole-step kernel (4, 8, 12, 16 and 32
rows per workgroup, the split and the selected-only layout, ConvNet3D), in every part of a batch that is cut into
several launches, next to dead rows, and on the layer-by-layer path."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

HIST = ("px", "actions", "plaqs", "charges", "charge_diff")
RUNGS = (1.0, 2.5, 4.0)
TWO_PI = 2 * np.pi


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    return l2hmc_amd


def _masks(N, D):
    from oracle.gauge_dynamics import make_masks
    return make_masks(N, D, np.random.RandomState(42))


_WEIGHTS = {}


def _dyn(T, X, N, eps, B, both=True, arch="generic", regime="mild"):
    key = (T, X, arch, regime)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = (H.gauge_weights if arch == "generic" else H.conv_weights)(T, X, regime=regime)
    xp, vp = _WEIGHTS[key]
    return H.gauge_hip(T, X, N, eps, xp, vp, _masks(N, 2 * T * X), B, both_directions=both, arch=arch)


def _x0(B, D, seed=21):
    return torch.as_tensor(np.random.default_rng(seed).uniform(0, TWO_PI, (B, D)), dtype=torch.float32, device="cuda")


def _ladder(B):
    """[1, B]: chain c at RUNGS[c % 3]."""
    return np.asarray(RUNGS)[np.arange(B) % len(RUNGS)][None, :]


def _assert_columns_are_uniform_runs(la, dyn, B, n=2, beta=None, uniform=None):
    """`run` with the ladder `beta` ([1, B] or [n, B]; default `_ladder`) against `run` of the WHOLE batch at each
    rung's own beta (`uniform(g)`: a float or a [n] schedule) from the same start, seed and draw counter."""
    D = dyn.x_dim
    x0 = _x0(B, D)
    beta = _ladder(B) if beta is None else beta
    uniform = (lambda g: RUNGS[g]) if uniform is None else uniform
    dyn._draws = 40
    out = la.GaugeSampler(dyn).run(n, beta, x0, keep_samples=True)
    draws = dyn._draws
    assert out["px"].shape == (n, B) and out["samples"].shape == (n, B, D)
    assert np.isfinite(out["px"]).all() and (out["px"] >= 0).all() and (out["px"] <= 1).all()
    for g in range(len(RUNGS)):
        dyn._draws = 40
        ref = la.GaugeSampler(dyn).run(n, uniform(g), x0, keep_samples=True)
        assert dyn._draws == draws
        for k in HIST + ("samples",):
            assert ref[k].dtype == out[k].dtype == np.float32
            assert np.array_equal(out[k][:, g::3], ref[k][:, g::3]), (k, g, B)
        assert torch.equal(out["samples_out"][g::3], ref["samples_out"][g::3]), (g, B)
    from l2hmc_amd.lattice import u1_plaq_exact
    assert out["plaq_exact"].shape == (B,)
    assert np.array_equal(out["plaq_exact"], u1_plaq_exact(np.asarray(beta, dtype=np.float64)[-1]))
    return out


# ------------------------------------------------------------------------------------------------ the launch forms
def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _parts(rows, cus):
    from l2hmc_amd import _lib
    rows_out, rpw_out = (C.c_int64 * 3)(), (C.c_int * 3)()
    n = _lib.lib().l2hmc_gauge_step_plan(rows, cus, rows_out, rpw_out)
    assert n >= 1
    return [(int(rows_out[i]), int(rpw_out[i])) for i in range(n)]


# the batch (in chain-rows: chains x directions) of each kind on a part with `cus` CUs, and the forms it must take.
# Every row count is odd in chains or off the tile where it can be, so that the last workgroup has dead rows.
KINDS = {
    "sub4": (lambda cus: 6, [4]),                                  # 3 chains x 2 / 6 chains: one 4-row launch, dead rows
    "sub8": (lambda cus: 4 * cus + 6, [8]),
    "sub12": (lambda cus: 8 * cus + 10, [12]),
    "one16": (lambda cus: 12 * cus + 6, [16]),
    "one32": (lambda cus: 24 * cus + 6, [32]),
    "two": (lambda cus: 16 * cus + 6, [16, 4]),                    # a 16-row round, then a sub-tile launch from c0 > 0
    "three": (lambda cus: 48 * cus + 112 - 2, [32, 16, 4]),        # 32-row rounds, a 16-row round, a sub-tile launch
}


def _batch(kind, both):
    """(B, parts) of `kind` on this device: B chains give the chain-rows of KINDS (both directions: rows = 2 B)."""
    cus = _cus()
    rows, forms = KINDS[kind][0](cus), KINDS[kind][1]
    B = rows // 2 if both else rows
    parts = _parts(B * (2 if both else 1), cus)
    assert [w for _, w in parts] == forms, (kind, both, B, parts)
    return B, parts


def test_the_kinds_cover_every_form_and_cut():
    """Through the library's own launch plan: all five forms occur, one batch is cut in two and one in three, and a
    batch ends in a workgroup with dead rows."""
    seen, cuts, dead = set(), set(), 0
    for both in (True, False):
        for kind in KINDS:
            B, parts = _batch(kind, both)
            seen |= {w for _, w in parts}
            cuts.add(len(parts))
            rows, w = parts[-1]
            dead += rows % w != 0
    assert seen == {4, 8, 12, 16, 32} and cuts == {1, 2, 3} and dead > 0


@pytest.mark.parametrize("both", [True, False], ids=["both", "selected"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_columns_of_a_ladder_are_uniform_steps_in_every_form(la, kind, both):
    B, _ = _batch(kind, both)
    dyn = _dyn(8, 8, 2, 0.2, B, both=both)
    _assert_columns_are_uniform_runs(la, dyn, B)


@pytest.mark.parametrize("both", [True, False], ids=["both", "selected"])
def test_a_beta_per_step_and_chain(la, both):
    """[run_steps, B]: every step takes its own row of the array that went to the device once."""
    B, n = 70, 3
    dyn = _dyn(8, 8, 3, 0.15, B, both=both)
    sched = np.asarray([1.0, 0.5, 2.0])[:, None] * _ladder(B)                  # [n, B]
    _assert_columns_are_uniform_runs(la, dyn, B, n, beta=sched, uniform=lambda g: sched[:, g])


@pytest.mark.parametrize("both", [True, False], ids=["both", "selected"])
def test_convnet3d_whole_step_kernel(la, both):
    B = 37
    dyn = _dyn(8, 8, 2, 0.1, B, both=both, arch="conv3D")
    from l2hmc_amd import _lib
    assert _lib.lib().l2hmc_gauge_plan_fused(C.byref(dyn._plan())) == 1
    _assert_columns_are_uniform_runs(la, dyn, B)


@pytest.mark.parametrize("both", [True, False], ids=["both", "selected"])
def test_layer_by_layer_at_8x8(la, both):
    B = 37
    dyn = _dyn(8, 8, 2, 0.2, B, both=both)
    dyn.fused = False
    _assert_columns_are_uniform_runs(la, dyn, B)


@pytest.mark.parametrize("both", [True, False], ids=["both", "selected"])
def test_a_lattice_without_a_whole_step_kernel(la, both):
    B = 37
    dyn = _dyn(6, 6, 3, 0.2, B, both=both)
    from l2hmc_amd import _lib
    assert _lib.lib().l2hmc_gauge_plan_fused(C.byref(dyn._plan())) == 0
    _assert_columns_are_uniform_runs(la, dyn, B, n=3)


@pytest.mark.parametrize("both", [True, False], ids=["both", "selected"])
def test_convnet3d_at_a_shape_of_conv3d_cases(la, both):
    from tests.conv3d_cases import STQ_CASES
    T, X, F, B = STQ_CASES[0]                                                   # 4 x 16, F = X = 16, 9 rows
    assert (T, X, F, B) == (4, 16, 16, 9)
    dyn = _dyn(T, X, 2, 0.1, B, both=both, arch="conv3D")
    _assert_columns_are_uniform_runs(la, dyn, B)


# ------------------------------------------------------------------------------------------------ equal entries
def _last_sums(smp):
    return smp._sums_ring[(smp._sums_next - 1) % smp._sums_ring.shape[0]].clone()


@pytest.mark.parametrize("case", ["three-both", "one16-selected", "sub4-both", "6x6-both"])
def test_equal_entries_give_the_scalar_step(la, case):
    kind, mode = case.split("-")
    both = mode == "both"
    if kind == "6x6":
        B, dyn = 37, _dyn(6, 6, 2, 0.2, 37, both=both)
    else:
        B, _ = _batch(kind, both)
        dyn = _dyn(8, 8, 2, 0.2, B, both=both)
    x0 = _x0(B, dyn.x_dim)
    got = {}
    for name, beta in (("float", 2.5), ("array", np.full(B, 2.5)), ("row", np.full((1, B), 2.5)),
                       ("device", torch.full((B,), 2.5, device="cuda"))):
        dyn._draws = 40
        smp = la.GaugeSampler(dyn)
        xn, px, obs, dq = smp.step(x0, beta)
        got[name] = [xn, px, dq, *(obs[k] for k in sorted(obs)), _last_sums(smp)]
        assert dyn._draws == 42
    for name in ("array", "row", "device"):
        for i, (a, b) in enumerate(zip(got[name], got["float"])):
            assert torch.equal(a, b), (case, name, i)
    assert float(got["float"][-1][2]) == B and float(got["float"][-1][3]) == 0


# ------------------------------------------------------------------------------------------------ the C entry
def _c_step(dyn, betas, stride, x_in, x_next, B, draw=9, outs=True, sums=True):
    from l2hmc_amd import _lib
    plan, L = dyn._plan(), _lib.lib()
    nb = L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    o = [torch.full((B,), np.nan, device="cuda") for _ in range(5)] if outs else [None] * 5
    s = torch.zeros(4, device="cuda") if sums else None
    _lib.call("l2hmc_gauge_mcmc_step_ladder", C.byref(plan), betas, stride, x_in, x_next, B, 42, draw, *o, s, ws, nb)
    torch.cuda.synchronize()
    return o, s


@pytest.mark.parametrize("case", ["three-both", "two-selected", "sub4-selected", "6x6-both", "6x6-selected"])
def test_step_sums_of_a_true_ladder(la, case):
    """[2] = B, [0] and [1] the sums of the per-chain px and |dQ| the step returns -- to the worst-case rounding of any
    fp32 summation order, B 2^-24 sum |term| -- and the ticket word back at 0."""
    kind, mode = case.split("-")
    both = mode == "both"
    if kind == "6x6":
        B, dyn = 37, _dyn(6, 6, 2, 0.2, 37, both=both)
    else:
        B, _ = _batch(kind, both)
        dyn = _dyn(8, 8, 2, 0.2, B, both=both)
    x0 = _x0(B, dyn.x_dim)
    betas = torch.as_tensor(_ladder(B)[0], dtype=torch.float32, device="cuda")
    (px, act, plq, chg, dq), sums = _c_step(dyn, betas, 1, x0, torch.empty_like(x0), B)
    assert float(sums[2]) == B
    assert int(sums.view(torch.int32)[3]) == 0
    for i, term in ((0, px), (1, dq)):
        t = term.double().cpu().numpy()
        print(f"{case}: sums[{i}] = {float(sums[i])!r}, float64 sum {t.sum()!r}, bound {B * 2.0 ** -24 * np.abs(t).sum():.3e}")
        assert abs(float(sums[i]) - t.sum()) <= B * 2.0 ** -24 * np.abs(t).sum(), (case, i)
    assert torch.isfinite(px).all() and float(px.min()) >= 0 and float(px.max()) <= 1


@pytest.mark.parametrize("case", ["two-both", "sub8-selected", "6x6-both"])
def test_c_entry_strides_aliasing_and_null_outputs(la, case):
    kind, mode = case.split("-")
    both = mode == "both"
    if kind == "6x6":
        B, dyn = 37, _dyn(6, 6, 2, 0.2, 37, both=both)
    else:
        B, _ = _batch(kind, both)
        dyn = _dyn(8, 8, 2, 0.2, B, both=both)
    x0 = _x0(B, dyn.x_dim)
    # chain_stride 0 (one value) against 1 (B equal values)
    one, many = torch.full((1,), 1.75, device="cuda"), torch.full((B,), 1.75, device="cuda")
    xa, xb = torch.empty_like(x0), torch.empty_like(x0)
    oa, sa = _c_step(dyn, one, 0, x0, xa, B)
    ob, sb = _c_step(dyn, many, 1, x0, xb, B)
    assert torch.equal(xa, xb) and torch.equal(sa, sb) and all(torch.equal(a, b) for a, b in zip(oa, ob))
    # x_next aliasing x_in, and every optional output NULL (the 6x6 path needs px and charge_diff for step_sums)
    betas = torch.as_tensor(_ladder(B)[0], dtype=torch.float32, device="cuda")
    want = torch.empty_like(x0)
    ow, _ = _c_step(dyn, betas, 1, x0, want, B)
    xi = x0.clone()
    _c_step(dyn, betas, 1, xi, xi, B, outs=False, sums=False)
    assert torch.equal(xi, want)
    assert float(want.min()) >= 0.0 and float(want.max()) <= TWO_PI and not torch.equal(want, x0)
    assert all(torch.isfinite(o).all() for o in ow)


# ------------------------------------------------------------------------------------------------ sanity
@pytest.mark.parametrize("both", [True, False], ids=["both", "selected"])
def test_rungs_order_their_plaquettes(la, both):
    """From a hot start (plaquette 0) the rungs thermalise towards their own beta: after a few steps the mean
    plaquettes are ordered with beta, which a kernel that read one beta for all chains would not show.  "Ordered":
    neighbouring rungs differ by more than 3 standard errors of their difference (256 chains per rung), which noise
    on two equal means reaches once in about 700 cases."""
    B, n = 768, 80
    dyn = _dyn(8, 8, 3, 0.2, B, both=both, regime="init")
    dyn._draws = 40
    out = la.GaugeSampler(dyn).run(n, _ladder(B), _x0(B, 128))
    assert np.isfinite(out["px"]).all() and (out["px"] >= 0).all() and (out["px"] <= 1).all()
    plq = [float(out["plaqs"][-1, g::3].mean()) for g in range(3)]
    err = [float(out["plaqs"][-1, g::3].std() / np.sqrt(B // 3)) for g in range(3)]
    print(f"mean plaquette of the rungs {RUNGS} after {n} steps: {plq} +/- {err}; mean px {out['px'].mean():.3f}")
    for lo in (0, 1):
        assert plq[lo + 1] - plq[lo] > 3 * np.hypot(err[lo], err[lo + 1]), (plq, err)


# ------------------------------------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("kind,both", [("sub4", True), ("three", False)], ids=["sub4-both", "three-selected"])
def test_a_ladder_step_is_graph_capturable(la, kind, both):
    """No allocation and no synchronisation inside the entry: one ladder step -- one launch, or the three kernel
    launches of a cut batch -- is captured into a HIP graph and replayed twice, and every output equals the eager
    step's.  (The cut batch is taken selected-only: with both directions its 16-row part is the split form with its
    hand-off tickets; that is launch_fused_step's, shared with the uniform step, and
    tests/test_gpu_workspace_state.py replays it, at one beta and on a ladder.)"""
    from l2hmc_amd import _lib
    B, _ = _batch(kind, both)
    dyn = _dyn(8, 8, 2, 0.2, B, both=both)
    plan, L = dyn._plan(), _lib.lib()
    nb = L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    outs = [torch.empty(B, device="cuda") for _ in range(5)]
    sums = torch.zeros(4, device="cuda")
    betas = torch.as_tensor(_ladder(B)[0], dtype=torch.float32, device="cuda")
    x0 = _x0(B, 128)

    def step(x_in, x_next):
        _lib.check(L.l2hmc_gauge_mcmc_step_ladder(C.byref(plan), betas.data_ptr(), 1, x_in.data_ptr(), x_next.data_ptr(),
                                                  B, 42, 7, *(o.data_ptr() for o in outs), sums.data_ptr(),
                                                  ws.data_ptr(), nb, _lib.stream_ptr()))
    eager = torch.empty_like(x0)
    step(x0, eager)
    torch.cuda.synchronize()
    want = [eager.clone(), sums.clone(), *(o.clone() for o in outs)]
    xin, xg = x0.clone(), torch.empty_like(x0)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(xin, xg)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        xg.zero_()
        for o in outs:
            o.zero_()
        xin.copy_(x0)
        g.replay()
        torch.cuda.synchronize()
        got = [xg, sums, *outs]
        assert all(torch.equal(a, b) for a, b in zip(got, want))
