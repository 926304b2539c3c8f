"""Host side of tests/test_gpu_periodic_scale.py: the case table of tests/periodic_scale_cases.py meets its conditions on
the float64 / float32 references of tests/periodic_ref.py alone, and a float64 reference that is wrong in one place --
the mask row of step s taken at s % 3, the backward time index taken at `step`, one chain of the last workgroup replaced
by its neighbour -- misses the gate of the GPU test by more than ten times.  No GPU; sizes at CUS = 256.

For every case that gates p or x_out: at least 90 % of the chains have |p - u| > 1e-4 in float64, the accepted
fraction lies in (0.1, 0.9), mean |sumlogdet| > 1e-3.  Every yardstick of an N = 10 case is finite and at most 2.5e-5,
so with GATE = 4 no gate is looser than the 1e-4 of the existing trajectory tests; the GPU test takes the smaller of
its yardstick and 2.5e-5 at N = 10, so the margins below (computed against GATE * 2.5e-5) hold there whatever the
layered device path adds to the yardstick.

Measured (printed by each test): accepted fractions 0.32 - 0.42 at N = 10 (eps 0.04) and 0.33 - 0.35 at the big N = 3
batches (eps 0.15); N = 10 yardsticks 4.5e-7 ... 1.5e-5; the perturbed references miss the loosest possible gate by
816 - 2519 (mask row), 1807 - 4255 (backward time index) and their own gate by 3.9e5 and more (neighbouring chain).  The
file runs in 21 s."""
import numpy as np
import pytest

from tests import periodic_scale_cases as S

ANG_T, ANG_A = ("x",), ("x_prop", "x_out")
_CACHE = {}


def _computed(name):
    """Inputs and both references' outputs of a case, computed once."""
    if name not in _CACHE:
        c = S.BY_NAME[name]
        if c in S.STEP_CASES:
            x = S.start(c, S.chains(c))
            v0f, v0b, coin, u = (np.asarray(a, dtype=np.float32) for a in S.step_draws_host(c))
        else:
            x, v0f, v0b, coin, u = S.inputs(c)
        r64, r32 = S.refs(c)
        out = dict(case=c, x=x, v0f=v0f, v0b=v0b, coin=coin, u=u)
        for tag, r in (("64", r64), ("32", r32)):
            out["tf" + tag] = S.traj(r, x, v0f, c.beta, False)
            out["tb" + tag] = S.traj(r, x, v0b, c.beta, True)
            out["a" + tag] = S.mix(out["tf" + tag], out["tb" + tag], x, coin, u)
        _CACHE[name] = out
    return _CACHE[name]


def _apply_yard(d):
    clear = S.clear_chains(d["a64"]["p"], d["u"])
    cut = lambda a: {k: (v[clear] if k == "x_out" else v) for k, v in a.items() if k != "sumlogdet"}   # noqa: E731
    return S.yard(cut(d["a32"]), cut(d["a64"]), ANG_A)


ALL = S.N10_CASES + S.BIG_CASES + S.STEP_CASES


def test_sizes_are_one_round_of_the_chip_and_one_chain():
    for c in S.BIG_CASES + S.STEP_CASES[1:]:
        B, nwg = S.chains(c), S.workgroups(c)
        per = S.WG_ROWS // 2 if c.both else S.WG_ROWS
        assert nwg == S.HOST_CUS + 1 and B - (nwg - 1) * per == 1, c
    assert (S.chains(S.BY_NAME["big-paired"]), S.chains(S.BY_NAME["big-selected"])) == (2049, 4097)
    rows = S.TRAJ_ROWS_PER_CU * S.HOST_CUS + S.TRAJ_ROWS_EXTRA
    assert rows == 4098 and -(-rows // S.WG_ROWS) == S.HOST_CUS + 1 and rows % S.WG_ROWS == 2
    # N = 10 cases: 19 chains are three paired workgroups (the last partial), two selected-only
    assert [S.workgroups(c) for c in S.N10_CASES] == [3, 2, 3, 3]
    assert all(c.N == 10 for c in S.N10_CASES) and {(c.T, c.X) for c in S.N10_CASES} == {(8, 8), (4, 16)}
    # the inputs are deterministic: the same table gives the same bits
    a, b = S.inputs(S.N10_CASES[0]), S.inputs(S.N10_CASES[0])
    assert all(np.array_equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("name", [c.name for c in ALL if c.gates_p])
def test_input_conditions(name):
    d = _computed(name)
    cond = S.conditions(d["a64"], d["u"], d["a64"]["sumlogdet"])
    print(f"[periodic scale host] {name}: clear {cond[0]:.4f} accepted {cond[1]:.3f} mean |sumlogdet| {cond[2]:.3f} "
          f"mean p {d['a64']['p'].mean():.3f}")
    assert S.conditions_hold(cond), cond
    # ... and in each direction alone, for the transition_kernel cases
    for t in (d["tf64"], d["tb64"]):
        assert np.abs(t["sumlogdet"]).mean() > 1e-3 and 0.05 < t["p"].mean() < 0.95
    for k in ("x", "v", "p", "sumlogdet"):
        assert np.isfinite(d["tf64"][k]).all() and np.isfinite(d["tb64"][k]).all()


@pytest.mark.parametrize("name", [c.name for c in ALL if c.N == 10])
def test_n10_yardsticks_are_finite_and_no_gate_is_looser_than_the_trajectory_tests(name):
    d = _computed(name)
    yards = dict(fwd=S.yard(d["tf32"], d["tf64"], ANG_T), bwd=S.yard(d["tb32"], d["tb64"], ANG_T), apply=_apply_yard(d))
    for group, y in yards.items():
        print(f"[periodic scale host] {name} {group}: " + " ".join(f"{k} {v:.2e}" for k, v in y.items()))
        for k, v in y.items():
            assert np.isfinite(v) and v <= S.YARD_CAP, (name, group, k, v)
    assert S.GATE * S.YARD_CAP <= 1e-4


def test_stress_at_n10_has_no_p_to_gate():
    d = _computed("n10-8x8-stress-paired")
    assert not d["case"].gates_p
    for t in (d["tf64"], d["tb64"], d["tf32"], d["tb32"]):
        assert t["p"].max() <= 1e-6                                       # what the GPU test asserts of the device
        assert np.abs(t["sumlogdet"]).mean() > 1e-3
    # x, v and sumlogdet are the gated outputs: they are finite and move
    assert np.isfinite(d["tf64"]["x"]).all() and np.abs(d["tf64"]["x"] - d["x"]).mean() > 1e-2


# ---- perturbed references ----------------------------------------------------------------------------------------
CAP = {k: S.YARD_CAP for k in S.TRAJ_NAMES}


@pytest.mark.parametrize("fault", ["mask", "time"])
@pytest.mark.parametrize("name", [c.name for c in ALL if c.N == 10])
def test_a_wrong_step_index_misses_the_gate_tenfold(name, fault):
    """Against the loosest gate the GPU test can have at N = 10 (GATE * YARD_CAP), on the outputs gated in every case
    (x, v, sumlogdet; p too where the case gates it)."""
    d = _computed(name)
    c = d["case"]
    keys = S.TRAJ_NAMES if c.gates_p else ("x", "v", "sumlogdet")
    p64, _ = S.refs(c, S.Perturbed, fault=fault)
    for bwd, v0, want in ((False, d["v0f"], d["tf64"]), (True, d["v0b"], d["tb64"])):
        m = S.margin(S.traj(p64, d["x"], v0, c.beta, bwd), want, CAP, ANG_T, keys)
        print(f"[periodic scale host] {name} fault {fault} bwd={bwd}: misses the gate by {m:.1f}")
        if fault == "time" and not bwd:
            assert m == 0                               # forward rows take `step` anyway
        else:
            assert m >= S.BITES, (name, fault, bwd, m)
    # the N = 3 cases cannot see the mask fault: s % 3 == s
    if fault == "mask":
        c3 = S.BY_NAME["big-paired"]
        q64, r64 = S.refs(c3, S.Perturbed, fault=fault)[0], S.refs(c3)[0]
        x, v0f, v0b, _, _ = (a[:5] for a in S.inputs(c3._replace(per_cu=0, extra=5)))
        for bwd, v0 in ((False, v0f), (True, v0b)):
            for a, b in zip(q64.trajectory(x, v0, c3.beta, bwd), r64.trajectory(x, v0, c3.beta, bwd)):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("name", [c.name for c in S.BIG_CASES + S.STEP_CASES[1:]])
def test_a_neighbours_chain_in_the_last_workgroup_misses_the_gate_tenfold(name):
    d = _computed(name)
    c = d["case"]
    B = S.chains(c)
    for group, want, f32, ang in (("fwd", d["tf64"], d["tf32"], ANG_T), ("bwd", d["tb64"], d["tb32"], ANG_T)):
        m = S.margin(S.neighbour_swap(want, B), want, S.yard(f32, want, ang), ang)
        print(f"[periodic scale host] {name} {group}: a neighbour's chain misses the gate by {m:.3g}")
        assert m >= S.BITES, (name, group, m)
    a64 = {k: v for k, v in d["a64"].items() if k != "sumlogdet"}
    a32 = {k: v for k, v in d["a32"].items() if k != "sumlogdet"}
    m = S.margin(S.neighbour_swap(a64, B), a64, S.yard(a32, a64, ANG_A), ANG_A, keys=("x_prop", "v_prop", "p"))
    print(f"[periodic scale host] {name} apply: a neighbour's chain misses the gate by {m:.3g}")
    assert m >= S.BITES, (name, m)
