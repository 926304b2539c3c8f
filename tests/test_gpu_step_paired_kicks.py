"""The whole-step kernel's paired momentum half-kicks: on the 16-row GenericNet sampling form the second half-kick of
leapfrog step s and the first of step s + 1 run as ONE pass over two time slices (the even wave of an image section
takes step s's slice, the odd wave step s + 1's).  Every output must EQUAL the per-call flow
(L2HMC_PLAN_SINGLE_KICKS) bit for bit: whatever the number of leapfrog steps (no pair, one pair, both stream
parities), the chain count, the directions, the mask rows' eligibility for the active-column path, a non-finite
input, and however a trajectory is cut into launches."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

T = X = 8
D = 2 * T * X
EPS, BETA = 0.25, 2.0


def _random_masks(rng, n):
    masks = np.zeros((n, D), np.float32)
    for s in range(n):
        masks[s, rng.permutation(D)[:D // 2]] = 1.
    return masks


_WEIGHTS = {}


def _dyn(B, n, both=True, masks=None, seed=106):
    if seed not in _WEIGHTS:
        _WEIGHTS[seed] = H.gauge_weights(T, X, seed=seed, regime="mild")
    xp, vp = _WEIGHTS[seed]
    if masks is None:
        masks = _random_masks(np.random.default_rng(seed + n), n)
    dyn = H.gauge_hip(T, X, n, EPS, xp, vp, masks, B, both_directions=both)
    dyn.tiles16_only = True                       # every batch on the 16-row form
    return dyn


def _x(B, seed=3):
    rng = np.random.default_rng(seed)
    return torch.as_tensor(rng.uniform(0, 2 * np.pi, (B, D)), dtype=torch.float32, device="cuda")


def _v(B, seed=5):
    rng = np.random.default_rng(seed)
    return torch.as_tensor(rng.standard_normal((B, D)), dtype=torch.float32, device="cuda")


def _outputs(dyn, x, single, draw=40):
    """step (x_next, px, action, avg_plaq, top_charge, dq), apply_transition (4), transition_kernel forward and
    backward (x, v, p, log-det each)."""
    from l2hmc_amd import GaugeSampler
    dyn.single_kicks = single
    try:
        dyn._draws = draw
        smp = GaugeSampler(dyn)
        xn, px, obs, dq = smp.step(x, BETA)
        dyn._draws = draw
        tr = dyn.apply_transition(x, BETA)
        v = _v(x.shape[0])
        kf = dyn.transition_kernel(x, BETA, forward=True, momentum=v, return_logdet=True)
        kb = dyn.transition_kernel(x, BETA, forward=False, momentum=v, return_logdet=True)
        torch.cuda.synchronize()
        return [xn, px, obs["action"], obs["avg_plaq"], obs["top_charge"], dq, *tr, *kf, *kb]
    finally:
        dyn.single_kicks = False


def _assert_equal_single(dyn, x):
    got, want = _outputs(dyn, x, False), _outputs(dyn, x, True)
    assert len(got) == len(want) == 18
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"output {i}: max |diff| {float((a - b).abs().max())}"
    return got


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("B", [16, 130])
@pytest.mark.parametrize("n", [1, 2, 3, 10])
def test_paired_kicks_equal_single_kicks(n, B, both):
    """num_steps 1: no pair; 2: one pair; 3, 10: pairs at both stream parities.  16 chains are one workgroup pair, 130
    leave a partial last workgroup.  both = False: per-row directions, no split (all-columns heads, full first layer)."""
    dyn = _dyn(B, n, both)
    if both:
        assert dyn._plan().heads
    got = _assert_equal_single(dyn, _x(B))
    assert all(bool(torch.isfinite(a).all()) for a in got)


def test_mask_row_outside_the_active_column_path():
    """Row 1 has D / 2 + 1 ones and row 2 a fractional entry: their steps (and, going backward, steps N - 2 and N - 3)
    take the all-columns heads and the full first layer, which the paired call's staging for the next step must
    follow row by row."""
    B, n = 48, 4
    dyn = _dyn(B, n)
    m = dyn.mask.detach().cpu().numpy().copy()
    m[1, np.flatnonzero(m[1] == 0)[0]] = 1.
    m[2, 7] = 0.5
    dyn.set_masks(m)
    _assert_equal_single(dyn, _x(B, seed=5))


def test_non_finite_input_gives_the_same_rows():
    """Chain 3 starts with an inf in a column that the forward direction's first position sub-update moves (mask 0
    at step 0): 0 x inf = NaN is raised as the row's poison, from step 1 on inside the paired call."""
    B, n = 32, 3
    dyn = _dyn(B, n)
    x = _x(B, seed=13)
    col = int(np.flatnonzero(dyn.mask[0].detach().cpu().numpy() == 0)[0])
    x[3, col] = float("inf")
    got, want = _outputs(dyn, x, False), _outputs(dyn, x, True)
    assert not bool(torch.isfinite(want[6][3]).all())          # x_prop of chain 3
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(torch.isnan(a), torch.isnan(b)), f"output {i}: NaN pattern"
        ok = ~torch.isnan(b)
        assert torch.equal(a[ok], b[ok]), f"output {i}: entries that are not NaN"
    rest = [i for i in range(B) if i != 3]
    assert bool(torch.isfinite(got[0][rest]).all())


@pytest.mark.parametrize("backward", [False, True])
def test_partial_launches_equal_the_whole_trajectory(backward):
    """One-step launches (no pair anywhere) and a 4 + 6 split (pairs inside both launches, none across the cut)
    against the whole-trajectory launch (nine pairs).  x and v must be equal; the log-det is the same 160 per-wave,
    per-call terms summed in another order (per launch first), so it may differ by the rounding of two sums of at
    most 43 adds each: 2 x 43 x 2^-24 x (sum of |terms|), and every term is at most its sub-update's step size times
    e^{coeff_scale}: N D eps (max e^{cs} of VNet + max e^{cs} of XNet) over the trajectory."""
    B, n = 130, 10
    dyn = _dyn(B, n)
    x, v = _x(B, seed=7), _v(B, seed=8)
    xw, vw, _, ldw = dyn.transition_kernel(x, BETA, forward=not backward, momentum=v, return_logdet=True)
    es = sum(float(np.exp(np.max(net.state_dict()["coeff_scale"].detach().cpu().numpy())))
             for net in (dyn.momentum_fn, dyn.position_fn))
    tol = 2 * 43 * 2.0 ** -24 * n * D * EPS * es

    def run(cuts, single):
        dyn.single_kicks = single
        try:
            xc, vc = x, v
            ld = torch.zeros(B, dtype=torch.float32, device="cuda")
            for b, e in cuts:
                xc, vc, l = dyn._lf(xc, vc, BETA, b, backward, step_end=e)
                ld = ld + l
            torch.cuda.synchronize()
            return xc, vc, ld
        finally:
            dyn.single_kicks = False

    for cuts in ([(s, s + 1) for s in range(n)], [(0, 4), (4, 10)]):
        xc, vc, ld = run(cuts, False)
        assert torch.equal(xc, xw) and torch.equal(vc, vw), cuts
        err = float((ld - ldw).abs().max())
        print(f"cuts {cuts}: max |log-det - whole| {err:.3e} (bound {tol:.3e})")
        assert err <= tol
        xs_, vs_, lds = run(cuts, True)
        assert torch.equal(xc, xs_) and torch.equal(vc, vs_) and torch.equal(ld, lds), cuts
