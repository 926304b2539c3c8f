"""The whole-step kernel's split form: every workgroup integrates 16 chains of ONE direction (the pair's last arriver
mixes, accepts and measures), and a position sub-update forms S / T / Q only on the D / 2 columns its mask moves
(l2hmc_gauge_pack_heads).  Every output must EQUAL the all-columns form (L2HMC_PLAN_ALL_COLUMNS) bit for bit; masks
that are not exactly half zeros and half ones fall back to all columns on the device; the image follows the masks and
the weights."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

T = X = 8
N, EPS, BETA = 10, 0.25, 2.0


def _dyn(B, regime="mild", seed=106):
    xp, vp = H.gauge_weights(T, X, seed=seed, regime=regime)
    rng = np.random.default_rng(seed)
    masks = np.zeros((N, 2 * T * X), np.float32)
    for s in range(N):
        masks[s, rng.permutation(2 * T * X)[:T * X]] = 1.
    dyn = H.gauge_hip(T, X, N, EPS, xp, vp, masks, B)
    dyn.tiles16_only = True                       # every batch on the 16-row form
    return dyn


def _x(B, seed=3):
    rng = np.random.default_rng(seed)
    return torch.as_tensor(rng.uniform(0, 2 * np.pi, (B, 2 * T * X)), dtype=torch.float32, device="cuda")


def _outputs(dyn, x, all_columns, draw=40):
    from l2hmc_amd import GaugeSampler
    dyn.all_columns = all_columns
    try:
        dyn._draws = draw
        smp = GaugeSampler(dyn)
        xn, px, obs, dq = smp.step(x, BETA)
        dyn._draws = draw
        tr = dyn.apply_transition(x, BETA)       # x_prop, v_prop, p, x_out (library draws: the step kernel)
        torch.cuda.synchronize()
        return [xn, px, obs["action"], obs["avg_plaq"], obs["top_charge"], dq, *tr], smp.stats.mean_accept()
    finally:
        dyn.all_columns = False


def _assert_equal(dyn, x):
    act, ma = _outputs(dyn, x, False)
    ref, mr = _outputs(dyn, x, True)
    for i, (a, b) in enumerate(zip(act, ref)):
        assert torch.equal(a, b), f"output {i}: max |diff| {float((a - b).abs().max())}"
    assert abs(float(ma) - float(mr)) <= 1e-6 * max(1., abs(float(mr)))
    return act


@pytest.mark.parametrize("B", [16, 130, 2048, 2049, 4096])
def test_active_heads_equal_all_columns(B):
    dyn = _dyn(B)
    assert dyn._plan().heads                     # the plan carries the packed image
    _assert_equal(dyn, _x(B))


def test_step_sums_mean_accept_matches_per_chain_mean():
    from l2hmc_amd import GaugeSampler
    B = 2049
    dyn = _dyn(B)
    x = _x(B)
    dyn._draws = 7
    smp = GaugeSampler(dyn)
    _, px, _, _ = smp.step(x, BETA)
    mean = float(smp.stats.mean_accept())
    assert abs(mean - float(px.double().mean())) <= 4 * np.finfo(np.float32).eps * max(1., mean)


def test_uneven_and_fractional_masks_take_all_columns():
    B = 130
    dyn = _dyn(B)
    m = dyn.mask.detach().cpu().numpy().copy()
    m[1, np.flatnonzero(m[1] == 0)[0]] = 1.      # row 1: D / 2 + 1 ones
    m[4, 7] = 0.5                                # row 4: a fractional entry
    dyn.set_masks(m)
    _assert_equal(dyn, _x(B, seed=5))


def test_image_follows_masks_and_weights():
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    B = 64
    dyn = _dyn(B)
    x = _x(B, seed=9)
    before = _assert_equal(dyn, x)
    rng = np.random.default_rng(1)
    dyn.set_masks(np.stack([rng.permutation(np.repeat([0., 1.], T * X)) for _ in range(N)]))
    after = _assert_equal(dyn, x)
    assert not torch.equal(before[6], after[6])  # the new masks did change the proposal
    tr = GaugeTrainer(dyn)
    dyn._draws = 11
    tr.train_step(x, BETA)
    trained = _assert_equal(dyn, x)
    assert not torch.equal(after[6], trained[6])


def test_overflowing_direction_gives_the_all_columns_pattern():
    """XNet's S head saturated at tanh = 1 with a huge scale: the forward position updates overflow (exp(+eps S)),
    the backward ones stay finite.  NaN / inf pattern, accept probabilities and the finite entries as all columns."""
    B = 64
    dyn = _dyn(B)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in dyn.position_fn.state_dict().items()}
    sd["scale_layer/b"][:] = 50.
    sd["coeff_scale"][:] = np.log(1e30)
    dyn.position_fn.load_state(sd)
    x = _x(B, seed=13)
    act, _ = _outputs(dyn, x, False)
    ref, _ = _outputs(dyn, x, True)
    assert not torch.isfinite(ref[6]).all()      # x_prop: some chains took the overflowing direction
    for i, (a, b) in enumerate(zip(act, ref)):
        assert torch.equal(torch.isnan(a), torch.isnan(b)), f"output {i}: NaN pattern"
        assert torch.equal(torch.isinf(a), torch.isinf(b)), f"output {i}: inf pattern"
        f = torch.isfinite(b)
        assert torch.equal(a[f], b[f]), f"output {i}: finite entries"
    assert torch.equal(act[1], ref[1])           # px
