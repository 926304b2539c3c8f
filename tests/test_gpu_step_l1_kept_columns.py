"""The whole-step kernel's kept-column first layer: in split step mode a position sub-update forms XNet's first-layer
product with keep (.) x over the D / 2 columns it keeps (l2hmc_gauge_pack_heads packs those rows of W1 per mask row
and keep sense, in the order the matrix instruction takes its k).  Every output must EQUAL the full-K form
(L2HMC_PLAN_FULL_L1) bit for bit, whatever the mask does to the k order; ineligible mask rows keep the full first
layer; a 0 x non-finite in a moving column still turns the row's product into NaN; the image follows W1."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

T = X = 8
D = 2 * T * X
N, EPS, BETA = 10, 0.25, 2.0


def _random_masks(rng, n=N):
    masks = np.zeros((n, D), np.float32)
    for s in range(n):
        masks[s, rng.permutation(D)[:D // 2]] = 1.
    return masks


def _dyn(B, masks=None, seed=106):
    xp, vp = H.gauge_weights(T, X, seed=seed, regime="mild")
    if masks is None:
        masks = _random_masks(np.random.default_rng(seed))
    dyn = H.gauge_hip(T, X, len(masks), EPS, xp, vp, masks, B)
    dyn.tiles16_only = True                       # every batch on the 16-row form
    return dyn


def _x(B, seed=3):
    rng = np.random.default_rng(seed)
    return torch.as_tensor(rng.uniform(0, 2 * np.pi, (B, D)), dtype=torch.float32, device="cuda")


def _outputs(dyn, x, full_l1=False, all_columns=False, draw=40):
    from l2hmc_amd import GaugeSampler
    dyn.full_l1, dyn.all_columns = full_l1, all_columns
    try:
        dyn._draws = draw
        smp = GaugeSampler(dyn)
        xn, px, obs, dq = smp.step(x, BETA)
        dyn._draws = draw
        tr = dyn.apply_transition(x, BETA)       # x_prop, v_prop, p, x_out (library draws: the step kernel)
        torch.cuda.synchronize()
        return [xn, px, obs["action"], obs["avg_plaq"], obs["top_charge"], dq, *tr], smp.stats.mean_accept()
    finally:
        dyn.full_l1 = dyn.all_columns = False


def _assert_same(got, want):
    (act, ma), (ref, mr) = got, want
    for i, (a, b) in enumerate(zip(act, ref)):
        assert torch.equal(a, b), f"output {i}: max |diff| {float((a - b).abs().max())}"
    assert abs(float(ma) - float(mr)) <= 1e-6 * max(1., abs(float(mr)))


def _assert_equal_full_l1(dyn, x):
    got = _outputs(dyn, x)
    _assert_same(got, _outputs(dyn, x, full_l1=True))
    return got


@pytest.mark.parametrize("B", [16, 130, 2049])
def test_kept_columns_equal_full_first_layer(B):
    """One workgroup pair; a partial last workgroup; without tiles16_only B = 2049 is a 16-row round plus the sub-tile
    remainder (which keeps full K), and both launch plans must agree with the switch."""
    dyn = _dyn(B)
    assert dyn._plan().heads                     # the plan carries the packed image
    x = _x(B)
    got = _assert_equal_full_l1(dyn, x)
    if B == 2049:
        dyn.tiles16_only = False
        _assert_same(_assert_equal_full_l1(dyn, x), got)


def _structured_masks():
    c = np.arange(D)
    first_half = (c < D // 2).astype(np.float32)               # the kept columns fill whole chunks
    even = (c % 2 == 0).astype(np.float32)                     # every chunk keeps e in {0, 2} (or {1, 3}) only
    q_even = ((c % 16) // 4 % 2 == 0).astype(np.float32)       # ... q in {0, 2} (or {1, 3}) only
    rnd = _random_masks(np.random.default_rng(7), 4)
    return np.stack([first_half, even, q_even, 1 - first_half, 1 - even, 1 - q_even, *rnd])


def test_masks_that_stress_the_k_permutation():
    masks = _structured_masks()
    B = 48
    dyn = _dyn(B, masks)
    x = _x(B, seed=4)
    got = _assert_equal_full_l1(dyn, x)
    _assert_same(got, _outputs(dyn, x, all_columns=True))
    # each structured row alone (a wrong order in e or in q cannot hide behind the other rows)
    for s in range(3):
        d1 = _dyn(B, np.stack([masks[s], masks[s + 3]]))
        _assert_equal_full_l1(d1, x)


def test_uneven_and_fractional_rows_keep_the_full_first_layer():
    B = 130
    dyn = _dyn(B)
    m = dyn.mask.detach().cpu().numpy().copy()
    m[1, np.flatnonzero(m[1] == 0)[0]] = 1.      # row 1: D / 2 + 1 ones
    m[4, 7] = 0.5                                # row 4: a fractional entry
    dyn.set_masks(m)
    x = _x(B, seed=5)
    got = _assert_equal_full_l1(dyn, x)
    _assert_same(got, _outputs(dyn, x, all_columns=True))


def test_overflowing_direction_gives_the_full_first_layer_pattern():
    """XNet's S head saturated at tanh = 1 with a huge scale: the forward position updates overflow (exp(+eps S)) and
    0 x inf = NaN enters the full first layer through the moving columns; the kept-column form must poison the same rows."""
    B = 64
    dyn = _dyn(B)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in dyn.position_fn.state_dict().items()}
    sd["scale_layer/b"][:] = 50.
    sd["coeff_scale"][:] = np.log(1e30)
    dyn.position_fn.load_state(sd)
    x = _x(B, seed=13)
    act, _ = _outputs(dyn, x)
    ref, _ = _outputs(dyn, x, full_l1=True)
    assert not torch.isfinite(ref[6]).all()      # x_prop: some chains took the overflowing direction
    for i, (a, b) in enumerate(zip(act, ref)):
        assert torch.equal(torch.isnan(a), torch.isnan(b)), f"output {i}: NaN pattern"
        assert torch.equal(torch.isinf(a), torch.isinf(b)), f"output {i}: inf pattern"
        f = torch.isfinite(b)
        assert torch.equal(a[f], b[f]), f"output {i}: finite entries"
    assert torch.equal(act[1], ref[1])           # px


def test_image_follows_first_layer_weights():
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    B = 64
    dyn = _dyn(B)
    x = _x(B, seed=9)
    before, _ = _assert_equal_full_l1(dyn, x)
    tr = GaugeTrainer(dyn)
    dyn._draws = 11
    tr.train_step(x, BETA)
    trained, _ = _assert_equal_full_l1(dyn, x)
    assert not torch.equal(before[6], trained[6])
