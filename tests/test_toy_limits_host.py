"""Host side of the toy-kernel limit tests (tests/toy_cases.py, tests/test_gpu_toy_limits.py), no GPU needed:
  * the two target builders agree: what l2hmc_amd packs for the kernels is what the oracle computes with;
  * the input conditions the GPU tests lean on hold in float64: no chain within 1e-4 of an accept tie, no hidden
    pre-activation of a training case within 1e-5 of zero, no H0 - H1 + logdet within 1e-4 of zero;
  * no gradient entry a training test measures against is a cancellation of the chains' shares;
  * every case can tell: an oracle without its last hidden unit, without its last component (or one precision
    entry), or blind to its last coordinate sits at least 100 bars away from the oracle on every output compared;
  * the C entries refuse one past each limit with L2HMC_ERR_ARG before any device call."""
import ctypes as C

import numpy as np
import pytest

from l2hmc_amd import _lib
from tests import toy_cases as tc

PTR = 16          # any non-NULL address: host checks only
ERR_ARG = 1


def _ids(cases):
    return [tc.case_id(c) for c in cases]


def test_the_case_tables_cover_what_they_promise():
    S = tc.SAMPLING_CASES
    classes = lambda H: 0 if H <= 16 else 1 if H <= 50 else 2        # noqa: E731 -- small_launch's instance classes
    assert {4, 5, 7, 8} <= {c.dim for c in S}
    for dim in (4, 5, 7, 8):
        assert {classes(c.H) for c in S if c.dim == dim} == {0, 1, 2}, dim
    assert {(1, tc.G), (1, tc.M), (4, tc.M), (8, tc.M)} <= {(c.K, c.kind) for c in S}
    assert {1, 16, 17, 50, 51, 63, 64} <= {c.H for c in S}
    assert {(8, 8, 64), (8, 8, 1)} <= {(c.dim, c.K, c.H) for c in S}
    assert {"stress", "mild"} <= {c.regime for c in S}
    assert all(c.N <= 5 for c in S) and max(tc.SAMPLING_BATCHES) == 37 and 1 in tc.SAMPLING_BATCHES
    assert len(tc.PIECEWISE_CASES) == 3 and len(tc.LAYERED_CASES) == 2
    want = {(4, 4, tc.M, 16, 4, 21, 1.0), (5, 8, tc.M, 17, 3, 9, 1.0), (7, 1, tc.G, 50, 4, 19, 1.0),
            (8, 1, tc.G, 51, 3, 17, 1.0), (8, 8, tc.M, 64, 3, 37, 1.0), (8, 4, tc.M, 1, 3, 9, 1.0),
            (4, 8, tc.M, 64, 5, 16, 2.5)}
    assert want <= {(c.dim, c.K, c.kind, c.H, c.N, c.B, c.temperature) for c in tc.TRAIN_CASES}
    for c in S:          # odd dimensions keep int(dim / 2) coordinates per step
        assert (tc.masks(c.N, c.dim, c.seed).sum(axis=1) == c.dim // 2).all()


ALL_TARGETS = sorted({(c.dim, c.K, c.kind) for c in tc.SAMPLING_CASES + tc.TRAIN_CASES} | set(tc.TARGET_CASES))


@pytest.mark.parametrize("dim,K,kind", ALL_TARGETS)
def test_both_target_builders_hold_the_same_arrays(dim, K, kind):
    tgt_o, tgt = tc.target(dim, K, kind)
    packed = tgt.get_energy_function().target
    assert (packed.dim, packed.K, packed.is_gaussian) == (dim, K, int(kind == tc.G))
    for name, got, want in zip(("mu", "precision", "log_const"), packed._host, tc.oracle_packing(tgt_o)):
        assert got.dtype == np.float32 and got.shape == want.shape, name
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1e-12, name
    mus, covs, pis = tc.target_arrays(dim, K)
    for S in covs:          # full, not diagonal, eigenvalues in [0.05, 0.3]
        w = np.linalg.eigvalsh(S)
        assert 0.05 <= w.min() and w.max() <= 0.3 and np.abs(S - np.diag(np.diag(S))).max() > 1e-3
    assert all(np.abs(m).max() <= 1 for m in mus) and (K == 1 or np.ptp(pis) > 0.01)
    # the oracle's closed-form gradient is the gradient of its energy (central differences in float64)
    x = tgt_o.get_samples(5, np.random.default_rng(0))
    g = tgt_o.grad_energy(x)
    for d in range(dim):
        e = np.zeros(dim)
        e[d] = 1e-6
        assert np.abs((tgt_o.energy(x + e) - tgt_o.energy(x - e)) / 2e-6 - g[:, d]).max() < 1e-5 * max(1., np.abs(g).max())


@pytest.mark.parametrize("c", tc.SAMPLING_CASES, ids=_ids(tc.SAMPLING_CASES))
def test_sampling_case_conditions(c):
    for B in tc.SAMPLING_BATCHES:
        w64, w32 = tc.sampling_reference(c, B)
        assert all(np.isfinite(v).all() for v in w64.values())
        # no chain is left out of the Metropolis-Hastings comparison
        assert tc.mh_safe(c, B).all(), (B, np.abs(w64["px"] - tc.sampling_inputs(c, B)["u"]).min())
        # the float32 oracle against the bars' floors: within them, or its ratio carries the bar
        for k in w64:
            if k in tc.P_OUTPUTS:
                own, floor = float(np.abs(w32[k] - w64[k]).max()), tc.TOL_P
                ratio = tc.P_RATIO
            else:
                own, floor, ratio = tc.relerr(w32[k], w64[k]), tc.TOL_OP, tc.MAX_RATIO
            print(f"{tc.case_id(c)} B={B} {k}: fp32 oracle {own:.2e}, bar "
                  f"{max(floor, ratio * own):.2e} ({'floor' if ratio * own <= floor else 'ratio'})")
            assert np.isfinite(own)
    acc = tc.sampling_reference(c, 37)[0]["px"] >= tc.sampling_inputs(c, 37)["u"]
    assert 0 < acc.sum() < 37, "the batch must hold accepted AND rejected proposals"


@pytest.mark.parametrize("perturb", tc.PERTURBATIONS)
@pytest.mark.parametrize("c", tc.SAMPLING_CASES, ids=_ids(tc.SAMPLING_CASES))
def test_sampling_case_sees_its_last_unit_component_and_coordinate(c, perturb):
    B = 37
    w64, w32 = tc.sampling_reference(c, B)
    off = tc.sampling_outputs(c, B, perturb=perturb)
    low = {}
    for k in w64:
        if k in tc.P_OUTPUTS:
            dist, bar = float(np.abs(off[k] - w64[k]).max()), tc.p_bar(w64[k], w32[k])
        else:
            dist, bar = tc.relerr(off[k], w64[k]), tc.max_bar(w64[k], w32[k])
        if not dist >= tc.SEES * bar:
            low[k] = dist / bar
    assert not low, f"{perturb}: within {tc.SEES:.0f} bars of the oracle on {low}"


@pytest.mark.parametrize("c", tc.TRAIN_CASES, ids=_ids(tc.TRAIN_CASES))
def test_training_case_conditions(c):
    relu, arg = tc.train_margins(c)
    assert relu > tc.RELU_MARGIN, f"a hidden pre-activation {relu:.2e} from zero: a relu flip in fp32 decides a gradient"
    assert arg > tc.MIN_MARGIN, f"H0 - H1 + logdet {arg:.2e} from zero: min() may change branch in fp32"
    tm, loss, _, p = tc.train_reference(c)
    assert np.isfinite(loss) and (p < 1).sum() >= 4 and (p == 1).sum() >= 2          # both branches of the min
    for name, net in (("xnet", tm.xnet), ("vnet", tm.vnet)):
        for k, t in net.items():
            assert np.isfinite(t.grad.numpy()).all() and float(t.grad.abs().max()) > 0, (name, k)
        wh_t = net['linear_1/W'].grad.numpy().T                                      # the packed layout: a row per unit
        share = np.abs(wh_t[-1]).max() / np.abs(wh_t).max()
        assert share >= tc.SEES * tc.TOL_G, f"{name}: the last unit's wh_t row is {share:.1e} of the tensor's max"
    assert float(tm.alpha.grad.abs()) > 0
    i = tc.train_inputs(c)
    assert np.abs(p[:c.B] - i["dx"][3]).min() > tc.MH_MARGIN                         # no accept tie among the x chains
    # the two float64 references (torch model, NumPy oracle) are one computation
    w64, _ = tc.train_forward_reference(c)
    x0, v0, dirs = tc.train_rows(c)
    assert np.abs(w64["p"] - p).max() < 1e-9 and (dirs == 1).sum() == 2 * c.B - i["dx"][2].sum() - i["dz"][2].sum()
    for bits in (i["dx"][2], i["dz"][2]):
        assert 0 < bits.sum() < c.B                                                  # both directions run


@pytest.mark.parametrize("c", tc.TRAIN_CASES, ids=_ids(tc.TRAIN_CASES))
def test_training_case_gradients_are_no_cancellations(c):
    """At the entry a gradient tensor's error is measured against, the chains' shares do not cancel (tc.cancellation):
    for the loss both training routes differentiate, and for the functional of the l2hmc_small_vjp test."""
    tm, rows = tc.mog_loss_rows(c)
    assert abs(float(rows.sum().detach()) - tc.train_reference(c)[1]) < 1e-9
    for what, (tm, rows) in (("loss", (tm, rows)), ("vjp", tc.vjp_reference(c)[::3])):
        worst = {k: v for k, v in tc.cancellation(tm, rows).items() if not v <= tc.CANCELLATION}
        assert not worst, (what, worst)
    assert all(np.abs(g).min() > 0 for g in tc.vjp_cotangents(c))


@pytest.mark.parametrize("dim,K,kind", tc.TARGET_CASES)
def test_target_points_hold_rows_far_from_every_mean(dim, K, kind):
    mus, covs, _ = tc.target_arrays(dim, K)
    for rows in tc.TARGET_ROWS:
        x, u = tc.target_points(dim, K, kind, rows)
        assert x.shape == u.shape == (rows, dim) and x.dtype == np.float32
        d2 = np.stack([np.einsum('bi,ij,bj->b', x - m, np.linalg.inv(S), x - m) for m, S in zip(mus, covs)], axis=1)
        far = (d2.min(axis=1) >= 9.0 - 1e-3).sum()
        assert far >= min(4, rows - 1)
        for t in tc.TARGET_TEMPERATURES:
            e, g, hv = tc.target_reference(dim, K, kind, rows, t)
            assert np.isfinite(e).all() and np.isfinite(g).all() and np.isfinite(hv).all()


# ------------------------------------------------------------------------------------------------------ refusals
def _net(dim, H):
    return _lib.DenseNet(D=dim, H=H, Ka=dim, Kb=dim, w1_t=PTR, wt=PTR, b1=PTR, wh_t=PTR, bh=PTR, whd_t=PTR, bhd=PTR,
                         coeff_s=PTR, coeff_q=PTR, q_tanh=1)


def _target(dim=8, K=8):
    return _lib.MogTarget(dim=dim, K=K, is_gaussian=0, temperature=1.0, mu=PTR, prec=PTR, log_const=PTR)


def _plan(dim=8, K=8, H=64):
    return _lib.SmallPlan(x_dim=dim, num_nodes=H, trajectory_length=3, hmc=0, eps=0.1, first_layer_form=0, masks=PTR,
                          xnet=_net(dim, H), vnet=_net(dim, H), target=_target(dim, K))


PLAN_ENTRIES = {
    "l2hmc_small_trajectory": lambda L, p: L.l2hmc_small_trajectory(C.byref(p), PTR, PTR, PTR, 4, PTR, PTR, PTR, PTR, None),
    "l2hmc_small_propose": lambda L, p: L.l2hmc_small_propose(C.byref(p), PTR, 4, 42, 0, PTR, PTR, PTR, PTR, None),
    "l2hmc_small_run": lambda L, p: L.l2hmc_small_run(C.byref(p), PTR, PTR, 4, 42, 0, 2, PTR, PTR, None),
    "l2hmc_small_run_tempered": lambda L, p: L.l2hmc_small_run_tempered(C.byref(p), PTR, PTR, 4, 42, 0, 2, PTR, 0, 0, PTR,
                                                                        PTR, None),
    "l2hmc_small_train_step": lambda L, p: L.l2hmc_small_train_step(C.byref(p), PTR, PTR, PTR, 4, 0.1, 0.25, PTR, PTR,
                                                                    PTR, PTR, PTR, PTR, 1 << 30, None),
    "l2hmc_small_vjp": lambda L, p: L.l2hmc_small_vjp(C.byref(p), PTR, PTR, PTR, 4, *([PTR] * 11), PTR, 1 << 30, None),
}
TARGET_ENTRIES = {
    "l2hmc_mog_energy_grad": lambda L, t: L.l2hmc_mog_energy_grad(C.byref(t), PTR, 4, PTR, PTR, None),
    "l2hmc_mog_energy_hvp": lambda L, t: L.l2hmc_mog_energy_hvp(C.byref(t), PTR, PTR, 4, PTR, None),
}
PAST_THE_LIMITS = [(dict(dim=9), "dim=9 (max 8)"), (dict(K=9), "K=9 (max 8)"), (dict(H=65), "num_nodes=65"),
                   (dict(H=0), "num_nodes=0")]


@pytest.mark.parametrize("entry", sorted(PLAN_ENTRIES))
def test_plan_entries_refuse_one_past_each_limit_before_any_device_call(entry):
    L = _lib.lib()
    for bad, word in PAST_THE_LIMITS:
        assert PLAN_ENTRIES[entry](L, _plan(**bad)) == ERR_ARG, (entry, bad)
        assert word in L.l2hmc_last_error().decode(), (entry, bad, L.l2hmc_last_error().decode())


@pytest.mark.parametrize("entry", sorted(TARGET_ENTRIES))
def test_target_entries_refuse_one_past_each_limit_before_any_device_call(entry):
    L = _lib.lib()
    for bad, word in PAST_THE_LIMITS[:2]:
        assert TARGET_ENTRIES[entry](L, _target(**bad)) == ERR_ARG, (entry, bad)
        assert word in L.l2hmc_last_error().decode(), (entry, bad, L.l2hmc_last_error().decode())


def test_python_constructors_route_by_the_same_limits():
    import torch
    import l2hmc_amd as la
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="beyond the fused kernel's limits"):
        la.GMM([np.zeros(2)] * 9, [np.eye(2)] * 9, [1. / 9] * 9).get_energy_function()
    with pytest.raises(ValueError, match="beyond the fused kernel's limits"):
        la.Gaussian(np.zeros(9), np.eye(9)).get_energy_function()
    _, tgt = tc.target(8, 8, tc.M)
    for H_nodes, layered in ((64, False), (65, True), (1, False)):
        dyn = la.Dynamics(8, tgt.get_energy_function(), trajectory_length=3, eps=0.1, device=cpu,
                          net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=H_nodes, device=cpu))
        assert dyn.layered == layered, H_nodes
