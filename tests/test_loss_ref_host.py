"""The yardstick of tests/test_gpu_loss_kernels.py, checked before anything is compared with a kernel: `loss_ref` in
float64 against the NumPy oracle of the forward value and against central finite differences, the conditions the
committed inputs must meet, and the host-side refusals of l2hmc_gauge_loss_backward.  No GPU needed."""
import numpy as np
import pytest
import torch

from oracle import loss as oloss
from tests import loss_ref as R

ADDR = 256          # any non-NULL address: these calls never reach a launch


def _t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


@pytest.mark.parametrize("metric", R.METRICS)
def test_terms_equal_the_numpy_oracle(metric):
    T, X, B, seed = 3, 5, 37, 1
    c = R.loss_case(T, X, B, seed)
    ref = R.reference(T, X, B, seed, metric, 1.0 / B)
    w = {k: R.f32(v) for k, v in R.WEIGHTS.items()}
    want = oloss.calc_loss_terms(c["x"], c["xN"][:B], ref.p[:B], c["z"], ref.p[B:], T, X, metric=metric, **w)
    assert np.max(np.abs(ref.terms - want) / np.maximum(1.0, np.abs(want))) < 1e-12


@pytest.mark.parametrize("metric", R.METRICS)
def test_gradients_equal_central_differences(metric):
    T, X, B, seed, h = 2, 3, 2, 3, 1e-6
    c = R.loss_case(T, X, B, seed)
    args = dict(beta=R.BETA, T=T, X=X, metric=metric, inv_count=1.0 / B, dtype=torch.float64, **R.WEIGHTS)

    def loss(xN, vN, sld):
        r = R.loss_ref(c["x"], c["z"], xN, vN, sld, c["H0"], **args)
        return R.f32(1.0 / B) * r.terms.sum()

    ref = R.loss_ref(c["x"], c["z"], c["xN"], c["vN"], c["sld"], c["H0"], **args)
    # the kinks (|.| of the metrics and of the charge difference, the min of p) lie further than h from these inputs
    A = np.log(ref.p[ref.p < 1])
    assert A.size and np.all(A < -10 * h) and (ref.p == 1).any()
    assert np.abs(c["x"] - c["xN"][:B]).min() > 10 * h and np.abs(np.cos(c["x"]) - np.cos(c["xN"][:B])).min() > 10 * h
    assert np.abs(c["z"] - c["xN"][:B]).min() > 10 * h and np.abs(np.cos(c["z"]) - np.cos(c["xN"][:B])).min() > 10 * h
    ins = [np.array(c[k]) for k in ("xN", "vN", "sld")]
    for k, want in enumerate((ref.dxN, ref.dvN, ref.dsld)):
        fd = np.zeros(want.size)
        for i in range(want.size):
            vals = []
            for s in (h, -h):
                a = [v.copy() for v in ins]
                a[k].reshape(-1)[i] += s
                vals.append(loss(*a))
            fd[i] = (vals[0] - vals[1]) / (2 * h)
        err = np.abs(fd - want.reshape(-1)).max() / np.abs(want).max()
        assert err < 1e-6, (metric, ("dxN", "dvN", "dsld")[k], err)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_committed_inputs_meet_their_conditions(case):
    """Conditions on the inputs; no chain is ever left out of a comparison.  They keep every sign the loss
    differentiates through the same in float32 and float64."""
    T, X, B, seed = case
    c = R.loss_case(*case)
    for a in c.values():
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64)) and not a.flags.writeable
    metrics = R.METRICS if case[:3] in R.ALL_METRICS_AT else ('cos_diff',)
    ref = R.reference(T, X, B, seed, metrics[-1], 1.0 / B)
    p = ref.p
    assert (p == 1).any() and p.min() >= 0.05
    assert np.all((p == 1) | (p <= np.exp(-0.015)))          # |A| >= 0.02 up to the rounding of sld
    if B >= 4:
        for half in (p[:B], p[B:]):
            assert (half == 1).any() and (half < 1).any()
    else:
        assert (p < 1).any()
    xp = c["xN"][:B]
    q = lambda a: R.charge_series(_t64(a), T, X).numpy()          # noqa: E731
    assert np.abs(q(c["x"]) - q(xp)).min() >= 1e-3 and np.abs(q(c["z"]) - q(xp)).min() >= 1e-3
    for a in (c["x"], c["z"]):
        assert np.abs(a - xp).min() >= 1e-6                         # 'l1'
        assert np.abs(np.cos(a) - np.cos(xp)).min() >= 1e-6         # 'cos'
    # the float32 evaluation takes the same side of every one of these
    p32 = R.reference(T, X, B, seed, metrics[-1], 1.0 / B, torch.float32).p
    assert np.array_equal(p32 == 1, p == 1)


def test_pairs_cover_every_case_and_metric():
    bwd, fwd = R.case_metric_pairs(True), R.case_metric_pairs(False)
    assert len(bwd) == len(R.CASES) + 4 * len(R.ALL_METRICS_AT) and len(fwd) == len(bwd) - len(R.BACKWARD_ONLY)
    assert {c[:3] for c, _ in bwd} == {c[:3] for c in R.CASES} and len(set(map(R.pair_id, bwd))) == len(bwd)


@pytest.fixture(scope="module")
def L():
    from l2hmc_amd import _lib, build as lbuild
    lbuild.build()
    return _lib.lib()


def test_loss_backward_refuses_a_lattice_that_does_not_fit_lds(L):
    f = L.l2hmc_gauge_loss_backward
    ptrs = [ADDR] * 4
    outs = [ADDR] * 4
    w = (0, 0.7, 0.9, 1.1, 1.3, 0.5)
    assert f(64, 128, 1.7, *ptrs, 1, *w, *outs, None) == 1
    msg = L.l2hmc_last_error().decode()
    assert "lattice" in msg and "LDS" in msg
    assert f(1, 8193, 1.7, *ptrs, 1, *w, *outs, None) == 1 and "LDS" in L.l2hmc_last_error().decode()
    assert f(64, 128, 1.7, *ptrs, 0, *w, *outs, None) == 0          # B = 0: nothing to launch
    assert f(8, 8, 1.7, None, None, None, None, 0, *w, None, None, None, None, None) == 0
    assert f(8, 8, 1.7, *ptrs, -1, *w, *outs, None) == 1 and "bad arguments" in L.l2hmc_last_error().decode()
    assert f(8, 8, 1.7, *ptrs, 1, 5, *w[1:], *outs, None) == 1      # metric out of range
    assert f(8, 8, 1.7, None, *ptrs[1:], 1, *w, *outs, None) == 1 and "NULL" in L.l2hmc_last_error().decode()
