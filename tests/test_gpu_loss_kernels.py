"""The lattice loss kernels and the optimiser kernels on their own, through the C ABI, against float64:
`gauge_loss_kernel` (csrc/loss.hip, l2hmc_gauge_loss_terms), `loss_bwd_kernel` (csrc/train.hip,
l2hmc_gauge_loss_backward), `sumsq_kernel` / `adam_kernel` (l2hmc_grad_sumsq, l2hmc_adam_step).

Reference and inputs: tests/loss_ref.py, validated without a GPU by tests/test_loss_ref_host.py.  Shapes (T, X, B),
each for one way the indexing or the reductions of the two loss kernels can go wrong:
  (2, 3, 5)                 6 sites: lanes mostly idle, waves 1-3 of the forward kernel contribute zeros
  (3, 5, 37)                odd extents, odd B: the z-row offset B + b
  (8, 8, 24)                the shape of test_loss_forward_matches_oracle, kept as the anchor
  (4, 16, 11), (16, 4, 11)  T != X both ways: an i / j or T / X swap that a square lattice hides
  (1, 6, 4), (6, 1, 4)      an extent of 1: both periodic neighbours are the site itself (torch.roll defines the answer)
  (10, 10, 9)               100 sites: a partial second stride-64 pass in the backward kernel
  (12, 24, 3)               288 sites, D = 576: a partial second pass over sites and a partial third over D in the
                            forward kernel, five passes over sites in the backward kernel
  (32, 32, 3)               cfg 5's width, D = 2048
  (64, 64, 2)               backward entry only: the largest lattice its host bound admits, 64 KiB of dynamic LDS
All five metrics run at (3, 5, 37), (10, 10, 9) and (12, 24, 3), cos_diff elsewhere, with non-default weights.

Bars.  The forward entry: that of test_loss_forward_matches_oracle, 5e-5 relative to max(1, |want|).  The backward
entry: the project's `assert_fp32_equivalent` (tests/test_gpu_parity.py, restated) with `loss_ref(float32)` as the fp32
yardstick: max < max(TOL_OP, MAX_RATIO x fp32's own error), rms < max(TOL_OP / 3, RMS_RATIO x fp32's own error).
The kernel takes p as an input, while that yardstick computes p = exp(min(H0 - H1 + sld, 0)) itself and so carries the
float32 rounding of a Hamiltonian of up to some thousands (1e-6 at 6 sites, 1e-3 at 64 x 64: far more than the kernel
can add).  So the same helper is applied a second time with a yardstick that is handed p as the kernel is
(`loss_ref(..., p_in=)`); its own error is 2e-8..8e-7 at every shape, which makes that bar TOL_OP (max) and
TOL_OP / 3 (rms) in effect.  Gradients are compared as those of sum(terms) (outputs / inv_count), so that the helper's
floor of 1 on the scale does not hide a small inv_count; the x rows of dxN whose chain has p == 1 carry no force
term and are compared once more on their own, smaller, scale.  What the MI355X gives is in
profiles/loss_kernels_parity.txt and in the docstring of `test_backward_entry_matches_float64`."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import loss_ref as R

pytestmark = pytest.mark.gpu

TOL_OP = 1e-5
MAX_RATIO, RMS_RATIO = 5.0, 1.6       # tests/test_gpu_parity.py: allowances over the fp32 yardstick's own error
W = R.WEIGHTS
BWD_PAIRS, FWD_PAIRS = R.case_metric_pairs(True), R.case_metric_pairs(False)


def rmserr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2)) / max(1.0, np.max(np.abs(want))))


def assert_fp32_equivalent(got, want64, want32, what):
    """`got` is as close to the float64 reference as an fp32 evaluation in the reference's op order
    (tests/test_gpu_parity.py::assert_fp32_equivalent, restated)."""
    emax, imax = H.relerr(got, want64), H.relerr(want32, want64)
    erms, irms = rmserr(got, want64), rmserr(want32, want64)
    ratio = lambda e, i: e / i if i > 0 else float("inf") if e > 0 else 0.0          # noqa: E731
    print(f"parity {what}: max {emax:.3e} (fp32 {imax:.3e}, ratio {ratio(emax, imax):.2f}), "
          f"rms {erms:.3e} (fp32 {irms:.3e}, ratio {ratio(erms, irms):.2f})")
    assert emax < max(TOL_OP, MAX_RATIO * imax), f"{what}: max err {emax:.2e} vs intrinsic fp32 {imax:.2e}"
    assert erms < max(TOL_OP / 3, RMS_RATIO * irms), f"{what}: rms err {erms:.2e} vs intrinsic fp32 {irms:.2e}"


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


_RUNS = {}


def _backward(case, metric, inv_count, with_terms=True):
    """One launch of l2hmc_gauge_loss_backward on a committed case -> (terms or None, dxN, dvN, dlogdet) as float32
    NumPy arrays.  Every output buffer is pre-filled with 7."""
    key = (case, metric, inv_count, with_terms)
    if key not in _RUNS:
        from l2hmc_amd import _lib
        T, X, B, seed = case
        D = 2 * T * X
        c = R.loss_case(*case)
        p = R.reference(T, X, B, seed, metric, 1.0 / B).p
        dev = _dev()
        ins = [_lib.as_dev(torch.tensor(a), dev) for a in (np.concatenate([c["x"], c["z"]]), c["xN"], c["vN"], p)]
        terms = torch.full((B,), 7., device=dev)
        outs = [torch.full((2 * B, D), 7., device=dev), torch.full((2 * B, D), 7., device=dev),
                torch.full((2 * B,), 7., device=dev)]
        _lib.check(_lib.lib().l2hmc_gauge_loss_backward(
            T, X, R.BETA, *[t.data_ptr() for t in ins], B, R.METRICS.index(metric), W["loss_scale"], W["aux_weight"],
            W["std_weight"], W["charge_weight"], inv_count, terms.data_ptr() if with_terms else None,
            *[t.data_ptr() for t in outs], _lib.stream_ptr()))
        torch.cuda.synchronize()
        _RUNS[key] = (terms.cpu().numpy() if with_terms else None,) + tuple(t.cpu().numpy() for t in outs)
    return _RUNS[key]


def _forward(case, metric):
    key = (case, metric)
    if key not in _RUNS:
        from l2hmc_amd import _lib
        T, X, B, seed = case
        c = R.loss_case(*case)
        p = R.reference(T, X, B, seed, metric, 1.0 / B).p
        dev = _dev()
        ins = [_lib.as_dev(torch.tensor(a), dev) for a in (c["x"], c["xN"][:B], p[:B], c["z"], p[B:])]
        terms = torch.full((B,), 7., device=dev)
        _lib.check(_lib.lib().l2hmc_gauge_loss_terms(
            *[t.data_ptr() for t in ins], B, T, X, R.METRICS.index(metric), W["loss_scale"], W["aux_weight"],
            W["std_weight"], W["charge_weight"], terms.data_ptr(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        _RUNS[key] = terms.cpu().numpy()
    return _RUNS[key]


@pytest.mark.parametrize("pair", FWD_PAIRS, ids=R.pair_id)
def test_forward_entry_matches_float64(pair):
    case, metric = pair
    T, X, B, seed = case
    want = R.reference(T, X, B, seed, metric, 1.0 / B).terms
    got = _forward(case, metric)
    assert np.isfinite(got).all() and not (got == 7.).any()
    err = np.max(np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want)))
    print(f"parity forward {R.pair_id(pair)} terms: max {err:.3e}")
    assert err < 5e-5


@pytest.mark.parametrize("pair", BWD_PAIRS, ids=R.pair_id)
def test_backward_entry_matches_float64(pair):
    """Measured on the MI355X over all cases and metrics (profiles/loss_kernels_parity.txt): kernel errors of at most
    8.4e-7 (max) and 1.2e-7 (rms), 12 and 28 times below the absolute bars.  Ratios to the fp32 yardstick's own error:
    at most 1.20 (max) and 1.06 (rms) where it computes p itself; at most 3.80 (max) and 3.62 (rms) where it is handed
    p.  The rms ratio passes RMS_RATIO = 1.6 in six quantities, all at rms errors of 1.5e-8..1.2e-7 where the fp32
    evaluation happened to land within a fraction of one rounding; the absolute bars decide there, so the allowances
    stay the project's (MAX_RATIO = 5, RMS_RATIO = 1.6)."""
    case, metric = pair
    T, X, B, seed = case
    inv = 1.0 / B
    w64 = R.reference(T, X, B, seed, metric, inv)
    w32 = R.reference(T, X, B, seed, metric, inv, torch.float32)
    terms, dxN, dvN, dld = _backward(case, metric, inv)
    for name, a in (("terms", terms), ("dxN", dxN), ("dvN", dvN), ("dlogdet", dld)):
        assert np.isfinite(a).all(), name          # pre-filled with 7: every element of all 2B rows is overwritten
    assert not (terms == 7.).any() and not (dxN == 7.).any() and not (dvN == 7.).any() and not (dld == 7.).any()
    assert not (dxN[:B] == 0).any()                                       # every link of an x row gets a metric term
    tag = R.pair_id(pair)
    s = 1.0 / R.f32(inv)          # gradients of sum(terms)
    free = w64.p[:B] == 1          # x rows without a force term
    for how, y32 in (("", w32), (" (p given)", R.reference(T, X, B, seed, metric, inv, torch.float32, given_p=True))):
        assert_fp32_equivalent(terms, w64.terms, y32.terms, f"{tag} terms{how}")
        assert_fp32_equivalent(dxN * s, w64.dxN * s, y32.dxN * s, f"{tag} dxN{how}")
        assert_fp32_equivalent(dvN * s, w64.dvN * s, y32.dvN * s, f"{tag} dvN{how}")
        assert_fp32_equivalent(dld * s, w64.dsld * s, y32.dsld * s, f"{tag} dlogdet{how}")
        if free.any():
            assert_fp32_equivalent(dxN[:B][free] * s, w64.dxN[:B][free] * s, y32.dxN[:B][free] * s,
                                   f"{tag} dxN[px == 1]{how}")
    # exact relations, bit for bit
    assert (dld[w64.p == 1] == 0).all() and (dld[w64.p < 1] != 0).all()
    vN = R.loss_case(*case)["vN"].astype(np.float32)
    assert np.array_equal(dvN, -(dld[:, None] * vN))
    assert (dxN[B:][w64.p[B:] == 1] == 0).all() and (dvN[w64.p == 1] == 0).all()


@pytest.mark.parametrize("pair", FWD_PAIRS, ids=R.pair_id)
def test_the_two_copies_of_the_forward_arithmetic_agree(pair):
    """`metric_val` and the projection series exist in loss.hip and in train.hip; only the summation order differs."""
    case, metric = pair
    fwd = _forward(case, metric).astype(np.float64)
    bwd = _backward(case, metric, 1.0 / case[2])[0].astype(np.float64)
    assert np.all(np.abs(fwd - bwd) <= 2e-6 * np.maximum(1.0, np.abs(fwd))), np.abs(fwd - bwd).max()


@pytest.mark.parametrize("pair", BWD_PAIRS, ids=R.pair_id)
def test_backward_entry_without_terms_and_with_another_count(pair):
    case, metric = pair
    B = case[2]
    terms, dxN, dvN, dld = _backward(case, metric, 1.0 / B)
    none, dxN0, dvN0, dld0 = _backward(case, metric, 1.0 / B, with_terms=False)          # terms = NULL is accepted
    assert none is None
    assert np.array_equal(dxN, dxN0) and np.array_equal(dvN, dvN0) and np.array_equal(dld, dld0)
    # inv_count / 4: a power of two scales every gradient exactly; the forward value does not see it
    terms4, dxN4, dvN4, dld4 = _backward(case, metric, 1.0 / (4 * B))
    assert np.array_equal(terms4, terms)
    quarter = np.float32(0.25)
    assert np.array_equal(dxN4, dxN * quarter) and np.array_equal(dvN4, dvN * quarter)
    assert np.array_equal(dld4, dld * quarter)


# ------------------------------------------------------------------------------------------------ optimiser
def _sumsq(g, n, lo, hi, out, accumulate):
    from l2hmc_amd import _lib
    _lib.check(_lib.lib().l2hmc_grad_sumsq(g.data_ptr(), n, lo, hi, out.data_ptr(), accumulate, _lib.stream_ptr()))


@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 2 ** 20 + 3])
def test_grad_sumsq_matches_float64(n):
    """Elements in [tri_lo, tri_hi) count three times.  The per-thread fp32 accumulation at cfg 5's 1.5e8 weights
    has never been measured and is not tested here; the error at 2^20 + 3 is in profiles/loss_kernels_parity.txt."""
    from l2hmc_amd import _lib
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n).astype(np.float32)
    g64 = g.astype(np.float64)
    gd = _lib.as_dev(g, _dev())
    out = torch.empty(1, device=_dev())
    k = n // 2 if n < 2048 else 1024 * 500 + 17          # where the split buffer is cut
    preset = 2.5
    idx = np.arange(n)
    # tri range: empty; straddling index 1024 (where n reaches it); everything
    for lo, hi in ((5, 5), (1000, 1050), (0, n)):
        want = float(np.sum(np.where((idx >= lo) & (idx < hi), 3., 1.) * g64 * g64))
        out.fill_(7.)
        _sumsq(gd, n, lo, hi, out, 0)
        whole = float(out.cpu()[0])
        err = abs(whole - want) / want
        print(f"parity sumsq n={n} tri=[{lo},{hi}): rel err {err:.3e}")
        assert err < TOL_OP
        out.fill_(preset)
        _sumsq(gd, n, lo, hi, out, 1)
        assert abs(float(out.cpu()[0]) - (preset + want)) / (preset + want) < TOL_OP
        out.fill_(7.)
        _sumsq(gd, k, lo, hi, out, 0)
        _sumsq(gd[k:], n - k, lo - k, hi - k, out, 1)
        split = float(out.cpu()[0])
        assert abs(split - want) / want < TOL_OP and abs(split - whole) / want < TOL_OP


def test_adam_step_matches_float64_in_every_clipping_state():
    """tf.train.AdamOptimizer's update with clip_by_global_norm on one ragged segment: no clipping (gnorm_sq = NULL),
    norm < clip (scale exactly 1: bit-equal to the NULL call) and norm > clip; three steps with changing gradients;
    the bar of test_adam_matches_reference_update_rule for w, m and v."""
    from l2hmc_amd import _lib
    L, dev = _lib.lib(), _dev()
    n, pad, lo, hi = 257, 31, 100, 180
    lr, b1, b2, eps = map(R.f32, (0.05, 0.9, 0.999, 1e-8))
    rng = np.random.default_rng(11)
    w0 = rng.standard_normal(n).astype(np.float32)
    gs = [rng.standard_normal(n).astype(np.float32) * np.float32(s) for s in (1.0, 0.5, 2.0)]
    tri = np.where((np.arange(n) >= lo) & (np.arange(n) < hi), 3., 1.)
    got = {}
    for state, clip in (("null", 0.), ("below", 1000.), ("above", 0.5)):
        buf = [torch.full((n + pad,), 7., device=dev) for _ in range(3)]          # w, m, v with a sentinel tail
        buf[0][:n] = torch.as_tensor(w0)
        buf[1][:n] = 0.
        buf[2][:n] = 0.
        w, m, v = w0.astype(np.float64), np.zeros(n), np.zeros(n)
        for t, g in enumerate(gs, start=1):
            g64 = g.astype(np.float64)
            gd = _lib.as_dev(np.concatenate([g, np.full(pad, 1e6, dtype=np.float32)]), dev)
            lr_t = R.f32(lr * (1. - b2 ** t) ** 0.5 / (1. - b1 ** t))
            gn = None
            scale = 1.
            if state != "null":
                gn = torch.tensor([float(np.sum(tri * g64 * g64))], dtype=torch.float32, device=dev)
                norm = np.sqrt(float(gn.cpu()[0]))
                assert (norm < clip) == (state == "below") and abs(norm - clip) > 1.
                scale = R.f32(clip) / max(norm, R.f32(clip))
            _lib.check(L.l2hmc_adam_step(buf[0].data_ptr(), gd.data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), n,
                                         lr_t, b1, b2, eps, gn.data_ptr() if gn is not None else None, clip, lo, hi,
                                         _lib.stream_ptr()))
            gc = g64 * scale
            m = b1 * m + (1. - b1) * gc
            v = b2 * v + (1. - b2) * gc * gc
            w = w - tri * lr_t * m / (np.sqrt(v) + eps)
            res = [b.cpu().numpy() for b in buf]
            for name, a, want in zip("wmv", res, (w, m, v)):
                np.testing.assert_allclose(a[:n], want, rtol=2e-5, atol=2e-7, err_msg=f"{state} step {t} {name}")
                assert (a[n:] == 7.).all(), (state, t, name)          # nothing outside [0, n) is touched
        got[state] = res
    for a, b in zip(got["null"], got["below"]):
        assert np.array_equal(a, b)
    assert not np.array_equal(got["null"][0], got["above"][0])
