"""Torus-exact training (`GaugeDynamics(periodic=True, tiled_train=True[, fused_forward=True])`) at the benchmark's
trajectory length and at the batches where the weight-gradient reductions split: what
tests/test_gpu_periodic_train.py and tests/test_gpu_periodic_train_forward.py (N <= 3, at most 37 chains, at most two
split-k parts) cannot see.

a. The taped launch (the TAPE instances of gauge_traj_ncp_kernel) has the bits of `l2hmc_gauge_trajectory` of a
   `whole_step=True` dynamics at N = 10 (the tape's call offset [2 N calls][rows] at 20 calls) and at 16 CUS + 2 rows
   (CUS + 1 workgroups; N = 2), scalar beta and ladder, `recompute=True` too.
b. Gradients at N = 10, 9 + 9 chains, 8x8 "mild", against float64 autograd at TOL_G = 2e-4 of each tensor's maximum,
   through the layer-by-layer taped forward, the one-launch taped forward, and on a ladder of betas.
   The seeds: a ten-step trajectory of 18 rows evaluates 737 000 relu pre-activations per network pair, and about
   twelve of them land within the 1e-5 of `TorchPeriodic.flip_free`'s default: no seed has none (400 seeds scanned on
   the CPU, the best 8.1e-6 on one beta and 7.6e-6 on the ladder).  The cases take those two seeds and the margin
   FLIP_MARGIN = 5e-6.  At both, float32 torch autograd of the same graph flips no relu and lies within TOL_G / 4 of
   float64 (1.3e-5 and 3.2e-5 of the tensor's maximum; the condition is asserted here on every run).
c. The three checks of tests/test_gpu_train_batch.py (batch additivity against shards of 32 chains after the forward
   outputs are shown bit identical; float64 autograd at the full batch; a second call bit equal) with its constants, on
   the periodic tiled entries at 1100 + 1100 and (8 CUS + 1) + (8 CUS + 1) chains, where every weight-gradient product
   of both networks -- the first layer's at the fan-in 3 D that only this mode has -- runs in at least two split-k parts
   with a ragged last part and the column sums in at least two chunks (asserted through that file's mirrors).

Measured on the MI355X (256 CUs).  a. bit equal in all four cases, recompute too.  b. worst tensor as error / max: 2.1e-5
(layer-by-layer forward), 1.9e-5 (one launch), on the ladder 9.8e-6 and 5.1e-6; float32 torch 1.8e-5 and 3.2e-5.
c. additivity <= 1.4e-5 (bar 5e-5; 8x8 1100 + 1100), Frobenius ratio <= 1.21 (bar 5; 2049 + 2049 on the ladder, xnet.w1_t),
ungated tensors <= 7.8e-6 (bar 1e-4); forward bits identical between batch and shards in every case; splits 18 (1100) and
32 - 33 (2049), column-sum chunks 34 and 64.  The file runs in 6 s, no test over 0.9 s.  More in
profiles/periodic_scale.txt."""
import time

import numpy as np
import pytest
import torch

from tests import periodic_ref as PR
from tests import periodic_scale_cases as S
from tests.test_gpu_periodic import _dev, _hip
from tests.test_gpu_periodic_train import _draws, _torch_ref, _train_forward, _trainer
from tests.test_gpu_periodic_train_forward import FLAGGED, _rows, _train_fused, _trajectory
from tests.test_gpu_train import TOL_G, _compare, _packed_ref, _ref_grads
from tests.test_gpu_train_batch import (C_ADD, FLOOR_ADD, FLOOR_F, GATED, K_F, TOL_U, UNGATED, _additivity, _colsum_chunks,
                                        _gauge_call, _segments, _threads, _tn_splits)

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- a. the taped launch at scale ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ladder", [False, True])
@pytest.mark.parametrize("N,rows", [(10, 18), (2, None)])
def test_taped_launch_has_the_bits_of_the_untaped_kernel_at_scale(N, rows, ladder):
    R = rows or S.TRAJ_ROWS_PER_CU * _cus() + S.TRAJ_ROWS_EXTRA
    B = R // 2                                          # a ladder of B rungs: rows i and B + i run at betas[i]
    eps = 0.1 if N == 10 else 0.2
    taped, _, _ = _hip(8, 8, N, eps, 8, "mild", **FLAGGED)
    taped_rc, _, _ = _hip(8, 8, N, eps, 8, "mild", recompute=True, **FLAGGED)
    plain, _, _ = _hip(8, 8, N, eps, 8, "mild", whole_step=True)
    assert _train_fused(taped) == 1 and _train_fused(taped_rc) == 1
    x0, v0, dirs = _rows(8, 8, R, 500 + N)
    assert 0 < int(dirs.sum()) < R
    names = ("x", "v", "sumlogdet", "p")
    if not ladder:
        want = _trajectory(plain, x0, v0, dirs, 2.5)
        kw = dict(beta=2.5)
    else:
        rungs = (1.5, 2.5, 3.5)
        betas = _dev(np.array([rungs[i % 3] for i in range(B)]))
        per_rung = {b: _trajectory(plain, x0, v0, dirs, b) for b in rungs}
        rung_of_row = torch.as_tensor([i % 3 for i in range(B)] * 2, device="cuda")
        every = torch.arange(R, device="cuda")
        want = tuple(torch.stack([per_rung[b][i] for b in rungs])[rung_of_row, every] for i in range(4))
        kw = dict(betas=betas)
    assert bool(torch.isfinite(want[0]).all()) and float(want[2].abs().mean()) > 1e-3
    for name, dyn in (("taped", taped), ("taped, recompute", taped_rc)):
        got = _train_forward(dyn, x0, v0, dirs, **kw)
        for k, a, b in zip(names, got, want):
            assert torch.equal(a, b), (name, N, R, ladder, k, float((a - b).abs().max()))
    print(f"[periodic train scale] taped launch N={N} rows={R} ladder={ladder}: x, v, sumlogdet, p bit equal to the "
          f"untaped kernel, recompute too")


# ---- b. gradients at benchmark length ------------------------------------------------------------------------------
N10 = (8, 8, 10, 0.1, 9, "mild")
SEEDS = {False: 362, True: 384}                        # one beta / the ladder: found on the CPU (module docstring)
FLIP_MARGIN = 5e-6
_REF = {}


def _beta(ladder, B):
    return np.linspace(1.5, 3.5, B).astype(np.float32) if ladder else 2.5


def _n10_reference(ladder):
    """float64 autograd of the N = 10 case (computed once per beta form), with the condition on float32 torch."""
    if ladder not in _REF:
        T, X, N, eps, B, regime = N10
        x, z, dx, dz = _draws(T, X, B, SEEDS[ladder])
        beta = _beta(ladder, B)
        tm = _torch_ref(T, X, N, eps, regime)
        b64 = torch.tensor(beta, dtype=torch.float64) if ladder else beta
        with _threads(16):
            want_loss, want_terms = _ref_grads(tm, x, z, dx, dz, b64, 'cos_diff')
            xp, vp = PR.periodic_weights(T, X, regime=regime)
            t32 = PR.TorchPeriodic(T, X, N, eps, PR.masks_for(N, 2 * T * X), xp, vp, dtype=torch.float32)
            f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)   # noqa: E731
            l32, _ = t32.loss(f32(x), f32(z), f32(beta) if ladder else beta, tuple(map(f32, dx)), tuple(map(f32, dz)))
            l32.backward()
        assert tm.flip_free(FLIP_MARGIN), (tm.min_preact, tm.min_clamp)
        worst = 0.0
        for n64, n32 in ((tm.xnet, t32.xnet), (tm.vnet, t32.vnet)):
            r64, r32 = _packed_ref(n64), _packed_ref(n32)
            worst = max([worst] + [float(np.abs(r32[k] - w).max() / np.abs(w).max()) for k, w in r64.items()])
        worst = max(worst, abs(float(t32.eps.grad) - float(tm.eps.grad)) / abs(float(tm.eps.grad)))
        print(f"[periodic train scale] N=10 ladder={ladder}: float32 torch autograd within {worst:.2e} of float64 "
              f"(bar TOL_G / 4 = {TOL_G / 4:.1e}); min |preact| {tm.min_preact:.2e} min |clamp| {tm.min_clamp:.2e}")
        assert worst <= TOL_G / 4
        _REF[ladder] = (tm, want_loss, want_terms, (x, z, dx, dz))
    return _REF[ladder]


@pytest.mark.parametrize("ladder", [False, True])
@pytest.mark.parametrize("fused_forward", [False, True])
def test_gradients_at_benchmark_length_match_autograd(fused_forward, ladder):
    from l2hmc_amd import _lib
    T, X, N, eps, B, regime = N10
    tm, want_loss, want_terms, (x, z, dx, dz) = _n10_reference(ladder)
    tr, *_ = _trainer(T, X, N, eps, B, regime, SEEDS[ladder], **(dict(fused_forward=True) if fused_forward else {}))
    assert tr.dynamics._plan().flags & _lib.PLAN_PERIODIC_TRAIN and _train_fused(tr.dynamics) == int(fused_forward)
    loss, _, _, _ = tr.calc_loss_and_grads(x, _beta(ladder, B), z=z, draws_x=dx, draws_z=dz)
    assert tr._walk is None
    np.testing.assert_allclose(tr.last_loss_terms.cpu().numpy(), want_terms, rtol=2e-4,
                               atol=1e-5 * max(1., np.abs(want_terms).max()))
    assert abs(float(loss) - want_loss) <= 2e-4 * max(1., abs(want_loss))
    worst = _compare(tr, tm)                            # every tensor within TOL_G of its maximum
    print(f"[periodic train scale] gradients N=10 fused_forward={fused_forward} ladder={ladder}: worst "
          f"{max(worst.values()):.3e} ({max(worst, key=worst.get)}) / {TOL_G:.0e}")


# ---- c. gradients where the reductions split -----------------------------------------------------------------------
def _regime(D, B, N=1):
    """Every weight-gradient product of both networks (fan-in Kin = 3 D) has at least two split-k parts whose last
    non-empty part is ragged, and the column sums at least two chunks; the shards have one of each."""
    Hn, Kin, Rt = 4 * D, 3 * D, 4 * B * N               # 2 calls per network and step x (x and z chains)
    prods = {"w1": _tn_splits(Hn, Kin, Rt), "wh": _tn_splits(Hn, Hn, Rt), "whd": _tn_splits(3 * D, Hn, Rt)}
    for k, (s, chunk) in prods.items():
        parts = -(-Rt // chunk)
        assert s >= 2 and 2 <= parts <= s and Rt % chunk, (k, s, chunk, Rt)
    S_, per = _colsum_chunks(Rt)
    assert S_ >= 2 and -(-Rt // per) >= 2, (S_, per)
    return prods, S_


def _f64_check(tr, tm, t32, x, z, dx, dz, beta, loss):
    """tests/test_gpu_train_batch.py::_f64_check for a periodic model (TorchPeriodic in float32 as the yardstick)."""
    b64 = torch.tensor(beta, dtype=torch.float64) if np.ndim(beta) else beta
    want_loss, _ = _ref_grads(tm, x, z, dx, dz, b64, 'cos_diff')
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)   # noqa: E731
    l32, _ = t32.loss(f32(x), f32(z), f32(beta) if np.ndim(beta) else beta, tuple(map(f32, dx)), tuple(map(f32, dz)))
    l32.backward()
    gv = tr.grad_views()
    ratios, bad = {"loss": abs(loss - want_loss) / max(1., abs(want_loss))}, []
    for name, net, n32 in (("xnet", tm.xnet, t32.xnet), ("vnet", tm.vnet, t32.vnet)):
        ref64, ref32 = _packed_ref(net), _packed_ref(n32)
        for k, w in ref64.items():
            got = gv[name][k].cpu().numpy().astype(np.float64).reshape(w.shape)
            if k in UNGATED:
                ratios[f"{name}.{k}"] = float(np.abs(got - w).max() / np.abs(w).max())
            else:
                assert k in GATED, k
                yard = max(np.linalg.norm(ref32[k] - w), FLOOR_F * np.linalg.norm(w))
                ratios[f"{name}.{k}/F"] = float(np.linalg.norm(got - w) / yard)
    ratios["eps"] = abs(float(gv["eps"][0]) - float(tm.eps.grad)) / abs(float(tm.eps.grad))
    for k, r in ratios.items():
        if not r <= (K_F if k.endswith("/F") else TOL_U):
            bad.append(k)
    assert not bad, f"float64 autograd: {[(k, f'{ratios[k]:.2e}') for k in bad]}\nall: {ratios}"
    return ratios


# Draw seeds (generator layout of tests/test_gpu_periodic_train.py::_draws).  A single relu flip moves one row of a first
# layer's gradient by about 1e-3 of the tensor's norm at these batches, ten times FLOOR_F: with seed 7 at 1100 + 1100 chains
# the float64 reference has a VNet pre-activation at -3.6e-7 (row 324, unit 483), which the tiled entries, the one-launch
# forward AND the layered walk put on the other side of 0 and float32 torch does not: unit 483 carries 1.000 of the
# squared error of vnet.w1_t, 1.1e-3 of its norm against float32 torch's 1.1e-5 (ratio 11.1 to K_F = 5; every other
# tensor <= 0.06).  Arithmetic, not a defect of a reduction.  The 8x8 cases at 1100 + 1100 therefore take the seed with
# the largest float64 min |pre-activation| of 348 scanned on the CPU (seed 156: 6.0e-7); none reaches 1e-6, so the
# figure is printed, not asserted.
SEED_DEFAULT, SEED_8x8_1100 = 7, 156
SHARD = 32                                             # 128 taped rows: one split-k part, one column-sum chunk
# (T, X, chains per half or None for 8 CUS + 1, one-launch forward, ladder)
SPLIT_CASES = [
    (8, 8, 1100, False, False), (8, 8, 1100, True, False),
    (8, 8, None, False, False), (8, 8, None, True, False),
    (8, 8, None, True, True),
    (4, 4, 1100, False, False),                         # D = 32, Kin = 96: tiled only (the one-launch forward is D = 128)
]


@pytest.mark.parametrize("T,X,B,fused_forward,ladder", SPLIT_CASES)
def test_gradients_where_the_reductions_split(T, X, B, fused_forward, ladder):
    B = B or 8 * _cus() + 1
    D, N, eps, regime = 2 * T * X, 1, 0.1, "mild"
    prods, chunks = _regime(D, B)
    seed = SEED_8x8_1100 if (D, B) == (128, 1100) else SEED_DEFAULT
    s1, c1 = _tn_splits(4 * D, 3 * D, 4 * SHARD)
    assert s1 == 1 and _colsum_chunks(4 * SHARD)[0] == 1, (s1, c1)
    tr, tm, x, z, dx, dz = _trainer(T, X, N, eps, B, regime, seed, **(dict(fused_forward=True) if fused_forward else {}))
    assert _train_fused(tr.dynamics) == int(fused_forward)
    if ladder:
        rungs = np.array([1.5, 2.5, 3.5], dtype=np.float32)
        beta = rungs[np.arange(B) % 3]
    else:
        beta = 2.0
    cutb = (lambda a, b: beta[a:b]) if ladder else (lambda a, b: beta)

    def call(xs, zs, dxs, dzs):
        # the shard's own rungs: located by the first chain's place in the batch
        if ladder and xs.shape[0] != B:
            a = int(np.flatnonzero((x == xs[0]).all(axis=1))[0])
            return _gauge_call(tr, xs, zs, dxs, dzs, cutb(a, a + xs.shape[0]))
        return _gauge_call(tr, xs, zs, dxs, dzs, beta)
    t0 = time.perf_counter()
    worst, nshards = _additivity(call, _segments(tr), B, SHARD, x, z, dx, dz)      # checks 1 and 3
    assert tr._walk is None
    t1 = time.perf_counter()
    loss, *_ = _gauge_call(tr, x, z, dx, dz, beta)
    xp, vp = PR.periodic_weights(T, X, regime=regime)
    t32 = PR.TorchPeriodic(T, X, N, eps, PR.masks_for(N, D), xp, vp, dtype=torch.float32)
    with _threads(16):
        ratios = _f64_check(tr, tm, t32, x, z, dx, dz, beta, loss)                # check 2
    t2 = time.perf_counter()
    fro = {k: v for k, v in ratios.items() if k.endswith("/F")}
    ung = {k: v for k, v in ratios.items() if not k.endswith("/F")}
    print(f"[periodic train scale] {T}x{X} B={B}+{B} fused_forward={fused_forward} ladder={ladder}: splits {prods} "
          f"colsum chunks {chunks}; additivity {worst:.2e} / {C_ADD:.0e} over {nshards} shards (floor {FLOOR_ADD:.0e}); "
          f"Frobenius worst {max(fro.values()):.2f} ({max(fro, key=fro.get)}) / {K_F}; ungated worst "
          f"{max(ung.values()):.2e} ({max(ung, key=ung.get)}) / {TOL_U:.0e}; float64 min |pre-activation| "
          f"{tm.min_preact:.2e}; {t1 - t0:.1f} s + {t2 - t1:.1f} s")
