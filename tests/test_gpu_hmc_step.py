"""Plain HMC (`GaugeDynamics(hmc=True)`) in one launch at any lattice shape (l2hmc_amd/csrc/hmc_step.hip).

The yardstick is the float64 NumPy oracle (`tests/helpers.gauge_oracle(..., hmc=True)`) at the project's own
tolerances (tests/test_gpu_parity.py: TOL_OP = 1e-5, TOL_P = 2e-5); the layer-by-layer path (`fused=False`,
L2HMC_PLAN_LAYERED), which is what every plain-HMC step ran before the kernel existed, is the cross-check."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lattice as olat
from tests import helpers as H
from tests.run_cases import count_launches

pytestmark = pytest.mark.gpu

TOL_OP = 1e-5
TOL_P = 2e-5
MAX_RATIO, Q999_RATIO, RMS_RATIO = 5.0, 2.5, 1.6      # tests/test_gpu_parity.py: allowances over the fp32 oracle's own error


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def rmserr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2)) / max(1.0, np.max(np.abs(want))))


def assert_fp32_equivalent(got, want64, want32, what):
    """`got` is as close to the fp64 oracle as an fp32 evaluation in the reference's op order
    (tests/test_gpu_parity.py::assert_fp32_equivalent, restated)."""
    emax, imax = H.relerr(got, want64), H.relerr(want32, want64)
    erms, irms = rmserr(got, want64), rmserr(want32, want64)
    print(f"{what}: max {emax:.3e} (fp32 oracle {imax:.3e}), rms {erms:.3e} (fp32 oracle {irms:.3e})")
    assert emax < max(TOL_OP, MAX_RATIO * imax), f"{what}: max err {emax:.2e} vs intrinsic fp32 {imax:.2e}"
    assert erms < max(TOL_OP / 3, RMS_RATIO * irms), f"{what}: rms err {erms:.2e} vs intrinsic fp32 {irms:.2e}"
    if np.size(want64) >= 4000:
        scale = max(1.0, np.max(np.abs(want64)))
        eq = np.quantile(np.abs(np.asarray(got, dtype=np.float64) - want64), 0.999) / scale
        iq = np.quantile(np.abs(np.asarray(want32, dtype=np.float64) - want64), 0.999) / scale
        assert eq < max(TOL_OP / 2, Q999_RATIO * iq), f"{what}: 99.9 % quantile {eq:.2e} vs intrinsic fp32 {iq:.2e}"


def circle(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    d = np.mod(d, 2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _pair(T, X, N, eps, B, fused=True, both=True, dtype=np.float64):
    orc = H.gauge_oracle(T, X, N, eps, None, None, hmc=True, dtype=dtype)
    dyn = H.gauge_hip(T, X, N, eps, None, None, orc.mask, B, hmc=True, both_directions=both)
    dyn.fused = fused
    return orc, dyn


def _plan_fused(dyn):
    from l2hmc_amd import _lib
    plan = dyn._plan()
    return _lib.lib().l2hmc_gauge_plan_fused(C.byref(plan))


# ----------------------------------------------------------------- 1. the step on its own draws
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("T,X,B", [(8, 8, 70), (4, 4, 9), (6, 6, 33), (3, 5, 1), (4, 16, 257), (16, 16, 5), (32, 32, 3)])
def test_hmc_step_matches_oracle_on_its_own_draws(la, T, X, B, both):
    """l2hmc_gauge_mcmc_step with hmc = 1 (draws + trajectories + mix / MH + observables + wrap in ONE launch).  Its
    Philox streams are reproducible through l2hmc_fill_*, so the oracle is fed the very same draws.  Chains whose
    accept decision sits within 1e-4 of the uniform are left out of the x_next / |dQ| comparison; that is a
    condition on the committed (seed, draw), asserted: none where B < 64, at most 2 % elsewhere."""
    from l2hmc_amd import _lib
    N, eps, beta, D = 3, 0.1, 2.0, 2 * T * X
    orc, dyn = _pair(T, X, N, eps, B, both=both)
    assert _plan_fused(dyn) == 1
    x0 = np.random.default_rng(3).uniform(0, 2 * np.pi, (B, D)).astype(np.float32)
    x = torch.as_tensor(x0, device="cuda").clone()
    outs = [torch.empty(B, device="cuda") for _ in range(5)]
    plan, Lh = dyn._plan(), _lib.lib()
    ws, nb = dyn._ws.get(Lh.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B), x.device)
    seed, draw = 77, 5
    _lib.check(Lh.l2hmc_gauge_mcmc_step(C.byref(plan), beta, x.data_ptr(), B, seed, draw, *[o.data_ptr() for o in outs],
                                         ws, nb, _lib.stream_ptr()))
    V = torch.empty(2 * B, D, device="cuda")
    cu = torch.empty(2 * B, device="cuda")
    _lib.check(Lh.l2hmc_fill_normal(V.data_ptr(), V.numel(), seed, 2 * draw, None))
    _lib.check(Lh.l2hmc_fill_uniform(cu.data_ptr(), cu.numel(), seed, 2 * draw + 1, None))
    V, cu = np_(V), np_(cu)
    x64 = x0.astype(np.float64)
    want = orc.apply_transition(x64, beta, V[:B], V[B:], cu[:B], cu[B:])
    px, actions, plaqs, charges, dq = [np_(o) for o in outs]
    safe = np.abs(want[2] - cu[B:]) > 1e-4
    xw = np.mod(want[3], 2 * np.pi)
    got = np_(x)
    figs = dict(px=np.abs(px - want[2]).max(), action=H.relerr(actions, olat.total_action(x64, T, X)),
                plaq=H.relerr(plaqs, olat.avg_plaq(x64, T, X)), charge=H.relerr(charges, olat.top_charge(x64, T, X)),
                dq=H.relerr(dq[safe], olat.top_charge_diff(x64, want[3], T, X)[safe]),
                x_next=circle(got, xw)[safe].max() if safe.any() else 0.0, excluded=int((~safe).sum()),
                accepted=int((want[2] > cu[B:]).sum()))
    print(f"hmc step {T}x{X} B={B} both={both}: {figs}")
    assert (~safe).sum() <= (0 if B < 64 else 0.02 * B)
    assert figs["px"] < TOL_P
    assert figs["action"] < TOL_OP and figs["plaq"] < TOL_OP and figs["charge"] < 1e-4
    assert figs["dq"] < 1e-3
    assert figs["x_next"] < 5e-5
    assert got.min() >= 0 and got.max() <= 2 * np.pi


# ----------------------------------------------------------------- 2. trajectory mode
@pytest.mark.parametrize("T,X", [(8, 8), (6, 6), (32, 32)])
def test_hmc_trajectory_and_single_steps_match_oracle(la, T, X):
    """transition_kernel forward / backward and `_lf` single steps at the parameters of
    test_hmc_mode_is_plain_leapfrog; backward after forward with the returned momentum gives x back."""
    N, eps, beta, B, D = 5, 0.05, 2.0, 20, 2 * T * X
    orc, dyn = _pair(T, X, N, eps, B)
    assert _plan_fused(dyn) == 1
    x, v0f, v0b, coin, u = H.gauge_inputs(B, D)
    for forward, v0 in ((True, v0f), (False, v0b)):
        xo, vo, p, sld = dyn.transition_kernel(x, beta, forward=forward, momentum=v0, return_logdet=True)
        want = orc.transition_kernel(x, beta, v0, forward=forward)
        errs = (H.relerr(np_(xo), want[0]), H.relerr(np_(vo), want[1]), np.abs(np_(p) - want[2]).max())
        print(f"hmc trajectory {T}x{X} forward={forward}: x {errs[0]:.3e} v {errs[1]:.3e} p {errs[2]:.3e}")
        assert errs[0] < TOL_OP and errs[1] < TOL_OP and errs[2] < TOL_P
        assert torch.all(sld == 0)
    for step in (0, 2, N - 1):
        for fn, ofn in ((dyn._forward_lf, orc._forward_lf), (dyn._backward_lf, orc._backward_lf)):
            x1, v1, ld = fn(x, v0f, beta, step)
            ox, ov, _ = ofn(np.asarray(x, dtype=np.float64), np.asarray(v0f, dtype=np.float64), beta, step)
            assert H.relerr(np_(x1), ox) < TOL_OP and H.relerr(np_(v1), ov) < TOL_OP, (step, fn.__name__)
            assert torch.all(ld == 0)
    xf, vf, _ = dyn.transition_kernel(x, beta, forward=True, momentum=v0f)
    xb, vb, _ = dyn.transition_kernel(xf, beta, forward=False, momentum=vf)
    back = circle(np_(xb), x).max()
    print(f"hmc trajectory {T}x{X}: backward o forward misses x by {back:.3e}")
    assert back < TOL_OP and H.relerr(np_(vb), v0f) < TOL_OP


def test_hmc_long_trajectory_at_32x32_is_fp32_equivalent(la):
    T = X = 32
    N, eps, beta, B, D = 25, 0.08, 2.0, 12, 2 * T * X
    orc, dyn = _pair(T, X, N, eps, B)
    orc32 = H.gauge_oracle(T, X, N, eps, None, None, hmc=True, dtype=np.float32)
    x, v0f, _, _, _ = H.gauge_inputs(B, D)
    x, v0f = x.astype(np.float32), v0f.astype(np.float32)
    xo, vo, p = dyn.transition_kernel(x, beta, forward=True, momentum=v0f)
    w64 = orc.transition_kernel(x.astype(np.float64), beta, v0f.astype(np.float64), forward=True)
    w32 = orc32.transition_kernel(x, beta, v0f, forward=True)
    assert_fp32_equivalent(np_(xo), w64[0], w32[0], "x after 25 steps")
    assert_fp32_equivalent(np_(vo), w64[1], w32[1], "v after 25 steps")


# ----------------------------------------------------------------- 3. the new path against the layered one
def _compare_paths(T, X, B, both, masks=None):
    """One step from the same state, seed and draw counter through GaugeSampler.step, dyn(x, beta) and
    apply_transition with injected draws, fused=True against fused=False.  Both paths are held to TOL against float64
    above, so twice TOL is the triangle inequality."""
    import l2hmc_amd as la
    N, eps, beta, D = 4, 0.12, 2.0, 2 * T * X
    _, new = _pair(T, X, N, eps, B, fused=True, both=both)
    _, old = _pair(T, X, N, eps, B, fused=False, both=both)
    if masks is not None:
        new.set_masks(masks)
        old.set_masks(masks)
    assert _plan_fused(new) == 1 and _plan_fused(old) == 0
    x = torch.as_tensor(np.random.default_rng(11).uniform(0, 2 * np.pi, (B, D)).astype(np.float32), device="cuda")
    few = 0 if B < 64 else 0.02 * B

    # dyn(x, beta): the library's own draws
    new._draws = old._draws = 6
    a, b = new(x, beta), old(x, beta)
    assert new._draws == old._draws
    u = torch.empty(2 * B, device="cuda")
    from l2hmc_amd import _lib
    _lib.check(_lib.lib().l2hmc_fill_uniform(u.data_ptr(), u.numel(), new._seed, 2 * 3 + 1, None))
    u = np_(u)[B:]
    dx, dv, dp = H.relerr(np_(a[0]), np_(b[0])), H.relerr(np_(a[1]), np_(b[1])), np.abs(np_(a[2]) - np_(b[2])).max()
    print(f"paths {T}x{X} B={B} both={both}: x_prop {dx:.3e} v_prop {dv:.3e} p {dp:.3e}")
    assert dx < 2 * TOL_OP and dv < 2 * TOL_OP and dp < 2 * TOL_P
    clear = np.abs(np_(b[2]) - u) > 2 * TOL_P
    assert (~clear).sum() <= few
    acc_a, acc_b = np_(a[2]) > u, np_(b[2]) > u
    assert np.array_equal(acc_a[clear], acc_b[clear])
    if clear.any():
        assert circle(np_(a[3]), np_(b[3]))[clear].max() < 5e-5

    # GaugeSampler.step
    new._draws = old._draws = 6
    sn, so = la.GaugeSampler(new), la.GaugeSampler(old)
    xn, pxn, obn, dqn = sn.step(x, beta)
    xo, pxo, obo, dqo = so.step(x, beta)
    assert np.abs(np_(pxn) - np_(pxo)).max() < 2 * TOL_P
    assert np.array_equal((np_(pxn) > u)[clear], (np_(pxo) > u)[clear])
    if clear.any():
        assert circle(np_(xn), np_(xo))[clear].max() < 5e-5
    for key in ("action", "avg_plaq"):
        assert H.relerr(np_(obn[key]), np_(obo[key])) < 2 * TOL_OP
    assert H.relerr(np_(obn["top_charge"]), np_(obo["top_charge"])) < 2e-4
    sums_n = np_(sn._sums_ring[0][:3])
    sums_o = np_(so._sums_ring[0][:3])
    assert sums_n[2] == B and sums_o[2] == B
    assert abs(sums_n[0] - np_(pxn).sum()) <= 1e-5 * max(1.0, abs(sums_n[0]))
    if np.array_equal(np_(pxn) > u, np_(pxo) > u):                   # no decision differs
        assert np.all(np.abs(sums_n - sums_o) <= 1e-5 * np.maximum(1.0, np.abs(sums_o))), (sums_n, sums_o)

    # apply_transition with injected draws: the composition around the trajectory launch
    _, v0f, v0b, coin, uu = H.gauge_inputs(B, D)
    a = new.apply_transition(x, beta, momentum_f=v0f, momentum_b=v0b, coin=coin, u=uu)
    b = old.apply_transition(x, beta, momentum_f=v0f, momentum_b=v0b, coin=coin, u=uu)
    assert H.relerr(np_(a[0]), np_(b[0])) < 2 * TOL_OP and H.relerr(np_(a[1]), np_(b[1])) < 2 * TOL_OP
    assert np.abs(np_(a[2]) - np_(b[2])).max() < 2 * TOL_P
    clear = np.abs(np_(b[2]) - uu) > 2 * TOL_P
    assert (~clear).sum() <= few
    if clear.any():
        assert circle(np_(a[3]), np_(b[3]))[clear].max() < 5e-5


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("B", [1, 9, 70, 2048, 4097])
@pytest.mark.parametrize("T,X", [(8, 8), (6, 6)])
def test_hmc_kernel_matches_layered_path(la, T, X, B, both):
    _compare_paths(T, X, B, both)


def test_hmc_kernel_matches_layered_path_with_fractional_masks(la):
    T, X, N = 6, 6, 4
    rng = np.random.default_rng(5)
    masks = rng.integers(0, 2, (N, 2 * T * X)).astype(np.float32)
    masks[1] = np.where(masks[1] > 0, 0.75, 0.25)        # a fractional row: k x + (1 - k) (x +- eps v) on every link
    _compare_paths(T, X, 70, True, masks=masks)


# ----------------------------------------------------------------- 4. one launch
@pytest.mark.parametrize("T,X", [(8, 8), (6, 6), (32, 32)])
def test_hmc_step_is_one_launch(la, T, X):
    N, B = 10, 64
    _, new = _pair(T, X, N, 0.1, B)
    _, old = _pair(T, X, N, 0.1, B, fused=False)
    x = torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)
    sn, so = la.GaugeSampler(new), la.GaugeSampler(old)
    sn.step(x, 2.0)
    so.step(x, 2.0)
    assert count_launches(5, lambda: sn.step(x, 2.0)) == 1
    assert count_launches(4, lambda: sn.step(x, 2.0)) == 0
    assert count_launches(5, lambda: so.step(x, 2.0)) == 0
    assert count_launches(4, lambda: so.step(x, 2.0)) > 2 * N


# ----------------------------------------------------------------- 5. determinism and capture
@pytest.mark.parametrize("T,X,B", [(8, 8, 300), (32, 32, 5), (3, 5, 40)])
def test_hmc_step_is_deterministic_and_graph_capturable(la, T, X, B):
    from l2hmc_amd import _lib
    N, D = 6, 2 * T * X
    _, dyn = _pair(T, X, N, 0.1, B)
    smp = la.GaugeSampler(dyn)
    x0 = torch.rand(B, D, device="cuda") * (2 * np.pi)
    dyn._draws = 4
    a = smp.step(x0, 2.0)
    dyn._draws = 4
    b = smp.step(x0, 2.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k])

    plan, L = dyn._plan(), _lib.lib()
    nb = L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    outs = [torch.empty(B, device="cuda") for _ in range(5)]

    def step(x):
        _lib.check(L.l2hmc_gauge_mcmc_step(C.byref(plan), 2.0, x.data_ptr(), B, 42, 7, *(o.data_ptr() for o in outs),
                                           ws.data_ptr(), nb, _lib.stream_ptr()))
    eager = x0.clone()
    step(eager)
    torch.cuda.synchronize()
    want_px = outs[0].clone()
    xg = x0.clone()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(xg)
    torch.cuda.current_stream().wait_stream(side)
    xg.copy_(x0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(xg, eager) and torch.equal(outs[0], want_px)
    assert float(xg.min()) >= 0.0 and float(xg.max()) <= 2 * np.pi
