"""Every exact sampling path leaves its target invariant.

The parity tests feed the float64 oracle the kernels' own draws and compare outputs, so an error that the oracle
shares (the accept rule, the log-det sign, the direction mix, how the momenta or the MH uniform are used, tempering,
the wrap) passes them.  These tests use the target itself as the reference.  B chains start as exact float64 draws
of the target (tests/invariance.py), cast to fp32; K MCMC steps go through the library.  If a step leaves the
target invariant, every chain is still an exact, independent sample after each step, so at checkpoints k = 1, 4, 16
    z_jk = (mean over chains of f_j(x_k) - E f_j) / (sd_k(f_j) / sqrt(B))
is N(0, 1) for every test function f_j: no burn-in, no autocorrelation.  A case passes with max |z| < 5; seeds are
fixed, so a build gives the same z every run.

The test functions: toy targets -- first and second moments and half-space indicators P(w^T x > c), the bisectors
between modes among them (a chain that gains or loses mass between modes moves them); 2-D U(1) -- the average
plaquette, the action, its square and Q^2, against the finite-volume values of the character expansion.

Power controls: a reference MH step is built in torch (float64 Hamiltonian) from the library's trajectories
(`Dynamics.both(..., log_jac=True)`, `GaugeDynamics.transition_kernel(..., return_logdet=True)`).  Its correct form
must pass the same bar, and each deliberate defect must reach max |z| > 8.  The force is deliberately not among the
defects: Metropolis-Hastings corrects a wrong force exactly, so these tests cannot see one -- the parity tests own
the force, and nothing here is a force test.

L2HMC mode on the lattice is out of scope: under reference quirk Q10 it is not reversible on the torus.
HMC mode is: leapfrog with a periodic force commutes with 2 pi shifts, so wrapping keeps it exact.

Measured on the MI355X (max |z| over all checkpoints and test functions; the whole file runs in about 50 s):
  one-launch (first-layer forms 1 and 2 alike):  scg 2.68, scg_T3 2.68, mog 1.80, gmm3 2.26;  0.4-0.9 s per case.
  piecewise, NumPy draws:  scg 2.71, scg_T3 2.70, mog 2.13, gmm3 1.89;  1.4-1.8 s.
  layered:  gmm12 2.75 (library draws) / 2.54 (NumPy draws), mog_wide 1.35, callable 3.08;  <= 2.5 s.
  HMC toys:  scg 1.99, scg_T3 2.24 (accept 0.96 / 0.99).
  toy reference step:  correct 2.66 (scg) / 2.48 (mog);  defects, scg / mog:  log-det dropped 74 / 94, sign
      flipped 136 / 201, coin reused as u 219 / 226, forward only 1469 / 1326.
  U(1) HMC, max over the four paths:  2x4 1.33, 4x16 2.86, 6x6 1.04, 8x8 1.44, 32x32 2.04;  <= 1.7 s per case.
  U(1) reference step (8x8):  correct 2.25;  always accept 50, initial kinetic at both ends 381;  coin reused as
      u 1.39 (not detected, and not asserted on).
  With `+ logdet` dropped from the accept probability of l2hmc_small_propose (csrc/small_mlp.hip), every one-launch
  case fails: scg 72, scg_T3 86, mog 92, gmm3 26."""
import time

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import invariance as I

pytestmark = pytest.mark.gpu

CHECKPOINTS = (1, 4, 16)
Z_PASS, Z_DEFECT = 5.0, 8.0
LOGDET_FLOOR = 0.05                  # mean |sumlogdet| of a trajectory: the nets really act
ACCEPT_RANGE = (0.2, 0.95)


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    return l2hmc_amd


def _report(name, zs, extra=""):
    zs = np.asarray(zs)
    k, j = np.unravel_index(np.argmax(np.abs(zs)), zs.shape)
    print(f"\n[invariance] {name}: max|z| = {np.abs(zs).max():.2f} (checkpoint {CHECKPOINTS[k]}, f{j}) {extra}")
    return float(np.abs(zs).max())


# ------------------------------------------------------------------------------------------------ toy targets
GMM3 = ([np.array([1., 0., 0.5]), np.array([0., 1., -0.5]), np.array([-1., -1., 0.])],
        [np.diag([0.05, 0.08, 0.1]), 0.07 * np.eye(3) + 0.02, np.diag([0.1, 0.05, 0.06])], [0.3, 0.5, 0.2])
SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])

# kind: (x_dim, trajectory length, eps, hidden units, chains)
TOYS = {
    "scg": (2, 5, 0.1, 32, 1 << 20),
    "scg_T3": (2, 5, 0.1, 32, 1 << 20),
    "mog": (2, 10, 0.1, 32, 1 << 20),
    "gmm3": (3, 5, 0.1, 32, 1 << 20),
    "gmm12": (12, 4, 0.1, 100, 1 << 16),     # x_dim > MAX_SMALL_DIM: a torch callable, layer by layer
    "mog_wide": (2, 5, 0.1, 96, 1 << 20),    # more than 64 hidden units: layer by layer on the packed target
    "callable": (2, 5, 0.1, 32, 1 << 20),    # a Gaussian energy as a lambda: autograd gradient, layer by layer
}


def _toy(la, kind, hmc=False, eps=None):
    """-> (dyn, ExactGMM of exp(-E/T), B).  Stress-regime nets (helpers.mlp_weights)."""
    from oracle import dynamics as od
    dim, N, eps0, nodes, B = TOYS[kind]
    eps = eps0 if eps is None else eps
    temperature = 3.0 if kind.endswith("_T3") else 1.0
    if kind.startswith("scg"):
        fn = la.Gaussian(np.zeros(2), SCG_SIGMA).get_energy_function()
        ex = I.ExactGMM.of_library_gaussian(np.zeros(2), SCG_SIGMA, temperature=temperature)
    elif kind.startswith("mog"):
        m = H.mog_target_oracle()
        fn = la.GMM(m.mus, m.sigmas, m.pis).get_energy_function()
        ex = I.ExactGMM.of_library_gmm(m.mus, m.sigmas, m.pis)
    elif kind == "gmm3":
        fn = la.GMM(*GMM3).get_energy_function()
        ex = I.ExactGMM.of_library_gmm(*GMM3)
    elif kind == "gmm12":
        rng = np.random.default_rng(12)
        mus = np.stack([rng.normal(0, 1.0, dim) for _ in range(3)]).astype(np.float32)
        precs = np.stack([np.diag(1. / rng.uniform(0.3, 0.8, dim)) for _ in range(3)]).astype(np.float32)
        lcs = np.log(np.array([0.5, 0.3, 0.2])).astype(np.float32)
        mu_t, prec_t, lc_t = (torch.tensor(a, device="cuda") for a in (mus, precs, lcs))

        def fn(x):
            d = x[:, None, :] - mu_t[None]
            return -torch.logsumexp(lc_t[None] - 0.5 * torch.einsum("bkd,kde,bke->bk", d, prec_t, d), dim=1)
        ex = I.ExactGMM.from_energy(mus, precs, lcs)
    else:
        mu = np.array([0.5, -0.3], dtype=np.float32)
        P = np.array([[2.0, 0.8], [0.8, 1.0]], dtype=np.float32)
        mu_t, P_t = torch.tensor(mu, device="cuda"), torch.tensor(P, device="cuda")
        fn = lambda x: 0.5 * (((x - mu_t) @ P_t) * (x - mu_t)).sum(dim=1)      # noqa: E731
        ex = I.ExactGMM.from_energy(mu[None], P[None])
    xp, vp = H.mlp_weights(dim, nodes, seed=106, regime="stress")
    dyn = la.Dynamics(dim, fn, trajectory_length=N, eps=eps, hmc=hmc,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes),
                      use_temperature=True, seed=7)
    dyn.temperature = temperature
    dyn.set_masks(od.make_masks(N, dim, np.random.RandomState(3)))
    if not hmc:
        dyn.XNet.load_state(xp)
        dyn.VNet.load_state(vp)
    return dyn, ex, B


def _run_toy(ex, B, step, seed=1):
    """Exact start, K = 16 steps of `step(x, k) -> (x, px)`; -> (z [checkpoints, J], accept rate of step 1)."""
    W, c = ex.halfspaces(np.random.default_rng(5))
    want = ex.expectations(W, c)
    x = torch.as_tensor(ex.sample(B, np.random.default_rng(seed)), dtype=torch.float32, device="cuda")
    zs, acc = [], None
    for k in range(1, max(CHECKPOINTS) + 1):
        x, px = step(x, k)
        if acc is None:
            acc = float(px.double().mean())
        if k in CHECKPOINTS:
            zs.append(I.zscores(ex.features(x.double().cpu().numpy(), W, c), want))
    return np.array(zs), acc


def _check_strength(dyn, ex, B):
    """The nets really act: mean |sumlogdet| of both directions above the floor."""
    x = torch.as_tensor(ex.sample(min(B, 1 << 16), np.random.default_rng(9)), dtype=torch.float32, device="cuda")
    (_, _, ljf), (_, _, ljb) = dyn.both(x, log_jac=True)
    ld = 0.5 * float(ljf.abs().mean() + ljb.abs().mean())
    assert ld > LOGDET_FLOOR, ld
    return ld


def _library_step(la, dyn, inject, seed=2):
    rng = np.random.default_rng(seed)

    def step(x, k):
        if not inject:
            _, _, px, (out,) = la.propose(x, dyn, do_mh_step=True)
            return out, px
        B, d = x.shape
        vf, vb = rng.standard_normal((B, d)), rng.standard_normal((B, d))
        bits = (rng.uniform(size=B) >= 0.5).astype(np.float32)
        _, _, px, (out,) = la.propose(x, dyn, init_v=vf, init_v_backward=vb, dir_bits=bits, u=rng.uniform(size=B),
                                      do_mh_step=True)
        return out, px
    return step


ONE_LAUNCH = [(kind, form) for kind in ("scg", "scg_T3", "mog", "gmm3") for form in (1, 2)]


@pytest.mark.parametrize("kind,form", ONE_LAUNCH)
def test_one_launch_propose_leaves_the_target_invariant(la, kind, form):
    """l2hmc_small_propose: direction coin, both momenta, both trajectories and MH in one kernel, library draws."""
    t0 = time.time()
    dyn, ex, B = _toy(la, kind)
    assert not dyn.layered
    dyn.first_layer_form = form
    ld = _check_strength(dyn, ex, B)
    zs, acc = _run_toy(ex, B, _library_step(la, dyn, inject=False))
    m = _report(f"one-launch {kind} form {form}", zs, f"accept {acc:.3f} |logdet| {ld:.3f} {time.time() - t0:.1f} s")
    assert ACCEPT_RANGE[0] < acc < ACCEPT_RANGE[1], acc
    assert m < Z_PASS, zs


@pytest.mark.parametrize("kind", ["scg", "scg_T3", "mog", "gmm3"])
def test_piecewise_propose_with_injected_draws_leaves_the_target_invariant(la, kind):
    """Dynamics.both + l2hmc_mix_accept on momenta, direction bits and MH uniforms from NumPy (not Philox)."""
    t0 = time.time()
    dyn, ex, B = _toy(la, kind)
    ld = _check_strength(dyn, ex, B)
    zs, acc = _run_toy(ex, B, _library_step(la, dyn, inject=True))
    m = _report(f"piecewise {kind}", zs, f"accept {acc:.3f} |logdet| {ld:.3f} {time.time() - t0:.1f} s")
    assert ACCEPT_RANGE[0] < acc < ACCEPT_RANGE[1], acc
    assert m < Z_PASS, zs


@pytest.mark.parametrize("kind,inject", [("gmm12", False), ("gmm12", True), ("mog_wide", False), ("callable", False)])
def test_layered_propose_leaves_the_target_invariant(la, kind, inject):
    """l2hmc_stq_dense + l2hmc_lf_update_v / _x per sub-update, l2hmc_accept_prob, l2hmc_mix_accept: a 12-D GMM as a
    torch callable, a 2-D packed target with 96 hidden units, a Gaussian energy as a lambda (autograd gradient)."""
    t0 = time.time()
    dyn, ex, B = _toy(la, kind)
    assert dyn.layered
    ld = _check_strength(dyn, ex, B)
    zs, acc = _run_toy(ex, B, _library_step(la, dyn, inject=inject))
    m = _report(f"layered {kind} inject={inject}", zs, f"accept {acc:.3f} |logdet| {ld:.3f} {time.time() - t0:.1f} s")
    assert ACCEPT_RANGE[0] < acc < ACCEPT_RANGE[1], acc
    assert m < Z_PASS, zs


@pytest.mark.parametrize("kind", ["scg", "scg_T3"])
def test_hmc_propose_leaves_the_target_invariant(la, kind):
    """hmc=True: forward leapfrog and tf_accept, library draws; tempered: N(0, T Sigma)."""
    t0 = time.time()
    dyn, ex, B = _toy(la, kind, hmc=True, eps=0.25)
    zs, acc = _run_toy(ex, B, _library_step(la, dyn, inject=False))
    m = _report(f"hmc {kind}", zs, f"accept {acc:.3f} {time.time() - t0:.1f} s")
    assert 0.2 < acc < 0.999, acc
    assert m < Z_PASS, zs


TOY_DEFECTS = [None, "no_logdet", "logdet_sign", "coin_as_u", "forward_only"]


def _reference_toy_step(dyn, ex, defect, seed=3):
    """One MH step from the library's trajectories (Dynamics.both, log_jac=True), H in float64."""
    rng = np.random.default_rng(seed)

    def step(x, k):
        B, d = x.shape
        vf = torch.as_tensor(rng.standard_normal((B, d)), dtype=torch.float32, device="cuda")
        vb = torch.as_tensor(rng.standard_normal((B, d)), dtype=torch.float32, device="cuda")
        coin = torch.as_tensor(rng.uniform(size=B), device="cuda")
        u = torch.as_tensor(rng.uniform(size=B), device="cuda")
        (Xf, Vf, ljf), (Xb, Vb, ljb) = dyn.both(x, vf, vb, log_jac=True)
        e0 = ex.energy(x.double())

        def p_acc(X, V, v0, lj):
            lj = lj.double()
            if defect == "no_logdet":
                lj = lj * 0
            elif defect == "logdet_sign":
                lj = -lj
            dH = e0 + 0.5 * (v0.double() ** 2).sum(1) - ex.energy(X.double()) - 0.5 * (V.double() ** 2).sum(1) + lj
            return torch.exp(torch.clamp(dH, max=0.0)).nan_to_num(0.0)
        fwd = coin >= 0.5
        if defect == "forward_only":
            fwd = torch.ones_like(fwd)
        if defect == "coin_as_u":
            u = coin
        p = torch.where(fwd, p_acc(Xf, Vf, vf, ljf), p_acc(Xb, Vb, vb, ljb))
        Xp = torch.where(fwd[:, None], Xf, Xb)
        return torch.where((p - u >= 0)[:, None], Xp, x), p
    return step


@pytest.mark.parametrize("kind", ["scg", "mog"])
@pytest.mark.parametrize("defect", TOY_DEFECTS)
def test_toy_power_controls(la, kind, defect):
    """The reference step passes; each defect is detected at the same B, K, seeds and nets."""
    t0 = time.time()
    dyn, ex, B = _toy(la, kind)
    ld = _check_strength(dyn, ex, B)
    zs, acc = _run_toy(ex, B, _reference_toy_step(dyn, ex, defect))
    m = _report(f"reference toy step {kind} defect={defect}", zs,
                f"accept {acc:.3f} |logdet| {ld:.3f} {time.time() - t0:.1f} s")
    if defect is None:
        assert ACCEPT_RANGE[0] < acc < ACCEPT_RANGE[1], acc
        assert m < Z_PASS, zs
    else:
        assert m > Z_DEFECT, zs


# ----------------------------------------------------------------------------------------------------- U(1)
# (T, X, beta, chains, num_steps, eps)
LATTICES = {
    "2x4": (2, 4, 1.0, 1 << 18, 5, 0.5),        # finite volume matters: <cos> 0.44889 against I1/I0 = 0.44639
    "4x16": (4, 16, 1.5, 1 << 15, 6, 0.2),      # not square
    "6x6": (6, 6, 3.0, 1 << 15, 6, 0.15),       # D = 72, not a multiple of 32
    "8x8": (8, 8, 2.0, 1 << 14, 6, 0.2),
    "32x32": (32, 32, 4.0, 1 << 11, 10, 0.08),  # the cfg-5 lattice
}
_U1_START = {}


def _u1_start(name):
    T, X, beta, B = LATTICES[name][:4]
    if name not in _U1_START:
        _U1_START[name] = (I.u1_samples(B, T, X, beta, np.random.default_rng(17)), I.u1_exact_vector(T, X, beta))
    return _U1_START[name]


def _action64(x, T, X):
    """float64 torch, as oracle/lattice.py: (action, average plaquette, real-valued charge) of x [B, 2TX]."""
    s = x.double().reshape(-1, T, X, 2)
    x0, x1 = s[..., 0], s[..., 1]
    P = x0 - x1 - torch.roll(x0, -1, dims=2) + torch.roll(x1, -1, dims=1)
    cs = torch.cos(P).sum(dim=(1, 2))
    proj = P - 2 * np.pi * torch.floor((P + np.pi) / (2 * np.pi))
    return T * X - cs, cs / (T * X), proj.sum(dim=(1, 2)) / (2 * np.pi)


def _u1_dyn(la, name, both_directions=True, seed=5):
    T, X, beta, B, N, eps = LATTICES[name]
    lat = la.GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    return la.GaugeDynamics(lat, lat.get_energy_function(), eps=eps, hmc=True, num_steps=N, eps_trainable=False,
                            network_arch='generic', both_directions=both_directions, seed=seed)


def _run_u1(name, step):
    T, X, beta = LATTICES[name][:3]
    x0, want = _u1_start(name)
    x = torch.as_tensor(x0, dtype=torch.float32, device="cuda")
    zs, acc = [], None
    for k in range(1, max(CHECKPOINTS) + 1):
        x, px = step(x, k)
        if acc is None:
            acc = float(px.double().mean())
        if k in CHECKPOINTS:
            a, p, q = _action64(x, T, X)
            zs.append(I.zscores(I.u1_features(p.cpu().numpy(), a.cpu().numpy(), q.cpu().numpy()), want))
    assert float(x.min()) >= 0 and float(x.max()) <= 2 * np.pi     # the chain state stays wrapped
    return np.array(zs), acc


U1_PATHS = ["sampler_step", "call_and_wrap", "injected_draws", "selected_only"]


@pytest.mark.parametrize("path", U1_PATHS)
@pytest.mark.parametrize("name", list(LATTICES))
def test_u1_hmc_leaves_the_finite_volume_distribution_invariant(la, name, path):
    """GaugeDynamics(hmc=True): GaugeSampler.step (l2hmc_gauge_mcmc_step_ex), dyn(x, beta) and the wrap,
    apply_transition on NumPy draws, and both_directions = False through GaugeSampler.step."""
    t0 = time.time()
    T, X, beta = LATTICES[name][:3]
    dyn = _u1_dyn(la, name, both_directions=(path != "selected_only"))
    sampler = la.GaugeSampler(dyn)
    rng = np.random.default_rng(23)

    def step(x, k):
        if path in ("sampler_step", "selected_only"):
            x_next, px, _, _ = sampler.step(x, beta)
            return x_next, px
        if path == "call_and_wrap":
            _, _, px, x_out = dyn(x, beta)
        else:
            B, D = x.shape
            _, _, px, x_out = dyn.apply_transition(x, beta, momentum_f=rng.standard_normal((B, D)),
                                                   momentum_b=rng.standard_normal((B, D)),
                                                   coin=rng.uniform(size=B), u=rng.uniform(size=B))
        return sampler.wrap(x_out), px
    zs, acc = _run_u1(name, step)
    m = _report(f"U(1) HMC {name} {path}", zs, f"accept {acc:.3f} {time.time() - t0:.1f} s")
    assert 0.3 < acc < 0.995, acc
    assert m < Z_PASS, zs


U1_DEFECTS = [None, "always_accept", "initial_kinetic_both_ends", "coin_as_u"]


@pytest.mark.parametrize("defect", U1_DEFECTS)
def test_u1_power_controls(la, defect):
    """Reference HMC step from dyn.transition_kernel(..., return_logdet=True) at 8 x 8, H in float64.  The coin
    reused as the MH uniform is not asserted on: in HMC mode the two directions are mirror images (v -> -v), so it
    biases nothing to first order; its |z| is recorded in the module docstring."""
    t0 = time.time()
    name = "8x8"
    T, X, beta = LATTICES[name][:3]
    dyn = _u1_dyn(la, name)
    sampler = la.GaugeSampler(dyn)
    rng = np.random.default_rng(29)

    def h64(x, v):
        return beta * _action64(x, T, X)[0] + 0.5 * (v.double() ** 2).sum(1)

    def step(x, k):
        B, D = x.shape
        vf = torch.as_tensor(rng.standard_normal((B, D)), dtype=torch.float32, device="cuda")
        vb = torch.as_tensor(rng.standard_normal((B, D)), dtype=torch.float32, device="cuda")
        coin = torch.as_tensor(rng.uniform(size=B), device="cuda")
        u = torch.as_tensor(rng.uniform(size=B), device="cuda")
        xf, wf, _, sf = dyn.transition_kernel(x, beta, forward=True, momentum=vf, return_logdet=True)
        xb, wb, _, sb = dyn.transition_kernel(x, beta, forward=False, momentum=vb, return_logdet=True)
        fwd = coin >= 0.5
        v0, v1 = torch.where(fwd[:, None], vf, vb), torch.where(fwd[:, None], wf, wb)
        x1, sld = torch.where(fwd[:, None], xf, xb), torch.where(fwd, sf, sb).double()
        if defect == "initial_kinetic_both_ends":
            v1 = v0
        p = torch.exp(torch.clamp(h64(x, v0) - h64(x1, v1) + sld, max=0.0)).nan_to_num(0.0)
        if defect == "always_accept":
            p = torch.ones_like(p)
        if defect == "coin_as_u":
            u = coin
        return torch.where((p - u >= 0)[:, None], sampler.wrap(x1), x), p
    zs, acc = _run_u1(name, step)
    m = _report(f"U(1) reference HMC step defect={defect}", zs, f"accept {acc:.3f} {time.time() - t0:.1f} s")
    if defect is None:
        assert m < Z_PASS, zs
    elif defect != "coin_as_u":
        assert m > Z_DEFECT, zs
