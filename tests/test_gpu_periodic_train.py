"""Torus-exact training on the tiled entries (`GaugeDynamics(periodic=True, tiled_train=True)`,
L2HMC_PLAN_PERIODIC_TRAIN) on the device, against the float64 reference of tests/periodic_ref.py.

Gradients: float64 autograd of the same loss, per tensor at 2e-4 of the tensor's max (the rule of
tests/test_gpu_train.py), on draws for which the float64 reference has no relu pre-activation within 1e-5 of 0 and no
accept exponent within 1e-5 of its clamp (`TorchPeriodic.flip_free`; the seeds were found on the CPU, generator layout
of tests/test_gpu_periodic.py::_trainer).  `tr._walk is None` is what fails without the feature: there `tiled_train`
is silently set as an attribute and the layered walk trains.

The taped forward is compared under the yardstick rule of tests/test_gpu_periodic.py: the error of the float32 NumPy
reference against the float64 one on the same inputs, gate 4 yardsticks, positions by angular distance.

Measured on the MI355X.  Gradients, worst tensor as error / max: 4x4 6.7e-6, 2x8 7.2e-6, 8x2 (stress) 1.6e-6, 4x8 1.3e-5,
8x8 7.9e-6; on the ladder 1.6e-4 (d/d eps, a sum of terms of both signs; the walk on the same draws: 8.0e-5, d/d eps
too); the walk on the first case 9.4e-6, 6x6 with the flag 7.6e-6; autograd 1.1e-5 on one beta, 2.1e-6 on the ladder.  Taped
forward, worst error / yardstick (gate 4): 4x4 1.77 (forward rows, sumlogdet: 1.2e-6 against 6.7e-7), 8x8 3.18 (backward
rows, sumlogdet: 6.1e-6 against 1.9e-6); x, v and p between 0.43 and 1.17."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import periodic_ref as PR
from tests import workspace_cases as W
from tests.test_gpu_autograd import _compare_to_oracle, _draw_kw, _rel, _requires_grad, _t64
from tests.test_gpu_periodic import _dev, _gate, _hip, _np, _yard
from tests.test_gpu_train import TOL_G, _compare, _ref_grads

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi


def _draws(T, X, B, seed):
    """x, z and the two transitions' draws: the generator layout of tests/test_gpu_periodic.py::_trainer."""
    D = 2 * T * X
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, TWO_PI, (B, D))
    z = rng.standard_normal((B, D))
    dx = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    dz = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    return x, z, dx, dz


def _torch_ref(T, X, N, eps, regime):
    xp, vp = PR.periodic_weights(T, X, regime=regime)
    return PR.TorchPeriodic(T, X, N, eps, PR.masks_for(N, 2 * T * X), xp, vp)


def _trainer(T, X, N, eps, B, regime, seed, tiled_train=True, **kw):
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    dyn, _, _ = _hip(T, X, N, eps, B, regime, **(dict(tiled_train=True) if tiled_train else {}), **kw)
    tr = GaugeTrainer(dyn, metric='cos_diff', lr_init=1e-3)
    return (tr, _torch_ref(T, X, N, eps, regime), *_draws(T, X, B, seed))


def _check_step(tr, tm, x, z, dx, dz, beta, name):
    """One calc_loss_and_grads against float64 autograd: loss, terms, every gradient tensor."""
    loss, _, _, _ = tr.calc_loss_and_grads(x, beta, z=z, draws_x=dx, draws_z=dz)
    b64 = torch.tensor(np.asarray(beta), dtype=torch.float64) if np.ndim(beta) else beta
    want_loss, want_terms = _ref_grads(tm, x, z, dx, dz, b64, 'cos_diff')
    assert tm.flip_free(), (tm.min_preact, tm.min_clamp)
    np.testing.assert_allclose(tr.last_loss_terms.cpu().numpy(), want_terms, rtol=2e-4,
                               atol=1e-5 * max(1., np.abs(want_terms).max()))
    assert abs(float(loss) - want_loss) <= 2e-4 * max(1., abs(want_loss))
    worst = _compare(tr, tm)
    print(f"[periodic train] {name}: worst {max(worst.values()):.3e} ({max(worst, key=worst.get)}) "
          f"min |preact| {tm.min_preact:.2e} min |clamp| {tm.min_clamp:.2e}")
    return worst


# ---- 1. gradients --------------------------------------------------------------------------------------------------
# (T, X, N_LF, eps, B, regime, flip-free seed)
GRAD_CASES = [
    (4, 4, 2, 0.2, 37, "mild", 2),       # 74 rows: partial 4-, 16- and 64-row blocks; 296 taped rows: two split-k parts
    (2, 8, 3, 0.2, 6, "mild", 1),        # T != X at D = 32, Kin = 96
    (8, 2, 2, 0.2, 9, "stress", 2),      # ... the other way, strong S / Q
    (4, 8, 2, 0.2, 5, "mild", 1),        # D = 64, Kin = 192
    (8, 8, 2, 0.2, 9, "mild", 2),        # D = 128: where the reference mode takes the fused kernels and this mode must not
]


@pytest.mark.parametrize("T,X,N,eps,B,regime,seed", GRAD_CASES)
def test_tiled_periodic_training_gradients_match_autograd(T, X, N, eps, B, regime, seed):
    tr, tm, x, z, dx, dz = _trainer(T, X, N, eps, B, regime, seed)
    from l2hmc_amd import _lib
    assert tr.dynamics._plan().flags & _lib.PLAN_PERIODIC_TRAIN
    _check_step(tr, tm, x, z, dx, dz, 2.5, f"gradients {T}x{X}")
    assert tr._walk is None                      # the tiled entries: no layered walk was built


# ---- 2. ladders ----------------------------------------------------------------------------------------------------
def test_tiled_periodic_training_on_a_ladder_of_betas():
    T, X, N, eps, B, regime, _ = GRAD_CASES[0]
    tr, tm, x, z, dx, dz = _trainer(T, X, N, eps, B, regime, 2)
    betas = np.linspace(1.5, 3.5, B).astype(np.float32)
    _check_step(tr, tm, x, z, dx, dz, betas, "ladder gradients")
    assert tr._walk is None
    # a ladder of equal betas is the scalar step, bit for bit
    tr.calc_loss_and_grads(x, np.full(B, 2.5, dtype=np.float32), z=z, draws_x=dx, draws_z=dz)
    g_ladder, terms_ladder = tr.grads.clone(), tr.last_loss_terms.clone()
    tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    assert torch.equal(tr.grads, g_ladder) and torch.equal(tr.last_loss_terms, terms_ladder)
    assert tr._walk is None


def _train_forward(dyn, x0, v0, dirs, beta=None, betas=None):
    """l2hmc_gauge_train_forward[_ladder] on R stacked rows -> (xN, vN, sumlogdet, p)."""
    from l2hmc_amd import _lib
    R = x0.shape[0]
    plan = dyn._plan()
    nb = int(_lib.lib().l2hmc_gauge_train_ws_bytes(C.byref(plan), R))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    xN, vN = torch.empty_like(x0), torch.empty_like(x0)
    sld, p = (torch.empty(R, dtype=torch.float32, device="cuda") for _ in range(2))
    if betas is None:
        _lib.call("l2hmc_gauge_train_forward", C.byref(plan), float(beta), x0, v0, dirs, R, xN, vN, sld, p, ws, nb,
                  device=x0.device)
    else:
        _lib.call("l2hmc_gauge_train_forward_ladder", C.byref(plan), betas, 1, betas.numel(), x0, v0, dirs, R, xN, vN,
                  sld, p, ws, nb, device=x0.device)
    return xN, vN, sld, p


def test_forward_ladder_rows_have_the_bits_of_the_scalar_entry():
    T, X, N, eps, B, regime, _ = GRAD_CASES[0]
    dyn, _, _ = _hip(T, X, N, eps, B, regime, tiled_train=True)
    rng = np.random.default_rng(3)
    R, D = 2 * B, 2 * T * X
    x0, v0 = _dev(rng.uniform(0, TWO_PI, (R, D))), _dev(rng.standard_normal((R, D)))
    dirs = torch.as_tensor(rng.integers(0, 2, R).astype(np.int32), device="cuda")
    betas = _dev(np.linspace(1.5, 3.5, B))
    lad = _train_forward(dyn, x0, v0, dirs, betas=betas)
    for i in range(B):                           # rows i and B + i ran at betas[i]
        one = _train_forward(dyn, x0, v0, dirs, beta=float(betas[i]))
        for a, b in zip(lad, one):
            assert torch.equal(a[i], b[i]) and torch.equal(a[B + i], b[B + i]), i


# ---- 3. the taped forward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,X,N,eps,B,regime", [(4, 4, 3, 0.2, 37, "stress"), (8, 8, 2, 0.1, 9, "mild")])
def test_taped_forward_matches_float64(T, X, N, eps, B, regime):
    dyn, r64, r32 = _hip(T, X, N, eps, B, regime, tiled_train=True)
    x, v0f, v0b, _, _ = H.gauge_inputs(B, 2 * T * X, seed=103 + T)
    x, v0f, v0b = (np.asarray(a, dtype=np.float32) for a in (x, v0f, v0b))
    beta = 2.5
    # B rows forward, then B rows backward, in one call
    dirs = torch.cat([torch.zeros(B, dtype=torch.int32), torch.ones(B, dtype=torch.int32)]).cuda()
    got = _train_forward(dyn, _dev(np.concatenate([x, x])), _dev(np.concatenate([v0f, v0b])), dirs, beta=beta)
    names = ("x", "v", "sumlogdet", "p")
    for bwd, v0, sl in ((False, v0f, slice(0, B)), (True, v0b, slice(B, 2 * B))):
        f64, f32 = ({k: v for k, v in zip(("x", "v", "p", "sumlogdet"), r.trajectory(x, v0, beta, bwd))}
                    for r in (r64, r32))
        assert np.abs(f64["sumlogdet"]).mean() > 1e-3
        worst = _gate(f"taped forward {T}x{X} {regime} bwd={bwd}", {k: _np(g[sl]) for k, g in zip(names, got)}, f64,
                      _yard(f32, f64, angular=("x",)), angular=("x",))
        print(f"[periodic train] taped forward {T}x{X} bwd={bwd}: worst ratio {worst:.2f}")


# ---- 4. cross-check and refusals -----------------------------------------------------------------------------------
def test_the_layered_walk_stays_as_cross_check_and_carries_other_lattices():
    T, X, N, eps, B, regime, seed = GRAD_CASES[0]
    tr, tm, x, z, dx, dz = _trainer(T, X, N, eps, B, regime, seed)
    tr.layered = True
    _check_step(tr, tm, x, z, dx, dz, 2.5, "layered = True")
    assert tr._walk is not None
    # 6x6: the flag is carried, the walk trains
    tr6, tm6, *args = _trainer(6, 6, 2, 0.2, 9, "mild", 7)
    assert tr6.dynamics.tiled_train is True
    _check_step(tr6, tm6, *args, 2.5, "6x6 with the flag")
    assert tr6._walk is not None
    tr6.layered = False
    with pytest.raises(NotImplementedError, match="72"):
        tr6.calc_loss_and_grads(args[0], 2.5, z=args[1], draws_x=args[2], draws_z=args[3])
    # an unflagged periodic trainer still walks
    tru, _, x, z, dx, dz = _trainer(4, 4, 2, 0.2, 6, "mild", 2, tiled_train=False)
    tru.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    assert tru._walk is not None


# ---- 5. workspace contract -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,X,B", [(4, 4, 37), (8, 8, 9)])
def test_gradients_do_not_depend_on_what_the_workspace_held(T, X, B, monkeypatch):
    tr, _, x, z, dx, dz = _trainer(T, X, 2, 0.2, B, "mild", 2)
    got = []
    for pattern in (0x00, 0xFF):
        with W.poisoned(monkeypatch, pattern) as shared:
            out = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
            assert shared.gets >= 1
        got.append((tr.grads.clone(), tr.last_loss_terms.clone(), out[0].clone()))
    for _ in range(2):                           # and on two calls in a row, on the trainer's own workspace
        out = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
        got.append((tr.grads.clone(), tr.last_loss_terms.clone(), out[0].clone()))
    assert tr._walk is None and bool(torch.isfinite(got[0][0]).all())
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert torch.equal(a, b)


# ---- 6. the public loop --------------------------------------------------------------------------------------------
def _loop_trainer(seed, eps=0.2, **kw):
    from l2hmc_amd import GaugeLattice, GaugeDynamics
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    np.random.seed(seed)
    lat = GaugeLattice(4, 4, 2, 'U1', num_samples=16, rand=True)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=eps, num_steps=3, eps_trainable=True, periodic=True,
                        tiled_train=True, seed=seed, **kw)
    return GaugeTrainer(dyn, lr_init=1e-3)


def test_public_training_loop_moves_every_weight_and_resumes_bit_for_bit(tmp_path):
    B = 16
    tr = _loop_trainer(5)
    before = {(i, k): v.detach().clone() for i, n in enumerate(tr._nets) for k, v in n.flat_params()[1].items()}
    eps0 = float(tr.dynamics.eps)
    x = _dev(np.random.default_rng(1).uniform(0, TWO_PI, (B, 32)))
    for _ in range(3):
        loss, x_out, px, _ = tr.train_step(x, 2.0)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(px).all())
    b0, b1 = np.tile(np.linspace(1.0, 2.5, 4), 4), np.tile(np.linspace(2.0, 4.0, 4), 4)
    out = tr.train(3, samples_init=x, beta_init=b0, beta_final=b1, replicas=4, swap_every=1)
    assert tr._walk is None and tr.global_step == 6
    for k in ("loss", "accept_prob", "eps"):
        assert np.isfinite(out[k]).all(), k
    assert out["swapped"].shape == (3, B) and out["beta"].shape == (3, B)
    for (i, k), w0 in before.items():
        assert not torch.equal(tr._nets[i].flat_params()[1][k], w0), (i, k)
    assert float(tr.dynamics.eps) != eps0
    # save -> load into a fresh flagged trainer: the next step's gradients, bit for bit, with injected draws
    path = str(tmp_path / "state.npz")
    xs = out["samples"]
    tr.save_state(path, samples=xs, beta=b1)
    _, z, dx, dz = _draws(4, 4, B, 9)
    tr.calc_loss_and_grads(xs, b1.astype(np.float32), z=z, draws_x=dx, draws_z=dz)
    tr2 = _loop_trainer(11, eps=0.3, whole_step=True)      # other weights, masks and eps: load_state restores them all
    extra = tr2.load_state(path)
    tr2.calc_loss_and_grads(torch.as_tensor(extra["samples"], device="cuda"), extra["beta"].astype(np.float32), z=z,
                            draws_x=dx, draws_z=dz)
    assert tr2._walk is None
    assert torch.equal(tr.grads, tr2.grads) and torch.equal(tr.last_loss_terms, tr2.last_loss_terms)


# ---- 7. torch.autograd ---------------------------------------------------------------------------------------------
AG = (4, 4, 2, 0.2, 6, "mild", 4)                # flip-free for beta 2.5 and for the ladder, with p < 1 and p = 1 chains


def _autograd_case(beta, tiled_train=True):
    T, X, N, eps, B, regime, seed = AG
    dyn, _, _ = _hip(T, X, N, eps, B, regime, **(dict(tiled_train=True) if tiled_train else {}))
    x, _, dx, _ = _draws(T, X, B, seed)
    rng = np.random.default_rng(17)
    c = [rng.standard_normal((B, 2 * T * X)), rng.standard_normal((B, 2 * T * X)), rng.standard_normal(B)]
    _requires_grad(dyn)
    xg = torch.tensor(x, dtype=torch.float32, device="cuda", requires_grad=True)
    bdev = _dev(beta) if np.ndim(beta) else beta
    outs = dyn(xg, bdev, **_draw_kw(dx))
    loss = sum((_dev(ci) * o).sum() for ci, o in zip(c, outs[:3]))        # reads x_prop, v_prop and p_accept
    return dyn, xg, loss, outs, (x, dx, c)


@pytest.mark.parametrize("ladder", [False, True])
def test_autograd_through_a_flagged_periodic_dynamics_matches_float64(ladder):
    T, X, N, eps, B, regime, _ = AG
    beta = np.linspace(1.5, 3.5, B).astype(np.float32) if ladder else 2.5
    dyn, xg, loss, outs, (x, dx, c) = _autograd_case(beta)
    assert loss.grad_fn is not None
    loss.backward()
    tm = _torch_ref(T, X, N, eps, regime)
    x64 = _t64(x).requires_grad_()
    want = tm.apply_transition(x64, _t64(beta) if ladder else beta, *map(_t64, dx))
    assert tm.flip_free(), (tm.min_preact, tm.min_clamp)
    p = want[2].detach().numpy()
    assert (p < 1).any() and (p == 1).any()
    sum((_t64(ci) * o).sum() for ci, o in zip(c, want[:3])).backward()
    worst = _compare_to_oracle(dyn, tm)
    worst["x"] = _rel(xg.grad, x64.grad)
    assert worst["x"] <= TOL_G, worst
    print(f"[periodic train] autograd ladder={ladder}: worst {max(worst.values()):.3e} ({max(worst, key=worst.get)})")
    # the call without a graph is the sampling path's, flag or not: same bits as an unflagged dynamics
    plain, _, _ = _hip(T, X, N, eps, B, regime)
    bdev = _dev(beta) if ladder else beta
    with torch.no_grad():
        a = dyn(_dev(x), bdev, **_draw_kw(dx))
        b = plain(_dev(x), bdev, **_draw_kw(dx))
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_autograd_on_a_ladder_of_equal_betas_is_the_scalar_call_and_the_unflagged_mode_is_refused():
    B = AG[4]
    dyn_s, xs, loss_s, _, _ = _autograd_case(2.5)
    loss_s.backward()
    dyn_l, xl, loss_l, _, _ = _autograd_case(np.full(B, 2.5, dtype=np.float32))
    loss_l.backward()
    assert torch.equal(loss_s.detach(), loss_l.detach()) and torch.equal(xs.grad, xl.grad)
    assert torch.equal(dyn_s.eps.grad, dyn_l.eps.grad)
    for ns, nl in ((dyn_s.position_fn, dyn_l.position_fn), (dyn_s.momentum_fn, dyn_l.momentum_fn)):
        for (k, a), b in zip(ns.state_dict().items(), nl.state_dict().values()):
            assert torch.equal(a.grad, b.grad), k
    with pytest.raises(NotImplementedError, match="periodic=True"):
        _autograd_case(2.5, tiled_train=False)
