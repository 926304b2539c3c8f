"""The one-launch training forward of the torus-exact mode (`GaugeDynamics(periodic=True, tiled_train=True,
fused_forward=True)`, L2HMC_PLAN_PERIODIC_TAPE) on the device: the taped instances of the mode's whole-trajectory kernel
(csrc/fused_traj_ncp.hip) under `l2hmc_gauge_train_forward[_ladder]`, the tiled reverse pass on the tape they write.

All at D = 128 / H = 512, the only shape the kernel has, small in rows and N_LF.  What fails without the feature: the
launch counts (one class-5 launch, no first-layer launch) -- there `fused_forward` is silently set as an attribute and
the forward goes layer by layer.

Bits: the taped launch against `l2hmc_gauge_trajectory` of a `whole_step=True` dynamics on the same rows, torch.equal.
Forward against float64: the yardstick rule of tests/test_gpu_periodic.py (gate 4 yardsticks, x by angular distance).
Gradients: float64 autograd at TOL_G = 2e-4 of the tensor's max on flip-free draws (`TorchPeriodic.flip_free`; seeds
found on the CPU, generator layout of tests/test_gpu_periodic_train.py::_draws) -- the reverse pass reads `in`, `st`,
h1, h2 and the S / T / Q planes of every call, so a wrong tape array shows here.

Measured on the MI355X.  Taped forward, worst error / yardstick (gate 4): 8x8 stress 2.09 on the forward rows and 2.58
on the backward rows (both sumlogdet: 1.6e-6 against 7.8e-7, 1.5e-6 against 5.7e-7), 4x16 mild 2.18 (forward rows, p:
4.0e-6 against 1.8e-6) and 1.24 (backward rows, sumlogdet); x and v between 0.72 and 1.40.  Gradients, worst tensor as
error / max, in the order of GRAD_CASES: 1.4e-6, 2.2e-5, 9.6e-6, 1.6e-5, 1.2e-5, 1.7e-6; on the ladder 2.2e-5; the third
case on the layer-by-layer forward with the same draws: 1.6e-5 (one launch: 9.6e-6).  Autograd 1.5e-5 on one beta
(d/d eps), 2.6e-6 on the ladder."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import periodic_ref as PR
from tests import run_cases as RC
from tests import workspace_cases as W
from tests.test_gpu_autograd import _compare_to_oracle, _draw_kw, _rel, _requires_grad, _t64
from tests.test_gpu_periodic import _dev, _gate, _hip, _np, _yard
from tests.test_gpu_periodic_train import _check_step, _draws, _torch_ref, _train_forward, _trainer
from tests.test_gpu_train import TOL_G

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi
FLAGGED = dict(tiled_train=True, fused_forward=True)
LATTICES = [(8, 8), (4, 16), (16, 4)]


def _rows(T, X, R, seed):
    """R rows of x0, v0 and a direction drawn per row (tiles mix forward and backward rows)."""
    rng = np.random.default_rng(seed)
    D = 2 * T * X
    x0, v0 = _dev(rng.uniform(0, TWO_PI, (R, D))), _dev(rng.standard_normal((R, D)))
    dirs = torch.as_tensor(rng.integers(0, 2, R).astype(np.int32), device="cuda")
    return x0, v0, dirs


def _trajectory(dyn, x0, v0, dirs, beta):
    """l2hmc_gauge_trajectory -> (xN, vN, sumlogdet, p)."""
    from l2hmc_amd import _lib
    R = x0.shape[0]
    plan, L = dyn._plan(), _lib.lib()
    nb = int(L.l2hmc_gauge_ws_bytes(C.byref(plan), R))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    xN, vN = torch.empty_like(x0), torch.empty_like(x0)
    sld, p = (torch.empty(R, dtype=torch.float32, device="cuda") for _ in range(2))
    _lib.call("l2hmc_gauge_trajectory", C.byref(plan), float(beta), x0, v0, dirs, R, xN, vN, sld, p, ws, nb,
              device=x0.device)
    return xN, vN, sld, p


def _train_fused(dyn):
    from l2hmc_amd import _lib
    return _lib.lib().l2hmc_gauge_plan_train_fused(C.byref(dyn._plan()))


# ---- 1. launch count -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ladder", [False, True])
def test_flagged_forward_is_one_launch(ladder):
    T, X, N, B = 8, 8, 2, 9
    x0, v0, dirs = _rows(T, X, 2 * B, 1)
    kw = dict(betas=_dev(np.linspace(1.5, 3.5, B))) if ladder else dict(beta=2.5)
    dyn, _, _ = _hip(T, X, N, 0.2, B, "mild", **FLAGGED)
    assert _train_fused(dyn) == 1
    run = lambda: _train_forward(dyn, x0, v0, dirs, **kw)       # noqa: E731
    assert RC.count_launches(5, run) == 1
    assert RC.count_launches(1, run) == 0
    plain, _, _ = _hip(T, X, N, 0.2, B, "mild", tiled_train=True)
    assert _train_fused(plain) == 0
    assert RC.count_launches(5, lambda: _train_forward(plain, x0, v0, dirs, **kw)) == 0
    # the flag does not need whole_step, and LAYERED wins over it
    both, _, _ = _hip(T, X, N, 0.2, B, "mild", whole_step=True, **FLAGGED)
    assert RC.count_launches(5, lambda: _train_forward(both, x0, v0, dirs, **kw)) == 1
    walk, _, _ = _hip(T, X, N, 0.2, B, "mild", fused=False, **FLAGGED)
    assert _train_fused(walk) == 0
    assert RC.count_launches(5, lambda: _train_forward(walk, x0, v0, dirs, **kw)) == 0


@pytest.mark.parametrize("ladder", [False, True])
def test_trainer_forward_is_one_launch(ladder):
    T, X, N, B = 8, 8, 2, 9
    beta = np.linspace(1.5, 3.5, B).astype(np.float32) if ladder else 2.5
    tr, _, x, z, dx, dz = _trainer(T, X, N, 0.2, B, "mild", 2, fused_forward=True)
    step = lambda t: t.calc_loss_and_grads(x, beta, z=z, draws_x=dx, draws_z=dz)      # noqa: E731
    assert RC.count_launches(5, lambda: step(tr)) == 1
    assert tr._walk is None
    tru, *_ = _trainer(T, X, N, 0.2, B, "mild", 2)
    assert RC.count_launches(5, lambda: step(tru)) == 0
    # trainer.layered = True still forces the walk
    tr.layered = True
    assert RC.count_launches(5, lambda: step(tr)) == 0
    assert tr._walk is not None


# ---- 2. the bits of the untaped kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("T,X", LATTICES)
def test_taped_launch_has_the_bits_of_the_untaped_kernel(T, X, N):
    taped, _, _ = _hip(T, X, N, 0.2, 8, "stress", **FLAGGED)
    taped_rc, _, _ = _hip(T, X, N, 0.2, 8, "stress", recompute=True, **FLAGGED)
    plain, _, _ = _hip(T, X, N, 0.2, 8, "stress", whole_step=True)
    plain_rc, _, _ = _hip(T, X, N, 0.2, 8, "stress", whole_step=True, recompute=True)
    assert _train_fused(taped) == 1 and _train_fused(taped_rc) == 1
    for R in (1, 15, 16, 17, 74):      # a lone row, a ragged last workgroup, a full one, a one-row tail, five workgroups
        x0, v0, dirs = _rows(T, X, R, 100 * R + N)
        if R > 1:
            assert 0 < int(dirs.sum()) < R
        want = _trajectory(plain, x0, v0, dirs, 2.5)
        assert bool(torch.isfinite(want[0]).all()) and float(want[2].abs().mean()) > 1e-3
        for name, got in (("taped", _train_forward(taped, x0, v0, dirs, beta=2.5)),
                          ("taped, recompute", _train_forward(taped_rc, x0, v0, dirs, beta=2.5)),
                          ("untaped, recompute", _trajectory(plain_rc, x0, v0, dirs, 2.5))):
            for k, a, b in zip(("x", "v", "sumlogdet", "p"), got, want):
                assert torch.equal(a, b), (name, R, k, float((a - b).abs().max()))


# ---- 3. ladder -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [9, 17])
def test_forward_ladder_rows_have_the_bits_of_the_scalar_entry(B):
    T, X, N = 8, 8, 2
    dyn, _, _ = _hip(T, X, N, 0.2, B, "mild", **FLAGGED)
    x0, v0, dirs = _rows(T, X, 2 * B, 3)
    betas = _dev(np.linspace(1.5, 3.5, B))
    lad = _train_forward(dyn, x0, v0, dirs, betas=betas)
    assert RC.count_launches(5, lambda: _train_forward(dyn, x0, v0, dirs, betas=betas)) == 1
    for i in range(B):                           # rows i and B + i ran at betas[i]
        one = _train_forward(dyn, x0, v0, dirs, beta=float(betas[i]))
        for a, b in zip(lad, one):
            assert torch.equal(a[i], b[i]) and torch.equal(a[B + i], b[B + i]), i


def test_a_ladder_of_equal_betas_is_the_scalar_step():
    B = 9
    tr, _, x, z, dx, dz = _trainer(8, 8, 2, 0.2, B, "mild", 6, fused_forward=True)
    out_l = tr.calc_loss_and_grads(x, np.full(B, 2.5, dtype=np.float32), z=z, draws_x=dx, draws_z=dz)
    g_ladder, terms_ladder, loss_ladder = tr.grads.clone(), tr.last_loss_terms.clone(), out_l[0].clone()
    out_s = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    assert torch.equal(tr.grads, g_ladder) and torch.equal(tr.last_loss_terms, terms_ladder)
    assert torch.equal(out_s[0], loss_ladder) and tr._walk is None


# ---- 4. forward against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,X,N,eps,B,regime", [(8, 8, 3, 0.2, 37, "stress"), (4, 16, 2, 0.2, 9, "mild")])
def test_taped_forward_matches_float64(T, X, N, eps, B, regime):
    dyn, r64, r32 = _hip(T, X, N, eps, B, regime, **FLAGGED)
    assert _train_fused(dyn) == 1
    R = 2 * B
    x, v0f, v0b, _, _ = H.gauge_inputs(R, 2 * T * X, seed=211 + X)
    x, v0f, v0b = (np.asarray(a, dtype=np.float32) for a in (x, v0f, v0b))
    beta = 2.5
    bwd_rows = np.arange(R) % 2 == 1             # interleaved: every tile mixes the directions
    v0 = np.where(bwd_rows[:, None], v0b, v0f)
    got = _train_forward(dyn, _dev(x), _dev(v0), torch.as_tensor(bwd_rows.astype(np.int32), device="cuda"), beta=beta)
    names = ("x", "v", "sumlogdet", "p")
    for bwd, sel in ((False, ~bwd_rows), (True, bwd_rows)):
        f64, f32 = ({k: v for k, v in zip(("x", "v", "p", "sumlogdet"), r.trajectory(x[sel], v0[sel], beta, bwd))}
                    for r in (r64, r32))
        assert np.abs(f64["sumlogdet"]).mean() > 1e-3
        worst = _gate(f"one-launch taped forward {T}x{X} {regime} bwd={bwd}", {k: _np(g)[sel] for k, g in zip(names, got)},
                      f64, _yard(f32, f64, angular=("x",)), angular=("x",))
        print(f"[periodic train forward] taped forward {T}x{X} bwd={bwd}: worst ratio {worst:.2f}")


# ---- 5. gradients --------------------------------------------------------------------------------------------------
# (T, X, N_LF, eps, B, regime, flip-free seed)
GRAD_CASES = [
    (8, 8, 1, 0.2, 1, "mild", 2),        # 2 rows
    (8, 8, 2, 0.2, 8, "mild", 1),        # one exactly full tile
    (8, 8, 3, 0.2, 9, "mild", 10),       # 18 rows, two kept-VNet step boundaries, both zig parities
    (8, 8, 2, 0.2, 17, "mild", 3),       # 34 rows: three workgroups, two-row tail
    (4, 16, 2, 0.2, 5, "mild", 5),       # T != X
    (16, 4, 2, 0.2, 5, "stress", 4),     # T != X the other way
]


@pytest.mark.parametrize("T,X,N,eps,B,regime,seed", GRAD_CASES)
def test_gradients_on_the_one_launch_tape_match_autograd(T, X, N, eps, B, regime, seed):
    tr, tm, x, z, dx, dz = _trainer(T, X, N, eps, B, regime, seed, fused_forward=True)
    from l2hmc_amd import _lib
    assert tr.dynamics._plan().flags & _lib.PLAN_PERIODIC_TAPE and _train_fused(tr.dynamics) == 1
    worst = _check_step(tr, tm, x, z, dx, dz, 2.5, f"one-launch forward, gradients {T}x{X} N={N} B={B}")
    assert tr._walk is None
    if (N, B) == (3, 9):                         # for the record, not a gate: the layer-by-layer forward on the same draws
        tru, tmu, *_ = _trainer(T, X, N, eps, B, regime, seed)
        wu = _check_step(tru, tmu, x, z, dx, dz, 2.5, "layer-by-layer forward, same draws")
        print(f"[periodic train forward] 8x8 N=3 B=9 worst: one launch {max(worst.values()):.3e}, "
              f"layer by layer {max(wu.values()):.3e}")


def test_gradients_on_a_ladder_of_betas():
    T, X, N, eps, B, regime, seed = 8, 8, 2, 0.2, 9, "mild", 6
    tr, tm, x, z, dx, dz = _trainer(T, X, N, eps, B, regime, seed, fused_forward=True)
    _check_step(tr, tm, x, z, dx, dz, np.linspace(1.5, 3.5, B).astype(np.float32), "one-launch forward, ladder gradients")
    assert tr._walk is None


# ---- 6. torch.autograd ---------------------------------------------------------------------------------------------
AG = (8, 8, 2, 0.2, 8, "mild", 1)                # flip-free for beta 2.5 (min |preact| 2.2e-5, min |clamp| 0.59) and for
                                                 # the ladder (2.2e-5, 0.64), with p < 1 and p = 1 chains in both


@pytest.mark.parametrize("ladder", [False, True])
def test_autograd_through_a_flagged_dynamics_matches_float64(ladder):
    T, X, N, eps, B, regime, seed = AG
    beta = np.linspace(1.5, 3.5, B).astype(np.float32) if ladder else 2.5
    dyn, _, _ = _hip(T, X, N, eps, B, regime, **FLAGGED)
    x, _, dx, _ = _draws(T, X, B, seed)
    rng = np.random.default_rng(17)
    c = [rng.standard_normal((B, 2 * T * X)), rng.standard_normal((B, 2 * T * X)), rng.standard_normal(B)]
    _requires_grad(dyn)
    xg = torch.tensor(x, dtype=torch.float32, device="cuda", requires_grad=True)
    bdev = _dev(beta) if ladder else beta
    outs = []
    assert RC.count_launches(5, lambda: outs.extend(dyn(xg, bdev, **_draw_kw(dx)))) == 1
    loss = sum((_dev(ci) * o).sum() for ci, o in zip(c, outs[:3]))        # reads x_prop, v_prop and p_accept
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
    print(f"[periodic train forward] autograd ladder={ladder}: worst {max(worst.values()):.3e} "
          f"({max(worst, key=worst.get)})")


# ---- 7. workspace contract -----------------------------------------------------------------------------------------
def test_gradients_do_not_depend_on_what_the_workspace_held(monkeypatch):
    tr, _, x, z, dx, dz = _trainer(8, 8, 2, 0.2, 9, "mild", 2, fused_forward=True)
    got = []
    for pattern in (0x00, 0xFF):
        with W.poisoned(monkeypatch, pattern) as shared:
            out = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
            assert shared.gets >= 1
        got.append((tr.grads.clone(), tr.last_loss_terms.clone(), out[0].clone()))
    for _ in range(2):                           # and on two calls in a row, on the trainer's own workspace
        out = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
        got.append((tr.grads.clone(), tr.last_loss_terms.clone(), out[0].clone()))
    assert tr._walk is None and _train_fused(tr.dynamics) == 1 and bool(torch.isfinite(got[0][0]).all())
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert torch.equal(a, b)


# ---- 8. the public loop --------------------------------------------------------------------------------------------
def _loop_trainer(seed, eps=0.2, T=8, X=8, **kw):
    from l2hmc_amd import GaugeLattice, GaugeDynamics
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    np.random.seed(seed)
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=16, rand=True)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=eps, num_steps=2, eps_trainable=True, periodic=True,
                        seed=seed, **FLAGGED, **kw)
    return GaugeTrainer(dyn, lr_init=1e-3)


def test_public_training_loop_moves_every_weight_and_resumes_bit_for_bit(tmp_path):
    B, D = 16, 128
    tr = _loop_trainer(5)
    assert _train_fused(tr.dynamics) == 1
    before = {(i, k): v.detach().clone() for i, n in enumerate(tr._nets) for k, v in n.flat_params()[1].items()}
    eps0 = float(tr.dynamics.eps)
    x = _dev(np.random.default_rng(1).uniform(0, TWO_PI, (B, D)))
    for _ in range(20):
        loss, x, px, _ = tr.train_step(x, 2.0)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(px).all())
    assert RC.count_launches(5, lambda: tr.train_step(x, 2.0)) == 1       # the packed images follow the optimiser
    for (i, k), w0 in before.items():
        assert not torch.equal(tr._nets[i].flat_params()[1][k], w0), (i, k)
    assert float(tr.dynamics.eps) != eps0
    b0, b1 = np.tile(np.linspace(1.0, 2.5, 4), 4), np.tile(np.linspace(2.0, 4.0, 4), 4)
    out = tr.train(4, samples_init=x, beta_init=b0, beta_final=b1, replicas=4, swap_every=2)
    assert tr._walk is None and tr.global_step == 25
    for k in ("loss", "accept_prob", "eps"):
        assert np.isfinite(out[k]).all(), k
    assert out["swapped"].shape == (2, B) and out["beta"].shape == (4, B)      # an exchange round every second step
    # save -> load into a fresh flagged trainer: the next step's gradients, bit for bit, with injected draws
    path = str(tmp_path / "state.npz")
    xs = out["samples"]
    tr.save_state(path, samples=xs, beta=b1)
    _, z, dx, dz = _draws(8, 8, B, 9)
    tr.calc_loss_and_grads(xs, b1.astype(np.float32), z=z, draws_x=dx, draws_z=dz)
    tr2 = _loop_trainer(11, eps=0.3, whole_step=True)      # other weights, masks and eps: load_state restores them all
    extra = tr2.load_state(path)
    tr2.calc_loss_and_grads(torch.as_tensor(extra["samples"], device="cuda"), extra["beta"].astype(np.float32), z=z,
                            draws_x=dx, draws_z=dz)
    assert tr2._walk is None
    assert torch.equal(tr.grads, tr2.grads) and torch.equal(tr.last_loss_terms, tr2.last_loss_terms)


# ---- 9. the carried flag -------------------------------------------------------------------------------------------
def test_other_lattices_carry_the_flag():
    args = (4, 4, 2, 0.2, 9, "mild", 2)
    trf, _, x, z, dx, dz = _trainer(*args, fused_forward=True)
    tru, *_ = _trainer(*args)
    assert _train_fused(trf.dynamics) == 0 and trf.dynamics.fused_forward is True
    outs = [t.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz) for t in (trf, tru)]
    assert torch.equal(trf.grads, tru.grads) and torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(trf.last_loss_terms, tru.last_loss_terms) and trf._walk is None
    # 6x6: the walk trains, flag or not
    tr6, tm6, *a6 = _trainer(6, 6, 2, 0.2, 9, "mild", 7, fused_forward=True)
    _check_step(tr6, tm6, *a6, 2.5, "6x6 with the flag")
    assert tr6._walk is not None
