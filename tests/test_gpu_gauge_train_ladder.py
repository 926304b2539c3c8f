"""Training GaugeDynamics on a ladder of beta in one step (l2hmc_gauge_train_forward_ladder / _loss_backward_ladder /
_train_backward_ladder; `GaugeTrainer.calc_loss_and_grads`, `train_step` and `train` with a beta per chain).

Three betas {1, 2, 3} lie on the chains in a fixed non-periodic pattern (tests/ladder_ref.py), so rows of one 16-row
workgroup differ and a chain's x row and z row sit at different places in their workgroups.
  1. per-row outputs of the three entries are the scalar entries' at the row's beta, bit for bit;
  2. degenerate ladders (one value, stride 0 or 1) are the scalar step, bit for bit;
  3. weight and eps gradients against float64 autograd (ladder_ref.LadderGaugeModel) at test_gpu_train.py's gate;
  4. the bucketed backward; 5. `train` with arrays and with exchange rounds; 6. reproducibility.
Every path: fused GenericNet, fused ConvNet3D forward with the trunk reverse, tiled, layered walk."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import ladder_ref as LR
from tests.test_gpu_train import TOL_G, _compare

pytestmark = pytest.mark.gpu

# (T, X, N, eps, B, regime, arch, fused): the paths a training step takes
FUSED_G24 = (8, 8, 2, 0.1, 24, "mild", "generic", True)
FUSED_G9 = (8, 8, 3, 0.1, 9, "mild", "generic", True)          # a partly filled tile (18 rows)
FUSED_C9 = (8, 8, 2, 0.1, 9, "mild", "conv3D", True)
TILED_6 = (4, 4, 3, 0.2, 6, "mild", "generic", True)
TILED_37 = (4, 4, 2, 0.15, 37, "mild", "generic", True)        # ragged
TILED_L8 = (8, 8, 2, 0.1, 9, "mild", "generic", False)         # benchmark widths through the tiled kernels
WALK_66 = (6, 6, 3, 0.1, 6, "mild", "generic", True)           # widths that are no multiples of 32: the layered walk
WALK_35 = (3, 5, 2, 0.1, 37, "mild", "generic", True)
CASES = [FUSED_G24, FUSED_G9, FUSED_C9, TILED_6, TILED_37, TILED_L8, WALK_66, WALK_35]
STRESS = [(8, 8, 2, 0.1, 9, "stress", "generic", True), (8, 8, 2, 0.1, 5, "stress", "conv3D", True),
          (4, 4, 2, 0.15, 37, "stress", "generic", True), (3, 5, 2, 0.1, 9, "stress", "generic", True)]
ONE_PER_PATH = [FUSED_G9, FUSED_C9, TILED_6, WALK_66]


def ids(c):
    return f"{c[0]}x{c[1]}-N{c[2]}-B{c[4]}-{c[5]}-{c[6]}-{'fused' if c[7] else 'tiled'}"


def _setup(case, cls=LR.LadderGaugeModel):
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    T, X, N, eps, B, regime, arch, fused = case
    xp, vp = H.gauge_weights(T, X, regime=regime) if arch == 'generic' else H.conv_weights(T, X, regime=regime)
    orc = H.gauge_oracle(T, X, N, eps, xp, vp, arch=arch)
    dyn = H.gauge_hip(T, X, N, eps, xp, vp, orc.mask, B, arch=arch)
    dyn.fused = fused
    tr = GaugeTrainer(dyn, lr_init=1e-3)
    tm = cls(T, X, N, eps, orc.mask, xp, vp, arch=arch)
    return tr, tm, LR.inputs(B, 2 * T * X)


def _tiled(tr):
    return not tr._use_layered()


def _entries(tr, x, z, dx, dz, beta, bucket_ids=None):
    """One training step's three C entries on explicit x0, v0, dir: `beta` a float (scalar entries) or a float32 device
    tensor [B] / [1] (the _ladder entries, stride 1 / 0).  Cotangents of the reverse pass are the loss entry's own, with
    the trainer's loss weights and 1 / B.  -> dict of the per-row outputs and the flat gradient buffer (deps last)."""
    from l2hmc_amd import _lib
    from l2hmc_amd._flat_trainer import stack_chains
    from l2hmc_amd.gauge_trainer import METRICS
    dyn = tr.dynamics
    dev = dyn._device
    T, X = dyn.lattice.time_size, dyn.lattice.space_size
    x0, v0, _, dirs, _ = stack_chains(dyn._x(x), dyn._x(z), tuple(_lib.as_dev(a, dev) for a in dx),
                                      tuple(_lib.as_dev(a, dev) for a in dz))
    B, R = x.shape[0], 2 * x.shape[0]
    lad = not isinstance(beta, float)
    head = (beta, int(beta.numel() > 1), B) if lad else (beta,)
    plan, L = dyn._plan(), _lib.lib()
    xN, vN = torch.empty_like(x0), torch.empty_like(x0)
    sld, p = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(2))
    ws, nb = tr._ws.get(L.l2hmc_gauge_train_ws_bytes(C.byref(plan), R), dev)
    _lib.call("l2hmc_gauge_train_forward_ladder" if lad else "l2hmc_gauge_train_forward", C.byref(plan), *head, x0, v0,
              dirs, R, xN, vN, sld, p, ws, nb, device=dev)
    terms = torch.empty(B, dtype=torch.float32, device=dev)
    dxN, dvN = torch.empty_like(x0), torch.empty_like(x0)
    dld = torch.empty(R, dtype=torch.float32, device=dev)
    _lib.call("l2hmc_gauge_loss_backward_ladder" if lad else "l2hmc_gauge_loss_backward", T, X, *head[:2], x0, xN, vN, p,
              B, METRICS[tr.metric], 1., 1., 1., 1., 1.0 / B, terms, dxN, dvN, dld, device=dev)
    out = dict(x_out=xN, v_out=vN, sumlogdet=sld, p_accept=p, terms=terms, dxN=dxN.clone(), dvN=dvN.clone(),
               dlogdet=dld)
    n0, n1 = tr._sizes
    tr.grads.zero_()
    bargs = (C.byref(plan), *head, dirs, R, dxN, dvN, dld, C.byref(tr._grad_structs[0]), C.byref(tr._grad_structs[1]),
             *(C.byref(g) if g is not None else None for g in tr._conv_grad_structs), tr.grads[n0 + n1:], ws, nb)
    cb = _lib.BUCKET_FN(lambda _u, b: bucket_ids.append(int(b))) if bucket_ids is not None else _lib.BUCKET_FN()
    if lad:
        _lib.call("l2hmc_gauge_train_backward_ladder", *bargs, device=dev, tail=(cb, None))
    elif bucket_ids is not None:
        _lib.call("l2hmc_gauge_train_backward_buckets", *bargs, device=dev, tail=(cb, None))
    else:
        _lib.call("l2hmc_gauge_train_backward", *bargs, device=dev)
    out.update(dx=dxN, dv=dvN, grads=tr.grads.clone())
    return out


PER_ROW = ("x_out", "v_out", "sumlogdet", "p_accept", "dxN", "dvN", "dlogdet", "dx", "dv")


# ---- 1. chain-axis outputs, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_rows_of_a_rung_have_the_bits_of_the_scalar_step_at_its_beta(case):
    tr, _, (x, z, dx, dz) = _setup(case)
    B = case[4]
    dev = tr.dynamics._device
    rung, betas = LR.rung_of(B), LR.ladder(B)
    if not _tiled(tr):
        # the layered walk has no C entry of its own: the forward columns through calc_loss_and_grads' outputs, and the
        # reverse walk's d loss / d (x_0, v_0) (LayeredWalk.start_cotangents: the host-scaled Hessian-vector product)
        lad = tr.calc_loss_and_grads(x, betas, z=z, draws_x=dx, draws_z=dz)
        terms, pz = tr.last_loss_terms.clone(), tr.last_pz.clone()
        dx0, dv0 = tr._walk.start_cotangents
        assert float(dx0.abs().max()) > 0 and float(dv0.abs().max()) > 0
        for g, b in enumerate(LR.RUNGS):
            ch = np.nonzero(rung == g)[0]
            rows, both = torch.as_tensor(ch, device=dev), torch.as_tensor(np.concatenate([ch, B + ch]), device=dev)
            ref = tr.calc_loss_and_grads(x, float(b), z=z, draws_x=dx, draws_z=dz)
            for a, w in zip(lad[1:], ref[1:]):                      # x_out, accept_prob, x_dq of the x chains
                assert torch.equal(a[rows], w[rows])
            assert torch.equal(terms[rows], tr.last_loss_terms[rows]) and torch.equal(pz[rows], tr.last_pz[rows])
            for a, w in zip((dx0, dv0), tr._walk.start_cotangents):
                assert torch.equal(a[both], w[both])
        return
    lad = _entries(tr, x, z, dx, dz, torch.as_tensor(betas, dtype=torch.float32, device=dev))
    for g, b in enumerate(LR.RUNGS):
        ch = np.nonzero(rung == g)[0]
        rows = torch.as_tensor(np.concatenate([ch, B + ch]), device=dev)
        ref = _entries(tr, x, z, dx, dz, float(b))
        for k in PER_ROW:
            assert torch.equal(lad[k][rows], ref[k][rows]), (k, b)
        cht = torch.as_tensor(ch, device=dev)
        assert torch.equal(lad["terms"][cht], ref["terms"][cht])


# ---- 2. degenerate ladders are the scalar step -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ONE_PER_PATH, ids=ids)
def test_degenerate_ladders_are_the_scalar_step_bit_for_bit(case):
    tr, _, (x, z, dx, dz) = _setup(case)
    B = case[4]
    dev = tr.dynamics._device
    want = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    wg = tr.grads.clone()
    got = tr.calc_loss_and_grads(x, np.full(B, 2.5), z=z, draws_x=dx, draws_z=dz)         # stride 1, B equal values
    assert torch.equal(tr.grads, wg) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if _tiled(tr):                                                                        # stride 0, one value
        a = _entries(tr, x, z, dx, dz, torch.full((1,), 2.5, dtype=torch.float32, device=dev))
        assert torch.equal(a["grads"], wg)                   # the whole buffer, deps in its last slot
        assert torch.equal(a["terms"].sum(dtype=torch.float32) / B, want[0])
        b = _entries(tr, x, z, dx, dz, 2.5)
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ---- 3. weight and eps gradients against float64 ---------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + STRESS, ids=ids)
def test_ladder_gradients_match_float64_autograd(case):
    """Per case the worst ratio of the ladder, and of the scalar entry at the case's top beta against the same float64
    model -- the run that shows the case is well chosen: it meets the gate on its own.  Both are printed (run with -s;
    the figures measured on the MI355X are in profiles/gauge_train_ladder.txt)."""
    tr, tm, (x, z, dx, dz) = _setup(case)
    betas = LR.ladder(case[4])
    top = float(betas.max())
    tr.calc_loss_and_grads(x, top, z=z, draws_x=dx, draws_z=dz)
    LR.ref_grads(tm, x, z, dx, dz, top)
    scalar = _compare(tr, tm, tol=TOL_G)
    loss, *_ = tr.calc_loss_and_grads(x, betas, z=z, draws_x=dx, draws_z=dz)
    want_loss, want_terms = LR.ref_grads(tm, x, z, dx, dz, betas)
    worst = _compare(tr, tm, tol=np.inf)
    print(f"ladder {ids(case)}: worst gradient ratio {max(worst.values()):.3g} ({max(worst, key=worst.get)}); "
          f"scalar at beta {top}: {max(scalar.values()):.3g} ({max(scalar, key=scalar.get)})")
    # (the tolerances of tests/test_gpu_train.py::test_loss_gradients_match_autograd)
    np.testing.assert_allclose(tr.last_loss_terms.cpu().numpy(), want_terms, rtol=2e-4,
                               atol=1e-5 * max(1., np.abs(want_terms).max()))
    assert abs(float(loss) - want_loss) <= 2e-4 * max(1., abs(want_loss))
    _compare(tr, tm, tol=TOL_G)


# ---- 4. bucketed backward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [FUSED_G9, FUSED_C9, TILED_6], ids=ids)
def test_bucketed_ladder_backward_is_the_plain_one(case):
    tr, _, (x, z, dx, dz) = _setup(case)
    betas = torch.as_tensor(LR.ladder(case[4]), dtype=torch.float32, device=tr.dynamics._device)
    plain = _entries(tr, x, z, dx, dz, betas)
    seen, seen_scalar = [], []
    bucketed = _entries(tr, x, z, dx, dz, betas, bucket_ids=seen)
    _entries(tr, x, z, dx, dz, 2.0, bucket_ids=seen_scalar)
    assert torch.equal(plain["grads"], bucketed["grads"])
    assert seen == seen_scalar == [0, 1, 2, 3, 4, 5, 6]


# ---- 5. train with arrays --------------------------------------------------------------------------------------------
def _train_setup():
    tr, _, (x, *_) = _setup((4, 4, 2, 0.1, 16, "init", "generic", True))
    tr.lr_init = 1e-4
    return tr, x


def test_train_anneals_a_ladder_rung_by_rung():
    tr, x = _train_setup()
    b0, b1 = np.linspace(1.0, 2.5, 16), np.linspace(2.0, 3.0, 16)
    out = tr.train(5, samples_init=x, beta_init=b0, beta_final=b1)
    assert out["beta"].shape == (5, 16) and out["loss"].shape == (5,) and np.isfinite(out["loss"]).all()
    want = np.stack([1. / ((1. / b0 - 1. / b1) * (1 - s / 5.) + 1. / b1) for s in range(5)])
    np.testing.assert_allclose(out["beta"], want, rtol=1e-12)
    xs = out["samples"].cpu().numpy()
    assert (xs >= 0).all() and (xs < 2 * np.pi + 1e-6).all()
    assert tr.global_step == 5 and len(set(out["eps"])) > 1
    assert "swapped" not in out


def test_train_with_replicas_is_the_hand_written_loop():
    from l2hmc_amd import ops
    from l2hmc_amd.gauge_sampler import GaugeSampler
    b0, b1 = np.tile([1.0, 1.5, 2.0, 2.5], 4), np.tile([1.5, 2.0, 2.5, 3.0], 4)
    tr, x = _train_setup()
    out = tr.train(5, samples_init=x, beta_init=b0, beta_final=b1, replicas=4, swap_every=2)
    assert out["swapped"].shape == (2, 16) and out["swapped"].dtype == np.bool_ and out["swap_rate"].shape == (3,)
    tr2, _ = _train_setup()
    dyn = tr2.dynamics
    smp = GaugeSampler(dyn)
    xs = dyn._x(x).clone()
    swapped = []
    for s in range(1, 6):
        beta = tr2.update_beta(s - 1, b0, b1, 5)
        _, x_out, _, _ = tr2.train_step(xs, beta)
        ops.wrap_angle(x_out, out=xs)
        if s % 2 == 0:
            swapped.append(smp.swap_replicas(xs, beta, 4, (s // 2 - 1) % 2)[1].cpu().numpy())
    assert torch.equal(out["samples"], xs) and tr.dynamics._draws == dyn._draws
    for a, b in zip(tr._nets, tr2._nets):
        assert torch.equal(a.flat_params()[0], b.flat_params()[0])
    assert float(tr.dynamics.eps) == float(dyn.eps)
    np.testing.assert_array_equal(out["swapped"], np.stack(swapped))


def test_train_without_replicas_is_the_train_it_was():
    from l2hmc_amd import ops
    tr, x = _train_setup()
    out = tr.train(4, samples_init=x, beta_init=2., beta_final=3.)
    tr2, _ = _train_setup()
    dyn = tr2.dynamics
    xs = dyn._x(x).clone()
    for s in range(4):
        _, x_out, _, _ = tr2.train_step(xs, tr2.update_beta(s, 2., 3., 4))
        ops.wrap_angle(x_out, out=xs)
    assert out["beta"].shape == (4,) and torch.equal(out["samples"], xs) and tr.dynamics._draws == dyn._draws
    for a, b in zip(tr._nets, tr2._nets):
        assert torch.equal(a.flat_params()[0], b.flat_params()[0])


def test_state_keeps_an_array_beta(tmp_path):
    tr, x = _train_setup()
    b = LR.ladder(16)
    tr.save_state(str(tmp_path / "s.npz"), samples=x, beta=b)
    np.testing.assert_array_equal(tr.load_state(str(tmp_path / "s.npz"))["beta"], b)


def test_bad_betas_are_refused_before_any_draw():
    tr, x = _train_setup()
    d0 = tr.dynamics._draws
    for bad in (np.ones(15), np.ones((2, 16)), -LR.ladder(16), np.where(np.arange(16) == 3, np.nan, 1.0),
                np.where(np.arange(16) == 3, np.inf, 1.0)):
        with pytest.raises(ValueError):
            tr.calc_loss_and_grads(x, bad)
    assert tr.dynamics._draws == d0


# ---- 6. reproducibility ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ONE_PER_PATH, ids=ids)
def test_two_ladder_calls_give_the_same_bits(case):
    tr, _, (x, z, dx, dz) = _setup(case)
    betas = LR.ladder(case[4])
    a = tr.calc_loss_and_grads(x, betas, z=z, draws_x=dx, draws_z=dz)
    ga = tr.grads.clone()
    b = tr.calc_loss_and_grads(x, betas[None, :], z=z, draws_x=dx, draws_z=dz)             # [1, B] is the same ladder
    assert torch.equal(ga, tr.grads) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
