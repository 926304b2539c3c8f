"""Training toy-target Dynamics on a ladder of temperatures in one step (l2hmc_small_train_step_tempered;
`DynamicsTrainer.calc_loss_and_grads`, `train_step` and `train` with a temperature per chain).

Three temperatures {1, 1.7, 2.5} lie on the chains in a fixed non-periodic pattern (tests/toy_ladder_ref.py), so rows of
one 16-chain workgroup differ and a chain's x row and z row sit in different slots of their workgroups.
  1. per-row outputs of the entry are the scalar entry's at the row's temperature, bit for bit;
  2. degenerate ladders (one value, stride 0 or 1) are the scalar step, bit for bit, the gradient buffer included;
  3. weight and alpha gradients against float64 autograd (toy_ladder_ref.LadderDynamicsModel) at test_gpu_train.py's gates;
  4. the layered path: the same gates, and per-row bits of the scalar layered step;
  5. `temperature=scalar` is the step at `dyn.temperature = scalar`; 6. `train` is the hand-written loop, and
  reproducible; 7. the sampler sees the trained weights."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import toy_ladder_ref as TL
from tests.test_gpu_train import TOL_G, _mlp_packed_ref

pytestmark = pytest.mark.gpu


def _stacked(tr, c):
    """The 2B stacked rows of a case as the training step runs them: (x0, v0, dirs) on the device."""
    from l2hmc_amd import _lib
    from l2hmc_amd._flat_trainer import stack_chains
    dev = tr.dynamics._device
    i = TL.inputs(c)
    dv = lambda a: _lib.as_dev(a, dev)          # noqa: E731
    x0, v0, _, dirs, _ = stack_chains(dv(i["x"]), dv(i["z"]), tuple(map(dv, i["dx"])), tuple(map(dv, i["dz"])))
    return x0, v0, dirs


def _entry(tr, c, temps):
    """One call of the C entry on the case's stacked rows: `temps` a float (l2hmc_small_train_step on a plan with that
    temperature) or a float32 device tensor [B] / [1] (l2hmc_small_train_step_tempered, stride 1 / 0; the plan's own
    temperature is then set to a value no rung has).  -> dict of the per-row outputs and the gradient buffer."""
    from l2hmc_amd import _lib
    dyn = tr.dynamics
    dev = dyn._device
    x0, v0, dirs = _stacked(tr, c)
    R = x0.shape[0]
    xN, vN = torch.empty_like(x0), torch.empty_like(x0)
    p, terms = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(2))
    grads = torch.full_like(tr.grads, float("nan"))
    plan, L = dyn._plan(), _lib.lib()
    ws, nb = tr._ws.get(L.l2hmc_small_train_ws_bytes(C.byref(plan), R), dev)
    tail = (x0, v0, dirs, R, tr.scale, 1.0 / c.B, xN, vN, p, terms, grads, ws, nb)
    if isinstance(temps, float):
        plan.target.temperature = temps
        _lib.call("l2hmc_small_train_step", C.byref(plan), *tail, device=dev)
    else:
        plan.target.temperature = 7.25          # ignored by the entry
        _lib.call("l2hmc_small_train_step_tempered", C.byref(plan), temps, int(temps.numel() > 1), c.B, *tail, device=dev)
    return dict(x_out=xN, v_out=vN, p_accept=p, terms=terms, grads=grads)


PER_ROW = ("x_out", "v_out", "p_accept", "terms")


def _dev32(tr, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=tr.dynamics._device)


# ---- 1. chain-axis outputs, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TL.ONE_LAUNCH_CASES, ids=TL.case_id)
def test_rows_of_a_rung_have_the_bits_of_the_scalar_step_at_its_temperature(c):
    tr = TL.trainer(c)
    dev = tr.dynamics._device
    rung, temps = TL.rung_of(c.B), TL.ladder(c.B)
    lad = _entry(tr, c, _dev32(tr, temps))
    assert all(bool(torch.isfinite(lad[k]).all()) for k in lad)
    seen = 0
    for g, t in enumerate(TL.RUNGS):
        ch = np.nonzero(rung == g)[0]
        rows = torch.as_tensor(np.concatenate([ch, c.B + ch]), device=dev)
        ref = _entry(tr, c, float(t))
        for k in PER_ROW:
            assert torch.equal(lad[k][rows], ref[k][rows]), (k, t)
        if g:              # ... and the temperature matters: the rung's rows differ from the rung-0 run's
            seen += int(not torch.equal(lad["x_out"][rows], first["x_out"][rows]))
        else:
            first = ref
    assert seen == 2


# ---- 2. degenerate ladders are the scalar step -----------------------------------------------------------------------
@pytest.mark.parametrize("c", TL.ONE_LAUNCH_CASES, ids=TL.case_id)
def test_degenerate_ladders_are_the_scalar_step_bit_for_bit(c):
    tr = TL.trainer(c)
    want = _entry(tr, c, 1.7)                   # (1.7 is no float32 number: the scalar and the entry round alike)
    assert bool(torch.isfinite(want["grads"]).all()) and float(want["grads"].abs().max()) > 0
    for temps in (np.full(c.B, 1.7), np.full(1, 1.7)):          # stride 1, B equal values; stride 0, one value
        got = _entry(tr, c, _dev32(tr, temps))
        for k in want:
            assert torch.equal(got[k], want[k]), (k, temps.shape)


def test_a_ladder_through_the_trainer_is_the_entry_and_leaves_the_dynamics_alone():
    c = TL.MOG
    tr = TL.trainer(c, temperature=3.0)
    i = TL.inputs(c)
    want = _entry(tr, c, _dev32(tr, TL.ladder(c.B)))
    d0 = tr.dynamics._draws
    for temps in (TL.ladder(c.B), TL.ladder(c.B)[None, :], _dev32(tr, TL.ladder(c.B))):
        tr.grads.zero_()
        tr.calc_loss_and_grads(i["x"], z=i["z"], draws_x=i["dx"], draws_z=i["dz"], temperature=temps)
        assert torch.equal(tr.last_proposals, want["x_out"]) and torch.equal(tr.last_p, want["p_accept"])
        assert torch.equal(tr.last_terms, want["terms"])
        assert torch.equal(tr.grads[:-1], want["grads"][:-1])
        assert torch.equal(tr.grads[-1], want["grads"][-1] * float(tr.dynamics.eps))          # d/d alpha = eps d/d eps
    assert tr.dynamics.temperature == 3.0 and tr.dynamics._draws == d0


# ---- 3. gradients against float64 ------------------------------------------------------------------------------------
def _grad_errors(tr, tm):
    gv = tr.grad_views()
    worst = {}
    for name, net in (("xnet", tm.xnet), ("vnet", tm.vnet)):
        for k, w in _mlp_packed_ref(net).items():
            got = gv[name][k].cpu().numpy().astype(np.float64).reshape(w.shape)
            worst[f"{name}.{k}"] = float(np.abs(got - w).max() / np.abs(w).max())
    worst["alpha"] = abs(float(gv["alpha"][0]) - float(tm.alpha.grad)) / abs(float(tm.alpha.grad))
    return worst


def _against_float64(c, ref_case):
    """The ladder step of case c through calc_loss_and_grads against toy_ladder_ref.reference(ref_case): every figure is
    printed (run with -s), then held at the gates of tests/test_gpu_train.py::test_toy_target_loss_gradients_match_autograd."""
    tr = TL.trainer(c)
    i = TL.inputs(c)
    loss, x_out, px = tr.calc_loss_and_grads(i["x"], z=i["z"], draws_x=i["dx"], draws_z=i["dz"],
                                             temperature=TL.ladder(c.B))
    tm, want, want_terms, Lw, pw = TL.reference(ref_case)
    e_prop = H.relerr(tr.last_proposals.cpu().numpy(), Lw)
    e_p = float(np.abs(tr.last_p.cpu().numpy() - pw).max())
    e_loss = abs(float(loss) - want) / max(1., abs(want))
    worst = _grad_errors(tr, tm)
    print(f"ladder {TL.case_id(c)}: proposals {e_prop:.3g}, p {e_p:.3g}, loss {e_loss:.3g}, worst gradient ratio "
          f"{max(worst.values()):.3g} ({max(worst, key=worst.get)})")
    assert e_prop < 1e-5 and e_p < 2e-5 and e_loss <= 2e-4
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, f"gradient mismatch: {bad}\nall: {worst}"
    acc = (tr.last_p[:c.B].cpu().numpy() - i["dx"][3]) >= 0                  # sampler.py:57-59 (>=)
    np.testing.assert_array_equal(x_out.cpu().numpy()[acc], tr.last_proposals[:c.B].cpu().numpy()[acc])
    np.testing.assert_array_equal(x_out.cpu().numpy()[~acc], i["x"][~acc].astype(np.float32))
    return tr


@pytest.mark.parametrize("c", TL.GRADIENT_CASES, ids=TL.case_id)
def test_ladder_gradients_match_float64_autograd(c):
    _against_float64(c, c)


# ---- 4. the layered path ---------------------------------------------------------------------------------------------
# A callable energy's scalar step divides by the Python number: torch multiplies by the float64 quotient 1 / 1.7 rounded
# to float32, which no float32 ladder entry reproduces (it holds float32(1.7), whose quotient rounds elsewhere).  Such
# rows are held bit for bit to the scalar step at the float32 temperature the ladder holds, and to the step at the
# float64 number within twice the gap measured on the MI355X (max |difference| over the rung's rows / max |value|:
# proposals 1.72e-8, p 1.37e-6, terms 3.39e-6, dx0 1.88e-7, dv0 2.47e-7).
CALLABLE_GAP = dict(proposals=3.5e-8, p=2.8e-6, terms=6.8e-6, dx0=3.8e-7, dv0=5.0e-7)


@pytest.mark.parametrize("c", TL.LAYERED_CASES, ids=TL.case_id)
def test_layered_ladder_matches_float64_and_the_scalar_layered_step_bit_for_bit(c):
    tr = _against_float64(c, c._replace(layered=c.kind == "quartic10"))
    assert tr.dynamics.layered
    dev = tr.dynamics._device
    i = TL.inputs(c)
    kw = dict(z=i["z"], draws_x=i["dx"], draws_z=i["dz"])
    rung = TL.rung_of(c.B)
    lad = (tr.last_proposals.clone(), tr.last_p.clone(), tr.last_terms.clone(), *tr._layered.walk.start_cotangents)
    assert all(float(a.abs().max()) > 0 for a in lad)
    for g, t in enumerate(TL.RUNGS):
        ch = np.nonzero(rung == g)[0]
        rows = torch.as_tensor(np.concatenate([ch, c.B + ch]), device=dev)
        names = ("proposals", "p", "terms", "dx0", "dv0")
        packed = tr.dynamics._target is not None
        tr.calc_loss_and_grads(i["x"], temperature=float(t) if packed else float(np.float32(t)), **kw)
        ref = (tr.last_proposals, tr.last_p, tr.last_terms, *tr._layered.walk.start_cotangents)
        for name, a, w in zip(names, lad, ref):
            assert torch.equal(a[rows], w[rows]), (name, t, float((a[rows] - w[rows]).abs().max()))
        if not packed:
            tr.calc_loss_and_grads(i["x"], temperature=float(t), **kw)
            ref = (tr.last_proposals, tr.last_p, tr.last_terms, *tr._layered.walk.start_cotangents)
            gap = {n: float((a[rows] - w[rows]).abs().max() / w[rows].abs().max()) for n, a, w in zip(names, lad, ref)}
            print(f"callable ladder against the scalar layered step at {t} (a float64 number): {gap}")
            assert all(gap[n] <= CALLABLE_GAP[n] for n in names), (t, gap)
    # equal values: the scalar layered step's gradients
    tr.calc_loss_and_grads(i["x"], temperature=float(np.float32(1.7)), **kw)
    want = tr.grads.clone()
    tr.calc_loss_and_grads(i["x"], temperature=np.full(c.B, 1.7), **kw)
    assert torch.equal(tr.grads, want)


# ---- 5. a scalar temperature= ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [TL.MOG_16, TL.QUARTIC], ids=TL.case_id)
def test_a_scalar_temperature_is_the_step_at_that_dynamics_temperature(c):
    i = TL.inputs(c)
    kw = dict(z=i["z"], draws_x=i["dx"], draws_z=i["dz"])
    a, b = TL.trainer(c, temperature=3.0), TL.trainer(c, temperature=3.0)
    out_a = a.train_step(i["x"], temperature=1.7, **kw)
    assert a.dynamics.temperature == 3.0
    b.dynamics.temperature = 1.7
    out_b = b.train_step(i["x"], **kw)
    for got, want in zip(out_a, out_b):
        assert torch.equal(got, want)
    assert torch.equal(a.grads, b.grads) and float(a.dynamics.alpha) == float(b.dynamics.alpha)
    for na, nb in zip(a._nets, b._nets):
        assert torch.equal(na.flat_params()[0], nb.flat_params()[0])
    # ... and it is not the step at the dynamics' own temperature
    d = TL.trainer(c, temperature=3.0)
    assert not torch.equal(d.train_step(i["x"], **kw)[2], out_a[2])


# ---- 6. train --------------------------------------------------------------------------------------------------------
TRAIN = TL.MOG3_16                  # B = 9: three groups of three rungs
T0 = np.tile([1.0, 1.7, 2.5], 3)
SCHEDULE = dict(annealing_steps=2, annealing_factor=0.9)


def _trained():
    tr = TL.trainer(TRAIN)
    tr.lr_init = 1e-3
    out = tr.train(6, TL.inputs(TRAIN)["x"], temp_init=T0, replicas=3, swap_every=2, **SCHEDULE)
    return tr, out


@pytest.fixture(scope="module")
def trained():
    return _trained()


def test_train_with_replicas_is_the_hand_written_loop(trained):
    from l2hmc_amd import _lib
    from l2hmc_amd.dynamics_sampler import DynamicsSampler
    from l2hmc_amd.dynamics_trainer import temperature_schedule
    tr, out = trained
    assert out["temperature"].shape == (6, 9) and out["loss"].shape == (6,) and np.isfinite(out["loss"]).all()
    assert out["swapped"].shape == (3, 9) and out["swapped"].dtype == np.bool_ and out["swap_rate"].shape == (2,)
    tr2 = TL.trainer(TRAIN)
    tr2.lr_init = 1e-3
    dyn = tr2.dynamics
    smp = DynamicsSampler(dyn)
    xs = _lib.as_dev(TL.inputs(TRAIN)["x"], dyn._device)
    hist = {k: [] for k in ("loss", "accept_prob", "eps", "lr", "temperature")}
    swapped = []
    for s in range(1, 7):
        t = temperature_schedule(s - 1, T0, **SCHEDULE)
        hist["lr"].append(tr2.learning_rate())
        loss, xs, px = tr2.train_step(xs, temperature=t)
        if s % 2 == 0:
            swapped.append(smp.swap_replicas(xs, t, 3, (s // 2 - 1) % 2)[1].cpu().numpy())
        for k, v in (("loss", float(loss)), ("accept_prob", float(px.mean())), ("eps", float(dyn.eps)), ("temperature", t)):
            hist[k].append(v)
    assert torch.equal(out["samples"], xs) and tr.dynamics._draws == dyn._draws
    for a, b in zip(tr._nets, tr2._nets):
        assert torch.equal(a.flat_params()[0], b.flat_params()[0])
    assert float(tr.dynamics.alpha) == float(dyn.alpha) and tr.global_step == tr2.global_step == 6
    for k, v in hist.items():
        np.testing.assert_array_equal(out[k], np.asarray(v, dtype=out[k].dtype), err_msg=k)
    np.testing.assert_array_equal(out["swapped"], np.stack(swapped))
    assert out["temperature"][0].tolist() == T0.tolist() and (out["temperature"][-1] < T0)[T0 > 1.2].all()
    assert (out["temperature"][:, 0] == 1.0).all() and len(set(out["eps"])) > 1


def test_two_train_runs_from_one_seed_are_identical(trained):
    tr, out = trained
    tr2, out2 = _trained()
    assert torch.equal(out["samples"], out2["samples"]) and tr.dynamics._draws == tr2.dynamics._draws
    for k in out:
        if k != "samples":
            np.testing.assert_array_equal(out[k], out2[k], err_msg=k)
    for a, b in zip(tr._nets, tr2._nets):
        assert torch.equal(a.flat_params()[0], b.flat_params()[0])


def test_train_with_a_scalar_anneals_and_can_stop_when_annealed():
    tr = TL.trainer(TRAIN)
    tr.lr_init = 1e-3
    x = TL.inputs(TRAIN)["x"]
    out = tr.train(9, x, temp_init=1.2, annealing_steps=1, annealing_factor=0.9, stop_when_annealed=True)
    # 1.2 -> 1.08 after step 0; 1.08 * 0.9 is not > 1: the run ends after step 1
    assert out["temperature"].tolist() == [1.2, 1.2 * 0.9] and out["loss"].shape == (2,) and "swapped" not in out
    assert tr.global_step == 2 and tr.dynamics.temperature == 1.0
    out = tr.train(3, x, temp_init=1.2, annealing_steps=1, annealing_factor=0.9)
    assert out["temperature"].tolist() == [1.2, 1.2 * 0.9, 1.2 * 0.9] and tuple(out["samples"].shape) == x.shape


def test_train_refuses_before_the_first_step():
    tr = TL.trainer(TRAIN)
    x = TL.inputs(TRAIN)["x"]
    d0 = tr.dynamics._draws
    for kw in (dict(temp_init=np.ones(8)), dict(temp_init=-T0), dict(temp_init=T0, replicas=2),
               dict(temp_init=T0, replicas=3, swap_every=0), dict(temp_init=0.0)):
        with pytest.raises(ValueError):
            tr.train(2, x, **kw)
    lay = TL.trainer(TL.QUARTIC)
    l0 = lay.dynamics._draws
    with pytest.raises(NotImplementedError, match="swap_replicas: this dynamics runs layer by layer"):
        lay.train(2, TL.inputs(TL.QUARTIC)["x"], temp_init=T0, replicas=3)
    assert tr.dynamics._draws == d0 and tr.global_step == 0 and lay.dynamics._draws == l0 and lay.global_step == 0


# ---- 7. the sampler sees the trained weights -------------------------------------------------------------------------
def test_the_sampler_runs_the_trained_weights_on_the_ladder(trained):
    from l2hmc_amd.dynamics_sampler import DynamicsSampler
    tr, out = trained
    tr2, _ = _trained()
    fresh = TL.trainer(TRAIN)
    fresh.dynamics._draws = tr.dynamics._draws
    x = TL.inputs(TRAIN)["x"]
    d0 = tr.dynamics._draws
    runs = [DynamicsSampler(t.dynamics).run(5, x, temperature=T0[None, :]) for t in (tr, tr2, fresh)]
    tr.dynamics._draws = d0
    np.testing.assert_array_equal(runs[0]["px"], runs[1]["px"])
    np.testing.assert_array_equal(runs[0]["samples"], runs[1]["samples"])
    assert not np.array_equal(runs[0]["px"], runs[2]["px"])          # the untrained weights give another run
