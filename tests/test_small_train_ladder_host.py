"""Host side of training toy-target Dynamics on a ladder of temperatures (l2hmc_small_train_step_tempered in
l2hmc_amd/csrc/small_train.hip; `DynamicsTrainer` with a temperature per chain): the declaration and its binding, the
refusals that must come before any launch, what the trainer refuses before a draw is taken, the annealing recurrence --
and the float64 reference the GPU tests use (tests/toy_ladder_ref.py) against the unmodified oracle, with the input
conditions of its gradient cases.  No GPU: plans and arguments carry any non-NULL address where a pointer is checked,
and the trainer's methods run on stub dynamics."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib
from l2hmc_amd.dynamics_trainer import DynamicsTrainer, temperature_schedule
from tests import toy_cases as tc
from tests import toy_ladder_ref as TL
from tests.run_cases import PTR, header_text

_P, _I64, _F, _SZ = C.c_void_p, C.c_int64, C.c_float, C.c_size_t
NAME = "l2hmc_small_train_step_tempered"


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _net(dim, H):
    return _lib.DenseNet(D=dim, H=H, Ka=dim, Kb=dim, w1_t=PTR, wt=PTR, b1=PTR, wh_t=PTR, bh=PTR, whd_t=PTR, bhd=PTR,
                         coeff_s=PTR, coeff_q=PTR, q_tanh=1)


def _plan(dim=2, K=2, H=50, hmc=0):
    tgt = _lib.MogTarget(dim=dim, K=K, is_gaussian=0, temperature=1.0, mu=PTR, prec=PTR, log_const=PTR)
    return _lib.SmallPlan(x_dim=dim, num_nodes=H, trajectory_length=3, hmc=hmc, eps=0.1, first_layer_form=0, masks=PTR,
                          xnet=_net(dim, H), vnet=_net(dim, H), target=tgt)


def _step(L, plan, temps=PTR, stride=1, chains=4, rows=8, scale=0.1, x0=PTR, ws_bytes=1 << 30):
    return L.l2hmc_small_train_step_tempered(None if plan is None else C.byref(plan), temps, stride, chains, x0, PTR, PTR,
                                             rows, scale, 0.25, PTR, PTR, PTR, PTR, PTR, PTR, ws_bytes, None)


# ------------------------------------------------------------------------------------------------ the C entry
def test_header_declares_and_binding_matches(L):
    assert NAME in _lib.declared_symbols() and getattr(L, NAME) is not None
    assert L.l2hmc_abi_version() == 1
    sp = C.POINTER(_lib.SmallPlan)
    assert _lib._PROTOS[NAME] == (C.c_int, [sp, _P, _I64, _I64, _P, _P, _P, _I64, _F, _F, _P, _P, _P, _P, _P, _P, _SZ, _P])
    text = header_text()
    assert ("int l2hmc_small_train_step_tempered(const l2hmc_small_plan* plan, const float* temps, int64_t chain_stride, "
            "int64_t chains, const float* x0, const float* v0, const int32_t* dir, int64_t rows, float scale, "
            "float inv_count, float* x_out, float* v_out, float* p_accept, float* terms, float* grads, void* ws, "
            "size_t ws_bytes, l2hmc_stream_t stream);") in text
    # the scalar entry keeps its signature
    assert ("int l2hmc_small_train_step(const l2hmc_small_plan* plan, const float* x0, const float* v0, "
            "const int32_t* dir, int64_t rows, float scale, float inv_count,") in text
    comments = header_text(comments=True)
    assert "plan->target.temperature is IGNORED" in comments
    assert "VALUES of * temps are on the device and are not checked" in comments


def test_refusals_come_with_a_message_and_without_a_device(L):
    ok = _plan()
    who = "small_train_step_tempered"
    for kw, word in ((dict(temps=None), "NULL temps"), (dict(stride=-1), "chain_stride = -1"),
                     (dict(stride=2), "chain_stride = 2"), (dict(chains=0), "chains = 0"),
                     (dict(chains=-4), "chains = -4"), (dict(chains=3), "no whole number of chains = 3")):
        assert _step(L, ok, **kw) == 1, kw
        msg = L.l2hmc_last_error().decode()
        assert msg.startswith(who + ": ") and word in msg, (kw, msg)
    # ... and everything l2hmc_small_train_step refuses: no plan, an hmc plan, widths and dimensions past the limits, a bad
    # scale, rows < 0, a NULL pointer, a workspace that is too small
    assert _step(L, None) == 1 and "plan is NULL" in L.l2hmc_last_error().decode()
    assert _step(L, _plan(hmc=1)) == 1 and "hmc plans" in L.l2hmc_last_error().decode()
    for bad, word in ((dict(dim=9), "dim=9 (max 8)"), (dict(K=9), "K=9 (max 8)"), (dict(H=65), "num_nodes=65"),
                      (dict(H=0), "num_nodes=0")):
        assert _step(L, _plan(**bad)) == 1 and word in L.l2hmc_last_error().decode(), bad
    assert _step(L, ok, scale=0.) == 1 and "scale" in L.l2hmc_last_error().decode()
    assert _step(L, ok, rows=-8) == 1 and "bad rows" in L.l2hmc_last_error().decode()
    assert _step(L, ok, x0=None) == 1 and "NULL pointer" in L.l2hmc_last_error().decode()
    assert _step(L, ok, ws_bytes=16) == 3 and "workspace" in L.l2hmc_last_error().decode()
    with pytest.raises(ValueError, match="small_train_step_tempered: NULL temps"):
        _lib.check(_step(L, ok, temps=None))


def test_an_empty_batch_is_a_no_op(L):
    assert _step(L, _plan(), rows=0) == 0
    assert _step(L, _plan(), rows=0, temps=None) == 1 and _step(L, None, rows=0) == 1


# ------------------------------------------------------------------------------------------------ the trainer
def _stub_trainer(B=6, D=2, use_temperature=True):
    def no_draw(*_a):
        raise AssertionError("a draw was taken")
    dyn = types.SimpleNamespace(_device=torch.device("cpu"), x_dim=D, use_temperature=use_temperature, _draws=7,
                                temperature=1.0, _normal=no_draw, layered=False)
    tr = types.SimpleNamespace(dynamics=dyn)
    tr._chain_temperatures = lambda *a: DynamicsTrainer._chain_temperatures(tr, *a)
    return DynamicsTrainer, tr, np.zeros((B, D))


def test_temperature_parsing_takes_none_a_scalar_or_one_value_per_chain():
    DT, tr, _ = _stub_trainer()
    assert DT._chain_temperatures(tr, None, 6, "t") == (None, None)
    for scalar in (2.0, 3, np.float32(1.5), np.asarray(2.0), torch.tensor(2.0)):
        assert DT._chain_temperatures(tr, scalar, 6, "t") == (float(scalar), None)
    for arr in (TL.ladder(6), TL.ladder(6)[None, :], list(TL.ladder(6)), torch.tensor(TL.ladder(6))):
        s, got = DT._chain_temperatures(tr, arr, 6, "t")
        assert s is None and got.dtype == torch.float32 and tuple(got.shape) == (6,)
        np.testing.assert_array_equal(got.numpy(), TL.ladder(6).astype(np.float32))


@pytest.mark.parametrize("bad", [np.ones(5), np.ones(7), np.ones((2, 6)), np.ones((6, 1)), -np.ones(6), np.zeros(6),
                                 [1, 2, np.nan, 1, 1, 1], [1, 2, np.inf, 1, 1, 1], [1, 2, 1e-50, 1, 1, 1],
                                 np.ones((1, 1, 6)), 0.0, -1.0, float("nan"), float("inf"), 1e-50])
def test_a_bad_temperature_is_refused_before_any_draw(bad):
    DT, tr, x = _stub_trainer()
    with pytest.raises(ValueError, match="DynamicsTrainer.calc_loss_and_grads: "):
        DT.calc_loss_and_grads(tr, x, temperature=np.asarray(bad, dtype=np.float64) if np.ndim(bad) else bad)
    assert tr.dynamics._draws == 7 and tr.dynamics.temperature == 1.0


@pytest.mark.parametrize("temperature", [1.0, 2.5, TL.ladder(6)], ids=["one", "scalar", "ladder"])
def test_any_temperature_without_use_temperature_is_refused_before_any_draw(temperature):
    DT, tr, x = _stub_trainer(use_temperature=False)
    with pytest.raises(ValueError, match="temperature= on a Dynamics built with use_temperature=False"):
        DT.calc_loss_and_grads(tr, x, temperature=temperature)
    assert tr.dynamics._draws == 7


def _reference_loop(temp, steps, annealing_steps, factor):
    """mog_model.py:940-943 as written, for one number: -> the temperature each of `steps` steps runs at."""
    out = []
    for step in range(steps):
        out.append(temp)
        if step % annealing_steps == 0:
            temp_ = temp * factor
            if temp_ > 1.:
                temp = temp_
    return out


@pytest.mark.parametrize("annealing_steps,factor", [(1, 0.9), (3, 0.8), (2, 1.0), (200, 0.98)])
def test_temperature_schedule_is_the_reference_recurrence(annealing_steps, factor):
    assert DynamicsTrainer.temperature_schedule is temperature_schedule
    steps = 14
    want = _reference_loop(3.0, steps, annealing_steps, factor)
    got = [temperature_schedule(s, 3.0, annealing_steps, factor) for s in range(steps)]
    assert got == want and all(isinstance(g, float) for g in got)
    t0 = np.asarray([3.0, 1.0, 1.01, 10.0])                  # a rung at 1 stays at 1; one that cannot fall keeps its value
    want = np.stack([_reference_loop(float(t), steps, annealing_steps, factor) for t in t0], axis=1)
    got = np.stack([temperature_schedule(s, t0, annealing_steps, factor) for s in range(steps)])
    np.testing.assert_array_equal(got, want)
    assert (got[:, 1] == 1.0).all() and (got >= 1.0).all()
    if factor < 1:
        assert got[-1, 0] < 3.0 and (got[:, 2] == 1.01).all()
    np.testing.assert_array_equal(temperature_schedule(0, t0, annealing_steps, factor), t0)


# ------------------------------------------------------------------------------------------------ the reference
SMALL = TL.Case("mog", 10, 3, 0.1, 6, "mild", 0, False)


def _grads(tm):
    leaves = {"alpha": tm.alpha, **{f"xnet.{k}": v for k, v in tm.xnet.items()},
              **{f"vnet.{k}": v for k, v in tm.vnet.items()}}
    return {k: v.grad.clone() for k, v in leaves.items()}


def test_ladder_model_with_a_scalar_is_the_parent():
    from oracle.torch_ref import TorchDynamicsModel
    i = TL.inputs(SMALL)
    _, o, _ = TL.oracle_target(SMALL.kind)
    a = TL.model(SMALL, 1.7)
    b = TorchDynamicsModel(o, SMALL.N, SMALL.eps, i["masks"], i["xp"], i["vp"], temperature=1.7)
    outs = []
    for tm in (a, b):
        loss, *rest = tm.mog_loss(tc.t64(i["x"]), tc.t64(i["z"]), tuple(map(tc.t64, i["dx"])), tuple(map(tc.t64, i["dz"])),
                                  TL.SCALE)
        loss.backward()
        outs.append([loss.detach()] + [r.detach() for r in rest] + list(_grads(tm).values()))
    for got, want in zip(*outs):
        assert torch.equal(got, want)


def test_ladder_reference_is_the_oracle_rung_by_rung():
    """MoG, N = 3, B = 6, three temperatures in the fixed pattern: per-chain terms equal the unmodified oracle's run on
    each rung's chains, gradients the B_g / B-weighted sum of those runs, and a uniform temperature at the mean is far
    off."""
    from oracle.torch_ref import TorchDynamicsModel
    c = SMALL
    i = TL.inputs(c)
    _, o, _ = TL.oracle_target(c.kind)
    temps, rung = TL.ladder(c.B), TL.rung_of(c.B)
    assert sorted(set(rung)) == [0, 1, 2] and list(rung) == [0, 2, 1, 1, 0, 2]
    lad = TL.model(c, temps)
    rows, _, _ = TL.loss_rows(lad, i, c.B)
    rows.sum().backward()
    g_lad = _grads(lad)
    terms = rows.detach().numpy() * c.B
    acc = {k: torch.zeros_like(g) for k, g in g_lad.items()}
    for g in range(3):
        ch = np.nonzero(rung == g)[0]
        plain = TorchDynamicsModel(o, c.N, c.eps, i["masks"], i["xp"], i["vp"], temperature=float(temps[ch[0]]))
        sub = dict(x=i["x"][ch], z=i["z"][ch], dx=tuple(a[ch] for a in i["dx"]), dz=tuple(a[ch] for a in i["dz"]))
        r_g, _, _ = TL.loss_rows(plain, sub, len(ch))
        r_g.sum().backward()
        np.testing.assert_allclose(terms[np.concatenate([ch, c.B + ch])], r_g.detach().numpy() * len(ch), rtol=1e-13)
        for k, v in _grads(plain).items():
            acc[k] += v * (len(ch) / c.B)
    for k in g_lad:
        assert float((g_lad[k] - acc[k]).abs().max()) <= 1e-12 * float(acc[k].abs().max()), k
    uni = TL.model(c, float(temps.mean()))
    TL.loss_rows(uni, i, c.B)[0].sum().backward()
    far = [float((g_lad[k] - v).abs().max() / g_lad[k].abs().max()) for k, v in _grads(uni).items()]
    assert min(far) > 10 * tc.TOL_G, far        # a kernel that ignores the chain axis misses the GPU gate tenfold


def test_batches_put_a_chains_two_rows_in_different_slots():
    for B in (37, 9):
        assert all((B + i) % 16 != i % 16 for i in range(B))
    assert TL.MOG.B == TL.MOG_LAYERED.B == 37 and -(-2 * 37 // 16) == 5 and (2 * 37) % 16 != 0
    assert TL.MOG_16.B == 16 and {c.B for c in TL.ONE_LAUNCH_CASES + TL.LAYERED_CASES} >= {37, 9, 16}
    for c in TL.ONE_LAUNCH_CASES + TL.LAYERED_CASES:
        assert sorted(set(TL.rung_of(c.B))) == [0, 1, 2]
        lad = TL.ladder(c.B)
        np.testing.assert_array_equal(lad, lad.astype(np.float32).astype(np.float64))
        i = TL.inputs(c)
        for bits in (i["dx"][2], i["dz"][2]):
            assert 0 < bits.sum() < c.B                                                  # both directions run


@pytest.mark.parametrize("c", TL.GRADIENT_CASES + [TL.QUARTIC], ids=TL.case_id)
def test_gradient_cases_meet_the_input_conditions(c):
    """toy_cases' conditions, for the ladder each case trains on, over ALL rows: no hidden pre-activation within
    RELU_MARGIN of 0, no H0 - H1 + logdet within MIN_MARGIN of 0, and no gradient tensor whose largest entry is a
    cancellation of the chains' shares beyond CANCELLATION."""
    relu, arg = TL.margins(c, TL.ladder(c.B))
    assert relu > tc.RELU_MARGIN and arg > tc.MIN_MARGIN, (relu, arg)
    tm = TL.model(c, TL.ladder(c.B))
    rows, _, p = TL.loss_rows(tm, TL.inputs(c), c.B)
    assert abs(float(rows.sum().detach()) - TL.reference(c)[1]) < 1e-9
    assert float(p.mean().detach()) > 0.01, "the case must accept"
    worst = {k: v for k, v in tc.cancellation(tm, rows).items() if not v <= tc.CANCELLATION}
    assert not worst, worst
