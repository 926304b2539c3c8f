"""Host side of autograd with a chain axis: the four C entries (l2hmc_gauge_accept_backward_ladder,
l2hmc_gauge_transition_ladder, l2hmc_small_trajectory_tempered, l2hmc_small_vjp_tempered) exist, are bound, and refuse
bad arguments before any device call; `GaugeDynamics.apply_transition(x, beta)` with a beta per chain and `propose` /
`Dynamics.forward / .backward / .both(..., temperature=)` refuse what they do not take before a draw is taken.  No GPU:
plans and arguments carry any non-NULL address, the Python callers run on stubs."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib
from tests import toy_ladder_ref as TL
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
NAMES = ("l2hmc_gauge_accept_backward_ladder", "l2hmc_gauge_transition_ladder", "l2hmc_small_trajectory_tempered",
         "l2hmc_small_vjp_tempered")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the C entries
def test_the_four_symbols_exist_and_are_bound(L):
    declared = set(_lib.declared_symbols())
    for name in NAMES:
        assert name in declared and name in _lib._PROTOS and getattr(L, name) is not None, name
    gp, sp = C.POINTER(_lib.GaugePlan), C.POINTER(_lib.SmallPlan)
    assert _lib._PROTOS[NAMES[0]] == (C.c_int, [_I32, _I32, _P, _I64, _I64, _I64] + [_P] * 15 + [_P])
    assert _lib._PROTOS[NAMES[1]] == (C.c_int, [gp, _P, _I64] + [_P] * 5 + [_I64, _I32] + [_P] * 4 + [_P, _SZ, _P])
    assert _lib._PROTOS[NAMES[2]] == (C.c_int, [sp, _P, _I64, _I64, _P, _P, _P, _I64] + [_P] * 4 + [_P])
    assert _lib._PROTOS[NAMES[3]] == (C.c_int, [sp, _P, _I64, _I64, _P, _P, _P, _I64] + [_P] * 11 + [_P, _SZ, _P])
    text = header_text()
    for start in ("int l2hmc_gauge_accept_backward_ladder(int32_t T, int32_t X, const float* betas, int64_t chain_stride, "
                  "int64_t chains, int64_t rows,",
                  "int l2hmc_gauge_transition_ladder(const l2hmc_gauge_plan* plan, const float* betas, "
                  "int64_t chain_stride, const float* x,",
                  "int l2hmc_small_trajectory_tempered(const l2hmc_small_plan* plan, const float* temps, "
                  "int64_t chain_stride, int64_t chains, const float* x0,",
                  "int l2hmc_small_vjp_tempered(const l2hmc_small_plan* plan, const float* temps, int64_t chain_stride, "
                  "int64_t chains, const float* x0,",
                  # the scalar twins keep their signatures
                  "int l2hmc_gauge_accept_backward(int32_t T, int32_t X, float beta, int64_t rows,",
                  "int l2hmc_gauge_transition(const l2hmc_gauge_plan* plan, float beta, const float* x,",
                  "int l2hmc_small_trajectory(const l2hmc_small_plan* plan, const float* x0,",
                  "int l2hmc_small_vjp(const l2hmc_small_plan* plan, const float* x0,"):
        assert start in text, start


def _accept(L, betas=PTR, stride=1, chains=4, rows=8, T=3, X=5, x0=PTR):
    return L.l2hmc_gauge_accept_backward_ladder(T, X, betas, stride, chains, rows, x0, PTR, PTR, PTR, PTR, PTR, None,
                                                None, None, None, PTR, PTR, PTR, None, None, None)


def _gauge_net(D=128, H=512):
    return _lib.DenseNet(D=D, H=H, Ka=D, Kb=D, w1_t=PTR, wt=PTR, b1=PTR, wh_t=PTR, bh=PTR, whd_t=PTR, bhd=PTR,
                         coeff_s=PTR, coeff_q=PTR)


def _gauge_plan(hmc=0, flags=0, masks=PTR):
    return _lib.GaugePlan(T=8, X=8, num_steps=3, hmc=hmc, eps=0.1, flags=flags, masks=masks, xnet=_gauge_net(),
                          vnet=_gauge_net())


def _transition(L, plan, betas=PTR, stride=1, B=4, x=PTR, ws_bytes=0):
    return L.l2hmc_gauge_transition_ladder(None if plan is None else C.byref(plan), betas, stride, x, PTR, PTR, PTR, PTR,
                                           B, 1, PTR, PTR, PTR, PTR, PTR, ws_bytes, None)


def _small_net(dim, H):
    return _lib.DenseNet(D=dim, H=H, Ka=dim, Kb=dim, w1_t=PTR, wt=PTR, b1=PTR, wh_t=PTR, bh=PTR, whd_t=PTR, bhd=PTR,
                         coeff_s=PTR, coeff_q=PTR, q_tanh=1)


def _small_plan(dim=2, K=2, H=50, hmc=0, form=0):
    tgt = _lib.MogTarget(dim=dim, K=K, is_gaussian=0, temperature=1.0, mu=PTR, prec=PTR, log_const=PTR)
    return _lib.SmallPlan(x_dim=dim, num_nodes=H, trajectory_length=3, hmc=hmc, eps=0.1, first_layer_form=form, masks=PTR,
                          xnet=_small_net(dim, H), vnet=_small_net(dim, H), target=tgt)


def _trajectory(L, plan, temps=PTR, stride=1, chains=4, rows=8, x0=PTR):
    return L.l2hmc_small_trajectory_tempered(None if plan is None else C.byref(plan), temps, stride, chains, x0, PTR,
                                             None, rows, PTR, PTR, PTR, PTR, None)


def _vjp(L, plan, temps=PTR, stride=1, chains=4, rows=8, x0=PTR, ws_bytes=1 << 30):
    return L.l2hmc_small_vjp_tempered(None if plan is None else C.byref(plan), temps, stride, chains, x0, PTR, None, rows,
                                      None, None, None, None, None, None, PTR, None, None, None, None, PTR, ws_bytes,
                                      None)


LADDER_REFUSALS = ((dict(stride=2), "chain_stride = 2"), (dict(stride=-1), "chain_stride = -1"),
                   (dict(chains=0), "chains = 0"), (dict(chains=3), "no whole number of chains = 3"))


def _refused(L, rc, who, word):
    msg = L.l2hmc_last_error().decode()
    assert rc == 1 and msg.startswith(who + ": ") and word in msg, (rc, msg, word)


def test_accept_backward_ladder_refuses_before_any_device_call(L):
    who = "accept_backward_ladder"
    _refused(L, _accept(L, betas=None), who, "NULL betas")
    for kw, word in LADDER_REFUSALS:
        _refused(L, _accept(L, **kw), who, word)
    # ... and everything the scalar entry refuses
    _refused(L, _accept(L, T=0), who, "bad arguments")
    _refused(L, _accept(L, x0=None), who, "NULL pointer")
    _refused(L, _accept(L, T=128, X=64), who, "LDS")
    assert _accept(L, rows=0) == 0
    assert _accept(L, rows=0, betas=None) == 1 and _accept(L, rows=0, chains=0) == 1
    with pytest.raises(ValueError, match="accept_backward_ladder: NULL betas"):
        _lib.check(_accept(L, betas=None))
    # the scalar entry's messages are what they were
    assert L.l2hmc_gauge_accept_backward(3, 5, 1.0, 4, None, *[None] * 14, None) == 1
    assert L.l2hmc_last_error().decode() == "accept_backward: NULL pointer"


@pytest.mark.parametrize("flags", [0, _lib.PLAN_LAYERED, _lib.PLAN_SELECTED_ONLY])
def test_transition_ladder_refuses_before_any_device_call(L, flags):
    who = "gauge_transition_ladder"
    ok = _gauge_plan(flags=flags)
    _refused(L, _transition(L, ok, betas=None), who, "NULL betas")
    _refused(L, _transition(L, ok, stride=2), who, "chain_stride = 2")
    _refused(L, _transition(L, ok, stride=-1), who, "chain_stride = -1")
    _refused(L, _transition(L, _gauge_plan(hmc=1, flags=flags)), who, "l2hmc_gauge_hmc_run_ladder")
    _refused(L, _transition(L, None), who, "plan is NULL")
    _refused(L, _transition(L, ok, B=-1), who, "B < 0")
    _refused(L, _transition(L, ok, x=None), who, "NULL pointer")
    assert _transition(L, _gauge_plan(flags=flags, masks=None)) == 1 and "masks" in L.l2hmc_last_error().decode()
    # the workspace is the scalar entry's, and a short one is refused on the host whatever the plan's fused flag says
    assert _transition(L, ok, ws_bytes=16) == 3
    msg = L.l2hmc_last_error().decode()
    assert msg.startswith(who + ": workspace 16 < ") and str(L.l2hmc_gauge_transition_ws_bytes(C.byref(ok), 4, 1)) in msg
    assert _transition(L, ok, B=0) == 0
    assert _transition(L, ok, B=0, betas=None) == 1 and _transition(L, _gauge_plan(hmc=1), B=0) == 1


@pytest.mark.parametrize("entry,who", [(_trajectory, "small_trajectory_tempered"), (_vjp, "small_vjp_tempered")])
def test_the_tempered_entries_refuse_before_any_device_call(L, entry, who):
    ok = _small_plan()
    _refused(L, entry(L, ok, temps=None), who, "NULL temps")
    for kw, word in LADDER_REFUSALS:
        _refused(L, entry(L, ok, **kw), who, word)
    # ... and everything the scalar twin refuses
    _refused(L, entry(L, None), who, "plan is NULL")
    _refused(L, entry(L, ok, rows=-8), who, "rows")
    _refused(L, entry(L, ok, x0=None), who, "NULL pointer")
    for bad, word in ((dict(dim=9), "dim=9 (max 8)"), (dict(K=9), "K=9 (max 8)"), (dict(H=65), "num_nodes=65")):
        assert entry(L, _small_plan(**bad)) == 1 and word in L.l2hmc_last_error().decode(), bad
    assert entry(L, ok, rows=0) == 0
    assert entry(L, ok, rows=0, temps=None) == 1 and entry(L, ok, rows=0, chains=0) == 1 and entry(L, None, rows=0) == 1


def test_the_two_tempered_entries_differ_where_their_twins_do(L):
    assert _vjp(L, _small_plan(hmc=1)) == 1 and "hmc plans" in L.l2hmc_last_error().decode()
    assert _vjp(L, _small_plan(), ws_bytes=16) == 3 and "small_vjp_tempered: workspace" in L.l2hmc_last_error().decode()
    assert _trajectory(L, _small_plan(form=4)) == 1 and "first_layer_form=4" in L.l2hmc_last_error().decode()
    assert _trajectory(L, _small_plan(hmc=1), rows=0) == 0          # an hmc plan is served


# ------------------------------------------------------------------------------------------------ GaugeDynamics
T_, X_, B_ = 8, 8, 4
D_ = 2 * T_ * X_


def _gauge_stub(hmc=False):
    from l2hmc_amd.gauge_dynamics import GaugeDynamics

    def no_draw(*_a):
        raise AssertionError("a draw was taken")

    def no_plan():
        raise AssertionError("a refused call must not build a plan")
    lat = types.SimpleNamespace(time_size=T_, space_size=X_)
    dyn = types.SimpleNamespace(hmc=hmc, lattice=lat, x_dim=D_, batch_size=B_, num_steps=3, eps=torch.tensor(0.1),
                                _draws=4, _seed=7, _device=torch.device("cpu"), _plan=no_plan, _normal=no_draw,
                                _uniform=no_draw, check_numerics=False)
    dyn._x = lambda a: GaugeDynamics._x(dyn, a)
    dyn._beta = lambda *a: GaugeDynamics._beta(dyn, *a)
    return GaugeDynamics, dyn


def test_signatures():
    import l2hmc_amd as la
    assert (str(inspect.signature(la.GaugeDynamics.apply_transition))
            == "(self, position, beta, momentum_f=None, momentum_b=None, coin=None, u=None)")
    assert (str(inspect.signature(la.propose))
            == "(x, dynamics, init_v=None, aux=None, do_mh_step=False, log_jac=False, *, init_v_backward=None, "
               "dir_bits=None, u=None, temperature=None)")
    for fn in (la.Dynamics.forward, la.Dynamics.backward, la.Dynamics.both):
        assert str(inspect.signature(fn)).endswith("log_jac=False, temperature=None)")
    assert str(inspect.signature(la.GaugeDynamics.transition_kernel)).startswith("(self, position, beta, forward=True")


@pytest.mark.parametrize("beta", [np.ones(B_ + 1), np.ones((2, B_)), np.ones((B_, 1)), np.ones((1, 1, B_)),
                                  [1.0, -1.0, 1.0, 1.0], [1.0, float("nan"), 1.0, 1.0], [[1.0, 1.0, float("inf"), 1.0]],
                                  [1.0, 1e60, 1.0, 1.0], torch.ones(B_ + 1), torch.tensor([1.0, 2.0, -3.0, 1.0])])
@pytest.mark.parametrize("grad", [False, True])
def test_bad_beta_ladders_are_refused_before_any_draw(beta, grad):
    GD, dyn = _gauge_stub()
    x = torch.zeros(B_, D_, requires_grad=grad)
    with pytest.raises(ValueError, match="apply_transition: (beta of shape|every beta)"):
        GD.apply_transition(dyn, x, beta)
    assert dyn._draws == 4


def test_a_beta_ladder_that_requires_grad_is_refused_and_says_why():
    GD, dyn = _gauge_stub()
    with pytest.raises(ValueError, match="not differentiated"):
        GD.apply_transition(dyn, torch.zeros(B_, D_), torch.ones(B_, requires_grad=True))
    assert dyn._draws == 4


def test_a_beta_ladder_on_plain_hmc_is_not_implemented():
    GD, dyn = _gauge_stub(hmc=True)
    for beta in (np.ones(B_), np.ones((1, B_)), torch.ones(B_)):
        with pytest.raises(NotImplementedError, match="hmc=True"):
            GD.apply_transition(dyn, torch.zeros(B_, D_), beta)
    assert dyn._draws == 4


def test_accepted_betas_get_as_far_as_the_draws():
    """A scalar in any of the forms float() takes is the scalar call it was; a ladder in any accepted form passes the
    host checks (the stub has no device: the first draw ends the call)."""
    for beta in (2.0, 3, np.float32(1.5), np.asarray(2.0), torch.tensor(2.0)):
        GD, dyn = _gauge_stub()
        assert GD._beta(dyn, beta, B_) == (beta, None)
    GD, dyn = _gauge_stub()
    assert GD._beta(dyn, [2.0], B_)[1] is None and GD._beta(dyn, torch.tensor([2.0]), B_)[1] is None
    for beta in (np.ones(B_), np.ones((1, B_)), [1.0, 2.0, 3.0, 0.0], torch.ones(1, B_, dtype=torch.float64)):
        GD, dyn = _gauge_stub()
        scalar, ladder = GD._beta(dyn, beta, B_)
        assert scalar is None and ladder.dtype == torch.float32 and tuple(ladder.shape) == (B_,)
        with pytest.raises(AssertionError, match="a draw was taken"):
            with torch.no_grad():
                GD.apply_transition(dyn, torch.zeros(B_, D_), beta, momentum_f=np.zeros((B_, D_)))


# ------------------------------------------------------------------------------------------------ Dynamics / propose
def _toy_stub(B=6, D=2, use_temperature=True, layered=False, hmc=False):
    from l2hmc_amd.dynamics import Dynamics

    def no_draw(*_a):
        raise AssertionError("a draw was taken")

    def no_plan(*_a):
        raise AssertionError("a refused call must not build a plan")
    dyn = types.SimpleNamespace(_device=torch.device("cpu"), x_dim=D, use_temperature=use_temperature, _draws=7, _seed=3,
                                temperature=1.0, _normal=no_draw, layered=layered, hmc=hmc, _plan=no_plan,
                                alpha=torch.tensor(0.1))
    for name in ("_chain_temperatures", "_call_temperature", "_run"):
        setattr(dyn, name, (lambda n: lambda *a, **k: getattr(Dynamics, n)(dyn, *a, **k))(name))
    return Dynamics, dyn, np.zeros((B, D))


def _toy_calls(Dyn, dyn, x, temperature):
    import l2hmc_amd as la
    return (lambda: la.propose(x, dyn, temperature=temperature),
            lambda: la.propose(x, dyn, do_mh_step=True, init_v=x, temperature=temperature),
            lambda: Dyn.forward(dyn, x, temperature=temperature),
            lambda: Dyn.backward(dyn, x, log_jac=True, temperature=temperature),
            lambda: Dyn.both(dyn, x, temperature=temperature))


@pytest.mark.parametrize("bad", [np.ones(5), np.ones(7), np.ones((2, 6)), np.ones((6, 1)), -np.ones(6), np.zeros(6),
                                 [1, 2, np.nan, 1, 1, 1], [1, 2, np.inf, 1, 1, 1], [1, 2, 1e-50, 1, 1, 1],
                                 np.ones((1, 1, 6)), 0.0, -1.0, float("nan"), float("inf"), 1e-50])
def test_a_bad_temperature_is_refused_before_any_draw(bad):
    Dyn, dyn, x = _toy_stub()
    bad = np.asarray(bad, dtype=np.float64) if np.ndim(bad) else bad
    for call in _toy_calls(Dyn, dyn, x, bad):
        with pytest.raises(ValueError, match="(propose|Dynamics.forward|Dynamics.backward|Dynamics.both): "):
            call()
    assert dyn._draws == 7 and dyn.temperature == 1.0


@pytest.mark.parametrize("temperature", [1.0, 2.5, TL.ladder(6)], ids=["one", "scalar", "ladder"])
def test_any_temperature_without_use_temperature_is_refused_before_any_draw(temperature):
    Dyn, dyn, x = _toy_stub(use_temperature=False)
    for call in _toy_calls(Dyn, dyn, x, temperature):
        with pytest.raises(ValueError, match="temperature= on a Dynamics built with use_temperature=False"):
            call()
    assert dyn._draws == 7


def test_a_temperature_ladder_that_requires_grad_is_refused_and_says_why():
    Dyn, dyn, x = _toy_stub()
    for call in _toy_calls(Dyn, dyn, x, torch.ones(6, requires_grad=True)):
        with pytest.raises(ValueError, match="not differentiated"):
            call()
    assert dyn._draws == 7


def test_a_temperature_ladder_on_a_layered_dynamics_is_not_implemented():
    Dyn, dyn, x = _toy_stub(layered=True)
    for call in _toy_calls(Dyn, dyn, x, TL.ladder(6)):
        with pytest.raises(NotImplementedError, match="layer by layer"):
            call()
    assert dyn._draws == 7


def test_accepted_temperatures_get_as_far_as_the_draws():
    Dyn, dyn, x = _toy_stub()
    assert Dyn._call_temperature(dyn, None, 6, "t") is None
    for scalar in (2.0, 3, np.float32(1.5), np.asarray(2.0), torch.tensor(2.0)):
        assert Dyn._call_temperature(dyn, scalar, 6, "t") == float(scalar)
    for arr in (TL.ladder(6), TL.ladder(6)[None, :], list(TL.ladder(6)), torch.tensor(TL.ladder(6))):
        got = Dyn._call_temperature(dyn, arr, 6, "t")
        assert got.dtype == torch.float32 and tuple(got.shape) == (6,)
        np.testing.assert_array_equal(got.numpy(), TL.ladder(6).astype(np.float32))
        with pytest.raises(AssertionError, match="a draw was taken"):
            with torch.no_grad():
                Dyn.forward(dyn, x, temperature=arr)
    assert dyn._draws == 7 and dyn.temperature == 1.0
