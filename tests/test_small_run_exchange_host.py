"""Host side of replica exchange INSIDE the one-launch L2HMC toy-target run: the C entry l2hmc_small_run_exchange
(l2hmc_amd/csrc/small_mlp.hip: the EXCHANGE instances of small_traj_mfma_kernel, the round of small_swap.h) and its
binding, the argument checks that fail before any device call, and what `DynamicsSampler.in_launch`,
`exchange_in_launch` and `run_exchange` serve and refuse.  No GPU: arguments carry any non-NULL address where a pointer
is checked and the sampler runs on stub dynamics that must not be asked for a plan."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
ENTRY = "l2hmc_small_run_exchange"


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _target(dim=2, K=1, kind=1, temperature=1.0, mu=PTR):
    return _lib.MogTarget(dim=dim, K=K, is_gaussian=kind, temperature=temperature, mu=mu, prec=PTR, log_const=PTR)


def _net(D=2, H=10, w=PTR):
    return _lib.DenseNet(D=D, Ka=D, Kb=D, H=H, q_tanh=1, w1_t=w, wt=PTR, b1=PTR, wh_t=PTR, bh=PTR, whd_t=PTR, bhd=PTR,
                         coeff_s=PTR, coeff_q=PTR)


def _plan(x_dim=2, hmc=0, N=5, masks=PTR, target=None, num_nodes=10, form=0, net=None):
    net = net if net is not None else _net(x_dim, num_nodes)
    return _lib.SmallPlan(x_dim=x_dim, num_nodes=num_nodes, trajectory_length=N, hmc=hmc, eps=0.1,
                          first_layer_form=form, masks=masks, target=target if target is not None else _target(),
                          xnet=net, vnet=net)


def _run(L, plan, x_in=PTR, x_next=PTR, B=8, draw0=0, n_steps=3, temps=PTR, step_stride=0, chain_stride=1, group=4,
         swap_every=1, swap_phase=0, first_parity=0):
    return getattr(L, ENTRY)(None if plan is None else C.byref(plan), x_in, x_next, B, 42, draw0, n_steps, temps,
                             step_stride, chain_stride, group, swap_every, swap_phase, first_parity, None, None, None,
                             None, None, None, None)


# ------------------------------------------------------------------------------------------------ the C entry
def test_header_declares_and_binding_matches():
    assert ENTRY in set(_lib.declared_symbols())
    # plan, x_in, x_next, B, seed, draw0, n_steps, temps, step_stride, chain_stride, group, swap_every, swap_phase,
    # first_parity, replica, px, samples, swap_p, swapped, replica_hist, stream
    assert _lib._PROTOS[ENTRY] == (
        C.c_int, [C.POINTER(_lib.SmallPlan), _P, _P, _I64, _U64, _U64, _I32, _P, _I64, _I64, _I32, _I32, _I32, _I32,
                  _P, _P, _P, _P, _P, _P, _P])
    text = header_text()
    decl = ("int l2hmc_small_run_exchange(const l2hmc_small_plan* plan, const float* x_in, float* x_next, int64_t B, "
            "uint64_t seed, uint64_t draw0, int32_t n_steps, const float* temps, int64_t step_stride, "
            "int64_t chain_stride, int32_t group, int32_t swap_every, int32_t swap_phase, int32_t first_parity, "
            "int32_t* replica, float* px, float* samples, float* swap_p, uint8_t* swapped, int32_t* replica_hist, "
            "l2hmc_stream_t stream);")
    assert decl in text
    assert decl.count(",") + 1 == len(_lib._PROTOS[ENTRY][1])            # the header's arity
    assert "#define L2HMC_ABI_VERSION 1" in text
    classes = header_text(comments=True).split("int l2hmc_profile_begin")[0].rsplit("8 =", 1)[1]
    assert ENTRY in classes and "class-7" in classes


def test_library_exports_the_entry(L):
    assert getattr(L, ENTRY) is not None
    assert L.l2hmc_abi_version() == 1


TARGET_REFUSALS = [(dict(x_dim=3, net=_net(3)), "x_dim=3 != target dim=2"),
                   (dict(x_dim=9, target=_target(dim=9), net=_net(9)), "target dim=9 (max 8)"),
                   (dict(target=_target(K=9)), "K=9 (max 8)"),
                   (dict(target=_target(kind=4)), "target kind 4 unknown"),
                   (dict(target=_target(temperature=0.0)), "temperature must be > 0"),
                   (dict(target=_target(mu=None)), "NULL parameter pointer")]


def test_the_run_refuses_bad_arguments_before_any_device_call(L):
    """Every case returns L2HMC_ERR_ARG with a worded message; none reaches a launch (the pointers are not memory)."""
    ok = _plan()
    # what l2hmc_small_run_tempered refuses ...
    cases = [(dict(plan=None), "plan is NULL"), (dict(x_in=None), "x_in / x_next is NULL"),
             (dict(x_next=None), "x_in / x_next is NULL"), (dict(B=-8), "B < 0"),
             (dict(n_steps=0), "n_steps=0"), (dict(n_steps=-1), "n_steps=-1"),
             (dict(plan=_plan(hmc=1)), "plain-HMC sampler"),
             (dict(step_stride=-1), "negative stride"), (dict(chain_stride=-1), "negative stride"),
             (dict(draw0=2 ** 64 - 8, n_steps=2), "draw0 + 4 * n_steps overflows 64 bits"),
             (dict(temps=None), "temps is NULL"),
             (dict(plan=_plan(N=0)), "bad trajectory_length / masks"),
             (dict(plan=_plan(masks=None)), "bad trajectory_length / masks"),
             (dict(plan=_plan(num_nodes=65, net=_net(2, 65))), "num_nodes=65 unsupported"),
             (dict(plan=_plan(num_nodes=0, net=_net(2, 0))), "num_nodes=0 unsupported"),
             (dict(plan=_plan(net=_net(2, 12))), "net shape"),
             (dict(plan=_plan(net=_net(w=None))), "NULL weight pointer"),
             (dict(plan=_plan(form=4)), "first_layer_form=4"), (dict(plan=_plan(form=-1)), "first_layer_form=-1"),
             # ... and what the schedule adds
             (dict(group=1), "group = 1"), (dict(group=0), "group = 0"), (dict(group=-4), "group = -4"),
             (dict(group=9, B=18), "group = 9"), (dict(group=16, B=16), "group = 16"),
             (dict(group=64, B=64), "group = 64"),
             (dict(B=7), "not a multiple"), (dict(B=6), "not a multiple"), (dict(B=8, group=3), "not a multiple"),
             (dict(swap_every=0), "swap_every = 0"), (dict(swap_every=-2), "swap_every = -2"),
             (dict(swap_phase=-1), "swap_phase = -1"), (dict(swap_phase=1), "swap_phase = 1"),
             (dict(swap_every=3, swap_phase=3), "swap_phase = 3"),
             (dict(first_parity=2), "first_parity = 2"), (dict(first_parity=-1), "first_parity = -1"),
             # 4 * 3 steps fit below 2^64 - 1, their three rounds do not
             (dict(draw0=2 ** 64 - 15, n_steps=3), "draw0 + 4 * n_steps + rounds overflows")]
    cases += [(dict(plan=_plan(**kw)), word) for kw, word in TARGET_REFUSALS]
    for kw, word in cases:
        plan = kw.pop("plan", ok)
        rc = _run(L, plan, **kw)
        msg = L.l2hmc_last_error().decode()
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        assert msg.startswith("small_run_exchange: ") and word in msg, (kw, msg)
    with pytest.raises(ValueError, match="small_run_exchange: group = 9"):
        _lib.check(_run(L, ok, group=9, B=9))


def test_a_round_takes_its_stream_whatever_the_group_and_an_empty_batch_is_a_no_op(L):
    """3 steps with a round after each take streams draw0 .. draw0 + 14, group 2 (a round without a pair) included;
    with swap_every = 4 and phase 0 the launch has no round and needs 12."""
    for group in (2, 3, 4, 8):
        assert _run(L, _plan(), B=0, group=group) == 0
        assert _run(L, _plan(), B=0, draw0=2 ** 64 - 16, n_steps=3, group=group) == 0       # streams up to 2^64 - 2
        assert _run(L, _plan(), B=0, draw0=2 ** 64 - 15, n_steps=3, group=group) == 1
        assert _run(L, _plan(), B=0, draw0=2 ** 64 - 13, n_steps=3, group=group, swap_every=4) == 0
        assert _run(L, _plan(), B=0, draw0=2 ** 64 - 13, n_steps=3, group=group, swap_every=4, swap_phase=1) == 1
    assert _run(L, _plan(hmc=1), B=0) == 1                                # checked before the batch size is looked at
    assert _run(L, _plan(), B=0, group=9) == 1
    assert _run(L, _plan(), B=0, temps=None) == 1


# ------------------------------------------------------------------------------------------------ the sampler on stubs
B_, D_ = 16, 2


def _stub(hmc=False, layered=False, use_temperature=True):
    def _plan_():
        raise AssertionError("a refused call must not build a plan")
    return types.SimpleNamespace(hmc=hmc, layered=layered, x_dim=D_, trajectory_length=5, temperature=1.0,
                                 use_temperature=use_temperature, _draws=4, _seed=7, _device=torch.device("cpu"),
                                 _plan=_plan_)


def _sampler(dyn, in_launch=True):
    import l2hmc_amd as la
    smp = la.DynamicsSampler(dyn)
    assert smp.in_launch is False                      # the default: the round between launches
    smp.in_launch = in_launch
    return smp


TEMPS = np.linspace(1.0, 4.5, B_)[None, :]


def test_exchange_in_launch_says_what_is_served():
    smp = _sampler(_stub())
    assert [G for G in range(0, 12) if smp.exchange_in_launch(G)] == [2, 3, 4, 5, 6, 7, 8]
    assert not smp.exchange_in_launch(9) and not smp.exchange_in_launch(64)
    assert not smp.exchange_in_launch(2.5) and not smp.exchange_in_launch(None)
    assert smp.exchange_in_launch(np.int64(4))
    assert smp.MAX_REPLICAS_IN_LAUNCH == 8 and smp.MAX_REPLICAS == 64
    for dyn in (_stub(hmc=True), _stub(layered=True)):
        assert not any(_sampler(dyn).exchange_in_launch(G) for G in range(2, 9))
    smp = _sampler(_stub())
    smp.steps_per_launch = 1
    assert not any(smp.exchange_in_launch(G) for G in range(2, 9))
    # what it says does not depend on the attribute it is about
    assert _sampler(_stub(), in_launch=False).exchange_in_launch(8)


def test_a_group_the_launch_does_not_hold_is_refused_before_any_launch():
    x0 = torch.zeros(B_, D_)
    dyn = _stub()
    with pytest.raises(NotImplementedError, match=r"run_exchange with in_launch = True: replicas=16.*8 rungs at the most"):
        _sampler(dyn).run_exchange(5, x0, temperature=TEMPS, replicas=16)
    with pytest.raises(NotImplementedError, match="replicas=16"):      # an empty run does not hide the limit
        _sampler(dyn).run_exchange(0, x0, temperature=TEMPS, replicas=16)
    assert dyn._draws == 4
    # the default serves it: it gets as far as the plan
    with pytest.raises(AssertionError, match="must not build a plan"):
        _sampler(dyn, in_launch=False).run_exchange(5, x0, temperature=TEMPS, replicas=16)


def test_the_existing_refusals_come_first_and_before_the_device():
    x0 = torch.zeros(B_, D_)
    for kw, word in ((dict(temperature=None, replicas=4), "without temperature="),
                     (dict(replicas=3), "no whole number of groups"), (dict(replicas=5), "no whole number of groups"),
                     (dict(replicas=32), "no whole number of groups"),         # not the NotImplementedError: B = 16
                     (dict(replicas=65), "replicas=65"), (dict(replicas=1), "2 rungs or more"),
                     (dict(replicas=2.5), "whole numbers"), (dict(replicas=4, swap_every=0), "swap_every=0"),
                     (dict(replicas=4, first_parity=2), "parity"),
                     (dict(replicas=4, replica0=np.arange(B_)), "replica0"),
                     (dict(replicas=4, temperature=0.0), "temperature")):
        dyn = _stub()
        args = dict(temperature=TEMPS)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            _sampler(dyn).run_exchange(5, x0, **args)
        assert dyn._draws == 4
    with pytest.raises(ValueError, match="`run_hmc_exchange`"):
        _sampler(_stub(hmc=True)).run_exchange(5, x0, temperature=TEMPS, replicas=4)
    with pytest.raises(NotImplementedError, match="run_exchange: "):
        _sampler(_stub(layered=True)).run_exchange(5, x0, temperature=TEMPS, replicas=4)
    smp = _sampler(_stub())
    smp.steps_per_launch = 1
    with pytest.raises(NotImplementedError, match="run_exchange: "):
        smp.run_exchange(5, x0, temperature=TEMPS, replicas=4)


def test_good_arguments_get_as_far_as_the_plan_and_an_empty_run_is_empty():
    x0 = torch.ones(B_, D_)
    for kw in (dict(replicas=2), dict(replicas=4, swap_every=3, first_parity=1), dict(replicas=8),
               dict(replicas=8, replica0=np.arange(B_, dtype=np.int32)), dict(replicas=np.int64(4)),
               dict(replicas=4, temperature=np.ones((5, B_)))):
        dyn = _stub()
        args = dict(temperature=TEMPS)
        args.update(kw)
        with pytest.raises(AssertionError, match="must not build a plan"):
            _sampler(dyn).run_exchange(5, x0, **args)
        assert dyn._draws == 4
    dyn = _stub()
    out = _sampler(dyn).run_exchange(0, x0, temperature=TEMPS, replicas=4)
    assert out["swap_p"].shape == (0, B_) and out["swapped"].dtype == np.bool_ and out["replica"].dtype == np.int32
    assert out["px"].shape == (0, B_) and torch.equal(out["samples_out"], x0) and dyn._draws == 4
    # without replicas it is `run`, whatever the attribute says: the stub is asked for its plan by `run` itself
    with pytest.raises(AssertionError, match="must not build a plan"):
        _sampler(dyn).run_exchange(5, x0, temperature=TEMPS, replicas=None, swap_every=0)
