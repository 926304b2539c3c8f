"""Host side of annealed importance sampling on the toy targets (l2hmc_small_ais_run in l2hmc_amd/csrc/small_ais.hip,
`DynamicsSampler.ais`, `ais_estimate`): the declaration and its binding, the argument checks that must fail before any
device call, what `ais` refuses before it takes a draw, the default schedule, and the float64 restatement of
tests/ais_ref.py against known normalising constants and at the cases tests/test_gpu_ais.py compares the kernel with.
No GPU: plans and arguments carry any non-NULL address where a pointer is checked, and the sampler runs on stub
dynamics that must not be asked for a plan."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib
from tests import ais_ref as A
from tests import toy_cases as tc
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _U64, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _target(dim=2, K=1, kind=1, temperature=1.0, mu=PTR, prec=PTR):
    return _lib.MogTarget(dim=dim, K=K, is_gaussian=kind, temperature=temperature, mu=mu, prec=prec, log_const=PTR)


def _plan(x_dim=2, hmc=1, N=5, masks=PTR, target=None):
    return _lib.SmallPlan(x_dim=x_dim, num_nodes=0, trajectory_length=N, hmc=hmc, eps=0.1, first_layer_form=0,
                          masks=masks, target=target if target is not None else _target())


_OK_INIT = _target()


def _run(L, plan, init=_OK_INIT, x_in=PTR, x_next=PTR, v=None, refreshment=0.1, B=4, draw0=0, n_steps=3, betas=PTR,
         log_w=PTR):
    return L.l2hmc_small_ais_run(None if plan is None else C.byref(plan), None if init is None else C.byref(init),
                                 x_in, x_next, v, refreshment, B, 42, draw0, n_steps, betas, log_w, None, None)


# ------------------------------------------------------------------------------------------------ the C entry
def test_header_declares_and_binding_matches():
    assert "l2hmc_small_ais_run" in _lib.declared_symbols()
    # plan, init, x_in, x_next, v, refreshment, B, seed, draw0, n_steps, betas, log_w, px, stream
    assert _lib._PROTOS["l2hmc_small_ais_run"] == (
        C.c_int, [C.POINTER(_lib.SmallPlan), C.POINTER(_lib.MogTarget), _P, _P, _P, _F, _I64, _U64, _U64, _I32, _P, _P,
                  _P, _P])
    text = header_text()
    assert ("int l2hmc_small_ais_run(const l2hmc_small_plan* plan, const l2hmc_mog_target* init, const float* x_in, "
            "float* x_next, float* v, float refreshment, int64_t B, uint64_t seed, uint64_t draw0, int32_t n_steps, "
            "const float* betas, double* log_w, float* px, l2hmc_stream_t stream);") in text
    assert "#define L2HMC_ABI_VERSION 1" in text


def test_library_exports_the_entry(L):
    assert L.l2hmc_small_ais_run is not None and L.l2hmc_abi_version() == 1


def test_bad_arguments_fail_with_a_message_before_any_device_call(L):
    ok = _plan()
    nan = float("nan")
    cases = [(dict(plan=None), "plan is NULL"), (dict(init=None), "init is NULL"),
             (dict(x_in=None), "x_in / x_next is NULL"), (dict(x_next=None), "x_in / x_next is NULL"),
             (dict(betas=None), "betas / log_w is NULL"), (dict(log_w=None), "betas / log_w is NULL"),
             (dict(B=-1), "B < 0"), (dict(n_steps=0), "n_steps=0"), (dict(n_steps=-1), "n_steps=-1"),
             (dict(plan=_plan(hmc=0)), "the plan is an L2HMC sampler's (hmc == 0)"),
             (dict(plan=_plan(x_dim=3)), "x_dim=3 != target dim=2"),
             (dict(plan=_plan(N=0)), "bad trajectory_length / masks"),
             (dict(plan=_plan(masks=None)), "bad trajectory_length / masks"),
             (dict(plan=_plan(target=_target(kind=4))), "target kind 4 unknown"),
             (dict(plan=_plan(target=_target(temperature=0.0))), "temperature must be > 0"),
             (dict(plan=_plan(target=_target(kind=3, dim=1), x_dim=1)), "funnel target needs dim >= 2"),
             (dict(init=_target(kind=0)), "init is a target of kind 0 and dim=2: expected a Gaussian (kind 1) of dim=2"),
             (dict(init=_target(kind=2)), "init is a target of kind 2"),
             (dict(init=_target(kind=3)), "init is a target of kind 3"),
             (dict(init=_target(dim=3)), "init is a target of kind 1 and dim=3"),
             (dict(plan=_plan(x_dim=3, target=_target(dim=3))), "init is a target of kind 1 and dim=2"),
             (dict(init=_target(mu=None)), "small_ais_run: init: target has a NULL parameter pointer"),
             (dict(init=_target(prec=None)), "small_ais_run: init: target has a NULL parameter pointer"),
             (dict(v=PTR, refreshment=0.0), "refreshment = 0 is not in (0, 1]"),
             (dict(v=PTR, refreshment=-0.1), "refreshment = -0.1 is not in (0, 1]"),
             (dict(v=PTR, refreshment=1.5), "refreshment = 1.5 is not in (0, 1]"),
             (dict(v=PTR, refreshment=nan), "is not in (0, 1]"),
             (dict(draw0=2 ** 64 - 4, n_steps=2), "draw0 + 2 * n_steps overflows 64 bits"),
             (dict(plan=_plan(N=9000)), "trajectory_length=9000: targets and masks take 72064 B of LDS (max 65536)")]
    for kw, word in cases:
        kw = dict(kw)
        plan = kw.pop("plan", ok)
        rc = _run(L, plan, **kw)
        msg = L.l2hmc_last_error().decode()
        assert rc == 1, (kw, rc)                      # L2HMC_ERR_ARG
        assert msg.startswith("small_ais_run: ") and word in msg, (kw, msg)
    with pytest.raises(ValueError, match="small_ais_run: n_steps=0 must be positive"):
        _lib.check(_run(L, ok, n_steps=0))


def test_an_empty_batch_is_a_no_op_after_the_checks(L):
    assert _run(L, _plan(), B=0) == 0
    assert _run(L, _plan(), B=0, v=PTR, refreshment=1.0) == 0                    # rho = 1 is allowed
    assert _run(L, _plan(), B=0, v=None, refreshment=7.0) == 0                    # not read without v
    assert _run(L, _plan(), B=0, init=_target(temperature=0.0)) == 0              # the init's temperature is not read
    for kind, dim in ((0, 2), (2, 2), (3, 2), (1, 8)):                            # every kind of final target
        tgt = _target(kind=kind, dim=dim, K=2 if kind == 0 else 1)
        assert _run(L, _plan(x_dim=dim, target=tgt), init=_target(dim=dim), B=0) == 0
    assert _run(L, _plan(hmc=0), B=0) == 1                                        # checked before the batch size
    assert _run(L, _plan(), B=0, draw0=2 ** 64 - 7, n_steps=3) == 0               # streams up to 2^64 - 2
    assert _run(L, _plan(), B=0, draw0=2 ** 64 - 6, n_steps=3) == 1


# ------------------------------------------------------------------------------------------------ `ais` on stubs
def _stub(hmc=True, layered=False, use_temperature=True, temperature=1.0):
    def _plan():
        raise AssertionError("a refused call must not build a plan")
    return types.SimpleNamespace(hmc=hmc, layered=layered, x_dim=2, trajectory_length=5, temperature=temperature,
                                 use_temperature=use_temperature, _draws=4, _seed=7, _device=torch.device("cpu"),
                                 _plan=_plan)


def _init(la, dim=2):
    return la.Gaussian(np.zeros(dim), np.eye(dim))


def test_signatures():
    import l2hmc_amd as la
    assert str(inspect.signature(la.DynamicsSampler.ais)) == "(self, anneal_steps, init, x, betas=None, refresh=None)"
    assert str(inspect.signature(la.ais_estimate)) == (
        "(init_energy, final_energy, anneal_steps, initial_x, step_size=0.5, leapfrogs=25, refresh=False, "
        "refreshment=0.1, seed=42)")


def test_ais_refuses_other_dynamics_without_a_draw():
    import l2hmc_amd as la
    x0 = torch.zeros(3, 2)
    dyn = _stub(hmc=False)
    with pytest.raises(ValueError, match="ais: the dynamics is an L2HMC sampler"):
        la.DynamicsSampler(dyn).ais(5, _init(la), x0)
    assert dyn._draws == 4
    dyn = _stub(layered=True)
    with pytest.raises(NotImplementedError, match="ais: this hmc dynamics runs layer by layer"):
        la.DynamicsSampler(dyn).ais(5, _init(la), x0)
    assert dyn._draws == 4
    dyn = _stub(use_temperature=False, temperature=3.0)
    with pytest.raises(ValueError, match="use_temperature=False"):
        la.DynamicsSampler(dyn).ais(5, _init(la), x0)
    assert dyn._draws == 4


def test_ais_refuses_another_init_without_a_draw():
    import l2hmc_amd as la
    dyn = _stub()
    x0 = torch.zeros(3, 2)
    gmm = la.GMM([np.zeros(2), np.ones(2)], [np.eye(2)] * 2, [0.5, 0.5])
    for bad in (gmm, la.RoughWell(2, 0.5), gmm.get_energy_function(), None, _init(la, 3)):
        with pytest.raises(ValueError, match="ais: init must be a Gaussian of dimension 2"):
            la.DynamicsSampler(dyn).ais(5, bad, x0)
    with pytest.raises(ValueError, match="pass the start"):
        la.DynamicsSampler(dyn).ais(5, _init(la), None)
    assert dyn._draws == 4


@pytest.mark.parametrize("betas", [[0.5, 1.0], np.ones((1, 3)), 1.0, [0.1, float("nan"), 1.0], [0.1, 0.5, 1.5],
                                   [-0.1, 0.5, 1.0], [0.2, 0.1, 1.0], [0.1, 0.5, float("inf")],
                                   [0.1, 0.5, 1.0 + 1e-7]])
def test_ais_refuses_a_bad_schedule_without_a_draw(betas):
    import l2hmc_amd as la
    dyn = _stub()
    with pytest.raises(ValueError, match="ais: betas"):
        la.DynamicsSampler(dyn).ais(3, _init(la), torch.zeros(3, 2), betas=betas)
    assert dyn._draws == 4


def test_ais_refuses_bad_counts_and_refresh_without_a_draw():
    import l2hmc_amd as la
    dyn = _stub()
    for n in (0, -1, 2.5):
        with pytest.raises(ValueError, match="ais: anneal_steps"):
            la.DynamicsSampler(dyn).ais(n, _init(la), torch.zeros(3, 2))
    for refresh in (0, 0.0, -0.1, 1.5, float("nan"), True, False, [0.1], 1e-60):
        with pytest.raises(ValueError, match="ais: refresh"):
            la.DynamicsSampler(dyn).ais(3, _init(la), torch.zeros(3, 2), refresh=refresh)
    assert dyn._draws == 4


def test_good_arguments_get_as_far_as_the_plan():
    """Schedules with equal neighbours, the ends 0 and 1, a float64 tensor and rho = 1 pass: the call gets as far as the
    plan (which the stub refuses), still without a draw."""
    import l2hmc_amd as la
    for kw in (dict(), dict(betas=[0.0, 0.0, 1.0]), dict(betas=np.ones(3)), dict(betas=torch.linspace(0.1, 1, 3).double()),
               dict(refresh=1.0), dict(refresh=0.1), dict(refresh=np.float32(0.5))):
        dyn = _stub()
        with pytest.raises(AssertionError, match="must not build a plan"):
            la.DynamicsSampler(dyn).ais(3, _init(la), torch.zeros(3, 2), **kw)
        assert dyn._draws == 4


@pytest.mark.parametrize("n", [1, 2, 7, 64, 1000])
def test_the_default_schedule_is_the_references_in_float32(n):
    import l2hmc_amd as la
    got = la.DynamicsSampler.ais_schedule(n)
    want = np.linspace(0, 1, n + 1)[1:].astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (n,) and np.array_equal(got, want)
    assert got[-1] == 1.0 and np.array_equal(got, A.default_schedule(n))


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("name", ["gaussian", "mixture", "funnel"])
def test_the_float64_restatement_finds_known_normalising_constants(name):
    """Gaussian to Gaussian: 0.5 logdet(Sigma1) - 0.5 logdet(Sigma0); the mixture at temperature 1: log Z1 = 0; the
    funnel: log Z1 = 0.5 log(8 pi).  The gate is |log_ratio - exact| <= 4 se and ess >= B / 8; init, schedule length and
    seed are chosen so that the restatement sits within 2 se, which leaves the kernel's run of the mixture case
    (tests/test_gpu_ais.py) room."""
    k = A.known(name)
    out, log_ratio, se, ess = A.known_reference(name)
    print(f"ais known answer {name}: exact {k.exact:.4f} log_ratio {log_ratio:.4f} se {se:.4f} "
          f"({abs(log_ratio - k.exact) / se:.2f} se off) ess {ess:.1f} of {k.B} mean accept {out['px'].mean():.3f}")
    assert np.isfinite(out["log_w"]).all() and out["draws"] == 2 * k.steps
    assert abs(log_ratio - k.exact) <= 4 * se and ess >= k.B / 8
    assert abs(log_ratio - k.exact) <= 2 * se
    if name == "mixture":
        assert k.exact == -np.log(2 * np.pi) and abs(log_ratio + A.log_norm(k.init_sigma)) <= 2 * se      # log Z1 = 0
    if name == "funnel":
        assert np.isclose(k.exact + A.log_norm(k.init_sigma), 0.5 * np.log(8 * np.pi))


def test_the_estimator_on_weights_with_a_known_mean():
    w = np.log(np.array([1.0, 2.0, 3.0, 6.0])) + 700.0              # exp overflows without the shift
    log_ratio, se, ess = A.estimate(w)
    assert np.isclose(log_ratio, 700.0 + np.log(3.0))
    assert np.isclose(se, np.std([1, 2, 3, 6], ddof=1) / (2.0 * 3.0)) and np.isclose(ess, 144.0 / 50.0)


# ------------------------------------------------------------------------------------------------ the parity cases
@pytest.mark.parametrize("refresh", [False, True], ids=["fresh", "refresh"])
@pytest.mark.parametrize("kind", list(A.KINDS))
def test_no_parity_chain_decides_near_a_tie(kind, refresh):
    """What tests/test_gpu_ais.py relies on: at every batch size every float64 |p - u| exceeds MH_MARGIN at every step
    (no chain has to be left out), the float32 restatement takes the same decisions and stays finite, every case has
    accepted and rejected proposals -- a `refresh` case therefore runs the -Lv branch --, and the streams are counted as
    `ais` counts them."""
    for B in A.PARITY_BATCHES:
        w64, w32 = A.parity_reference(kind, refresh, B)
        assert w64["margin"].shape == (B,) and w64["margin"].min() > tc.MH_MARGIN, (B, w64["margin"].min())
        assert np.array_equal(w64["accepted"], w32["accepted"])
        assert w64["accepted"].any() and not w64["accepted"].all(), B
        assert all(np.isfinite(w[k]).all() for w in (w64, w32) for k in ("log_w", "x", "px"))
        assert w64["draws"] == 2 * A.PARITY_STEPS + (1 if refresh else 0)
        assert ("v" in w64) == refresh
    rate = A.parity_reference(kind, refresh, 130)[0]["accepted"].mean()
    print(f"ais parity {kind} refresh={refresh}: accept rate {rate:.3f}, smallest |p - u| "
          f"{A.parity_reference(kind, refresh, 130)[0]['margin'].min():.2e}")
    assert 0.8 < rate < 0.97


def test_parity_step_sizes_stay_at_half_the_stability_limit():
    """eps * sqrt(largest curvature of E1 / temperature) <= 1 (tests/ais_ref.py: KINDS), with the curvatures recomputed
    from the targets."""
    for kind, (dim, temperature, eps) in A.KINDS.items():
        if kind == "funnel":
            continue
        t = A.final_oracle(kind)
        if kind == "rw":
            stiff = 1.0 + t.eps / (t.eps if t.easy else t.eps ** 2) ** 2
        else:
            precs = [t.i_sigma] if hasattr(t, "i_sigma") else t.i_sigmas
            stiff = max(float(np.linalg.eigvalsh(np.asarray(p, dtype=np.float64)).max()) for p in precs)
        assert np.isclose(stiff, A.STIFFNESS[kind], rtol=1e-3), (kind, stiff)
        assert 0.8 < eps * np.sqrt(stiff / temperature) <= 1.0, (kind, eps * np.sqrt(stiff / temperature))


def test_chains_are_the_same_at_every_batch_size():
    a, b = A.parity_reference("mog", True, 130)[0], A.parity_reference("mog", True, 65)[0]
    for k in ("log_w", "x", "v"):
        assert np.array_equal(a[k][:65], b[k])
    assert np.array_equal(a["px"][:, :65], b["px"])


def test_the_restatement_at_the_ends_of_the_schedule():
    """betas all 0: the chains sample the init Gaussian and the weights stay 0; a one-step schedule [1] is plain
    importance sampling, log_w = E0(x) - E1(x) at the start."""
    from oracle import dynamics as od
    mu, sigma = A.init_arrays(2)
    E0, E1, x0 = od.Gaussian(mu, sigma), A.final_oracle("mog"), A.start(2, 65)
    out = A.anneal(E0, E1, 1.0, A.masks(5, 2), 0.2, x0, np.zeros(4, np.float32), 1, 0)
    assert (out["log_w"] == 0).all() and not np.array_equal(out["x"], x0)
    out = A.anneal(E0, E1, 1.0, A.masks(5, 2), 0.2, x0, np.ones(1, np.float32), 1, 0)
    assert np.allclose(out["log_w"], E0.energy(x0) - E1.energy(x0), rtol=1e-12, atol=0)
