"""Host side of training GaugeDynamics on a ladder of beta (l2hmc_gauge_train_forward_ladder, _train_backward_ladder,
_loss_backward_ladder in l2hmc_amd/csrc/train.hip; `GaugeTrainer` with a beta per chain): the declarations and their
bindings, the refusals that must come before any device call, what the trainer refuses before a draw is taken, the
annealing of an array and the schedule of the exchange rounds inside `train` -- and the float64 reference the GPU tests
use (tests/ladder_ref.py) against the unmodified oracle.  No GPU: plans and arguments carry any non-NULL address where a
pointer is checked, and the trainer's methods run on stub dynamics."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib
from tests import ladder_ref as LR
from tests.run_cases import PTR, header_text

_P, _I32, _I64, _F, _SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
NAMES = ("l2hmc_gauge_train_forward_ladder", "l2hmc_gauge_train_backward_ladder", "l2hmc_gauge_loss_backward_ladder")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _net(D=128, H=512):
    w = dict(w1_t=PTR, wt=PTR, b1=PTR, wh_t=PTR, bh=PTR, whd_t=PTR, bhd=PTR, coeff_s=PTR, coeff_q=PTR)
    return _lib.DenseNet(D=D, H=H, Ka=D, Kb=D, **w)


def _plan(T=8, X=8, N=3, hmc=0):
    D = 2 * T * X
    return _lib.GaugePlan(T=T, X=X, num_steps=N, hmc=hmc, masks=PTR, xnet=_net(D, 4 * D), vnet=_net(D, 4 * D))


def _fwd(L, plan, betas=PTR, stride=1, chains=4, rows=8):
    return L.l2hmc_gauge_train_forward_ladder(None if plan is None else C.byref(plan), betas, stride, chains, PTR, PTR,
                                              PTR, rows, PTR, PTR, PTR, PTR, PTR, 0, None)


def _bwd(L, plan, betas=PTR, stride=1, chains=4, rows=8):
    g = _lib.DenseGrads()
    return L.l2hmc_gauge_train_backward_ladder(None if plan is None else C.byref(plan), betas, stride, chains, PTR, rows,
                                               PTR, PTR, PTR, C.byref(g), C.byref(g), None, None, PTR, PTR, 0, None,
                                               _lib.BUCKET_FN(), None)


def _loss(L, betas=PTR, stride=1, B=4, metric=4, T=8, x0=PTR):
    return L.l2hmc_gauge_loss_backward_ladder(T, 8, betas, stride, x0, PTR, PTR, PTR, B, metric, 1., 1., 1., 1., 1., PTR,
                                              PTR, PTR, PTR, None)


# ------------------------------------------------------------------------------------------------ the C entries
def test_header_declares_and_bindings_match(L):
    declared = set(_lib.declared_symbols())
    for name in NAMES:
        assert name in declared and getattr(L, name) is not None
    gp, dg, cg = C.POINTER(_lib.GaugePlan), C.POINTER(_lib.DenseGrads), C.POINTER(_lib.Conv3DGrads)
    assert _lib._PROTOS[NAMES[0]] == (C.c_int, [gp, _P, _I64, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _SZ, _P])
    assert _lib._PROTOS[NAMES[1]] == (C.c_int, [gp, _P, _I64, _I64, _P, _I64, _P, _P, _P, dg, dg, cg, cg, _P, _P, _SZ,
                                                _P, _lib.BUCKET_FN, _P])
    assert _lib._PROTOS[NAMES[2]] == (C.c_int, [_I32, _I32, _P, _I64] + [_P] * 4 + [_I64, _I32] + [_F] * 5 + [_P] * 5)
    text = header_text()
    assert ("int l2hmc_gauge_train_forward_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t chain_stride, "
            "int64_t chains, const float* x0, const float* v0, const int32_t* dir, int64_t rows, float* x_out, "
            "float* v_out, float* sumlogdet, float* p_accept, void* ws, size_t ws_bytes, l2hmc_stream_t stream);") in text
    assert ("int l2hmc_gauge_train_backward_ladder(const l2hmc_gauge_plan* plan, const float* betas, int64_t chain_stride, "
            "int64_t chains, const int32_t* dir, int64_t rows, float* dx, float* dv, const float* dlogdet,") in text
    assert ("int l2hmc_gauge_loss_backward_ladder(int32_t T, int32_t X, const float* betas, int64_t chain_stride, "
            "const float* x0,") in text
    # the scalar entries keep their signatures
    assert "int l2hmc_gauge_train_forward(const l2hmc_gauge_plan* plan, float beta, const float* x0," in text
    assert "int l2hmc_gauge_loss_backward(int32_t T, int32_t X, float beta, const float* x0," in text
    # the header says that the values on the device are not checked
    assert "VALUES of betas are on the device and are not checked" in header_text(comments=True)


def test_refusals_come_with_a_message_and_without_a_device(L):
    ok = _plan()
    for fn, who in ((_fwd, "train_forward_ladder"), (_bwd, "train_backward_ladder")):
        for kw, word in ((dict(betas=None), "NULL betas"), (dict(stride=2), "chain_stride = 2"),
                         (dict(stride=-1), "chain_stride = -1"), (dict(chains=0), "chains = 0"),
                         (dict(chains=-4), "chains = -4"), (dict(chains=3), "no whole number of chains = 3")):
            assert fn(L, ok, **kw) == 1, (who, kw)
            msg = L.l2hmc_last_error().decode()
            assert msg.startswith(who + ": ") and word in msg, (kw, msg)
        # ... and everything the scalar entries refuse: no plan, an hmc plan, widths that are no multiples of 32
        assert fn(L, None) == 1 and "NULL plan" in L.l2hmc_last_error().decode()
        assert fn(L, _plan(hmc=1)) == 1 and "hmc plans" in L.l2hmc_last_error().decode()
        assert fn(L, _plan(6, 6)) == 1 and "multiples of 32" in L.l2hmc_last_error().decode()
    assert _fwd(L, ok, rows=-8) == 1 and "rows < 0" in L.l2hmc_last_error().decode()
    for kw, word in ((dict(betas=None), "NULL betas"), (dict(stride=3), "chain_stride = 3"), (dict(metric=7), "bad"),
                     (dict(T=0), "bad"), (dict(B=-1), "bad"), (dict(x0=None), "NULL pointer")):
        assert _loss(L, **kw) == 1, kw
        assert word in L.l2hmc_last_error().decode(), (kw, L.l2hmc_last_error().decode())
    with pytest.raises(ValueError, match="train_forward_ladder: NULL betas"):
        _lib.check(_fwd(L, ok, betas=None))


def test_an_empty_batch_is_a_no_op(L):
    assert _fwd(L, _plan(), rows=0) == 0
    assert _loss(L, B=0) == 0
    assert _bwd(L, _plan(), rows=0) == 0                    # (nothing is written: the gradients stay what they were)
    assert _bwd(L, None, rows=0) == 1 and _bwd(L, _plan(), rows=0, betas=None) == 1


# ------------------------------------------------------------------------------------------------ the trainer
def _stub_trainer(B=6, D=32):
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    draws = []

    def no_draw(*_a):
        draws.append(1)
        raise AssertionError("a draw was taken")
    dyn = types.SimpleNamespace(_device=torch.device("cpu"), _x=lambda a: torch.as_tensor(np.asarray(a, np.float32)),
                                lattice=types.SimpleNamespace(time_size=4, space_size=4), _normal=no_draw,
                                _uniform=no_draw)
    tr = types.SimpleNamespace(dynamics=dyn)
    tr._chain_betas = lambda *a: GaugeTrainer._chain_betas(tr, *a)
    return GaugeTrainer, tr, draws, np.zeros((B, D))


def test_beta_parsing_takes_a_scalar_or_one_value_per_chain():
    GT, tr, _, _ = _stub_trainer()
    for scalar in (2.0, 3, np.float32(1.5), np.asarray(2.0), torch.tensor(2.0)):
        assert GT._chain_betas(tr, scalar, 6, "t") is None
    for arr in (LR.ladder(6), LR.ladder(6)[None, :], list(LR.ladder(6)), torch.tensor(LR.ladder(6))):
        got = GT._chain_betas(tr, arr, 6, "t")
        assert got.dtype == torch.float32 and tuple(got.shape) == (6,)
        np.testing.assert_array_equal(got.numpy(), LR.ladder(6).astype(np.float32))


@pytest.mark.parametrize("bad", [np.ones(5), np.ones(7), np.ones((2, 6)), np.ones((6, 1)), -np.ones(6),
                                 [1, 2, np.nan, 1, 1, 1], [1, 2, np.inf, 1, 1, 1], np.ones((1, 1, 6))])
def test_a_bad_ladder_is_refused_before_any_draw(bad):
    GT, tr, draws, x = _stub_trainer()
    with pytest.raises(ValueError, match="GaugeTrainer.calc_loss_and_grads: "):
        GT.calc_loss_and_grads(tr, x, np.asarray(bad, dtype=np.float64))
    assert not draws


def test_update_beta_anneals_an_array_elementwise():
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    b0, b1 = np.asarray([1.0, 2.0, 2.5]), np.asarray([2.0, 4.0, 2.5])
    for step in (0, 3, 9):
        got = GaugeTrainer.update_beta(None, step, b0, b1, 10)
        want = [GaugeTrainer.update_beta(None, step, float(a), float(b), 10) for a, b in zip(b0, b1)]
        np.testing.assert_allclose(got, want, rtol=1e-15)
    np.testing.assert_array_equal(GaugeTrainer.update_beta(None, 0, b0, b1, 10), b0)
    assert isinstance(GaugeTrainer.update_beta(None, 2, 2., 4., 10), float)


def test_round_schedule_of_train_with_replicas():
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    assert GaugeTrainer.swap_schedule(5, 2) == {2: 0, 4: 1}
    assert GaugeTrainer.swap_schedule(4, 1) == {1: 0, 2: 1, 3: 0, 4: 1}
    assert GaugeTrainer.swap_schedule(7, 3) == {3: 0, 6: 1}
    assert GaugeTrainer.swap_schedule(2, 3) == {} and GaugeTrainer.swap_schedule(0, 1) == {}
    # the sampler's rule (GaugeSampler.run_hmc_exchange with first_parity 0): (s // k - 1) % 2 after every k-th step
    for n, k in ((9, 2), (6, 1), (10, 4)):
        assert GaugeTrainer.swap_schedule(n, k) == {s: (s // k - 1) % 2 for s in range(1, n + 1) if s % k == 0}


# ------------------------------------------------------------------------------------------------ the reference
def test_ladder_reference_is_the_oracle_rung_by_rung():
    """4 x 4, N = 3, B = 6, three betas in the fixed pattern: per-chain terms equal the unmodified oracle's run on each
    rung's chains exactly, gradients the B_g / B-weighted sum of those runs, and a uniform beta at the mean is far off."""
    from oracle.torch_ref import TorchGaugeModel
    from tests import helpers as H
    T = X = 4
    N, eps, B = 3, 0.2, 6
    xp, vp = H.gauge_weights(T, X, regime="mild")
    mask = H.gauge_oracle(T, X, N, eps, xp, vp).mask
    x, z, dx, dz = LR.inputs(B, 2 * T * X)
    betas, rung = LR.ladder(B), LR.rung_of(B)
    assert sorted(set(rung)) == [0, 1, 2] and list(rung) == [0, 2, 1, 1, 0, 2]
    lad = LR.LadderGaugeModel(T, X, N, eps, mask, xp, vp)
    _, terms = LR.ref_grads(lad, x, z, dx, dz, betas)
    g_lad = [p.grad.clone() for p in lad.parameters()]
    acc = [torch.zeros_like(g) for g in g_lad]
    for g, b in enumerate(LR.RUNGS):
        ch = np.nonzero(rung == g)[0]
        plain = TorchGaugeModel(T, X, N, eps, mask, xp, vp)
        sub = lambda d: tuple(a[ch] for a in d)      # noqa: E731
        _, t_g = LR.ref_grads(plain, x[ch], z[ch], sub(dx), sub(dz), float(b))
        np.testing.assert_array_equal(terms[ch], t_g)
        for a, p in zip(acc, plain.parameters()):
            a += p.grad * (len(ch) / B)
    for got, want in zip(g_lad, acc):
        assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    uni = TorchGaugeModel(T, X, N, eps, mask, xp, vp)
    LR.ref_grads(uni, x, z, dx, dz, float(betas.mean()))
    far = [float((a - p.grad).abs().max() / a.abs().max()) for a, p in zip(g_lad, uni.parameters())]
    assert min(far) > 0.1, far        # a kernel that ignores the chain axis cannot pass the GPU gate of 2e-4
