"""ConvNet3D kernels where T != X and the filter count is not the extent.

include/l2hmc_hip.h promises ConvNet3D for any lattice with T and X multiples of 4 and any F % 4 == 0; every
other ConvNet3D test is square with F = L (the compile-time instances conv3d_front_kernel<8, 8> / <16, 16> and
their _bwd twins) or square with F = 4.  The run-time-shaped instances <0, 0> index with T, X, T/2, X/2, T/4,
X/4 and their padded versions separately, and so does the host code that carves their buffers (conv3d_nflat,
ldo = Ka, the dfeat offsets, the conv_part slots of conv3d_cpw): a T <-> X mix-up in any of them is the identity
on a square lattice.  tests/test_conv3d_shapes_host.py shows on the float64 references alone that at the shapes
used here such mix-ups move S / T / Q by >= 0.2, i.e. 2e4 x TOL_OP.

The stages are ordered so that a failure localises:
  1. front-end + trunk alone  (ConvNet3D.__call__ -> l2hmc_stq_conv3d; "stress" weights, TOL_OP);
  2. leapfrog steps, transitions and the native step on the layer-by-layer path ("mild" weights; the yardsticks of
     tests/test_gpu_parity.py, imported);
  3. training gradients against float64 autograd (the yardsticks of tests/test_gpu_train.py, imported).
Every case asserts the launch form its comment names through mirrors of the launchers' rules
(tests/conv3d_cases.py, tests/test_gpu_train_batch.py::_conv_cpw): a change to a heuristic fails here instead of
silently moving coverage.

Stage 3 inputs are fixed (weights "mild" seed 106, default_rng(7) in the order test_gpu_train.py::_setup draws
them, eps 0.1, beta 2.5, cos_diff).  At these inputs float32 torch autograd of the same graph (16 CPU threads)
stays within 4.7e-5 of float64 in every tensor and in eps (worst: 12 x 8, where every tensor sits at 2-5e-5),
i.e. within TOL_G / 4, so relu and pooling-winner flips do not decide the outcome and the plain max-norm
comparison of test_gpu_train.py applies.

Measured on the MI355X: see MEASURED below (worst error per stage, wall time per case)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lattice as olat
from oracle.torch_ref import TorchGaugeModel
from tests import conv3d_cases as CC
from tests import helpers as H
from tests.test_gpu_parity import P_RATIO, TOL_OP, TOL_P, assert_fp32_equivalent, np_
from tests.test_gpu_train import TOL_G, _compare, _packed_ref, _ref_grads
from tests.test_gpu_train_batch import _conv_cpw

pytestmark = pytest.mark.gpu

MEASURED = """
Worst error per stage and wall time per case on the MI355X (the kernels are deterministic: exact for these inputs).
  1. S / T / Q relerr against TOL_OP = 1e-5: 2.5e-7 .. 1.0e-6 (worst: S at 8 x 16 / F = 16, rows = 5; with the
     mask 3.9e-7).  0.01-0.10 s per case (0.3 s for the first, which loads the library).
  2. single leapfrog steps (x, v, log-det) 1.9e-7 .. 4.1e-7 against TOL_OP; transitions: x_prop 1.3e-7 .. 2.1e-7
     where the fp32 oracle itself sits at 2.1e-7 .. 3.2e-7; accept probability 6.7e-7 .. 1.6e-5 against TOL_P = 2e-5
     (worst: 4 x 12, whose fp32 oracle is 9.2e-6 away).  0.06-0.27 s per case.
  3. gradients, worst tensor / eps / loss against TOL_G = 2e-4:
       4 x 16 / F = 16   2.5e-5 (xnet.w2_b)    1.2e-5   3.9e-6
       16 x 4 / F = 4    1.6e-5 (vnet.b2_b)    1.1e-5   2.1e-6
       8 x 16 / F = 16   8.7e-6 (xnet.w1_b)    7.0e-6   2.4e-6
       8 x 8 / F = 20    7.7e-6 (xnet.b2_a)    1.2e-6   1.1e-6
       4 x 8 / F = 8     8.1e-6 (xnet.w2_b)    1.8e-6   4.9e-7
       12 x 8 / F = 8    1.1e-4 (xnet.b1_b, vnet.coeff_q; xnet.w1_b 8.9e-5)   3.6e-7   1.3e-5
       4 x 16 / F = 8    9.8e-6 (xnet.coeff_s) 8.9e-7   1.0e-6
     12 x 8 is the noisiest case for float32 torch as well (every tensor 2-5e-5 from float64): tensors of both
     networks move together there, which is the rounding of the shared loss terms, not one kernel's index.
     0.09-0.17 s per case with its float64 graph (0.6 s for the first).
Power, on the device: with `(c * T2P + 2 * I2) * X2P` of the forward kernel's second convolution read with
min(T2P, X2P) as its row stride (the identity for T >= X), stage 1 fails at 4 x 16, 8 x 16 (both row counts),
4 x 12 and with the mask, and passes at 16 x 4, 12 x 8 and the square shapes; with the backward kernel's dfeat offset
taken as which * min(T4, X4)^2 * F2 and its wider-filter-set loop skipped, the first six cases of stage 3 fail
(8 x 8 / F = 20 through the loop alone; 4 x 16 / F = 8 was added afterwards) while stage 1 passes.  Every ConvNet3D test of test_gpu_parity.py and test_gpu_train.py
passes with either change.
"""


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _conv_net(la, T, X, F, rows, scope='position', factor=2.):
    D = 2 * T * X
    return la.ConvNet3D('XNet' if scope == 'position' else 'VNet', _input_shape=(rows, T, X, 2), links_shape=(T, X, 2),
                        x_dim=D, factor=factor, spatial_size=X, num_hidden=2 * D, num_filters=F,
                        filter_sizes=[(3, 3, 2), (2, 2, 2)], name_scope=scope, data_format='channels_last')


# ================================================================= 1. front-end + trunk alone
@pytest.mark.parametrize("T,X,F,rows", CC.STQ_CASES)
def test_stq_conv3d_matches_oracle_at_any_shape(la, T, X, F, rows):
    """l2hmc_stq_conv3d = conv3d_front_kernel<0, 0> + the dense trunk, against oracle.nets.conv3d_net on fp32-rounded
    weights and inputs, as test_stq_conv3d_matches_oracle does for the square shapes."""
    assert not CC.is_instance(T, X, F)
    assert CC.front_form(T, X, F, rows) == CC.STQ_FORMS[T, X, F, rows]       # (cpw, full workgroups, rows of the last)
    xp, a, b, t, (So, To, Qo) = CC.stq_reference(T, X, F, rows)
    net = _conv_net(la, T, X, F, rows)
    net.load_state(xp)
    assert net.nflat == CC.nflat(T, X, F) == xp['x_layer/W'].shape[0]
    S, Tr, Q = net([a, b, t])
    errs = [H.relerr(np_(g), w) for g, w in zip((S, Tr, Q), (So, To, Qo))]
    print(f"stq {T}x{X} F={F} rows={rows}: relerr S/T/Q = " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < TOL_OP, errs
    assert np.abs(To).max() > 1e-4


def test_stq_conv3d_with_a_mask_on_the_second_input(la):
    """l2hmc_stq_conv3d's `bmask` (a 0/1 mask of length D on the second input, applied while the chain is staged):
    ConvNet3D.__call__ always passes NULL, so the argument is otherwise reached through the dynamics only."""
    from l2hmc_amd import _lib
    T, X, F, rows = 4, 16, 16, 9
    D = 2 * T * X
    mask = (np.random.default_rng(17).permutation(D) < D // 2).astype(np.float64)
    xp, a, b, t, (So, To, Qo) = CC.stq_reference(T, X, F, rows, bmask=mask)
    plain = CC.stq_reference(T, X, F, rows)[4]
    assert min(H.relerr(p, w) for p, w in zip(plain, (So, To, Qo))) > 100 * TOL_OP      # the mask matters
    net = _conv_net(la, T, X, F, rows)
    net.load_state(xp)
    st, fr = net.pack(), net.pack_front()
    dev = net._device
    a_d, b_d, m_d = (_lib.as_dev(z, dev) for z in (a, b, mask))
    S, Tr, Q = (torch.empty(rows, D, dtype=torch.float32, device=dev) for _ in range(3))
    ws = _lib.Workspace()
    wp, nb = ws.get(_lib.lib().l2hmc_stq_conv3d_ws_bytes(rows, st.H, T, X, fr.F), dev)
    tc, ts = float(np.float32(t[0, 0])), float(np.float32(t[0, 1]))
    _lib.call("l2hmc_stq_conv3d", C.byref(fr), C.byref(st), T, X, a_d, b_d, m_d, tc, ts, rows, S, Tr, Q, wp, nb,
              device=dev)
    errs = [H.relerr(np_(g), w) for g, w in zip((S, Tr, Q), (So, To, Qo))]
    print(f"stq bmask {T}x{X}: relerr S/T/Q = " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < TOL_OP, errs


# ================================================================= 2. leapfrog steps and transitions
def _dynamics(la, T, X, F, N, eps, B, regime="mild"):
    """(oracle, fp32 oracle, HIP dynamics) with the same ConvNet3D weights; F = None: the default F = X.  Another F is
    swapped in the way test_conv3d_gradients_generic_filter_count swaps its networks."""
    xp, vp = H.conv_weights(T, X, regime=regime, F=F)
    orc = H.gauge_oracle(T, X, N, eps, xp, vp, arch='conv3D')
    orc32 = H.gauge_oracle(T, X, N, eps, xp, vp, arch='conv3D', dtype=np.float32)
    if F in (None, X):
        dyn = H.gauge_hip(T, X, N, eps, xp, vp, orc.mask, B, arch='conv3D')
    else:
        dxp, dvp = H.conv_weights(T, X, regime=regime)
        dyn = H.gauge_hip(T, X, N, eps, dxp, dvp, orc.mask, B, arch='conv3D')
        dyn.position_fn = _conv_net(la, T, X, F, B, 'position', 2.)
        dyn.momentum_fn = _conv_net(la, T, X, F, B, 'momentum', 1.)
        dyn.position_fn.load_state(xp)
        dyn.momentum_fn.load_state(vp)
    assert dyn.position_fn.num_filters == (X if F is None else F) and dyn.position_fn.num_hidden == 4 * T * X
    assert dyn.position_fn.nflat == dyn.momentum_fn.nflat == CC.nflat(T, X, X if F is None else F)
    return orc, orc32, dyn, (xp, vp)


def _layer_by_layer(dyn):
    from l2hmc_amd import _lib
    plan = dyn._plan()
    return _lib.lib().l2hmc_gauge_plan_fused(C.byref(plan)) == 0


@pytest.mark.parametrize("T,X,F,N,B", [
    (4, 16, None, 3, 11),      # D = 128 (the whole-step kernel's width) on a lattice it must refuse for ConvNet3D
    (16, 4, None, 3, 11),      # ... and X/4 = 1, F = 4
    (8, 16, None, 2, 6),
    (4, 12, None, 3, 9),       # nflat = 24: ragged trunk, no kept products
    (8, 8, 12, 3, 21),         # D = 128 on the 8 x 8 lattice with a filter count the whole-step kernel has no form for
])
def test_conv3d_dynamics_matches_oracle_at_any_shape(la, T, X, F, N, B):
    eps, beta, D = 0.2, 2.0, 2 * T * X
    orc, orc32, dyn, _ = _dynamics(la, T, X, F, N, eps, B)
    assert _layer_by_layer(dyn)
    x, v0f, v0b, coin, u = H.gauge_inputs(B, D)
    worst = 0.0
    for step in (0, N - 1):
        for fn, ofn in ((dyn._forward_lf, orc._forward_lf), (dyn._backward_lf, orc._backward_lf)):
            x1, v1, ld = fn(x, v0f, beta, step)
            ox, ov, old = ofn(x, v0f, beta, step)
            errs = (H.relerr(np_(x1), ox), H.relerr(np_(v1), ov), H.relerr(np_(ld), old))
            worst = max(worst, *errs)
            assert max(errs) < TOL_OP, (step, errs)
    want = orc.apply_transition(x, beta, v0f, v0b, coin, u)
    f32 = orc32.apply_transition(x.astype(np.float32), beta, v0f.astype(np.float32), v0b.astype(np.float32), coin,
                                 u.astype(np.float32))
    perr = 0.0
    for both in (True, False):                  # both directions, and the selected direction only
        dyn.both_directions = both
        assert _layer_by_layer(dyn)
        got = [np_(g) for g in dyn.apply_transition(x, beta, momentum_f=v0f, momentum_b=v0b, coin=coin, u=u)]
        assert_fp32_equivalent(got[0], want[0], f32[0], "x_prop")
        assert_fp32_equivalent(got[1], want[1], f32[1], "v_prop")
        perr = max(perr, np.abs(got[2] - want[2]).max())
        assert np.abs(got[2] - want[2]).max() < max(TOL_P, P_RATIO * np.abs(f32[2] - want[2]).max())
    print(f"dyn {T}x{X} F={F} N={N} B={B}: worst single-step relerr {worst:.2e}, transition x {H.relerr(got[0], want[0]):.2e} "
          f"(fp32 oracle {H.relerr(f32[0], want[0]):.2e}), p {perr:.2e}")


@pytest.mark.parametrize("T,X,N,B", [(4, 16, 3, 9), (8, 16, 2, 6)])
def test_kept_products_equal_recomputed_at_non_square_shapes(la, T, X, N, B):
    """test_gpu_parity.py::test_kept_products_equal_recomputed on non-square ConvNet3D lattices: the kept first-layer
    products are carved per row with H and nflat of this shape."""
    orc, _, dyn, _ = _dynamics(la, T, X, None, N, 0.15, B)
    dyn.fused = False
    x, v0f, v0b, coin, u = H.gauge_inputs(B, 2 * T * X, seed=311)
    outs = {}
    for rec in (False, True):
        dyn.recompute = rec
        o = [dyn.transition_kernel(x, 2.0, forward=fwd, momentum=v0, return_logdet=True)
             for fwd, v0 in ((True, v0f), (False, v0b))]
        o.append(dyn.apply_transition(x, 2.0, momentum_f=v0f, momentum_b=v0b, coin=coin, u=u))
        outs[rec] = [t for tup in o for t in tup]
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a, b)
    want = orc.transition_kernel(x, 2.0, v0f, forward=True)
    assert H.relerr(np_(outs[False][0]), want[0]) < 2 * TOL_OP and H.relerr(np_(outs[False][1]), want[1]) < 2 * TOL_OP


def test_active_column_heads_equal_all_columns_at_4x16(la):
    """test_gpu_parity.py::test_active_column_heads_equal_all_columns at 4 x 16, B = 64 (whole row tiles)."""
    T, X, N, B = 4, 16, 3, 64
    orc, _, dyn, _ = _dynamics(la, T, X, None, N, 0.15, B)
    dyn.fused = False
    x, v0f, v0b, coin, u = H.gauge_inputs(B, 2 * T * X, seed=313)
    outs = {}
    try:
        for on in (1, 0):
            dyn.all_columns = not on
            f = dyn.transition_kernel(x, 2.0, forward=True, momentum=v0f, return_logdet=True)
            tr = dyn.apply_transition(x, 2.0, momentum_f=v0f, momentum_b=v0b, coin=coin, u=u)
            lf = dyn._forward_lf(x, v0f, 2.0, 1)
            outs[on] = (f, tr, lf)
    finally:
        dyn.all_columns = False
    (f1, tr1, lf1), (f0, tr0, lf0) = outs[1], outs[0]
    assert torch.equal(f1[0], f0[0]) and torch.equal(f1[1], f0[1])
    assert torch.equal(lf1[0], lf0[0]) and torch.equal(lf1[1], lf0[1])
    assert torch.equal(tr1[0], tr0[0]) and torch.equal(tr1[1], tr0[1]) and torch.equal(tr1[3], tr0[3])
    scale = max(1.0, float(f0[3].abs().max()))
    assert float((f1[3] - f0[3]).abs().max()) <= 2e-6 * scale
    assert float((lf1[2] - lf0[2]).abs().max()) <= 2e-6 * max(1.0, float(lf0[2].abs().max()))
    assert float((f1[2] - f0[2]).abs().max()) <= 1e-5 and float((tr1[2] - tr0[2]).abs().max()) <= 1e-5
    want = orc.transition_kernel(x, 2.0, v0f, forward=True)
    assert H.relerr(np_(f1[0]), want[0]) < 2 * TOL_OP and H.relerr(np_(f1[1]), want[1]) < 2 * TOL_OP


def test_native_mcmc_step_matches_oracle_on_its_own_draws_at_4x16(la):
    """test_gpu_parity.py::test_native_mcmc_step_matches_oracle_on_its_own_draws at 4 x 16, B = 21: the one-call step
    (draws, both trajectories, mix / MH, observables, wrap) with ConvNet3D on a non-square lattice."""
    from l2hmc_amd import _lib
    T, X, B = 4, 16, 21
    N, eps, beta, D = 3, 0.1, 2.0, 2 * T * X
    orc, _, dyn, _ = _dynamics(la, T, X, None, N, eps, B)
    assert _layer_by_layer(dyn)
    x0 = np.random.default_rng(3).uniform(0, 2 * np.pi, (B, D)).astype(np.float32)
    x = torch.as_tensor(x0, device="cuda").clone()
    outs = [torch.empty(B, device="cuda") for _ in range(5)]
    plan, Lh = dyn._plan(), _lib.lib()
    ws, nb = dyn._ws.get(Lh.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B), x.device)
    seed, draw = 77, 5
    _lib.check(Lh.l2hmc_gauge_mcmc_step(C.byref(plan), beta, x.data_ptr(), B, seed, draw, *[o.data_ptr() for o in outs],
                                         ws, nb, _lib.stream_ptr()))
    V = torch.empty(2 * B, D, device="cuda")
    cu = torch.empty(2 * B, device="cuda")
    _lib.check(Lh.l2hmc_fill_normal(V.data_ptr(), V.numel(), seed, 2 * draw, None))
    _lib.check(Lh.l2hmc_fill_uniform(cu.data_ptr(), cu.numel(), seed, 2 * draw + 1, None))
    V, cu = np_(V), np_(cu)
    x64 = x0.astype(np.float64)
    want = orc.apply_transition(x64, beta, V[:B], V[B:], cu[:B], cu[B:])
    px, actions, plaqs, charges, dq = [np_(o) for o in outs]
    assert np.abs(px - want[2]).max() < TOL_P
    assert H.relerr(actions, olat.total_action(x64, T, X)) < TOL_OP
    assert H.relerr(plaqs, olat.avg_plaq(x64, T, X)) < TOL_OP
    assert H.relerr(charges, olat.top_charge(x64, T, X)) < 1e-4
    safe = np.abs(want[2] - cu[B:]) > 1e-4
    assert H.relerr(dq[safe], olat.top_charge_diff(x64, want[3], T, X)[safe]) < 1e-3
    xw = np.mod(want[3], 2 * np.pi)
    got = np_(x)
    d = np.abs(got - xw)[safe]
    d = np.minimum(d, 2 * np.pi - d)
    assert d.max() < 5e-5
    assert got.min() >= 0 and got.max() < 2 * np.pi + 1e-6


# ================================================================= 3. training gradients
def train_reference(T, X, F, N, B, dtype=torch.float64):
    """(xp, vp, masks, TorchGaugeModel, x, z, dx, dz): the fixed inputs of a stage-3 case (no GPU)."""
    eps = 0.1
    xp, vp = H.conv_weights(T, X, regime="mild", F=F)
    orc = H.gauge_oracle(T, X, N, eps, xp, vp, arch='conv3D')
    tm = TorchGaugeModel(T, X, N, eps, orc.mask, xp, vp, arch='conv3D', dtype=dtype)
    D = 2 * T * X
    rng = np.random.default_rng(7)
    x = rng.uniform(0, 2 * np.pi, (B, D))
    z = rng.standard_normal((B, D))
    dx = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    dz = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    return xp, vp, orc.mask, tm, x, z, dx, dz


@pytest.mark.parametrize("T,X,F,N,B", list(CC.TRAIN_CASES))
def test_conv3d_loss_gradients_match_autograd_at_any_shape(la, T, X, F, N, B):
    """GaugeTrainer.calc_loss_and_grads = taped conv3d_front_kernel<0, 0> forward + conv3d_front_bwd_kernel<0, 0>
    (winner routing, transposed convolutions, per-workgroup filter partials) + the dense trunk's products, against
    float64 autograd of TorchGaugeModel."""
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    beta = 2.5
    cpw = CC.TRAIN_CASES[T, X, F, N, B]
    assert _conv_cpw(T, X, F) == cpw and not CC.is_instance(T, X, F)
    assert (CC.bwd_entries(F) > CC.BWD_SLOT_ENTRIES) == (F == 20)      # entries only the wider-filter-set loop adds up
    assert CC.single_call_trunk(T, X, F) == ((T, X, F) == (4, 16, 8))   # the one-launch trunk reverse of 8 x 8 / F = 8
    xp, vp, masks, tm, x, z, dx, dz = train_reference(T, X, F, N, B)
    if F == X:
        dyn = H.gauge_hip(T, X, N, 0.1, xp, vp, masks, B, arch='conv3D')
    else:
        dxp, dvp = H.conv_weights(T, X, regime="mild")
        dyn = H.gauge_hip(T, X, N, 0.1, dxp, dvp, masks, B, arch='conv3D')
        dyn.position_fn = _conv_net(la, T, X, F, B, 'position', 2.)
        dyn.momentum_fn = _conv_net(la, T, X, F, B, 'momentum', 1.)
        dyn.position_fn.load_state(xp)
        dyn.momentum_fn.load_state(vp)
    tr = GaugeTrainer(dyn, metric='cos_diff', lr_init=1e-3)
    loss, *_ = tr.calc_loss_and_grads(x, beta, z=z, draws_x=dx, draws_z=dz)
    first = tr.grads.clone()
    want_loss, _ = _ref_grads(tm, x, z, dx, dz, beta, 'cos_diff')
    lerr = abs(float(loss) - want_loss) / max(1., abs(want_loss))
    gv = tr.grad_views()
    errs = {f"{n}.{k}": float(np.abs(gv[n][k].cpu().numpy().astype(np.float64).reshape(w.shape) - w).max()
                              / np.abs(w).max())
            for n, net in (("xnet", tm.xnet), ("vnet", tm.vnet)) for k, w in _packed_ref(net).items()}
    top = sorted(errs, key=errs.get, reverse=True)[:3]
    eerr = abs(float(gv["eps"][0]) - float(tm.eps.grad)) / abs(float(tm.eps.grad))
    print(f"train {T}x{X} F={F} N={N} B={B}: loss {lerr:.2e}, eps {eerr:.2e}, worst tensors "
          + ", ".join(f"{k} {errs[k]:.2e}" for k in top))
    assert {"xnet.w1_a", "xnet.w2_b", "vnet.b1_a", "vnet.b2_b", "xnet.w1_t"} <= set(errs)
    assert lerr <= 2e-4
    worst = _compare(tr, tm)
    assert max(worst.values()) <= TOL_G
    # the dd = 1 slice of the second kernel only multiplies padding
    for n in ("xnet", "vnet"):
        for k in ("w2_a", "w2_b"):
            assert float(gv[n][k].reshape(2, 2, 2, F, 2 * F)[:, :, 1].abs().max()) == 0.0, (n, k)
    # no float atomics, fixed summation orders: a second call gives the same bits
    tr.calc_loss_and_grads(x, beta, z=z, draws_x=dx, draws_z=dz)
    assert torch.equal(first, tr.grads)
