"""The one-launch toy-target kernels at the limits include/l2hmc_hip.h states (x_dim <= 8, <= 8 mixture components,
<= 64 hidden units), against float64 references, on the cases of tests/toy_cases.py (whose input conditions
tests/test_toy_limits_host.py asserts without a GPU).

  * sampling: Dynamics.forward / .backward (x, v, p and the log-Jacobian) and `propose` on injected draws against
    DynamicsOracle in float64, in every first-layer form the width allows, at 37 chains and at one; every x_dim with a
    width of each instance class of small_launch (H <= 16, 17..50, 51..64), both edges of each class;
  * `propose` on library draws against the piecewise path on the same Philox streams, bit for bit;
  * training: DynamicsTrainer.calc_loss_and_grads, the autograd route and l2hmc_small_vjp alone against float64 autograd
    of oracle.torch_ref.TorchDynamicsModel;
  * l2hmc_mog_energy_grad / _hvp alone against float64 autograd (a double backward);
  * the layer-by-layer path against the one-launch result (a diagnostic: both are held to float64 on their own).

Bars: those of tests/test_gpu_parity.py (`assert_fp32_equivalent` against DynamicsOracle(dtype=float32), and
max(TOL_P, P_RATIO x the float32 oracle's error) for accept probabilities: the float32 oracle itself reaches 1.2e-5
on p over these shapes); TOL_G = 2e-4 per gradient tensor as tests/test_gpu_train.py; 2e-5 for the target entries
as test_mog_energy_hvp_matches_autograd.  Every figure is printed before it is asserted (profiles/toy_limits_parity.txt
is that output)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import toy_cases as tc
from tests.test_gpu_autograd_toy import SCALE, _compare_to_oracle, _mog_loss, _rel, _requires_grad
from tests.test_gpu_parity import TOL_OP, TOL_P, np_
from tests.test_gpu_train import _mlp_packed_ref
from tests.test_gpu_train_layered import _dev, _relmax

pytestmark = pytest.mark.gpu

TOL_G = tc.TOL_G
TOL_TARGET = 2e-5


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _ids(cases):
    return [tc.case_id(c) for c in cases]


def _dynamics(la, c, temperature=1.0):
    _, tgt = tc.target(c.dim, c.K, c.kind)
    xp, vp = tc.nets(c.dim, c.H, c.regime, c.seed)
    dyn = tc.library_dynamics(la, c, tgt, xp, vp, tc.masks(c.N, c.dim, c.seed), temperature)
    assert not dyn.layered
    return dyn


def _sampling_outputs(la, dyn, i):
    """Every output tc.sampling_outputs names, from the library."""
    x = i["x"]
    got = {}
    got["Xf"], got["Vf"], got["pf"] = dyn.forward(x, init_v=i["v0f"])
    got["Xb"], got["Vb"], got["pb"] = dyn.backward(x, init_v=i["v0b"])
    Xf2, Vf2, got["ljf"] = dyn.forward(x, init_v=i["v0f"], log_jac=True)
    Xb2, Vb2, got["ljb"] = dyn.backward(x, init_v=i["v0b"], log_jac=True)
    if not dyn.layered:
        assert torch.equal(Xf2, got["Xf"]) and torch.equal(Vb2, got["Vb"])
    got["Lx"], got["Lv"], got["px"], (got["x_out"],) = la.propose(
        x, dyn, init_v=i["v0f"], do_mh_step=True, init_v_backward=i["v0b"], dir_bits=i["bits"], u=i["u"])
    return {k: np_(v) for k, v in got.items()}


@pytest.mark.parametrize("c", tc.SAMPLING_CASES, ids=_ids(tc.SAMPLING_CASES))
def test_sampling_matches_float64_in_every_first_layer_form(la, c):
    dyn = _dynamics(la, c)
    bad = []
    for B in tc.SAMPLING_BATCHES:
        i = tc.sampling_inputs(c, B)
        w64, w32 = tc.sampling_reference(c, B)
        safe = tc.mh_safe(c, B)
        assert safe.all()                      # nothing is left out of the Metropolis-Hastings comparison
        for form in tc.forms(c.H):
            dyn.first_layer_form = form
            got = _sampling_outputs(la, dyn, i)
            for k in w64:
                sel = safe if k == "x_out" else slice(None)
                fails, fig = tc.check_output(k, got[k][sel], w64[k][sel], w32[k][sel])
                print(tc.report(tc.case_id(c), B, f"form{form}", k, fig))
                bad += [f"B={B} form {form} {k}: {f}" for f in fails]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", tc.PIECEWISE_CASES, ids=_ids(tc.PIECEWISE_CASES))
def test_one_launch_propose_equals_the_piecewise_path_bit_for_bit(la, c):
    """l2hmc_small_propose on library draws against the same streams written out with l2hmc_fill_* and fed to the
    two-direction trajectory launch + l2hmc_mix_accept (as test_generic_dynamics_in_three_dimensions)."""
    from l2hmc_amd import _lib
    dyn = _dynamics(la, c)
    Lh, d0, B = _lib.lib(), 20, 37
    x = tc.sampling_inputs(c, B)["x"]

    def fill(fn, n, off):
        out = torch.empty(n, device="cuda")
        _lib.check(fn(out.data_ptr(), n, dyn._seed, off, None))
        return out
    fb = (fill(Lh.l2hmc_fill_uniform, B, d0) >= 0.5).float()
    fvf = fill(Lh.l2hmc_fill_normal, c.dim * B, d0 + 1).reshape(B, c.dim)
    fvb = fill(Lh.l2hmc_fill_normal, c.dim * B, d0 + 2).reshape(B, c.dim)
    fu = fill(Lh.l2hmc_fill_uniform, B, d0 + 3)
    pLx, _, ppx, pouts = la.propose(x, dyn, init_v=fvf, do_mh_step=True, init_v_backward=fvb, dir_bits=fb, u=fu)
    dyn._draws = d0
    oLx, oLv, opx, oouts = la.propose(x, dyn, do_mh_step=True)
    assert dyn._draws == d0 + 4 and oLv is None
    assert torch.equal(oLx, pLx) and torch.equal(opx, ppx) and torch.equal(oouts[0], pouts[0])
    assert 0 < float(fb.sum()) < B and not torch.equal(oouts[0], oLx) and not torch.equal(oouts[0], _dev(x))


@pytest.mark.parametrize("c", tc.LAYERED_CASES, ids=_ids(tc.LAYERED_CASES))
def test_layer_by_layer_path_agrees_with_the_one_launch_kernels(la, c):
    """A diagnostic: each path is held to float64 on its own (here and in tests/test_gpu_parity.py), so by the
    triangle inequality they sit within twice TOL_OP / TOL_P of each other; on a failure this tells which side
    moved."""
    B = 37
    i = tc.sampling_inputs(c, B)
    dyn = _dynamics(la, c)
    one = _sampling_outputs(la, dyn, i)
    dyn.layered = True
    lay = _sampling_outputs(la, dyn, i)
    w64, _ = tc.sampling_reference(c, B)
    bad = []
    for k in one:
        if k == "x_out":
            continue
        if k in tc.P_OUTPUTS:
            d, bar = float(np.abs(lay[k] - one[k]).max()), 2 * TOL_P
        else:
            d, bar = tc.relerr(lay[k], one[k]), 2 * TOL_OP
        print(f"toy_limits {tc.case_id(c):<28s} B={B:<3d} layered-one {k:<6s} max {d:.2e} | layered-f64 "
              f"{np.abs(lay[k] - w64[k]).max():.2e} one-f64 {np.abs(one[k] - w64[k]).max():.2e}")
        if not d < bar:
            bad.append(f"{k}: {d:.2e} (bar {bar:.2e})")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- training
def _print_worst(c, what, worst):
    for k, v in worst.items():
        print(f"toy_limits {tc.case_id(c):<28s} B={c.B:<3d} {what:<10s} {k:<14s} rel max {v:.2e}")


@pytest.mark.parametrize("c", tc.TRAIN_CASES, ids=_ids(tc.TRAIN_CASES))
def test_training_step_matches_float64_autograd(la, c):
    """l2hmc_small_train_step through DynamicsTrainer.calc_loss_and_grads: proposals, p, the loss and every packed
    gradient tensor of both nets and alpha (metric of test_toy_target_loss_gradients_match_autograd)."""
    from l2hmc_amd.dynamics_trainer import DynamicsTrainer
    i = tc.train_inputs(c)
    tr = DynamicsTrainer(_dynamics(la, c, c.temperature), scale=SCALE)
    loss, x_out, px = tr.calc_loss_and_grads(i["x"], z=i["z"], draws_x=i["dx"], draws_z=i["dz"])
    tm, want, props, p = tc.train_reference(c)
    w64, w32 = tc.train_forward_reference(c)
    fails_x, fig_x = tc.check_output("x", tr.last_proposals.cpu().numpy(), w64["x"], w32["x"])
    fails_p, fig_p = tc.check_output("p", tr.last_p.cpu().numpy(), w64["p"], w32["p"])
    print(tc.report(tc.case_id(c), c.B, "trainer", "x", fig_x))
    print(tc.report(tc.case_id(c), c.B, "trainer", "p", fig_p))
    e_loss = abs(float(loss) - want) / max(1., abs(want))
    gv = tr.grad_views()
    worst = {}
    for name, net in (("xnet", tm.xnet), ("vnet", tm.vnet)):
        for k, w in _mlp_packed_ref(net).items():
            got = gv[name][k].cpu().numpy().astype(np.float64).reshape(w.shape)
            worst[f"{name}.{k}"] = float(np.abs(got - w).max() / np.abs(w).max())
    worst["alpha"] = abs(float(gv["alpha"][0]) - float(tm.alpha.grad)) / abs(float(tm.alpha.grad))
    _print_worst(c, "trainer", dict(loss=e_loss, **worst))
    assert not fails_x and not fails_p, (fails_x, fails_p)
    assert e_loss <= 2e-4
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, f"gradient mismatch: {bad}\nall: {worst}"
    acc = (p[:c.B] - i["dx"][3]) >= 0
    assert np.abs(p[:c.B] - i["dx"][3]).min() > tc.MH_MARGIN
    np.testing.assert_array_equal(x_out.cpu().numpy()[acc], tr.last_proposals[:c.B].cpu().numpy()[acc])
    np.testing.assert_array_equal(x_out.cpu().numpy()[~acc], i["x"][~acc].astype(np.float32))


@pytest.mark.parametrize("c", tc.TRAIN_CASES, ids=_ids(tc.TRAIN_CASES))
def test_autograd_route_matches_float64_autograd(la, c):
    """The reference's loss written in torch around two `propose` calls (l2hmc_amd/autograd_toy.py)."""
    i = tc.train_inputs(c)
    dyn = _dynamics(la, c, c.temperature)
    _requires_grad(dyn)
    loss, out = _mog_loss(dyn, i["x"], i["z"], i["dx"], i["dz"])
    assert loss.grad_fn is not None and out.grad_fn is not None
    loss.backward()
    tm, want, _, _ = tc.train_reference(c)
    e_loss = abs(float(loss.detach()) - want) / max(1., abs(want))
    worst = {}
    for name, net, ref in (("xnet", dyn.XNet, tm.xnet), ("vnet", dyn.VNet, tm.vnet)):
        for k, t in net.state_dict().items():
            assert t.grad is not None, (name, k)
            worst[f"{name}.{k}"] = _rel(t.grad, ref[k].grad)
    worst["alpha"] = _rel(dyn.alpha.grad, tm.alpha.grad)
    _print_worst(c, "autograd", dict(loss=e_loss, **worst))
    assert e_loss <= 2e-4
    _compare_to_oracle(dyn, tm, TOL_G)


@pytest.mark.parametrize("c", tc.TRAIN_CASES, ids=_ids(tc.TRAIN_CASES))
def test_vjp_entry_matches_float64_autograd(la, c):
    """l2hmc_small_vjp alone on the case's stacked x and z chains, each in the direction its bit picks, with all four
    cotangents non-zero: dx0, dv0, every weight gradient and alpha (as test_vjp_entry_matches_float64)."""
    from l2hmc_amd import _lib, autograd_toy
    dyn = _dynamics(la, c, c.temperature)
    x0, v0, dirs = tc.train_rows(c)                         # dirs: 1 = backward
    R, D = x0.shape
    g = tc.vjp_cotangents(c)
    dev = dyn._device
    f = lambda a: _lib.as_dev(a, dev)          # noqa: E731
    plan = dyn._plan()
    L, s = _lib.lib(), _lib.stream_ptr(dev)
    xt, vt, dt = f(x0), f(v0), torch.tensor(dirs, device=dev)
    gs = [f(a) for a in g]
    n_grads = sum(t.numel() for n in (dyn.XNet, dyn.VNet) for t in autograd_toy._segments(n).values()) + 1
    grads = torch.full((n_grads,), 7., device=dev)
    outs = [torch.full((R, D), 7., device=dev) for _ in range(4)] + [torch.full((R,), 7., device=dev) for _ in range(2)]
    nb = L.l2hmc_small_train_ws_bytes(C.byref(plan), R)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(L.l2hmc_small_vjp(C.byref(plan), xt.data_ptr(), vt.data_ptr(), dt.data_ptr(), R,
                                 *[t.data_ptr() for t in gs], outs[0].data_ptr(), outs[1].data_ptr(), grads.data_ptr(),
                                 outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr(),
                                 ws.data_ptr(), nb, s))
    tm, x64, v64, rows = tc.vjp_reference(c)
    # the forward outputs the entry hands out, against the float64 oracle
    w64, w32 = tc.train_forward_reference(c)
    fwd_bad = []
    for k, o in zip(("x", "v", "logdet", "p"), outs[2:]):
        fails, fig = tc.check_output(k, np_(o), w64[k], w32[k])
        print(tc.report(tc.case_id(c), c.B, "vjp", k, fig))
        fwd_bad += [f"{k}: {m}" for m in fails]
    rows.sum().backward()
    worst = {"dx0": _rel(outs[0], x64.grad), "dv0": _rel(outs[1], v64.grad)}
    gx, gv, deps = autograd_toy.unpack(dyn, grads)
    for name, got, ref in (("xnet", gx, tm.xnet), ("vnet", gv, tm.vnet)):
        for k in got:
            worst[f"{name}.{k}"] = _rel(got[k], ref[k].grad)
    worst["alpha"] = _rel(deps * float(plan.eps), tm.alpha.grad)
    _print_worst(c, "vjp", worst)
    assert not fwd_bad, fwd_bad
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, f"gradient mismatch: {bad}\nall: {worst}"


# ------------------------------------------------------------------------------------------- standalone target entries
@pytest.mark.parametrize("temperature", tc.TARGET_TEMPERATURES)
@pytest.mark.parametrize("rows", tc.TARGET_ROWS)
@pytest.mark.parametrize("dim,K,kind", tc.TARGET_CASES)
def test_target_entries_match_float64_autograd(la, dim, K, kind, rows, temperature):
    """l2hmc_mog_energy_grad and l2hmc_mog_energy_hvp on rows drawn from the target plus rows 3 sigma away from every
    mean (metric and bar of test_mog_energy_hvp_matches_autograd)."""
    from l2hmc_amd import _lib
    _, tgt = tc.target(dim, K, kind)
    x, u = tc.target_points(dim, K, kind, rows)
    e64, g64, hv64 = tc.target_reference(dim, K, kind, rows, temperature)
    packed = tgt.get_energy_function().target          # held: struct() points into its device buffers
    st = packed.struct(temperature)
    xd, ud = _dev(x), _dev(u)
    e, g, hv = torch.full((rows,), 7., device="cuda"), torch.full((rows, dim), 7., device="cuda"), \
        torch.full((rows, dim), 7., device="cuda")
    L, s = _lib.lib(), _lib.stream_ptr()
    _lib.check(L.l2hmc_mog_energy_grad(C.byref(st), xd.data_ptr(), rows, e.data_ptr(), g.data_ptr(), s))
    _lib.check(L.l2hmc_mog_energy_hvp(C.byref(st), xd.data_ptr(), ud.data_ptr(), rows, hv.data_ptr(), s))
    errs = dict(energy=_relmax(e, e64), grad=_relmax(g, g64), hvp=_relmax(hv, hv64))
    for k, v in errs.items():
        print(f"toy_limits target d{dim}-K{K}{kind[0]} rows={rows:<3d} T={temperature} {k:<6s} rel max {v:.2e}")
    bad = {k: v for k, v in errs.items() if not v < TOL_TARGET}
    assert not bad, bad
