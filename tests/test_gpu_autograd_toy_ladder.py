"""torch.autograd through the toy-target Dynamics with one temperature per chain: `propose(..., temperature=ladder)`,
`Dynamics.forward / .backward / .both(..., temperature=ladder)` (l2hmc_amd/autograd_toy.py on
l2hmc_small_trajectory_tempered and l2hmc_small_vjp_tempered).

Three temperatures {1, 1.7, 2.5} lie on the chains in the fixed non-periodic pattern of tests/toy_ladder_ref.py.
  1., 2. the two entries: a rung's rows have the bits of the scalar entry at its temperature; 3., 4. float64 autograd
  (toy_ladder_ref.LadderDynamicsModel) at the gate tests/test_gpu_small_train_ladder.py holds the same inputs to;
  5. plumbing, draws, a scalar temperature=, and the trainer."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import toy_cases as TC
from tests import toy_ladder_ref as TL
from tests.test_gpu_autograd_toy import TOL_G, _compare_to_oracle, _far_from, _flat, _rel, _requires_grad, _t64

pytestmark = pytest.mark.gpu


def _dynamics(c, temperature=1.0, hmc=False):
    """A Dynamics of the case that no trainer owns (toy_ladder_ref.trainer's, without the trainer)."""
    import l2hmc_amd as la
    i = TL.inputs(c)
    dyn = la.Dynamics(i["dim"], TL.library_energy(la, c.kind), trajectory_length=c.N, eps=c.eps, hmc=hmc,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=c.H),
                      use_temperature=True)
    dyn.temperature = temperature
    dyn.set_masks(i["masks"])
    if not hmc:
        dyn.XNet.load_state(i["xp"])
        dyn.VNet.load_state(i["vp"])
    return dyn


def _dev(dyn, a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device=dyn._device)


def _stacked(dyn, c):
    """Both directions of the case's x chains stacked: rows i (forward) and B + i (backward) are chain i."""
    i = TL.inputs(c)
    x = _dev(dyn, i["x"])
    xx = torch.cat([x, x])
    vv = torch.cat([_dev(dyn, i["dx"][0]), _dev(dyn, i["dx"][1])])
    dirs = torch.cat([torch.zeros(c.B, dtype=torch.int32), torch.ones(c.B, dtype=torch.int32)]).to(dyn._device)
    return xx, vv, dirs


def _trajectory(dyn, temps, x0, v0, dirs, chains=None):
    """`temps` a float: l2hmc_small_trajectory on a plan at that temperature; a float32 device tensor [C] / [1]:
    l2hmc_small_trajectory_tempered (stride 1 / 0), the plan's own temperature set to a value no rung has."""
    from l2hmc_amd import _lib
    R = x0.shape[0]
    X, V = torch.full_like(x0, 7.), torch.full_like(x0, 7.)
    ld, p = (torch.full((R,), 7., device=x0.device) for _ in range(2))
    plan = dyn._plan()
    if isinstance(temps, float):
        plan.target.temperature = temps
        _lib.call("l2hmc_small_trajectory", C.byref(plan), x0, v0, dirs, R, X, V, ld, p, device=x0.device)
    else:
        plan.target.temperature = 7.25          # ignored by the entry
        _lib.call("l2hmc_small_trajectory_tempered", C.byref(plan), temps, int(temps.numel() > 1),
                  chains if chains is not None else temps.numel(), x0, v0, dirs, R, X, V, ld, p, device=x0.device)
    return dict(x_out=X, v_out=V, sumlogdet=ld, p_accept=p)


def _rung_rows(c, dev):
    rung = TL.rung_of(c.B)
    for g, t in enumerate(TL.RUNGS):
        ch = np.nonzero(rung == g)[0]
        yield float(t), torch.as_tensor(np.concatenate([ch, c.B + ch]), device=dev)


# ---- 1. l2hmc_small_trajectory_tempered ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TL.ONE_LAUNCH_CASES, ids=TL.case_id)
def test_trajectory_rows_of_a_rung_have_the_bits_of_the_scalar_entry(c):
    dyn = _dynamics(c)
    x0, v0, dirs = _stacked(dyn, c)
    temps = _dev(dyn, TL.ladder(c.B))
    for form in TC.forms(c.H):
        dyn.first_layer_form = form
        lad = _trajectory(dyn, temps, x0, v0, dirs)
        assert all(bool(torch.isfinite(lad[k]).all()) for k in lad), form
        seen = 0
        for g, (t, rows) in enumerate(_rung_rows(c, dyn._device)):
            ref = _trajectory(dyn, t, x0, v0, dirs)
            for k in lad:
                assert torch.equal(lad[k][rows], ref[k][rows]), (k, t, form)
            if g:              # ... and the temperature matters
                seen += int(not torch.equal(lad["x_out"][rows], first["x_out"][rows]))
            else:
                first = ref
        assert seen == 2
        # equal values, stride 1 and stride 0 (chains = B and chains = 1), are the scalar entry
        want = _trajectory(dyn, 1.7, x0, v0, dirs)
        for tt, chains in ((torch.full((c.B,), 1.7, device=dyn._device), c.B),
                           (torch.full((1,), 1.7, device=dyn._device), c.B), (torch.full((1,), 1.7, device=dyn._device), 1)):
            got = _trajectory(dyn, tt, x0, v0, dirs, chains)
            for k in want:
                assert torch.equal(got[k], want[k]), (k, chains, form)
    # one row
    one = _trajectory(dyn, temps[1:2].contiguous(), x0[1:2].contiguous(), v0[1:2].contiguous(), None)
    ref = _trajectory(dyn, float(TL.ladder(c.B)[1]), x0[1:2].contiguous(), v0[1:2].contiguous(), None)
    for k in one:
        assert torch.equal(one[k], ref[k]), k


def test_trajectory_tempered_serves_an_hmc_plan():
    c = TL.MOG
    dyn = _dynamics(c, hmc=True)
    x0, v0, dirs = _stacked(dyn, c)
    lad = _trajectory(dyn, _dev(dyn, TL.ladder(c.B)), x0, v0, dirs)
    for t, rows in _rung_rows(c, dyn._device):
        ref = _trajectory(dyn, t, x0, v0, dirs)
        for k in lad:
            assert torch.equal(lad[k][rows], ref[k][rows]), (k, t)


# ---- 2. l2hmc_small_vjp_tempered -------------------------------------------------------------------------------------
def _vjp(dyn, temps, x0, v0, dirs, cot):
    from l2hmc_amd import _lib, autograd_toy
    dev = x0.device
    R = x0.shape[0]
    plan, L = dyn._plan(), _lib.lib()          # (packs the weights: the segments below are the packed buffers)
    n = sum(t.numel() for net in (dyn.XNet, dyn.VNet) for t in autograd_toy._segments(net).values()) + 1
    grads = torch.full((n,), float("nan"), device=dev)
    outs = [torch.full_like(x0, 7.) for _ in range(4)] + [torch.full((R,), 7., device=dev) for _ in range(2)]
    nb = max(int(L.l2hmc_small_train_ws_bytes(C.byref(plan), R)), 256)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    tail = (x0, v0, dirs, R, *cot, outs[0], outs[1], grads, *outs[2:], ws, nb)
    if isinstance(temps, float):
        plan.target.temperature = temps
        _lib.call("l2hmc_small_vjp", C.byref(plan), *tail, device=dev)
    else:
        plan.target.temperature = 7.25          # ignored by the entry
        _lib.call("l2hmc_small_vjp_tempered", C.byref(plan), temps, int(temps.numel() > 1), x0.shape[0] // 2, *tail,
                  device=dev)
    return dict(zip(("dx0", "dv0", "x_out", "v_out", "sumlogdet", "p_accept"), outs), grads=grads)


@pytest.mark.parametrize("c", TL.ONE_LAUNCH_CASES, ids=TL.case_id)
def test_vjp_rows_of_a_rung_have_the_bits_of_the_scalar_entry(c):
    dyn = _dynamics(c)
    x0, v0, dirs = _stacked(dyn, c)
    R, D = x0.shape
    rng = np.random.default_rng(23)
    cot = [_dev(dyn, TC.f32(rng.standard_normal(s))) for s in ((R, D), (R, D), R, R)]
    lad = _vjp(dyn, _dev(dyn, TL.ladder(c.B)), x0, v0, dirs, cot)
    assert all(bool(torch.isfinite(v).all()) for v in lad.values())
    assert float(lad["dx0"].abs().max()) > 0 and float(lad["dv0"].abs().max()) > 0
    for t, rows in _rung_rows(c, dyn._device):
        ref = _vjp(dyn, t, x0, v0, dirs, cot)
        for k in lad:
            if k != "grads":
                assert torch.equal(lad[k][rows], ref[k][rows]), (k, t)
    want = _vjp(dyn, 1.7, x0, v0, dirs, cot)
    for temps in (np.full(c.B, 1.7), np.full(1, 1.7)):          # stride 1, B equal values; stride 0, one value
        got = _vjp(dyn, _dev(dyn, temps), x0, v0, dirs, cot)
        for k in want:
            assert torch.equal(got[k], want[k]), (k, temps.shape)


# ---- 3. float64, the MoG loss ----------------------------------------------------------------------------------------
def _mog_loss(dyn, i, temperature):
    """mog_model.py:336-355 written in plain torch on two `propose` calls at `temperature`."""
    import l2hmc_amd as la
    x, z = _dev(dyn, i["x"]), _dev(dyn, i["z"])
    dx, dz = i["dx"], i["dz"]
    Lx, _, px, out = la.propose(x, dyn, init_v=dx[0], init_v_backward=dx[1], dir_bits=dx[2], u=dx[3], do_mh_step=True,
                                temperature=temperature)
    Lz, _, pz, _ = la.propose(z, dyn, init_v=dz[0], init_v_backward=dz[1], dir_bits=dz[2], temperature=temperature)
    v1 = ((x - Lx) ** 2).sum(1) * px + 1e-4
    v2 = ((z - Lz) ** 2).sum(1) * pz + 1e-4
    loss = TL.SCALE * ((1. / v1).mean() + (1. / v2).mean()) + (-v1.mean() - v2.mean()) / TL.SCALE
    return loss, out[0], torch.cat([Lx, Lz]), torch.cat([px, pz])


@pytest.mark.parametrize("c", TL.GRADIENT_CASES, ids=TL.case_id)
def test_mog_loss_on_a_ladder_matches_float64(c):
    dyn = _dynamics(c, temperature=3.0)
    _requires_grad(dyn)
    loss, out, L, p = _mog_loss(dyn, TL.inputs(c), TL.ladder(c.B))
    assert loss.grad_fn is not None and out.grad_fn is not None
    loss.backward()
    tm, want, _, Lw, pw = TL.reference(c)
    e_prop = TC.relerr(L.detach().cpu().numpy(), Lw)
    e_p = float(np.abs(p.detach().cpu().numpy() - pw).max())
    worst = _compare_to_oracle(dyn, tm, tol=np.inf)
    print(f"ladder {TL.case_id(c)}: proposals {e_prop:.3g}, p {e_p:.3g}, loss {float(loss.detach()):.6g} against "
          f"{want:.6g}, worst gradient ratio {max(worst.values()):.3g} ({max(worst, key=worst.get)})")
    assert abs(float(loss.detach()) - want) <= 2e-4 * max(1., abs(want))
    _compare_to_oracle(dyn, tm)
    assert dyn.temperature == 3.0


# ---- 4. float64, every output and both inputs ------------------------------------------------------------------------
def test_every_output_and_both_inputs_match_float64_on_a_ladder():
    """tests/test_gpu_autograd_toy.py::test_every_output_and_both_inputs_match_float64 with chain i at temperature[i]."""
    import l2hmc_amd as la
    c = TL.Case("mog", 50, 5, 0.1, 37, "mild", 11, False)
    dyn = _dynamics(c)
    temps = TL.ladder(c.B)
    tm = TL.model(c, temps)
    B, D = c.B, 2
    bits = TL.inputs(c)["dx"][2]
    rng = np.random.default_rng(17)
    x = rng.normal(0.5, 0.4, (B, D))
    v = rng.standard_normal((B, D))
    with torch.no_grad():
        _, _, pf, _ = tm.trajectory(_t64(x), _t64(v), None, False)
        _, _, pb, _ = tm.trajectory(_t64(x), _t64(v), None, True)
    p_sel = np.where(bits > 0.5, pf.numpy(), pb.numpy())
    u = _far_from(p_sel, rng.uniform(size=B))
    assert 0 < ((p_sel - u) >= 0).sum() < B and (p_sel < 1).any()
    cs = [rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.standard_normal(B), rng.standard_normal((B, D)),
          rng.standard_normal(B)] + [rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.standard_normal(B)] * 2
    _requires_grad(dyn)
    xg, vg = _dev(dyn, x).requires_grad_(), _dev(dyn, v).requires_grad_()
    kw = dict(temperature=temps)
    Lx, Lv, px, outs = la.propose(xg, dyn, init_v=vg, dir_bits=bits, u=u, do_mh_step=True, **kw)
    _, _, ldx, _ = la.propose(xg, dyn, init_v=vg, dir_bits=bits, log_jac=True, **kw)
    got = [Lx, Lv, px, outs[0], ldx, *dyn.forward(xg, init_v=vg, log_jac=True, **kw),
           *dyn.backward(xg, init_v=vg, log_jac=True, **kw)]
    sum((_dev(dyn, ci) * o).sum() for ci, o in zip(cs, got)).backward()
    x64, v64 = _t64(x).requires_grad_(), _t64(v).requires_grad_()
    Xf, Vf, Pf, LDf = tm.trajectory(x64, v64, None, False)
    Xb, Vb, Pb, LDb = tm.trajectory(x64, v64, None, True)
    m = _t64(bits)
    mix = lambda a, b: (m[:, None] * a + (1 - m)[:, None] * b) if a.dim() == 2 else m * a + (1 - m) * b  # noqa: E731
    Lx64, p64 = mix(Xf, Xb), mix(Pf, Pb)
    acc = ((p64 - _t64(u)) >= 0).to(torch.float64)[:, None]
    want = [Lx64, mix(Vf, Vb), p64, acc * Lx64 + (1 - acc) * x64, mix(LDf, LDb), Xf, Vf, LDf, Xb, Vb, LDb]
    sum((_t64(ci) * o).sum() for ci, o in zip(cs, want)).backward()
    worst = _compare_to_oracle(dyn, tm)
    worst["x"], worst["init_v"] = _rel(xg.grad, x64.grad), _rel(vg.grad, v64.grad)
    assert worst["x"] <= TOL_G and worst["init_v"] <= TOL_G, worst


# ---- 5. plumbing and draws -------------------------------------------------------------------------------------------
def test_ladder_plumbing_is_exact():
    """The Function's gradients are, bit for bit, those of a direct l2hmc_small_vjp_tempered on the same rows."""
    from l2hmc_amd import autograd_toy
    c = TL.MOG
    dyn = _dynamics(c)
    i = TL.inputs(c)
    temps = _dev(dyn, TL.ladder(c.B))
    B, D = i["x"].shape
    rng = np.random.default_rng(3)
    cot = [_dev(dyn, rng.standard_normal(s)) for s in ((B, D), (B, D), B)]
    _requires_grad(dyn)
    xg, vg = _dev(dyn, i["x"]).requires_grad_(), _dev(dyn, i["dx"][1]).requires_grad_()
    out = dyn.backward(xg, init_v=vg, log_jac=True, temperature=temps)
    sum((ci * o).sum() for ci, o in zip(cot, out)).backward()
    dirs = torch.ones(B, dtype=torch.int32, device=dyn._device)
    plan = dyn._plan()
    grads, dx0, dv0 = autograd_toy.vjp_grads(dyn, plan, xg.detach(), vg.detach(), dirs, (*cot, None), temps=temps)
    assert torch.equal(xg.grad, dx0) and torch.equal(vg.grad, dv0)
    gx, gv, deps = autograd_toy.unpack(dyn, grads)
    for net, ref in ((dyn.XNet, gx), (dyn.VNet, gv)):
        for k, t in net.state_dict().items():
            assert torch.equal(t.grad, ref[k]), k
    assert torch.equal(dyn.alpha.grad, (deps * float(plan.eps)).cpu().reshape(()))


def test_ladder_calls_take_the_draws_of_the_calls_without_a_graph():
    import l2hmc_amd as la
    c = TL.MOG
    dyn = _dynamics(c)
    x = _dev(dyn, TL.inputs(c)["x"])
    kw = dict(temperature=TL.ladder(c.B))
    _requires_grad(dyn)
    for call in (lambda: la.propose(x, dyn, do_mh_step=True, **kw), lambda: la.propose(x, dyn, **kw),
                 lambda: dyn.forward(x, **kw), lambda: dyn.backward(x, log_jac=True, **kw)):
        dyn._draws = 5
        with torch.no_grad():
            a = call()
        draws_a = dyn._draws
        dyn._draws = 5
        b = call()
        assert dyn._draws == draws_a
        fa, fb = _flat(a), _flat(b)
        assert len(fa) == len(fb) and all(t.grad_fn is not None for t in fb)
        for ta, tb in zip(fa, fb):
            assert torch.equal(ta, tb.detach())
    # ... which are the Philox streams l2hmc_small_propose takes: a ladder of equal values is the one-launch call
    with torch.no_grad():
        dyn._draws = 5
        a = la.propose(x, dyn, do_mh_step=True, temperature=np.full(c.B, 1.7))
        draws_a = dyn._draws
        dyn._draws = 5
        b = la.propose(x, dyn, do_mh_step=True, temperature=1.7)
    assert dyn._draws == draws_a
    for ta, tb in zip(_flat(a), _flat(b)):
        assert torch.equal(ta, tb)


def test_a_scalar_temperature_is_the_call_at_that_dynamics_temperature():
    import l2hmc_amd as la
    c = TL.MOG_16
    i = TL.inputs(c)
    a, b = _dynamics(c, temperature=3.0), _dynamics(c, temperature=1.7)
    kw = dict(init_v=i["dx"][0], init_v_backward=i["dx"][1], dir_bits=i["dx"][2], u=i["dx"][3], do_mh_step=True)
    results = []
    for dyn, extra in ((a, dict(temperature=1.7)), (b, {})):
        _requires_grad(dyn)
        x = _dev(dyn, i["x"]).requires_grad_()
        out = _flat(la.propose(x, dyn, **kw, **extra)) + list(dyn.forward(x, init_v=i["dx"][0], **extra))
        sum(o.sum() for o in out).backward()
        with torch.no_grad():
            plain = _flat(la.propose(x, dyn, **kw, **extra)) + _flat(la.propose(x, dyn, do_mh_step=True, **extra))
        results.append([o.detach() for o in out] + plain + [x.grad] + [v.grad for v in dyn.variables])
    assert a.temperature == 3.0 and a._draws == b._draws
    for ta, tb in zip(*results):
        assert torch.equal(ta, tb)
    with torch.no_grad():          # ... and it is not the call at the dynamics' own temperature
        assert not torch.equal(la.propose(_dev(a, i["x"]), a, **kw)[2], results[0][2])


def test_autograd_on_a_ladder_matches_dynamics_trainer():
    c = TL.MOG
    i = TL.inputs(c)
    tr = TL.trainer(c)
    loss_t, _, _ = tr.calc_loss_and_grads(i["x"], z=i["z"], draws_x=i["dx"], draws_z=i["dz"], temperature=TL.ladder(c.B))
    dyn = _dynamics(c)
    _requires_grad(dyn)
    loss_a, *_ = _mog_loss(dyn, i, TL.ladder(c.B))
    loss_a.backward()
    assert abs(float(loss_a.detach()) - float(loss_t)) <= 2e-4 * max(1., abs(float(loss_t)))
    gv = tr.grad_views()
    worst = {}
    for name, net in (("xnet", dyn.XNet), ("vnet", dyn.VNet)):
        ref = net.unpack_grads(gv[name])
        for k, t in net.state_dict().items():
            worst[f"{name}.{k}"] = _rel(t.grad, ref[k].cpu().double())
    worst["alpha"] = _rel(dyn.alpha.grad, gv["alpha"].cpu().double().reshape(()))
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, f"{bad}\nall: {worst}"
