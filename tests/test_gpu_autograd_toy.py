"""torch.autograd through the toy-target Dynamics (l2hmc_amd/autograd_toy.py): a loss written in torch around
`propose` / `Dynamics.forward` / `.backward` -- the reference's own MoG loss (mog_model.py:324-355) and arbitrary
linear functionals of every output -- differentiated through l2hmc_small_vjp, against float64 autograd on the torch
restatement (oracle/torch_ref.py), against DynamicsTrainer, and against direct calls of the C ABI.

Tolerances as tests/test_gpu_train.py: gradients per tensor in the max norm relative to the tensor's largest
entry at TOL_G = 2e-4."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_train import _small_setup

pytestmark = pytest.mark.gpu

TOL_G = 2e-4
SCALE = 0.1


def _fresh(dyn_t, tm):
    """A Dynamics no trainer owns, with the weights, masks, target and temperature of the trainer's."""
    import l2hmc_amd as la
    H_nodes = dyn_t.XNet.num_nodes
    dyn = la.Dynamics(dyn_t.x_dim, dyn_t._fn, trajectory_length=dyn_t.trajectory_length, eps=float(dyn_t.eps.detach()),
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=H_nodes),
                      use_temperature=True)
    dyn.temperature = dyn_t.temperature
    dyn.set_masks(dyn_t.mask.cpu().numpy())
    dyn.XNet.load_state({k: v.detach().numpy() for k, v in tm.xnet.items()})
    dyn.VNet.load_state({k: v.detach().numpy() for k, v in tm.vnet.items()})
    return dyn


def _setup(kind, H_nodes, N, eps, B, regime, temperature=1.0, seed=11):
    tr, tm, x, z, dx, dz = _small_setup(kind, H_nodes, N, eps, B, regime, seed=seed, temperature=temperature)
    return _fresh(tr.dynamics, tm), tr, tm, x, z, dx, dz


def _requires_grad(dyn):
    for v in dyn.variables:
        v.requires_grad_()
        v.grad = None


def _mog_loss(dyn, x, z, dx, dz):
    """mog_model.py:336-355 written in plain torch on two `propose` calls."""
    import l2hmc_amd as la
    x, z = (torch.as_tensor(a, dtype=torch.float32, device=dyn._device) for a in (x, z))
    Lx, _, px, out = la.propose(x, dyn, init_v=dx[0], init_v_backward=dx[1], dir_bits=dx[2], u=dx[3], do_mh_step=True)
    Lz, _, pz, _ = la.propose(z, dyn, init_v=dz[0], init_v_backward=dz[1], dir_bits=dz[2])
    v1 = ((x - Lx) ** 2).sum(1) * px + 1e-4
    v2 = ((z - Lz) ** 2).sum(1) * pz + 1e-4
    return SCALE * ((1. / v1).mean() + (1. / v2).mean()) + (-v1.mean() - v2.mean()) / SCALE, out[0]


def _t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _rel(got, want):
    want = want.detach()
    got = got.detach().cpu().double().reshape(want.shape)
    scale = float(want.abs().max())
    assert scale > 0
    return float((got - want).abs().max()) / scale


def _compare_to_oracle(dyn, tm, tol=TOL_G):
    worst = {}
    for name, net, ref in (("xnet", dyn.XNet, tm.xnet), ("vnet", dyn.VNet, tm.vnet)):
        for k, t in net.state_dict().items():
            assert t.grad is not None, (name, k)
            worst[f"{name}.{k}"] = _rel(t.grad, ref[k].grad)
    worst["alpha"] = _rel(dyn.alpha.grad, tm.alpha.grad)
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, f"gradient mismatch: {bad}\nall: {worst}"
    return worst


@pytest.mark.parametrize("kind,H_nodes,N,eps,B,regime,temp", [
    ("mog", 50, 5, 0.1, 37, "stress", 1.0),        # cfg 2 widths, ragged batch (3 workgroups, one partly empty)
    ("mog", 50, 10, 0.1, 16, "mild", 2.5),         # full trajectory length, tempered target
    ("scg", 10, 5, 0.1, 21, "stress", 1.0),        # cfg 1: 16-wide kernel variant, Gaussian target
    ("mog3", 50, 4, 0.1, 19, "stress", 1.0),       # x_dim 3, three components: run-time-dimension instance, H = 50
    ("mog3", 12, 3, 0.1, 9, "mild", 1.5),          # ... and its 16-wide variant
])
def test_reference_mog_loss_through_autograd_matches_float64(kind, H_nodes, N, eps, B, regime, temp):
    dyn, _, tm, x, z, dx, dz = _setup(kind, H_nodes, N, eps, B, regime, temperature=temp)
    _requires_grad(dyn)
    loss, out = _mog_loss(dyn, x, z, dx, dz)
    assert loss.grad_fn is not None and out.grad_fn is not None
    loss.backward()
    want, *_ = tm.mog_loss(_t64(x), _t64(z), tuple(map(_t64, dx)), tuple(map(_t64, dz)), SCALE)
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 2e-4 * max(1., abs(float(want.detach())))
    _compare_to_oracle(dyn, tm)


def _far_from(p, u):
    """MH uniforms kept off p, where fp32 and fp64 could select apart."""
    return np.where(np.abs(p - u) < 1e-3, 0.5 * p, u)


def test_every_output_and_both_inputs_match_float64():
    """A random linear functional of Lx, Lv, px, outputs[0] of propose (with init_v), px of propose(log_jac=True),
    and (X, V, sumlogdet) of forward / backward(log_jac=True): gradients of x, init_v, alpha and every weight."""
    import l2hmc_amd as la
    dyn, _, tm, _, _, dx, _ = _setup("mog", 50, 5, 0.1, 45, "mild")
    B, D = 45, 2
    rng = np.random.default_rng(17)
    x = rng.normal(0.5, 0.4, (B, D))
    v = rng.standard_normal((B, D))
    bits = dx[2]
    with torch.no_grad():
        xf, _, pf, _ = tm.trajectory(_t64(x), _t64(v), None, False)
        xb, _, pb, _ = tm.trajectory(_t64(x), _t64(v), None, True)
    p_sel = np.where(bits > 0.5, pf.numpy(), pb.numpy())
    u = _far_from(p_sel, rng.uniform(size=B))
    assert 0 < ((p_sel - u) >= 0).sum() < B and (p_sel < 1).any()
    c = [rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.standard_normal(B), rng.standard_normal((B, D)),
         rng.standard_normal(B)] + [rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.standard_normal(B)] * 2
    _requires_grad(dyn)
    dev = dyn._device
    xg = torch.tensor(x, dtype=torch.float32, device=dev, requires_grad=True)
    vg = torch.tensor(v, dtype=torch.float32, device=dev, requires_grad=True)
    Lx, Lv, px, outs = la.propose(xg, dyn, init_v=vg, dir_bits=bits, u=u, do_mh_step=True)
    _, _, ldx, _ = la.propose(xg, dyn, init_v=vg, dir_bits=bits, log_jac=True)
    got = [Lx, Lv, px, outs[0], ldx, *dyn.forward(xg, init_v=vg, log_jac=True), *dyn.backward(xg, init_v=vg, log_jac=True)]
    cg = [torch.tensor(a, dtype=torch.float32, device=dev) for a in c]
    sum((ci * o).sum() for ci, o in zip(cg, got)).backward()
    x64, v64 = _t64(x).requires_grad_(), _t64(v).requires_grad_()
    Xf, Vf, Pf, LDf = tm.trajectory(x64, v64, None, False)
    Xb, Vb, Pb, LDb = tm.trajectory(x64, v64, None, True)
    m = _t64(bits)
    mix = lambda a, b: (m[:, None] * a + (1 - m)[:, None] * b) if a.dim() == 2 else m * a + (1 - m) * b  # noqa: E731
    Lx64, p64 = mix(Xf, Xb), mix(Pf, Pb)
    acc = ((p64 - _t64(u)) >= 0).to(torch.float64)[:, None]
    want = [Lx64, mix(Vf, Vb), p64, acc * Lx64 + (1 - acc) * x64, mix(LDf, LDb), Xf, Vf, LDf, Xb, Vb, LDb]
    sum((_t64(ci) * o).sum() for ci, o in zip(c, want)).backward()
    worst = _compare_to_oracle(dyn, tm)
    worst["x"], worst["init_v"] = _rel(xg.grad, x64.grad), _rel(vg.grad, v64.grad)
    assert worst["x"] <= TOL_G and worst["init_v"] <= TOL_G, worst


def test_vjp_entry_matches_float64():
    """l2hmc_small_vjp alone: random cotangents on all four outputs, mixed directions, 37 rows (the last workgroup
    partly empty); dx0, dv0 and grads against the float64 VJP of the trajectory, H0 term included."""
    from l2hmc_amd import _lib, autograd_toy
    dyn, _, tm, _, _, _, _ = _setup("mog", 50, 4, 0.1, 37, "stress")
    R, D = 37, 2
    rng = np.random.default_rng(23)
    x0, v0 = rng.normal(0.5, 0.4, (R, D)), rng.standard_normal((R, D))
    dirs = (rng.uniform(size=R) < 0.5).astype(np.int32)
    g = [rng.standard_normal((R, D)), rng.standard_normal((R, D)), rng.standard_normal(R), rng.standard_normal(R)]
    dev = dyn._device
    f = lambda a: _lib.as_dev(a, dev)          # noqa: E731
    plan = dyn._plan()
    L, s = _lib.lib(), _lib.stream_ptr(dev)
    xt, vt, dt = f(x0), f(v0), torch.tensor(dirs, device=dev)
    gs = [f(a) for a in g]
    grads = torch.full((sum(t.numel() for n in (dyn.XNet, dyn.VNet) for t in autograd_toy._segments(n).values()) + 1,),
                       7., device=dev)
    outs = [torch.full((R, D), 7., device=dev) for _ in range(4)] + [torch.full((R,), 7., device=dev) for _ in range(2)]
    nb = L.l2hmc_small_train_ws_bytes(C.byref(plan), R)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(L.l2hmc_small_vjp(C.byref(plan), xt.data_ptr(), vt.data_ptr(), dt.data_ptr(), R,
                                 *[t.data_ptr() for t in gs], outs[0].data_ptr(), outs[1].data_ptr(), grads.data_ptr(),
                                 outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr(),
                                 ws.data_ptr(), nb, s))
    # the optional forward outputs: those of l2hmc_small_trajectory on the same rows
    X, V = torch.empty_like(xt), torch.empty_like(xt)
    ld, p = torch.empty(R, device=dev), torch.empty(R, device=dev)
    _lib.check(L.l2hmc_small_trajectory(C.byref(plan), xt.data_ptr(), vt.data_ptr(), dt.data_ptr(), R, X.data_ptr(),
                                        V.data_ptr(), ld.data_ptr(), p.data_ptr(), s))
    for a, b in zip(outs[2:], (X, V, ld, p)):
        assert float((a - b).abs().max()) <= 1e-5 * max(1., float(b.abs().max()))
    # float64 VJP, row by row in its direction
    x64, v64 = _t64(x0).requires_grad_(), _t64(v0).requires_grad_()
    fw = torch.tensor(dirs == 0)
    res = [tm.trajectory(x64, v64, None, bwd) for bwd in (False, True)]
    pick = lambda i: torch.where(fw[:, None] if res[0][i].dim() == 2 else fw, res[0][i], res[1][i])  # noqa: E731
    Xw, Vw, Pw, LDw = pick(0), pick(1), pick(2), pick(3)
    assert ((Pw.detach().numpy() < 1) & fw.numpy()).sum() > 3 and ((Pw.detach().numpy() < 1) & ~fw.numpy()).sum() > 3
    ((_t64(g[0]) * Xw).sum() + (_t64(g[1]) * Vw).sum() + (_t64(g[2]) * LDw).sum() + (_t64(g[3]) * Pw).sum()).backward()
    worst = {"dx0": _rel(outs[0], x64.grad), "dv0": _rel(outs[1], v64.grad)}
    gx, gv, deps = autograd_toy.unpack(dyn, grads)
    for name, got, ref in (("xnet", gx, tm.xnet), ("vnet", gv, tm.vnet)):
        for k in got:
            worst[f"{name}.{k}"] = _rel(got[k], ref[k].grad)
    worst["alpha"] = _rel(deps * float(plan.eps), tm.alpha.grad)
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, f"gradient mismatch: {bad}\nall: {worst}"


def test_autograd_matches_dynamics_trainer():
    """Same weights, same draws, same loss: DynamicsTrainer's one-launch step and the autograd path at cfg-2 widths
    with initial weights.  The autograd seed comes from l2hmc_small_trajectory's outputs, the trainer's from its own
    recomputed forward; the two agree to rounding (p within 4e-6), and the x/z row grouping differs.  Measured on
    MI355X: loss within 1e-7, gradients within 6.6e-6 of each tensor's scale.  (With trained-looking weights a chain
    whose v = |x - x_N|^2 p + 1e-4 sits near 1e-4 amplifies that p rounding in 1/v^2: 3e-3 at 300 chains.)"""
    dyn, tr, _, x, z, dx, dz = _setup("mog", 50, 10, 0.1, 300, "init")
    loss_t, _, _ = tr.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
    _requires_grad(dyn)
    loss_a, _ = _mog_loss(dyn, x, z, dx, dz)
    loss_a.backward()
    assert abs(float(loss_a.detach()) - float(loss_t)) <= 1e-5 * abs(float(loss_t))
    gv = tr.grad_views()
    worst = {}
    for name, net in (("xnet", dyn.XNet), ("vnet", dyn.VNet)):
        ref = net.unpack_grads(gv[name])
        for k, t in net.state_dict().items():
            worst[f"{name}.{k}"] = _rel(t.grad, ref[k].cpu().double())
    worst["alpha"] = _rel(dyn.alpha.grad, gv["alpha"].cpu().double().reshape(()))
    bad = {k: v for k, v in worst.items() if not v <= 2e-5}
    assert not bad, f"{bad}\nall: {worst}"


def _flat(r):
    out = []
    for t in r:
        if isinstance(t, list):
            out += t
        elif t is not None:
            out.append(t)
    return out


def test_same_draws_as_the_sampling_path():
    """Library draws: the differentiable propose / forward / backward return what the no-grad calls return, bit for
    bit, and advance _draws alike (propose: the Philox streams of l2hmc_small_propose)."""
    import l2hmc_amd as la
    dyn, _, _, x, _, _, _ = _setup("mog", 50, 10, 0.1, 200, "mild")
    x = torch.as_tensor(x, dtype=torch.float32, device=dyn._device)
    _requires_grad(dyn)
    for call in (lambda: la.propose(x, dyn, do_mh_step=True), lambda: la.propose(x, dyn),
                 lambda: dyn.forward(x), lambda: dyn.backward(x, log_jac=True)):
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


def test_plumbing_is_exact():
    """The Function's gradients are, bit for bit, those of a direct l2hmc_small_vjp on the same rows after
    unpack_grads; two backward runs of the same loss give the same bits."""
    from l2hmc_amd import _lib, autograd_toy
    dyn, _, _, x, _, dx, _ = _setup("mog", 50, 5, 0.1, 40, "mild")
    B, D = x.shape
    dev = dyn._device
    rng = np.random.default_rng(3)
    c = [torch.tensor(rng.standard_normal(s), dtype=torch.float32, device=dev) for s in ((B, D), (B, D), B, B)]
    _requires_grad(dyn)
    runs = []
    for _ in range(2):
        for v in dyn.variables:
            v.grad = None
        xg = torch.tensor(x, dtype=torch.float32, device=dev, requires_grad=True)
        vg = _lib.as_dev(dx[0], dev).requires_grad_()
        out = dyn.backward(xg, init_v=vg, log_jac=True)
        p = dyn.backward(xg, init_v=vg)[2]
        ((c[0] * out[0]).sum() + (c[1] * out[1]).sum() + (c[2] * out[2]).sum() + (c[3] * p).sum()).backward()
        runs.append([xg.grad, vg.grad, dyn.alpha.grad] + [t.grad for t in dyn.variables[1:]])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # direct: autograd adds the gradients of the two calls, whose cotangents are (c0, c1, c2, -) and (-, -, -, c3)
    xt, vt = torch.tensor(x, dtype=torch.float32, device=dev), _lib.as_dev(dx[0], dev)
    dirs = torch.ones(B, dtype=torch.int32, device=dev)
    plan = dyn._plan()
    g1, dx1, dv1 = autograd_toy.vjp_grads(dyn, plan, xt, vt, dirs, (c[0], c[1], c[2], None))
    g2, dx2, dv2 = autograd_toy.vjp_grads(dyn, plan, xt, vt, dirs, (None, None, None, c[3]))
    xg_grad, vg_grad, a_grad, *wgrads = runs[0]
    assert torch.equal(xg_grad, dx1 + dx2) and torch.equal(vg_grad, dv1 + dv2)
    u1, u2 = autograd_toy.unpack(dyn, g1), autograd_toy.unpack(dyn, g2)
    names = list(dyn.XNet.state_dict()) + list(dyn.VNet.state_dict())
    refs = [(u1[0] if i < len(names) // 2 else u1[1])[n] for i, n in enumerate(names)]
    refs2 = [(u2[0] if i < len(names) // 2 else u2[1])[n] for i, n in enumerate(names)]
    for n, w, r1, r2 in zip(names, wgrads, refs, refs2):
        assert torch.equal(w, r1 + r2), n
    e = float(plan.eps)
    assert torch.equal(a_grad, (u1[2] * e).cpu().reshape(()) + (u2[2] * e).cpu().reshape(()))


def test_torch_optim_loop():
    """About 30 Adam steps at cfg-2 shape: the loss falls, and after every step the no-grad sampler runs the moved
    weights (equal, bit for bit, to a fresh object loaded with them)."""
    import l2hmc_amd as la
    dyn, _, tm, x, z, dx, dz = _setup("mog", 50, 10, 0.1, 512, "init")
    _requires_grad(dyn)
    opt = torch.optim.Adam(dyn.trainable_variables, lr=1e-3)
    xin = torch.as_tensor(x[:64], dtype=torch.float32, device=dyn._device)
    kw = dict(init_v=dx[0][:64], init_v_backward=dx[1][:64], dir_bits=dx[2][:64], u=dx[3][:64], do_mh_step=True)
    losses = []
    for step in range(30):
        opt.zero_grad()
        loss, _ = _mog_loss(dyn, x, z, dx, dz)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if step % 10 == 9:
            fresh = _fresh(dyn, tm)
            fresh.alpha = dyn.alpha.detach().clone()
            fresh.XNet.load_state({k: v.detach().clone() for k, v in dyn.XNet.state_dict().items()})
            fresh.VNet.load_state({k: v.detach().clone() for k, v in dyn.VNet.state_dict().items()})
            with torch.no_grad():
                got = la.propose(xin, dyn, **kw)
            want = la.propose(xin, fresh, **kw)
            for g, w in ((got[0], want[0]), (got[2], want[2]), (got[3][0], want[3][0])):
                assert torch.equal(g, w)
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert float(dyn.eps.detach()) != pytest.approx(0.1, abs=1e-7)
    w0 = tm.xnet["linear_1/W"].detach().numpy().astype(np.float32)
    assert not np.array_equal(dyn.XNet.linear_1.kernel.detach().cpu().numpy(), w0)
    # an in-place change between forward and backward
    loss, _ = _mog_loss(dyn, x, z, dx, dz)
    with torch.no_grad():
        dyn.VNet.linear_1.kernel.mul_(1.0)
    with pytest.raises(RuntimeError):
        loss.backward()
    # a second backward through the same graph
    loss, _ = _mog_loss(dyn, x, z, dx, dz)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="backward ran twice"):
        loss.backward()
