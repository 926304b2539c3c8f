"""torch.autograd through GaugeDynamics transitions (l2hmc_amd/autograd.py): a loss written in torch around
`dyn(x, beta)` -- here the reference's own _calc_loss (gauge_model.py:728-797) and arbitrary linear functionals
of all four outputs -- differentiated through the HIP training entries, against float64 autograd on the torch
restatement (oracle/torch_ref.py), against GaugeTrainer, and against direct calls of the C ABI.

Tolerances as tests/test_gpu_train.py: gradients per tensor in the max norm relative to the tensor's largest
entry at TOL_G = 2e-4."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.torch_ref import TorchGaugeModel, action
from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL_G = 2e-4
TWO_PI = 2 * np.pi


def _plaq(a, T, X):
    s = a.reshape(a.shape[0], T, X, 2)
    return s[..., 0] - s[..., 1] - torch.roll(s[..., 0], -1, 2) + torch.roll(s[..., 1], -1, 1)


def _calc_loss(x, x_prop, px, z, pz, T, X, metric='cos_diff', loss_scale=1., aux_weight=1., std_weight=1.,
               charge_weight=1.):
    """gauge_model.py:728-797 written in plain torch on the outputs of two transitions."""
    eps = 1e-3
    m = {'l1': lambda a, b: torch.abs(a - b), 'l2': lambda a, b: (a - b) ** 2,
         'cos': lambda a, b: torch.abs(torch.cos(a) - torch.cos(b)),
         'cos2': lambda a, b: (torch.cos(a) - torch.cos(b)) ** 2,
         'cos_diff': lambda a, b: 1. - torch.cos(a - b)}[metric]

    def charge(a):
        P = _plaq(a, T, X)
        q = sum((-2. / n) * (-1.) ** n * torch.sin(n * P) for n in range(1, 5))
        return q.sum(dim=(1, 2)) / TWO_PI

    x_std = m(x, x_prop).sum(1) * px + eps
    z_std = aux_weight * (m(z, x_prop).sum(1) * pz + eps)
    std_loss = std_weight * (loss_scale * (1. / x_std + 1. / z_std) - (x_std + z_std) / loss_scale)
    qp = charge(x_prop)
    xq = px * torch.abs(charge(x) - qp) + eps
    zq = aux_weight * (pz * torch.abs(charge(z) - qp) + eps)
    return (std_loss + charge_weight * (xq + zq)).mean()


def _setup(T, X, N, eps, B, regime, arch='generic', seed=7):
    xp, vp = H.gauge_weights(T, X, regime=regime) if arch == 'generic' else H.conv_weights(T, X, regime=regime)
    orc = H.gauge_oracle(T, X, N, eps, xp, vp, arch=arch)
    dyn = H.gauge_hip(T, X, N, eps, xp, vp, orc.mask, B, arch=arch)
    tm = TorchGaugeModel(T, X, N, eps, orc.mask, xp, vp, arch=arch)
    D = 2 * T * X
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 2 * np.pi, (B, D))
    z = rng.standard_normal((B, D))
    dx = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    dz = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    return dyn, tm, orc, x, z, dx, dz


def _draw_kw(d):
    return dict(momentum_f=d[0], momentum_b=d[1], coin=d[2], u=d[3])


def _requires_grad(dyn):
    for v in dyn.variables:
        v.requires_grad_()
        v.grad = None


def _autograd_loss(dyn, x, z, dx, dz, beta):
    T, X = dyn.lattice.time_size, dyn.lattice.space_size
    x = dyn._x(x)
    z = dyn._x(z)
    x_prop, _, px, _ = dyn(x, beta, **_draw_kw(dx))
    _, _, pz, _ = dyn(z, beta, **_draw_kw(dz))
    return _calc_loss(x, x_prop, px, z, pz, T, X)


def _t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _rel(got, want):
    got = got.detach().cpu().double().reshape(want.shape)
    scale = float(want.abs().max())
    assert scale > 0
    return float((got - want).abs().max()) / scale


def _compare_to_oracle(dyn, tm, tol=TOL_G):
    worst = {}
    for name, net, ref in (("xnet", dyn.position_fn, tm.xnet), ("vnet", dyn.momentum_fn, tm.vnet)):
        for k, t in net.state_dict().items():
            assert t.grad is not None, (name, k)
            worst[f"{name}.{k}"] = _rel(t.grad, ref[k].grad.detach())
    worst["eps"] = _rel(dyn.eps.grad, tm.eps.grad.detach())
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, f"gradient mismatch: {bad}\nall: {worst}"
    return worst


@pytest.mark.parametrize("T,X,N,eps,B,regime,arch,fused", [
    (8, 8, 2, 0.1, 16, "mild", "generic", True),     # benchmark widths D=128, H=512: whole-trajectory kernels
    (4, 4, 2, 0.15, 37, "stress", "generic", True),  # ragged batch, strong S/Q
    (8, 8, 2, 0.1, 16, "mild", "generic", False),    # layered kernels
    (8, 8, 2, 0.1, 9, "mild", "conv3D", True),       # ConvNet3D front-end
    (4, 16, 2, 0.1, 11, "mild", "generic", True),    # non-square lattice
])
def test_reference_loss_through_autograd_matches_float64(T, X, N, eps, B, regime, arch, fused):
    dyn, tm, _, x, z, dx, dz = _setup(T, X, N, eps, B, regime, arch)
    dyn.fused = fused
    _requires_grad(dyn)
    beta = 2.5
    loss = _autograd_loss(dyn, x, z, dx, dz, beta)
    assert loss.grad_fn is not None
    loss.backward()
    want, _ = tm.loss(_t64(x), _t64(z), beta, tuple(map(_t64, dx)), tuple(map(_t64, dz)))
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 2e-4 * max(1., abs(float(want.detach())))
    _compare_to_oracle(dyn, tm)


def test_autograd_matches_gauge_trainer():
    """Same weights, same draws: GaugeTrainer's training step and the autograd path.  Measured on MI355X: equal
    losses, gradients within 4.8e-7 of each tensor's scale.  The bars (loss 1e-5 relative, gradients TOL_G) are
    looser than that because the trainer integrates x and z stacked in one call and autograd in two."""
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    T = X = 8
    dyn_t, _, orc, x, z, dx, dz = _setup(T, X, 2, 0.1, 16, "mild")
    dyn_a = H.gauge_hip(T, X, 2, 0.1, *H.gauge_weights(T, X, regime="mild"), orc.mask, 16)
    dyn_a.position_fn.load_state({k: v.detach().clone() for k, v in dyn_t.position_fn.state_dict().items()})
    dyn_a.momentum_fn.load_state({k: v.detach().clone() for k, v in dyn_t.momentum_fn.state_dict().items()})
    tr = GaugeTrainer(dyn_t)
    loss_t, *_ = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    _requires_grad(dyn_a)
    loss_a = _autograd_loss(dyn_a, x, z, dx, dz, 2.5)
    loss_a.backward()
    assert abs(float(loss_a.detach()) - float(loss_t)) <= 1e-5 * abs(float(loss_t))
    gv = tr.grad_views()
    worst = {}
    for name, net in (("xnet", dyn_a.position_fn), ("vnet", dyn_a.momentum_fn)):
        ref = net.unpack_grads(gv[name])
        for k, t in net.state_dict().items():
            worst[f"{name}.{k}"] = _rel(t.grad, ref[k].detach().cpu().double())
    worst["eps"] = _rel(dyn_a.eps.grad, gv["eps"].detach().cpu().double().reshape(()))
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, bad


def test_every_output_and_the_input_match_float64():
    """loss = sum c1 x_prop + c2 v_prop + c3 p + c4 x_out with x.requires_grad_(): the weights' and the start
    state's gradients (through the trajectory AND through H(x0) and the select) against float64 autograd."""
    T = X = 8
    N, eps, B, beta = 3, 0.1, 96, 2.0          # smoke()'s regime: accepted and rejected chains
    dyn, tm, _, _, _, dx, _ = _setup(T, X, N, eps, B, "mild")
    D = 2 * T * X
    rng = np.random.default_rng(11)
    x = rng.normal(0, 0.3, (B, D))
    c = [rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.standard_normal(B), rng.standard_normal((B, D))]
    with torch.no_grad():                      # MH uniforms kept off p, where fp32 and fp64 could select apart
        p = tm.apply_transition(_t64(x), beta, *map(_t64, dx))[2].numpy()
    dx = (*dx[:3], np.where(np.abs(p - dx[3]) < 1e-3, 0.5 * p, dx[3]))
    _requires_grad(dyn)
    xg = torch.tensor(x, dtype=torch.float32, device=dyn._device, requires_grad=True)
    outs = dyn(xg, beta, **_draw_kw(dx))
    cg = [torch.tensor(a, dtype=torch.float32, device=dyn._device) for a in c]
    sum((ci * o).sum() for ci, o in zip(cg, outs)).backward()
    x64 = _t64(x).requires_grad_()
    want = tm.apply_transition(x64, beta, *map(_t64, dx))
    sum((_t64(ci) * o).sum() for ci, o in zip(c, want)).backward()
    p, u = want[2].detach().numpy(), dx[3]
    acc = p > u
    assert 0 < acc.sum() < B and (p < 1).any() and (p == 1).any(), (acc.sum(), p)
    worst = _compare_to_oracle(dyn, tm)
    worst["x"] = _rel(xg.grad, x64.grad)
    assert worst["x"] <= TOL_G, worst


def _accept_vjp_ref(x0, v0, xN, vN, sld, u, g, beta, T, X):
    """float64 autograd of p = exp(min(H0 - H1 + sld, 0)), x_out = where(p > u, xN, x0)."""
    x0, v0, xN, vN, sld = (_t64(a).requires_grad_() for a in (x0, v0, xN, vN, sld))
    h0 = beta * action(x0, T, X) + 0.5 * (v0 ** 2).sum(1)
    h1 = beta * action(xN, T, X) + 0.5 * (vN ** 2).sum(1)
    p = torch.exp(torch.minimum(h0 - h1 + sld, torch.zeros((), dtype=torch.float64)))
    a = (p > _t64(u)).to(torch.float64)[:, None]
    x_out = a * xN + (1. - a) * x0
    gx, gv, gp, go = map(_t64, g)
    ((gx * xN).sum() + (gv * vN).sum() + (gp * p).sum() + (go * x_out).sum()).backward()
    return p.detach().numpy(), xN.grad.numpy(), vN.grad.numpy(), sld.grad.numpy(), x0.grad.numpy(), v0.grad.numpy()


def test_accept_backward_kernel_matches_float64():
    from l2hmc_amd import _lib
    T, X, R, beta = 3, 5, 131, 1.7             # odd lattice, rows not a multiple of 64
    D = 2 * T * X
    rng = np.random.default_rng(5)
    x0, xN = rng.uniform(0, 2 * np.pi, (R, D)), rng.uniform(0, 2 * np.pi, (R, D))
    v0, vN = rng.standard_normal((R, D)), rng.standard_normal((R, D))
    h = lambda x, v: (beta * action(_t64(x), T, X) + 0.5 * (_t64(v) ** 2).sum(1)).numpy()  # noqa: E731
    sld = h(xN, vN) - h(x0, v0) + rng.standard_normal(R)      # A ~ N(0, 1): p = 1 and 0 < p < 1
    g = [rng.standard_normal((R, D)), rng.standard_normal((R, D)), rng.standard_normal(R), rng.standard_normal((R, D))]
    p0 = np.exp(np.minimum(h(x0, v0) - h(xN, vN) + sld, 0))
    u = np.where(rng.uniform(size=R) < 0.5, p0 * 0.5, np.minimum(p0 + 0.25, 1.5))   # accept / reject, far from p
    p, dxN, dvN, dld, dx0, dv0 = _accept_vjp_ref(x0, v0, xN, vN, sld, u, g, beta, T, X)
    bad = np.arange(R) % 7 == 3                # non-finite proposals: p = 0
    xN_in = xN.copy()
    xN_in[bad, 0], xN_in[bad, 1] = np.nan, np.inf
    p_in = np.where(bad, 0., p)
    dxN[bad] = g[0][bad]
    dvN[bad] = g[1][bad]
    dld[bad] = 0.
    dx0[bad] = g[3][bad]
    dv0[bad] = 0.
    assert ((p < 1) & ~bad).sum() > 20 and ((p == 1) & ~bad).sum() > 20
    dev = torch.device("cuda", torch.cuda.current_device())
    f = lambda a: _lib.as_dev(a, dev)          # noqa: E731
    ins = [f(a) for a in (x0, v0, xN_in, vN, p_in, u)]
    gs = [f(a) for a in g]
    outs = [torch.full((R, D), 7.), torch.full((R, D), 7.), torch.full((R,), 7.), torch.full((R, D), 7.),
            torch.full((R, D), 7.)]
    outs = [o.to(dev) for o in outs]
    L = _lib.lib()
    _lib.check(L.l2hmc_gauge_accept_backward(T, X, beta, R, *[t.data_ptr() for t in ins + gs + outs],
                                             _lib.stream_ptr()))
    got = [o.cpu().numpy() for o in outs]
    for name, a, b in zip(("dxN", "dvN", "dlogdet", "dx0", "dv0"), got, (dxN, dvN, dld, dx0, dv0)):
        assert np.isfinite(a).all(), name
        assert H.relerr(a, b) <= 1e-5, (name, H.relerr(a, b))
    assert (got[2][bad] == 0).all() and (got[2][p == 1] == 0).all()


def test_plumbing_is_exact():
    """Cotangents on x_prop and v_prop only: the autograd weight gradients are, bit for bit, those of a direct
    l2hmc_gauge_train_forward + l2hmc_gauge_train_backward with the same cotangents and dlogdet = 0."""
    from l2hmc_amd import _lib
    dyn, _, _, x, _, dx, _ = _setup(8, 8, 2, 0.1, 24, "mild")
    B, D = x.shape
    rng = np.random.default_rng(3)
    c1, c2 = (torch.tensor(rng.standard_normal((B, D)), dtype=torch.float32, device=dyn._device) for _ in range(2))
    _requires_grad(dyn)
    xt = dyn._x(x)
    xp, vp, _, _ = dyn(xt, 2.0, **_draw_kw(dx))
    ((c1 * xp).sum() + (c2 * vp).sum()).backward()
    # direct
    dev = dyn._device
    vf, vb, coin = (_lib.as_dev(a, dev) for a in dx[:3])
    fwd = coin > 0.5
    v0 = torch.where(fwd[:, None], dyn._x(vf), dyn._x(vb)).contiguous()
    dirs = (~fwd).to(torch.int32).contiguous()
    plan, L = dyn._plan(), _lib.lib()
    nb = L.l2hmc_gauge_train_ws_bytes(C.byref(plan), B)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    xN, vN = torch.empty_like(xt), torch.empty_like(xt)
    sld, p = torch.empty(B, device=dev), torch.empty(B, device=dev)
    s = _lib.stream_ptr()
    _lib.check(L.l2hmc_gauge_train_forward(C.byref(plan), 2.0, xt.data_ptr(), v0.data_ptr(), dirs.data_ptr(), B,
                                           xN.data_ptr(), vN.data_ptr(), sld.data_ptr(), p.data_ptr(), ws.data_ptr(),
                                           nb, s))
    assert torch.equal(xN, xp) and torch.equal(vN, vp)
    grads = []
    for net in (dyn.position_fn, dyn.momentum_fn):
        bufs = net._packed[1]
        grads.append({k: torch.zeros_like(bufs[k]) for k in net.SEGMENTS})
    structs = [_lib.DenseGrads(**{k: v.data_ptr() for k, v in g.items()}) for g in grads]
    dxN, dvN, dld = c1.clone(), c2.clone(), torch.zeros(B, device=dev)
    deps = torch.zeros(1, device=dev)
    _lib.check(L.l2hmc_gauge_train_backward(C.byref(plan), 2.0, dirs.data_ptr(), B, dxN.data_ptr(), dvN.data_ptr(),
                                            dld.data_ptr(), C.byref(structs[0]), C.byref(structs[1]), None, None,
                                            deps.data_ptr(), ws.data_ptr(), nb, s))
    for net, g in zip((dyn.position_fn, dyn.momentum_fn), grads):
        ref = net.unpack_grads(g)
        for k, t in net.state_dict().items():
            assert torch.equal(t.grad, ref[k]), k
    assert torch.equal(dyn.eps.grad.reshape(1), deps.cpu())


def test_same_draws_as_the_sampling_path():
    """Without injected draws, grad-enabled and no-grad `dyn(x, beta)` take the same Philox streams."""
    dyn, _, _, x, _, _, _ = _setup(8, 8, 3, 0.1, 48, "mild")
    _requires_grad(dyn)
    x = np.random.default_rng(9).normal(0, 0.3, x.shape)
    dyn._draws = 5
    with torch.no_grad():
        a = dyn(x, 2.0)
    draws_a = dyn._draws
    dyn._draws = 5
    b = dyn(x, 2.0)
    assert b[0].grad_fn is not None and a[0].grad_fn is None
    assert dyn._draws == draws_a
    a = [t.cpu().numpy() for t in a]
    b = [t.detach().cpu().numpy() for t in b]
    for i in range(3):
        assert H.relerr(b[i], a[i]) <= 2e-5, i
    from l2hmc_amd import _lib
    cu = torch.empty(96, device=dyn._device)
    d, _ = _lib.step_draw_index(5)
    _lib.check(_lib.lib().l2hmc_fill_uniform(cu.data_ptr(), 96, dyn._seed, 2 * d + 1, _lib.stream_ptr()))
    u = cu.cpu().numpy()[48:]
    safe = np.abs(a[2] - u) > 1e-4
    assert safe.sum() > 40
    assert H.relerr(b[3][safe], a[3][safe]) <= 2e-5


def test_torch_optim_loop():
    import l2hmc_amd as la
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    T = X = 8
    N, eps, B, beta = 2, 0.15, 32, 2.0
    dyn, _, orc, x, z, dx, dz = _setup(T, X, N, eps, B, "init")
    _requires_grad(dyn)
    opt = torch.optim.Adam(dyn.trainable_variables, lr=1e-4)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = _autograd_loss(dyn, x, z, dx, dz, beta)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    # the sampler runs the moved weights: equal, bit for bit, to a fresh object loaded with them
    fresh = H.gauge_hip(T, X, N, float(dyn.eps.detach()), *H.gauge_weights(T, X, regime="init"), orc.mask, B)
    fresh.position_fn.load_state({k: v.detach().clone() for k, v in dyn.position_fn.state_dict().items()})
    fresh.momentum_fn.load_state({k: v.detach().clone() for k, v in dyn.momentum_fn.state_dict().items()})
    xin, v0f, v0b, coin, u = H.gauge_inputs(B, 2 * T * X)
    with torch.no_grad():
        got = dyn(xin, beta, momentum_f=v0f, momentum_b=v0b, coin=coin, u=u)
    want = fresh(xin, beta, momentum_f=v0f, momentum_b=v0b, coin=coin, u=u)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    w0 = H.gauge_weights(T, X, regime="init")[0]["h_layer/W"]
    assert not np.array_equal(dyn.position_fn.h_layer.kernel.detach().cpu().numpy(), np.float32(w0))
    # an in-place change between forward and backward
    loss = _autograd_loss(dyn, x, z, dx, dz, beta)
    with torch.no_grad():
        dyn.momentum_fn.h_layer.kernel.mul_(1.0)
    with pytest.raises(RuntimeError):
        loss.backward()
    # a second backward through the same graph
    loss = _autograd_loss(dyn, x, z, dx, dz, beta)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="backward ran twice"):
        loss.backward()
    loss = _autograd_loss(dyn, x, z, dx, dz, beta)
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    # refused before any launch (no draw is consumed)
    xg = torch.zeros(B, 2 * T * X, device=dyn._device, requires_grad=True)
    hmc = H.gauge_hip(T, X, N, eps, None, None, orc.mask, B, hmc=True)
    with pytest.raises(NotImplementedError, match="hmc"):
        hmc(xg, beta)
    assert hmc._draws == 0
    lat = la.GaugeLattice(6, 6, 2, 'U1', num_samples=4, rand=False)
    small = la.GaugeDynamics(lat, lat.get_energy_function(), eps=0.1, num_steps=2)
    with pytest.raises(ValueError, match="multiples of 32"):
        small(torch.zeros(4, 72, device=dyn._device, requires_grad=True), beta)
    assert small._draws == 0
    owned = H.gauge_hip(T, X, N, eps, *H.gauge_weights(T, X, regime="init"), orc.mask, B)
    GaugeTrainer(owned)
    with pytest.raises(ValueError, match="GaugeTrainer"):
        owned(xg, beta)
    assert owned._draws == 0
