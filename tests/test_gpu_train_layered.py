"""DynamicsTrainer on a layer-by-layer Dynamics (any x_dim, num_nodes or energy; l2hmc_amd/layered_train.py):
loss and gradients against float64 autograd of the reference graph (oracle.torch_ref), against the one-launch
trainer on a shape both paths take, the new C-ABI entries one by one at ragged shapes, the split-k regime, and a
short training run.

Bars: TOL_G = 2e-4 of each tensor's largest entry (test_gpu_train.py).  Layered vs one-launch trainer (MoG, 50
hidden units, "mild"): 2e-5 of each tensor's max.  At 4096 + 4096 chains the gated gradients carry fp32 relu-flip
noise, so that case uses each tensor's relative Frobenius error, also against 2e-4."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu
TOL_G = 2e-4


def _mlp_packed_ref(net):
    g = {k: v.grad.numpy() for k, v in net.items()}
    return {
        "w1_t": np.concatenate([g['embed_1/W'], g['embed_2/W']], axis=0).T, "wt": g['embed_3/W'], "b1": g['embed_1/b'],
        "wh_t": g['linear_1/W'].T, "bh": g['linear_1/b'],
        "whd_t": np.stack([g['linear_s/W'].T, g['linear_t/W'].T, g['linear_f/W'].T]),
        "bhd": np.stack([g['linear_s/b'], g['linear_t/b'], g['linear_f/b']]),
        "coeff_s": g['scale_s'].reshape(-1), "coeff_q": g['scale_f'].reshape(-1),
    }


def _quartic_model():
    from oracle.torch_ref import TorchDynamicsModel

    class QuarticModel(TorchDynamicsModel):
        """E(x) = sum_d (x_d^2 - 1)^2 / 4 + 0.3 sum_d x_d x_{d+1} (periodic), float64."""

        def __init__(self, *a, **k):
            super().__init__(_DummyGaussian(), *a, **k)

        def _energy(self, x, beta):
            return (((x * x - 1.) ** 2).sum(1) / 4. + 0.3 * (x * torch.roll(x, -1, dims=1)).sum(1)) / self.temperature

        def _force(self, x, beta):
            return ((x * x - 1.) * x + 0.3 * (torch.roll(x, -1, dims=1) + torch.roll(x, 1, dims=1))) / self.temperature

    return QuarticModel


class _DummyGaussian:
    mu = np.zeros(1)
    i_sigma = np.eye(1)


def _quartic_fn(x):
    return ((x * x - 1.) ** 2).sum(dim=1) / 4. + 0.3 * (x * torch.roll(x, -1, dims=1)).sum(dim=1)


def _target(kind, la):
    """-> (x_dim, energy function for Dynamics, float64 model class factory, sampler of start states)."""
    from oracle import dynamics as od
    from oracle.torch_ref import TorchDynamicsModel
    if kind == "mog":
        o = H.mog_target_oracle()
        t = la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])
        return 2, t.get_energy_function(), lambda *a, **k: TorchDynamicsModel(o, *a, **k), o.get_samples
    if kind == "mog3":
        mus = [np.array([1., 0., 0.5]), np.array([0., 1., -0.5]), np.array([-1., -1., 0.])]
        covs = [np.diag([0.05, 0.08, 0.1]), 0.07 * np.eye(3) + 0.02, np.diag([0.1, 0.05, 0.06])]
        pis = [0.3, 0.5, 0.2]
        o, t = od.GMM(mus, covs, pis), la.GMM(mus, covs, pis)
        return 3, t.get_energy_function(), lambda *a, **k: TorchDynamicsModel(o, *a, **k), o.get_samples
    if kind == "gmm12":
        rng = np.random.default_rng(12)
        mus = [rng.normal(0, 1.0, 12) for _ in range(3)]
        sig = [np.diag(rng.uniform(0.3, 0.8, 12)) for _ in range(3)]
        pis = [0.5, 0.3, 0.2]
        o = od.GMM(mus, sig, pis)
        mu_t = torch.tensor(np.stack([m.astype(np.float32) for m in mus]), dtype=torch.float32, device="cuda")
        prec_t = torch.tensor(np.stack(o.i_sigmas), dtype=torch.float32, device="cuda")
        lc_t = torch.tensor(np.log(np.asarray(o.constants)), dtype=torch.float32, device="cuda")

        def fn(x):
            d = x[:, None, :] - mu_t[None]
            q = -0.5 * torch.einsum("bkd,kde,bke->bk", d, prec_t, d) + lc_t[None]
            return -torch.logsumexp(q, dim=1)
        return 12, fn, lambda *a, **k: TorchDynamicsModel(o, *a, **k), o.get_samples
    if kind == "icg50":
        var = np.logspace(-2, 2, 50)
        o = od.Gaussian(np.zeros(50), np.diag(var))
        prec = torch.tensor(np.diag(o.i_sigma).astype(np.float32), device="cuda")

        def fn(x):
            return 0.5 * (x * x * prec).sum(dim=1)
        return 50, fn, lambda *a, **k: TorchDynamicsModel(o, *a, **k), o.get_samples
    if kind == "quartic20":
        def samples(n, rng):
            return rng.normal(0, 0.8, (n, 20))
        return 20, _quartic_fn, _quartic_model(), samples
    raise ValueError(kind)


def _setup(kind, nodes, N, eps, B, regime, seed=11, force_layered=False):
    import l2hmc_amd as la
    from l2hmc_amd.dynamics_trainer import DynamicsTrainer
    from oracle import dynamics as od
    dim, fn, model, samples = _target(kind, la)
    xp, vp = H.mlp_weights(dim, nodes, regime=regime)
    masks = od.make_masks(N, dim, np.random.RandomState(3))
    dyn = la.Dynamics(dim, fn, trajectory_length=N, eps=eps,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes))
    dyn.set_masks(masks)
    dyn.XNet.load_state(xp)
    dyn.VNet.load_state(vp)
    if force_layered:
        dyn.layered = True
    tr = DynamicsTrainer(dyn, scale=0.1)
    rng = np.random.default_rng(seed)
    x = samples(B, rng)
    z = rng.standard_normal((B, dim))
    mk = lambda: (rng.standard_normal((B, dim)), rng.standard_normal((B, dim)),   # noqa: E731
                  rng.integers(0, 2, B).astype(np.float64), rng.uniform(size=B))
    return tr, (lambda: model(N, eps, masks, xp, vp)), x, z, mk(), mk()


def _oracle_loss(make_model, x, z, dx, dz):
    tm = make_model()
    tt = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))   # noqa: E731
    want, Lx, wpx, Lz, wpz = tm.mog_loss(tt(x), tt(z), tuple(map(tt, dx)), tuple(map(tt, dz)), 0.1)
    want.backward()
    return tm, float(want.detach()), np.concatenate([Lx.detach().numpy(), Lz.detach().numpy()]), \
        np.concatenate([wpx.detach().numpy(), wpz.detach().numpy()])


def _grad_errors(tr, tm, norm="max"):
    gv = tr.grad_views()
    worst = {}
    for name, net in (("xnet", tm.xnet), ("vnet", tm.vnet)):
        for k, w in _mlp_packed_ref(net).items():
            got = gv[name][k].cpu().numpy().astype(np.float64).reshape(w.shape)
            if norm == "max":
                worst[f"{name}.{k}"] = float(np.abs(got - w).max() / np.abs(w).max())
            else:
                worst[f"{name}.{k}"] = float(np.linalg.norm(got - w) / np.linalg.norm(w))
    worst["alpha"] = abs(float(gv["alpha"][0]) - float(tm.alpha.grad)) / abs(float(tm.alpha.grad))
    return worst


@pytest.mark.parametrize("kind,nodes,N,eps,B,regime", [
    ("mog", 100, 5, 0.1, 37, "mild"),            # packed target beyond 64 hidden units: l2hmc_mog_energy_hvp runs
    ("mog3", 70, 4, 0.1, 19, "stress"),          # packed, x_dim 3, 70 hidden units (ragged widths)
    ("gmm12", 100, 3, 0.1, 24, "stress"),        # torch callable: double-backward Hessian-vector products
    ("icg50", 100, 5, 0.05, 16, "mild"),         # the paper's 50-d ill-conditioned Gaussian, as a callable
    ("quartic20", 100, 10, 0.05, 9, "mild"),     # float64 subclass of TorchDynamicsModel with a quartic energy
])
def test_layered_loss_gradients_match_autograd(kind, nodes, N, eps, B, regime):
    tr, make_model, x, z, dx, dz = _setup(kind, nodes, N, eps, B, regime)
    assert tr.dynamics.layered
    loss, x_out, px = tr.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
    tm, want, Lw, pw = _oracle_loss(make_model, x, z, dx, dz)
    assert H.relerr(tr.last_proposals.cpu().numpy(), Lw) < 2e-5
    assert np.abs(tr.last_p.cpu().numpy() - pw).max() < 2e-5
    assert pw.mean() > 0.01, "the case must accept"
    assert abs(float(loss) - want) <= 2e-4 * max(1., abs(want))
    worst = _grad_errors(tr, tm)
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, f"gradient mismatch: {bad}\nall: {worst}"
    acc = (tr.last_p[:B].cpu().numpy() - dx[3]) >= 0
    np.testing.assert_array_equal(x_out.cpu().numpy()[acc], tr.last_proposals[:B].cpu().numpy()[acc])
    np.testing.assert_array_equal(x_out.cpu().numpy()[~acc], x[~acc].astype(np.float32))


def test_layered_proposals_are_the_sampling_path_bits():
    """The taped forward runs Dynamics.forward / .backward's kernels: the proposals and p are the same bits."""
    tr, _, x, z, dx, dz = _setup("icg50", 100, 4, 0.05, 33, "mild")
    tr.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
    dyn = tr.dynamics
    bits = dx[2] > 0.5
    Xf, _, pf = dyn.forward(x, init_v=dx[0])
    Xb, _, pb = dyn.backward(x, init_v=dx[1])
    want = torch.where(torch.tensor(bits, device="cuda")[:, None], Xf, Xb)
    wp = torch.where(torch.tensor(bits, device="cuda"), pf, pb)
    assert torch.equal(tr.last_proposals[:len(x)], want)
    assert torch.equal(tr.last_p[:len(x)], wp)


def test_layered_trainer_matches_the_one_launch_trainer():
    """MoG 2-D, 50 hidden units, "mild": the same draws through the one-launch trainer (l2hmc_small_train_step) and
    the forced layered path.  Bar 2e-5 of each tensor's max."""
    B = 64
    tr1, _, x, z, dx, dz = _setup("mog", 50, 6, 0.1, B, "mild")
    tr2, _, _, _, _, _ = _setup("mog", 50, 6, 0.1, B, "mild", force_layered=True)
    assert not tr1.dynamics.layered and tr2.dynamics.layered
    l1, xo1, p1 = tr1.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
    l2, xo2, p2 = tr2.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))   # noqa: E731
    errs = {"loss": abs(float(l1) - float(l2)) / abs(float(l1)), "x_out": rel(xo2, xo1), "px": rel(p2, p1)}
    g1, g2 = tr1.grad_views(), tr2.grad_views()
    for net in ("xnet", "vnet"):
        for k in g1[net]:
            errs[f"{net}.{k}"] = rel(g2[net][k], g1[net][k])
    errs["alpha"] = rel(g2["alpha"], g1["alpha"])
    bad = {k: v for k, v in errs.items() if not v <= 2e-5}
    assert not bad, f"{bad}\nall: {errs}"


def _tn_splits(M, N, R):
    """Mirror of layered_train.hip tn_plan: -> number of split-k partials."""
    mt, nt = -(-M // 64), -(-N // 64)
    s = min(max(1, 512 // (mt * nt)), max(1, -(-R // 256)))
    chunk = -(-(-(-R // s)) // 16) * 16
    return -(-R // chunk)


def _colsum_chunks(R):
    return min(512, max(1, R // 128))


def test_split_k_regime_matches_float64_and_is_reproducible():
    """x_dim 50, 4096 + 4096 chains, 10 leapfrog steps: 163840 taped rows per network, so every weight-gradient
    product runs split-k and the column sums run in 512 chunks."""
    B, N, H_ = 4096, 10, 100
    R = 2 * N * 2 * B
    assert _tn_splits(H_, 2 * 50, R) > 1 and _tn_splits(H_, H_, R) > 1 and _tn_splits(150, H_, R) > 1
    assert _colsum_chunks(R) == 512
    tr, make_model, x, z, dx, dz = _setup("icg50", H_, N, 0.02, B, "mild")
    loss, _, _ = tr.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
    g_first = tr.grads.clone()
    loss2, _, _ = tr.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
    assert torch.equal(g_first, tr.grads) and float(loss) == float(loss2)
    tm, want, _, _ = _oracle_loss(make_model, x, z, dx, dz)
    assert abs(float(loss) - want) <= 2e-4 * max(1., abs(want))
    worst = _grad_errors(tr, tm, norm="fro")
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, f"gradient mismatch: {bad}\nall: {worst}"


def test_short_training_run_on_the_50d_icg():
    from oracle import dynamics as od
    B, N = 512, 10
    tr, _, x, z, dx, dz = _setup("icg50", 100, N, 0.05, B, "init", seed=5)
    tr.lr_init = 1e-3
    dyn = tr.dynamics
    flat0 = [n.flat_params()[0].clone() for n in tr._nets]
    xs = torch.tensor(x, dtype=torch.float32, device="cuda")
    losses = []
    for _ in range(100):
        loss, xs, _ = tr.train_step(xs)
        losses.append(float(loss))
        assert torch.isfinite(tr.grads).all()
    losses = np.array(losses)
    assert np.isfinite(losses).all()
    assert losses[-20:].mean() < losses[:20].mean(), losses
    for n, f0 in zip(tr._nets, flat0):
        assert not torch.equal(n.flat_params()[0], f0)
    tr.sync_weights()
    xp, vp = dyn.XNet.state_dict(), dyn.VNet.state_dict()
    xp = {k: np.asarray(v.cpu() if hasattr(v, "cpu") else v, dtype=np.float64) for k, v in xp.items()}
    vp = {k: np.asarray(v.cpu() if hasattr(v, "cpu") else v, dtype=np.float64) for k, v in vp.items()}
    var = np.logspace(-2, 2, 50)
    orc = od.DynamicsOracle(50, od.Gaussian(np.zeros(50), np.diag(var)), N, float(dyn.eps), dyn.mask.cpu().numpy(),
                            xp, vp)
    rng = np.random.default_rng(9)
    x1 = xs[:64].cpu().numpy().astype(np.float64)
    v1 = rng.standard_normal((64, 50))
    Xf, Vf, pf = dyn.forward(x1, init_v=v1)
    wf = orc.forward(x1, v1)
    assert H.relerr(Xf.cpu().numpy(), wf[0]) < 2e-5 and H.relerr(Vf.cpu().numpy(), wf[1]) < 2e-5
    assert np.abs(pf.cpu().numpy() - wf[2]).max() < 2e-5


# ------------------------------------------------------------------ the new C-ABI entries one by one
def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda").contiguous()


def _relmax(got, want):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else got
    want = want.detach().numpy() if torch.is_tensor(want) else want
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


@pytest.mark.parametrize("D,Hn,rows", [(3, 70, 37), (50, 100, 4100), (72, 288, 1), (50, 288, 37)])
def test_network_entries_match_float64_autograd(D, Hn, rows):
    """l2hmc_stq_dense_taped (bit-equal to l2hmc_stq_dense), l2hmc_dense_backward_data and l2hmc_dense_weight_grads
    (one call's tape) against float64 autograd of utils/network.py's MLP."""
    import ctypes as C
    import l2hmc_amd as la
    from l2hmc_amd import _lib
    from oracle.torch_ref import mlp_net
    L, s = _lib.lib(), _lib.stream_ptr()
    xp, _ = H.mlp_weights(D, Hn, regime="stress", seed=D + Hn)
    net = la.network(D, "XNet", 2.0, num_nodes=Hn)
    net.load_state(xp)
    st = net.pack()
    rng = np.random.default_rng(D * 7 + rows)
    a, b = _dev(rng.standard_normal((rows, D))), _dev(rng.standard_normal((rows, D)))
    tc, ts = float(np.float32(np.cos(0.7))), float(np.float32(np.sin(0.7)))
    S0, T0, Q0 = net([a, b, torch.tensor([[tc, ts]])])
    S, T, Q = (torch.empty(rows, D, device="cuda") for _ in range(3))
    h1, h2 = (torch.empty(rows, Hn, device="cuda") for _ in range(2))
    _lib.check(L.l2hmc_stq_dense_taped(C.byref(st), a.data_ptr(), b.data_ptr(), None, tc, ts, rows, S.data_ptr(),
                                       T.data_ptr(), Q.data_ptr(), h1.data_ptr(), h2.data_ptr(), s))
    assert torch.equal(S, S0) and torch.equal(T, T0) and torch.equal(Q, Q0)
    # float64 reference
    W = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in xp.items()}
    A = torch.tensor(a.cpu().numpy().astype(np.float64), requires_grad=True)
    Bm = torch.tensor(b.cpu().numpy().astype(np.float64), requires_grad=True)
    S64, T64, Q64 = mlp_net(W, [A, Bm, torch.tensor([[tc, ts]], dtype=torch.float64).repeat(rows, 1)])
    assert _relmax(S, S64) < 1e-5 and _relmax(Q, Q64) < 1e-5
    cS, cT, cQ = (rng.standard_normal((rows, D)) for _ in range(3))
    (S64 * torch.tensor(cS) + T64 * torch.tensor(cT) + Q64 * torch.tensor(cQ)).sum().backward()
    dS, dT, dQ = _dev(cS), _dev(cT), _dev(cQ)
    dpre, dsq = torch.empty(rows, 3 * D, device="cuda"), torch.empty(rows, 2 * D, device="cuda")
    dz2, dz1, din = (torch.empty(rows, n, device="cuda") for n in (Hn, Hn, 2 * D))
    ws = torch.empty(L.l2hmc_dense_backward_data_ws_bytes(C.byref(st)), dtype=torch.uint8, device="cuda")
    _lib.check(L.l2hmc_dense_backward_data(C.byref(st), S.data_ptr(), Q.data_ptr(), dS.data_ptr(), dT.data_ptr(),
                                           dQ.data_ptr(), h1.data_ptr(), h2.data_ptr(), rows, dpre.data_ptr(),
                                           dsq.data_ptr(), dz2.data_ptr(), dz1.data_ptr(), din.data_ptr(),
                                           ws.data_ptr(), ws.numel(), s))
    assert _relmax(din[:, :D], A.grad) <= TOL_G and _relmax(din[:, D:], Bm.grad) <= TOL_G
    shapes = dict(w1_t=(Hn, 2 * D), wt=(2, Hn), b1=(Hn,), wh_t=(Hn, Hn), bh=(Hn,), whd_t=(3, D, Hn), bhd=(3, D),
                  coeff_s=(D,), coeff_q=(D,))
    out = {k: torch.full(v, float("nan"), device="cuda") for k, v in shapes.items()}
    g = _lib.DenseGrads(**{k: t.data_ptr() for k, t in out.items()})
    inp = torch.cat([a, b], 1).contiguous()
    tcs = torch.tensor([[tc, ts]], device="cuda").repeat(rows, 1).contiguous()
    wsg = torch.empty(L.l2hmc_dense_weight_grads_ws_bytes(C.byref(st), rows), dtype=torch.uint8, device="cuda")
    args = (C.byref(st), rows, inp.data_ptr(), h1.data_ptr(), h2.data_ptr(), dz1.data_ptr(), dz2.data_ptr(),
            dpre.data_ptr(), dsq.data_ptr(), tcs.data_ptr(), C.byref(g), wsg.data_ptr(), wsg.numel(), s)
    _lib.check(L.l2hmc_dense_weight_grads(*args))
    first = {k: v.clone() for k, v in out.items()}
    _lib.check(L.l2hmc_dense_weight_grads(*args))
    worst = {}
    for k, w in _mlp_packed_ref(W).items():
        assert torch.equal(first[k], out[k]), k            # fixed-order reductions
        worst[k] = _relmax(out[k].reshape(w.shape), w)
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, f"{bad}\nall: {worst}"


def _update_ref(kind, d, eps, st, other, S, T, Q, keep=None):
    """float64 l2hmc_lf_update_v (st = v, other = grad) / _x (st = x, other = v): -> (out, per-row logdet)."""
    eq = torch.exp(eps * Q)
    if kind == "v":
        if not d:
            s_ = 0.5 * eps * S
            return st * torch.exp(s_) - 0.5 * eps * (eq * other - T), s_.sum(1)
        s_ = -0.5 * eps * S
        return torch.exp(s_) * (st + 0.5 * eps * (eq * other - T)), s_.sum(1)
    mi = 1. - keep
    if not d:
        s_ = eps * S
        y = st * torch.exp(s_) + eps * (eq * other + T)
    else:
        s_ = -eps * S
        y = torch.exp(s_) * (st - eps * (eq * other + T))
    return keep * st + mi * y, (mi * s_).sum(1)


@pytest.mark.parametrize("kind", ["v", "x"])
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("D,rows", [(3, 37), (50, 4100), (72, 1)])
def test_sub_update_vjps_match_float64_autograd(kind, d, D, rows):
    from l2hmc_amd import _lib
    L, s = _lib.lib(), _lib.stream_ptr()
    rng = np.random.default_rng(rows + D + 10 * d)
    eps = np.float32(0.13)
    st, other = rng.standard_normal((2, rows, D))
    S, T, Q = 0.5 * rng.standard_normal((3, rows, D))
    keep = (rng.uniform(size=D) < 0.5).astype(np.float64)
    u, dl = rng.standard_normal((rows, D)), rng.standard_normal(rows)
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64), requires_grad=True)   # noqa: E731
    E, ST, OT, S6, T6, Q6 = f64(eps), f64(st), f64(other), f64(S), f64(T), f64(Q)
    out, ld = _update_ref(kind, d, E, ST, OT, S6, T6, Q6, torch.tensor(keep))
    ((out * torch.tensor(u)).sum() + (ld * torch.tensor(dl)).sum()).backward()
    dev = {k: _dev(np.asarray(v, dtype=np.float32)) for k, v in
           dict(st=st, other=other, S=S, T=T, Q=Q, keep=keep, u=u, dl=dl).items()}
    o = {k: torch.empty(rows, D, device="cuda") for k in ("dst", "doth", "dS", "dT", "dQ")}
    de = torch.empty(rows, device="cuda")
    fn = L.l2hmc_lf_update_v_vjp if kind == "v" else L.l2hmc_lf_update_x_vjp
    head = [dev["st"].data_ptr(), dev["other"].data_ptr()] + ([dev["keep"].data_ptr()] if kind == "x" else [])
    _lib.check(fn(*head, dev["S"].data_ptr(), dev["T"].data_ptr(), dev["Q"].data_ptr(), float(eps), d, rows, D,
                  dev["u"].data_ptr(), dev["dl"].data_ptr(), o["dst"].data_ptr(), o["doth"].data_ptr(),
                  o["dS"].data_ptr(), o["dT"].data_ptr(), o["dQ"].data_ptr(), de.data_ptr(), s))
    errs = {"dst": _relmax(o["dst"], ST.grad), "doth": _relmax(o["doth"], OT.grad), "dS": _relmax(o["dS"], S6.grad),
            "dT": _relmax(o["dT"], T6.grad), "dQ": _relmax(o["dQ"], Q6.grad),
            "deps": abs(float(de.double().sum()) - float(E.grad)) / abs(float(E.grad))}
    bad = {k: v for k, v in errs.items() if not v <= 2e-5}
    assert not bad, f"{bad}\nall: {errs}"


@pytest.mark.parametrize("kind,rows,temp", [("mog3", 37, 1.0), ("mog", 4100, 1.7), ("scg", 1, 1.0)])
def test_mog_energy_hvp_matches_autograd(kind, rows, temp):
    import ctypes as C
    import l2hmc_amd as la
    from l2hmc_amd import _lib
    from oracle.torch_ref import TorchDynamicsModel
    if kind == "scg":
        o = H.scg_target_oracle()
        t = la.Gaussian(np.zeros(2), np.array([[50.05, -49.95], [-49.95, 50.05]]))
        dim = 2
    else:
        dim, _, _, _ = _target(kind, la)
        from oracle import dynamics as od
        if kind == "mog":
            o, t = H.mog_target_oracle(), la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2,
                                                 [0.5, 0.5])
        else:
            mus = [np.array([1., 0., 0.5]), np.array([0., 1., -0.5]), np.array([-1., -1., 0.])]
            covs = [np.diag([0.05, 0.08, 0.1]), 0.07 * np.eye(3) + 0.02, np.diag([0.1, 0.05, 0.06])]
            o, t = od.GMM(mus, covs, [0.3, 0.5, 0.2]), la.GMM(mus, covs, [0.3, 0.5, 0.2])
    tm = TorchDynamicsModel(o, 1, 0.1, np.zeros((1, dim)), {}, {}, temperature=temp)
    rng = np.random.default_rng(rows)
    x = rng.normal(0.3, 0.4, (rows, dim)).astype(np.float32)
    u = rng.standard_normal((rows, dim)).astype(np.float32)
    X = torch.tensor(x.astype(np.float64), requires_grad=True)
    (g,) = torch.autograd.grad(tm._energy(X, None).sum(), X, create_graph=True)
    (want,) = torch.autograd.grad(g, X, grad_outputs=torch.tensor(u.astype(np.float64)))
    out = torch.empty(rows, dim, device="cuda")
    tgt = t.get_energy_function().target          # held: struct() points into its device buffers
    st = tgt.struct(temp)
    xd, ud = _dev(x), _dev(u)
    _lib.check(_lib.lib().l2hmc_mog_energy_hvp(C.byref(st), xd.data_ptr(), ud.data_ptr(), rows, out.data_ptr(),
                                               _lib.stream_ptr()))
    assert _relmax(out, want) < 2e-5
