"""The rough-well and funnel targets in the one-launch toy kernels (the AN instances of csrc/small_mlp.hip and
csrc/small_train.hip) against float64 references written here: the operators, trajectories and `propose`, the fused path
against the layered one, `DynamicsSampler.run` against the loop, and gradients against float64 autograd.

Inputs are rounded to fp32 before the float64 evaluation.  Tolerances are those of tests/test_gpu_parity.py (TOL_OP,
the three-part check of assert_fp32_equivalent, FORMS_TOL) and of tests/test_gpu_train.py (TOL_G), copied."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import dynamics as ogen
from oracle.torch_ref import TorchDynamicsModel
from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL_OP, TOL_P = 1e-5, 2e-5
MAX_RATIO, RMS_RATIO, P_RATIO = 5.0, 1.6, 3.5
FORMS_TOL = 1e-4
TOL_G = 2e-4
SCALE = 0.1
SIGMA, CLIP = 2.0, 8.0


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def rmserr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2)) / max(1.0, np.max(np.abs(want))))


def assert_fp32_equivalent(got, want64, want32, what):
    emax, imax = H.relerr(got, want64), H.relerr(want32, want64)
    erms, irms = rmserr(got, want64), rmserr(want32, want64)
    print(f"{what}: max {emax:.2e} (fp32 oracle {imax:.2e}), rms {erms:.2e} ({irms:.2e})")
    assert emax < max(TOL_OP, MAX_RATIO * imax), f"{what}: max err {emax:.2e} vs intrinsic fp32 {imax:.2e}"
    assert erms < max(TOL_OP / 3, RMS_RATIO * irms), f"{what}: rms err {erms:.2e} vs intrinsic fp32 {irms:.2e}"


# ------------------------------------------------------------------------------------------- references
class RoughWellRef:
    """distributions.py:101-121 in NumPy, in the dtype of its input (float64, or float32 in the reference's order)."""

    def __init__(self, eps, easy=False):
        self.eps, self.easy = eps, easy

    def _a(self, dt):
        e = dt(self.eps)
        return e if self.easy else e * e

    def energy(self, x):
        dt = x.dtype.type
        return dt(0.5) * np.sum(np.square(x), 1) + dt(self.eps) * np.sum(np.cos(x / self._a(dt)), 1)

    def grad_energy(self, x):
        dt = x.dtype.type
        a = self._a(dt)
        return x - (dt(self.eps) / a) * np.sin(x / a)

    def hvp(self, x, u):
        dt = x.dtype.type
        a = self._a(dt)
        return (dt(1) - (dt(self.eps) / (a * a)) * np.cos(x / a)) * u


class FunnelRef:
    """distributions.py:184-211 in NumPy; gradient and Hessian of the branch tf.where selects."""

    def _s(self, v):
        dt = v.dtype.type
        hi, lo = v > CLIP, -CLIP > v
        s = np.where(hi, np.exp(dt(CLIP)), np.where(lo, np.exp(dt(-CLIP)), np.exp(np.where(hi | lo, 0, v))))
        return s, hi | lo

    def energy(self, x):
        dt = x.dtype.type
        v, n = x[:, 0], dt(x.shape[1] - 1)
        s, _ = self._s(v)
        return dt(0.5) * (np.square(v / dt(SIGMA)) + np.sum(np.square(x[:, 1:]), 1) / s + n * np.log(dt(2 * np.pi) * s))

    def grad_energy(self, x):
        dt = x.dtype.type
        v, n = x[:, 0], dt(x.shape[1] - 1)
        s, cl = self._s(v)
        ss = np.sum(np.square(x[:, 1:]), 1)
        g = np.empty_like(x)
        g[:, 0] = v / dt(SIGMA * SIGMA) + np.where(cl, 0, dt(0.5) * (n - ss / s))
        g[:, 1:] = x[:, 1:] / s[:, None]
        return g

    def hvp(self, x, u):
        dt = x.dtype.type
        v = x[:, 0]
        s, cl = self._s(v)
        ss = np.sum(np.square(x[:, 1:]), 1)
        on = np.where(cl, 0, 1).astype(x.dtype)
        out = np.empty_like(x)
        out[:, 0] = (dt(1 / (SIGMA * SIGMA)) + on * dt(0.5) * ss / s) * u[:, 0] - on * np.sum(x[:, 1:] * u[:, 1:], 1) / s
        out[:, 1:] = u[:, 1:] / s[:, None] - on[:, None] * x[:, 1:] * u[:, :1] / s[:, None]
        return out


class TorchAnalyticModel(TorchDynamicsModel):
    """oracle/torch_ref.py with the energy of a rough well or a funnel in float64 torch; the force is autograd's."""

    def __init__(self, kind, params, *args, **kw):
        super().__init__(ogen.Gaussian(np.zeros(2), np.eye(2)), *args, **kw)
        self.kind, self.params = kind, params

    def _energy(self, x, beta):
        if self.kind == "rw":
            eps, easy = self.params
            a = eps if easy else eps * eps
            e = 0.5 * (x * x).sum(1) + eps * torch.cos(x / a).sum(1)
        else:
            v, n = x[:, 0], x.shape[1] - 1
            hi, lo = v > CLIP, -CLIP > v
            s = torch.where(hi, torch.full_like(v, math.exp(CLIP)),
                            torch.where(lo, torch.full_like(v, math.exp(-CLIP)), torch.exp(torch.where(hi | lo, 0 * v, v))))
            e = 0.5 * ((v / SIGMA) ** 2 + (x[:, 1:] ** 2).sum(1) / s + n * torch.log(2 * math.pi * s))
        return e / self.temperature

    def _force(self, x, beta):
        if not x.requires_grad:
            x = x.detach().requires_grad_()
        with torch.enable_grad():
            (g,) = torch.autograd.grad(self._energy(x, beta).sum(), x, create_graph=True)
        return g


def _eps32(eps):
    return float(np.float32(eps))


def _target(la, kind, dim, eps=0.8, easy=False):
    """-> (l2hmc_amd distribution, NumPy reference, parameters of the torch model).  eps is fp32-representable."""
    if kind == "rw":
        eps = _eps32(eps)
        return la.RoughWell(dim, eps, easy), RoughWellRef(eps, easy), (eps, easy)
    return la.GaussianFunnel(dim), FunnelRef(), None


def _funnel_rows(rng, rows, dim):
    x = rng.normal(0, 1.0, (rows, dim))
    vs = np.array([-9., -8., -7.5, 0., 7.5, 8., 9.])
    x[:, 0] = np.resize(vs, rows) if rows >= vs.size else vs[[3]]
    x[:, 1:] *= np.exp(np.clip(x[:, :1], -CLIP, CLIP) / 2)
    return x


# ------------------------------------------------------------------------------------------- 1. operators
def _operators(la, dist, x, u, temp):
    from l2hmc_amd import _lib
    tgt = dist.get_energy_function().target
    e, g = tgt.energy_grad(x, temp)
    xd, ud = _lib.as_dev(x), _lib.as_dev(u)
    hv = torch.empty_like(xd)
    st = tgt.struct(temp)
    _lib.check(_lib.lib().l2hmc_mog_energy_hvp(C.byref(st), xd.data_ptr(), ud.data_ptr(), xd.shape[0], hv.data_ptr(),
                                               _lib.stream_ptr()))
    e_only = tgt.energy_grad(x, temp, want_grad=False)[0]
    assert torch.equal(e_only, e)
    return np_(e), np_(g), np_(hv)


@pytest.mark.parametrize("temp", [1.0, 2.5])
@pytest.mark.parametrize("rows", [1, 255, 257])
@pytest.mark.parametrize("kind,dim,eps,easy", [("rw", d, e, z) for d in (1, 2, 3, 8) for e, z in ((0.8, False), (0.5, True))]
                         + [("funnel", d, None, None) for d in (2, 3, 8)])
def test_energy_gradient_and_hvp_match_float64(la, kind, dim, eps, easy, rows, temp):
    rng = np.random.default_rng(100 * dim + rows)
    dist, ref, _ = _target(la, kind, dim, eps, easy)
    x = f32(rng.normal(0, 1.5, (rows, dim)) if kind == "rw" else _funnel_rows(rng, rows, dim))
    u = f32(rng.standard_normal((rows, dim)))
    e, g, hv = _operators(la, dist, x, u, temp)
    for name, got, want in (("energy", e, ref.energy(x)), ("grad", g, ref.grad_energy(x)), ("hvp", hv, ref.hvp(x, u))):
        err = H.relerr(got, want / temp)
        print(f"{kind} dim={dim} rows={rows} T={temp} {name}: {err:.2e}")
        assert err < TOL_OP, (name, err)


def test_funnel_rows_hit_every_branch():
    x = _funnel_rows(np.random.default_rng(0), 255, 3)
    v = x[:, 0]
    assert (v > CLIP).any() and (v < -CLIP).any() and (v == CLIP).any() and (v == -CLIP).any() and (np.abs(v) < CLIP).any()
    _, cl = FunnelRef()._s(v)
    assert not cl[np.abs(v) == CLIP].any() and cl[np.abs(v) > CLIP].all()          # v == +-clip is unclipped


@pytest.mark.parametrize("temp", [1.0, 2.5])
@pytest.mark.parametrize("rows", [1, 255, 257])
@pytest.mark.parametrize("dim", [1, 2, 3, 8])
@pytest.mark.parametrize("eps,easy", [(0.01, True), (0.1, False)])
def test_paper_rough_wells_are_as_close_as_fp32_allows(la, eps, easy, dim, rows, temp):
    """The paper's parameters: x / a reaches several hundred, and its fp32 rounding alone moves the gradient by about
    1e-5 of its scale.  Yardstick: the same formulas in NumPy float32, in the reference's operation order."""
    rng = np.random.default_rng(7 * dim + rows)
    dist, ref, _ = _target(la, "rw", dim, eps, easy)
    x = f32(rng.uniform(-3, 3, (rows, dim)))
    u = f32(rng.standard_normal((rows, dim)))
    e, g, hv = _operators(la, dist, x, u, temp)
    x32, u32 = x.astype(np.float32), u.astype(np.float32)
    for name, got, want, w32 in (("energy", e, ref.energy(x), ref.energy(x32)), ("grad", g, ref.grad_energy(x), ref.grad_energy(x32)),
                                 ("hvp", hv, ref.hvp(x, u), ref.hvp(x32, u32))):
        err, intrinsic = H.relerr(got, want / temp), H.relerr(w32.astype(np.float64) / np.float32(temp), want / temp)
        print(f"rough well eps={eps} dim={dim} rows={rows} T={temp} {name}: {err:.2e} (float32 NumPy {intrinsic:.2e})")
        assert err < max(TOL_OP, MAX_RATIO * intrinsic), (name, err, intrinsic)


# ------------------------------------------------------------------------------------------- 2. trajectories, propose
def _dyn(la, fn, dim, nodes, N, masks, xp, vp, eps=0.1, hmc=False, temp=1.0, seed=7):
    dyn = la.Dynamics(dim, fn, trajectory_length=N, eps=eps, hmc=hmc,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes),
                      use_temperature=True, seed=seed)
    dyn.temperature = temp
    dyn.set_masks(masks)
    if not hmc:
        dyn.XNet.load_state(xp)
        dyn.VNet.load_state(vp)
    return dyn


def _setup(la, kind, dim, nodes, N, B, easy=False, hmc=False, temp=1.0, regime="mild", seed=5):
    dist, ref, params = _target(la, kind, dim, 0.5 if easy else 0.8, easy)
    xp, vp = H.mlp_weights(dim, nodes, seed=106, regime=regime)
    masks = ogen.make_masks(N, dim, np.random.RandomState(3))
    dyn = _dyn(la, dist.get_energy_function(), dim, nodes, N, masks, xp, vp, hmc=hmc, temp=temp)
    assert not dyn.layered
    mk = lambda dt: ogen.DynamicsOracle(dim, ref, N, 0.1, masks, xp, vp, hmc=hmc, temperature=temp, dtype=dt)  # noqa: E731
    rng = np.random.default_rng(seed + B)
    np.random.seed(seed + B)
    x = f32(dist.get_samples(B) if kind == "funnel" else rng.normal(0, 1.0, (B, dim)))
    draws = (f32(rng.standard_normal((B, dim))), f32(rng.standard_normal((B, dim))),
             rng.integers(0, 2, B).astype(np.float64), rng.uniform(size=B))
    return dyn, mk(np.float64), mk(np.float32), x, draws, (dist, ref, params, masks, xp, vp)


CASES = [("rw", 2, 10, 3, 8, False), ("rw", 2, 50, 10, 24, True), ("rw", 3, 50, 3, 129, False), ("rw", 8, 10, 10, 24, True),
         ("rw", 2, 50, 10, 129, False), ("funnel", 2, 50, 10, 24, None), ("funnel", 2, 10, 3, 129, None),
         ("funnel", 3, 10, 10, 8, None), ("funnel", 8, 50, 3, 24, None), ("funnel", 3, 50, 10, 129, None)]


@pytest.mark.parametrize("kind,dim,nodes,N,B,easy", CASES)
def test_trajectories_and_propose_match_the_oracle_in_every_form(la, kind, dim, nodes, N, B, easy):
    dyn, o64, o32, x, (vf, vb, bits, u), _ = _setup(la, kind, dim, nodes, N, B, bool(easy))
    want = {"f": o64.forward(x, vf), "b": o64.backward(x, vb), "p": ogen.propose(x, o64, vf, vb, bits, u=u, do_mh_step=True)}
    x32, vf32, vb32 = (a.astype(np.float32) for a in (x, vf, vb))
    w32 = {"f": o32.forward(x32, vf32), "b": o32.backward(x32, vb32),
           "p": ogen.propose(x32, o32, vf32, vb32, bits.astype(np.float32), u=u.astype(np.float32), do_mh_step=True)}
    assert float(want["p"][2].mean()) > 0.01
    outs = {}
    for form in ((1, 2, 3) if nodes > 16 else (1, 2)):
        dyn.first_layer_form = form
        got = {"f": dyn.forward(x, init_v=vf), "b": dyn.backward(x, init_v=vb)}
        Lx, Lv, px, (out,) = la.propose(x, dyn, init_v=vf, init_v_backward=vb, dir_bits=bits, u=u, do_mh_step=True)
        for d in "fb":
            for i, name in enumerate(("x", "v")):
                assert_fp32_equivalent(np_(got[d][i]), want[d][i], w32[d][i], f"{kind} form {form} {d} {name}")
            perr, pint = np.abs(np_(got[d][2]) - want[d][2]).max(), np.abs(w32[d][2] - want[d][2]).max()
            assert perr < max(TOL_P, P_RATIO * pint), (form, d, perr, pint)
        assert_fp32_equivalent(np_(Lx), want["p"][0], w32["p"][0], f"{kind} form {form} propose Lx")
        assert_fp32_equivalent(np_(Lv), want["p"][4], w32["p"][4], f"{kind} form {form} propose Lv")
        perr, pint = np.abs(np_(px) - want["p"][2]).max(), np.abs(w32["p"][2] - want["p"][2]).max()
        assert perr < max(TOL_P, P_RATIO * pint), (form, perr, pint)
        safe = np.abs(want["p"][2] - u) > 1e-4
        assert H.relerr(np_(out)[safe], want["p"][3][0][safe]) < max(TOL_OP, MAX_RATIO * H.relerr(w32["p"][0], want["p"][0]))
        outs[form] = (got["f"][0], got["b"][0], Lx, px)
    for form in outs:
        errs = [H.relerr(np_(a), np_(b)) for a, b in zip(outs[1], outs[form])]
        assert max(errs) < FORMS_TOL, (form, errs)


@pytest.mark.parametrize("kind,dim", [("rw", 2), ("funnel", 3)])
def test_plain_hmc_plan(la, kind, dim):
    dyn, o64, o32, x, (vf, _, _, _), _ = _setup(la, kind, dim, 10, 10, 24, hmc=True, temp=2.5)
    got, want, w32 = dyn.forward(x, init_v=vf), o64.forward(x, vf), o32.forward(x.astype(np.float32), vf.astype(np.float32))
    for i, name in enumerate(("x", "v")):
        assert_fp32_equivalent(np_(got[i]), want[i], w32[i], f"hmc {kind} {name}")
    assert np.abs(np_(got[2]) - want[2]).max() < max(TOL_P, P_RATIO * np.abs(w32[2] - want[2]).max())


# ------------------------------------------------------------------------------------------- 3. fused against layered
def _torch_energy(kind, params):
    if kind == "rw":
        eps, easy = params
        a = np.float32(eps) if easy else np.float32(eps) * np.float32(eps)

        def fn(x):
            return 0.5 * (x * x).sum(1) + eps * torch.cos(x / float(a)).sum(1)
    else:
        def fn(x):
            v, n = x[:, 0], x.shape[1] - 1
            hi, lo = v > CLIP, -CLIP > v
            s = torch.where(hi, torch.full_like(v, math.exp(CLIP)),
                            torch.where(lo, torch.full_like(v, math.exp(-CLIP)), torch.exp(torch.where(hi | lo, 0 * v, v))))
            return 0.5 * ((v / SIGMA) ** 2 + (x[:, 1:] ** 2).sum(1) / s + n * torch.log(2 * math.pi * s))
    return fn


@pytest.mark.parametrize("kind,dim,nodes,B,easy", [("rw", 2, 50, 129, False), ("rw", 3, 10, 24, True),
                                                  ("funnel", 2, 50, 129, None), ("funnel", 3, 10, 24, None)])
def test_fused_and_layered_proposals_agree(la, kind, dim, nodes, B, easy):
    N = 5
    fused, _, _, x, _, (dist, ref, params, masks, xp, vp) = _setup(la, kind, dim, nodes, N, B, bool(easy))
    layered = _dyn(la, _torch_energy(kind, params), dim, nodes, N, masks, xp, vp)
    assert layered.layered and not fused.layered
    outs = []
    for dyn in (fused, layered):
        dyn._draws = 8
        Lx, _, px, _ = la.propose(x, dyn, do_mh_step=False)
        dyn._draws = 8
        v = dyn._normal((B, dim))
        _, Lv, _, _ = la.propose(x, dyn, init_v=v, do_mh_step=False)
        outs.append((np_(Lx), np_(Lv), np_(px)))
    errs = [H.relerr(a, b) for a, b in zip(*outs)]
    print(f"{kind} fused vs layered Lx, Lv, px: {errs}")
    assert max(errs) < FORMS_TOL, errs
    assert outs[0][2].mean() > 0.01


# ------------------------------------------------------------------------------------------- 4. DynamicsSampler.run
def _sampler(la, kind, dim, nodes, spl, form=0):
    dist, _, _ = _target(la, kind, dim, 0.5, True)
    xp, vp = H.mlp_weights(dim, nodes, seed=106, regime="stress")
    N = 5
    dyn = _dyn(la, dist.get_energy_function(), dim, nodes, N, ogen.make_masks(N, dim, np.random.RandomState(3)), xp, vp)
    dyn.first_layer_form = form
    dyn._draws = 4
    smp = la.DynamicsSampler(dyn)
    assert smp.steps_per_launch == 256
    smp.steps_per_launch = spl
    return smp


@pytest.mark.parametrize("B", [24, 129])
@pytest.mark.parametrize("kind,dim,nodes,form", [("rw", 2, 50, 3), ("rw", 3, 10, 1), ("funnel", 2, 10, 2), ("funnel", 3, 50, 0)])
def test_run_equals_the_loop_over_propose(la, kind, dim, nodes, form, B):
    g = torch.Generator(device="cpu").manual_seed(99 + B)
    x0 = (0.7 * torch.randn(B, dim, generator=g)).to("cuda")
    new, old = _sampler(la, kind, dim, nodes, 256, form), _sampler(la, kind, dim, nodes, 1, form)
    a, b = new.run(5, x0, keep_samples=True), old.run(5, x0, keep_samples=True)
    for k in ("px", "samples"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))
    assert torch.equal(a["samples_out"], b["samples_out"]) and new.dynamics._draws == old.dynamics._draws == 24
    assert np.isfinite(a["samples"]).all() and 0.0 < a["mean_accept"] <= 1.0
    assert (a["samples"][1:] != a["samples"][:-1]).any()


@pytest.mark.parametrize("kind", ["rw", "funnel"])
def test_run_is_one_launch_per_chunk(la, kind):
    from l2hmc_amd import _lib
    Lh = _lib.lib()
    x = torch.zeros(64, 2, device="cuda") + 0.3
    for spl in (8, 3, 1):
        smp = _sampler(la, kind, 2, 10, spl)
        smp.run(8, x)
        _lib.check(Lh.l2hmc_profile_begin(7))
        smp.run(8, x)
        ms, n = C.c_double(), C.c_int64()
        _lib.check(Lh.l2hmc_profile_end(C.byref(ms), C.byref(n)))
        assert int(n.value) == (math.ceil(8 / spl) if spl > 1 else 8)


# ------------------------------------------------------------------------------------------- 5. gradients
def _t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _rel(got, want):
    want = want.detach()
    got = got.detach().cpu().double().reshape(want.shape)
    scale = float(want.abs().max())
    assert scale > 0
    return float((got - want).abs().max()) / scale


def _far_from(p, u):
    return np.where(np.abs(p - u) < 1e-3, 0.5 * p, u)


def _grad_setup(la, kind, dim, nodes, N, B, temp, easy):
    dyn, _, _, x, dx, (dist, ref, params, masks, xp, vp) = _setup(la, kind, dim, nodes, N, B, easy, temp=temp, seed=31)
    rng = np.random.default_rng(77 + B)
    z = f32(rng.standard_normal((B, dim)))
    if kind == "funnel":
        # chains on each side of both clips: the Hessian's branch selection runs in the reverse pass
        x[:4, 0] = f32([8.6, 7.4, -8.6, -7.4])[:min(4, B)]
        x[:4, 1:] = f32(rng.standard_normal((4, dim - 1)) * np.exp(np.clip(x[:4, :1], -CLIP, CLIP) / 2))
    dz = (f32(rng.standard_normal((B, dim))), f32(rng.standard_normal((B, dim))),
          rng.integers(0, 2, B).astype(np.float64), rng.uniform(size=B))
    tm = TorchAnalyticModel(kind, params, N, 0.1, masks, xp, vp, temperature=temp)
    with torch.no_grad():
        _, px = tm.propose(_t64(x), _t64(dx[0]), _t64(dx[1]), _t64(dx[2]))
    dx = dx[:3] + (_far_from(px.numpy(), dx[3]),)
    return dyn, tm, x, z, dx, dz


def _want(tm, x, z, dx, dz):
    for t in [tm.alpha, *tm.xnet.values(), *tm.vnet.values()]:
        t.grad = None
    loss, *_ = tm.mog_loss(_t64(x), _t64(z), tuple(map(_t64, dx)), tuple(map(_t64, dz)), SCALE)
    loss.backward()
    return float(loss.detach())


def _compare(grads_x, grads_v, g_alpha, tm, what):
    worst = {}
    for name, got, ref in (("xnet", grads_x, tm.xnet), ("vnet", grads_v, tm.vnet)):
        for k, t in ref.items():
            worst[f"{name}.{k}"] = _rel(got[k], t.grad)
    worst["alpha"] = _rel(g_alpha, tm.alpha.grad)
    print(what, {k: f"{v:.1e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= TOL_G}
    assert not bad, f"{what}: gradient mismatch {bad}"


GRAD_CASES = [("rw", 2, 10, 5, 9, 1.0, False), ("rw", 2, 50, 5, 37, 2.5, True), ("rw", 3, 50, 4, 21, 1.0, True),
              ("funnel", 2, 50, 5, 21, 1.0, None), ("funnel", 3, 10, 4, 37, 2.5, None), ("funnel", 2, 10, 5, 9, 2.5, None)]


@pytest.mark.parametrize("kind,dim,nodes,N,B,temp,easy", GRAD_CASES)
def test_trainer_gradients_match_float64(la, kind, dim, nodes, N, B, temp, easy):
    from l2hmc_amd import autograd_toy
    from l2hmc_amd.dynamics_trainer import DynamicsTrainer
    dyn, tm, x, z, dx, dz = _grad_setup(la, kind, dim, nodes, N, B, temp, bool(easy))
    want = _want(tm, x, z, dx, dz)
    tr = DynamicsTrainer(dyn, scale=SCALE)
    loss, _, _ = tr.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
    assert abs(float(loss) - want) <= 2e-4 * max(1., abs(want)), (float(loss), want)
    gx, gv, ga = autograd_toy.unpack(dyn, tr.grads)
    _compare(gx, gv, ga, tm, f"trainer {kind} dim={dim} H={nodes} B={B} T={temp}")


@pytest.mark.parametrize("kind,dim,nodes,N,B,temp,easy", GRAD_CASES)
def test_autograd_route_matches_float64(la, kind, dim, nodes, N, B, temp, easy):
    dyn, tm, x, z, dx, dz = _grad_setup(la, kind, dim, nodes, N, B, temp, bool(easy))
    want = _want(tm, x, z, dx, dz)
    for v in dyn.variables:
        v.requires_grad_()
    xt, zt = (torch.as_tensor(a, dtype=torch.float32, device=dyn._device) for a in (x, z))
    Lx, _, px, out = la.propose(xt, dyn, init_v=dx[0], init_v_backward=dx[1], dir_bits=dx[2], u=dx[3], do_mh_step=True)
    Lz, _, pz, _ = la.propose(zt, dyn, init_v=dz[0], init_v_backward=dz[1], dir_bits=dz[2])
    v1 = ((xt - Lx) ** 2).sum(1) * px + 1e-4
    v2 = ((zt - Lz) ** 2).sum(1) * pz + 1e-4
    loss = SCALE * ((1. / v1).mean() + (1. / v2).mean()) + (-v1.mean() - v2.mean()) / SCALE
    loss.backward()
    assert abs(float(loss.detach()) - want) <= 2e-4 * max(1., abs(want))
    gx = {k: t.grad for k, t in dyn.XNet.state_dict().items()}
    gv = {k: t.grad for k, t in dyn.VNet.state_dict().items()}
    _compare(gx, gv, dyn.alpha.grad, tm, f"autograd {kind} dim={dim} H={nodes} B={B} T={temp}")


@pytest.mark.parametrize("kind", ["rw", "funnel"])
def test_start_state_gradients_match_float64(la, kind):
    dyn, tm, x, _, dx, _ = _grad_setup(la, kind, 2, 10, 5, 21, 1.0, True)
    rng = np.random.default_rng(3)
    c = [rng.standard_normal(x.shape), rng.standard_normal(x.shape), rng.standard_normal(x.shape[0])]
    xg = torch.tensor(x, dtype=torch.float32, device=dyn._device, requires_grad=True)
    vg = torch.tensor(dx[0], dtype=torch.float32, device=dyn._device, requires_grad=True)
    got = dyn.forward(xg, init_v=vg)
    sum((torch.tensor(ci, dtype=torch.float32, device=dyn._device) * o).sum() for ci, o in zip(c, got)).backward()
    x64, v64 = _t64(x).requires_grad_(), _t64(dx[0]).requires_grad_()
    X, V, P, _ = tm.trajectory(x64, v64, None, False)
    sum((_t64(ci) * o).sum() for ci, o in zip(c, (X, V, P))).backward()
    ex, ev = _rel(xg.grad, x64.grad), _rel(vg.grad, v64.grad)
    print(f"{kind} d/dx {ex:.1e} d/dinit_v {ev:.1e}")
    assert ex <= TOL_G and ev <= TOL_G, (ex, ev)


# ------------------------------------------------------------------------------------------- 6. training moves
def test_training_lowers_the_loss_on_an_easy_rough_well(la):
    from l2hmc_amd.dynamics_trainer import DynamicsTrainer
    np.random.seed(0)
    torch.manual_seed(0)
    dist = la.RoughWell(2, 0.5, easy=True)
    dyn = la.Dynamics(2, dist.get_energy_function(), trajectory_length=5, eps=0.1,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=10), seed=1)
    tr = DynamicsTrainer(dyn, scale=SCALE)
    x = torch.as_tensor(dist.get_samples(256), dtype=torch.float32, device="cuda")
    losses = []
    for _ in range(200):
        loss, x, _ = tr.train_step(x)[:3]
        losses.append(float(loss))
    assert np.isfinite(losses).all()
    assert np.mean(losses[-20:]) < np.mean(losses[:20]), (np.mean(losses[:20]), np.mean(losses[-20:]))


# ------------------------------------------------------------------------------------------- 7. the old targets
@pytest.mark.parametrize("name", ["mog_cfg2", "scg_cfg1"])
def test_old_targets_are_deterministic(la, name):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    if name.startswith("mog"):
        m = H.mog_target_oracle()
        fn, nodes = la.GMM(m.mus, m.sigmas, m.pis).get_energy_function(), 50
    else:
        fn, nodes = la.Gaussian(np.zeros(2), np.array([[50.05, -49.95], [-49.95, 50.05]])).get_energy_function(), 10
    N = int(g["masks"].shape[0])
    xp, vp = H.mlp_weights(2, nodes, seed=106, regime="stress")
    x = torch.as_tensor(g["x"], dtype=torch.float32, device="cuda")
    outs = []
    for _ in range(2):
        dyn = _dyn(la, fn, 2, nodes, N, g["masks"], xp, vp, eps=float(g["eps"]))
        dyn._draws = 4
        Lx, _, px, (out,) = la.propose(x, dyn, do_mh_step=True)
        smp = la.DynamicsSampler(dyn)
        run = smp.run(3, x, keep_samples=True)
        outs.append((Lx, px, out, torch.as_tensor(run["px"]), torch.as_tensor(run["samples"])))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert torch.isfinite(outs[0][0]).all()
