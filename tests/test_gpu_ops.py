"""l2hmc_amd/ops.py on the GPU: every function against the raw C call on the same inputs, bit for bit, and the checks
that keep a tensor the kernels would misread from reaching them.  Shapes: a 4 x 6 lattice (D = 48) with 9 rows, and
D = 8 (a 2 x 2 lattice) with 5 and 70 rows: a partial wave, and more rows than one wave."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(4, 6, 9), (2, 2, 5), (2, 2, 70)]


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    return l2hmc_amd


def _inputs(T, X, B):
    rng = np.random.default_rng(1000 * T + 10 * X + B)
    D = 2 * T * X
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")   # noqa: E731
    t = {k: dev(rng.standard_normal((B, D))) for k in ("v", "grad", "vf", "xb", "vb", "u2")}
    t["x"] = dev(rng.uniform(-7, 13, (B, D)))
    t["xf"] = dev(rng.uniform(0, 2 * np.pi, (B, D)))
    t.update({k: dev(0.3 * rng.standard_normal((B, D))) for k in ("S", "T", "Q")})
    t["keep"] = dev(rng.uniform(size=D) < 0.5)
    t.update({k: dev(rng.uniform(size=B)) for k in ("pf", "pb", "coin", "u")})
    t.update({k: dev(rng.standard_normal(B)) for k in ("h_old", "h_new", "sld")})
    return t


def _raw(name, *args):
    from l2hmc_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream_ptr()))


def _eq(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None and w is None) or torch.equal(g, w)


@pytest.mark.parametrize("T,X,B", SHAPES)
def test_ops_equal_the_raw_c_calls(la, T, X, B):
    from l2hmc_amd import ops
    t = _inputs(T, X, B)
    D = 2 * T * X
    p = lambda k: t[k].data_ptr()                 # noqa: E731
    rows = lambda: torch.empty(B, device="cuda")  # noqa: E731
    mat = lambda: torch.empty(B, D, device="cuda")  # noqa: E731

    want = rows()
    _raw("l2hmc_kinetic_energy", p("v"), B, D, want.data_ptr())
    assert torch.equal(ops.kinetic_energy(t["v"]), want)

    want = rows()
    _raw("l2hmc_accept_prob", p("h_old"), p("h_new"), p("sld"), B, want.data_ptr())
    assert torch.equal(ops.accept_prob(t["h_old"], t["h_new"], t["sld"]), want)

    want = mat()
    _raw("l2hmc_wrap_angle", p("x"), B * D, want.data_ptr())
    assert torch.equal(ops.wrap_angle(t["x"]), want)
    other = torch.full((B, D), -1.0, device="cuda")
    assert ops.wrap_angle(t["x"], out=other) is other and torch.equal(other, want)
    assert float(want.min()) >= 0.0 and float(want.max()) < 2 * np.pi + 1e-6

    for d in (0, 1):
        wv, wl = mat(), rows()
        _raw("l2hmc_lf_update_v", p("v"), p("grad"), p("S"), p("T"), p("Q"), 0.1, d, B, D, wv.data_ptr(), wl.data_ptr())
        _eq(ops.lf_update_v(t["v"], t["grad"], t["S"], t["T"], t["Q"], 0.1, d), (wv, wl))
        wx, wl = mat(), rows()
        _raw("l2hmc_lf_update_x", p("x"), p("v"), p("keep"), p("S"), p("T"), p("Q"), 0.1, d, B, D, wx.data_ptr(),
             wl.data_ptr())
        _eq(ops.lf_update_x(t["x"], t["v"], t["keep"], t["S"], t["T"], t["Q"], 0.1, d), (wx, wl))

    mix = [t[k] for k in ("x", "xf", "vf", "pf", "xb", "vb", "pb", "coin")]
    mp = [a.data_ptr() for a in mix]
    for strict in (0, 1):
        full = (mat(), mat(), rows(), mat())
        _raw("l2hmc_mix_accept", *mp, p("u"), strict, B, D, *(a.data_ptr() for a in full))
        _eq(ops.mix_accept(*mix, t["u"], strict), full)
        only_out = mat()                                   # sampler.tf_accept's form
        _raw("l2hmc_mix_accept", *mp, p("u"), strict, B, D, None, None, None, only_out.data_ptr())
        _eq(ops.mix_accept(*mix, t["u"], strict, want_proposal=False), (None, None, None, only_out))
        assert torch.equal(only_out, full[3])
        prop = (mat(), mat(), rows())                      # no MH step
        _raw("l2hmc_mix_accept", *mp, None, strict, B, D, *(a.data_ptr() for a in prop), None)
        _eq(ops.mix_accept(*mix, None, strict, want_out=False), (*prop, None))
        _eq(ops.mix_accept(*mix, t["u"], strict, want_out=False), (*prop, None))

    act, force, plaq, chg = rows(), mat(), rows(), rows()
    _raw("l2hmc_u1_action_force", p("xf"), B, T, X, 2.5, act.data_ptr(), force.data_ptr(), plaq.data_ptr(), chg.data_ptr())
    _eq(ops.u1_action_force(t["xf"], T, X, 2.5), (act, force, plaq, chg))
    f_only = mat()
    _raw("l2hmc_u1_action_force", p("xf"), B, T, X, 2.5, None, f_only.data_ptr(), None, None)
    _eq(ops.u1_action_force(t["xf"], T, X, 2.5, want_observables=False), (None, f_only, None, None))
    o_only = (rows(), rows(), rows())
    _raw("l2hmc_u1_action_force", p("xf"), B, T, X, 2.5, o_only[0].data_ptr(), None, o_only[1].data_ptr(),
         o_only[2].data_ptr())
    _eq(ops.u1_action_force(t["xf"], T, X, 2.5, want_force=False), (o_only[0], None, o_only[1], o_only[2]))
    obs = la.lattice.u1_observables(t["xf"], T, X, 2.5, want_force=True)
    _eq([obs[k] for k in ("action", "force", "avg_plaq", "top_charge")], (act, force, plaq, chg))

    want = mat()
    _raw("l2hmc_u1_force_hvp", p("xf"), p("u2"), B, T, X, 2.5, want.data_ptr())
    assert torch.equal(ops.u1_force_hvp(t["xf"], t["u2"], T, X, 2.5), want)

    for name in ("fill_normal", "fill_uniform"):
        want = mat()
        _raw("l2hmc_" + name, want.data_ptr(), B * D, 42, 7)
        got = getattr(ops, name)((B, D), 42, 7, torch.device("cuda", torch.cuda.current_device()))
        assert got.shape == (B, D) and torch.equal(got, want)
        buf = torch.full((3 * B * D,), -5.0, device="cuda")      # the out= form on a slice: the rest stays
        assert getattr(ops, name)(None, 42, 7, out=buf[B * D:2 * B * D]).data_ptr() == buf[B * D:].data_ptr()
        assert torch.equal(buf[B * D:2 * B * D], want.reshape(-1))
        assert bool((buf[:B * D] == -5.0).all()) and bool((buf[2 * B * D:] == -5.0).all())


def _calls(ops, T, X):
    """({argument name: key of _inputs}, callable) over every caller-supplied tensor of every function."""
    same = lambda *ks: dict(zip(ks, ks))          # noqa: E731
    return [
        (same("v"), ops.kinetic_energy),
        (dict(h_old="h_old", h_new="h_new", sumlogdet="sld"), ops.accept_prob),
        (dict(x="x", out="xb"), lambda x, out: ops.wrap_angle(x, out=out)),
        (same("v", "grad", "S", "T", "Q"), lambda *a: ops.lf_update_v(*a, 0.1, 0)),
        (same("x", "v", "keep", "S", "T", "Q"), lambda *a: ops.lf_update_x(*a, 0.1, 1)),
        (same("x", "xf", "vf", "pf", "xb", "vb", "pb", "coin", "u"), lambda *a: ops.mix_accept(*a, 1)),
        (dict(x="xf"), lambda x: ops.u1_action_force(x, T, X, 2.5)),
        (dict(x="xf", u="u2"), lambda x, u: ops.u1_force_hvp(x, u, T, X, 2.5)),
        (dict(out="xb"), lambda out: ops.fill_normal(None, 1, 2, out=out)),
        (dict(out="xb"), lambda out: ops.fill_uniform(None, 1, 2, out=out)),
    ]


def _strided(a):
    """The same shape and values, not contiguous: [B, D] transposed and restored, [n] every other element."""
    v = a.t().contiguous().t() if a.dim() == 2 else torch.stack([a, a], 1)[:, 0]
    assert v.shape == a.shape and not v.is_contiguous() and torch.equal(v, a)
    return v


def test_non_contiguous_and_float64_tensors_raise_and_touch_nothing(la):
    from l2hmc_amd import ops
    T, X, B = SHAPES[0]
    t = _inputs(T, X, B)
    good = ops.lf_update_v(t["v"], t["grad"], t["S"], t["T"], t["Q"], 0.1, 0) + (ops.wrap_angle(t["x"]),)
    kept = [a.clone() for a in good] + [t["xb"].clone()]
    good += (t["xb"],)                            # the out= target of the calls below
    for names, fn in _calls(ops, T, X):
        for i, name in enumerate(names):
            args = [t[k] for k in names.values()]
            for bad, exc, text in ((_strided(args[i]), ValueError, "tensor must be contiguous"),
                                   (args[i].double(), TypeError, "expected torch.float32, got torch.float64")):
                with pytest.raises(exc, match=f"^{name}: {text}"):
                    fn(*args[:i], bad, *args[i + 1:])
    with pytest.raises(ValueError, match="^out: expected shape"):
        ops.wrap_angle(t["x"], out=t["x"][:-1])
    torch.cuda.synchronize()
    for a, k in zip(good, kept):
        assert torch.equal(a, k)


def test_gauge_sampler_wrap_refuses_a_non_contiguous_view(la):
    T, X, B = SHAPES[0]
    lattice = la.lattice.GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    dyn = la.gauge_dynamics.GaugeDynamics(lattice, lattice.get_energy_function(), hmc=True, num_steps=2, eps=0.1)
    sampler = la.gauge_sampler.GaugeSampler(dyn)
    x = _inputs(T, X, B)["x"]
    want = torch.empty_like(x)
    _raw("l2hmc_wrap_angle", x.data_ptr(), x.numel(), want.data_ptr())
    assert torch.equal(sampler.wrap(x), want)
    with pytest.raises(ValueError, match="^x: tensor must be contiguous"):
        sampler.wrap(x.t().contiguous().t())
