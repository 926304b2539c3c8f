"""Host-side pieces of the toy-target autograd path (l2hmc_amd/autograd_toy.py), no GPU needed: the argument
checks of l2hmc_small_vjp, the refusals of what it does not take, the re-pack of MLPNet after a weight moved, and
Dynamics.variables."""
import ctypes as C

import numpy as np
import pytest
import torch

import l2hmc_amd as la
from l2hmc_amd import _lib, build as lbuild

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def L():
    lbuild.build()
    return _lib.lib()


def _plan(dim=2, H=10, N=3, hmc=0):
    """A plan whose pointers are any non-NULL address: the host checks reject before a launch."""
    net = lambda: _lib.DenseNet(D=dim, H=H, Ka=dim, Kb=dim, q_tanh=1, reserved=0, packed=None,  # noqa: E731
                                **{k: 16 for k in ("w1_t", "wt", "b1", "wh_t", "bh", "whd_t", "bhd", "coeff_s",
                                                   "coeff_q")})
    tgt = _lib.MogTarget(dim=dim, K=2, is_gaussian=0, temperature=1.0, mu=16, prec=16, log_const=16)
    return _lib.SmallPlan(x_dim=dim, num_nodes=H, trajectory_length=N, hmc=hmc, eps=0.1, first_layer_form=0,
                          masks=16, xnet=net(), vnet=net(), target=tgt)


def _vjp(L, plan, rows, null=None, ws_bytes=1 << 30):
    names = ("x0", "v0", "dir", "g_x", "g_v", "g_logdet", "g_p", "dx0", "dv0", "grads", "x_out", "v_out",
             "sumlogdet", "p_accept", "ws")
    args = [None if n == null else 16 for n in names]
    return L.l2hmc_small_vjp(C.byref(plan), *args[:3], rows, *args[3:], ws_bytes, None)


def test_vjp_checks_arguments_on_the_host(L):
    assert L.l2hmc_small_vjp(None, *([None] * 3), 4, *([None] * 11), None, 0, None) == 1
    assert _vjp(L, _plan(hmc=1), 4) == 1
    assert b"hmc" in L.l2hmc_last_error()
    for bad in (dict(dim=9), dict(dim=0), dict(H=65), dict(H=0), dict(N=0)):
        assert _vjp(L, _plan(**bad), 4) == 1, bad
    plan = _plan()
    plan.target.dim = 3                                    # target and plan disagree
    assert _vjp(L, plan, 4) == 1
    plan = _plan()
    plan.xnet.H = 12                                       # net and plan disagree
    assert _vjp(L, plan, 4) == 1
    assert b"shape" in L.l2hmc_last_error()
    plan = _plan()
    plan.vnet.whd_t = None
    assert _vjp(L, plan, 4) == 1
    for name in ("x0", "v0", "grads", "ws"):
        assert _vjp(L, _plan(), 4, null=name) == 1, name
        assert b"NULL" in L.l2hmc_last_error()
    assert _vjp(L, _plan(), -1) == 1
    assert _vjp(L, _plan(N=400, H=64), 4) == 1             # the LDS tape of 1600 calls does not fit
    assert b"LDS" in L.l2hmc_last_error()
    assert _vjp(L, _plan(), 4, ws_bytes=16) == 3           # workspace too small
    # nothing to do, nothing launched; optional pointers may all be NULL
    assert _vjp(L, _plan(), 0) == 0
    assert L.l2hmc_small_vjp(C.byref(_plan()), *([None] * 3), 0, *([None] * 11), None, 0, None) == 0


def _dyn(hmc=False, H=10, x_dim=2, target=None, net_factory=None):
    np.random.seed(0)
    tgt = target or la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])
    fn = tgt.get_energy_function() if target is not False else (lambda x: (x ** 2).sum(1))
    nf = net_factory or (lambda d, scope, factor: la.network(d, scope, factor, num_nodes=H, device=CPU))
    return la.Dynamics(x_dim, fn, trajectory_length=3, eps=0.1, hmc=hmc, net_factory=nf, device=CPU)


def test_variables_order_and_contents():
    dyn = _dyn()
    v = dyn.variables
    assert v[0] is dyn.alpha and v[0].shape == () and v[0].is_leaf
    assert float(dyn.alpha) == pytest.approx(np.log(0.1), abs=1e-7)
    layers = ("embed_1", "embed_2", "embed_3", "linear_1", "linear_s", "linear_t", "linear_f")
    for i, net in enumerate((dyn.XNet, dyn.VNet)):
        want = []
        for n in layers:
            want += [getattr(net, n).kernel, getattr(net, n).bias]
        want += [net.scale_s, net.scale_f]
        got = v[1 + i * 16:1 + (i + 1) * 16]
        assert len(got) == 16 and all(a is b for a, b in zip(got, want))
    assert len(v) == 33
    assert [t is u for t, u in zip(dyn.trainable_variables, v)] == [True] * 33
    dyn.eps_trainable = False
    assert len(dyn.trainable_variables) == 32 and dyn.trainable_variables[0] is dyn.XNet.embed_1.kernel
    dyn.alpha.requires_grad_()
    assert float(dyn.eps.detach()) == pytest.approx(0.1)
    hmc = _dyn(hmc=True)
    assert len(hmc.variables) == 1 and hmc.variables[0] is hmc.alpha


def test_refusals_before_any_draw():
    x = torch.zeros(4, 2, requires_grad=True)
    hmc = _dyn(hmc=True)
    with pytest.raises(NotImplementedError, match="hmc"):
        hmc.forward(x)
    with pytest.raises(NotImplementedError, match="hmc"):
        la.propose(x, hmc, do_mh_step=True)
    hmc.alpha.requires_grad_()
    with pytest.raises(NotImplementedError, match="hmc"):
        hmc.backward(torch.zeros(4, 2))
    assert hmc._draws == 0
    layered = _dyn(target=False)                           # an arbitrary energy callable
    assert layered.layered
    with pytest.raises(NotImplementedError, match="layer by layer"):
        layered.forward(x)
    with pytest.raises(NotImplementedError, match="layer by layer"):
        la.propose(x, layered, init_v=torch.zeros(4, 2))
    wide = _dyn(H=65)
    assert wide.layered
    with pytest.raises(NotImplementedError, match="layer by layer"):
        wide.backward(x)
    assert layered._draws == 0 and wide._draws == 0
    owned = _dyn()
    owned.XNet.flat_params()                               # what DynamicsTrainer does
    with pytest.raises(ValueError, match="DynamicsTrainer"):
        owned.forward(x)
    with pytest.raises(ValueError, match="DynamicsTrainer"):
        la.propose(x, owned, do_mh_step=True)
    assert owned._draws == 0
    # a weight that requires grad makes the call differentiable (and so refused) too
    for t in layered.XNet._ref_tensors():
        t.requires_grad_()
    with pytest.raises(NotImplementedError, match="layer by layer"):
        layered.forward(torch.zeros(4, 2))
    # no grad mode: the sampling path, not the refusal (which would have come first)
    with torch.no_grad():
        from l2hmc_amd import autograd_toy
        assert not autograd_toy.wants_grad(layered, x)


def test_mlpnet_repacks_after_a_weight_moves():
    net = la.network(2, "XNet", 2.0, num_nodes=10, device=CPU)
    assert net._tracks_versions
    net._check_ref_version()
    net._packed = "built"
    net._check_ref_version()
    assert net._packed == "built"
    with torch.no_grad():
        net.linear_1.kernel.add_(1.0)                      # in place, as torch.optim does
    net._check_ref_version()
    assert net._packed is None
    net._packed = "built"
    net.scale_f = net.scale_f.clone()                      # a new tensor object
    net._check_ref_version()
    assert net._packed is None
    net._packed = "built"
    net.flat_params()                                      # a trainer owns the weights: its optimiser re-packs
    net._packed = "built"
    with torch.no_grad():
        net.linear_1.kernel.add_(1.0)
    net._check_ref_version()
    assert net._packed == "built"


def test_unpack_grads_inverts_the_mlp_packing():
    net = la.network(3, "VNet", 1.0, num_nodes=12, device=CPU)
    torch.manual_seed(0)
    for t in net._ref_tensors():
        t.copy_(torch.randn_like(t))
    packed = net._pack_tensors()
    got = net.unpack_grads(packed)
    sd = net.state_dict()
    assert set(got) == set(sd)
    b1 = net.embed_1.bias + net.embed_2.bias + net.embed_3.bias
    for k, t in sd.items():
        assert got[k].shape == t.shape, k
        assert torch.equal(got[k], b1 if k in ("embed_1/b", "embed_2/b", "embed_3/b") else t), k
