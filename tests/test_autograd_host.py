"""Host-side pieces of the autograd path (l2hmc_amd/autograd.py), no GPU needed: the argument checks of
l2hmc_gauge_accept_backward, the inverse of the weight packing, and the re-pack after a weight moved."""
import ctypes as C

import pytest
import torch

from l2hmc_amd import _lib, build as lbuild
from l2hmc_amd.network import ConvNet3D, GenericNet


@pytest.fixture(scope="module")
def L():
    lbuild.build()
    return _lib.lib()


def _accept_bwd(L, rows, T=3, X=5, null=None):
    """Every required pointer non-NULL (any address: the host check rejects before a launch), except `null`."""
    names = ("x0", "v0", "xN", "vN", "p", "u", "g_xprop", "g_vprop", "g_p", "g_xout", "dxN", "dvN", "dlogdet",
             "dx0", "dv0")
    args = [None if n == null else 16 for n in names]
    return L.l2hmc_gauge_accept_backward(T, X, 1.0, rows, *args, None)


def test_accept_backward_checks_arguments_on_the_host(L):
    for name in ("x0", "xN", "vN", "p", "u", "dxN", "dvN", "dlogdet"):
        assert _accept_bwd(L, 4, null=name) == 1, name
        assert b"NULL" in L.l2hmc_last_error()
    assert _accept_bwd(L, 4, null="v0") == 1              # dv0 needs v0
    assert _accept_bwd(L, -1) == 1
    assert _accept_bwd(L, 4, T=0) == 1
    assert _accept_bwd(L, 4, T=128, X=128) == 1           # the staged chain would not fit in LDS
    assert _accept_bwd(L, 0) == 0                         # nothing to do, nothing launched
    assert L.l2hmc_gauge_accept_backward(3, 5, 1.0, 0, *([None] * 15), None) == 0


def _net(cls, **kw):
    torch.manual_seed(0)
    net = cls(model_name="XNet", device=torch.device("cpu"), **kw)
    for t in net._ref_tensors():
        t.copy_(torch.randn_like(t))
    return net


@pytest.mark.parametrize("cls,kw", [
    (GenericNet, dict(x_dim=32, num_hidden=64, factor=2., links_shape=(4, 4, 2))),
    (ConvNet3D, dict(x_dim=128, num_hidden=256, factor=2., links_shape=(8, 8, 2), num_filters=8, spatial_size=8)),
])
def test_unpack_grads_inverts_the_packing(cls, kw):
    """unpack_grads maps every buffer of the packed layout back onto the reference-layout tensor it came from."""
    net = _net(cls, **kw)
    packed = net._pack_tensors()
    packed.update(net._extra_flat_tensors())
    got = net.unpack_grads(packed)
    sd = net.state_dict()
    assert set(got) == set(sd)
    b1 = net.v_layer.bias + net.x_layer.bias + net.t_layer.bias     # the packed bias is their sum
    for k, t in sd.items():
        assert got[k].shape == t.shape and got[k].is_contiguous(), k
        assert torch.equal(got[k], b1 if k in ("v_layer/b", "x_layer/b", "t_layer/b") else t), k
    # each of the three biases owns its gradient tensor (autograd may accumulate into it in place)
    assert len({got[k].data_ptr() for k in ("v_layer/b", "x_layer/b", "t_layer/b")}) == 3


def test_packed_buffers_are_dropped_when_a_weight_moves():
    net = _net(GenericNet, x_dim=32, num_hidden=64, factor=2., links_shape=(4, 4, 2))
    net._check_ref_version()
    net._packed = "built"
    net._check_ref_version()
    assert net._packed == "built"                     # nothing moved
    with torch.no_grad():
        net.h_layer.kernel.add_(1.0)                  # in place, as torch.optim does
    net._check_ref_version()
    assert net._packed is None
    net._packed = "built"
    net.coeff_scale = net.coeff_scale.clone()         # a new tensor object
    net._check_ref_version()
    assert net._packed is None
    net._packed = "built"
    net._flat = ("flat master copy",)                 # a trainer owns the weights: its optimiser re-packs
    with torch.no_grad():
        net.h_layer.kernel.add_(1.0)
    net._check_ref_version()
    assert net._packed == "built"
    # _pack_tensors never aliases a reference tensor: a pending tape keeps the values it ran with
    del net._flat
    ptrs = {t.data_ptr() for t in net._ref_tensors()}
    assert not ptrs & {b.data_ptr() for b in net._pack_tensors().values()}
