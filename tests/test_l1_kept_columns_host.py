"""Host side of the kept-column first layer (l2hmc_gauge_pack_heads): the image grows by one (D / 2) x H first-layer
section per (mask row, keep sense) and the column -> compact k map, and only for plans that had an image before.
No GPU: the plans carry any non-NULL address where a pointer is checked."""
import ctypes as C

import pytest

from l2hmc_amd import _lib

PTR = 16          # any non-NULL address: host checks only
D, H = 128, 512


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _net(D, H, Ka=None, packed=PTR):
    w = {k: PTR for k in ("w1_t", "wt", "b1", "wh_t", "bh", "whd_t", "bhd", "coeff_s", "coeff_q")}
    Ka = D if Ka is None else Ka
    return _lib.DenseNet(D=D, H=H, Ka=Ka, Kb=Ka, packed=packed, **w)


def _align(n, a=256):
    return (n + a - 1) // a * a


@pytest.mark.parametrize("N", [1, 3, 10, 25])
@pytest.mark.parametrize("flags", [0, _lib.PLAN_FULL_L1, _lib.PLAN_ALL_COLUMNS, _lib.PLAN_TILES16_ONLY])
def test_image_grows_by_the_first_layer_sections_and_the_map(L, N, flags):
    net = _net(D, H)
    plan = _lib.GaugePlan(T=8, X=8, num_steps=N, xnet=net, vnet=net, masks=PTR, flags=flags)
    # before: eligibility [N][2] and columns [N][2][D / 2] (int), padded to 256 bytes, then the heads sections
    before = _align(4 * (2 * N + N * D)) + 4 * 2 * N * 3 * (D // 2) * H
    # now: the column -> compact k map [N][D] (int) joins the meta block; the first-layer sections follow the heads
    meta = _align(4 * (2 * N + 2 * N * D))
    want = meta + 4 * 2 * N * 3 * (D // 2) * H + 2 * N * (D // 2) * H * 4
    got = L.l2hmc_gauge_pack_heads_bytes(C.byref(plan))
    assert got == want
    assert got - before == 2 * N * (D // 2) * H * 4 + (meta - _align(4 * (2 * N + N * D)))
    assert (got - 2 * N * (D // 2) * H * 4) % 256 == 0        # the first-layer sections start 256-byte aligned


def test_plans_without_an_image_still_have_none(L):
    gen, conv, n66, wide = _net(D, H), _net(128, 256, Ka=64), _net(72, 288), _net(128, 256)
    zero = [
        _lib.GaugePlan(T=8, X=8, num_steps=10, hmc=1, masks=PTR),
        _lib.GaugePlan(T=8, X=8, num_steps=10, hmc=1, xnet=gen, vnet=gen, masks=PTR),
        _lib.GaugePlan(T=8, X=8, num_steps=0, xnet=gen, vnet=gen, masks=PTR),
        _lib.GaugePlan(T=8, X=8, num_steps=10, xnet=conv, vnet=conv, masks=PTR, flags=_lib.PLAN_CONV3D),
        _lib.GaugePlan(T=6, X=6, num_steps=10, xnet=n66, vnet=n66, masks=PTR),
        _lib.GaugePlan(T=8, X=8, num_steps=10, xnet=wide, vnet=wide, masks=PTR),
        _lib.GaugePlan(T=4, X=8, num_steps=10, xnet=gen, vnet=gen, masks=PTR),
    ]
    for plan in zero:
        for extra in (0, _lib.PLAN_FULL_L1):
            plan.flags |= extra
            assert L.l2hmc_gauge_pack_heads_bytes(C.byref(plan)) == 0


def test_switch_is_the_next_free_plan_bit():
    bits = [_lib.PLAN_LAYERED, _lib.PLAN_CONV3D, _lib.PLAN_SELECTED_ONLY, _lib.PLAN_RECOMPUTE, _lib.PLAN_TILES16_ONLY,
            _lib.PLAN_ALL_COLUMNS, _lib.PLAN_FULL_L1]
    assert bits == [1 << i for i in range(7)]
    with open(_lib.HEADER_PATH) as f:
        assert "#define L2HMC_PLAN_FULL_L1 64" in f.read()
