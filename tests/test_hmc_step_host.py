"""Host logic around the one-launch plain-HMC kernel (l2hmc_amd/csrc/hmc_step.hip): which plans take it, and that
the workspace queries did not grow.  No GPU: the plans carry any non-NULL address where a pointer is checked."""
import ctypes as C

import pytest

from l2hmc_amd import _lib

PTR = 16          # any non-NULL address: host checks only
SHAPES = [(2, 4), (3, 5), (6, 6), (4, 16), (8, 8), (16, 16), (32, 32)]


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _hmc_plan(T, X, N, flags=0):
    return _lib.GaugePlan(T=T, X=X, num_steps=N, hmc=1, flags=flags, masks=PTR)


def _net(D, H, packed=0):
    w = {k: PTR for k in ("w1_t", "wt", "b1", "wh_t", "bh", "whd_t", "bhd", "coeff_s", "coeff_q")}
    return _lib.DenseNet(D=D, H=H, Ka=D, Kb=D, packed=packed or None, **w)


@pytest.mark.parametrize("N", [1, 10, 25])
@pytest.mark.parametrize("T,X", SHAPES)
def test_hmc_plans_take_the_one_launch_kernel(L, T, X, N):
    assert L.l2hmc_gauge_plan_fused(C.byref(_hmc_plan(T, X, N))) == 1
    assert L.l2hmc_gauge_plan_fused(C.byref(_hmc_plan(T, X, N, _lib.PLAN_SELECTED_ONLY))) == 1
    assert L.l2hmc_gauge_plan_fused(C.byref(_hmc_plan(T, X, N, _lib.PLAN_LAYERED))) == 0


def test_plans_outside_the_kernel_keep_their_answers(L):
    # a chain beyond the kernel's budget (more than 1024 sites: 4 sites per thread x 256 threads per row) is not
    # refused: it keeps the layer-by-layer path
    assert L.l2hmc_gauge_plan_fused(C.byref(_hmc_plan(512, 512, 10))) == 0
    assert L.l2hmc_gauge_plan_fused(C.byref(_hmc_plan(32, 33, 10))) == 0
    assert L.l2hmc_gauge_plan_fused(C.byref(_hmc_plan(8, 8, 0))) < 0
    assert L.l2hmc_gauge_plan_fused(C.byref(_lib.GaugePlan(T=8, X=8, num_steps=10, hmc=1))) < 0      # masks NULL
    # plans with networks: the answers of the commit before the kernel, recorded
    gen, genp, n66 = _net(128, 512), _net(128, 512, packed=PTR), _net(72, 288)
    assert L.l2hmc_gauge_plan_fused(C.byref(_lib.GaugePlan(T=8, X=8, num_steps=10, xnet=gen, vnet=gen, masks=PTR))) == 0
    assert L.l2hmc_gauge_plan_fused(C.byref(_lib.GaugePlan(T=8, X=8, num_steps=10, xnet=genp, vnet=genp, masks=PTR))) == 1
    assert L.l2hmc_gauge_plan_fused(C.byref(_lib.GaugePlan(T=8, X=8, num_steps=10, xnet=genp, vnet=genp, masks=PTR,
                                                           flags=_lib.PLAN_LAYERED))) == 0
    assert L.l2hmc_gauge_plan_fused(C.byref(_lib.GaugePlan(T=6, X=6, num_steps=10, xnet=n66, vnet=n66, masks=PTR))) == 0


# (T, X, N) -> {B: (l2hmc_gauge_mcmc_step_ws_bytes(plan, B), l2hmc_gauge_ws_bytes(plan, 2 B))} of hmc = 1 plans at the
# commit before the kernel; l2hmc_gauge_pack_heads_bytes was 0 for all of them
PARENT_WS = {
    (2, 4, 1): {1: (5504, 2304), 70: (66304, 13568), 2048: (1852160, 344832)},
    (3, 5, 10): {1: (9088, 5632), 70: (120832, 24832), 2048: (3346432, 577536)},
    (6, 6, 10): {1: (20864, 11264), 70: (280064, 54528), 2048: (7857152, 1303552)},
    (4, 16, 25): {1: (47616, 40960), 70: (513024, 115712), 2048: (13866752, 2266880)},
    (8, 8, 10): {1: (35712, 17920), 70: (489984, 92672), 2048: (13843712, 2243840)},
    (16, 16, 10): {1: (140160, 67072), 70: (1940480, 360448), 2048: (54980864, 8777984)},
    (32, 32, 25): {1: (723712, 632576), 70: (8111360, 1800448), 2048: (219898112, 35283200)},
    (512, 512, 10): {1: (142607232, 67241216), 70: (1980504320, 365694208), 2048: (56166056192, 8921350400)},
}


@pytest.mark.parametrize("shape", sorted(PARENT_WS))
def test_hmc_workspace_queries_did_not_grow(L, shape):
    T, X, N = shape
    for flags in (0, _lib.PLAN_LAYERED, _lib.PLAN_SELECTED_ONLY):
        plan = _hmc_plan(T, X, N, flags)
        assert L.l2hmc_gauge_pack_heads_bytes(C.byref(plan)) == 0
        for B, (step_ws, traj_ws) in PARENT_WS[shape].items():
            got = L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B)
            assert 0 < got <= step_ws
            # the one-launch step keeps its per-workgroup partial sums (2 floats for at most B workgroups) in the head
            assert got >= 8 * B
            assert 0 < L.l2hmc_gauge_ws_bytes(C.byref(plan), 2 * B) <= traj_ws
