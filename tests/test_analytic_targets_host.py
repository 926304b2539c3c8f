"""Host side of the rough-well and funnel targets (l2hmc_amd/distributions.py: RoughWell, GaussianFunnel) and of the
tilted Gaussians: constructors and refusals, sample streams, the struct they hand to the C ABI, and the host checks of
every entry that takes a target.  No kernel is launched in this file."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import l2hmc_amd as la
from l2hmc_amd import _lib, build as lbuild


@pytest.fixture(scope="module")
def L():
    lbuild.build()
    return _lib.lib()


def test_constructors_and_refusals():
    rw = la.RoughWell(2, 0.1)
    assert (rw.dim, rw.eps, rw.easy) == (2, 0.1, False) and la.RoughWell(8, 0.5, easy=True).easy
    fn = rw.get_energy_function()
    assert callable(fn) and fn.target.dim == 2 and fn.target.K == 1
    f = la.GaussianFunnel()
    assert (f.dim, f.sigma, f.clip) == (2, 2.0, 8.0)
    assert la.GaussianFunnel(3, clip=1.0).clip == 8.0          # the argument is ignored, as in the reference
    assert la.GaussianFunnel(8).get_energy_function().target.dim == 8
    for make in (lambda: la.RoughWell(9, 0.5), lambda: la.GaussianFunnel(9)):
        with pytest.raises(ValueError, match="beyond the fused kernel's limits.*torch callable for the layer-by-layer path"):
            make()
    with pytest.raises(ValueError, match="torch callable for the layer-by-layer path"):
        la.Gaussian(np.zeros(9), np.eye(9)).get_energy_function()
    for dim in (1, 0):
        with pytest.raises(ValueError, match="at least 2"):
            la.GaussianFunnel(dim)
    for eps in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            la.RoughWell(2, eps)


def test_get_samples_shapes_and_streams():
    np.random.seed(3)
    a = la.RoughWell(3, 0.1).get_samples(7)
    np.random.seed(3)
    assert a.shape == (7, 3) and np.array_equal(a, np.random.randn(7, 3))
    assert la.GaussianFunnel(5).get_samples(11).shape == (11, 5)


@pytest.mark.parametrize("dim,n", [(2, 9), (4, 33)])
def test_funnel_samples_follow_the_reference_loop(dim, n):
    """distributions.py:213-220 draws row by row: v's normal, then the row's dim - 1."""
    np.random.seed(12)
    want = np.zeros((n, dim))
    for t in range(n):
        v = 2.0 * np.random.randn()
        want[t, 0] = v
        want[t, 1:] = np.exp(v / 2) * np.random.randn(dim - 1)
    np.random.seed(12)
    got = la.GaussianFunnel(dim).get_samples(n)
    assert np.array_equal(got, want)


def test_tilted_gaussians():
    np.random.seed(5)
    t = la.TiltedGaussian(4, -1., 1.)
    assert np.allclose(t.R @ t.R.T, np.eye(4), atol=1e-12)
    assert np.array_equal(t.diag, np.diag(np.diag(t.diag))) and (np.diag(t.diag) > 0).all()
    assert np.allclose(t.sigma, t.R.T @ t.diag @ t.R, rtol=0, atol=1e-12)
    assert np.allclose(t.i_sigma @ t.sigma, np.eye(4), atol=1e-9)
    assert t.get_samples(7).shape == (7, 4) and t.get_samples(300).shape == (300, 4)     # n is honoured
    fn = t.get_energy_function()
    assert fn.target.dim == 4 and fn.target.K == 1 and fn.target.is_gaussian == _lib.TARGET_GAUSSIAN
    # the samples have the covariance of the energy: x = z sqrt(diag) R
    A = np.sqrt(t.diag) @ t.R
    assert np.allclose(A.T @ A, t.sigma, atol=1e-12)
    g = la.random_tilted_gaussian(3)
    assert isinstance(g, la.Gaussian) and g.sigma.shape == (3, 3) and np.allclose(g.sigma, g.sigma.T)
    w = np.linalg.eigvalsh(g.sigma)
    assert (w > 1e-2 - 1e-9).all() and (w < 1e2 + 1e-3).all() and np.array_equal(g.mu, np.zeros(3))


def test_struct_carries_the_kind_and_the_scalars():
    import torch
    cpu = torch.device("cpu")          # (nothing is allocated for these kinds)
    st = la.RoughWell(3, 0.25, easy=True).get_energy_function().target.to(cpu).struct(2.5)
    assert (st.dim, st.K, st.is_gaussian, st.temperature) == (3, 1, _lib.TARGET_ROUGH_WELL, 2.5)
    assert st.rough_well.eps == 0.25 and st.rough_well.easy == 1 and not st.prec and not st.log_const
    st = la.GaussianFunnel(4).get_energy_function().target.to(cpu).struct()
    assert (st.dim, st.K, st.is_gaussian, st.temperature) == (4, 1, _lib.TARGET_FUNNEL, 1.0)
    # the scalars share the slot of `mu`: same offset, same size, the struct as large as it was
    assert _lib.MogTarget.mu.offset == _lib.MogTarget.rough_well.offset == 16
    assert C.sizeof(_lib.RoughWellParams) == C.sizeof(C.c_void_p) == 8 and C.sizeof(_lib.MogTarget) == 40
    old = _lib.MogTarget(dim=2, K=2, is_gaussian=0, temperature=1.0, mu=4096, prec=16, log_const=32)
    assert (old.mu, old.prec, old.log_const) == (4096, 16, 32)


def test_header_and_ctypes_agree_on_the_target(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "l2hmc_hip.h"\n'
        'int main(void){l2hmc_mog_target t; printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(t),'
        ' offsetof(l2hmc_mog_target, mu), offsetof(l2hmc_mog_target, rough_well), offsetof(l2hmc_mog_target, rough_well.easy),'
        ' offsetof(l2hmc_mog_target, prec), offsetof(l2hmc_mog_target, log_const), sizeof(t.rough_well),'
        ' L2HMC_TARGET_MIXTURE, L2HMC_TARGET_GAUSSIAN, L2HMC_TARGET_ROUGH_WELL, L2HMC_TARGET_FUNNEL, L2HMC_ABI_VERSION);'
        ' return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", str(_lib.HEADER_PATH.rsplit("/", 1)[0]), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    M = _lib.MogTarget
    assert got == [C.sizeof(M), M.mu.offset, M.rough_well.offset, M.rough_well.offset + _lib.RoughWellParams.easy.offset,
                   M.prec.offset, M.log_const.offset, C.sizeof(_lib.RoughWellParams), _lib.TARGET_MIXTURE,
                   _lib.TARGET_GAUSSIAN, _lib.TARGET_ROUGH_WELL, _lib.TARGET_FUNNEL, 1]


def _rw(dim=2, eps=0.5, **kw):
    return _lib.MogTarget(**{**dict(dim=dim, K=1, is_gaussian=_lib.TARGET_ROUGH_WELL, temperature=1.0,
                                    rough_well=_lib.RoughWellParams(eps=eps, easy=0)), **kw})


def _funnel(dim=2, **kw):
    return _lib.MogTarget(**{**dict(dim=dim, K=1, is_gaussian=_lib.TARGET_FUNNEL, temperature=1.0), **kw})


BAD = [(_rw(eps=0.0), b"eps"), (_rw(eps=-1.0), b"eps"), (_rw(eps=float("nan")), b"eps"), (_rw(eps=float("inf")), b"eps"),
       (_rw(K=2), b"K == 1"), (_rw(dim=9), b"dim=9"), (_rw(temperature=0.0), b"temperature"),
       (_funnel(dim=1), b"dim >= 2"), (_funnel(K=3), b"K == 1"),
       (_lib.MogTarget(dim=2, K=1, is_gaussian=4, temperature=1.0, mu=16, prec=16, log_const=16), b"kind 4"),
       (_lib.MogTarget(dim=2, K=1, is_gaussian=-1, temperature=1.0, mu=16, prec=16, log_const=16), b"kind -1")]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_bad_targets_are_refused_before_any_launch(L, i):
    """By the two standalone operators and, as the target of a plan, by trajectory, propose, run, train_step and vjp.
    Every other pointer is a non-NULL dummy that the host code never follows."""
    tgt, word = BAD[i]
    P = 64
    calls = [lambda: L.l2hmc_mog_energy_grad(C.byref(tgt), P, 4, P, P, None),
             lambda: L.l2hmc_mog_energy_hvp(C.byref(tgt), P, P, 4, P, None)]
    net = _lib.DenseNet(D=tgt.dim, H=10, Ka=tgt.dim, Kb=tgt.dim, w1_t=P, wt=P, b1=P, wh_t=P, bh=P, whd_t=P, bhd=P,
                        coeff_s=P, coeff_q=P, q_tanh=1)
    plan = _lib.SmallPlan(x_dim=tgt.dim, num_nodes=10, trajectory_length=3, hmc=0, eps=0.1, masks=P, xnet=net, vnet=net,
                          target=tgt)
    calls += [lambda: L.l2hmc_small_trajectory(C.byref(plan), P, P, None, 4, P, P, P, P, None),
              lambda: L.l2hmc_small_propose(C.byref(plan), P, 4, 1, 0, P, P, P, P, None),
              lambda: L.l2hmc_small_run(C.byref(plan), P, P, 4, 1, 0, 2, P, P, None),
              lambda: L.l2hmc_small_train_step(C.byref(plan), P, P, None, 4, 0.1, 1., P, P, P, P, P, P, 1 << 30, None),
              lambda: L.l2hmc_small_vjp(C.byref(plan), P, P, None, 4, *([None] * 6), P, *([None] * 4), P, 1 << 30, None)]
    for call in calls:
        assert call() == 1
        assert word in L.l2hmc_last_error(), L.l2hmc_last_error()


def test_good_analytic_targets_pass_the_host_checks(L):
    """rows = 0 returns after the checks: NULL mu / prec / log_const are fine for the two new kinds, and still an
    error for the mixture."""
    for tgt in (_rw(eps=0.01), _rw(dim=1), _rw(dim=8), _funnel(), _funnel(dim=8)):
        assert L.l2hmc_mog_energy_grad(C.byref(tgt), None, 0, None, None, None) == 0
        assert L.l2hmc_mog_energy_hvp(C.byref(tgt), None, None, 0, None, None) == 0
    mix = _lib.MogTarget(dim=2, K=2, is_gaussian=0, temperature=1.0)
    assert L.l2hmc_mog_energy_grad(C.byref(mix), None, 0, None, None, None) == 1
    assert b"NULL" in L.l2hmc_last_error()


def test_python_keys_on_the_target_attribute_only():
    """Dynamics, the sampler, the trainer and the autograd route pick the one-launch path from
    `energy_function.target`; none of them looks at the kind."""
    import inspect
    from l2hmc_amd import autograd_toy, dynamics, dynamics_sampler, dynamics_trainer
    for fn in (la.RoughWell(2, 0.5).get_energy_function(), la.GaussianFunnel(3).get_energy_function()):
        assert fn.target.dim in (2, 3) and callable(fn.target.struct) and callable(fn.target.energy_grad)
    for mod in (autograd_toy, dynamics, dynamics_sampler, dynamics_trainer):
        assert "is_gaussian" not in inspect.getsource(mod), mod.__name__
