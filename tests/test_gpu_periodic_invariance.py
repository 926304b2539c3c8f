"""The torus-exact L2HMC mode leaves the finite-volume distribution of the 2-D U(1) lattice invariant.

tests/test_gpu_invariance.py excludes lattice L2HMC: under reference quirk Q10 the reference's proposal
does not commute with 2 pi shifts and its wrapped chain is not reversible.  `GaugeDynamics(periodic=True)` is: with the
method and the constants of that file (exact finite-volume starts of tests/invariance.py, checkpoints 1, 4, 16,
max |z| < 5 over the average plaquette, the action, its square and Q^2), periodic L2HMC steps through
`GaugeSampler.step` and through `dyn(x, beta)` followed by the wrap must pass.  The networks have to act: the mean
|sumlogdet| of a trajectory above LOGDET_FLOOR and the acceptance inside ACCEPT_RANGE are asserted conditions
("mild" weights of tests/helpers.REGIMES; the "stress" ones accept below 0.1 at these step sizes).

The same cases run with periodic=False (reference-mode nets of the same regime, seed and masks) are measured and
printed, not asserted on: a lightly trained reference sampler is known to stay near exact.

Measured on the MI355X, max |z| (accept of step 1, mean |sumlogdet|); both paths give the same numbers, and the file
runs in about 5 s:
  2x4:  periodic 1.50 (0.522, 0.718);  reference mode 19.81 (0.089, 2.638).
  6x6:  periodic 2.72 (0.485, 0.411);  reference mode 2.49 (0.001, 1.147): its chains hardly move in 16 steps."""
import time

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import invariance as I
from tests import periodic_ref as PR
from tests.test_gpu_invariance import ACCEPT_RANGE, CHECKPOINTS, LOGDET_FLOOR, Z_PASS, _action64, _report

pytestmark = pytest.mark.gpu

# (T, X, beta, chains, num_steps, eps)
LATTICES = {"2x4": (2, 4, 1.0, 1 << 16, 5, 0.3), "6x6": (6, 6, 3.0, 1 << 14, 4, 0.1)}
_START = {}


def _start(name):
    T, X, beta, B = LATTICES[name][:4]
    if name not in _START:
        _START[name] = (I.u1_samples(B, T, X, beta, np.random.default_rng(17)), I.u1_exact_vector(T, X, beta))
    return _START[name]


def _dyn(name, periodic):
    from l2hmc_amd import GaugeLattice, GaugeDynamics
    T, X, beta, B, N, eps = LATTICES[name]
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=eps, num_steps=N, eps_trainable=False,
                        network_arch='generic', periodic=periodic, seed=5)
    dyn.set_masks(PR.masks_for(N, 2 * T * X, seed=3))
    xp, vp = PR.periodic_weights(T, X, regime="mild") if periodic else H.gauge_weights(T, X, regime="mild")
    dyn.position_fn.load_state(xp)
    dyn.momentum_fn.load_state(vp)
    return dyn


def _run(name, periodic, path):
    """-> (z [checkpoints, J], accept rate of step 1, mean |sumlogdet| of both directions at the start)."""
    from l2hmc_amd import GaugeSampler
    T, X, beta = LATTICES[name][:3]
    dyn = _dyn(name, periodic)
    sampler = GaugeSampler(dyn)
    x0, want = _start(name)
    x = torch.as_tensor(x0, dtype=torch.float32, device="cuda")
    ld = 0.5 * sum(float(dyn.transition_kernel(x, beta, forward=f, return_logdet=True)[3].abs().mean())
                   for f in (True, False))
    zs, acc = [], None
    for k in range(1, max(CHECKPOINTS) + 1):
        if path == "sampler_step":
            x, px, _, _ = sampler.step(x, beta)
        else:
            _, _, px, x_out = dyn(x, beta)
            x = sampler.wrap(x_out)
        if acc is None:
            acc = float(px.double().mean())
        if k in CHECKPOINTS:
            a, p, q = _action64(x, T, X)
            zs.append(I.zscores(I.u1_features(p.cpu().numpy(), a.cpu().numpy(), q.cpu().numpy()), want))
    assert float(x.min()) >= 0 and float(x.max()) <= 2 * np.pi     # the chain state stays wrapped
    return np.array(zs), acc, ld


@pytest.mark.parametrize("path", ["sampler_step", "call_and_wrap"])
@pytest.mark.parametrize("name", list(LATTICES))
def test_periodic_l2hmc_leaves_the_finite_volume_distribution_invariant(name, path):
    t0 = time.time()
    zs, acc, ld = _run(name, True, path)
    m = _report(f"U(1) periodic L2HMC {name} {path}", zs, f"accept {acc:.3f} |logdet| {ld:.3f} {time.time() - t0:.1f} s")
    assert ld > LOGDET_FLOOR, ld
    assert ACCEPT_RANGE[0] < acc < ACCEPT_RANGE[1], acc
    assert m < Z_PASS, zs
    # the reference mode on the same cases: recorded in the module docstring, not asserted on
    t0 = time.time()
    zr, accr, ldr = _run(name, False, path)
    _report(f"U(1) reference-mode L2HMC {name} {path}", zr, f"accept {accr:.3f} |logdet| {ldr:.3f} {time.time() - t0:.1f} s")
