"""The corners of the (seed, stream) domain and the cases at which tests/test_philox_domain_host.py (no GPU) and
tests/test_gpu_philox_domain.py run the library's generators: one table for both, so that what the host test shows about
a case (its truncated twins give other draws; the float64 oracle fed the reference draws keeps every accept decision
clear of its uniform) is shown about the case the GPU test runs."""
import collections
import functools

import numpy as np

from tests import helpers as H
from tests import philox_ref as R

SEED_HIGH = 2 ** 64 - 59          # high word all ones
SEED_LOW_ZERO = 2 ** 32           # low word zero, high word 1
SEED_SMALL = 7                    # the control
SEEDS = (SEED_HIGH, SEED_LOW_ZERO, SEED_SMALL)
FILL_STREAMS = (2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 0x0123456789ABCDEF)
FILL_N = 4099

# lattice steps: streams (2^32 - 2, 2^32 - 1); the carry into the high word; streams (2^64 - 2, 2^64 - 1)
STEP_DRAWS = (2 ** 31 - 1, 2 ** 31, 2 ** 63 - 1)
RUN_STEPS = 4
RUN_DRAW0 = (2 ** 31 - 2, 2 ** 63 - RUN_STEPS)          # steps straddle the carry in one launch; the last value taken
EXCHANGE_EVERY, EXCHANGE_ROUNDS = 2, 2
EXCHANGE_DRAW0 = (2 ** 31 - 3, 2 ** 63 - RUN_STEPS - EXCHANGE_ROUNDS)

# toy entries: (draw0, n_steps).  Four streams a step for the L2HMC sampler, two for plain HMC
TOY_PROPOSE_DRAW0 = (2 ** 32 - 2, 2 ** 64 - 4)
TOY_RUN = ((2 ** 32 - 6, 3), (2 ** 64 - 13, 3))
TOY_HMC_RUN = ((2 ** 32 - 3, 3), (2 ** 64 - 7, 3))
TOY_EXCHANGE_STEPS, TOY_EXCHANGE_EVERY = 4, 2            # two rounds
TOY_EXCHANGE_DRAW0 = (2 ** 32 - 5, 2 ** 64 - 1 - 2 * TOY_EXCHANGE_STEPS - TOY_EXCHANGE_STEPS // TOY_EXCHANGE_EVERY)
SWAP_STREAMS = (2 ** 64 - 1, 2 ** 32)

N_LF, EPS, BETA = 2, 0.1, 2.0
MARGIN_GPU = 1e-4                 # the oracle comparisons leave out chains whose |p - u| is below it
MARGIN_HOST = 2e-4                # twice that: device normals differ from the reference ones at the 1e-6 level

# entry: "step" (l2hmc_gauge_mcmc_step) or "draw" (l2hmc_gauge_transition_draw); layered: L2HMC_PLAN_LAYERED;
# x_seed: the rng seed of the start state, one at which the accept condition of the host test holds at every draw
LatticeCase = collections.namedtuple("LatticeCase", "name arch T X B hmc layered both entry x_seed")
LATTICE_CASES = [
    LatticeCase("generic-8x8-subtile", "generic", 8, 8, 3, False, False, True, "step", 3),
    LatticeCase("generic-8x8-16row", "generic", 8, 8, 70, False, False, True, "step", 3),
    LatticeCase("conv3d-8x8", "conv3D", 8, 8, 5, False, False, True, "step", 3),
    LatticeCase("generic-8x8-transition-draw", "generic", 8, 8, 9, False, False, True, "draw", 3),
    LatticeCase("generic-6x6-step-draws", "generic", 6, 6, 9, False, False, True, "step", 3),
    LatticeCase("generic-8x8-layered-step-draws", "generic", 8, 8, 9, False, True, True, "step", 3),
    LatticeCase("hmc-4x4", None, 4, 4, 9, True, False, True, "step", 3),
    LatticeCase("hmc-16x32-two-sites", None, 16, 32, 3, True, False, True, "step", 3),
    LatticeCase("hmc-32x32-four-sites", None, 32, 32, 2, True, False, True, "step", 3),
    LatticeCase("hmc-4x4-selected", None, 4, 4, 9, True, False, False, "step", 3),
    LatticeCase("hmc-16x32-selected", None, 16, 32, 3, True, False, False, "step", 3),
    LatticeCase("hmc-32x32-selected", None, 32, 32, 2, True, False, False, "step", 3),
]


def excluded_cap(B):
    """Chains an oracle comparison may leave out: none where B < 64, at most 2 % elsewhere."""
    return 0 if B < 64 else int(0.02 * B)


@functools.lru_cache(maxsize=None)
def lattice_weights(arch, T, X):
    if arch is None:
        return None, None
    return (H.conv_weights if arch == "conv3D" else H.gauge_weights)(T, X, regime="mild")


def lattice_oracle(c):
    xp, vp = lattice_weights(c.arch, c.T, c.X)
    return H.gauge_oracle(c.T, c.X, N_LF, EPS, xp, vp, hmc=c.hmc, arch=c.arch or "generic")


def lattice_x0(c):
    """The start state [B, 2TX], float32."""
    return np.random.default_rng(c.x_seed).uniform(0, 2 * np.pi, (c.B, 2 * c.T * c.X)).astype(np.float32)


def truncated_seeds(seed):
    """The seeds a generator that drops the key's high word would use instead (none if the seed has no high word)."""
    return [seed & R.M32] if seed >> 32 else []


def truncated_streams(stream):
    return [stream & R.M32] if stream >> 32 else []


def truncated_draws(draw):
    """The step draw indices of a generator that forms 2 * draw in 32 bits (draw & 0x7FFFFFFF), where that differs."""
    return [draw & 0x7FFFFFFF] if draw >> 31 else []
