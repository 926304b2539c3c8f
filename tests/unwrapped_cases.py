"""Inputs, float64 references and bars of tests/test_gpu_unwrapped_links.py: links far outside [0, 2 pi), on both sides of
the switch of `fast_sincos` (csrc/common.h: the Cody-Waite polynomial below |x| = 8192, libm's sincosf from there on).
Importable without a GPU; tests/test_nonfinite_host.py proves the conditions.

Inputs on a grid.  Every link is an integer multiple of 2^-10 with |x| <= 4096, so every plaquette
P = x0 - x1 - x0' + x1' is exact in float32 however the four terms are grouped (|partial sum| <= 2^14 is at most 2^24
grid steps): the device and float64 see the SAME P, and the only error left in a stencil output is sin, cos and the
float32 operations behind them.  Classes of magnitude: |x| <= 8 (negative links and links beyond 2 pi), |x| <= 1024
(polynomial path only, quadrant counts in the thousands), |x| <= 4096 (both paths: 1 / 12 of uniform plaquettes has
|P| >= 8192).  The last chain of every batch is constructed: its plaquettes include exactly +-8192 (the first arguments
of the libm path) and +-(8192 - 2^-11) (the last float32 of the polynomial path; link 4096 - 2^-11 is off the grid and
still exact).  Links are re-drawn until no plaquette lies within 1e-2 of the branch cut of the charge's projection.

Bars.  DELTA = 2e-7 per sine or cosine is what common.h states for fast_sincos (a plain-C model of the polynomial path
measures 9.3e-8 over 1.4e8 arguments); E = 2^-24 bounds the relative rounding error of one float32 operation.  Each
bar below is DELTA and the output's own float32 operations, written out where it is defined."""
import functools

import numpy as np

from oracle import lattice as olat

GRID = 2.0 ** -10
SWITCH = 8192.0
DELTA = 2e-7
E = 2.0 ** -24
C2PI = abs(float(np.float32(2 * np.pi)) - 2 * np.pi)      # what the float32 constant 2 pi is off by: 1.75e-7
CLASSES = {"small": 8.0, "poly": 1024.0, "both": 4096.0}
LATTICES = [(8, 8), (6, 6), (3, 5)]
ROWS = 12                                                  # eleven random chains and the constructed one
CUT_MARGIN = 1e-2
BETA = 2.5
# the four sites of the constructed chain and their (x0, x1): none is the (i, j + 1) or (i + 1, j) of another
EDGE_SITES = (((0, 0), (4096.0, -4096.0)), ((0, 2), (-4096.0, 4096.0)),
              ((1, 1), (4096.0 - 2.0 ** -11, -4096.0)), ((1, 3), (-4096.0 + 2.0 ** -11, 4096.0)))
EDGE_PLAQUETTES = (SWITCH, -SWITCH, SWITCH - 2.0 ** -11, -SWITCH + 2.0 ** -11)


def cut_distance(P):
    """Distance of a plaquette from the branch cut of project_angle (P = pi mod 2 pi)."""
    return np.abs(olat.project_angle(np.asarray(P, dtype=np.float64) + np.pi))


def constructed(T, X):
    x = np.zeros((T, X, 2))
    for (i, j), (a, b) in EDGE_SITES:
        x[i, j] = (a, b)
    return x.reshape(-1)


@functools.lru_cache(maxsize=None)
def links(T, X, cls, rows=ROWS, seed=0, edge=True):
    """[rows, 2 T X] float32 on the grid, |x| <= CLASSES[cls]; the last row is `constructed` (class "both" only)."""
    M = CLASSES[cls]
    rng = np.random.default_rng(1000 * T + 10 * X + int(M) + seed)
    n = int(M / GRID)
    x = rng.integers(-n, n + 1, (rows, 2 * T * X)).astype(np.float64) * GRID
    if edge and cls == "both":
        x[-1] = constructed(T, X)
    for _ in range(1000):
        near = cut_distance(olat.plaq_sums(x, T, X)) < CUT_MARGIN
        near[-1] &= not (edge and cls == "both")
        if not near.any():
            break
        for b, i, j in zip(*np.nonzero(near)):
            x[b, 2 * (i * X + j)] = rng.integers(-n, n + 1) * GRID
    else:
        raise AssertionError("no start off the branch cut found")
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    x32.setflags(write=False)
    return x32


def tangent(T, X, rows=ROWS):
    u = np.random.default_rng(7 * T + X).standard_normal((rows, 2 * T * X)).astype(np.float32)
    u.setflags(write=False)
    return u


def exact_sincos(P):
    return np.sin(P), np.cos(P)


def wrong_from_the_switch_on(P):
    """sin = cos = 0 for |P| >= 8192: a libm branch that returns nothing."""
    s, c = exact_sincos(P)
    far = np.abs(P) >= SWITCH
    return np.where(far, 0.0, s), np.where(far, 0.0, c)


def wrong_below_the_switch(P):
    """sin = cos = 0 for 4096 <= |P| < 8192: a guard moved to 4096 with nothing behind it."""
    s, c = exact_sincos(P)
    mid = (np.abs(P) >= SWITCH / 2) & (np.abs(P) < SWITCH)
    return np.where(mid, 0.0, s), np.where(mid, 0.0, c)


def _stencil(sp):
    """The force's stencil on a per-plaquette field [B, T, X] -> [B, 2 T X] (oracle/lattice.py::grad_action)."""
    g = np.empty(sp.shape + (2,), dtype=sp.dtype)
    g[..., 0] = sp - np.roll(sp, 1, axis=2)
    g[..., 1] = -sp + np.roll(sp, 1, axis=1)
    return g.reshape(g.shape[0], -1)


def reference(x, u, T, X, beta=BETA, sincos=exact_sincos):
    """float64 on the float32 inputs: action, force = beta dS/dx, avg_plaq, top_charge, hvp = d(force)/dx . u."""
    x = np.asarray(x, dtype=np.float64)
    P = olat.plaq_sums(x, T, X)
    s, c = sincos(P)
    w = olat.plaq_sums(np.asarray(u, dtype=np.float64), T, X)
    return dict(action=np.sum(1.0 - c, axis=(1, 2)), force=beta * _stencil(s), avg_plaq=np.sum(c, axis=(1, 2)) / (T * X),
                top_charge=np.sum(olat.project_angle(P), axis=(1, 2)) / (2 * np.pi), hvp=beta * _stencil(c * w))


def bars(x, u, T, X, beta=BETA):
    """Absolute bars per output (scalars, or one per chain)."""
    sites = T * X
    x = np.asarray(x, dtype=np.float64)
    P = olat.plaq_sums(x, T, X)
    # force_k = beta * (sin Pa - sin Pb): two sines, DELTA each; the difference (at most 2) rounds by 2 E; the product by
    # beta (at most 2 beta) rounds by 2 beta E
    force = beta * (2 * DELTA + 2 * E) + 2 * beta * E
    # action = sum of `sites` terms 1 - cos P: DELTA and the rounding of a term (at most 2) each, then sites - 1 float32
    # additions of partial sums of at most 2 sites, in any order
    action = sites * (DELTA + 2 * E) + (sites - 1) * E * 2 * sites
    # avg_plaq = (sum cos P) / sites: DELTA per term, sites - 1 additions of partial sums of at most `sites`, one division
    avg_plaq = (sites * DELTA + (sites - 1) * E * sites) / sites + E
    # top_charge = sum (P - 2pi_f32 * n) / 2 pi, n = floor((P + pi) / 2 pi): no sine in it.  Per plaquette the float32
    # constant is off by C2PI per turn, the product 2 pi n rounds by 2 pi |n| E (nothing, if contracted into an fma), the
    # difference (at most pi) by pi E; then sites - 1 additions of partial sums of at most pi sites and the division
    n = np.abs(np.floor((P + np.pi) / (2 * np.pi)))
    per = n * C2PI + 2 * np.pi * n * E + np.pi * E
    q = np.abs(np.sum(olat.project_angle(P), axis=(1, 2)) / (2 * np.pi))
    top_charge = (per.sum(axis=(1, 2)) + (sites - 1) * E * sites * np.pi) / (2 * np.pi) + 2 * E * q
    # hvp_k = beta * (cos Pa wa - cos Pb wb), w = u0 - u1 - u0' + u1' (three additions: 3 E on the sum of the four |u|):
    # a term is off by DELTA |w| + 3 E sum|u| + E |w| (its product), the difference (at most 2 W) rounds by 2 W E, the
    # product by beta likewise
    au = np.abs(np.asarray(u, dtype=np.float64)).reshape(-1, T, X, 2)
    a0, a1 = au[..., 0], au[..., 1]
    usum = float((a0 + a1 + np.roll(a0, -1, axis=2) + np.roll(a1, -1, axis=1)).max())
    W = float(np.abs(olat.plaq_sums(np.asarray(u, dtype=np.float64), T, X)).max())
    hvp = beta * (2 * (DELTA * W + 3 * E * usum + E * W) + 2 * W * E) + 2 * W * beta * E
    return dict(action=action, force=force, avg_plaq=avg_plaq, top_charge=top_charge, hvp=hvp)


def path_fractions(x, T, X):
    """(fraction of plaquettes on the polynomial path, on the libm path)."""
    P = np.abs(olat.plaq_sums(np.asarray(x, dtype=np.float64), T, X))
    return float((P < SWITCH).mean()), float((P >= SWITCH).mean())


# ---- one-launch kernels: an N = 1 plain-HMC transition from a grid start -------------------------------------------------
HMC_LATTICES = [(8, 8), (16, 32), (32, 32)]               # one, two and four sites per thread (tests/hmc_geometry_cases.py)
HMC_ROWS, HMC_EPS, HMC_BETA = 9, 0.1, 2.0


def hmc_inputs(T, X, cls):
    """(x, v0f, v0b, coin, u) float32: a grid start and injected draws."""
    x = links(T, X, cls, rows=HMC_ROWS, seed=1, edge=False)
    rng = np.random.default_rng(T + X)
    D = 2 * T * X
    v0f, v0b = rng.standard_normal((HMC_ROWS, D)), rng.standard_normal((HMC_ROWS, D))
    coin, u = rng.uniform(size=HMC_ROWS), rng.uniform(size=HMC_ROWS)
    return (x, *(np.asarray(a, dtype=np.float32) for a in (v0f, v0b, coin, u)))


def hmc_n1(x, v, T, X, beta=HMC_BETA, eps=HMC_EPS, sincos=exact_sincos):
    """One plain leapfrog step forward in float64 with a pluggable sin / cos -> (x', v', p): what
    GaugeDynamicsOracle(hmc=True, num_steps=1).transition_kernel computes (shown by the host test)."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    eps = float(np.float32(eps))

    def force_action(y):
        s, c = sincos(olat.plaq_sums(y, T, X))
        return beta * _stencil(s), np.sum(1.0 - c, axis=(1, 2))
    f0, a0 = force_action(x)
    v1 = v - 0.5 * eps * f0
    x1 = x + eps * v1
    f1, a1 = force_action(x1)
    v2 = v1 - 0.5 * eps * f1
    dh = beta * (a0 - a1) + 0.5 * ((v ** 2).sum(1) - (v2 ** 2).sum(1))
    return x1, v2, np.exp(np.minimum(dh, 0.0))


def ulp(a):
    """Spacing of float32 at max |a|."""
    return float(np.spacing(np.float32(np.abs(a).max())))


def bar_x_prop(x_prop, v, beta=HMC_BETA, eps=HMC_EPS):
    """x' = x + eps v1, v1 = v - eps / 2 F(x): one rounding of the sum (half an ulp of the result) on top of eps times what
    v1 is off by: eps / 2 times the force's bar and four roundings of numbers of at most max |v| + eps beta."""
    vmax = float(np.abs(v).max()) + eps * beta
    force = beta * (2 * DELTA + 2 * E) + 2 * beta * E
    return 0.5 * ulp(x_prop) + eps * (0.5 * eps * force + 4 * E * vmax)


# ---- the torus-exact whole-step kernel: an N = 1 transition at 8x8 from the same grid starts ---------------------------
def torus_references(sincos=exact_sincos):
    """(float64, float32) references of tests/periodic_ref.py at 8x8, N = 1, "mild" weights, with a pluggable sin / cos of
    the PLAQUETTES (action and force; the links themselves stay below the switch, |x| <= 4096).  Weights, masks and eps
    as tests/test_gpu_periodic.py builds them for the device."""
    from tests import periodic_ref as PR

    class Ref(PR.NumpyPeriodic):
        def action(self, x):
            return np.sum(1 - sincos(self.plaq(x))[1], axis=(1, 2))

        def force(self, x):
            sp = sincos(self.plaq(x))[0]
            return np.stack([sp - np.roll(sp, 1, 2), -sp + np.roll(sp, 1, 1)], axis=-1).reshape(x.shape[0], -1)

    T = X = 8
    xp, vp = PR.periodic_weights(T, X, regime="mild")
    xp = {k: np.asarray(v, dtype=np.float32) for k, v in xp.items()}
    vp = {k: np.asarray(v, dtype=np.float32) for k, v in vp.items()}
    args = (T, X, 1, float(np.float32(HMC_EPS)), PR.masks_for(1, 2 * T * X), xp, vp)
    return Ref(*args, np.float64), Ref(*args, np.float32)


def bar_x_angle(x, x_prop, e32, max_ratio):
    """x_prop of the torus-exact kernel, by angle: half an ulp of max |x| for the one rounding of the result, and the ratio
    of tests/test_gpu_parity.py over the float32 reference's own angular error e32 for the rest; no absolute floor."""
    return 0.5 * max(ulp(x), ulp(x_prop)) + max_ratio * e32
