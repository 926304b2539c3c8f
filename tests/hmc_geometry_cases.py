"""Cases for the one-launch plain-HMC kernels (l2hmc_amd/csrc/hmc_step.hip) in every thread-geometry class, in one
place for tests/test_hmc_geometry_host.py (which validates them without a GPU) and tests/test_gpu_hmc_geometry.py
(which compares the kernels with the float64 oracle on them).  Nothing here touches the library.

The rule.  `geom(T, X)` restates the host rule `hmc_geom` by which every entry of the family maps a row (chain x
direction) onto threads: `spt` sites per thread, `2^tsh` threads per row, `R` rows per workgroup, and `ragged` where some
lanes of a row own no site.  A class is a `(spt, tsh, ragged)`.

The inputs.  At the parameters of the older step tests (uniform start, eps 0.1) every chain of the float64 reference
accepts with p on its clipped branch, so the reject branch and the sign of the energy error are never compared.  The
cases here start near the ordered state (links N(0, START^2), wrapped, float32-representable) and take a step size at
which the reference accepts some chains and rejects others; `(eps, draw)` of a case is one at which the conditions of
tests/test_hmc_geometry_host.py hold at BOTH of its batch sizes (found by a scan of eps in steps of 0.02 and of the
draw index from 5 upwards; they are conditions on the committed numbers, asserted there, not measurements).

The batches.  A class has R / 2 chains per workgroup with both directions and R with the selected direction only.  A
case carries a batch for each: a whole number of workgroups and one chain more, so that the last workgroup is partial
(with one chain per workgroup, an odd batch, which leaves the selected-only launch a half-filled workgroup).  On the
lattices of at most 16 sites (TINY_SITES) the batch is one workgroup and a chain, at most 130 chains: the selected-only
batch of 1x1 is a partial workgroup alone, and its paired batch is the full-and-partial one.  Elsewhere a batch has at
most 16 chains."""
import collections

import numpy as np

N_LF = 3
SEED = 77
START = 0.7                # links N(0, 0.7^2) around the ordered state, wrapped
MARGIN = 1e-3              # min |p - u| over ALL chains of a case: no chain is left out of any comparison
MAX_SITES = 1024
TINY_SITES, TINY_BATCH, BATCH = 16, 130, 16


def geom(T, X):
    """-> (spt, tsh, threads, R, ragged) of a T x X lattice, 1 <= T * X <= 1024 (hmc_geom in hmc_step.hip)."""
    sites = T * X
    if T < 1 or X < 1 or sites > MAX_SITES:
        raise ValueError(f"{T}x{X}: no one-launch kernel")
    spt = 1 if sites <= 256 else 2 if sites <= 512 else 4
    per = -(-sites // spt)
    tsh = (per - 1).bit_length()                 # ceil(log2(per))
    threads = 512 if tsh == 8 else 256
    return spt, tsh, threads, threads >> tsh, sites != spt << tsh


def chains_per_workgroup(T, X, both):
    R = geom(T, X)[3]
    return R // 2 if both else R


# mixed: False where the conditions on accepts, rejects and interior p cannot hold and the case is exempt from them
# (1x1: P = x0 - x1 - x0 + x1 = 0 on every configuration, the force vanishes, H is conserved and every chain accepts
# with p = 1); the margin holds for it like for every other case
Case = collections.namedtuple("Case", "T X B B_sel eps beta start draw mixed")


def _c(T, X, B, B_sel, eps, draw=5, beta=2.0, mixed=True):
    return Case(T, X, B, B_sel, eps, beta, START, draw, mixed)


# T, X, B (both directions), B (selected only), eps, draw      # geom(T, X)
CASES = [
    _c(1, 1, 129, 130, 0.3, mixed=False),   # (1, 0, 256, 256, False): exempt, every chain accepts
    _c(1, 2, 65, 129, 0.3),                 # (1, 1, 256, 128, False)
    _c(2, 2, 33, 65, 0.32),                 # (1, 2, 256, 64, False)
    _c(1, 3, 33, 65, 0.34),                 # (1, 2, 256, 64, True)
    _c(2, 4, 17, 33, 0.32),                 # (1, 3, 256, 32, False)
    _c(2, 3, 17, 33, 0.36),                 # (1, 3, 256, 32, True)
    _c(1, 7, 17, 33, 0.32),                 # (1, 3, 256, 32, True)
    _c(5, 3, 9, 17, 0.4),                   # (1, 4, 256, 16, True)
    _c(4, 4, 9, 17, 0.36),                  # (1, 4, 256, 16, False)
    _c(4, 8, 9, 9, 0.34),                   # (1, 5, 256, 8, False)
    _c(5, 5, 9, 9, 0.34),                   # (1, 5, 256, 8, True)
    _c(7, 9, 9, 9, 0.34),                   # (1, 6, 256, 4, True)
    _c(3, 11, 9, 9, 0.4),                   # (1, 6, 256, 4, True)
    _c(11, 3, 9, 9, 0.38),                  # (1, 6, 256, 4, True)
    _c(64, 1, 9, 9, 0.46),                  # (1, 6, 256, 4, False)
    _c(2, 32, 9, 9, 0.34),                  # (1, 6, 256, 4, False)
    _c(8, 16, 9, 9, 0.32),                  # (1, 7, 256, 2, False)
    _c(16, 8, 9, 9, 0.38),                  # (1, 7, 256, 2, False)
    _c(10, 10, 9, 9, 0.38),                 # (1, 7, 256, 2, True)
    _c(9, 9, 9, 9, 0.36),                   # (1, 7, 256, 2, True)
    _c(12, 12, 9, 9, 0.38),                 # (1, 8, 512, 2, True)
    _c(15, 17, 9, 9, 0.38),                 # (1, 8, 512, 2, True)
    _c(16, 16, 9, 9, 0.4),                  # (1, 8, 512, 2, False)
    _c(16, 32, 9, 9, 0.4, draw=6),          # (2, 8, 512, 2, False)
    _c(17, 17, 9, 9, 0.38),                 # (2, 8, 512, 2, True)
    _c(20, 20, 9, 9, 0.42),                 # (2, 8, 512, 2, True)
    _c(1, 257, 9, 9, 0.4),                  # (2, 8, 512, 2, True)
    _c(257, 1, 9, 9, 0.4),                  # (2, 8, 512, 2, True)
    _c(19, 27, 9, 9, 0.38),                 # (4, 8, 512, 2, True)
    _c(24, 24, 9, 9, 0.38),                 # (4, 8, 512, 2, True)
    _c(31, 33, 9, 9, 0.4),                  # (4, 8, 512, 2, True)
    _c(32, 32, 9, 9, 0.4, draw=6),          # (4, 8, 512, 2, False)
]


def case_id(c):
    return f"{c.T}x{c.X}"


def batch(c, both):
    return c.B if both else c.B_sel


def start(c, B):
    """[B, 2 T X] float32 in [0, 6.283]: every value is its own wrap, so a rejected chain returns these very bits."""
    rng = np.random.default_rng(1000 * c.T + c.X)
    x = np.mod(rng.normal(0.0, c.start, (B, 2 * c.T * c.X)), 2 * np.pi).astype(np.float32)
    x[x > np.float32(6.283)] = 0.0
    return x


def oracle(c, dtype=np.float64):
    from tests import helpers as H
    return H.gauge_oracle(c.T, c.X, N_LF, c.eps, None, None, hmc=True, dtype=dtype)


def figures(p, u):
    """What the conditions are stated on: accepts (p > u, strict), rejects, chains with p inside (0.02, 0.98) and the
    smallest |p - u|."""
    p, u = np.asarray(p, dtype=np.float64), np.asarray(u, dtype=np.float64)
    return dict(accepted=int((p > u).sum()), rejected=int((p <= u).sum()),
                interior=int(((p > 0.02) & (p < 0.98)).sum()), margin=float(np.abs(p - u).min()))


def conditions_hold(c, f):
    """The conditions of a case on `figures`: 2 accepts and 2 rejects or more, 2 chains with p inside (0.02, 0.98) (1
    above 512 sites, where dH is extensive and p is nearly 0 or 1), and the margin on every chain."""
    if f["margin"] < MARGIN:
        return False
    if not c.mixed:
        return True
    need = 1 if c.T * c.X > 512 else 2
    return f["accepted"] >= 2 and f["rejected"] >= 2 and f["interior"] >= need


def reference_figures(c, B):
    """`figures` of the float64 oracle on the reference Philox draws of the case at batch B."""
    from tests import philox_ref
    v0f, v0b, coin, u = philox_ref.lattice_step(SEED, c.draw, B, 2 * c.T * c.X)
    p = oracle(c).apply_transition(start(c, B).astype(np.float64), c.beta, v0f, v0b, coin, u)[2]
    return figures(p, u)


def class_of(c):
    spt, tsh, _, _, ragged = geom(c.T, c.X)
    return spt, tsh, ragged


def equality_cases():
    """One full and one ragged case per (spt, tsh): the first of each class in the table."""
    seen, out = set(), []
    for c in CASES:
        k = class_of(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def exchange_group(T, X, both):
    """The replica group of the exchange test of a lattice: the first of 3, 2, 4 whose workgroup of lcm(G, cpw0) chains
    fits 1024 threads and 64 KiB of LDS (3: a workgroup size that is no power of two), or None where none is served
    (four sites per thread: no instance)."""
    import math
    spt, tsh, _, R, _ = geom(T, X)
    if spt > 2:
        return None
    rpc = 2 if both else 1
    for G in (3, 2, 4):
        rows = math.lcm(G, R // rpc) * rpc
        if rows << tsh <= 1024 and 4 * (rows * (5 * T * X + 18) + 512) <= 64 * 1024:
            return G
    return None
