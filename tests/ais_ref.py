"""Annealed importance sampling (l2hmc/utils/ais.py:30-82) restated in NumPy on the oracle's target classes and the
draws of tests/philox_ref.py, and the cases the host tests (tests/test_ais_host.py) validate and the GPU tests
(tests/test_gpu_ais.py) compare the kernel with.  Nothing here touches the library.

The loop (`anneal`), per chain, for s = 1 .. n with b_0 = 0:
  w += (b_s - b_{s-1}) (E0(x) - E1(x))                       on the state step s - 1 left; w is float64 in every dtype
  v  = N(0, I), or with `refresh` = rho:  v sqrt(1 - rho) + n sqrt(rho),  n ~ N(0, I)
  (Lx, Lv, p) = DynamicsOracle(hmc=True).forward on E_s = (1 - b_s) E0 + b_s E1     (E1 includes 1 / temperature)
  accept iff p - u >= 0: x <- Lx, v <- Lv;  else x stays, v <- -Lv (the PROPOSED momentum negated: ais.py:63)
Streams as l2hmc_small_ais_run takes them: with `refresh` the start v is stream draw0 and the steps start at draw0 + 1;
step s (from 0) takes its normals from elements c * dim + d of the next stream and its uniforms from element c of the
one after.

A Philox seed in a table below is one at which the conditions tests/test_ais_host.py asserts hold."""
import collections
import functools

import numpy as np

from oracle import dynamics as od
from tests import helpers as H
from tests import philox_ref as R
from tests.test_gpu_analytic_targets import FunnelRef, RoughWellRef
from tests.test_gpu_small_hmc_run import GAUSS8_VAR, GMM3, SCG_SIGMA

MASK_SEED = 3                   # tests/test_gpu_small_hmc_run.py::_toy: od.make_masks(N, dim, RandomState(3))


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def default_schedule(n):
    return np.linspace(0., 1., n + 1)[1:].astype(np.float32)


class Interpolated:
    """(1 - b) E0 + b E1 / temperature as a target of DynamicsOracle, in the dtype of x."""

    def __init__(self, E0, E1, temperature, b):
        self.E0, self.E1, self.temperature, self.b = E0, E1, temperature, b

    def parts(self, x):
        dt = x.dtype.type
        return self.E0.energy(x), self.E1.energy(x) / dt(self.temperature)

    def energy(self, x):
        dt = x.dtype.type
        e0, e1 = self.parts(x)
        return (dt(1) - dt(self.b)) * e0 + dt(self.b) * e1

    def grad_energy(self, x):
        dt = x.dtype.type
        return (dt(1) - dt(self.b)) * self.E0.grad_energy(x) + dt(self.b) * (self.E1.grad_energy(x) / dt(self.temperature))


def anneal(E0, E1, temperature, masks, eps, x0, betas, seed, draw0, refresh=None, dtype=np.float64,
           draws=(R.normal, R.uniform)):
    """-> dict: log_w [B] float64, x [B, D], v [B, D] (with `refresh`), px [n, B], accepted [n, B] bool, margin [B]
    (the smallest |p - u| over the steps), draws (the streams taken).  `betas` [n]: b_1 .. b_n as float32 values."""
    dt = np.dtype(dtype).type
    x = np.asarray(x0, dtype=dtype)
    B, D = x.shape
    N = np.asarray(masks).shape[0]
    b = np.concatenate([np.zeros(1, np.float32), np.asarray(betas, dtype=np.float32)])
    n = b.shape[0] - 1
    w = np.zeros(B, dtype=np.float64)
    stream, elems = int(draw0), np.arange(B * D)
    v = None
    if refresh is not None:
        rho = dt(np.float32(refresh))
        keep, mix = np.sqrt(dt(1) - rho), np.sqrt(rho)
        v = np.asarray(draws[0](seed, stream, elems), dtype=dtype).reshape(B, D)
        stream += 1
    px, accepted, margin = np.empty((n, B)), np.empty((n, B), dtype=bool), np.full(B, np.inf)
    for s in range(n):
        tgt = Interpolated(E0, E1, temperature, b[s + 1])
        e0, e1 = tgt.parts(x)
        w += (np.float64(b[s + 1]) - np.float64(b[s])) * (e0.astype(np.float64) - e1.astype(np.float64))
        noise = np.asarray(draws[0](seed, stream, elems), dtype=dtype).reshape(B, D)
        u = np.asarray(draws[1](seed, stream + 1, np.arange(B)), dtype=dtype)
        stream += 2
        v0 = noise if v is None else v * keep + noise * mix
        orc = od.DynamicsOracle(D, tgt, N, eps, masks, hmc=True, dtype=dt)
        Lx, Lv, p = orc.forward(x, v0)
        acc = (p - u) >= 0
        x = np.where(acc[:, None], Lx, x)
        if v is not None:
            v = np.where(acc[:, None], Lv, -Lv)
        px[s], accepted[s] = p, acc
        margin = np.minimum(margin, np.abs(p.astype(np.float64) - u.astype(np.float64)))
    out = dict(log_w=w, x=np.asarray(x, dtype=np.float64), px=px, accepted=accepted, margin=margin,
               draws=stream - int(draw0))
    if v is not None:
        out["v"] = np.asarray(v, dtype=np.float64)
    return out


def estimate(log_w):
    """-> (log_ratio, se, ess): logsumexp(w) - log(B), the delta-method standard error std(w~, ddof=1) / (sqrt(B)
    mean(w~)) and the effective sample size (sum w~)^2 / sum w~^2, with w~ = exp(w - max w); float64."""
    w = np.asarray(log_w, dtype=np.float64)
    wt = np.exp(w - w.max())
    return (float(w.max() + np.log(wt.mean())), float(wt.std(ddof=1) / (np.sqrt(w.size) * wt.mean())),
            float(wt.sum() ** 2 / np.square(wt).sum()))


def log_norm(sigma):
    """0.5 logdet(2 pi Sigma): log of the integral of exp(-0.5 (x - mu)^T Sigma^-1 (x - mu))."""
    return 0.5 * float(np.linalg.slogdet(2 * np.pi * np.asarray(sigma, dtype=np.float64))[1])


# ------------------------------------------------------------------------------------------------- parity cases
# kind -> (dim, temperature of the final target, eps): the kinds of tests/test_gpu_small_hmc_run.py and a final target at
# temperature 3.  The step sizes: large enough that the float64 restatement rejects 3 to 16 % of its proposals (at
# eps = 0.1 every kind accepts more than 97 %, the rough well 99.9 %, and the rejected branch would hardly run), and
# at most HALF the leapfrog stability limit of the final target, eps * sqrt(largest curvature of E1 / temperature) <= 1
# (STIFFNESS below; the limit is 2).  Nearer the limit a trajectory amplifies rounding so much that ONE float32 evaluation
# no longer tells the float32 error: with the rough well at eps = 0.8 (1.39) and the mixture at 0.2 (1.26) the float32
# restatement's largest px error moved by factors of 2 and 3.3 (2.9e-5 .. 5.5e-5, 8.7e-5 .. 2.9e-4) between twelve
# evaluations whose starts differed by one float32 ulp, and the kernel's px at the rough well (9.6e-5) missed a bar
# formed from one of them (1.3e-5); with the rough well at 0.5 (0.87) the twelve lie within 1.4e-6 .. 2.9e-6.
KINDS = {"scg": (2, 1.0, 0.3), "mog": (2, 1.0, 0.15), "gmm3": (3, 1.0, 0.2), "gauss8": (8, 1.0, 0.5),
         "rw": (2, 1.0, 0.5), "funnel": (2, 1.0, 0.4), "scg_T3": (2, 3.0, 0.5)}
# the largest curvature of the final target's energy at temperature 1 where it has one: the largest eigenvalue of a
# precision matrix; 1 + eps / a^2 for the rough well (eps = a = 0.5).  (The funnel's, exp(-v), has no bound)
STIFFNESS = {"scg": 10.0, "mog": 40.0, "gmm3": 20.0, "gauss8": 1 / 0.3, "rw": 3.0, "scg_T3": 10.0}
PARITY_STEPS, PARITY_LF = 8, 5
PARITY_BATCHES = (1, 65, 130)
PARITY_SCHEDULE = np.array([0.05, 0.05, 0.2, 0.45, 0.7, 0.9, 1.0, 1.0], dtype=np.float32)    # uneven, two repeats
REFRESH = 0.1
DRAW0 = 4
# (kind, refresh) -> Philox seed
PARITY_SEEDS = {("scg", False): 9, ("scg", True): 5, ("mog", False): 1, ("mog", True): 5, ("gmm3", False): 9,
                ("gmm3", True): 3, ("gauss8", False): 15, ("gauss8", True): 2, ("rw", False): 13, ("rw", True): 3,
                ("funnel", False): 4, ("funnel", True): 6, ("scg_T3", False): 19, ("scg_T3", True): 3}


def final_oracle(kind):
    if kind.startswith("scg"):
        return od.Gaussian(np.zeros(2), SCG_SIGMA)
    if kind == "mog":
        return H.mog_target_oracle()
    if kind == "gmm3":
        return od.GMM(*GMM3)
    if kind == "gauss8":
        return od.Gaussian(np.linspace(-0.4, 0.4, 8), np.diag(GAUSS8_VAR))
    if kind == "rw":
        return RoughWellRef(0.5, easy=True)
    assert kind == "funnel"
    return FunnelRef()


def final_library(la, kind):
    """The library's object of `final_oracle(kind)`."""
    if kind.startswith("scg"):
        return la.Gaussian(np.zeros(2), SCG_SIGMA)
    if kind == "mog":
        m = H.mog_target_oracle()
        return la.GMM(m.mus, m.sigmas, m.pis)
    if kind == "gmm3":
        return la.GMM(*GMM3)
    if kind == "gauss8":
        return la.Gaussian(np.linspace(-0.4, 0.4, 8), np.diag(GAUSS8_VAR))
    if kind == "rw":
        return la.RoughWell(2, 0.5, easy=True)
    return la.GaussianFunnel(2)


def init_arrays(dim):
    """The init Gaussian of the parity cases: a full covariance (every off-diagonal entry 0.2) and a mean off the
    origin, so that the precision matrix and the mean both show."""
    return np.linspace(-0.2, 0.2, dim), np.eye(dim) + 0.2


def masks(N, dim):
    return od.make_masks(N, dim, np.random.RandomState(MASK_SEED))


@functools.lru_cache(maxsize=None)
def start(dim, B):
    """The first B of 130 float32 rows drawn from the init Gaussian: chain c is the same chain at every batch size."""
    mu, sigma = init_arrays(dim)
    rows = mu + od.Gaussian(mu, sigma).get_samples(130, np.random.default_rng(77 + dim))
    return f32(rows)[:B]


@functools.lru_cache(maxsize=None)
def parity_reference(kind, refresh, B, seed=None):
    """-> (float64 restatement, float32 restatement) of a parity case, computed once and shared; callers leave them
    unchanged."""
    dim, temperature, eps = KINDS[kind]
    mu, sigma = init_arrays(dim)
    seed = PARITY_SEEDS[(kind, refresh)] if seed is None else seed
    args = (od.Gaussian(mu, sigma), final_oracle(kind), temperature, masks(PARITY_LF, dim), eps, start(dim, B),
            PARITY_SCHEDULE, seed, DRAW0)
    return tuple(anneal(*args, refresh=REFRESH if refresh else None, dtype=dt) for dt in (np.float64, np.float32))


# ------------------------------------------------------------------------------------------------- known answers
# name -> (init covariance, final target, exact log(Z1 / Z0), chains, steps, leapfrog steps, eps, Philox seed)
Known = collections.namedtuple("Known", "init_sigma final exact B steps lf eps seed")


def known(name):
    if name == "mixture":                       # cfg 2 from N(0, I): Z1 = 1
        s0 = np.eye(2)
        return Known(s0, H.mog_target_oracle(), -log_norm(s0), 256, 64, 10, 0.1, KNOWN_SEEDS[name])
    if name == "gaussian":                      # the SCG from an init of matching scale (from N(0, I) it is 5 se off)
        s0 = np.array([[30., -20.], [-20., 30.]])
        return Known(s0, od.Gaussian(np.zeros(2), SCG_SIGMA), log_norm(SCG_SIGMA) - log_norm(s0), 256, 64, 10, 0.2,
                     KNOWN_SEEDS[name])
    assert name == "funnel"                     # Z1 = integral of exp(-v^2 / 8) = sqrt(8 pi)
    s0 = np.diag([4.0, 4.0])
    return Known(s0, FunnelRef(), 0.5 * np.log(8 * np.pi) - log_norm(s0), 256, 64, 10, 0.1, KNOWN_SEEDS[name])


KNOWN_SEEDS = {"mixture": 2, "gaussian": 2, "funnel": 3}


def known_start(k):
    rng = np.random.default_rng(11)
    return f32(od.Gaussian(np.zeros(2), k.init_sigma).get_samples(k.B, rng))


@functools.lru_cache(maxsize=None)
def known_reference(name, seed=None):
    """The float64 restatement of a known-answer case -> (its dictionary, log_ratio, se, ess)."""
    k = known(name)
    out = anneal(od.Gaussian(np.zeros(2), k.init_sigma), k.final, 1.0, masks(k.lf, 2), k.eps, known_start(k),
                 default_schedule(k.steps), k.seed if seed is None else seed, 0)
    return (out, *estimate(out["log_w"]))
