"""Toy targets with the reference's class surface (l2hmc/utils/distributions.py:
quadratic_gaussian :32-39, random_tilted_gaussian :47-54, Gaussian :56-80, TiltedGaussian :82-98, RoughWell :101-121,
GMM :124-181, GaussianFunnel :184-228, gen_ring :231-243).
Parameters live on the host as in the reference; `get_energy_function()` returns
a callable that evaluates on the device through l2hmc_mog_energy_grad and
carries the packed parameters (`.target`) so that Dynamics can hand them to the
fused trajectory kernel."""
import collections
import ctypes as C

import numpy as np
import torch
from scipy.stats import ortho_group

from . import _lib

_LAYERED_HINT = "pass the energy as a torch callable for the layer-by-layer path"


class _PackedTarget:
    def __init__(self, mus, precs, log_consts, is_gaussian, device=None):
        self.K, self.dim = len(mus), int(np.asarray(mus[0]).shape[0])
        if self.dim > _lib.MAX_SMALL_DIM or self.K > _lib.MAX_MIX:
            raise ValueError(f"target: dim={self.dim} / K={self.K} beyond the fused kernel's limits "
                             f"({_lib.MAX_SMALL_DIM}, {_lib.MAX_MIX}). To go beyond them, {_LAYERED_HINT}.")
        self.is_gaussian = int(is_gaussian)
        self._host = (np.stack([np.asarray(m, dtype=np.float32) for m in mus]),
                      np.stack([np.asarray(p, dtype=np.float32) for p in precs]),
                      np.asarray(log_consts, dtype=np.float32))
        self.device = None
        if device is not None:
            self.to(device)

    def to(self, device):
        """Parameters onto `device` (done on first use with the current CUDA device when nobody asked earlier)."""
        if self.device != device:
            self.device = device
            self.mu, self.prec, self.log_const = (_lib.as_dev(a, device) for a in self._host)
        return self

    def struct(self, temperature=1.0):
        if self.device is None:
            self.to(torch.device("cuda", torch.cuda.current_device()))
        return _lib.MogTarget(dim=self.dim, K=self.K, is_gaussian=self.is_gaussian,
                              temperature=float(temperature), mu=self.mu.data_ptr(),
                              prec=self.prec.data_ptr(), log_const=self.log_const.data_ptr())

    def energy_grad(self, x, temperature=1.0, want_grad=True):
        if self.device is None:
            self.to(torch.device("cuda", torch.cuda.current_device()))
        x = _lib.as_dev(x, self.device).reshape(-1, self.dim)
        e = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        g = torch.empty_like(x) if want_grad else None
        st = self.struct(temperature)
        _lib.call("l2hmc_mog_energy_grad", C.byref(st), x, x.shape[0], e, g, device=x.device)
        return e, g


class _AnalyticTarget(_PackedTarget):
    """A target kind without parameter arrays (rough well, funnel): the struct carries all there is."""

    def __init__(self, dim, kind, eps=0.0, easy=False):
        self.K, self.dim = 1, int(dim)
        if self.dim > _lib.MAX_SMALL_DIM:
            raise ValueError(f"target: dim={self.dim} / K={self.K} beyond the fused kernel's limits "
                             f"({_lib.MAX_SMALL_DIM}, {_lib.MAX_MIX}). To go beyond them, {_LAYERED_HINT}.")
        self.is_gaussian = int(kind)
        self._rough_well = _lib.RoughWellParams(eps=float(eps), easy=int(bool(easy)))
        self.device = None

    def to(self, device):
        self.device = device
        return self

    def struct(self, temperature=1.0):
        if self.device is None:
            self.to(torch.device("cuda", torch.cuda.current_device()))
        return _lib.MogTarget(dim=self.dim, K=1, is_gaussian=self.is_gaussian, temperature=float(temperature),
                              rough_well=self._rough_well, prec=None, log_const=None)


def _energy_fn(target):
    def fn(x, *args, **kwargs):
        return target.energy_grad(x, want_grad=False)[0]
    fn.target = target
    return fn


def quadratic_gaussian(x, mu, S):
    """:32-39 -- 0.5 (x-mu) S (x-mu)^T per row (the reference takes the diagonal of a BxB product)."""
    t = _PackedTarget([np.asarray(mu)], [np.asarray(S)], [0.], True)
    return t.energy_grad(x, want_grad=False)[0]


class Gaussian(object):
    """:56-80."""

    def __init__(self, mu, sigma):
        self.mu = np.asarray(mu)
        self.sigma = np.asarray(sigma)
        self.i_sigma = np.linalg.inv(np.copy(self.sigma))

    def get_energy_function(self):
        return _energy_fn(_PackedTarget([self.mu.astype('float32')], [self.i_sigma.astype('float32')], [0.], True))

    def get_samples(self, n):
        C_ = np.linalg.cholesky(self.sigma)
        X = np.random.randn(n, self.sigma.shape[0])
        return X.dot(C_.T)


class TiltedGaussian(Gaussian):
    """:82-98.  `get_samples(n)` returns n rows (the reference returns 200 whatever n is: DESIGN.md quirk list)."""

    def __init__(self, dim, log_min, log_max):
        self.R = ortho_group.rvs(dim)
        self.diag = (np.diag(np.exp(np.log(10.) * np.random.uniform(log_min, log_max, size=(dim,))))
                     + 1e-8 * np.eye(dim))
        self.dim = dim
        Gaussian.__init__(self, np.zeros((dim,)), self.R.T.dot(self.diag).dot(self.R))

    def get_samples(self, n):
        X = np.random.randn(n, self.dim)
        return X.dot(np.sqrt(self.diag)).dot(self.R)


def random_tilted_gaussian(dim, log_min=-2., log_max=2.):
    """:47-54."""
    mu = np.zeros((dim,))
    R = ortho_group.rvs(dim)
    sigma = (np.diag(np.exp(np.log(10.) * np.random.uniform(log_min, log_max, size=(dim,))))
             + 1e-6 * np.eye(dim))
    return Gaussian(mu, R.T.dot(sigma).dot(R))


class RoughWell(object):
    """:101-121 -- 0.5 |x|^2 + eps sum_i cos(x_i / a), a = eps^2, or a = eps when `easy`."""

    def __init__(self, dim, eps, easy=False):
        if int(dim) < 1:
            raise ValueError(f"RoughWell: dim={dim} must be positive")
        if not (np.isfinite(eps) and eps > 0):
            raise ValueError(f"RoughWell: eps={eps} must be a finite number > 0")
        self.dim, self.eps, self.easy = int(dim), eps, easy
        self._target = _AnalyticTarget(self.dim, _lib.TARGET_ROUGH_WELL, eps, easy)

    def get_energy_function(self):
        return _energy_fn(self._target)

    def get_samples(self, n):
        return np.random.randn(n, self.dim)


class GaussianFunnel(object):
    """:184-228 -- v = x_0 ~ N(0, sigma^2), x_i ~ N(0, exp(v)); exp(v) is held constant beyond |v| > clip.
    As in the reference, sigma = 2 and clip = 4 sigma = 8 whatever `clip` is given: the argument is accepted and
    ignored (:185-188)."""

    def __init__(self, dim=2, clip=6.):
        if int(dim) < 2:
            raise ValueError(f"GaussianFunnel: dim={dim} must be at least 2 (v and one coordinate it scales)")
        self.dim = int(dim)
        self.sigma = 2.0
        self.clip = 4 * self.sigma
        self._target = _AnalyticTarget(self.dim, _lib.TARGET_FUNNEL)

    def get_energy_function(self):
        return _energy_fn(self._target)

    def get_samples(self, n):
        """The reference's per-row loop (:213-220) draws v's normal, then the row's dim - 1: the order in which
        randn(n, dim) fills its rows, so one call reproduces it under the same np.random.seed."""
        z = np.random.randn(n, self.dim)
        samples = np.empty((n, self.dim))
        samples[:, 0] = self.sigma * z[:, 0]
        samples[:, 1:] = np.exp(samples[:, 0] / 2)[:, None] * z[:, 1:]
        return samples


class GMM(object):
    """:124-181."""

    def __init__(self, mus, sigmas, pis):
        assert len(mus) == len(sigmas)
        if not isinstance(pis, np.ndarray):
            pis = np.array(pis)
        if np.sum(pis) != 1.0:
            pis = pis / pis.sum()
        self.mus, self.sigmas, self.pis = mus, sigmas, pis
        self.nb_mixtures = len(pis)
        self.k = mus[0].shape[0]
        self.i_sigmas, self.constants = [], []
        for i, sigma in enumerate(sigmas):
            self.i_sigmas.append(np.linalg.inv(sigma).astype('float32'))
            det = np.sqrt((2 * np.pi) ** self.k * np.linalg.det(sigma)).astype('float32')
            self.constants.append((pis[i] / det).astype('float32'))

    def get_energy_function(self):
        return _energy_fn(_PackedTarget(self.mus, self.i_sigmas, np.log(np.asarray(self.constants)), False))

    def get_samples(self, n):
        categorical = np.random.choice(self.nb_mixtures, size=(n,), p=self.pis)
        counter_samples = collections.Counter(categorical)
        samples = [np.random.multivariate_normal(self.mus[k], self.sigmas[k], size=(v,))
                   for k, v in counter_samples.items()]
        samples = np.concatenate(samples, axis=0)
        np.random.shuffle(samples)
        return samples


def gen_ring(r=1.0, var=1.0, nb_mixtures=2):
    """:231-243."""
    base_points = [np.array([r * np.cos(2 * np.pi * t / nb_mixtures), r * np.sin(2 * np.pi * t / nb_mixtures)])
                   for t in range(nb_mixtures)]
    sigmas = [var * np.eye(2) for _ in range(nb_mixtures)]
    pis = [1. / nb_mixtures] * nb_mixtures
    pis[0] += 1 - sum(pis)
    return sigmas, GMM(base_points, sigmas, pis)
