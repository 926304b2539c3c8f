"""Exact references for the invariance tests: float64 samplers of the targets and their expectations in closed
form.  An MCMC step that leaves its target invariant maps exact samples to exact samples, so a batch of
independent exact chains stays exact after any number of steps; `zscores` measures how far a batch has moved.

Toy targets (GMM / Gaussian) are described by the numbers the library's energy actually evaluates: the float32
means, (symmetrised) float32 precision matrices and float32 log-constants, E(x) = -log sum_k exp(lc_k - q_k(x) / 2)
(or q(x) / 2 for a single Gaussian).  exp(-E / T) is then an exact mixture, whose parameters `ExactGMM` derives.

2-D U(1) on a periodic T x X lattice (V = T*X plaquettes, D = 2V links) at finite volume:
  * plaquette angles: theta_1..theta_{V-1} iid von Mises(beta), theta_V = -sum, the row kept with probability
    exp(beta (cos theta_V - 1)) -- exactly prod_p exp(beta cos theta_p) on sum_p theta_p = 0 (mod 2 pi);
  * links: the least-squares preimage of the plaquettes under the linear map of oracle.lattice.plaq_sums, plus a
    uniform gauge transformation and two uniform holonomies (together uniform on the map's kernel), wrapped;
  * exact values from the character expansion Z = sum_n I_n(beta)^V, and P(Q) proportional to f_V(2 pi Q) with f_V
    the density of a sum of V iid von Mises angles on [-pi, pi)."""
import numpy as np
from scipy.special import ive, ndtr

from oracle import lattice as olat

TWO_PI = 2.0 * np.pi


def zscores(feats, exact):
    """feats [B, J] (f_j at B independent chains), exact [J] (E f_j) -> z_j = (mean - E f) / (sd / sqrt(B))."""
    f = np.asarray(feats, dtype=np.float64)
    sd = f.std(axis=0, ddof=1)
    return (f.mean(axis=0) - np.asarray(exact, dtype=np.float64)) / (sd / np.sqrt(f.shape[0]))


# ------------------------------------------------------------------------------------------------ toy targets
class ExactGMM:
    """Mixture sum_k w_k N(mu_k, cov_k) in float64, with first / second moments and half-space probabilities."""

    def __init__(self, mus, covs, weights):
        self.mus = np.asarray(mus, dtype=np.float64)
        self.covs = np.asarray(covs, dtype=np.float64)
        w = np.asarray(weights, dtype=np.float64)
        self.w = w / w.sum()
        self.dim = self.mus.shape[1]

    @classmethod
    def from_energy(cls, mus, precs, log_consts=None, temperature=1.0):
        """The density exp(-E / T) of the energy above; a mixture (K > 1) only at T = 1."""
        mus = np.asarray(mus, dtype=np.float64)
        precs = np.asarray(precs, dtype=np.float64)
        precs = 0.5 * (precs + np.swapaxes(precs, 1, 2))
        K, d = mus.shape
        if K > 1 and temperature != 1.0:
            raise ValueError("a tempered mixture is not a mixture")
        lc = np.zeros(K) if log_consts is None else np.asarray(log_consts, dtype=np.float64)
        covs = np.linalg.inv(precs) * temperature
        # integral of exp(lc - q / 2) = exp(lc) (2 pi)^(d/2) det(cov)^(1/2)
        logw = lc + 0.5 * np.linalg.slogdet(covs)[1]
        return cls(mus, covs, np.exp(logw - logw.max()))

    @classmethod
    def of_library_gmm(cls, mus, sigmas, pis):
        """What l2hmc_amd.GMM(mus, sigmas, pis) packs (distributions.py): float32 inv(sigma), constants, means."""
        pis = np.asarray(pis, dtype=np.float64)
        pis = pis / pis.sum() if np.sum(pis) != 1.0 else pis
        d = np.asarray(mus[0]).shape[0]
        precs = [np.linalg.inv(s).astype(np.float32) for s in sigmas]
        consts = [(p / np.sqrt((2 * np.pi) ** d * np.linalg.det(s)).astype(np.float32)).astype(np.float32)
                  for p, s in zip(pis, sigmas)]
        lcs = np.log(np.asarray(consts)).astype(np.float32)
        return cls.from_energy([np.asarray(m, dtype=np.float32) for m in mus], precs, lcs)

    @classmethod
    def of_library_gaussian(cls, mu, sigma, temperature=1.0):
        """What l2hmc_amd.Gaussian(mu, sigma) packs: float32 mean and float32 inv(sigma); E / T with T."""
        prec = np.linalg.inv(np.asarray(sigma, dtype=np.float64)).astype(np.float32)
        return cls.from_energy([np.asarray(mu, dtype=np.float32)], [prec], temperature=temperature)

    def sample(self, n, rng):
        k = rng.choice(len(self.w), size=n, p=self.w)
        z = rng.standard_normal((n, self.dim))
        chol = np.linalg.cholesky(self.covs)
        return self.mus[k] + np.einsum("nij,nj->ni", chol[k], z)

    def energy(self, x):
        """-log density (up to a constant), float64; works on NumPy arrays and float64 torch tensors alike."""
        import torch
        xt = torch.as_tensor(x, dtype=torch.float64)
        mus = torch.as_tensor(self.mus, device=xt.device)
        precs = torch.as_tensor(np.linalg.inv(self.covs), device=xt.device)
        lw = torch.as_tensor(np.log(self.w) - 0.5 * np.linalg.slogdet(self.covs)[1], device=xt.device)
        dd = xt[:, None, :] - mus[None]
        q = torch.einsum("bki,kij,bkj->bk", dd, precs, dd)
        e = -torch.logsumexp(lw[None] - 0.5 * q, dim=1)
        return e if isinstance(x, torch.Tensor) else e.numpy()

    def halfspaces(self, rng, n_random=2):
        """(W [H, d], c [H]): every bisector between two modes (when K > 1), the two axes of the largest component
        through its mean shifted by one sd, and n_random random directions through random quantiles."""
        W, c = [], []
        K = len(self.w)
        for a in range(K):
            for b in range(a + 1, K):
                w = self.mus[a] - self.mus[b]
                W.append(w)
                c.append(w @ (self.mus[a] + self.mus[b]) / 2)
        k = int(np.argmax(self.w))
        ev, evec = np.linalg.eigh(self.covs[k])
        for i in (0, -1):
            w = evec[:, i]
            W.append(w)
            c.append(w @ self.mus[k] + np.sqrt(ev[i]))
        mean = self.mean()
        cov = self.second_moment() - np.outer(mean, mean)
        for _ in range(n_random):
            w = rng.standard_normal(self.dim)
            W.append(w)
            c.append(w @ mean + rng.uniform(-1, 1) * np.sqrt(w @ cov @ w))
        return np.asarray(W), np.asarray(c)

    def mean(self):
        return self.w @ self.mus

    def second_moment(self):
        return np.einsum("k,kij->ij", self.w, self.covs + np.einsum("ki,kj->kij", self.mus, self.mus))

    def prob_above(self, W, c):
        """P(w^T x > c) = sum_k w_k Phi((w^T mu_k - c) / sqrt(w^T cov_k w)), per row of W."""
        m = W @ self.mus.T                                          # [H, K]
        s = np.sqrt(np.einsum("hi,kij,hj->hk", W, self.covs, W))
        return ndtr((m - np.asarray(c)[:, None]) / s) @ self.w

    def features(self, x, W, c):
        """[B, J]: x_i, x_i x_j (i <= j), 1[w_h^T x > c_h]."""
        x = np.asarray(x, dtype=np.float64)
        iu = np.triu_indices(self.dim)
        return np.concatenate([x, (x[:, :, None] * x[:, None, :])[:, iu[0], iu[1]],
                               (x @ W.T > c).astype(np.float64)], axis=1)

    def expectations(self, W, c):
        iu = np.triu_indices(self.dim)
        return np.concatenate([self.mean(), self.second_moment()[iu], self.prob_above(W, c)])


# ------------------------------------------------------------------------------------------------- 2-D U(1)
def plaq_matrix(T, X):
    """A [V, D] with plaq_sums(x) = A x (flattened over the sites), built column by column from unit vectors."""
    D = 2 * T * X
    return olat.plaq_sums(np.eye(D), T, X).reshape(D, T * X).T


_PINV = {}


def _pinv(T, X):
    if (T, X) not in _PINV:
        _PINV[(T, X)] = np.linalg.pinv(plaq_matrix(T, X))
    return _PINV[(T, X)]


def u1_plaquette_angles(n, V, beta, rng):
    """[n, V] plaquette angles, exact draws of prod_p exp(beta cos theta_p) on sum_p theta_p = 0; theta_V is the
    unwrapped -sum of the others (the row sums to 0 exactly in exact arithmetic)."""
    out, have = [], 0
    while have < n:
        m = int(1.2 * (n - have) / max(ive(0, beta), 1e-3)) + 64      # accept rate ~ I0(beta) exp(-beta)
        th = rng.vonmises(0.0, beta, size=(m, V - 1))
        last = -th.sum(axis=1)
        keep = rng.uniform(size=m) < np.exp(beta * (np.cos(last) - 1.0))
        rows = np.concatenate([th[keep], last[keep, None]], axis=1)
        out.append(rows)
        have += rows.shape[0]
    return np.concatenate(out)[:n]


def u1_links_from_plaquettes(theta, T, X, rng, wrap=True):
    """[n, D] links whose plaquettes are theta (mod 2 pi), uniform over gauge orbits and holonomies."""
    n = theta.shape[0]
    x = theta @ _pinv(T, X).T
    links = x.reshape(n, T, X, 2)
    lam = rng.uniform(0, TWO_PI, (n, T, X))
    links[..., 0] += lam - np.roll(lam, -1, axis=1)      # link 0 points along T, link 1 along X (plaq_sums)
    links[..., 1] += lam - np.roll(lam, -1, axis=2)
    links[..., 0] += rng.uniform(0, TWO_PI, (n, 1, 1))   # holonomies: one constant per direction
    links[..., 1] += rng.uniform(0, TWO_PI, (n, 1, 1))
    x = links.reshape(n, -1)
    return np.mod(x, TWO_PI) if wrap else x


def u1_samples(n, T, X, beta, rng):
    """[n, 2*T*X] exact samples of exp(-beta S) on the torus, in [0, 2 pi)."""
    return u1_links_from_plaquettes(u1_plaquette_angles(n, T * X, beta, rng), T, X, rng)


def _bessel_terms(beta, nmax=60):
    n = np.arange(-nmax, nmax + 1)
    I = ive(n, beta)                                             # I_n e^-beta; the e^-beta cancels in the ratios
    d1 = 0.5 * (ive(n - 1, beta) + ive(n + 1, beta))
    d2 = 0.25 * (ive(n - 2, beta) + 2 * I + ive(n + 2, beta))
    return I, d1, d2


def u1_exact_moments(V, beta):
    """(<cos theta_p>, <(sum_p cos theta_p)^2>) at finite volume V from Z = sum_n I_n(beta)^V."""
    I, d1, d2 = _bessel_terms(beta)
    ok = I > 0
    I, d1, d2 = I[ok], d1[ok], d2[ok]
    logw = V * np.log(I)
    wts = np.exp(logw - logw.max())
    r1, r2 = d1 / I, d2 / I
    Z = wts.sum()
    plaq = float((wts * r1).sum() / Z)
    c2 = float((wts * (V * (V - 1) * r1 ** 2 + V * r2)).sum() / Z)
    return plaq, c2


def u1_charge_probs(V, beta, cells=2048):
    """{Q: P(Q)} of the real-valued charge sum_p project(theta_p) / 2 pi of oracle.lattice.top_charge (an
    integer on these samples): P(Q) proportional to f_V(2 pi Q), f_V by an FFT convolution of the von Mises
    density on `cells` cells (trapezoid weights; the truncated density jumps at +-pi)."""
    h = TWO_PI / cells
    phi = -np.pi + h * np.arange(cells + 1)
    p = np.exp(beta * (np.cos(phi) - 1.0))
    p[0] *= 0.5
    p[-1] *= 0.5
    p /= p.sum()
    L = V * cells + 1                                            # support of the V-fold sum: -V pi + k h
    nfft = 1 << int(np.ceil(np.log2(L)))
    f = np.fft.irfft(np.fft.rfft(p, nfft) ** V, nfft)[:L]
    qmax = V // 2
    qs = np.arange(-qmax, qmax + 1)
    k = qs * cells + V * cells // 2                              # (2 pi q + V pi) / h
    ok = (k >= 0) & (k < L)
    pq = np.clip(f[k[ok]], 0, None)
    pq /= pq.sum()
    return dict(zip(qs[ok].tolist(), pq.tolist()))


def u1_exact(T, X, beta, cells=2048):
    """dict(avg_plaq, action, action2, q2): exact expectations of the observables u1_features measures."""
    V = T * X
    plaq, c2 = u1_exact_moments(V, beta)
    probs = u1_charge_probs(V, beta, cells)
    q2 = sum(q * q * p for q, p in probs.items())
    # S = V - sum cos:  <S> = V (1 - plaq),  <S^2> = V^2 - 2 V^2 plaq + <(sum cos)^2>
    return dict(avg_plaq=plaq, action=V * (1 - plaq), action2=V * V - 2 * V * V * plaq + c2, q2=q2)


U1_FEATURES = ("avg_plaq", "action", "action2", "q2")


def u1_features(avg_plaq, action, charge):
    """[B, 4] per-chain values of U1_FEATURES from the observables (any float arrays)."""
    a = np.asarray(action, dtype=np.float64)
    q = np.asarray(charge, dtype=np.float64)
    return np.stack([np.asarray(avg_plaq, dtype=np.float64), a, a * a, q * q], axis=1)


def u1_exact_vector(T, X, beta):
    e = u1_exact(T, X, beta)
    return np.array([e[k] for k in U1_FEATURES])
