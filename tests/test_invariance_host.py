"""The exact references of the invariance tests (tests/invariance.py) against closed forms and oracle/lattice.py:
the float64 generators sample what the formulas say, at batch sizes where a bias of a few tenths of a percent
would show."""
import numpy as np
import pytest
from scipy.special import i0, i1

from oracle import lattice as olat
from tests import helpers as H
from tests import invariance as I


def _gmm3():
    mus = [np.array([1., 0., 0.5]), np.array([0., 1., -0.5]), np.array([-1., -1., 0.])]
    covs = [np.diag([0.05, 0.08, 0.1]), 0.07 * np.eye(3) + 0.02, np.diag([0.1, 0.05, 0.06])]
    return mus, covs, [0.3, 0.5, 0.2]


@pytest.mark.parametrize("kind", ["scg", "scg_T3", "mog", "gmm3"])
def test_toy_generators_match_their_closed_forms(kind):
    if kind.startswith("scg"):
        ex = I.ExactGMM.of_library_gaussian(np.zeros(2), H.scg_target_oracle().sigma,
                                            temperature=3.0 if kind == "scg_T3" else 1.0)
    elif kind == "mog":
        m = H.mog_target_oracle()
        ex = I.ExactGMM.of_library_gmm(m.mus, m.sigmas, m.pis)
    else:
        ex = I.ExactGMM.of_library_gmm(*_gmm3())
    W, c = ex.halfspaces(np.random.default_rng(5))
    x = ex.sample(400_000, np.random.default_rng(1))
    z = I.zscores(ex.features(x, W, c), ex.expectations(W, c))
    assert np.abs(z).max() < 5, z
    # the energy is the negative log of the density the sampler draws from
    ref = np.log(sum(w * np.exp(-0.5 * np.einsum("bi,ij,bj->b", x[:8] - m, np.linalg.inv(S), x[:8] - m))
                     / np.sqrt(np.linalg.det(2 * np.pi * S)) for w, m, S in zip(ex.w, ex.mus, ex.covs)))
    e = ex.energy(x[:8])
    np.testing.assert_allclose(-e - (-e[0]), ref - ref[0], rtol=0, atol=1e-10)


def test_library_targets_are_the_float32_energies():
    """The mixture from_energy derives has exactly the energy the oracle's GMM / Gaussian evaluate (float32
    parameters, float64 arithmetic), up to a constant; a tempered Gaussian has T times the covariance."""
    rng = np.random.default_rng(2)
    m = H.mog_target_oracle()
    for tgt, ex in ((m, I.ExactGMM.of_library_gmm(m.mus, m.sigmas, m.pis)),
                    (I.ExactGMM.of_library_gmm(*_gmm3()), None),
                    (H.scg_target_oracle(), I.ExactGMM.of_library_gaussian(np.zeros(2), H.scg_target_oracle().sigma))):
        if ex is None:
            from oracle import dynamics as od
            ex, tgt = tgt, od.GMM(*_gmm3())
        x = ex.sample(64, rng)
        d = tgt.energy(x) - ex.energy(x)
        assert np.ptp(d) < 1e-9, np.ptp(d)
    s = H.scg_target_oracle().sigma
    e1 = I.ExactGMM.of_library_gaussian(np.zeros(2), s)
    e3 = I.ExactGMM.of_library_gaussian(np.zeros(2), s, temperature=3.0)
    np.testing.assert_allclose(e3.covs, 3 * e1.covs, rtol=1e-12)
    np.testing.assert_allclose(e1.covs[0], s, rtol=1e-4)          # float32 precision of a cond-1e3 matrix
    with pytest.raises(ValueError):
        I.ExactGMM.from_energy(m.mus, [np.eye(2)] * 2, temperature=2.0)


def test_halfspace_probabilities_include_the_mode_bisector():
    m = H.mog_target_oracle()
    ex = I.ExactGMM.of_library_gmm(m.mus, m.sigmas, m.pis)
    W, c = ex.halfspaces(np.random.default_rng(5))
    np.testing.assert_allclose(W[0], ex.mus[0] - ex.mus[1])
    assert abs(ex.prob_above(W[:1], c[:1])[0] - 0.5) < 1e-12      # equal weights, equal covariances
    # a one-component closed form against numerical integration of the Gaussian along w
    g = I.ExactGMM([np.array([0.3, -0.2])], [np.array([[2.0, 0.5], [0.5, 1.0]])], [1.0])
    w, cc = np.array([1.0, 2.0]), 0.7
    s = np.sqrt(w @ g.covs[0] @ w)
    t = np.linspace(cc, cc + 12 * s, 200_001)
    dens = np.exp(-0.5 * ((t - w @ g.mus[0]) / s) ** 2) / (s * np.sqrt(2 * np.pi))
    assert abs(g.prob_above(w[None], [cc])[0] - np.sum(0.5 * (dens[1:] + dens[:-1]) * np.diff(t))) < 1e-9


@pytest.mark.parametrize("T,X", [(2, 4), (4, 4), (6, 6), (4, 16), (8, 8)])
def test_links_reproduce_the_drawn_plaquettes(T, X):
    """oracle.lattice.plaq_sums of the constructed (gauge-transformed, holonomy-shifted, wrapped) links gives back
    the drawn angles mod 2 pi, and the real-valued charge is an integer."""
    rng = np.random.default_rng(T * 100 + X)
    th = I.u1_plaquette_angles(300, T * X, 1.5, rng)
    np.testing.assert_allclose(th.sum(axis=1), 0, atol=1e-11)
    x = I.u1_links_from_plaquettes(th, T, X, rng)
    assert x.min() >= 0 and x.max() < 2 * np.pi
    p = olat.plaq_sums(x, T, X).reshape(300, -1)
    d = np.mod(p - th + np.pi, 2 * np.pi) - np.pi
    assert np.abs(d).max() < 1e-12
    q = olat.top_charge(x, T, X)
    assert np.abs(q - np.round(q)).max() < 1e-11
    # the gauge and holonomy parts leave the plaquettes alone but do move the links
    x0 = np.mod(th @ I._pinv(T, X).T, 2 * np.pi)
    assert np.abs(np.mod(x - x0 + np.pi, 2 * np.pi) - np.pi).min(axis=1).max() > 1e-3
    # A has rank V - 1: the plaquettes always sum to 0 mod 2 pi
    assert np.linalg.matrix_rank(I.plaq_matrix(T, X)) == T * X - 1


@pytest.mark.parametrize("T,X,beta", [(2, 4, 1.0), (4, 4, 2.0), (6, 6, 3.0), (4, 16, 1.5)])
def test_u1_generator_matches_the_finite_volume_values(T, X, beta):
    """Plaquette, action, action^2 and Q^2 of exact samples, measured with oracle/lattice.py, against the character
    expansion and the charge distribution."""
    B = 100_000 if T * X <= 16 else 30_000
    x = I.u1_samples(B, T, X, beta, np.random.default_rng(11))
    f = I.u1_features(olat.avg_plaq(x, T, X), olat.total_action(x, T, X), olat.top_charge(x, T, X))
    z = I.zscores(f, I.u1_exact_vector(T, X, beta))
    assert np.abs(z).max() < 5, z


def test_finite_volume_values():
    """At V = 8 the plaquette differs visibly from the infinite-volume I1/I0 (the issue's scratch numbers), at
    8 x 8 the two agree to 1e-9; P(Q) is normalised, symmetric, and converged in the grid."""
    e = I.u1_exact(2, 4, 1.0)
    assert abs(e["avg_plaq"] - 0.44889) < 1e-5 and abs(e["q2"] - 0.3120) < 1e-4
    assert e["avg_plaq"] - i1(1.0) / i0(1.0) > 2e-3
    assert abs(I.u1_exact(8, 8, 2.0)["avg_plaq"] - olat.u1_plaq_exact(2.0)) < 1e-9
    assert abs(I.u1_exact(32, 32, 4.0)["avg_plaq"] - olat.u1_plaq_exact(4.0)) < 1e-12
    for V, beta in ((8, 1.0), (64, 2.0), (36, 3.0)):
        p = I.u1_charge_probs(V, beta)
        assert abs(sum(p.values()) - 1) < 1e-12 and abs(p[1] - p[-1]) < 1e-9
        fine = I.u1_charge_probs(V, beta, cells=4096)
        coarse = I.u1_charge_probs(V, beta, cells=512)
        q2 = [sum(q * q * w for q, w in d.items()) for d in (fine, coarse)]
        assert abs(q2[0] - q2[1]) < 1e-5 * max(1.0, q2[0]), q2
    # <(sum cos)^2> - <sum cos>^2 is V times the derivative of <cos> in beta (the action's variance)
    V, b, h = 8, 1.0, 1e-5
    plaq, c2 = I.u1_exact_moments(V, b)
    dplaq = (I.u1_exact_moments(V, b + h)[0] - I.u1_exact_moments(V, b - h)[0]) / (2 * h)
    assert abs((c2 - (V * plaq) ** 2) - V * dplaq) < 1e-6


def test_zscores_are_standard_normal_for_exact_samples():
    rng = np.random.default_rng(0)
    z = np.array([I.zscores(rng.standard_normal((4000, 1)), [0.0])[0] for _ in range(400)])
    assert abs(z.mean()) < 0.2 and abs(z.std() - 1) < 0.1
    assert I.zscores(rng.standard_normal((4000, 1)) + 0.2, [0.0])[0] > 8
