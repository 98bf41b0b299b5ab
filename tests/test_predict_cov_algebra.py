"""The host half of the joint posterior covariance, _predict_cov_from_terms (HIP-free):
fed terms built with numpy on a random SPD K (n = 40, n* = 7, m in {0, 1, 3}) it equals
the universal-kriging covariance computed directly,
  cov = sigma^2 (K** - K* S^-1 K*^T + r B^-1 r^T),  r = Phi* - K* S^-1 X,  B = X^T S^-1 X,
to 1e-12 of its largest entry (every quantity is O(1) and cond(S) is small: the rounding
of a few 40-term sums, orders below the bar); its diagonal is _predict_from_terms'
variance to the same bar; noise touches only the diagonal; shapes are checked."""
import numpy
import pytest

from gaussian_proc._likelihood._profile_likelihood import _predict_cov_from_terms, \
    _predict_from_terms

N, NS = 40, 7
SIGMA, SIGMA0 = 0.8, 0.25


def _problem(m, seed=11):
    rng = numpy.random.RandomState(seed + m)
    A = rng.randn(N + NS, N + NS)
    full = A @ A.T / (N + NS) + 0.5 * numpy.eye(N + NS)   # a joint SPD "correlation"
    d = numpy.sqrt(numpy.diag(full))
    full = full / numpy.outer(d, d)                        # unit diagonal
    K, Ks, Kss = full[:N, :N], full[N:, :N], full[N:, N:]
    X = rng.randn(N, m)
    Phi = rng.randn(NS, m)
    z = rng.randn(N)
    return K, Ks, Kss, X, Phi, z


def _terms(K, Ks, Kss, X, z, eta):
    S = K + eta * numpy.eye(N)
    R = numpy.column_stack([X, z])
    SiR = numpy.linalg.solve(S, R)
    SiK = numpy.linalg.solve(S, Ks.T)
    return Ks @ SiR, numpy.sum(Ks.T * SiK, axis=0), R.T @ SiR, Kss - Ks @ SiK


def _direct(K, Ks, Kss, X, Phi, sigma, sigma0):
    S = K + (sigma0 / sigma) ** 2 * numpy.eye(N)
    Si = numpy.linalg.inv(S)
    cov = Kss - Ks @ Si @ Ks.T
    if X.shape[1]:
        r = Phi - Ks @ Si @ X
        cov = cov + r @ numpy.linalg.inv(X.T @ Si @ X) @ r.T
    return sigma ** 2 * cov


@pytest.mark.parametrize('m', [0, 1, 3])
def test_cov_from_terms_vs_direct_kriging(m):
    K, Ks, Kss, X, Phi, z = _problem(m)
    c, q, G, C0 = _terms(K, Ks, Kss, X, z, (SIGMA0 / SIGMA) ** 2)
    cov = _predict_cov_from_terms(c, G, C0, Phi, SIGMA, SIGMA0)
    ref = _direct(K, Ks, Kss, X, Phi, SIGMA, SIGMA0)
    assert cov.shape == (NS, NS)
    err = numpy.max(numpy.abs(cov - ref)) / numpy.max(numpy.abs(ref))
    print('m = %d: err %.3g' % (m, err))
    assert err <= 1e-12
    # the diagonal is the pointwise variance (C0's diagonal is 1 - q here)
    _, var = _predict_from_terms(c, q, G, Phi, SIGMA, SIGMA0)
    assert numpy.max(numpy.abs(numpy.diag(cov) - var)) <= 1e-12 * numpy.max(numpy.abs(ref))
    # a symmetric C0 gives a symmetric covariance, bit for bit
    C0s = 0.5 * (C0 + C0.T)
    covs = _predict_cov_from_terms(c, G, C0s, Phi, SIGMA, SIGMA0)
    numpy.testing.assert_array_equal(covs, covs.T)
    # the input is not modified
    C0_before = C0.copy()
    _predict_cov_from_terms(c, G, C0, Phi, SIGMA, SIGMA0, noise=True)
    numpy.testing.assert_array_equal(C0, C0_before)


@pytest.mark.parametrize('m', [0, 3])
def test_noise_changes_only_the_diagonal(m):
    K, Ks, Kss, X, Phi, z = _problem(m)
    c, q, G, C0 = _terms(K, Ks, Kss, X, z, (SIGMA0 / SIGMA) ** 2)
    cov = _predict_cov_from_terms(c, G, C0, Phi, SIGMA, SIGMA0)
    noisy = _predict_cov_from_terms(c, G, C0, Phi, SIGMA, SIGMA0, noise=True)
    numpy.testing.assert_array_equal(noisy, cov + SIGMA0 ** 2 * numpy.eye(NS))
    off = ~numpy.eye(NS, dtype=bool)
    numpy.testing.assert_array_equal(noisy[off], cov[off])
    assert numpy.all(numpy.diag(noisy) > numpy.diag(cov))


def test_shape_errors():
    K, Ks, Kss, X, Phi, z = _problem(3)
    c, q, G, C0 = _terms(K, Ks, Kss, X, z, 0.1)
    with pytest.raises(ValueError):
        _predict_cov_from_terms(c[:, :3], G, C0, Phi, SIGMA, SIGMA0)      # c columns
    with pytest.raises(ValueError):
        _predict_cov_from_terms(c, G[:3, :3], C0, Phi, SIGMA, SIGMA0)     # G size
    with pytest.raises(ValueError):
        _predict_cov_from_terms(c, G, C0[:-1], Phi, SIGMA, SIGMA0)        # C0 not n* x n*
    with pytest.raises(ValueError):
        _predict_cov_from_terms(c, G, C0[:-1, :-1], Phi, SIGMA, SIGMA0)   # C0 of other n*
    with pytest.raises(ValueError):
        _predict_cov_from_terms(c, G, C0, Phi[:, :2], SIGMA, SIGMA0)      # Phi columns
    with pytest.raises(ValueError):
        _predict_cov_from_terms(c, numpy.empty((0, 0)), C0, Phi, SIGMA, SIGMA0)
    with pytest.raises(ValueError):
        _predict_cov_from_terms(c, G, C0, Phi, 0.0, SIGMA0)               # sigma
