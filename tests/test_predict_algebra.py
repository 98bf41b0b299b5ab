"""Host algebra of the prediction (CPU, no device).

GaussianProcess.predict forms the posterior mean and variance from the device terms
c_j = R^T S^-1 k*_j, q_j = k*_j^T S^-1 k*_j and G = R^T S^-1 R, R = [X z]
(_profile_likelihood._predict_from_terms). Here the terms come from numpy and the result
is checked against the universal-kriging formulas written out directly.
"""
import numpy
import pytest

from oracle import matern
from _util import rel

N, M, NSTAR = 60, 3, 17
SCALE, NU = 0.2, 1.5


def _inputs(seed=11):
    rng = numpy.random.RandomState(seed)
    pts = rng.rand(N, 2)
    tst = rng.rand(NSTAR, 2)
    tst[3] = pts[7]                       # a test point that is a training point
    sc = matern.broadcast_scale(pts, SCALE)
    K = matern.dense_correlation(pts, SCALE, NU)
    Ks = matern.matern_kernel(matern.scaled_distance(tst, pts, sc), NU)   # n* x n
    X = numpy.column_stack([numpy.ones(N), pts])
    Xs = numpy.column_stack([numpy.ones(NSTAR), tst])
    z = numpy.sin(3 * pts[:, 0]) + pts[:, 1] + 0.1 * rng.randn(N)
    return K, Ks, X, Xs, z


def _kriging(K, Ks, X, Xs, z, sigma, sigma0, noise):
    """The formulas themselves, one test point at a time."""
    eta = (sigma0 / sigma) ** 2
    S = K + eta * numpy.eye(K.shape[0])
    mean = numpy.empty(Ks.shape[0])
    var = numpy.empty(Ks.shape[0])
    if X.shape[1]:
        B = X.T @ numpy.linalg.solve(S, X)
        beta = numpy.linalg.solve(B, X.T @ numpy.linalg.solve(S, z))
    for j in range(Ks.shape[0]):
        k = Ks[j]
        Sik = numpy.linalg.solve(S, k)
        if X.shape[1]:
            mean[j] = Xs[j] @ beta + Sik @ (z - X @ beta)
            r = Xs[j] - X.T @ Sik
            var[j] = sigma ** 2 * (1.0 - k @ Sik + r @ numpy.linalg.solve(B, r))
        else:
            mean[j] = Sik @ z
            var[j] = sigma ** 2 * (1.0 - k @ Sik)
        if noise:
            var[j] += sigma0 ** 2
    return mean, var


def _terms(K, Ks, X, z, eta):
    S = K + eta * numpy.eye(K.shape[0])
    R = numpy.column_stack([X, z])
    SiR = numpy.linalg.solve(S, R)
    SiK = numpy.linalg.solve(S, Ks.T)
    return Ks @ SiR, numpy.sum(Ks.T * SiK, axis=0), R.T @ SiR


@pytest.mark.parametrize('noise', [False, True])
@pytest.mark.parametrize('eta', [1e-2, 1.0])
def test_predict_from_terms_matches_kriging_formulas(eta, noise):
    from gaussian_proc._likelihood._profile_likelihood import _predict_from_terms
    K, Ks, X, Xs, z = _inputs()
    sigma = 0.7
    sigma0 = sigma * numpy.sqrt(eta)
    c, q, G = _terms(K, Ks, X, z, eta)
    mean, var = _predict_from_terms(c, q, G, Xs, sigma, sigma0, noise)
    mean_ref, var_ref = _kriging(K, Ks, X, Xs, z, sigma, sigma0, noise)
    assert mean.shape == var.shape == (NSTAR,)
    assert rel(mean, mean_ref) <= 1e-10
    assert rel(var, var_ref) <= 1e-10
    assert numpy.all(var > 0.0)


def test_noise_adds_sigma0_squared_exactly():
    from gaussian_proc._likelihood._profile_likelihood import _predict_from_terms
    K, Ks, X, Xs, z = _inputs()
    c, q, G = _terms(K, Ks, X, z, 0.25)
    m0, v0 = _predict_from_terms(c, q, G, Xs, 2.0, 1.0, False)
    m1, v1 = _predict_from_terms(c, q, G, Xs, 2.0, 1.0, True)
    numpy.testing.assert_array_equal(m0, m1)
    numpy.testing.assert_array_equal(v1, v0 + 1.0)


def test_no_basis_functions():
    """m = 0: X is n x 0, the terms have the z column only (simple kriging)."""
    from gaussian_proc._likelihood._profile_likelihood import _predict_from_terms
    K, Ks, X, Xs, z = _inputs()
    X0, Xs0 = numpy.empty((N, 0)), numpy.empty((NSTAR, 0))
    c, q, G = _terms(K, Ks, X0, z, 0.1)
    assert c.shape == (NSTAR, 1) and G.shape == (1, 1)
    mean, var = _predict_from_terms(c, q, G, Xs0, 0.5, 0.5 * numpy.sqrt(0.1))
    mean_ref, var_ref = _kriging(K, Ks, X0, Xs0, z, 0.5, 0.5 * numpy.sqrt(0.1), False)
    assert rel(mean, mean_ref) <= 1e-10 and rel(var, var_ref) <= 1e-10


def test_shape_errors():
    from gaussian_proc._likelihood._profile_likelihood import _predict_from_terms
    K, Ks, X, Xs, z = _inputs()
    c, q, G = _terms(K, Ks, X, z, 0.1)
    with pytest.raises(ValueError):
        _predict_from_terms(c, q, G, Xs[:, :2], 1.0, 0.1)       # basis width
    with pytest.raises(ValueError):
        _predict_from_terms(c[:, :3], q, G, Xs, 1.0, 0.1)       # c against G
    with pytest.raises(ValueError):
        _predict_from_terms(c, q[:-1], G, Xs, 1.0, 0.1)         # q against c
    with pytest.raises(ValueError):
        _predict_from_terms(c, q, G, Xs, 0.0, 0.1)              # sigma
