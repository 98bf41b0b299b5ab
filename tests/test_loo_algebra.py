"""Host algebra of the leave-one-out cross-validation (CPU, no device).

GaussianProcess.leave_one_out forms the n leave-one-out predictions from the device terms
dinv = diag(S^-1), sol = S^-1 R and G = R^T S^-1 R, R = [X z]
(_profile_likelihood._loo_from_terms). Here the terms come from numpy and the result is
checked against n explicit refits: point i deleted, the universal-kriging formulas of the
prediction at point i from the other n - 1. The bar is test_predict_algebra's, 1e-10
relative; the closed form agrees with the refits to <= 8e-14 at these sizes.
"""
import numpy
import pytest

from oracle import matern
from _util import rel

N, M = 60, 3
SCALE, NU = 0.2, 1.5


def _inputs(seed=11):
    """The training set of test_predict_algebra."""
    rng = numpy.random.RandomState(seed)
    pts = rng.rand(N, 2)
    rng.rand(17, 2)                       # (its test points: keeps z's noise the same)
    K = matern.dense_correlation(pts, SCALE, NU)
    X = numpy.column_stack([numpy.ones(N), pts])
    z = numpy.sin(3 * pts[:, 0]) + pts[:, 1] + 0.1 * rng.randn(N)
    return K, X, z


def _terms(K, X, z, eta):
    S = K + eta * numpy.eye(K.shape[0])
    R = numpy.column_stack([X, z])
    Si = numpy.linalg.inv(S)
    SiR = numpy.linalg.solve(S, R)
    return numpy.diag(Si).copy(), SiR, R.T @ SiR


def _without(K, X, z, i):
    keep = numpy.arange(K.shape[0]) != i
    return K[numpy.ix_(keep, keep)], K[i, keep], X[keep], z[keep]


def _refits(K, X, z, sigma, sigma0, noise):
    """n refits: the kriging formulas at point i from the other n - 1 points."""
    n, m = X.shape
    eta = (sigma0 / sigma) ** 2
    mean, var = numpy.empty(n), numpy.empty(n)
    for i in range(n):
        Ki, k, Xi, zi = _without(K, X, z, i)
        S = Ki + eta * numpy.eye(n - 1)
        Sik = numpy.linalg.solve(S, k)
        if m:
            B = Xi.T @ numpy.linalg.solve(S, Xi)
            beta = numpy.linalg.solve(B, Xi.T @ numpy.linalg.solve(S, zi))
            mean[i] = X[i] @ beta + Sik @ (zi - Xi @ beta)
            r = X[i] - Xi.T @ Sik
            var[i] = sigma ** 2 * (1.0 - k @ Sik + r @ numpy.linalg.solve(B, r))
        else:
            mean[i] = Sik @ zi
            var[i] = sigma ** 2 * (1.0 - k @ Sik)
        if noise:
            var[i] += sigma0 ** 2
    return mean, var


@pytest.fixture(scope='module')
def refits():
    """(m, eta, noise) -> the refits' (mean, var), computed once."""
    K, X, z = _inputs()
    out = {}
    for m in (0, 3):
        for eta in (1e-2, 1.0):
            for noise in (False, True):
                out[m, eta, noise] = _refits(K, X[:, :m], z, 0.7, 0.7 * numpy.sqrt(eta), noise)
    return out


@pytest.mark.parametrize('noise', [False, True])
@pytest.mark.parametrize('eta', [1e-2, 1.0])
@pytest.mark.parametrize('m', [0, 3])
def test_loo_from_terms_matches_n_refits(refits, m, eta, noise):
    from gaussian_proc._likelihood._profile_likelihood import _loo_from_terms
    K, X, z = _inputs()
    sigma = 0.7
    sigma0 = sigma * numpy.sqrt(eta)
    dinv, sol, G = _terms(K, X[:, :m], z, eta)
    assert sol.shape == (N, m + 1) and G.shape == (m + 1, m + 1)
    mean, var = _loo_from_terms(dinv, sol, G, z, sigma, sigma0, noise)
    mean_ref, var_ref = refits[m, eta, noise]
    assert mean.shape == var.shape == (N,)
    print('loo m=%d eta=%g noise=%s: rel mean %.3g var %.3g'
          % (m, eta, noise, rel(mean, mean_ref), rel(var, var_ref)))
    assert rel(mean, mean_ref) <= 1e-10
    assert rel(var, var_ref) <= 1e-10
    assert numpy.all(var > 0.0)


@pytest.mark.parametrize('noise', [False, True])
def test_loo_is_predict_on_the_reduced_data_set(noise):
    """For each i: _predict_from_terms on the data without point i, at point i."""
    from gaussian_proc._likelihood._profile_likelihood import _loo_from_terms, \
        _predict_from_terms
    K, X, z = _inputs()
    eta, sigma = 0.05, 1.3
    sigma0 = sigma * numpy.sqrt(eta)
    mean, var = _loo_from_terms(*_terms(K, X, z, eta), z, sigma, sigma0, noise)
    for i in range(N):
        Ki, k, Xi, zi = _without(K, X, z, i)
        R = numpy.column_stack([Xi, zi])
        SiR = numpy.linalg.solve(Ki + eta * numpy.eye(N - 1), R)
        Sik = numpy.linalg.solve(Ki + eta * numpy.eye(N - 1), k)
        mi, vi = _predict_from_terms((k @ SiR)[None, :], numpy.array([k @ Sik]), R.T @ SiR,
                                     X[i][None, :], sigma, sigma0, noise)
        assert rel(mean[i], mi[0]) <= 1e-10 and rel(var[i], vi[0]) <= 1e-10


def test_noise_shifts_the_variance_by_sigma0_squared():
    from gaussian_proc._likelihood._profile_likelihood import _loo_from_terms
    K, X, z = _inputs()
    terms = _terms(K, X, z, 0.25)
    m0, v0 = _loo_from_terms(*terms, z, 2.0, 1.0, False)
    m1, v1 = _loo_from_terms(*terms, z, 2.0, 1.0, True)
    numpy.testing.assert_array_equal(m0, m1)
    numpy.testing.assert_array_equal(v0, v1 - 1.0)
    assert numpy.all(v0 > 0.0)


def test_shape_errors():
    from gaussian_proc._likelihood._profile_likelihood import _loo_from_terms
    K, X, z = _inputs()
    dinv, sol, G = _terms(K, X, z, 0.1)
    with pytest.raises(ValueError):
        _loo_from_terms(dinv, sol[:, :3], G, z, 1.0, 0.1)        # sol against G
    with pytest.raises(ValueError):
        _loo_from_terms(dinv[:-1], sol, G, z, 1.0, 0.1)          # dinv against sol
    with pytest.raises(ValueError):
        _loo_from_terms(dinv, sol, G, z[:-1], 1.0, 0.1)          # z
    with pytest.raises(ValueError):
        _loo_from_terms(dinv, sol, G, z, 0.0, 0.1)               # sigma


class _StubMixed(object):
    """MixedCorrelation.loo_terms from numpy: GaussianProcess above it needs no device."""

    def __init__(self, K):
        self.K = K

    def loo_terms(self, eta, X, z):
        return _terms(self.K, X, z, eta)


def _stub_gp(K, X):
    from gaussian_proc.gaussian_process import GaussianProcess

    class _Likelihood(object):
        K_mixed = _StubMixed(K)

    g = GaussianProcess.__new__(GaussianProcess)
    g.X, g.K, g.likelihood, g.z, g.results = X, K, _Likelihood(), None, None
    return g


def test_cross_validate_scores_follow_from_mean_and_var(refits):
    K, X, z = _inputs()
    eta, sigma = 1e-2, 0.7
    hp = (sigma, sigma * numpy.sqrt(eta))
    g = _stub_gp(K, X)
    mean, var = g.leave_one_out(z=z, hyperparam=hp)               # noise=True
    mean_ref, var_ref = refits[3, eta, True]
    assert rel(mean, mean_ref) <= 1e-10 and rel(var, var_ref) <= 1e-10
    numpy.testing.assert_array_equal(g.leave_one_out(z=z, hyperparam=hp, return_var=False),
                                     mean)
    cv = g.cross_validate(z=z, hyperparam=hp)
    assert sorted(cv) == ['log_pseudo_likelihood', 'mean_squared_standardized', 'residual',
                          'rmse', 'standardized']
    res = z - mean
    numpy.testing.assert_array_equal(cv['residual'], res)
    numpy.testing.assert_allclose(cv['standardized'], res / numpy.sqrt(var), rtol=1e-15)
    assert abs(cv['rmse'] - numpy.sqrt(numpy.mean(res ** 2))) <= 1e-15
    assert abs(cv['mean_squared_standardized'] - numpy.mean(res ** 2 / var)) <= 1e-13
    lpl = sum(-0.5 * numpy.log(2 * numpy.pi * v) - r * r / (2 * v) for r, v in zip(res, var))
    assert abs(cv['log_pseudo_likelihood'] - lpl) <= 1e-12 * abs(lpl)
    # against the refits themselves
    res_ref = z - mean_ref
    lpl_ref = numpy.sum(-0.5 * numpy.log(2 * numpy.pi * var_ref) - res_ref ** 2 / (2 * var_ref))
    assert abs(cv['log_pseudo_likelihood'] - lpl_ref) <= 1e-9 * abs(lpl_ref)


def test_gaussian_process_argument_errors():
    K, X, z = _inputs()
    g = _stub_gp(K, X)
    with pytest.raises(ValueError):
        g.leave_one_out()                                         # no train, no z
    with pytest.raises(ValueError):
        g.leave_one_out(z=z)                                      # ... hyperparam missing
    with pytest.raises(ValueError):
        g.cross_validate(z=z)
    with pytest.raises(ValueError):
        g.leave_one_out(z=z, hyperparam=(0.0, 0.1))               # sigma
    with pytest.raises(ValueError):
        g.leave_one_out(z=z[:-1], hyperparam=(1.0, 0.1))          # z's length
    few = _stub_gp(K[:3, :3], X[:3])                              # n = m = 3
    with pytest.raises(ValueError):
        few.leave_one_out(z=z[:3], hyperparam=(1.0, 0.1))
    # defaults from a train
    g.z, g.results = z, {'sigma': 0.7, 'sigma0': 0.07}
    numpy.testing.assert_array_equal(g.leave_one_out()[0],
                                     g.leave_one_out(z=z, hyperparam=(0.7, 0.07))[0])
