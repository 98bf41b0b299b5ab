"""The expected information in (sigma, sigma0, rho) from the device's terms (CPU only).

_profile_likelihood._fisher_from_terms turns T[a, b] = tr(A^-1 N_a A^-1 N_b), U[a] and
V[a, b] into I_ab = tr(P_S S_a P_S S_b) / 2. Here the terms are built in numpy
(_fisher_ref.terms) and the result is checked twice: against the same formula with every
matrix formed and the projector explicit (1e-10 of sqrt(I_aa I_bb): two float64
evaluations of one expression), and against an independent derivation, minus the
derivative of the expected score by central differences of step 1e-5 theta_b (1e-8 of
max|I|: the numpy statement meets 3.0e-10 at n = 127, d = 2, nu = 1.5, m = 3).
"""
import numpy
import pytest

import _fisher_ref as fref
import _scale_grad_ref as sref

N, D, NU = 127, 2, 1.5
RHO = numpy.array([0.2, 0.35])
SIGMA, SIGMA0 = 0.7, 0.3


@pytest.fixture(scope='module')
def problem():
    rng = numpy.random.RandomState(21)
    pts = rng.rand(N, D)
    X3 = numpy.column_stack([numpy.ones(N), pts[:, 0], numpy.sin(2 * pts[:, 1])])
    z = numpy.sin(3 * pts[:, 0]) + pts[:, 1] + 0.1 * rng.randn(N)
    K = sref.correlation(pts, RHO, NU)
    dK = sref.dcorrelation(pts, RHO, NU)
    return pts, X3, z, K, dK


def _from_terms(problem, m):
    from gaussian_proc._likelihood._profile_likelihood import _fisher_from_terms
    pts, X3, z, K, dK = problem
    X = X3[:, :m]
    T = fref.terms(K, dK, X, z, (SIGMA0 / SIGMA) ** 2)
    return X, _fisher_from_terms(N, m, SIGMA, SIGMA0, T)


@pytest.mark.parametrize('m', [0, 3])
def test_information_equals_direct_formula(problem, m):
    pts = problem[0]
    X, got = _from_terms(problem, m)
    want = fref.information(pts, NU, X, numpy.concatenate([[SIGMA, SIGMA0], RHO]))
    assert got.shape == (D + 2, D + 2)
    scale = numpy.sqrt(numpy.outer(numpy.diag(want), numpy.diag(want)))
    err = numpy.max(numpy.abs(got - want) / scale)
    print('information from terms, m = %d: max |err| / sqrt(I_aa I_bb) = %.3g' % (m, err))
    assert err <= 1e-10


@pytest.mark.parametrize('m', [0, 3])
def test_information_equals_minus_derivative_of_expected_score(problem, m):
    pts = problem[0]
    X, got = _from_terms(problem, m)
    theta0 = numpy.concatenate([[SIGMA, SIGMA0], RHO])
    # the expected score vanishes at theta0 itself
    s0 = fref.expected_score(pts, NU, X, theta0, theta0)
    assert numpy.max(numpy.abs(s0)) <= 1e-9 * N
    fd = fref.information_by_differences(pts, NU, X, theta0, step=1e-5)
    err = numpy.max(numpy.abs(got - fd)) / numpy.max(numpy.abs(got))
    print('information against central differences of the expected score, m = %d: %.3g'
          % (m, err))
    assert err <= 1e-8


@pytest.mark.parametrize('m', [0, 3])
def test_information_is_symmetric_and_positive_semidefinite(problem, m):
    _, got = _from_terms(problem, m)
    numpy.testing.assert_array_equal(got, got.T)
    w = numpy.linalg.eigvalsh(got)
    assert w[0] >= -1e-12 * w[-1]


def test_information_without_noise_has_a_zero_row(problem):
    """sigma0 = 0: S_sigma0 = 0, so row and column sigma0 vanish."""
    from gaussian_proc._likelihood._profile_likelihood import _fisher_from_terms
    pts, X3, z, K, dK = problem
    T = fref.terms(K + 1e-3 * numpy.eye(N), dK, X3, z, 0.0)
    info = _fisher_from_terms(N, 3, SIGMA, 0.0, T)
    assert numpy.all(info[1] == 0.0) and numpy.all(info[:, 1] == 0.0)


def test_argument_checks(problem):
    from gaussian_proc._likelihood._profile_likelihood import _fisher_from_terms
    pts, X3, z, K, dK = problem
    T = fref.terms(K, dK, X3, z, 0.1)
    with pytest.raises(ValueError):
        _fisher_from_terms(N, 2, SIGMA, SIGMA0, T)            # G is 4 x 4, not 3 x 3
    with pytest.raises(ValueError):
        _fisher_from_terms(N, 3, 0.0, SIGMA0, T)
    with pytest.raises(ValueError):
        _fisher_from_terms(N, 3, SIGMA, SIGMA0, dict(T, t=T['t'][:1]))
