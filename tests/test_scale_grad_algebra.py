"""Host algebra of the correlation-scale gradient (CPU, no device).

_profile_likelihood._scale_grad_from_terms turns the device terms t_k = tr(A^-1 dK_k),
qX_k = tr(A^-1 X G_XX^-1 X^T A^-1 dK_k) and qc_k = w^T dK_k w into d l / d rho_k of the
direct likelihood and of the likelihood profiled over sigma. Here the terms come from
numpy (_scale_grad_ref.terms) and the gradient is checked against central differences
(step 1e-5 rho_k) of a numpy log-likelihood. Bar: 1e-6 of the largest component; the
differences' own error at this step is about 1e-8 of it (truncation 1e-10, rounding of
the log-likelihood 1e-13 / 1e-5).
"""
import numpy
import pytest

import _scale_grad_ref as ref

N = 90
ETA = 0.05
RHO = {1: [0.15], 2: [0.2, 0.35], 3: [0.3, 0.2, 0.45]}


def _case(d, m, seed=21):
    rng = numpy.random.RandomState(seed + d)
    pts = rng.rand(N, d)
    cols = [numpy.ones(N), pts[:, 0], numpy.sin(2 * pts[:, -1])]
    X = numpy.column_stack(cols[:m]) if m else numpy.empty((N, 0))
    z = numpy.sin(3 * pts[:, 0]) + pts[:, -1] + 0.1 * rng.randn(N)
    return pts, X, z


@pytest.mark.parametrize('m', [0, 3])
@pytest.mark.parametrize('nu', [0.5, 1.5, 2.5, 200.0])
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('form', ['direct', 'profiled'])
def test_gradient_vs_central_differences(form, d, nu, m):
    from gaussian_proc._likelihood._profile_likelihood import _scale_grad_from_terms
    pts, X, z = _case(d, m)
    rho = numpy.array(RHO[d])
    sigma = 0.7
    sigma0 = numpy.sqrt(ETA) * sigma
    T = ref.terms(ref.correlation(pts, rho, nu), ref.dcorrelation(pts, rho, nu), X, z, ETA)
    if form == 'direct':
        got = _scale_grad_from_terms(N, m, T['t'], T['qX'], T['qc'], T['G'], sigma=sigma)
        want = ref.central_differences(
            lambda r: ref.direct_lp(ref.correlation(pts, r, nu), X, z, sigma, sigma0), rho)
    else:
        got = _scale_grad_from_terms(N, m, T['t'], T['qX'], T['qc'], T['G'])
        want = ref.central_differences(
            lambda r: ref.profiled_lp(ref.correlation(pts, r, nu), X, z, ETA), rho)
    err = numpy.max(numpy.abs(got - want)) / numpy.max(numpy.abs(want))
    print('%s d=%d nu=%g m=%d: gradient %s, err %.3g' % (form, d, nu, m, got, err))
    assert got.shape == (d,)
    assert err <= 1e-6


@pytest.mark.parametrize('m', [0, 3])
def test_eta_gradient_vs_central_differences(m):
    from gaussian_proc._likelihood._profile_likelihood import _eta_grad_from_terms
    pts, X, z = _case(2, m)
    rho = numpy.array(RHO[2])
    K = ref.correlation(pts, rho, 1.5)
    T = ref.terms(K, ref.dcorrelation(pts, rho, 1.5), X, z, ETA)
    got = _eta_grad_from_terms(N, m, T['trinv'], T['sol'], T['G'])
    h = 1e-5 * ETA
    want = (ref.profiled_lp(K, X, z, ETA + h) - ref.profiled_lp(K, X, z, ETA - h)) / (2 * h)
    assert abs(got - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize('m', [0, 3])
def test_coefficient_matrices(m):
    """C_X and c c^T: symmetric, Sol c = P z, and Sol C_X Sol^T = A^-1 X G_XX^-1 X^T A^-1."""
    from gaussian_proc._likelihood._profile_likelihood import _scale_grad_coef
    pts, X, z = _case(2, m)
    K = ref.correlation(pts, RHO[2], 1.5)
    T = ref.terms(K, ref.dcorrelation(pts, RHO[2], 1.5), X, z, ETA)
    coef = _scale_grad_coef(T['G'])
    assert coef.shape == (2, m + 1, m + 1)
    numpy.testing.assert_array_equal(coef, numpy.transpose(coef, (0, 2, 1)))
    Ai = numpy.linalg.inv(K + ETA * numpy.eye(N))
    AiX = Ai @ X
    P = Ai - (AiX @ numpy.linalg.solve(X.T @ AiX, AiX.T) if m else 0.0)
    w = P @ z
    E1 = T['sol'] @ coef[1] @ T['sol'].T
    assert numpy.max(numpy.abs(E1 - numpy.outer(w, w))) <= 1e-10 * numpy.max(numpy.abs(E1))
    E0 = T['sol'] @ coef[0] @ T['sol'].T
    assert numpy.max(numpy.abs((Ai - E0) - P)) <= 1e-10 * numpy.max(numpy.abs(P))


def test_half_order_is_zero_at_duplicated_points():
    """x = 0 off the diagonal: the nu = 1/2 derivative is 0 there, not NaN."""
    pts = numpy.array([[0.1, 0.2], [0.1, 0.2], [0.4, 0.9]])
    dK = ref.dcorrelation(pts, [0.2, 0.3], 0.5)
    assert numpy.all(numpy.isfinite(dK)) and dK[0, 0, 1] == 0.0 and dK[1, 1, 0] == 0.0


def test_argument_checks():
    from gaussian_proc._likelihood._profile_likelihood import _scale_grad_from_terms, \
        _scale_grad_coef
    G = numpy.eye(3)
    with pytest.raises(ValueError):
        _scale_grad_from_terms(10, 2, numpy.ones(2), numpy.ones(3), numpy.ones(2), G)
    with pytest.raises(ValueError):
        _scale_grad_from_terms(10, 1, numpy.ones(2), numpy.ones(2), numpy.ones(2), G)
    with pytest.raises(ValueError):
        _scale_grad_from_terms(10, 2, numpy.ones(2), numpy.ones(2), numpy.ones(2), G, sigma=0.0)
    with pytest.raises(ValueError):
        _scale_grad_coef(numpy.ones((2, 3)))
