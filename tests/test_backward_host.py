"""The backward-error metrics of _backward.py see what they are for (CPU only).

On the n = 300 conditioning ladder of test_gpu_dense_stages.py (oracle K + eta I):

Clean factors. LAPACK's factor has omega_chol <= (n + 1) u (Higham, Accuracy and Stability
of Numerical Algorithms, 2nd ed., Theorem 10.3; measured 0.055 ... 0.072 of it), and its
triangular inverse has omega_inv <= (n + 1) u (Theorem 8.5, per column). blocked_reference,
the device's algorithm in numpy, stays below the first-order ceiling of a panel formed
with an explicit inverse, (n + 1) u (1 + kappa_max) (measured 0.083, 0.39, 0.63, 0.88 and
28.4 times (n + 1) u down the ladder).

Injected errors. Starting from the LAPACK L, W = L^-T and T = W W^T, each defect on its own
must push the matching metric to at least 10 x the bar the device is held to on that rung
(cholesky: max((n + 1) u, 16 omega_chol(blocked_reference)); inverse: the same with
omega_inv; A^-1: (n_pad + 1) u). One defect cannot reach that on every rung and the test
says so by arithmetic, not by looking at the result: a relative 1e-12 in one entry L_ij
moves (L L^T)_ii by at most 2e-12 (|L| |L^T|)_ii and any other entry by less, so omega_chol
is at most 2e-12 (attained for L_00, the entry perturbed here). That is 10 x the bar only
where the bar is below 2e-13 = 6.0 (n + 1) u: on the first rung, bar 1.3 (n + 1) u (45 x),
but not where the reference itself sits at 0.39 ... 28 (n + 1) u and the bar is 16 times
that (9.7 x, 5.9 x, 4.3 x, 0.13 x). There the test asserts that the metric reports the
defect at its full size, 2e-12.

||W||_F^2 and ||T||_F^2, which are what traceinv(eta, 1) and traceinv(eta, 2) return, do
not move under the sign and transpose defects: the blindness the read-backs remove.
"""

import numpy
import pytest
import scipy.linalg

from oracle import matern
import _backward as bw

U = bw.U
N = 300
N_PAD = 384
# (nu, scale, eta); nu = 100 is the Gaussian limit
LADDER = [(1.5, 0.2, 1e-2), (2.5, 0.2, 1e-6), (2.5, 1.0, 1e-6), (2.5, 1.0, 1e-10),
          (100, 0.5, 1e-10)]
RUNGS = list(range(len(LADDER)))

_CACHE = {}


def _rung(r):
    """A, LAPACK's L, W, T, the blocked reference and the device's bars: once per rung,
    never modified."""
    if r not in _CACHE:
        nu, scale, eta = LADDER[r]
        pts = numpy.random.RandomState(N).rand(N, 2)
        A = matern.dense_correlation(pts, scale, nu) + eta * numpy.eye(N)
        L = numpy.linalg.cholesky(A)
        W = numpy.ascontiguousarray(
            scipy.linalg.solve_triangular(L, numpy.eye(N), lower=True).T)
        T = W @ W.T
        T = numpy.tril(T) + numpy.tril(T, -1).T
        Lb, Wb = bw.blocked_reference(A)
        d = dict(A=A, L=L, W=W, T=T, Lb=Lb, Wb=Wb,
                 chol_ref=bw.omega_chol(A, Lb), inv_ref=bw.omega_inv(Lb, Wb),
                 kappa=bw.kappa_max(Lb))
        d['chol_bar'] = max((N + 1) * U, 16 * d['chol_ref'])
        d['inv_bar'] = max((N + 1) * U, 16 * d['inv_ref'])
        d['gram_bar'] = (N_PAD + 1) * U
        for v in d.values():
            if isinstance(v, numpy.ndarray):
                v.setflags(write=False)
        _CACHE[r] = d
    return _CACHE[r]


@pytest.mark.parametrize('r', RUNGS)
def test_clean_factors(r):
    d = _rung(r)
    nu1 = (N + 1) * U
    o_lapack = bw.omega_chol(d['A'], d['L'])
    o_inv = bw.omega_inv(d['L'], d['W'])
    o_gram = bw.omega_gram(d['W'], d['T'])
    print('rung %d: kappa_max %.2g; (n+1)u multiples: chol lapack %.3f blocked %.3f, '
          'inv lapack %.3f blocked %.3f, gram %.3f'
          % (r, d['kappa'], o_lapack / nu1, d['chol_ref'] / nu1, o_inv / nu1,
             d['inv_ref'] / nu1, o_gram / nu1))
    assert o_lapack <= nu1
    assert o_inv <= nu1
    assert o_gram <= nu1
    assert d['chol_ref'] <= nu1 * (1 + d['kappa'])
    # (the other two bars of the device are multiples of the reference's own value)
    assert d['chol_ref'] <= d['chol_bar'] and d['inv_ref'] <= d['inv_bar']


def test_ladder_matches_the_recorded_reference_errors():
    """The ladder is the one DESIGN's table records: blocked_reference's omega_chol in
    multiples of (n + 1) u, to the two digits written there."""
    got = [_rung(r)['chol_ref'] / ((N + 1) * U) for r in RUNGS]
    numpy.testing.assert_allclose(got, [0.083, 0.39, 0.63, 0.88, 28.4], rtol=0.02)


# ---------------------------------------------------------------- injected --

T0 = slice(0, 128)
T1 = slice(128, 256)


def _negated_tile(d):
    L = d['L'].copy()
    L[T1, T0] *= -1.0
    return L


def _transposed_tile(d):
    L = d['L'].copy()
    L[T1, T0] = d['L'][T1, T0].T
    return L


def _dropped_slab(d):
    """Tile (1, 1)'s trailing update without the last 16 columns of the k-loop: its
    diagonal tile is then the factor of A_11 - L_10[:, :112] L_10[:, :112]^T."""
    L = d['L'].copy()
    P = d['L'][T1, T0][:, :112]
    L[T1, T1] = numpy.linalg.cholesky(d['A'][T1, T1] - P @ P.T)
    return L


def _one_entry(d):
    L = d['L'].copy()
    L[0, 0] *= 1.0 + 1e-12
    return L


def _one_newton_step(d):
    """The pivots of the first 16 x 16 diagonal block as d r_1, r_1 one Newton step from a
    seed of relative error 2^-13: r_1 is accurate to 1.5 * 2^-26, where the second step
    would reach 2^-51. (Row 0 holds its pivot alone, so omega_chol is twice that error on
    every rung; further down a pivot is a small part of its row of |L| |L^T|.)"""
    L = d['L'].copy()
    j = numpy.arange(0, 16)
    piv = d['L'][j, j]
    dd = piv * piv
    r0 = (1.0 / piv) * (1.0 + 2.0 ** -13)
    r1 = r0 * (1.5 - 0.5 * dd * r0 * r0)
    L[j, j] = dd * r1
    return L


CHOL_DEFECTS = [_negated_tile, _transposed_tile, _dropped_slab, _one_newton_step]


@pytest.mark.parametrize('r', RUNGS)
@pytest.mark.parametrize('defect', CHOL_DEFECTS, ids=lambda f: f.__name__.strip('_'))
def test_factor_defect_is_seen(defect, r):
    d = _rung(r)
    o = bw.omega_chol(d['A'], defect(d))
    print('%s rung %d: omega_chol %.3g = %.3g x bar' % (defect.__name__, r, o,
                                                        o / d['chol_bar']))
    assert o >= 10 * d['chol_bar']


@pytest.mark.parametrize('r', RUNGS)
def test_one_entry_defect_is_seen(r):
    d = _rung(r)
    o = bw.omega_chol(d['A'], _one_entry(d))
    print('one entry rung %d: omega_chol %.3g = %.3g x bar' % (r, o, o / d['chol_bar']))
    # the defect at its full size (module docstring) ...
    assert 1.99e-12 <= o <= 2.01e-12
    # ... which is 10 x the bar wherever the bar permits that at all
    if r == 0:
        assert d['chol_bar'] <= 2e-13
    if d['chol_bar'] <= 2e-13:
        assert o >= 10 * d['chol_bar']


def _sumsq(X):
    return float(numpy.sum(numpy.asarray(X, dtype=bw.LD) ** 2))


@pytest.mark.parametrize('r', RUNGS)
def test_trinv_defect_is_seen_and_its_trace_is_blind(r):
    d = _rung(r)
    W = d['W'].copy()
    W[T0, T1] *= -1.0
    o = bw.omega_inv(d['L'], W)
    print('negated W tile rung %d: omega_inv %.3g = %.3g x bar' % (r, o, o / d['inv_bar']))
    assert o >= 10 * d['inv_bar']
    assert _sumsq(W) == _sumsq(d['W'])


@pytest.mark.parametrize('r', RUNGS)
def test_inverse_defect_is_seen_and_its_trace_is_blind(r):
    d = _rung(r)
    T = d['T'].copy()
    T[T1, T0] = d['T'][T1, T0].T
    o = bw.omega_gram(d['W'], T)
    print('transposed T tile rung %d: omega_gram %.3g = %.3g x bar'
          % (r, o, o / d['gram_bar']))
    assert o >= 10 * d['gram_bar']
    # the same numbers in another order: equal to the longdouble sum's rounding
    assert abs(_sumsq(T) - _sumsq(d['T'])) <= 2.0 ** -50 * _sumsq(d['T'])


@pytest.mark.parametrize('r', [0, 4])
def test_factor_sign_defect_leaves_logdet_and_traces(r):
    """logdet, and tr(A^-1) through a consistent W, do not see a negated tile of L."""
    d = _rung(r)
    L = _negated_tile(d)
    assert bw.logdet_from_factor(L)[0] == bw.logdet_from_factor(d['L'])[0]
    assert _sumsq(L) == _sumsq(d['L'])


# ---------------------------------------------------------------- products --

@pytest.mark.parametrize('r', [0, 4])
def test_exact_product_against_longdouble(r):
    d = _rung(r)
    L, W = d['L'], d['W']
    Lq = L.astype(bw.LD)
    full = Lq @ Lq.T
    bar = 1e-3 * (N + 1) * U * bw.abs_gram(L)
    g = bw.exact_gram(L)
    assert numpy.all(numpy.abs(g - full) <= bar)
    assert numpy.array_equal(g, g.T)
    assert numpy.all(numpy.abs(bw.exact_product(L, L.T) - full) <= bar)
    # a general product, and one with a wide range of magnitudes within a row
    full = W.T.astype(bw.LD) @ Lq
    bar = 1e-3 * (N + 1) * U * (numpy.abs(W.T) @ numpy.abs(L))
    assert numpy.all(numpy.abs(bw.exact_product(W.T, L) - full) <= bar)


def test_split_is_exact():
    rng = numpy.random.RandomState(5)
    A = rng.randn(40, 70) * numpy.exp2(rng.randint(-40, 40, size=(40, 70)))
    A[3] = 0.0
    S, R = bw._split_rows(A, 3)
    acc = R[3].astype(bw.LD)
    for s in S:
        acc = acc + s
    assert numpy.array_equal(acc, A.astype(bw.LD))
    amax = numpy.max(numpy.abs(A), axis=1)
    for p, s in enumerate(S, 1):
        unit = numpy.exp2(numpy.frexp(numpy.where(amax > 0, amax, 1.0))[1] - 20.0 * p)[:, None]
        k = s / unit
        assert numpy.array_equal(k, numpy.rint(k)) and numpy.max(numpy.abs(k)) <= 2 ** 20


def test_solve_metric():
    d = _rung(0)
    b = numpy.random.RandomState(7).randn(N, 3)
    x = scipy.linalg.cho_solve((d['L'], True), b)
    assert bw.omega_solve(d['A'], d['L'], x, b) <= (3 * N + 1) * U
    x[17, 1] *= 1.0 + 1e-9
    assert bw.omega_solve(d['A'], d['L'], x, b) >= 10 * (3 * N + 1) * U
