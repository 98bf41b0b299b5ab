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

The band path's metrics (test_gpu_band_stages.py) and their injected defects are the
second half of this file, with their own notes.
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


def test_exact_product_of_longdouble_operands():
    """hi + lo operands against a plain longdouble matmul at 384: both sides round at
    2^-64, the plain product 384 times per entry."""
    rng = numpy.random.RandomState(11)
    n = N_PAD
    A = rng.randn(n, n).astype(bw.LD) + rng.randn(n, n).astype(bw.LD) * bw.LD(2.0) ** -40
    B = rng.randn(n, n).astype(bw.LD) * (1 + bw.LD(2.0) ** -60)
    assert bw._hi_lo(A)[1] is not None and bw._hi_lo(B)[1] is not None
    full = A @ B
    bound = (n + 8) * 2.0 ** -64 * (numpy.abs(A) @ numpy.abs(B))
    assert numpy.all(numpy.abs(bw.exact_product(A, B) - full) <= bound)
    A64 = A.astype(numpy.float64)
    assert numpy.all(numpy.abs(bw.exact_product(A64, B) - A64.astype(bw.LD) @ B) <= bound)
    assert numpy.all(numpy.abs(bw.exact_product(A, A64.T) - A @ A64.T.astype(bw.LD)) <= bound)


# ==================================================================== band path ==
# The metrics of test_gpu_band_stages.py on the numpy restatements of the band path
# (tools/band_proto.py, cholqr_proto.py, chase_proto.py, _backward.bcr_sinv_reference), on
# the same ladder with the oracle's K (n = 300, N = 384: two panels, the second ragged;
# the cyclic reduction's upper-level defect needs nt >= 5: n = 640).
#
# Each injected defect must push its metric to at least 10 x the bar the device is held to
# on every rung, max((N + 1) u, 16 x the restatements' value). Beside each: what the far-end
# scalars of test_gpu_band.py (logdet at 1e-10, tr1 / tr2 at 1e-10, lambda at 1e-12 ||K||)
# do under it.
#   a 128-tile of V negated        B is untouched: logdet, traces, lambda do not move at all
#   a panel's T transposed         the same
#   Q^T R with a panel left out    the same; the Gram blocks move (a forward test sees it
#                                  at cond <= 1e6 only)
#   a SYR2K tile skipped           B is wrong: lambda moves by O(||K||), everything sees it
#   W_l / W_r swapped (level 1)    tr1 moves; omega_sinv names the block
#   a Z_{k+1,k} block transposed   tr1 = sum tr Zd does not move at all
#   an eigenvalue moved 100 u ||T||   below 1e-12 ||K|| by 1e4: only the Sturm test sees it
#   an e^2 entry off by 1e-10      moves lambda by at most 1e-10 |e| / 2: see
#                                  test_band_e2_defect for where that can reach 10 x the bar
#   a dZ_{k-1,k} block dropped     tr2 = -sum tr dZd does not move at all (a level-0 block)
# Not seen by any bar (stated, as the dense file does): one entry of V off by 1e-14.

import os  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                'tools'))
import band_proto  # noqa: E402
import chase_proto  # noqa: E402
import cholqr_proto  # noqa: E402

TS = bw.TS
_BAND = {}


def _reduce_hh(K, skip_tile=False):
    """band_proto.band_reduce; skip_tile: panel 0's trailing update leaves out the tile
    (1, 0) of the trailing block (and its mirror image)."""
    A = numpy.tril(K).copy()
    A = A + numpy.tril(A, -1).T
    Vs, Ts = [], []
    for j in range(A.shape[0] // TS - 1):
        r0, c0 = (j + 1) * TS, j * TS
        P = A[r0:, c0:c0 + TS]
        tau = band_proto.householder_panel(P)
        V = band_proto.v_of(P)
        T = band_proto.t_of(V, tau)
        A22 = A[r0:, r0:]
        X = (A22 @ V) @ T
        W = X - V @ (0.5 * (T.T @ (V.T @ X)))
        upd = W @ V.T + V @ W.T
        if skip_tile and j == 0:
            upd[TS:2 * TS, :TS] = 0.0
            upd[:TS, TS:2 * TS] = 0.0
        A22 -= upd
        Vs.append(V.copy())
        Ts.append(T)
    return A, Vs, Ts


def _band_rung(r, n=N):
    """The restatements on a rung and the device's bars there: once, never modified."""
    key = (r, n)
    if key not in _BAND:
        nu, scale, eta = LADDER[r]
        npad = (n + TS - 1) // TS * TS
        rng = numpy.random.RandomState(n)
        pts = rng.rand(n, 2)
        K = numpy.eye(npad)
        K[:n, :n] = matern.dense_correlation(pts, scale, nu)
        R = numpy.zeros((npad, 16))
        R[:n] = numpy.column_stack([numpy.ones(n), pts, rng.randn(n, 13)])
        A, Vs, Ts = _reduce_hh(K)
        Y = band_proto.apply_qt(Vs, Ts, R, TS)
        V, T = bw.panels_to_v(Vs, Ts, npad)
        B = bw.band_of(A)
        d = dict(n=n, N=npad, eta=eta, K=K, R=R, B=B, V=V, T=T, Y=Y, Vs=Vs, Ts=Ts)
        d['hh'] = {k: v[0] for k, v in bw.reduction_metrics(K, B, V, T, R, Y).items()}
        Ac, Vc, Tc = cholqr_proto.band_reduce_cholqr(K, TS, [], n_real=n, want_vt=True)
        Yc = band_proto.apply_qt(Vc, Tc, R, TS)
        d['cq'] = {k: v[0] for k, v in bw.reduction_metrics(
            K, bw.band_of(Ac), *bw.panels_to_v(Vc, Tc, npad), R, Yc).items()}
        floor = (npad + 1) * U
        d['bars'] = {k: max(floor, 16 * max(d['hh'][k], d['cq'][k])) for k in d['hh']}
        Ae = B + eta * numpy.eye(npad)
        d['x'] = bw.band_chol_solve(Ae, Y)
        d['solve_ref'] = bw.omega_band_solve(Ae, d['x'], Y)[0]
        d['bars']['solve'] = max(floor, 16 * d['solve_ref'])
        d['Zd'], d['Zsub'], _ = bw.bcr_sinv_reference(B, eta)
        d['sinv_ref'] = bw.omega_sinv(B, eta, d['Zd'], d['Zsub'])[0]
        d['bars']['sinv'] = max(floor, 16 * d['sinv_ref'])
        for v in d.values():
            if isinstance(v, numpy.ndarray):
                v.setflags(write=False)
        _BAND[key] = d
    return _BAND[key]


@pytest.mark.parametrize('r', RUNGS)
def test_band_restatements_are_clean(r):
    d = _band_rung(r)
    floor = (d['N'] + 1) * U
    print('rung %d, (N+1)u multiples: householder %s, cholqr %s, solve %.3f, sinv %.3f' % (
        r, {k: round(v / floor, 3) for k, v in d['hh'].items()},
        {k: round(v / floor, 3) for k, v in d['cq'].items()}, d['solve_ref'] / floor,
        d['sinv_ref'] / floor))
    assert bw.band_structure(d['B'], d['V'], d['n']) == []
    # Householder panels: each below (N + 1) u on every rung (the CholeskyQR panels'
    # omega_sim and the solve are not, which is what the 16 x term of the bars is for)
    for k, v in d['hh'].items():
        assert v <= floor, k
    assert d['sinv_ref'] <= floor


def _negated_v_tile(d):
    V = d['V'].copy()
    V[2 * TS:3 * TS, :TS] *= -1.0
    return dict(V=V)


def _transposed_t(d):
    T = d['T'].copy()
    T[0] = d['T'][0].T
    return dict(T=T)


def _panel_left_out_of_qt(d):
    return dict(Y=_apply_qt_without(d, 0))


def _apply_qt_without(d, skip):
    R = d['R'].copy()
    for j, (V, T) in enumerate(zip(d['Vs'], d['Ts'])):
        if j != skip:
            r0 = (j + 1) * TS
            R[r0:] -= V @ (T.T @ (V.T @ R[r0:]))
    return R


def _skipped_syr2k_tile(d):
    A, Vs, Ts = _reduce_hh(d['K'], skip_tile=True)
    V, T = bw.panels_to_v(Vs, Ts, d['N'])
    return dict(B=bw.band_of(A), V=V, T=T, Y=band_proto.apply_qt(Vs, Ts, d['R'], TS))


# (defect, the metric that must see it)
# (omega_orth sees neither of the first two: Q^T Q = I needs T^-1 + T^-T = V^T V only,
# which holds as well for -V_2 in a row tile, V^T V being a sum over row tiles, and for
# T^T, whose Q is the transpose; both are another orthogonal matrix, so omega_sim sees them)
RED_DEFECTS = [(_negated_v_tile, 'sim'), (_transposed_t, 'sim'),
               (_skipped_syr2k_tile, 'sim'), (_panel_left_out_of_qt, 'rhs')]


@pytest.mark.parametrize('r', RUNGS)
@pytest.mark.parametrize('defect,metric', RED_DEFECTS, ids=lambda f: getattr(f, '__name__', f))
def test_band_reduction_defect_is_seen(defect, metric, r):
    d = _band_rung(r)
    a = dict(B=d['B'], V=d['V'], T=d['T'], Y=d['Y'])
    a.update(defect(d))
    m = bw.reduction_metrics(d['K'], a['B'], a['V'], a['T'], d['R'], a['Y'])
    o, at = m[metric]
    print('%s rung %d: omega_%s %.3g = %.3g x bar, at %s' % (defect.__name__, r, metric, o,
                                                            o / d['bars'][metric], at))
    assert o >= 10 * d['bars'][metric]


@pytest.mark.parametrize('r', RUNGS)
def test_band_one_entry_of_v_is_not_seen(r):
    """The perturbation the bars do not see: one entry of V off by 1e-14 moves Q by about
    1e-14 in a rank-one term, 0.2 (N + 1) u."""
    d = _band_rung(r)
    V = d['V'].copy()
    V[2 * TS + 5, 7] += 1e-14
    m = bw.reduction_metrics(d['K'], d['B'], V, d['T'], d['R'], d['Y'])
    for k in ('orth', 'sim', 'rhs'):
        assert m[k][0] <= d['bars'][k], k


@pytest.mark.parametrize('r', RUNGS)
def test_band_solve_defect_is_seen(r):
    d = _band_rung(r)
    Ae = d['B'] + d['eta'] * numpy.eye(d['N'])
    x = d['x'].copy()
    x[TS:2 * TS] = d['x'][TS:2 * TS][::-1]        # a block's rows in another order
    o, at = bw.omega_band_solve(Ae, x, d['Y'])
    print('reversed block rung %d: omega_solve %.3g = %.3g x bar' % (r, o, o / d['bars']['solve']))
    assert at in (0, 1, 2) and o >= 10 * d['bars']['solve']
    # G2 = x^T x, a sum of squares, does not move
    assert bw.gram_residual(x, x, d['x'].T @ d['x']) <= (d['N'] + 2) * U


@pytest.mark.parametrize('r', RUNGS)
def test_band_logdet_reference(r):
    """The longdouble banded Cholesky against LAPACK's float64 one, inside the bound the
    device is held to."""
    d = _band_rung(r)
    n = d['n']
    A = d['B'][:n, :n] + d['eta'] * numpy.eye(n)
    ld = bw.band_logdet(A)[0]
    ref = 2 * numpy.sum(numpy.log(numpy.diag(numpy.linalg.cholesky(A))))
    bar = bw.logdet_bar(A, 16 * (d['N'] + 1) * U)
    print('rung %d: logdet %.12g, LAPACK off by %.3g, bar %.3g' % (r, float(ld),
                                                                 float(abs(ld - ref)), bar))
    assert abs(ld - ref) <= bar


@pytest.mark.parametrize('r', RUNGS)
def test_band_sinv_transposed_block_is_seen_and_its_trace_is_blind(r):
    d = _band_rung(r)
    Zsub = d['Zsub'].copy()
    Zsub[0] = d['Zsub'][0].T
    o, at = bw.omega_sinv(d['B'], d['eta'], d['Zd'], Zsub)
    print('transposed Z_10 rung %d: omega_sinv %.3g = %.3g x bar at block %d'
          % (r, o, o / d['bars']['sinv'], at))
    assert o >= 10 * d['bars']['sinv'] and at in (0, 1)
    # tr1 is a function of Zd alone: it cannot move


@pytest.mark.parametrize('r', RUNGS)
def test_band_swapped_w_is_seen(r):
    """W_l and W_r of block 2 (level 1 of nt = 5) in each other's place."""
    d = _band_rung(r, 640)
    B, eta = d['B'], d['eta']
    Zd, Zsub, _ = bw.bcr_sinv_reference(B, eta, swap=2)
    o, at = bw.omega_sinv(B, eta, Zd, Zsub)
    tr_move = abs(numpy.trace(Zd.sum(axis=0)) - numpy.trace(d['Zd'].sum(axis=0))) / \
        numpy.trace(d['Zd'].sum(axis=0))
    print('swapped W rung %d: omega_sinv %.3g = %.3g x bar at block %d; tr1 moves by %.3g'
          % (r, o, o / d['bars']['sinv'], at, tr_move))
    assert o >= 10 * d['bars']['sinv']


def _chase(r):
    d = _band_rung(r)
    if 'chase' not in d:
        n = d['n']
        B = d['B'][:n, :n]
        dd, e, _ = chase_proto.chase(B, TS)
        lam = scipy.linalg.eigvalsh_tridiagonal(dd, e)
        d['chase'] = (B, dd, e * e, lam)
    return d['chase']


@pytest.mark.parametrize('r', RUNGS)
def test_band_moved_eigenvalue_is_seen(r):
    B, dd, e2, lam = _chase(r)
    scale = float(numpy.max(numpy.abs(lam)))
    m_ref = bw.sturm_margin(dd, e2, lam, scale)
    m = max(8, 4 * m_ref)
    assert bw.sturm_ok(dd, e2, lam, m * U * scale)[0]
    bad = lam.copy()
    i = len(lam) // 2
    bad[i] += 100 * U * scale
    ok, at = bw.sturm_ok(dd, e2, bad, m * U * scale)
    print('rung %d: m_ref %d, allowed %d u max|lam|; moved eigenvalue %d by 100 u: seen %s'
          % (r, m_ref, m, i, not ok))
    # (100 u is 3 x the allowed 32 u at m_ref = 8: the test is a count, not a ratio)
    assert m_ref <= 16 and not ok and at == i
    assert abs(bad[i] - lam[i]) < 1e-12 * scale / 50        # far below the forward test


@pytest.mark.parametrize('r', RUNGS)
def test_band_chase_invariants_and_e2_defect(r):
    """The restatement keeps trace and Frobenius norm to (N + 2) u. A relative 1e-10 in
    one e^2 moves ||T||_F by 1e-10 e^2 / ||T||_F^2 relatively and an eigenvalue by at most
    0.5e-10 |e|: with e the largest subdiagonal entry, that is seen at 10 x the bar only
    where e^2 >= 10 bar ||T||_F^2 / 1e-10; the test asserts the metric reports the defect
    at its full size, and 10 x the bar where that arithmetic permits."""
    B, dd, e2, lam = _chase(r)
    npad = N_PAD
    tr, fro = bw.chase_invariants(B, dd, e2)
    floor = (npad + 2) * U
    print('rung %d: chase invariants tr %.3f fro %.3f of (N+2)u' % (r, tr / floor, fro / floor))
    assert tr <= floor and fro <= floor
    k = int(numpy.argmax(e2))
    bad = e2.copy()
    bad[k] *= 1.0 + 1e-10
    fro_bad = bw.chase_invariants(B, dd, bad)[1]
    t2 = float(numpy.sum(dd * dd) + 2 * numpy.sum(e2))
    expect = 1e-10 * e2[k] / t2
    print('rung %d: e2[%d] off by 1e-10: fro %.3g (expected %.3g) = %.3g x bar'
          % (r, k, fro_bad, expect, fro_bad / max(floor, 16 * fro)))
    assert abs(fro_bad - expect) <= fro + 1e-3 * expect
    if expect >= 10 * max(floor, 16 * fro) + fro:
        assert fro_bad >= 10 * max(floor, 16 * fro)


@pytest.mark.parametrize('r', RUNGS)
def test_band_tangent_dropped_block_is_seen(r):
    """The eta-tangent of the selected inverse: the restatement's residual of
    Z + A dZ = 0, and dZ_{0,1} left zero. tr2 = -sum tr dZd does not move: the block is
    written after everything that reads it (level 0)."""
    d = _band_rung(r)
    B, eta = d['B'], d['eta']
    floor = (d['N'] + 1) * U
    Zd, Zsub, dZd, dZsub = bw.bcr_dsinv_reference(B, eta)
    ref = bw.omega_sinv(B, eta, Zd, Zsub, tangent=(dZd, dZsub))[0]
    bar = max(floor, 16 * ref)
    _, _, dZd1, dZsub1 = bw.bcr_dsinv_reference(B, eta, drop=1)
    o, at = bw.omega_sinv(B, eta, Zd, Zsub, tangent=(dZd1, dZsub1))
    print('rung %d: tangent residual %.3f (N+1)u; dropped dZ_01: %.3g = %.3g x bar at block %d'
          % (r, ref / floor, o, o / bar, at))
    assert o >= 10 * bar and at in (0, 1)
    assert numpy.array_equal(dZd1, dZd)
