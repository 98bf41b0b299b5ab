"""The dense Cholesky's left-looking panel schedule (GPMI_PANEL=col: colpanel_kernel)
against the recursive one (GPMI_PANEL=rec, the default: band SYRKs + panel_kernel) on
the same K.

Per matrix element both run the same fp64 MFMA sequence (updates in ascending operand
order, cut at multiples of 128; the panel step only leaves out products with an exact
zero of the triangular Linv), so logdet, Gram and info of a batched call, and solve /
traceinv through the single-eta cached factor, are compared bit for bit. Members whose
pivot fails hold garbage either way: for them only info is compared. One test pins the
left-looking schedule and the default (no GPMI_PANEL) to the oracle as well.

Shapes: the smallest that reach each branch of the schedule (n -> nt tiles of 128):
  300 (3), outer 16   one panel, no bulk SYRK; panel columns j = 0, 1, 2
  1000 (8), outer 4   two panels: the first bulk update reads K, the next-diagonal step
                      is skipped on each panel's last column, j up to 3; ragged pad
  1100 (9), outer 4   a one-column last panel
  1100 (9), outer 1   every column its own panel
Batches: 1; 3 (two-stream halves 1 + 2); 33 at n = 300 (one stream).
"""

import numpy
import pytest

from oracle import matern
from oracle.mixed_correlation import MixedCorrelation as OracleMC
from _util import rel

pytestmark = pytest.mark.gpu

_CACHE = {}


def _inputs(n):
    """K (Matern 3/2), [X | z] for size n: computed once, never modified."""
    if n not in _CACHE:
        rng = numpy.random.RandomState(n)
        pts = rng.rand(n, 2)
        K = matern.dense_correlation(pts, 0.2, 1.5)
        X = numpy.column_stack([numpy.ones(n), pts])
        z = numpy.sin(3 * pts[:, 0]) + 0.1 * rng.randn(n)
        for a in (K, X, z):
            a.setflags(write=False)
        _CACHE[n] = (K, X, z)
    return _CACHE[n]


@pytest.fixture(scope='module')
def hip():
    from gaussian_proc import _hip
    _hip.require_device(0)
    return _hip


def _operator(hip, monkeypatch, mode, K, R, outer, max_batch):
    """An Operator created under GPMI_PANEL=mode (None: unset, the default)."""
    if mode is None:
        monkeypatch.delenv('GPMI_PANEL', raising=False)
    else:
        monkeypatch.setenv('GPMI_PANEL', mode)
    op = hip.Operator(K.shape[0], device=0, max_batch=max_batch)
    monkeypatch.delenv('GPMI_PANEL', raising=False)
    op.load_matrix(K)
    op.set_rhs(R)
    op.set_outer(outer)
    return op


def _pair(hip, monkeypatch, n, outer, max_batch):
    K, X, z = _inputs(n)
    R = numpy.column_stack([X, z])
    return (_operator(hip, monkeypatch, 'col', K, R, outer, max_batch),
            _operator(hip, monkeypatch, 'rec', K, R, outer, max_batch), z)


def _compare_batch(col, rec, etas):
    ld_c, g_c, info_c = col.loglik_batch(etas)
    ld_r, g_r, info_r = rec.loglik_batch(etas)
    numpy.testing.assert_array_equal(info_c, info_r)
    ok = info_c == 0
    numpy.testing.assert_array_equal(ld_c[ok], ld_r[ok])
    numpy.testing.assert_array_equal(g_c[ok], g_r[ok])
    return ld_c, g_c, info_c


CASES = [(300, 16, 1), (300, 16, 3), (300, 16, 33),
         (1000, 4, 1), (1000, 4, 3),
         (1100, 4, 1), (1100, 4, 3),
         (1100, 1, 1), (1100, 1, 3)]


@pytest.mark.parametrize('n,outer,batch', CASES)
def test_colpanel_bitwise_equals_recursive(hip, monkeypatch, n, outer, batch):
    col, rec, z = _pair(hip, monkeypatch, n, outer, batch)
    try:
        etas = numpy.logspace(-2, 1, batch)
        _, _, info = _compare_batch(col, rec, etas)
        assert numpy.all(info == 0)
        # the single-eta path: its own factorization (batch of one), then the cached
        # factor's forward / backward substitution and triangular inverse
        for eta in (0.03, 2.0):
            numpy.testing.assert_array_equal(col.solve(eta, z), rec.solve(eta, z))
            assert col.traceinv(eta, 1) == rec.traceinv(eta, 1)
    finally:
        col.close()
        rec.close()


def test_colpanel_failed_pivot_info_equal(hip, monkeypatch):
    """A negative eta between the smallest eigenvalues of the leading 128 x 128 block
    and of the whole K: the first tile column factors, a later pivot fails."""
    n = 300
    K, _, _ = _inputs(n)
    lmin_all = numpy.linalg.eigvalsh(K)[0]
    lmin_lead = numpy.linalg.eigvalsh(K[:128, :128])[0]
    assert lmin_lead > lmin_all > 0
    eta = -0.5 * (lmin_all + lmin_lead)
    assert numpy.linalg.eigvalsh(K[:128, :128] + eta * numpy.eye(128))[0] > 0
    assert numpy.linalg.eigvalsh(K + eta * numpy.eye(n))[0] < 0
    col, rec, _ = _pair(hip, monkeypatch, n, 16, 3)
    try:
        etas = numpy.array([0.5, eta, 0.1])
        _, _, info = _compare_batch(col, rec, etas)
        assert info[0] == 0 and info[2] == 0
        assert info[1] > 128
    finally:
        col.close()
        rec.close()


@pytest.mark.parametrize('mode', ['col', None])
def test_colpanel_vs_oracle(hip, monkeypatch, mode):
    """The left-looking schedule, and whatever an unset GPMI_PANEL selects, against the
    CPU oracle (as test_ragged_sizes_vs_oracle)."""
    n, outer = 1000, 4
    K, X, z = _inputs(n)
    R = numpy.column_stack([X, z])
    op = _operator(hip, monkeypatch, mode, K, R, outer, 3)
    ref = OracleMC(K, 'cholesky')
    try:
        for eta in (1e-2, 1.0):
            assert rel(op.logdet(eta), ref.logdet(eta)) < 1e-10
            numpy.testing.assert_allclose(op.solve(eta, z), ref.solve(eta, z), rtol=1e-8,
                                          atol=1e-10)
            numpy.testing.assert_allclose(op.solve(eta, X), ref.solve(eta, X), rtol=1e-8,
                                          atol=1e-10)
        etas = [0.05, 0.5, 5.0]
        ld, G, info = op.loglik_batch(etas)
        assert numpy.all(info == 0)
        for e, l, g in zip(etas, ld, G):
            assert rel(l, ref.logdet(e)) < 1e-10
            numpy.testing.assert_allclose(g, R.T @ ref.solve(e, R), rtol=1e-8, atol=1e-10)
    finally:
        op.close()
