"""The two pipeline forms of syrk_kernel's k-loop (GPMI_KLOOP=late, the form with the LDS
writes behind a stage's last MFMA, against the default, GPMI_KLOOP=early) on the same K.

Both forms run, per accumulator, the same fp64 MFMA sequence in the same k order; only
when a slab is loaded, written to LDS and read back differs. So logdet, Gram and info of
a batched call, and solve / traceinv through the single-eta cached factor, are compared
bit for bit (inputs and comparisons as in test_gpu_dense_colpanel.py). One test pins the
old form and the default (no GPMI_KLOOP) to the oracle as well.

Shapes: the smallest that reach every prologue and epilogue of the pipeline (a k-loop of
kdim runs kdim / 16 stages; the last two request no further slab):
  300, outer 16    band updates of kdim 128 at widths 2 and 1 (8 stages); no bulk
  1000, outer 4    kdim 128 and 256 bands; the bulk update (kdim 512) reads its C tiles
                   from K; grouped tile order
  1100, outer 4    a second bulk update from the member copy; a one-column last panel
  1100, outer 1    every bulk update at kdim 128
  2100, outer 16   band kdim 128 ... 1024: 8 to 64 stages
Batches: 1; 3 (two-stream halves 1 + 2); 33 at n = 300 (one stream); 2 at n = 2100.
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


def _operator(hip, monkeypatch, form, K, R, outer, max_batch):
    """An Operator created under GPMI_KLOOP=form (None: unset, the default)."""
    monkeypatch.delenv('GPMI_PANEL', raising=False)
    if form is None:
        monkeypatch.delenv('GPMI_KLOOP', raising=False)
    else:
        monkeypatch.setenv('GPMI_KLOOP', form)
    op = hip.Operator(K.shape[0], device=0, max_batch=max_batch)
    monkeypatch.delenv('GPMI_KLOOP', raising=False)
    op.load_matrix(K)
    op.set_rhs(R)
    op.set_outer(outer)
    return op


def _pair(hip, monkeypatch, n, outer, max_batch):
    K, X, z = _inputs(n)
    R = numpy.column_stack([X, z])
    return (_operator(hip, monkeypatch, None, K, R, outer, max_batch),
            _operator(hip, monkeypatch, 'late', K, R, outer, max_batch), z)


def _compare_batch(new, old, etas):
    ld_n, g_n, info_n = new.loglik_batch(etas)
    ld_o, g_o, info_o = old.loglik_batch(etas)
    numpy.testing.assert_array_equal(info_n, info_o)
    ok = info_n == 0
    numpy.testing.assert_array_equal(ld_n[ok], ld_o[ok])
    numpy.testing.assert_array_equal(g_n[ok], g_o[ok])
    return ld_n, g_n, info_n


CASES = [(300, 16, 1), (300, 16, 3), (300, 16, 33),
         (1000, 4, 1), (1000, 4, 3),
         (1100, 4, 1), (1100, 4, 3),
         (1100, 1, 1), (1100, 1, 3),
         (2100, 16, 2)]


@pytest.mark.parametrize('n,outer,batch', CASES)
def test_kloop_default_bitwise_equals_late(hip, monkeypatch, n, outer, batch):
    new, old, z = _pair(hip, monkeypatch, n, outer, batch)
    try:
        etas = numpy.logspace(-2, 1, batch)
        _, _, info = _compare_batch(new, old, etas)
        assert numpy.all(info == 0)
        # the single-eta path: its own factorization (batch of one), then the cached
        # factor's forward / backward substitution and triangular inverse
        for eta in (0.03, 2.0):
            numpy.testing.assert_array_equal(new.solve(eta, z), old.solve(eta, z))
            assert new.traceinv(eta, 1) == old.traceinv(eta, 1)
    finally:
        new.close()
        old.close()


def test_kloop_rejects_unknown_form(hip, monkeypatch):
    monkeypatch.setenv('GPMI_KLOOP', 'sideways')
    with pytest.raises(hip.GPMIError):
        hip.Operator(300, device=0, max_batch=1)


@pytest.mark.parametrize('form', ['late', 'early', None])
def test_kloop_vs_oracle(hip, monkeypatch, form):
    """Each form, and whatever an unset GPMI_KLOOP selects, against the CPU oracle (as
    test_colpanel_vs_oracle)."""
    n, outer = 1000, 4
    K, X, z = _inputs(n)
    R = numpy.column_stack([X, z])
    op = _operator(hip, monkeypatch, form, K, R, outer, 3)
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
