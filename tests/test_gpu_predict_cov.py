"""Joint posterior covariance of the new points on an MI355X (gfx950): the device block
C0 = K** - K* S^-1 K*^T = K** - V V^T (csrc/gpmi_predict.hip: pred_cov_partial_kernel,
pred_cov_reduce_kernel over the block V that the wide forward substitution keeps) and
GaussianProcess.predict(return_cov=True) above it.

Bars. C0: max |C0 - reference| <= 1e-8 ABSOLUTE against numpy on the device's own K (K**
and V V^T are both O(1) with unit diagonal), the bar q is held to in test_gpu_predict.py;
at these sizes cond(K + eta I) <= (n + eta) / eta <= 7e4, so the fp64 forward error is
orders below it. diag(C0) against 1 - q of the same call: 1e-11, the two being the same
sum in another order (n u < 1e-13 at n <= 700). Symmetry, and equality with
predict_terms, with the uploaded route and across chunk widths: bit for bit. End to end:
1e-8 max|reference|, as the variance in test_gpu_predict.py.
"""
import ctypes

import numpy
import pytest

from oracle import data

pytestmark = pytest.mark.gpu

SCALE, NU = 0.2, 1.5


@pytest.fixture(scope='module')
def gp():
    import gaussian_proc
    from gaussian_proc import _hip
    _hip.require_device(0)
    return gaussian_proc


def _mixed(gp, n, seed=3, max_batch=1):
    """-> (MixedCorrelation on a DeviceCorrelation, points, K on the host)."""
    from gaussian_proc._mixed_correlation import MixedCorrelation
    rng = numpy.random.RandomState(seed)
    pts = rng.rand(n, 2)
    D = gp.generate_correlation(pts, SCALE, NU, device_resident=True, max_batch=max_batch)
    return MixedCorrelation(D, imate_method='cholesky'), pts, D.toarray()


def _rhs(pts, ncol, seed=4):
    """X (n x (ncol - 1)) and z: ncol = m + 1 resident columns."""
    rng = numpy.random.RandomState(seed)
    n = pts.shape[0]
    cols = [numpy.ones(n), pts[:, 0], pts[:, 1]]
    while len(cols) < ncol - 1:
        cols.append(rng.randn(n))
    X = numpy.column_stack(cols[:ncol - 1]) if ncol > 1 else numpy.empty((n, 0))
    z = numpy.sin(3 * pts[:, 0]) + pts[:, 1] + 0.1 * rng.randn(n)
    return X, z


def _err(a, ref):
    return float(numpy.max(numpy.abs(a - ref)) / numpy.max(numpy.abs(ref)))


def _ref_c0(K, Ks, Kss, eta):
    S = K + eta * numpy.eye(K.shape[0])
    return Kss - Ks @ numpy.linalg.solve(S, Ks.T)


def _setenv(monkeypatch, name, value):
    if value is not None:
        monkeypatch.setenv(name, str(value))
    else:
        monkeypatch.delenv(name, raising=False)


def _equal4(a, b):
    for x, y in zip(a, b):
        numpy.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------- terms --

# (n, outer panel width or None, n*, GPMI_PREDICT_CHUNK or None, m + 1,
#  GPMI_PREDICT_COV_SPLIT or None)
COV_CASES = [
    (1, None, 1, None, 1, None),       # the smallest call
    (127, None, 130, None, 4, None),   # one tile row, two column tiles, ragged
    (129, None, 257, None, 16, 2),
    (300, None, 257, 128, 4, None),    # three solve chunks, covariance tiles spanning chunks
    (300, 1, 257, 128, 4, 3),          # one piece per tile row
    (700, None, 130, None, 4, 4),      # six tile rows in four ragged pieces, across the
                                       # default panel width
    (700, None, 130, None, 4, 99),     # split clipped to nt
]


@pytest.mark.parametrize('n,outer,ns,chunk,ncol,split', COV_CASES)
def test_cov_terms_vs_numpy_and_routes(gp, monkeypatch, n, outer, ns, chunk, ncol, split):
    _setenv(monkeypatch, 'GPMI_PREDICT_CHUNK', chunk)
    _setenv(monkeypatch, 'GPMI_PREDICT_COV_SPLIT', split)
    mc, pts, K = _mixed(gp, n)
    if outer is not None:
        mc.op.set_outer(outer)
    X, z = _rhs(pts, ncol)
    tst = numpy.random.RandomState(5).rand(ns, 2)
    tst[ns // 2] = pts[n // 3]
    Ks = gp.generate_cross_correlation(tst, pts, SCALE, NU)
    Kss = gp.generate_cross_correlation(tst, tst, SCALE, NU)
    numpy.testing.assert_array_equal(Kss, Kss.T)
    nt = (n + 127) // 128
    for eta in (1e-2, 1.0):
        c, q, G, C0 = mc.predict_cov_terms(eta, X, z, test_points=tst)
        assert c.shape == (ns, ncol) and q.shape == (ns,) and G.shape == (ncol, ncol)
        assert C0.shape == (ns, ns)
        used = mc.op.predict_cov_ms()['split']
        assert 1 <= used <= nt and (split is None or used == min(split, nt))
        err = float(numpy.max(numpy.abs(C0 - _ref_c0(K, Ks, Kss, eta))))
        dq = float(numpy.max(numpy.abs(numpy.diag(C0) - (1.0 - q))))
        print('cov n=%d outer=%s n*=%d chunk=%s cols=%d split=%s (%d) eta=%g: '
              'max|C0 - ref| %.3g  max|diag - (1 - q)| %.3g'
              % (n, outer, ns, chunk, ncol, split, used, eta, err, dq))
        assert err <= 1e-8
        numpy.testing.assert_array_equal(C0, C0.T)
        assert dq <= 1e-11
        # c, q, G are predict_terms' own
        _equal4((c, q, G), mc.predict_terms(eta, X, z, test_points=tst))
        # the uploaded route runs the same solve and product on the same numbers
        _equal4((c, q, G, C0), mc.predict_cov_terms(eta, X, z, cross=Ks, cross_star=Kss))
        if chunk is not None:
            # the chunk width of the solve does not reach the covariance
            monkeypatch.delenv('GPMI_PREDICT_CHUNK')
            _equal4((c, q, G, C0), mc.predict_cov_terms(eta, X, z, test_points=tst))
            monkeypatch.setenv('GPMI_PREDICT_CHUNK', str(chunk))


def test_workspace_order(gp, monkeypatch):
    """A narrow predict_terms, a wider predict_cov_terms (which widens the working block)
    and predict_terms again, with and without a solve in between: every call reproduces
    its stand-alone result bit for bit."""
    monkeypatch.delenv('GPMI_PREDICT_CHUNK', raising=False)
    monkeypatch.delenv('GPMI_PREDICT_COV_SPLIT', raising=False)
    X = z = None
    narrow = numpy.random.RandomState(12).rand(40, 2)
    wide = numpy.random.RandomState(13).rand(257, 2)
    eta = 0.1

    def fresh():
        mc, pts, _ = _mixed(gp, 300)
        return mc, _rhs(pts, 4)

    mc, (X, z) = fresh()
    alone_terms = mc.predict_terms(eta, X, z, test_points=narrow)
    mc, _ = fresh()
    alone_cov = mc.predict_cov_terms(eta, X, z, test_points=wide)
    mc, _ = fresh()
    alone_cov_narrow = mc.predict_cov_terms(eta, X, z, test_points=narrow)
    for with_solve in (False, True):
        mc, _ = fresh()
        _equal4(alone_terms, mc.predict_terms(eta, X, z, test_points=narrow))
        if with_solve:
            mc.solve(eta, z)
        _equal4(alone_cov, mc.predict_cov_terms(eta, X, z, test_points=wide))
        if with_solve:
            mc.solve(eta, z)
        _equal4(alone_terms, mc.predict_terms(eta, X, z, test_points=narrow))
        # and a narrower covariance inside the buffers the wide one left
        _equal4(alone_cov_narrow, mc.predict_cov_terms(eta, X, z, test_points=narrow))
        _equal4(alone_cov, mc.predict_cov_terms(eta, X, z, test_points=wide))


# -------------------------------------------------------------- end to end --

def _kriging_cov(K, Ks, Kss, X, Xs, z, sigma, sigma0):
    S = K + (sigma0 / sigma) ** 2 * numpy.eye(K.shape[0])
    SiX, Siz, SiK = (numpy.linalg.solve(S, A) for A in (X, z, Ks.T))
    B = X.T @ SiX
    beta = numpy.linalg.solve(B, X.T @ Siz)
    mean = Xs @ beta + SiK.T @ (z - X @ beta)
    r = Xs - (X.T @ SiK).T
    cov = sigma ** 2 * (Kss - Ks @ SiK + r @ numpy.linalg.solve(B, r.T))
    return mean, cov


@pytest.fixture(scope='module')
def grid(gp):
    pts = data.generate_points(16, 2, True)            # the 16 x 16 grid
    z = data.generate_data(pts, 0.2)
    X = data.generate_basis_functions(pts, 1)           # m = 3: 1, x, y
    tst = numpy.random.RandomState(8).rand(40, 2)
    tst[5] = pts[100]
    Xs = data.generate_basis_functions(tst, 1)
    D = gp.generate_correlation(pts, 0.1, 1.5, device_resident=True)
    return pts, z, X, tst, Xs, D


def test_predict_cov_end_to_end(gp, grid, monkeypatch):
    monkeypatch.delenv('GPMI_PREDICT_CHUNK', raising=False)
    monkeypatch.delenv('GPMI_PREDICT_COV_SPLIT', raising=False)
    pts, z, X, tst, Xs, D = grid
    K = D.toarray()
    Ks = gp.generate_cross_correlation(tst, pts, 0.1, 1.5)
    Kss = gp.generate_cross_correlation(tst, tst, 0.1, 1.5)
    hp = (0.8, 0.25)
    s2 = hp[0] ** 2
    g_dev = gp.GaussianProcess(X, D)
    mean, cov = g_dev.predict(tst, Xs, z=z, hyperparam=hp, return_cov=True)
    mean_ref, cov_ref = _kriging_cov(K, Ks, Kss, X, Xs, z, *hp)
    assert cov.shape == (40, 40)
    lam = float(numpy.min(numpy.linalg.eigvalsh(cov)))
    mean0, var = g_dev.predict(tst, Xs, z=z, hyperparam=hp)
    dv = float(numpy.max(numpy.abs(numpy.diag(cov) - var)))
    print('predict cov 16x16: err mean %.3g cov %.3g  max|diag - var| %.3g  min eig %.3g'
          % (_err(mean, mean_ref), _err(cov, cov_ref), dv, lam))
    assert _err(mean, mean_ref) <= 1e-8 and _err(cov, cov_ref) <= 1e-8
    numpy.testing.assert_array_equal(mean, mean0)
    numpy.testing.assert_array_equal(cov, cov.T)
    assert dv <= 1e-10 * s2
    assert lam >= -1e-8 * s2
    # return_var is ignored with return_cov
    mean1, cov1 = g_dev.predict(tst, Xs, z=z, hyperparam=hp, return_cov=True, return_var=False)
    numpy.testing.assert_array_equal(mean1, mean)
    numpy.testing.assert_array_equal(cov1, cov)
    # noise: sigma0^2 on the diagonal only
    mean2, cov2 = g_dev.predict(tst, Xs, z=z, hyperparam=hp, return_cov=True, noise=True)
    numpy.testing.assert_array_equal(mean2, mean)
    numpy.testing.assert_array_equal(cov2, cov + hp[1] ** 2 * numpy.eye(40))
    # K as an ndarray with the kernel parameters: the same bits
    g_host = gp.GaussianProcess(X, K)
    mean3, cov3 = g_host.predict(tst, Xs, z=z, hyperparam=hp, return_cov=True, points=pts,
                                 correlation_scale=0.1, nu=1.5)
    numpy.testing.assert_array_equal(mean3, mean)
    numpy.testing.assert_array_equal(cov3, cov)
    # ... and with the matrices themselves
    mean4, cov4 = g_host.predict(tst, Xs, z=z, hyperparam=hp, return_cov=True, cross=Ks,
                                 cross_star=Kss)
    numpy.testing.assert_array_equal(mean4, mean)
    numpy.testing.assert_array_equal(cov4, cov)
    # return_cov=False: as before, cross_star accepted and unused
    mean5, var5 = g_host.predict(tst, Xs, z=z, hyperparam=hp, cross=Ks, cross_star=Kss)
    numpy.testing.assert_array_equal(mean5, mean0)
    numpy.testing.assert_array_equal(var5, var)


# ------------------------------------------------------------------ errors --

def test_predict_cov_errors(gp, grid):
    from gaussian_proc._mixed_correlation import MixedCorrelation
    pts, z, X, tst, Xs, D = grid
    Ks = gp.generate_cross_correlation(tst, pts, 0.1, 1.5)
    mc = MixedCorrelation(D, imate_method='cholesky')
    with pytest.raises(ValueError):
        mc.predict_cov_terms(0.1, X, z, cross=Ks)              # cross without cross_star
    with pytest.raises(ValueError):
        mc.predict_cov_terms(0.1, X, z)                        # neither points nor cross
    with pytest.raises(ValueError):
        mc.predict_cov_terms(0.1, X, z, cross=Ks, cross_star=numpy.eye(39))
    g = gp.GaussianProcess(X, D)
    with pytest.raises(ValueError):
        g.predict(tst, Xs, z=z, hyperparam=(1.0, 0.1), return_cov=True, cross=Ks)
    with pytest.raises(TypeError):
        g.predict(tst, Xs, z=z, hyperparam=(1.0, 0.1), return_cov=True, cross_start=Ks)
    # sparse K: the CG route is not built
    import scipy.sparse
    sp = MixedCorrelation(scipy.sparse.identity(256, format='csr'), imate_method='slq')
    with pytest.raises(NotImplementedError):
        sp.predict_cov_terms(0.1, X, z, test_points=tst)
    # K = -I is indefinite by construction
    neg = MixedCorrelation(-numpy.eye(256), imate_method='cholesky')
    with pytest.raises(numpy.linalg.LinAlgError):
        neg.predict_cov_terms(0.5, X, z, cross=numpy.zeros((3, 256)), cross_star=numpy.eye(3))


def test_c_abi_status_codes(gp):
    from gaussian_proc import _hip
    lib = _hip.load()
    dp = _hip.dptr
    one = numpy.ones((4, 1))
    sc = numpy.ones(1)
    out = numpy.empty(16)
    cov = numpy.empty((4, 4))
    ks = numpy.zeros((4, 4))

    def call(h, nstar=4, ldcov=4, kstar=None, kss=None, ldkss=4, cov_out=cov):
        return lib.gpmi_op_predict_cov(h, 0.5, dp(one), 1, dp(sc), 0.5, dp(one), nstar,
                                       None if kstar is None else dp(kstar), 4,
                                       None if kss is None else dp(kss), ldkss, dp(out), dp(out),
                                       dp(out), None if cov_out is None else dp(cov_out), ldcov)

    assert call(None) < 0 and 'null handle' in _hip.last_error()
    op = _hip.Operator(4)
    op.load_matrix(numpy.eye(4))
    assert call(op.h) < 0 and 'right-hand' in _hip.last_error()      # no resident RHS
    op.set_rhs(numpy.ones((4, 2)))
    assert call(op.h, nstar=0) < 0
    assert call(op.h, ldcov=3) < 0 and 'ldcov' in _hip.last_error()
    assert call(op.h, kstar=ks) < 0 and 'kss' in _hip.last_error()   # kstar without kss
    assert call(op.h, kstar=ks, kss=ks, ldkss=3) < 0 and 'ldkss' in _hip.last_error()
    assert call(op.h, cov_out=None) < 0
    assert call(op.h) == 0
    # four coincident test points on K = I, eta = 0.5: K** = 1, k* = 1, V V^T = 4 / 1.5
    numpy.testing.assert_allclose(cov, 1.0 - 4.0 / 1.5, rtol=0, atol=1e-14)
    assert call(op.h, kstar=ks, kss=numpy.eye(4)) == 0
    numpy.testing.assert_array_equal(cov, numpy.eye(4))
    ms, fl = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    assert lib.gpmi_op_predict_cov_ms(op.h, ctypes.byref(ms), ctypes.byref(fl)) == 0
    assert ms.value == 0.0 and fl.value == 0.0                        # timing is off
    assert lib.gpmi_op_predict_cov_ms(None, None, None) < 0
    op.set_timing(True)
    assert call(op.h) == 0
    assert lib.gpmi_op_predict_cov_ms(op.h, ctypes.byref(ms), ctypes.byref(fl)) == 0
    assert ms.value > 0.0 and fl.value == 2.0 * 128 ** 3
    op.set_timing(False)
    op.load_matrix(-numpy.eye(4))
    assert call(op.h) == 1                                            # first pivot
