"""Prediction on an MI355X (gfx950): the cross Matérn assembly, the device terms
c_j = R^T S^-1 k*_j, q_j = k*_j^T S^-1 k*_j, G = R^T S^-1 R of the wide forward
substitution (csrc/gpmi_predict.hip) and GaussianProcess.predict above them.

Bars. Cross assembly: those of test_matern_general_nu_vs_scipy_and_exact (2e-14 for the
orders used here). Terms: <= 1e-8 max|reference| against numpy on the device's own K, the
bar the Gram blocks of this factor are held to (__graft_entry__.smoke); at these sizes
cond(K + eta I) <= (n + eta) / eta <= 7e4, so the fp64 forward error is orders below it
(observed maxima: DESIGN section 6). Mean and variance end to end: the same bar, both
being sums of a few such terms with O(1) coefficients.
"""
import ctypes

import numpy
import pytest

from oracle import data, matern

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


def _ref_terms(K, Ks, X, z, eta):
    S = K + eta * numpy.eye(K.shape[0])
    R = numpy.column_stack([X, z])
    SiR = numpy.linalg.solve(S, R)
    return Ks @ SiR, numpy.sum(Ks.T * numpy.linalg.solve(S, Ks.T), axis=0), R.T @ SiR


def _err(a, ref):
    return float(numpy.max(numpy.abs(a - ref)) / numpy.max(numpy.abs(ref)))


# ---------------------------------------------------------------- assembly --

@pytest.mark.parametrize('nu', [0.5, 1.5, 2.5, 0.75, 150.0])
def test_cross_assembly_vs_oracle(gp, nu):
    rng = numpy.random.RandomState(17)
    tol = 2e-14 if nu <= 7.5 or nu >= 100 else 3e-13
    worst = 0.0
    for d in (1, 2, 3):
        scale = [0.15, 0.3, 0.2][:d]
        for n in (1, 130):
            pts = rng.rand(n, d)
            for ns in (1, 65, 129):
                tst = rng.rand(ns, d)
                tst[0] = pts[n // 2]     # a test point that is a training point
                C = gp.generate_cross_correlation(tst, pts, scale, nu)
                assert C.shape == (ns, n)
                ref = matern.matern_kernel(
                    matern.scaled_distance(tst, pts, numpy.asarray(scale)), nu)
                worst = max(worst, float(numpy.max(numpy.abs(C - ref))))
                assert C[0, n // 2] == 1.0
    print('cross assembly nu = %g: max |C - oracle| = %.3g (bar %.0e)' % (nu, worst, tol))
    assert worst <= tol


@pytest.mark.parametrize('nu', [0.5, 1.5, 2.5, 0.75, 150.0])
def test_cross_of_the_training_points_is_K_bit_for_bit(gp, nu):
    rng = numpy.random.RandomState(19)
    for d, n in ((1, 130), (2, 129), (3, 65)):
        pts = rng.rand(n, d)
        scale = [0.15, 0.3, 0.2][:d]
        K = gp.generate_correlation(pts, scale, nu, grid=False)
        C = gp.generate_cross_correlation(pts, pts, scale, nu)
        numpy.testing.assert_array_equal(C, K)


# ------------------------------------------------------------------- terms --

# (n, outer panel width or None for the default, n*, GPMI_PREDICT_CHUNK or None, m + 1)
TERM_CASES = [
    (1, None, 1, None, 1),
    (1, None, 130, None, 4),
    (127, None, 130, None, 4),
    (127, None, 1, None, 16),
    (129, None, 257, None, 16),
    (129, None, 1, None, 1),
    (300, 1, 257, None, 4),
    (300, 2, 130, None, 16),
    (300, None, 257, None, 16),
    (300, None, 257, 128, 4),      # three chunks, the last ragged
    (300, 1, 257, 128, 16),
    (300, 2, 1, None, 1),
    (700, None, 130, None, 4),     # six tile rows: the default panel width (4) is crossed
]


@pytest.mark.parametrize('n,outer,ns,chunk,ncol', TERM_CASES)
def test_terms_vs_numpy_and_cross_route(gp, monkeypatch, n, outer, ns, chunk, ncol):
    if chunk is not None:
        monkeypatch.setenv('GPMI_PREDICT_CHUNK', str(chunk))
    else:
        monkeypatch.delenv('GPMI_PREDICT_CHUNK', raising=False)
    mc, pts, K = _mixed(gp, n)
    if outer is not None:
        mc.op.set_outer(outer)
    X, z = _rhs(pts, ncol)
    tst = numpy.random.RandomState(5).rand(ns, 2)
    tst[ns // 2] = pts[n // 3]
    Ks = gp.generate_cross_correlation(tst, pts, SCALE, NU)
    for eta in (1e-2, 1.0):
        c, q, G = mc.predict_terms(eta, X, z, test_points=tst)
        assert c.shape == (ns, ncol) and q.shape == (ns,) and G.shape == (ncol, ncol)
        c_ref, q_ref, G_ref = _ref_terms(K, Ks, X, z, eta)
        errs = (_err(c, c_ref), _err(q, q_ref), _err(G, G_ref))
        print('terms n=%d outer=%s n*=%d chunk=%s cols=%d eta=%g: err c %.3g q %.3g G %.3g'
              % ((n, outer, ns, chunk, ncol, eta) + errs))
        assert max(errs) <= 1e-8
        # the uploaded-k* route runs the same solve on the same numbers
        c2, q2, G2 = mc.predict_terms(eta, X, z, cross=Ks)
        numpy.testing.assert_array_equal(c2, c)
        numpy.testing.assert_array_equal(q2, q)
        numpy.testing.assert_array_equal(G2, G)


def test_against_solve_and_stale_y(gp):
    """k*^T solve(eta, z) is the z column of c; and a solve between two predictions
    (its backward substitution overwrites the resident L^-1 [X z]) changes no bit."""
    mc, pts, K = _mixed(gp, 300)
    X, z = _rhs(pts, 4)
    tst = numpy.random.RandomState(6).rand(130, 2)
    Ks = gp.generate_cross_correlation(tst, pts, SCALE, NU)
    for eta in (1e-2, 1.0):
        c, q, G = mc.predict_terms(eta, X, z, test_points=tst)
        w = mc.solve(eta, z)
        assert _err(Ks @ w, c[:, 3]) <= 1e-9
        c2, q2, G2 = mc.predict_terms(eta, X, z, test_points=tst)
        numpy.testing.assert_array_equal(c2, c)
        numpy.testing.assert_array_equal(q2, q)
        numpy.testing.assert_array_equal(G2, G)
        # a wide solve (several 16-column passes) in between as well
        mc.solve(eta, Ks.T[:, :40])
        c3, q3, G3 = mc.predict_terms(eta, X, z, test_points=tst)
        numpy.testing.assert_array_equal(c3, c)
        numpy.testing.assert_array_equal(q3, q)
        numpy.testing.assert_array_equal(G3, G)


def test_predict_after_a_solve_that_factorized(gp):
    """The factor cached by a solve was formed beside the solve's right-hand sides, not
    [X z]: the prediction forward-substitutes the resident block itself."""
    mc, pts, K = _mixed(gp, 300)
    X, z = _rhs(pts, 4)
    tst = numpy.random.RandomState(9).rand(65, 2)
    Ks = gp.generate_cross_correlation(tst, pts, SCALE, NU)
    mc.set_rhs(X, z)
    w = mc.solve(0.3, z)
    c, q, G = mc.predict_terms(0.3, X, z, test_points=tst)
    c_ref, q_ref, G_ref = _ref_terms(K, Ks, X, z, 0.3)
    assert max(_err(c, c_ref), _err(q, q_ref), _err(G, G_ref)) <= 1e-8
    assert _err(Ks @ w, c[:, 3]) <= 1e-9


def test_after_a_batched_likelihood_and_a_new_rhs(gp):
    """A batch of several eta leaves only the first one's factor in slot 0; and new
    right-hand sides with the factor still cached are forward-substituted again."""
    mc, pts, K = _mixed(gp, 300, max_batch=2)
    X, z = _rhs(pts, 4)
    tst = numpy.random.RandomState(7).rand(65, 2)
    Ks = gp.generate_cross_correlation(tst, pts, SCALE, NU)
    mc.loglik_terms([0.5, 2.0], X, z)
    for eta in (0.5, 2.0):
        c, q, G = mc.predict_terms(eta, X, z, test_points=tst)
        c_ref, q_ref, G_ref = _ref_terms(K, Ks, X, z, eta)
        assert max(_err(c, c_ref), _err(q, q_ref), _err(G, G_ref)) <= 1e-8
    z2 = numpy.cos(5 * pts[:, 1])
    c, q, G = mc.predict_terms(2.0, X, z2, test_points=tst)
    c_ref, q_ref, G_ref = _ref_terms(K, Ks, X, z2, 2.0)
    assert max(_err(c, c_ref), _err(q, q_ref), _err(G, G_ref)) <= 1e-8


# -------------------------------------------------------------- end to end --

def _kriging(K, Ks, X, Xs, z, sigma, sigma0):
    S = K + (sigma0 / sigma) ** 2 * numpy.eye(K.shape[0])
    SiX, Siz, SiK = (numpy.linalg.solve(S, A) for A in (X, z, Ks.T))
    B = X.T @ SiX
    beta = numpy.linalg.solve(B, X.T @ Siz)
    mean = Xs @ beta + SiK.T @ (z - X @ beta)
    r = Xs - (X.T @ SiK).T
    var = sigma ** 2 * (1.0 - numpy.sum(Ks.T * SiK, axis=0) +
                        numpy.sum(r * numpy.linalg.solve(B, r.T).T, axis=1))
    return mean, var


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


def test_predict_end_to_end(gp, grid):
    pts, z, X, tst, Xs, D = grid
    assert X.shape == (256, 3)
    K = D.toarray()
    Ks = gp.generate_cross_correlation(tst, pts, 0.1, 1.5)
    hp = (0.8, 0.25)
    g_dev = gp.GaussianProcess(X, D)
    mean, var = g_dev.predict(tst, Xs, z=z, hyperparam=hp)
    mean_ref, var_ref = _kriging(K, Ks, X, Xs, z, *hp)
    print('predict 16x16: err mean %.3g var %.3g' % (_err(mean, mean_ref), _err(var, var_ref)))
    assert _err(mean, mean_ref) <= 1e-8 and _err(var, var_ref) <= 1e-8
    assert numpy.all(var >= 0.0)
    # K as an ndarray with the kernel parameters: the same numbers
    g_host = gp.GaussianProcess(X, K)
    mean2, var2 = g_host.predict(tst, Xs, z=z, hyperparam=hp, points=pts,
                                 correlation_scale=0.1, nu=1.5)
    numpy.testing.assert_array_equal(mean2, mean)
    numpy.testing.assert_array_equal(var2, var)
    # noise and return_var
    mean3, var3 = g_dev.predict(tst, Xs, z=z, hyperparam=hp, noise=True)
    numpy.testing.assert_array_equal(mean3, mean)
    numpy.testing.assert_array_equal(var3, var + hp[1] ** 2)
    only = g_dev.predict(tst, Xs, z=z, hyperparam=hp, return_var=False)
    numpy.testing.assert_array_equal(only, mean)


def test_train_then_predict(gp, grid, capsys):
    pts, z, X, tst, Xs, D = grid
    g = gp.GaussianProcess(X, D)
    g.train(z)
    out = capsys.readouterr().out
    assert "'sigma'" in out and "'max_lp'" in out      # train prints as before
    mean, var = g.predict(tst, Xs)
    hp = (g.results['sigma'], g.results['sigma0'])
    mean2, var2 = g.predict(tst, Xs, z=z, hyperparam=hp)
    numpy.testing.assert_array_equal(mean, mean2)
    numpy.testing.assert_array_equal(var, var2)
    assert numpy.all(numpy.isfinite(mean)) and numpy.all(var >= 0.0)


# ------------------------------------------------------------------ errors --

def test_predict_errors(gp, grid):
    from gaussian_proc._mixed_correlation import MixedCorrelation
    pts, z, X, tst, Xs, D = grid
    g = gp.GaussianProcess(X, D)
    with pytest.raises(ValueError):
        g.predict(tst, Xs)                                   # no train, no z / hyperparam
    with pytest.raises(ValueError):
        g.predict(tst, Xs, z=z)                              # ... hyperparam still missing
    with pytest.raises(ValueError):
        g.predict(tst, Xs[:, :2], z=z, hyperparam=(1.0, 0.1))        # X_star shape
    with pytest.raises(ValueError):
        g.predict(tst[:-1], Xs, z=z, hyperparam=(1.0, 0.1))          # X_star rows
    with pytest.raises(ValueError):
        g.predict(numpy.column_stack([tst, tst[:, 0]]), Xs, z=z, hyperparam=(1.0, 0.1))
    with pytest.raises(ValueError):
        gp.generate_cross_correlation(tst[:, :1], pts)       # point dimension
    # an ndarray K carries no kernel parameters
    g_host = gp.GaussianProcess(X, D.toarray())
    with pytest.raises(ValueError):
        g_host.predict(tst, Xs, z=z, hyperparam=(1.0, 0.1))
    # sparse K: the CG route is not built
    import scipy.sparse
    sp = MixedCorrelation(scipy.sparse.identity(256, format='csr'), imate_method='slq')
    with pytest.raises(NotImplementedError):
        sp.predict_terms(0.1, X, z, test_points=tst)
    # K = -I is indefinite by construction
    neg = MixedCorrelation(-numpy.eye(256), imate_method='cholesky')
    with pytest.raises(numpy.linalg.LinAlgError):
        neg.predict_terms(0.5, X, z, cross=numpy.zeros((3, 256)))


def test_c_abi_status_codes(gp):
    from gaussian_proc import _hip
    lib = _hip.load()
    dp = _hip.dptr
    one = numpy.ones((4, 1))
    sc = numpy.ones(1)
    out = numpy.empty(16)

    def call(h, d=1, nstar=4):
        return lib.gpmi_op_predict_terms(h, 0.5, dp(one), d, dp(sc), 0.5, dp(one), nstar, None,
                                         0, dp(out), dp(out), dp(out))

    assert call(None) < 0 and 'null handle' in _hip.last_error()
    op = _hip.Operator(4)
    op.load_matrix(numpy.eye(4))
    assert call(op.h) < 0 and 'right-hand' in _hip.last_error()      # no resident RHS
    op.set_rhs(numpy.ones((4, 2)))
    assert call(op.h, d=0) < 0 and call(op.h, d=9) < 0
    assert call(op.h, nstar=0) < 0
    assert call(op.h) == 0
    tot = ctypes.c_double(-1.0)
    assert lib.gpmi_op_predict_ms(op.h, ctypes.byref(tot), None, None) == 0
    assert tot.value == 0.0                                           # timing is off
    assert lib.gpmi_op_predict_ms(None, None, None, None) < 0
    op.load_matrix(-numpy.eye(4))
    assert call(op.h) == 1                                            # first pivot
