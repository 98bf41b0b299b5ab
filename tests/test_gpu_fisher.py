"""The expected information in (sigma, sigma0, rho) on an MI355X (gfx950): the device's
second-order terms T[a, b] = tr(M_a M_b), U[a] = S^T Y_a, V[a, b] = Y_a^T A^-1 Y_b
(csrc/gpmi_fisher.hip: M_k = A^-1 dK_k on fp64 MFMA from the tiles of A^-1),
DirectLikelihood.fisher_information above them and GaussianProcess.fisher_information,
hyperparam_covariance and standard_errors.

Bars. Terms, against numpy on the device's own K: |T_ab - ref| <= 1e-8 sqrt(ref_aa ref_bb)
(the Cauchy-Schwarz scale: T_ab = <W^T N_a W, W^T N_b W>_F with A^-1 = W W^T), each U[a]
and V[a, b] to 1e-8 of its own block's max|ref|: the bars of the scale-gradient terms of
this factor. numpy's own two inverses (inv, cho_solve) agree to <= 5e-14 (T) and <= 3e-13
(U, V) on these cases. End to end against the direct formula with the projector explicit:
1e-7 of sqrt(I_aa I_bb), the terms' bar through B^-1 and the cancellation in p_ab.
"""
import numpy
import pytest

import _fisher_ref as fref
import _scale_grad_ref as sref

pytestmark = pytest.mark.gpu

RHO = {1: [0.15], 2: [0.2, 0.35], 3: [0.3, 0.2, 0.45],
       8: [0.9, 1.3, 0.7, 1.1, 1.6, 0.8, 1.2, 1.0]}


@pytest.fixture(scope='module')
def gp():
    import gaussian_proc
    from gaussian_proc import _hip
    _hip.require_device(0)
    return gaussian_proc


def _points(n, d, seed=3):
    return numpy.random.RandomState(seed + 10 * d).rand(n, d)


def _rhs(pts, ncol, seed=4):
    """X (n x (ncol - 1)) and z: ncol = m + 1 resident columns."""
    rng = numpy.random.RandomState(seed)
    n = pts.shape[0]
    cols = [numpy.ones(n), pts[:, 0], numpy.sin(2 * pts[:, -1])]
    while len(cols) < ncol - 1:
        cols.append(rng.randn(n))
    X = numpy.column_stack(cols[:ncol - 1]) if ncol > 1 else numpy.empty((n, 0))
    z = numpy.sin(3 * pts[:, 0]) + pts[:, -1] + 0.1 * rng.randn(n)
    return X, z


def _mixed(gp, pts, rho, nu, method='cholesky'):
    from gaussian_proc._mixed_correlation import MixedCorrelation
    D = gp.generate_correlation(pts, rho, nu, device_resident=True)
    return MixedCorrelation(D, imate_method=method), D


def _term_errs(T, R):
    """(T, U, V) errors in units of their bars' scales (0 / 0 = 0)."""
    dg = numpy.diag(R['T'])
    eT = numpy.abs(T['T'] - R['T']) / numpy.sqrt(numpy.outer(dg, dg))

    def blocks(key):
        num = numpy.max(numpy.abs(T[key] - R[key]), axis=(-2, -1))
        den = numpy.max(numpy.abs(R[key]), axis=(-2, -1))
        return numpy.max(numpy.where(num == 0.0, 0.0, num / numpy.where(den > 0, den, 1.0)))

    return float(numpy.max(eT)), float(blocks('U')), float(blocks('V'))


def _check_terms(T, R, d, ncol, tag):
    assert T['T'].shape == (d + 1, d + 1)
    assert T['U'].shape == (d + 1, ncol, ncol)
    assert T['V'].shape == (d + 1, d + 1, ncol, ncol)
    errs = _term_errs(T, R)
    print('fisher terms %s: err T %.3g U %.3g V %.3g' % ((tag,) + errs))
    assert max(errs) <= 1e-8
    numpy.testing.assert_array_equal(T['T'], T['T'].T)


# ------------------------------------------------------------------- terms --

# (n, m + 1, d, nu, eta)
TERM_CASES = [
    (127, 4, 2, 1.5, 0.1),       # one tile, with pad
    (129, 16, 3, 2.5, 0.1),      # two tiles, 127 pad rows, full RHS width
    (300, 4, 1, 0.5, 0.1),       # three tiles
    (520, 4, 8, 200.0, 0.1),     # five tiles, d = 8, Gaussian
    (520, 1, 2, 0.5, 0.1),       # m = 0
    (260, 3, 2, 200.0, 1e-3),    # cond(A) = 7.5e4
]


@pytest.mark.parametrize('n,ncol,d,nu,eta', TERM_CASES)
def test_terms_vs_numpy(gp, n, ncol, d, nu, eta):
    pts = _points(n, d)
    rho = numpy.array(RHO[d])
    mc, D = _mixed(gp, pts, rho, nu)
    X, z = _rhs(pts, ncol)
    T = mc.fisher_terms(eta, X, z)
    R = fref.terms(D.toarray(), sref.dcorrelation(pts, rho, nu), X, z, eta)
    _check_terms(T, R, d, ncol, 'n=%d cols=%d d=%d nu=%g eta=%g' % (n, ncol, d, nu, eta))
    for key in ('t', 'sol', 'G'):
        assert numpy.max(numpy.abs(T[key] - R[key])) <= 1e-8 * numpy.max(numpy.abs(R[key]))
    assert abs(T['trinv'] - R['trinv']) <= 1e-8 * abs(R['trinv'])


def test_single_point(gp):
    pts = numpy.array([[0.3, 0.6]])
    mc, D = _mixed(gp, pts, [0.2, 0.3], 1.5)
    T = mc.fisher_terms(0.5, numpy.empty((1, 0)), numpy.array([1.7]))
    want = numpy.zeros((3, 3))
    want[0, 0] = (1.0 / 1.5) ** 2
    assert abs(T['T'][0, 0] - want[0, 0]) <= 1e-15
    T['T'][0, 0] = want[0, 0]
    numpy.testing.assert_array_equal(T['T'], want)       # T_0k = T_kl = 0
    numpy.testing.assert_array_equal(T['U'][1:], 0.0)
    numpy.testing.assert_array_equal(T['V'][1:], 0.0)
    numpy.testing.assert_array_equal(T['V'][:, 1:], 0.0)


def test_duplicated_points_half_order(gp):
    """x = 0 off the diagonal: the nu = 1/2 form gives 0 there, not NaN."""
    pts = _points(200, 2)
    pts[130:140] = pts[0:10]          # pairs in different tiles
    pts[20:25] = pts[40:45]           # and inside one
    rho = numpy.array(RHO[2])
    mc, D = _mixed(gp, pts, rho, 0.5)
    X, z = _rhs(pts, 4)
    T = mc.fisher_terms(0.1, X, z)
    R = fref.terms(D.toarray(), sref.dcorrelation(pts, rho, 0.5), X, z, 0.1)
    assert all(numpy.all(numpy.isfinite(T[k])) for k in ('T', 'U', 'V'))
    _check_terms(T, R, 2, 4, 'duplicated points')


# ------------------------------------------------------------- bit for bit --

def _gather(T):
    return [T['T'], T['U'], T['V'], T['t'], numpy.array([T['trinv']]), T['sol'], T['G']]


def _same(a, b):
    for x, y in zip(a, b):
        numpy.testing.assert_array_equal(x, y)


def test_repeated_and_after_the_neighbours_same_bits(gp):
    eta = 1e-2
    pts = _points(520, 2)
    rho = numpy.array(RHO[2])
    X, z = _rhs(pts, 4)
    mc, _ = _mixed(gp, pts, rho, 1.5)
    a = _gather(mc.fisher_terms(eta, X, z))
    _same(_gather(mc.fisher_terms(eta, X, z)), a)
    S = mc.scale_grad_terms(eta, X, z)                 # t, trinv, sol, G are its own
    _same([S['t'], numpy.array([S['trinv']]), S['sol'], S['G']], a[3:])
    mc2, _ = _mixed(gp, pts, rho, 1.5)
    mc2.set_rhs(X, z)
    mc2.traceinv(eta, 2)
    mc2.loo_terms(eta, X, z)
    mc2.scale_grad_terms(eta, X, z)
    _same(_gather(mc2.fisher_terms(eta, X, z)), a)


def test_neighbours_undisturbed(gp):
    """traceinv(eta, 1), traceinv(eta, 2), loo_terms and scale_grad_terms return the same
    bits whether or not fisher_terms ran first."""
    eta = 1e-2
    pts = _points(300, 2)
    rho = numpy.array(RHO[2])
    X, z = _rhs(pts, 4)

    def run(with_fisher):
        mc, _ = _mixed(gp, pts, rho, 2.5)
        # (resident before the first factorization on both handles: a factorization
        # substitutes the resident block in its own launches)
        mc.set_rhs(X, z)
        if with_fisher:
            mc.fisher_terms(eta, X, z)
        out = [numpy.array([mc.traceinv(eta, 1), mc.traceinv(eta, 2)])]
        out += list(mc.loo_terms(eta, X, z))
        S = mc.scale_grad_terms(eta, X, z)
        out += [S['t'], S['qX'], S['qc'], S['sol'], S['G']]
        ld, G = mc.loglik_terms([eta], X, z)
        return out + [ld, G]

    _same(run(True), run(False))


# -------------------------------------------------------------- end to end --

def _rel(got, want):
    dg = numpy.diag(want)
    return float(numpy.max(numpy.abs(got - want) / numpy.sqrt(numpy.outer(dg, dg))))


@pytest.mark.parametrize('nu', [0.5, 1.5, 2.5, 200.0])
def test_information_end_to_end(gp, nu):
    n, m = 300, 3
    pts = _points(n, 2)
    rho = numpy.array(RHO[2])
    X, z = _rhs(pts, m + 1)
    sigma, eta = 0.8, 1e-2
    sigma0 = numpy.sqrt(eta) * sigma
    D = gp.generate_correlation(pts, rho, nu, device_resident=True)
    g = gp.GaussianProcess(X, D)
    info = g.fisher_information(z=z, hyperparam=(sigma, sigma0))
    want = fref.information(pts, nu, X, numpy.concatenate([[sigma, sigma0], rho]))
    err = _rel(info, want)
    print('information nu=%g: max |err| / sqrt(I_aa I_bb) = %.3g, diag %s'
          % (nu, err, numpy.diag(info)))
    assert info.shape == (4, 4)
    assert err <= 1e-7
    numpy.testing.assert_array_equal(info, info.T)
    # an ndarray K with the kernel parameters as keywords
    g2 = gp.GaussianProcess(X, D.toarray())
    numpy.testing.assert_array_equal(
        g2.fisher_information(z=z, hyperparam=(sigma, sigma0), points=pts,
                              correlation_scale=rho, nu=nu), info)
    # the covariance and the standard errors
    cov = g.hyperparam_covariance(z=z, hyperparam=(sigma, sigma0))
    cond = numpy.linalg.cond(info)
    resid = numpy.max(numpy.abs(cov @ info - numpy.eye(4)))
    print('covariance nu=%g: |C I - 1| = %.3g, cond %.3g' % (nu, resid, cond))
    assert resid <= 1e-8 * cond
    se = g.standard_errors(z=z, hyperparam=(sigma, sigma0))
    assert sorted(se) == ['correlation_scale', 'sigma', 'sigma0']
    numpy.testing.assert_array_equal(
        numpy.concatenate([[se['sigma'], se['sigma0']], se['correlation_scale']]),
        numpy.sqrt(numpy.diag(cov)))


def test_defaults_of_train_scale(gp, capsys):
    n, nu = 200, 1.5
    pts = _points(n, 2)
    X, z = _rhs(pts, 4)
    D = gp.generate_correlation(pts, RHO[2], nu, device_resident=True)
    g = gp.GaussianProcess(X, D)
    g.train_scale(z, eta0=1.0, maxiter=3, bounds=((1e-2, 1e2), (0.05, 2.0), (0.05, 2.0)))
    capsys.readouterr()
    res = g.results
    info = g.fisher_information()
    theta = numpy.concatenate([[res['sigma'], res['sigma0']], res['correlation_scale']])
    err = _rel(info, fref.information(pts, nu, X, theta))
    print('information at the train_scale result %s: %.3g' % (theta, err))
    assert err <= 1e-7
    numpy.testing.assert_array_equal(
        g.fisher_information(z=z, hyperparam=(res['sigma'], res['sigma0'])), info)
    assert g.standard_errors()['correlation_scale'].shape == (2,)


def test_no_noise_is_singular(gp):
    pts = _points(127, 2)
    X, z = _rhs(pts, 4)
    g = gp.GaussianProcess(X, gp.generate_correlation(pts, RHO[2], 0.5, device_resident=True))
    info = g.fisher_information(z=z, hyperparam=(0.8, 0.0))
    assert numpy.all(info[1] == 0.0)
    with pytest.raises(numpy.linalg.LinAlgError, match='sigma0'):
        g.hyperparam_covariance(z=z, hyperparam=(0.8, 0.0))


# ------------------------------------------------------------------ errors --

def test_fisher_errors(gp):
    from gaussian_proc import _hip
    from gaussian_proc._mixed_correlation import MixedCorrelation
    pts = _points(40, 2)
    X, z = _rhs(pts, 4)
    rho = numpy.array(RHO[2])
    # a general nu: no closed form of the derivative
    mc, D = _mixed(gp, pts, rho, 1.2)
    with pytest.raises(NotImplementedError):
        mc.fisher_terms(0.1, X, z)
    mc.set_rhs(X, z)
    with pytest.raises(_hip.GPMIError):
        D.op.fisher_terms(0.1, pts, rho, 1.2)
    assert 'general nu' in _hip.last_error()
    # the C entry point's own checks
    lib = _hip.load()
    assert lib.gpmi_op_fisher_terms(None, 0.1, None, 2, None, 1.5, None, None, None) == -1006
    assert lib.gpmi_op_fisher_ms(None, None, None) < 0
    p9 = numpy.random.RandomState(1).rand(40, 9)
    s9 = numpy.ones(9)
    assert lib.gpmi_op_fisher_terms(D.op.h, 0.1, _hip.dptr(p9), 9, _hip.dptr(s9), 1.5, None,
                                    None, None) == -1003
    assert 'dimension' in _hip.last_error()
    norhs = gp.generate_correlation(pts, rho, 1.5, device_resident=True)
    assert norhs.op.nrhs == 0
    assert lib.gpmi_op_fisher_terms(norhs.op.h, 0.1, _hip.dptr(pts), 2, _hip.dptr(rho), 1.5,
                                    None, None, None) == -1012
    assert 'right-hand' in _hip.last_error()
    assert norhs.op.fisher_ms() == dict(product_ms=0.0, total_ms=0.0)
    # sparse K
    import scipy.sparse
    sp = MixedCorrelation(scipy.sparse.identity(256, format='csr'), imate_method='slq')
    with pytest.raises(NotImplementedError):
        sp.fisher_terms(0.1, numpy.ones((256, 1)), numpy.arange(256.0))
    # an ndarray K without its points; an unknown keyword
    D15 = gp.generate_correlation(pts, rho, 1.5, device_resident=True)
    nd = gp.GaussianProcess(X, D15.toarray())
    with pytest.raises(ValueError):
        nd.fisher_information(z=z, hyperparam=(0.8, 0.1))
    with pytest.raises(ValueError):
        nd.fisher_information(z=z, hyperparam=(0.8, 0.1), points=pts, nu=1.5)
    g = gp.GaussianProcess(X, D15)
    with pytest.raises(TypeError):
        g.fisher_information(z=z, hyperparam=(0.8, 0.1), cross=numpy.ones((2, 40)))
    with pytest.raises(TypeError):
        g.standard_errors(z=z, hyperparam=(0.8, 0.1), rho=rho)
    with pytest.raises(ValueError):
        g.fisher_information()                            # no train, no z
    # not positive definite, and the handle still works
    mc15 = MixedCorrelation(D15, imate_method='cholesky')
    with pytest.raises(numpy.linalg.LinAlgError):
        mc15.fisher_terms(-2.0, X, z)
    T = mc15.fisher_terms(0.5, X, z)
    R = fref.terms(D15.toarray(), sref.dcorrelation(pts, rho, 1.5), X, z, 0.5)
    _check_terms(T, R, 2, 4, 'after a failed factorization')
