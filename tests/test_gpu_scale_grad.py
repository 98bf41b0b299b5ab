"""The likelihood's gradient in the correlation scale on an MI355X (gfx950): the device
terms t_k = tr(A^-1 dK_k), q_k(C) = sum_ij (Sol C Sol^T)_ij dK_k,ij of the fused pass over
the tiles of A^-1 (csrc/gpmi_scale_grad.hip), log_likelihood_der1_scale above them,
DeviceCorrelation.set_correlation_scale and GaussianProcess.train_scale.

Bars. Terms: <= 1e-8 max|reference term| against numpy on the device's own K, the bar the
Gram blocks, the prediction and the leave-one-out terms of this factor are held to (at
these sizes cond(K + eta I) <= (n + eta) / eta <= 6e4 and the reference's own float64
error is about 1e-14). End to end against the numpy formulas: the gradient is
-t_k / 2 + qX_k / 2 + s qc_k / 2, so the bar is 1e-8 (|t_k| + |qX_k| + s |qc_k|) / 2, the
terms' bar carried through. Against central differences of the device's own
log-likelihood on re-assembled K (step 1e-5 rho_k): 1e-6 of the largest component (the
numpy restatement of the formulas meets 1.1e-8 at this step).
"""
import numpy
import pytest

import _scale_grad_ref as ref

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
    """max|device - reference| / max|reference| of t, qX, qc (0 / 0 = 0)."""
    out = []
    for key in ('t', 'qX', 'qc'):
        scale = numpy.max(numpy.abs(R[key]))
        err = numpy.max(numpy.abs(T[key] - R[key]))
        out.append(0.0 if err == 0.0 else err / scale)
    return out


# ------------------------------------------------------------------- terms --

# (n, outer panel width or None, m + 1, d, nu)
TERM_CASES = [
    (127, None, 4, 2, 1.5),      # one tile, with pad
    (129, None, 16, 3, 2.5),     # two tiles, 127 pad rows, full RHS width
    (300, 1, 4, 1, 0.5),         # three tiles, a trinv panel boundary at every tile
    (520, None, 4, 8, 200.0),    # five tiles (a 4-tile k-panel and one more), d = 8, Gaussian
    (520, None, 1, 2, 0.5),      # m = 0
    (260, None, 3, 2, 200.0),
    (260, None, 3, 3, 1.5),
]


@pytest.mark.parametrize('n,outer,ncol,d,nu', TERM_CASES)
def test_terms_vs_numpy(gp, n, outer, ncol, d, nu):
    pts = _points(n, d)
    rho = numpy.array(RHO[d])
    mc, D = _mixed(gp, pts, rho, nu)
    if outer is not None:
        mc.op.set_outer(outer)
    X, z = _rhs(pts, ncol)
    K = D.toarray()
    dK = ref.dcorrelation(pts, rho, nu)
    for eta in (1e-2, 1.0):
        T = mc.scale_grad_terms(eta, X, z)
        R = ref.terms(K, dK, X, z, eta)
        assert T['t'].shape == T['qX'].shape == T['qc'].shape == (d,)
        errs = _term_errs(T, R)
        print('scale grad terms n=%d outer=%s cols=%d d=%d nu=%g eta=%g: err t %.3g qX %.3g '
              'qc %.3g' % ((n, outer, ncol, d, nu, eta) + tuple(errs)))
        assert max(errs) <= 1e-8
        assert abs(T['trinv'] - R['trinv']) <= 1e-8 * abs(R['trinv'])
        if ncol == 1:
            assert numpy.all(T['qX'] == 0.0)      # no basis: C_X = 0


def test_single_point_is_all_zero(gp):
    pts = numpy.array([[0.3, 0.6]])
    mc, D = _mixed(gp, pts, [0.2, 0.3], 1.5)
    T = mc.scale_grad_terms(0.5, numpy.empty((1, 0)), numpy.array([1.7]))
    for key in ('t', 'qX', 'qc'):
        numpy.testing.assert_array_equal(T[key], numpy.zeros(2))


def test_duplicated_points_half_order(gp):
    """x = 0 off the diagonal: the nu = 1/2 form gives 0 there, not NaN."""
    pts = _points(200, 2)
    pts[130:140] = pts[0:10]          # pairs in different tiles
    pts[20:25] = pts[40:45]           # and inside one
    rho = numpy.array(RHO[2])
    mc, D = _mixed(gp, pts, rho, 0.5)
    X, z = _rhs(pts, 4)
    T = mc.scale_grad_terms(0.1, X, z)
    R = ref.terms(D.toarray(), ref.dcorrelation(pts, rho, 0.5), X, z, 0.1)
    assert all(numpy.all(numpy.isfinite(T[k])) for k in ('t', 'qX', 'qc'))
    assert max(_term_errs(T, R)) <= 1e-8


def test_no_coefficients_needs_no_rhs(gp):
    pts = _points(300, 2)
    rho = numpy.array(RHO[2])
    mc, D = _mixed(gp, pts, rho, 1.5)
    assert D.op.nrhs == 0
    t, q = D.op.scale_grad_terms(1e-2, pts, rho, 1.5)
    assert q.shape == (0, 2)
    Ai = numpy.linalg.inv(D.toarray() + 1e-2 * numpy.eye(300))
    t_ref = numpy.array([numpy.sum(Ai * dk) for dk in ref.dcorrelation(pts, rho, 1.5)])
    assert numpy.max(numpy.abs(t - t_ref)) <= 1e-8 * numpy.max(numpy.abs(t_ref))
    # four coefficient matrices, the widest instantiation: q is linear in C
    X, z = _rhs(pts, 4)
    mc.set_rhs(X, z)
    rng = numpy.random.RandomState(8)
    C = rng.randn(4, 4, 4)
    C = C + numpy.transpose(C, (0, 2, 1))
    t4, q4 = D.op.scale_grad_terms(1e-2, pts, rho, 1.5, C)
    numpy.testing.assert_array_equal(t4, t)
    sol = Ai @ numpy.column_stack([X, z])
    dK = ref.dcorrelation(pts, rho, 1.5)
    q_ref = numpy.array([[numpy.sum((sol @ c @ sol.T) * dk) for dk in dK] for c in C])
    assert numpy.max(numpy.abs(q4 - q_ref)) <= 1e-8 * numpy.max(numpy.abs(q_ref))
    t1, q1 = D.op.scale_grad_terms(1e-2, pts, rho, 1.5, C[:1])       # ncoef = 1 of 2
    assert numpy.max(numpy.abs(q1 - q_ref[:1])) <= 1e-8 * numpy.max(numpy.abs(q_ref[:1]))


# ------------------------------------------------------------- bit for bit --

def _gather(T):
    return [T['t'], T['qX'], T['qc'], numpy.array([T['trinv']]), T['sol'], T['G']]


def _same(a, b):
    for x, y in zip(a, b):
        numpy.testing.assert_array_equal(x, y)


def test_repeated_and_after_traceinv2_same_bits(gp):
    eta = 1e-2
    pts = _points(520, 2)
    rho = numpy.array(RHO[2])
    X, z = _rhs(pts, 4)
    mc, _ = _mixed(gp, pts, rho, 1.5)
    a = _gather(mc.scale_grad_terms(eta, X, z))
    _same(_gather(mc.scale_grad_terms(eta, X, z)), a)
    t2 = mc.traceinv(eta, 2)                       # reuses the gradient's tiles
    _same(_gather(mc.scale_grad_terms(eta, X, z)), a)
    mc2, _ = _mixed(gp, pts, rho, 1.5)
    mc2.set_rhs(X, z)
    assert mc2.traceinv(eta, 2) == t2              # tiles built by traceinv itself
    _same(_gather(mc2.scale_grad_terms(eta, X, z)), a)


def test_neighbours_undisturbed(gp):
    """traceinv(eta, 1), traceinv(eta, 2) and loo_terms return the same bits whether or not
    the gradient ran first."""
    eta = 1e-2
    pts = _points(300, 2)
    rho = numpy.array(RHO[2])
    X, z = _rhs(pts, 4)

    def run(with_grad):
        mc, _ = _mixed(gp, pts, rho, 2.5)
        # (resident before the first factorization on both handles: a factorization
        # substitutes the resident block in its own launches, a later block is substituted
        # on its own, and the two round differently)
        mc.set_rhs(X, z)
        if with_grad:
            mc.scale_grad_terms(eta, X, z)
        out = [numpy.array([mc.traceinv(eta, 1), mc.traceinv(eta, 2)])]
        out += list(mc.loo_terms(eta, X, z))
        ld, G = mc.loglik_terms([eta], X, z)
        return out + [ld, G]

    _same(run(True), run(False))


# -------------------------------------------------------------- end to end --

def _device_lps(gp, D, mc, X, z, sigma, sigma0, eta):
    """The device's direct and profiled log-likelihoods as functions of rho (K re-assembled
    in place), restoring the scale afterwards."""
    from gaussian_proc._likelihood._direct_likelihood import DirectLikelihood
    n, m = X.shape
    rho0 = D.correlation_scale.copy()

    def direct(r):
        D.set_correlation_scale(r)
        v = DirectLikelihood.log_likelihood(z, X, mc, False, [sigma, sigma0])
        D.set_correlation_scale(rho0)
        return v

    def profiled(r):
        D.set_correlation_scale(r)
        ld, G = mc.loglik_terms([eta], X, z)
        D.set_correlation_scale(rho0)
        G = G[0]
        zPz = G[m, m] - G[:m, m] @ numpy.linalg.solve(G[:m, :m], G[:m, m])
        return -0.5 * (n - m) * numpy.log(zPz / (n - m)) - 0.5 * ld[0] \
            - 0.5 * numpy.linalg.slogdet(G[:m, :m])[1]

    return direct, profiled


@pytest.mark.parametrize('nu', [0.5, 1.5, 2.5, 200.0])
def test_der1_scale_end_to_end(gp, nu):
    from gaussian_proc._likelihood._direct_likelihood import DirectLikelihood
    from gaussian_proc._likelihood._profile_likelihood import ProfileLikelihood
    n, m = 300, 3
    pts = _points(n, 2)
    rho = numpy.array(RHO[2])
    X, z = _rhs(pts, m + 1)
    sigma, eta = 0.8, 1e-2
    sigma0 = numpy.sqrt(eta) * sigma
    mc, D = _mixed(gp, pts, rho, nu)
    R = ref.terms(D.toarray(), ref.dcorrelation(pts, rho, nu), X, z, eta)
    G = R['G']
    zPz = G[m, m] - G[:m, m] @ numpy.linalg.solve(G[:m, :m], G[:m, m])
    direct, profiled = _device_lps(gp, D, mc, X, z, sigma, sigma0, eta)
    got = {'direct': DirectLikelihood.log_likelihood_der1_scale(z, X, mc, [sigma, sigma0]),
           'profiled': ProfileLikelihood.log_likelihood_der1_scale(z, X, mc, eta)}
    for form, s, lp in (('direct', 1.0 / sigma ** 2, direct),
                        ('profiled', (n - m) / zPz, profiled)):
        want = -0.5 * (R['t'] - R['qX']) + 0.5 * s * R['qc']
        bar = 1e-8 * (numpy.abs(R['t']) + numpy.abs(R['qX']) + s * numpy.abs(R['qc'])) / 2
        fd = ref.central_differences(lp, rho)
        e_fd = numpy.max(numpy.abs(got[form] - fd)) / numpy.max(numpy.abs(fd))
        print('der1_scale %s nu=%g: gradient %s, |err| / bar %s, against central differences '
              '%.3g' % (form, nu, got[form], numpy.abs(got[form] - want) / bar, e_fd))
        assert got[form].shape == (2,)
        assert numpy.all(numpy.abs(got[form] - want) <= bar)
        assert e_fd <= 1e-6
    # the user class, and an ndarray K with the kernel parameters as keywords
    g = gp.GaussianProcess(X, D)
    numpy.testing.assert_array_equal(g.scale_gradient(z=z, hyperparam=(sigma, sigma0)),
                                     got['direct'])
    g2 = gp.GaussianProcess(X, D.toarray())
    numpy.testing.assert_array_equal(
        g2.scale_gradient(z=z, hyperparam=(sigma, sigma0), points=pts, correlation_scale=rho,
                          nu=nu), got['direct'])


# --------------------------------------------------- set_correlation_scale --

@pytest.mark.parametrize('method', ['cholesky', 'eigenvalue'])
def test_set_correlation_scale_equals_fresh(gp, method):
    pts = _points(300, 2)
    X, z = _rhs(pts, 4)
    tst = numpy.random.RandomState(5).rand(7, 2)
    new = numpy.array([0.12, 0.4])
    mc, D = _mixed(gp, pts, RHO[2], 1.5, method)
    # fill every cache from the old K
    mc.loglik_terms([0.1, 1.0], X, z)
    mc.trace(0.0, 2)
    mc.traceinv(0.1, 1)
    mc.predict_terms(0.1, X, z, test_points=tst)
    D.set_correlation_scale(new)
    numpy.testing.assert_array_equal(D.correlation_scale, new)
    mf, Df = _mixed(gp, pts, new, 1.5, method)
    numpy.testing.assert_array_equal(D.toarray(), Df.toarray())
    _same(mc.loglik_terms([0.1, 1.0], X, z), mf.loglik_terms([0.1, 1.0], X, z))
    assert mc.trace(0.0, 1) == mf.trace(0.0, 1) and mc.trace(0.3, 2) == mf.trace(0.3, 2)
    assert mc.traceinv(0.1, 1) == mf.traceinv(0.1, 1)
    _same(mc.predict_terms(0.1, X, z, test_points=tst),
          mf.predict_terms(0.1, X, z, test_points=tst))
    with pytest.raises(ValueError):
        D.set_correlation_scale([0.1, -0.2])
    with pytest.raises(ValueError):
        D.set_correlation_scale([0.1, 0.2, 0.3])


# ------------------------------------------------------------- train_scale --

def _sample(nu, n=300, seed=12):
    """A host-drawn sample with rho = (0.2, 0.3), sigma = 1, sigma0 = 0.1."""
    rng = numpy.random.RandomState(seed)
    pts = rng.rand(n, 2)
    K = ref.correlation(pts, [0.2, 0.3], nu)
    L = numpy.linalg.cholesky(K + 1e-10 * numpy.eye(n))
    X = numpy.column_stack([numpy.ones(n), pts])
    z = X @ numpy.array([0.5, -1.0, 2.0]) + L @ rng.randn(n) + 0.1 * rng.randn(n)
    return pts, X, z


def _fit(gp, nu):
    pts, X, z = _sample(nu)
    D = gp.generate_correlation(pts, [0.1, 0.1], nu, device_resident=True)
    g = gp.GaussianProcess(X, D)
    g.train_scale(z, eta0=1.0)
    return g, D, pts, X, z


@pytest.mark.parametrize('nu', [0.5, 1.5])
def test_train_scale(gp, nu, capsys):
    from gaussian_proc._mixed_correlation import MixedCorrelation
    g, D, pts, X, z = _fit(gp, nu)
    printed = capsys.readouterr().out
    res = g.results
    assert sorted(res) == ['correlation_scale', 'eta', 'evaluations', 'iterations', 'max_lp',
                           'sigma', 'sigma0', 'success']
    assert 'correlation_scale' in printed
    print('train_scale nu=%g: %s' % (nu, res))
    assert res['success']
    assert res['evaluations'] <= 100
    rho_hat, eta_hat = res['correlation_scale'], res['eta']
    numpy.testing.assert_array_equal(D.correlation_scale, rho_hat)
    assert res['sigma0'] == numpy.sqrt(eta_hat) * res['sigma']
    n, m = X.shape

    def lp(rho, eta):
        mc = MixedCorrelation(gp.generate_correlation(pts, rho, nu, device_resident=True),
                              imate_method='cholesky')
        ld, G = mc.loglik_terms([eta], X, z)
        G = G[0]
        zPz = G[m, m] - G[:m, m] @ numpy.linalg.solve(G[:m, :m], G[:m, m])
        return -0.5 * (n - m) * numpy.log(zPz / (n - m)) - 0.5 * ld[0] \
            - 0.5 * numpy.linalg.slogdet(G[:m, :m])[1] - 0.5 * (n - m)

    at_fit = lp(rho_hat, eta_hat)
    assert abs(at_fit - res["max_lp"]) <= 1e-10 * abs(at_fit)
    assert at_fit >= lp(numpy.array([0.1, 0.1]), 1.0)
    assert at_fit >= lp(1.05 * rho_hat, eta_hat) and at_fit >= lp(0.95 * rho_hat, eta_hat)
    # a second run is identical
    g2 = _fit(gp, nu)[0]
    capsys.readouterr()
    for key in res:
        numpy.testing.assert_array_equal(g2.results[key], res[key])
    # predict, leave_one_out and sample work unchanged, and predict equals that of a fresh
    # GaussianProcess built at the fitted scale
    tst = numpy.random.RandomState(13).rand(9, 2)
    Xs = numpy.column_stack([numpy.ones(9), tst])
    mean, var = g.predict(tst, Xs)
    fresh = gp.GaussianProcess(X, gp.generate_correlation(pts, rho_hat, nu,
                                                          device_resident=True))
    mean_f, var_f = fresh.predict(tst, Xs, z=z, hyperparam=(res['sigma'], res['sigma0']))
    numpy.testing.assert_array_equal(mean, mean_f)
    numpy.testing.assert_array_equal(var, var_f)
    loo_mean, loo_var = g.leave_one_out()
    assert numpy.all(numpy.isfinite(loo_mean)) and numpy.all(loo_var > 0.0)
    assert g.sample(tst, Xs, size=2, noise=True).shape == (2, 9)
    assert g.scale_gradient().shape == (2,)


# ------------------------------------------------------------------ errors --

def test_scale_grad_errors(gp):
    from gaussian_proc import _hip
    from gaussian_proc._mixed_correlation import MixedCorrelation
    pts = _points(40, 2)
    X, z = _rhs(pts, 4)
    rho = numpy.array(RHO[2])
    # a general nu: no closed form of the derivative
    mc, D = _mixed(gp, pts, rho, 1.2)
    with pytest.raises(NotImplementedError):
        mc.scale_grad_terms(0.1, X, z)
    with pytest.raises(_hip.GPMIError):
        D.op.scale_grad_terms(0.1, pts, rho, 1.2)
    assert 'general nu' in _hip.last_error()
    # the C entry point's own checks
    lib = _hip.load()
    assert lib.gpmi_op_scale_grad_terms(None, 0.1, None, 2, None, 1.5, None, 0, None, None) < 0
    assert 'null handle' in _hip.last_error()
    assert lib.gpmi_op_scale_grad_ms(None, None, None) < 0
    empty = _hip.Operator(40)
    with pytest.raises(_hip.GPMIError):
        empty.scale_grad_terms(0.1, pts, rho, 1.5)
    assert 'no matrix' in _hip.last_error()
    with pytest.raises(_hip.GPMIError):
        D.op.scale_grad_terms(0.1, pts, rho, 1.5, numpy.zeros((1, 0, 0)))   # no RHS
    assert 'right-hand' in _hip.last_error()
    p9 = numpy.random.RandomState(1).rand(40, 9)
    with pytest.raises(_hip.GPMIError):
        D.op.scale_grad_terms(0.1, p9, numpy.ones(9), 1.5)
    assert 'dimension' in _hip.last_error()
    assert D.op.scale_grad_ms() == dict(pass_ms=0.0, pass_bytes=0.0)
    # sparse K
    import scipy.sparse
    sp = MixedCorrelation(scipy.sparse.identity(256, format='csr'), imate_method='slq')
    with pytest.raises(NotImplementedError):
        sp.scale_grad_terms(0.1, numpy.ones((256, 1)), numpy.arange(256.0))
    # an ndarray K without its points
    nd = MixedCorrelation(D.toarray(), imate_method='cholesky')
    with pytest.raises(ValueError):
        nd.scale_grad_terms(0.1, X, z)
    # train_scale needs a K it can re-assemble
    with pytest.raises(TypeError):
        gp.GaussianProcess(X, D.toarray()).train_scale(z)
    # not positive definite, and the handle still works
    mc15, D15 = _mixed(gp, pts, rho, 1.5)
    with pytest.raises(numpy.linalg.LinAlgError):
        mc15.scale_grad_terms(-2.0, X, z)
    T = mc15.scale_grad_terms(0.5, X, z)
    R = ref.terms(D15.toarray(), ref.dcorrelation(pts, rho, 1.5), X, z, 0.5)
    assert max(_term_errs(T, R)) <= 1e-8
