"""Leave-one-out cross-validation on an MI355X (gfx950): the device terms
dinv = diag(S^-1), sol = S^-1 R, G = R^T S^-1 R of the fused pass over W = L^-T
(csrc/gpmi_loo.hip) and GaussianProcess.leave_one_out / cross_validate above them.

Bars. Terms: <= 1e-8 max|reference| against numpy on the device's own K, the bar the Gram
blocks and the prediction terms of this factor are held to; at these sizes
cond(K + eta I) <= (n + eta) / eta <= 7e4, so the fp64 forward error is orders below it
(observed maxima: DESIGN section 6). sum(dinv) against traceinv(eta, 1): the same W summed
in another order, 1e-12 relative. Two chunk widths: another order again, 1e-13 of the
largest entry. End to end: mean_i = z_i - (Pz)_i / P_ii and var_i = sigma^2 / P_ii divide
terms held to 1e-8 max|term| by P_ii, so to first order the bar is 1e-8 kappa with
kappa = max_i d_i / min_i P_ii from the numpy reference.
"""
import numpy
import pytest

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


def _ref_terms(K, X, z, eta):
    S = K + eta * numpy.eye(K.shape[0])
    R = numpy.column_stack([X, z])
    SiR = numpy.linalg.solve(S, R)
    return numpy.diag(numpy.linalg.inv(S)).copy(), SiR, R.T @ SiR


def _err(a, ref):
    return float(numpy.max(numpy.abs(a - ref)) / numpy.max(numpy.abs(ref)))


def _chunk(monkeypatch, chunk):
    if chunk is not None:
        monkeypatch.setenv('GPMI_LOO_CHUNK', str(chunk))
    else:
        monkeypatch.delenv('GPMI_LOO_CHUNK', raising=False)


# ------------------------------------------------------------------- terms --

# (n, outer panel width or None for the default, GPMI_LOO_CHUNK or None, m + 1)
TERM_CASES = [
    (1, None, None, 1),        # single point
    (127, None, None, 4),      # one tile, with pad
    (129, None, None, 16),     # two tiles, 127 pad rows, full RHS width
    (300, 1, 128, 4),          # three tiles, three chunks, a trinv panel boundary at every tile
    (300, 2, 256, 16),         # chunk boundary not on a panel boundary
    (520, None, 128, 4),       # five tiles, five chunks
    (520, None, None, 1),      # m = 0
]


@pytest.mark.parametrize('n,outer,chunk,ncol', TERM_CASES)
def test_terms_vs_numpy(gp, monkeypatch, n, outer, chunk, ncol):
    _chunk(monkeypatch, chunk)
    mc, pts, K = _mixed(gp, n)
    if outer is not None:
        mc.op.set_outer(outer)
    X, z = _rhs(pts, ncol)
    for eta in (1e-2, 1.0):
        dinv, sol, G = mc.loo_terms(eta, X, z)
        assert dinv.shape == (n,) and sol.shape == (n, ncol) and G.shape == (ncol, ncol)
        d_ref, s_ref, G_ref = _ref_terms(K, X, z, eta)
        errs = (_err(dinv, d_ref), _err(sol, s_ref), _err(G, G_ref))
        print('loo terms n=%d outer=%s chunk=%s cols=%d eta=%g: err dinv %.3g sol %.3g G %.3g'
              % ((n, outer, chunk, ncol, eta) + errs))
        assert max(errs) <= 1e-8
        # the same W, summed tile by tile on the host
        tr = mc.traceinv(eta, 1)
        assert abs(numpy.sum(dinv) - tr) <= 1e-12 * abs(tr)


def test_gram_is_predict_terms_gram_bit_for_bit(gp):
    mc, pts, K = _mixed(gp, 300)
    X, z = _rhs(pts, 4)
    tst = numpy.random.RandomState(5).rand(3, 2)
    for eta in (1e-2, 1.0):
        G = mc.loo_terms(eta, X, z)[2]
        numpy.testing.assert_array_equal(G, mc.predict_terms(eta, X, z, test_points=tst)[2])


# ------------------------------------------------------------- determinism --

def test_repeated_call_and_full_lower_triangle_same_bits(gp, monkeypatch):
    """A second call gives the same bits; and so does a handle on which
    traceinv(eta, 2) ran first, whose W holds tiles of S^-1 below the diagonal tiles."""
    _chunk(monkeypatch, 128)
    eta = 1e-2
    mc, pts, K = _mixed(gp, 520)
    X, z = _rhs(pts, 4)
    d0, s0, G0 = mc.loo_terms(eta, X, z)
    d1, s1, G1 = mc.loo_terms(eta, X, z)
    numpy.testing.assert_array_equal(d1, d0)
    numpy.testing.assert_array_equal(s1, s0)
    numpy.testing.assert_array_equal(G1, G0)
    mc2, _, _ = _mixed(gp, 520)
    mc2.set_rhs(X, z)
    t2 = mc2.traceinv(eta, 2)
    d2, s2, G2 = mc2.loo_terms(eta, X, z)
    numpy.testing.assert_array_equal(d2, d0)
    numpy.testing.assert_array_equal(s2, s0)
    # ... and on the first handle, with the lower triangle filled afterwards
    assert mc.traceinv(eta, 2) == t2
    d3, s3, _ = mc.loo_terms(eta, X, z)
    numpy.testing.assert_array_equal(d3, d0)
    numpy.testing.assert_array_equal(s3, s0)


def test_chunk_widths_agree(gp, monkeypatch):
    """Another chunk width is another summation order: equal to rounding, not bitwise."""
    mc, pts, K = _mixed(gp, 700)
    X, z = _rhs(pts, 4)
    # n_pad = 768: the default is two chunks of 384, 1024 one chunk staged in three
    got = {}
    for chunk in (None, 128, 256, 512, 1024):
        _chunk(monkeypatch, chunk)
        got[chunk] = mc.loo_terms(1e-2, X, z)
    for chunk in (128, 256, 512, 1024):
        ed, es = _err(got[chunk][0], got[None][0]), _err(got[chunk][1], got[None][1])
        print('loo chunk %s against the default: dinv %.3g sol %.3g' % (chunk, ed, es))
        assert ed <= 1e-13 and es <= 1e-13
        numpy.testing.assert_array_equal(got[chunk][2], got[None][2])
    monkeypatch.setenv('GPMI_LOO_CHUNK', '100')            # not a multiple of 128
    from gaussian_proc import _hip
    with pytest.raises(_hip.GPMIError):
        mc.loo_terms(1e-2, X, z)


# ------------------------------------------------------------- neighbours --

def _neighbours(mc, eta, X, z, tst, B):
    c, q, G = mc.predict_terms(eta, X, z, test_points=tst)
    w = mc.solve(eta, B)
    ld, Gl = mc.loglik_terms([eta], X, z)
    return [c, q, G, w, ld, Gl, numpy.array([mc.traceinv(eta, 1), mc.traceinv(eta, 2)])]


def _same(a, b):
    for x, y in zip(a, b):
        numpy.testing.assert_array_equal(x, y)


def _sequence(gp, variant, with_loo):
    """One handle: the neighbours, the variant's step, loo_terms or not, the neighbours
    again. -> (first, second, loo_terms' result and its numpy reference)."""
    eta = 1e-2
    mc, pts, K = _mixed(gp, 300)
    X, z = _rhs(pts, 4)
    tst = numpy.random.RandomState(6).rand(65, 2)
    B = numpy.random.RandomState(7).randn(300, 3)
    first = _neighbours(mc, eta, X, z, tst, B)
    zl = z
    if variant == 'solve_before':
        mc.solve(eta, B)                       # R slot 0 no longer holds L^-1 [X z]
    elif variant == 'new_rhs_between':
        zl = numpy.cos(5 * pts[:, 1])
        mc.set_rhs(X, zl)
    loo = mc.loo_terms(eta, X, zl) if with_loo else None
    return first, _neighbours(mc, eta, X, z, tst, B), loo, _ref_terms(K, X, zl, eta)


@pytest.mark.parametrize('variant', ['plain', 'solve_before', 'new_rhs_between'])
def test_neighbours_undisturbed(gp, variant):
    """predict_terms, solve, loglik_terms and traceinv on a handle return after a
    loo_terms call what they return on a handle that ran the same calls without it, bit
    for bit; and loo_terms itself is right in between."""
    first, second, loo, ref = _sequence(gp, variant, True)
    first0, second0, _, _ = _sequence(gp, variant, False)
    assert max(_err(a, b) for a, b in zip(loo, ref)) <= 1e-8
    _same(first, first0)
    _same(second, second0)
    if variant == 'plain':
        _same(second, first)                   # record, loo_terms, record again


def test_loo_after_a_solve_that_factorized(gp):
    """The factor cached by a solve was formed beside the solve's right-hand sides, not
    [X z]: loo_terms forward-substitutes the resident block itself."""
    mc, pts, K = _mixed(gp, 300)
    X, z = _rhs(pts, 4)
    mc.set_rhs(X, z)
    w = mc.solve(0.3, z)
    dinv, sol, G = mc.loo_terms(0.3, X, z)
    d_ref, s_ref, G_ref = _ref_terms(K, X, z, 0.3)
    assert max(_err(dinv, d_ref), _err(sol, s_ref), _err(G, G_ref)) <= 1e-8
    assert _err(sol[:, 3], w) <= 1e-9


# -------------------------------------------------------------- end to end --

def _refits(K, X, z, sigma, sigma0, noise):
    """n refits: the kriging formulas at point i from the other n - 1 points."""
    n = K.shape[0]
    eta = (sigma0 / sigma) ** 2
    mean, var = numpy.empty(n), numpy.empty(n)
    for i in range(n):
        keep = numpy.arange(n) != i
        S = K[numpy.ix_(keep, keep)] + eta * numpy.eye(n - 1)
        k, Xi, zi = K[i, keep], X[keep], z[keep]
        Sik = numpy.linalg.solve(S, k)
        B = Xi.T @ numpy.linalg.solve(S, Xi)
        beta = numpy.linalg.solve(B, Xi.T @ numpy.linalg.solve(S, zi))
        mean[i] = X[i] @ beta + Sik @ (zi - Xi @ beta)
        r = X[i] - Xi.T @ Sik
        var[i] = sigma ** 2 * (1.0 - k @ Sik + r @ numpy.linalg.solve(B, r)) + \
            (sigma0 ** 2 if noise else 0.0)
    return mean, var


@pytest.fixture(scope='module')
def fitted(gp):
    """n = 129, m = 3, eta = 1e-2: the device K, its refits and kappa."""
    n, sigma = 129, 0.8
    sigma0 = sigma * 0.1
    pts = numpy.random.RandomState(3).rand(n, 2)
    D = gp.generate_correlation(pts, SCALE, NU, device_resident=True)
    K = D.toarray()
    X, z = _rhs(pts, 4)
    refs = {noise: _refits(K, X, z, sigma, sigma0, noise) for noise in (False, True)}
    Si = numpy.linalg.inv(K + (sigma0 / sigma) ** 2 * numpy.eye(n))
    SiX = Si @ X
    P = Si - SiX @ numpy.linalg.solve(X.T @ SiX, SiX.T)
    kappa = float(numpy.max(numpy.diag(Si)) / numpy.min(numpy.diag(P)))
    return D, X, z, (sigma, sigma0), refs, kappa


@pytest.mark.parametrize('noise', [False, True])
def test_leave_one_out_end_to_end(gp, fitted, noise):
    D, X, z, hp, refs, kappa = fitted
    g = gp.GaussianProcess(X, D)
    mean, var = g.leave_one_out(z=z, hyperparam=hp, noise=noise)
    mean_ref, var_ref = refs[noise]
    bar = 1e-8 * kappa
    print('leave_one_out n=129 noise=%s: err mean %.3g var %.3g (kappa %.3g, bar %.3g)'
          % (noise, _err(mean, mean_ref), _err(var, var_ref), kappa, bar))
    assert mean.shape == var.shape == (129,)
    assert _err(mean, mean_ref) <= bar and _err(var, var_ref) <= bar
    assert numpy.all(var > 0.0)
    numpy.testing.assert_array_equal(
        g.leave_one_out(z=z, hyperparam=hp, noise=noise, return_var=False), mean)


def test_cross_validate_end_to_end(gp, fitted):
    """The scores against those of the refits; each bound is the mean's and the variance's
    bar carried through the score's formula to first order."""
    D, X, z, hp, refs, kappa = fitted
    cv = gp.GaussianProcess(X, D).cross_validate(z=z, hyperparam=hp)
    m, v = refs[True]
    r = z - m
    dm, dv = 1e-8 * kappa * numpy.max(numpy.abs(m)), 1e-8 * kappa * numpy.max(numpy.abs(v))
    lpl = numpy.sum(-0.5 * numpy.log(2 * numpy.pi * v) - r ** 2 / (2 * v))
    errs = {
        'residual': numpy.max(numpy.abs(cv['residual'] - r)) / dm,
        'standardized': numpy.max(numpy.abs(cv['standardized'] - r / numpy.sqrt(v)) /
                                  (dm / numpy.sqrt(v) + numpy.abs(r) * dv / (2 * v ** 1.5))),
        'rmse': abs(cv['rmse'] - numpy.sqrt(numpy.mean(r ** 2))) / dm,
        'mean_squared_standardized':
            abs(cv['mean_squared_standardized'] - numpy.mean(r ** 2 / v)) /
            numpy.mean(2 * numpy.abs(r) * dm / v + r ** 2 * dv / v ** 2),
        'log_pseudo_likelihood':
            abs(cv['log_pseudo_likelihood'] - lpl) /
            numpy.sum(dv / (2 * v) + numpy.abs(r) * dm / v + r ** 2 * dv / (2 * v ** 2)),
    }
    print('cross_validate n=129: error / first-order bound: %s'
          % ', '.join('%s %.3g' % kv for kv in sorted(errs.items())))
    assert sorted(cv) == sorted(errs)
    assert max(errs.values()) <= 1.0


def test_train_then_cross_validate(gp, fitted, capsys):
    D, X, z, hp, refs, kappa = fitted
    g = gp.GaussianProcess(X, D)
    g.train(z)
    capsys.readouterr()
    mean, var = g.leave_one_out()
    hp = (g.results['sigma'], g.results['sigma0'])
    mean2, var2 = g.leave_one_out(z=z, hyperparam=hp)
    numpy.testing.assert_array_equal(mean, mean2)
    numpy.testing.assert_array_equal(var, var2)
    cv = g.cross_validate()
    numpy.testing.assert_array_equal(cv['residual'], z - mean)
    assert numpy.all(numpy.isfinite(mean)) and numpy.all(var > 0.0)


# ------------------------------------------------------------------ errors --

def test_loo_errors(gp):
    from gaussian_proc import _hip
    from gaussian_proc._mixed_correlation import MixedCorrelation
    op = _hip.Operator(4)
    op.load_matrix(numpy.eye(4))
    with pytest.raises(_hip.GPMIError):
        op.loo_terms(0.5)                                         # no resident RHS
    assert 'right-hand' in _hip.last_error()
    lib = _hip.load()
    assert lib.gpmi_op_loo_terms(None, 0.5, None, None, 0, None) < 0
    assert 'null handle' in _hip.last_error()
    op.set_rhs(numpy.ones((4, 2)))
    out = numpy.empty(8)
    assert lib.gpmi_op_loo_terms(op.h, 0.5, None, _hip.dptr(out), 1, None) < 0   # ldsol < nrhs
    assert lib.gpmi_op_loo_terms(op.h, 0.5, None, None, 0, None) == 0            # all NULL
    assert op.loo_ms() == dict(pass_ms=0.0, pass_bytes=0.0)                      # timing is off
    assert lib.gpmi_op_loo_ms(None, None, None) < 0
    X = numpy.ones((256, 1))
    z = numpy.arange(256.0)
    # sparse K: not built
    import scipy.sparse
    sp = MixedCorrelation(scipy.sparse.identity(256, format='csr'), imate_method='slq')
    with pytest.raises(NotImplementedError):
        sp.loo_terms(0.1, X, z)
    # n <= m: the leave-one-out fit of beta is undefined
    few = gp.GaussianProcess(numpy.eye(3), numpy.eye(3))
    with pytest.raises(ValueError):
        few.leave_one_out(z=numpy.ones(3), hyperparam=(1.0, 0.1))
    with pytest.raises(ValueError):
        few.cross_validate(z=numpy.ones(3), hyperparam=(1.0, 0.1))
    # K + eta I not positive definite: eta = -2 on a small correlation matrix
    mc, pts, K = _mixed(gp, 40)
    Xs, zs = _rhs(pts, 4)
    with pytest.raises(numpy.linalg.LinAlgError):
        mc.loo_terms(-2.0, Xs, zs)
    # ... and the handle still works
    dinv, sol, G = mc.loo_terms(0.5, Xs, zs)
    assert _err(dinv, _ref_terms(K, Xs, zs, 0.5)[0]) <= 1e-8
