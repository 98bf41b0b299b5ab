"""Draws from a dense factor on an MI355X (gfx950): the device normal generator, the
triangular product Y_t = Xi_t L^T on fp64 MFMA (csrc/gpmi_sample.hip), the hand-over of the
prediction's joint covariance to a second operator, and GaussianProcess.sample above them.

Bars.
Generator: K = I, eta = 0, so L = I exactly and the product adds exact zeros; the draws
must equal gaussian_proc._normal.standard_normals within 1e-13 absolute. sqrt(-2 ln u)
<= 8.6 for u >= 2^-54, and the device's log / cos / sqrt and the rounding of 2 pi u2 differ
from the host's by a few ulp of that, < 1e-14: a margin of 10.
Product: against numpy.linalg.cholesky(K + eta I) @ xi, per draw j
  ||got_j - ref_j||_2 <= 64 n eps cond(K + eta I) ||L||_2 ||xi_j||_2,
the forward error of a Cholesky factor (n eps cond ||L||, Higham 10.7) carried through a
product of depth n, with 64 for the constants. What the factorization leaves above the
diagonal of a diagonal tile is zero in this build (diag_block_kernel zeroes it on load
and on store; every diagonal tile goes through it last), so a leak past the mask would
add exact zeros today: the n = 129 and 300 cases pin the product's indexing across tile
rows, and the mask stays for a factorization that leaves something else there.
Covariance hand-over: bit for bit C0 at m = 0; at m = 2 within 4 m eps (|U| |U|^T) of
C0 + U U^T, with U chosen of entries 1 <= |u| < 2: the bound has no |C0| term, so the
partial sums it majorises must be dominated by the trend term (|C0| <= 1 <= |U| |U|^T).
Moments: 5 standard errors, after the host restatement passed at 4 on the same numbers.
Indexing: the piece depth of the product depends on the number of draw tiles, so calls
that differ in size or chunk width are compared to the product's rounding bound, not bit
for bit; the same call twice is bit-identical.
"""
import numpy
import pytest

from oracle import data

pytestmark = pytest.mark.gpu

SCALE, NU = 0.2, 1.5
EPS = numpy.finfo(float).eps


@pytest.fixture(scope='module')
def gp():
    import gaussian_proc
    from gaussian_proc import _hip
    _hip.require_device(0)
    return gaussian_proc


def _setenv(monkeypatch, name, value):
    if value is not None:
        monkeypatch.setenv(name, str(value))
    else:
        monkeypatch.delenv(name, raising=False)


# --------------------------------------------------------------- generator --

@pytest.mark.parametrize('n', [1, 127, 129])
@pytest.mark.parametrize('size', [1, 130])
@pytest.mark.parametrize('first', [0, 7])
def test_generator_matches_host_restatement(gp, monkeypatch, n, size, first):
    from gaussian_proc import _hip
    from gaussian_proc._normal import standard_normals
    _setenv(monkeypatch, 'GPMI_SAMPLE_CHUNK', None)
    _setenv(monkeypatch, 'GPMI_SAMPLE_DEPTH', None)
    op = _hip.Operator(n)
    op.load_matrix(numpy.eye(n))
    got = op.sample(0.0, size, seed=11, first=first)
    ref = standard_normals(11, first, n, size).T
    assert got.shape == (size, n)
    err = float(numpy.max(numpy.abs(got - ref)))
    print('generator n=%d size=%d first=%d: max |device - host| %.3g' % (n, size, first, err))
    assert err <= 1e-13
    op.close()


# ----------------------------------------------------------------- product --

@pytest.fixture(scope='module')
def matern(gp):
    """n -> (MixedCorrelation on a device Matérn K, its numpy factor of K + 0.5 I, the
    norm and condition number that go into the bound), computed once."""
    from gaussian_proc._mixed_correlation import MixedCorrelation
    out = {}
    for n in (1, 128, 129, 300):
        pts = numpy.random.RandomState(n).rand(n, 2)
        D = gp.generate_correlation(pts, SCALE, NU, device_resident=True)
        S = D.toarray() + 0.5 * numpy.eye(n)
        L = numpy.linalg.cholesky(S)
        out[n] = (MixedCorrelation(D, imate_method='cholesky'), L,
                  float(numpy.linalg.norm(L, 2)), float(numpy.linalg.cond(S)))
    return out


def _product_bound(n, cond, normL, xi):
    """Per draw (column of xi): 64 n eps cond ||L|| ||xi_j||."""
    return 64.0 * n * EPS * cond * normL * numpy.linalg.norm(xi, axis=0)


def _check_product(got, L, xi, n, cond, normL, what):
    ref = (L @ xi).T
    err = numpy.linalg.norm(got - ref, axis=1)
    bound = _product_bound(n, cond, normL, xi)
    print('%s: max ||got - ref|| %.3g, max over draws of error / bound %.3g'
          % (what, err.max(), (err / bound).max()))
    assert numpy.all(err <= bound)


# depth: GPMI_SAMPLE_DEPTH (None: the plan's choice; 99: clipped to nt, unsplit)
@pytest.mark.parametrize('n', [1, 128, 129, 300])
@pytest.mark.parametrize('size', [1, 129, 260])
@pytest.mark.parametrize('depth', [None, 2, 99])
def test_product_vs_numpy(gp, matern, monkeypatch, n, size, depth):
    _setenv(monkeypatch, 'GPMI_SAMPLE_CHUNK', None)
    _setenv(monkeypatch, 'GPMI_SAMPLE_DEPTH', depth)
    mc, L, normL, cond = matern[n]
    xi = numpy.random.RandomState(1000 + size).randn(n, size)
    got = mc.sample(0.5, size=size, xi=xi)
    assert got.shape == (size, n)
    _check_product(got, L, xi, n, cond, normL, 'product n=%d size=%d depth=%s' % (n, size, depth))


# -------------------------------------------------------- load_predict_cov --

@pytest.fixture(scope='module')
def parent(gp):
    """A 200-point operator with [X | z] resident (m = 2), and test points."""
    from gaussian_proc import _hip
    rng = numpy.random.RandomState(21)
    pts = rng.rand(200, 2)
    D = gp.generate_correlation(pts, SCALE, NU, device_resident=True)
    R = numpy.column_stack([numpy.ones(200), pts[:, 0], numpy.sin(3 * pts[:, 0]) + pts[:, 1]])
    D.op.set_rhs(R)
    return D, pts, rng.rand(130, 2)


@pytest.mark.parametrize('nstar', [1, 130])
@pytest.mark.parametrize('m', [0, 2])
def test_load_predict_cov(gp, parent, nstar, m):
    from gaussian_proc import _hip
    D, pts, tst = parent
    tst = tst[:nstar]
    kw = dict(test_points=tst, points=pts, scale=numpy.full(2, SCALE), nu=NU)
    eta = 0.05
    c, q, G, C0 = D.op.predict_cov(eta, **kw)
    c1, q1, G1 = D.op.predict_cov_resident(eta, **kw)
    for a, b in ((c, c1), (q, q1), (G, G1)):
        numpy.testing.assert_array_equal(a, b)
    rng = numpy.random.RandomState(5)
    U = (1.0 + rng.rand(nstar, m)) * numpy.where(rng.rand(nstar, m) < 0.5, -1.0, 1.0)
    child = _hip.Operator(nstar)
    gen = child.generation
    child.load_predict_cov(D.op, U)
    assert child.generation == gen + 1
    got = child.get_matrix()
    numpy.testing.assert_array_equal(got, got.T)
    if m == 0:
        numpy.testing.assert_array_equal(got, C0)
        child.load_predict_cov(D.op)          # U left out: the same
        numpy.testing.assert_array_equal(child.get_matrix(), C0)
    else:
        ref = C0 + U @ U.T
        bound = 4.0 * m * EPS * (numpy.abs(U) @ numpy.abs(U).T)
        err = numpy.abs(got - ref)
        print('load_predict_cov n*=%d m=%d: max err %.3g, max err / bound %.3g'
              % (nstar, m, err.max(), (err / bound).max()))
        assert numpy.all(err <= bound)
    # the loaded matrix is the child's K: its draws are those of numpy's factor
    if nstar > 1:
        S = got + 0.1 * numpy.eye(nstar)
        L = numpy.linalg.cholesky(S)
        xi = numpy.random.RandomState(6).randn(nstar, 3)
        _check_product(child.sample(0.1, 3, xi=xi), L, xi, nstar, float(numpy.linalg.cond(S)),
                       float(numpy.linalg.norm(L, 2)), 'child n*=%d m=%d' % (nstar, m))
    child.close()


def test_load_predict_cov_errors(gp, parent):
    from gaussian_proc import _hip
    D, pts, tst = parent
    D.op.predict_cov_resident(0.05, test_points=tst, points=pts, scale=numpy.full(2, SCALE),
                              nu=NU)
    wrong = _hip.Operator(129)
    with pytest.raises(_hip.GPMIError):
        wrong.load_predict_cov(D.op)                     # resident C0 is of 130 points
    assert 'resident covariance is of 130' in _hip.last_error()
    fresh = _hip.Operator(130)
    with pytest.raises(_hip.GPMIError):
        wrong.load_predict_cov(fresh)                    # nothing resident
    assert 'no resident covariance' in _hip.last_error()
    right = _hip.Operator(130)
    with pytest.raises(ValueError):
        right.load_predict_cov(D.op, numpy.ones((129, 1)))
    with pytest.raises(_hip.GPMIError):
        right.load_predict_cov(D.op, numpy.ones((130, 16)))   # m above 15
    lib = _hip.load()
    assert lib.gpmi_op_load_predict_cov(None, D.op.h, None, 0, 0) < 0
    assert lib.gpmi_op_load_predict_cov(right.h, D.op.h, _hip.dptr(numpy.ones((130, 2))), 1, 2) < 0
    assert 'ldu' in _hip.last_error()
    # a call that has no matrix yet, and the C-level argument checks of the draws
    out = numpy.empty((2, 130))
    assert lib.gpmi_op_sample(right.h, 0.0, None, 0, 0, 0, 2, _hip.dptr(out), 130) < 0
    assert 'no matrix' in _hip.last_error()
    right.load_predict_cov(D.op)
    assert lib.gpmi_op_sample(None, 0.0, None, 0, 0, 0, 2, _hip.dptr(out), 130) < 0
    assert lib.gpmi_op_sample(right.h, 0.5, None, 0, 0, 0, 0, _hip.dptr(out), 130) < 0
    assert lib.gpmi_op_sample(right.h, 0.5, None, 0, 0, 0, 2, _hip.dptr(out), 129) < 0
    assert 'ldout' in _hip.last_error()
    assert lib.gpmi_op_sample(right.h, 0.5, _hip.dptr(out), 1, 0, 0, 2, _hip.dptr(out), 130) < 0
    assert 'ldxi' in _hip.last_error()
    assert lib.gpmi_op_sample(right.h, 0.5, None, 0, 0, 0, 2, _hip.dptr(out), 130) == 0
    assert right.sample_ms() == dict(normal_ms=0.0, trmm_ms=0.0, trmm_flops=0.0)
    right.set_timing(True)
    right.sample(0.5, 2)
    t = right.sample_ms()
    assert t['normal_ms'] > 0.0 and t['trmm_ms'] > 0.0 and t['trmm_flops'] == 2.0 * 128 ** 3 * 3
    for op in (wrong, fresh, right):
        op.close()


# -------------------------------------------------------------- end to end --

@pytest.fixture(scope='module')
def model(gp):
    rng = numpy.random.RandomState(31)
    pts = rng.rand(200, 2)
    z = numpy.sin(3 * pts[:, 0]) + pts[:, 1] + 0.1 * rng.randn(200)
    X = numpy.column_stack([numpy.ones(200), pts[:, 0]])       # m = 2
    tst = rng.rand(130, 2)
    Xs = numpy.column_stack([numpy.ones(130), tst[:, 0]])
    D = gp.generate_correlation(pts, SCALE, NU, device_resident=True)
    return gp.GaussianProcess(X, D), z, tst, Xs, (0.8, 0.25)


def _check_draws(draws, mean, cov, xi, what):
    L = numpy.linalg.cholesky(cov)
    n = cov.shape[0]
    ref = mean[None, :] + (L @ xi).T
    err = numpy.linalg.norm(draws - ref, axis=1)
    bound = _product_bound(n, float(numpy.linalg.cond(cov)), float(numpy.linalg.norm(L, 2)), xi)
    print('%s: cond %.3g, max ||draw - ref|| %.3g, max error / bound %.3g'
          % (what, numpy.linalg.cond(cov), err.max(), (err / bound).max()))
    assert numpy.all(err <= bound)


def test_sample_end_to_end(gp, model, monkeypatch):
    _setenv(monkeypatch, 'GPMI_SAMPLE_CHUNK', None)
    _setenv(monkeypatch, 'GPMI_SAMPLE_DEPTH', None)
    g, z, tst, Xs, hp = model
    xi = numpy.random.RandomState(32).randn(130, 5)
    mean, cov = g.predict(tst, Xs, z=z, hyperparam=hp, return_cov=True, noise=True)
    draws, mean_s = g.sample(tst, Xs, size=5, z=z, hyperparam=hp, noise=True, xi=xi,
                             return_mean=True)
    assert draws.shape == (5, 130)
    numpy.testing.assert_array_equal(mean_s, mean)
    _check_draws(draws, mean, cov, xi, 'end to end, noise')
    numpy.testing.assert_array_equal(
        draws, g.sample(tst, Xs, size=5, z=z, hyperparam=hp, noise=True, xi=xi))
    # the latent function, with a jitter
    mean0, cov0 = g.predict(tst, Xs, z=z, hyperparam=hp, return_cov=True)
    draws0 = g.sample(tst, Xs, size=5, z=z, hyperparam=hp, jitter=1e-8, xi=xi)
    _check_draws(draws0, mean0, cov0 + hp[0] ** 2 * 1e-8 * numpy.eye(130), xi,
                 'end to end, jitter 1e-8')


MOMENT_SEED = 1


def _moments_ok(dev, cov, size, k):
    """Second moments about zero and means of the centred draws within k standard errors."""
    S = dev.T @ dev / size
    d = numpy.diag(cov)
    se = numpy.sqrt((numpy.outer(d, d) + cov ** 2) / size)
    zc = float(numpy.max(numpy.abs(S - cov) / se))
    zm = float(numpy.max(numpy.abs(dev.mean(axis=0)) / numpy.sqrt(d / size)))
    return zc, zm, zc <= k and zm <= k


def test_sample_moments(gp, model, monkeypatch):
    from gaussian_proc._normal import standard_normals
    _setenv(monkeypatch, 'GPMI_SAMPLE_CHUNK', None)
    _setenv(monkeypatch, 'GPMI_SAMPLE_DEPTH', None)
    g, z, tst, Xs, hp = model
    tst, Xs, size = tst[:8], Xs[:8], 4096
    mean, cov = g.predict(tst, Xs, z=z, hyperparam=hp, return_cov=True, noise=True)
    # the host restatement on numpy's factor passes at 4 standard errors (the seed was
    # chosen for that on the CPU, from the same inputs through the oracle's Matérn), so
    # the device's rounding does not decide the test at 5
    host = (numpy.linalg.cholesky(cov) @ standard_normals(MOMENT_SEED, 0, 8, size)).T
    zc, zm, ok = _moments_ok(host, cov, size, 4.0)
    print('moments, host restatement: covariance %.3g se, mean %.3g se' % (zc, zm))
    assert ok
    draws, mean_s = g.sample(tst, Xs, size=size, seed=MOMENT_SEED, z=z, hyperparam=hp, noise=True,
                             return_mean=True)
    zc, zm, ok = _moments_ok(draws - mean_s[None, :], cov, size, 5.0)
    print('moments, device: covariance %.3g se, mean %.3g se' % (zc, zm))
    assert ok


# ------------------------------------------------ indexing, repeatability --

def test_indexing_and_repeatability(gp, matern, monkeypatch):
    from gaussian_proc._normal import standard_normals
    _setenv(monkeypatch, 'GPMI_SAMPLE_CHUNK', None)
    _setenv(monkeypatch, 'GPMI_SAMPLE_DEPTH', None)
    n = 300
    mc, L, normL, cond = matern[n]
    four = mc.sample(0.5, size=4, seed=9, first=0)
    three = mc.sample(0.5, size=3, seed=9, first=1)
    # the rounding bound of the product, twice (either side is within one of the exact one)
    b4 = 2.0 * _product_bound(n, cond, normL, standard_normals(9, 0, n, 4))
    err = numpy.linalg.norm(three - four[1:4], axis=1)
    print('first=1 against rows 1..3: max diff %.3g (bound %.3g)' % (err.max(), b4[1:4].min()))
    assert numpy.all(err <= b4[1:4])
    _check_product(four, L, standard_normals(9, 0, n, 4), n, cond, normL, 'device normals')
    numpy.testing.assert_array_equal(four, mc.sample(0.5, size=4, seed=9, first=0))
    # chunk width
    wide = mc.sample(0.5, size=260, seed=9)
    monkeypatch.setenv('GPMI_SAMPLE_CHUNK', '128')
    narrow = mc.sample(0.5, size=260, seed=9)
    numpy.testing.assert_array_equal(narrow, mc.sample(0.5, size=260, seed=9))
    b = 2.0 * _product_bound(n, cond, normL, standard_normals(9, 0, n, 260))
    err = numpy.linalg.norm(wide - narrow, axis=1)
    print('chunk 128 against the default: max diff %.3g (bound %.3g)' % (err.max(), b.min()))
    assert numpy.all(err <= b)
    monkeypatch.setenv('GPMI_SAMPLE_CHUNK', '100')
    from gaussian_proc import _hip
    with pytest.raises(_hip.GPMIError):
        mc.sample(0.5, size=2)


# ------------------------------------------------------------------ errors --

def test_sample_errors(gp, model):
    from gaussian_proc._mixed_correlation import MixedCorrelation
    g, z, tst, Xs, hp = model
    # every test point twice: the latent covariance is singular
    twice = numpy.vstack([tst[:65], tst[:65]])
    Xs2 = numpy.vstack([Xs[:65], Xs[:65]])
    with pytest.raises(numpy.linalg.LinAlgError) as e:
        g.sample(twice, Xs2, size=2, z=z, hyperparam=hp)
    assert 'jitter=' in str(e.value) and 'noise=True' in str(e.value)
    assert g.sample(twice, Xs2, size=2, z=z, hyperparam=hp, noise=True).shape == (2, 130)
    assert g.sample(twice, Xs2, size=2, z=z, hyperparam=hp, jitter=1e-6).shape == (2, 130)
    with pytest.raises(ValueError):
        g.sample(tst, Xs, size=0, z=z, hyperparam=hp)
    with pytest.raises(ValueError):
        g.sample(tst, Xs, size=2, z=z, hyperparam=hp, xi=numpy.zeros((130, 3)))
    with pytest.raises(ValueError):
        g.sample(tst, Xs, size=2, z=z, hyperparam=hp, jitter=-1e-9)
    with pytest.raises(TypeError):
        g.sample(tst, Xs, size=2, z=z, hyperparam=hp, jiter=1e-9)
    untrained = gp.GaussianProcess(g.X, g.K)
    with pytest.raises(ValueError):
        untrained.sample(tst, Xs)
    import scipy.sparse
    sp = MixedCorrelation(scipy.sparse.identity(256, format='csr'), imate_method='slq')
    with pytest.raises(NotImplementedError):
        sp.sample(0.1, size=2)
    with pytest.raises(NotImplementedError):
        sp.posterior_sample_terms(0.1, numpy.ones((256, 1)), numpy.ones(256), test_points=tst)
    neg = MixedCorrelation(-numpy.eye(4), imate_method='cholesky')
    with pytest.raises(numpy.linalg.LinAlgError):
        neg.sample(0.5, size=1)
