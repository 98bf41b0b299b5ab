"""Prediction on a sparse (tapered Matérn) K on an MI355X: the cross CSR K* of new
points (cell list and all pairs), the terms c = K* S^-1 R, q = diag(K* S^-1 K*^T),
G = R^T S^-1 R from the device-resident CGs, the ``cross=`` route, and
GaussianProcess.predict on a sparse K.

Six small cases (d = 1 .. 4, grids and scattered points, an anisotropic scale, n = 500 ..
729) with 70 new points each (32 + 32 + 6: two full variance blocks and a short one): 60
uniform in [-0.15, 1.15]^d, four training points, two far points, a training point moved by
1e-3 and three duplicates. eta = 5 throughout: the tapered matrices are indefinite
(lambda_min >= -3.49), so cond(K + 5 I) <= 16.

Tolerances: the cross CSR's structure exact and its values <= 4e-16 absolute against the
oracle's Matérn thresholded at tau (the bar of test_sparse_assembly_matches_reference; no
cross value of these cases lies within 1e-4 of tau); c, q, G at CG rtol 1e-10 against
scipy's spsolve to rtol 1e-8 / atol 1e-9 (the bar test_spmm_and_cg sets for the CG they rest
on); the posterior mean and variance to 1e-7 relative at cg_rtol 1e-10 (the mean relative
to its largest entry, since entries of a mean cross zero; the variance, entry by entry,
relative to sigma^2 (1 + |q| + |t|), the terms whose sum it is: the tapered kernel is not
positive semi-definite, so that sum cancels and is negative at some new points of cases B
and C; where the reference variance is positive at every new point, cases A, D, E and F, it
is also held entry by entry to 1e-7 of itself, and that figure is printed for B and C).
"""

import ctypes
import warnings

import numpy
import pytest
import scipy.sparse
import scipy.sparse.linalg

from oracle import data, matern as omat, sparse as osp

pytestmark = pytest.mark.gpu

ETA = 5.0

# name: (training points, scale, nu, density, seed of the new points)
CASES = {
    'A': (lambda: data.generate_points(24, 2, True), 0.08, 1.5, 0.03, 1),
    'B': (lambda: numpy.random.RandomState(2).rand(700, 2), 0.1, 1.5, 0.06, 2),
    'C': (lambda: numpy.random.RandomState(3).rand(600, 1), 0.05, 0.5, 0.05, 3),
    'D': (lambda: data.generate_points(9, 3, True), 0.2, 2.5, 0.05, 4),
    'E': (lambda: numpy.random.RandomState(5).rand(640, 3), [0.2, 0.1, 0.3], 1.5, 0.05, 5),
    'F': (lambda: numpy.random.RandomState(6).rand(500, 4), 0.3, 1.5, 0.05, 6),
}
NAMES = sorted(CASES)
TRAIN_ROWS = slice(60, 64)      # training points 0, 17, n // 2, n - 1
FAR_ROWS = (64, 65)
DUP_ROWS = (slice(67, 70), slice(0, 3))


@pytest.fixture(scope='module')
def gp():
    import gaussian_proc
    from gaussian_proc import _hip
    _hip.require_device(0)
    return gaussian_proc


def new_points(pts, seed):
    n, d = pts.shape
    u = -0.15 + 1.3 * numpy.random.RandomState(seed + 1).rand(60, d)
    return numpy.ascontiguousarray(numpy.vstack([
        u, pts[[0, 17, n // 2, n - 1]], numpy.full((1, d), 1.9), numpy.full((1, d), -1.9),
        pts[5:6] + 1e-3, u[:3]]))


class Case(object):
    """One case's inputs and its host references, computed once and left unchanged."""

    def __init__(self, name):
        make, scale, nu, density, seed = CASES[name]
        self.pts = numpy.ascontiguousarray(make(), dtype=float)
        self.n, self.d = self.pts.shape
        self.scale = omat.broadcast_scale(self.pts, scale)
        self.nu, self.density = nu, density
        self.tau = osp.kernel_threshold(self.n, self.d, density, self.scale, nu)
        self.tp = new_points(self.pts, seed)
        # the oracle's tapered K and K*
        Kd = omat.matern_kernel(omat.scaled_distance(self.pts, self.pts, self.scale), nu)
        Ks = omat.matern_kernel(omat.scaled_distance(self.tp, self.pts, self.scale), nu)
        assert numpy.min(numpy.abs(Ks - self.tau)) > 1e-4
        self.K_ref = numpy.where(Kd > self.tau, Kd, 0.0)
        self.Ks_ref = numpy.where(Ks > self.tau, Ks, 0.0)
        self.empty = numpy.flatnonzero((self.Ks_ref != 0).sum(axis=1) == 0)
        rng = numpy.random.RandomState(100 + seed)
        self.X = numpy.column_stack([numpy.ones(self.n), self.pts])
        self.X_star = numpy.column_stack([numpy.ones(70), self.tp])
        self.z = numpy.sin(3.0 * self.pts.sum(axis=1)) + 0.1 * rng.randn(self.n)
        self.R = numpy.column_stack([self.X, self.z])
        self._sop = None
        self._terms = None

    def sop(self):
        from gaussian_proc import _hip
        if self._sop is None:
            self._sop = _hip.SparseOperator.from_points(self.pts, self.scale, self.nu, self.tau)
        return self._sop

    def terms(self):
        """(c, q, G) of the device at rtol 1e-10 (one call, shared)."""
        if self._terms is None:
            self._terms = self.sop().predict_terms(ETA, self.R, test_points=self.tp, rtol=1e-10)
        return self._terms


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def assert_same_csr(a, b):
    a, b = a.tocsr(), b.tocsr()
    assert a.shape == b.shape
    numpy.testing.assert_array_equal(a.indptr, b.indptr)
    numpy.testing.assert_array_equal(a.indices, b.indices)
    numpy.testing.assert_array_equal(a.data, b.data)


def test_case_facts():
    """What the docstring says of the cases (host only; the other tests lean on it)."""
    for name in NAMES:
        cs = case(name)
        row = (cs.Ks_ref != 0).sum(axis=1)
        assert cs.tp.shape == (70, cs.d)
        assert 4 <= cs.empty.size <= 21 and row.max() <= 26, (name, cs.empty.size, row.max())
        assert set(FAR_ROWS) <= set(cs.empty)
        lam = numpy.linalg.eigvalsh(cs.K_ref)
        assert lam[0] > -3.5 and (lam[-1] + ETA) / (lam[0] + ETA) <= 16.0, (name, lam[0], lam[-1])


@pytest.mark.parametrize('name', NAMES)
def test_cross_csr(gp, name, monkeypatch):
    cs = case(name)
    sop = cs.sop()
    Ks = sop.cross(cs.tp)
    assert Ks.shape == (70, cs.n) and Ks.has_sorted_indices
    ref = scipy.sparse.csr_matrix(cs.Ks_ref)
    numpy.testing.assert_array_equal(Ks.indptr, ref.indptr)
    numpy.testing.assert_array_equal(Ks.indices, ref.indices)
    err = numpy.max(numpy.abs(Ks.data - ref.data))
    print(name, 'cross nnz', Ks.nnz, 'max abs err', err)
    assert err <= 4e-16
    # a new point equal to a training point: that row of K, bit for bit
    K = sop.csr()
    assert_same_csr(Ks[TRAIN_ROWS], K[[0, 17, cs.n // 2, cs.n - 1]])
    # duplicated new points, far points
    assert_same_csr(Ks[DUP_ROWS[0]], Ks[DUP_ROWS[1]])
    for j in FAR_ROWS:
        assert Ks.indptr[j + 1] == Ks.indptr[j]
    # the all-pairs kernels (the variable is read at the call)
    monkeypatch.setenv('GPMI_SPARSE_BRUTE', '1')
    assert_same_csr(sop.cross(cs.tp), Ks)
    monkeypatch.delenv('GPMI_SPARSE_BRUTE')
    # the public spelling, on a DeviceSparseCorrelation's own tau
    if name == 'B':
        D = gp.generate_correlation(cs.pts, cs.scale, cs.nu, sparse=True, density=cs.density,
                                    device_resident=True)
        Kg = gp.generate_cross_correlation(cs.tp, D)
        numpy.testing.assert_array_equal(Kg.indices, ref.indices)
        assert numpy.max(numpy.abs(Kg.data - ref.data)) <= 4e-16


def test_cross_row_over_cell_cap(gp, monkeypatch):
    """Rows with more than 512 kept entries (all 576 here) leave the cell list for the
    all-pairs fall-back: the same CSR."""
    from gaussian_proc import _hip
    cs = case('A')
    scale = numpy.array([10.0, 10.0])
    sop = _hip.SparseOperator.from_points(cs.pts, scale, cs.nu, 1e-3)
    Ks = sop.cross(cs.tp)
    Kd = omat.matern_kernel(omat.scaled_distance(cs.tp, cs.pts, scale), cs.nu)
    ref = scipy.sparse.csr_matrix(numpy.where(Kd > 1e-3, Kd, 0.0))
    assert numpy.diff(Ks.indptr).max() > 512
    numpy.testing.assert_array_equal(Ks.indptr, ref.indptr)
    numpy.testing.assert_array_equal(Ks.indices, ref.indices)
    assert numpy.max(numpy.abs(Ks.data - ref.data)) <= 4e-16
    monkeypatch.setenv('GPMI_SPARSE_BRUTE', '1')
    assert_same_csr(sop.cross(cs.tp), Ks)


@pytest.mark.parametrize('name', NAMES)
def test_predict_terms(gp, name):
    cs = case(name)
    sop = cs.sop()
    c, q, G = cs.terms()
    K, Ks = sop.csr(), sop.cross(cs.tp)
    S = (K + ETA * scipy.sparse.identity(cs.n)).tocsc()
    lu = scipy.sparse.linalg.splu(S)
    Sol = lu.solve(cs.R)
    V = lu.solve(Ks.T.toarray())
    c_ref, G_ref = Ks @ Sol, cs.R.T @ Sol
    q_ref = numpy.asarray(Ks.multiply(V.T).sum(axis=1)).ravel()
    for what, got, ref in (('c', c, c_ref), ('q', q, q_ref), ('G', G, G_ref)):
        print(name, what, 'max abs diff', numpy.max(numpy.abs(got - ref)), 'iterations',
              sop.last_predict_iterations)
        numpy.testing.assert_allclose(got, ref, rtol=1e-8, atol=1e-9)
    assert cs.empty.size >= 4
    assert numpy.all(q[cs.empty] == 0.0) and numpy.all(c[cs.empty] == 0.0)
    c2, q2, G2 = sop.predict_terms(ETA, cs.R, test_points=cs.tp, rtol=1e-10)
    numpy.testing.assert_array_equal(q2, q)
    c3, q3, G3 = sop.predict_terms(ETA, cs.R, test_points=cs.tp, want_q=False, rtol=1e-10)
    assert q3 is None
    numpy.testing.assert_array_equal(c3, c)
    numpy.testing.assert_array_equal(G3, G)
    # the resident block in place of the host one
    sop.set_rhs(cs.R)
    c4, q4, G4 = sop.predict_terms(ETA, None, test_points=cs.tp, rtol=1e-10)
    numpy.testing.assert_array_equal(c4, c)
    numpy.testing.assert_array_equal(q4, q)
    numpy.testing.assert_array_equal(G4, G)


@pytest.mark.parametrize('name', ['B', 'E'])
def test_cross_route(gp, name, monkeypatch):
    """K* given by the caller: bit for bit the geometry route, on the handle that has the
    geometry (locality order) and on a handle made from that K's scipy CSR (original
    order; compared with a geometry handle kept in the original order)."""
    from gaussian_proc import _hip
    from gaussian_proc._mixed_correlation import MixedCorrelation
    cs = case(name)
    sop = cs.sop()
    terms = cs.terms()
    Ks = sop.cross(cs.tp)
    for cross in (Ks, Ks.toarray(), Ks.tocoo()):
        got = sop.predict_terms(ETA, cs.R, cross=cross, rtol=1e-10)
        for a, b in zip(got, terms):
            numpy.testing.assert_array_equal(a, b)
    # a scipy-CSR K
    monkeypatch.setenv('GPMI_SPARSE_REORDER', '0')
    plain = _hip.SparseOperator.from_points(cs.pts, cs.scale, cs.nu, cs.tau)
    monkeypatch.delenv('GPMI_SPARSE_REORDER')
    assert_same_csr(plain.csr(), sop.csr())
    want = plain.predict_terms(ETA, cs.R, test_points=cs.tp, rtol=1e-10)
    mc = MixedCorrelation(sop.csr(), imate_method='slq', imate_options={'cg_rtol': 1e-10})
    for cross in (Ks, Ks.toarray()):
        got = mc.predict_terms(ETA, cs.X, cs.z, cross=cross)
        for a, b in zip(got, want):
            numpy.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError):
        mc.predict_terms(ETA, cs.X, cs.z, test_points=cs.tp)
    with pytest.raises(ValueError):
        mc.sop.predict_terms(ETA, cs.R, test_points=cs.tp)
    with pytest.raises(ValueError):
        mc.sop.cross(cs.tp)
    # unsorted columns: sorted by the Python layer, refused by the C entry
    ri, rd = Ks.indices.copy(), Ks.data.copy()
    for j in range(70):
        a, b = Ks.indptr[j], Ks.indptr[j + 1]
        ri[a:b] = Ks.indices[a:b][::-1]
        rd[a:b] = Ks.data[a:b][::-1]
    rev = scipy.sparse.csr_matrix((rd, ri, Ks.indptr.copy()), shape=Ks.shape)
    assert not rev.has_sorted_indices
    got = sop.predict_terms(ETA, cs.R, cross=rev, rtol=1e-10)
    for a, b in zip(got, terms):
        numpy.testing.assert_array_equal(a, b)
    lib = _hip.load()
    i64p = ctypes.POINTER(ctypes.c_int64)
    ip = numpy.ascontiguousarray(rev.indptr, dtype=numpy.int64)
    dv = numpy.ascontiguousarray(rev.data, dtype=float)
    R = numpy.ascontiguousarray(cs.R)
    s = R.shape[1]
    c, q, G = numpy.empty((70, s)), numpy.empty(70), numpy.empty((s, s))
    it = (ctypes.c_int * 2)()

    def call(ix):
        ix = numpy.ascontiguousarray(ix, dtype=numpy.int32)
        return lib.gpmi_sp_predict_terms_csr(
            sop.h, ETA, _hip.dptr(R), s, s, 70, ip.ctypes.data_as(i64p),
            ix.ctypes.data_as(_hip.c_int_p), _hip.dptr(dv), 1, 1e-10, 1000, _hip.dptr(c),
            _hip.dptr(q), _hip.dptr(G), it)

    assert call(rev.indices) == -1109
    out_of_range = Ks.indices.copy()
    out_of_range[-1] = cs.n
    assert call(out_of_range) == -1109
    # a handle without geometry, and another dimension, at the C entry
    tp = numpy.ascontiguousarray(cs.tp)
    assert lib.gpmi_sp_predict_terms(mc.sop.h, ETA, _hip.dptr(R), s, s, _hip.dptr(tp), 70, cs.d,
                                     1, 1e-10, 1000, _hip.dptr(c), _hip.dptr(q), _hip.dptr(G),
                                     it) == -1108
    assert lib.gpmi_sp_predict_terms(sop.h, ETA, _hip.dptr(R), s, s, _hip.dptr(tp), 70, cs.d + 1,
                                     1, 1e-10, 1000, _hip.dptr(c), _hip.dptr(q), _hip.dptr(G),
                                     it) == -1108
    assert lib.gpmi_sp_cross_matern(sop.h, _hip.dptr(tp), 0, cs.d, None) < 0   # n* = 0
    for rtol, maxiter in ((1e-10, -1), (-1.0, 1000), (float('nan'), 1000)):
        assert lib.gpmi_sp_predict_terms(sop.h, ETA, _hip.dptr(R), s, s, _hip.dptr(tp), 70, cs.d,
                                         1, rtol, maxiter, _hip.dptr(c), _hip.dptr(q),
                                         _hip.dptr(G), it) == -1104
    # a non-empty cross CSR without its columns
    assert lib.gpmi_sp_predict_terms_csr(
        sop.h, ETA, _hip.dptr(R), s, s, 70, ip.ctypes.data_as(i64p), None, None, 1, 1e-10, 1000,
        _hip.dptr(c), _hip.dptr(q), _hip.dptr(G), it) == -1006


@pytest.mark.parametrize('name', NAMES)
def test_gaussian_process_predict(gp, name):
    """GaussianProcess.predict on a sparse K against the universal-kriging formulas
    written out on the dense tapered matrix. Fails without the feature:
    MixedCorrelation._predict_args raises NotImplementedError on a sparse K."""
    cs = case(name)
    sigma = 0.7
    sigma0 = sigma * numpy.sqrt(ETA)
    D = gp.generate_correlation(cs.pts, cs.scale, cs.nu, sparse=True, density=cs.density,
                                device_resident=True)
    g = gp.GaussianProcess(cs.X, D)
    g.likelihood.K_mixed.cg_rtol = 1e-10
    mean, var = g.predict(cs.tp, cs.X_star, z=cs.z, hyperparam=(sigma, sigma0))
    S = cs.K_ref + ETA * numpy.eye(cs.n)
    SiX = numpy.linalg.solve(S, cs.X)
    Siz = numpy.linalg.solve(S, cs.z)
    B = cs.X.T @ SiX
    beta = numpy.linalg.solve(B, cs.X.T @ Siz)
    SiK = numpy.linalg.solve(S, cs.Ks_ref.T)
    mean_ref = cs.X_star @ beta + SiK.T @ (cs.z - cs.X @ beta)
    r = cs.X_star - cs.Ks_ref @ SiX
    q_ref = numpy.sum(cs.Ks_ref * SiK.T, axis=1)
    t_ref = numpy.sum(r * numpy.linalg.solve(B, r.T).T, axis=1)
    var_ref = sigma ** 2 * (1.0 - q_ref + t_ref)
    em = numpy.max(numpy.abs(mean - mean_ref)) / numpy.max(numpy.abs(mean_ref))
    # The tapered kernel is not positive semi-definite, so 1 - q + t cancels and may even be
    # negative (case B): the variance is held to 1e-7 relative to the terms it is the sum
    # of, sigma^2 (1 + |q| + |t|), each of which the device has to 1e-7 relative.
    ev = numpy.max(numpy.abs(var - var_ref) /
                   (sigma ** 2 * (1.0 + numpy.abs(q_ref) + numpy.abs(t_ref))))
    # Entry by entry relative to the reference variance itself: asserted where that is a
    # variance everywhere (positive: A, D, E, F), printed where the sum goes negative (B, C).
    ee = numpy.max(numpy.abs(var - var_ref) / numpy.abs(var_ref))
    print(name, 'mean rel err', em, 'var rel err', ev, 'var entrywise rel err', ee,
          'min var_ref', var_ref.min())
    assert em <= 1e-7 and ev <= 1e-7
    if var_ref.min() > 0.0:
        assert ee <= 1e-7
    mean_only = g.predict(cs.tp, cs.X_star, z=cs.z, hyperparam=(sigma, sigma0),
                          return_var=False)
    numpy.testing.assert_array_equal(mean_only, mean)
    # an empty row of K*: only the trend's uncertainty is left
    re = cs.X_star[cs.empty]
    ve = sigma ** 2 * (1.0 + numpy.sum(re * numpy.linalg.solve(B, re.T).T, axis=1))
    numpy.testing.assert_allclose(var[cs.empty], ve, rtol=1e-7)
    with pytest.raises(NotImplementedError):
        g.predict(cs.tp, cs.X_star, z=cs.z, hyperparam=(sigma, sigma0), return_cov=True)


def test_indefinite_and_maxiter(gp):
    cs = case('A')
    sop = cs.sop()
    with pytest.raises(numpy.linalg.LinAlgError):     # lambda_min(K) = -2.01
        sop.predict_terms(1.0, cs.R, test_points=cs.tp, rtol=1e-10)
    with pytest.warns(RuntimeWarning):
        c, q, G = sop.predict_terms(ETA, cs.R, test_points=cs.tp, rtol=1e-10, maxiter=2)
    assert numpy.all(numpy.isfinite(c)) and numpy.all(numpy.isfinite(q)) and \
        numpy.all(numpy.isfinite(G))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        sop.predict_terms(ETA, cs.R, test_points=cs.tp, rtol=1e-10)   # converges: no warning


def test_cg_unchanged_by_predict(gp):
    """gpmi_sp_cg shares its workspaces with the prediction: the same call before and
    after one returns the same bits."""
    cs = case('B')
    sop = cs.sop()
    Bm = numpy.random.RandomState(7).randn(cs.n, 5)
    before = sop.cg(ETA, Bm, rtol=1e-10)
    sop.predict_terms(ETA, cs.R, test_points=cs.tp, rtol=1e-10)
    after = sop.cg(ETA, Bm, rtol=1e-10)
    numpy.testing.assert_array_equal(after, before)
