"""Each stage of the dense path held to a backward-error bar of its own, on what the
device left in memory: the factor L (Operator.factor), W = L^-T (trinv) and A^-1
(inverse), read back after the calls that build them, and the solves and logdet beside
them. The metrics and the host arithmetic that evaluates them are in _backward.py
(test_backward_host.py shows what they can see); none of the bars depends on cond(A),
and a failure names the stage and the 128-tile.

The device assembles K itself (assemble_matern), so the Matern kernel and the shift copy
are in the chain; A = K_device + eta I is formed on the host from get_matrix(), so the
assembly's few-ulp difference from the oracle is not counted against the factor.

Shapes (Matern 3/2, scale 0.2, eta 0.03): the smallest that reach every launch kind, as in
test_gpu_dense_kloop.py:
  300, outer 16    3 tile rows, ragged last tile; band SYRK kdim 128; no bulk update
  1000, outer 4    bulk update reading C from K, grouped tile order
  1100, outer 4    a second bulk update from the member copy; one-column last panel
  1100, outer 1    every bulk update at kdim 128
  2100, outer 16   band kdim 128 ... 1024, 17 tile rows; traceinv_build_w's bulk
                   trinv_update_kernel (ke < nt) at the default outer width
GPMI_PANEL=rec and col at the first three; GPMI_KLOOP=late at (1000, 4) only.
Conditioning ladder at n = 300, outer 16 (LADDER below): cond(A) 5.5e3 ... 1.8e12, kappa_max
of the diagonal tiles 48 ... 8.8e5.

Bars (u = 2^-53; `ref` is _backward.blocked_reference, the device's algorithm in numpy, on
the same A; none is taken from the code under test):
  cholesky   omega_chol <= max((n + 1) u, 16 omega_chol(ref)), the margin of 16 for the
             device's other summation order (MFMA 16x16x4 chains, the 16-blocked diagonal
             tile with rsq + Newton pivots); and <= (n + 1) u (1 + kappa_max), the first-order
             ceiling of a panel formed with an explicit inverse
  inverse    omega_inv <= max((n + 1) u, 16 omega_inv(ref))
  A^-1       omega_gram <= (n_pad + 1) u on the W the device returned (a plain product)
  solve      omega_solve <= (3 n + 1) u max(1, 16 omega_chol(ref) / ((n + 1) u)) (Higham
             10.4 with the reference's ratio), one column and 37 columns, on a fresh
             factorization (fused forward substitution) and on the cached factor
  logdet     |logdet - 2 sum log l_ii| <= (n + 2) u 2 sum |log l_ii|, the sum in longdouble
  traces     traceinv(eta, 1) = ||W||_F^2 and traceinv(eta, 2) = ||A^-1||_F^2 of the arrays
             read back, (n + 2) u relative; diag(A^-1) = loo_terms' diagonal, 4 (n + 1) u
Measured values: DESIGN section 6 (the tests print them under -s).
"""

import ctypes

import numpy
import pytest

import _backward as bw

pytestmark = pytest.mark.gpu

U = bw.U
ETA = 0.03
# (nu, scale, eta); nu = 100 is the Gaussian limit
LADDER = [(1.5, 0.2, 1e-2), (2.5, 0.2, 1e-6), (2.5, 1.0, 1e-6), (2.5, 1.0, 1e-10),
          (100, 0.5, 1e-10)]

# (n, outer, GPMI_PANEL, GPMI_KLOOP or None, ladder rung or None)
SHAPES = [(300, 16, 'rec', None, None), (300, 16, 'col', None, None),
          (1000, 4, 'rec', None, None), (1000, 4, 'col', None, None),
          (1000, 4, 'rec', 'late', None),
          (1100, 4, 'rec', None, None), (1100, 4, 'col', None, None),
          (1100, 1, 'rec', None, None),
          (2100, 16, 'rec', None, None)]
RUNGS = [(300, 16, 'rec', None, r) for r in range(len(LADDER))]
CASES = SHAPES + RUNGS


def _id(case):
    n, outer, panel, kloop, rung = case
    return 'rung%d' % rung if rung is not None else \
        '%d-%d-%s%s' % (n, outer, panel, '-' + kloop if kloop else '')


_CACHE = {}


def _inputs(n):
    """Points, [X | z] and a 37-column block for size n: computed once, never modified."""
    if n not in _CACHE:
        rng = numpy.random.RandomState(n)
        pts = rng.rand(n, 2)
        X = numpy.column_stack([numpy.ones(n), pts])
        z = numpy.sin(3 * pts[:, 0]) + 0.1 * rng.randn(n)
        B = rng.randn(n, 37)
        for a in (pts, X, z, B):
            a.setflags(write=False)
        _CACHE[n] = (pts, X, z, B)
    return _CACHE[n]


def _params(case):
    rung = case[4]
    return (1.5, 0.2, ETA) if rung is None else LADDER[rung]


@pytest.fixture(scope='module')
def hip():
    from gaussian_proc import _hip
    _hip.require_device(0)
    return _hip


def _operator(hip, monkeypatch, n, nu, scale, outer, panel=None, kloop=None, max_batch=1):
    """An Operator created under GPMI_PANEL / GPMI_KLOOP (None: unset), K assembled on the
    device, [X | z] resident."""
    for name, val in (('GPMI_PANEL', panel), ('GPMI_KLOOP', kloop)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    op = hip.Operator(n, device=0, max_batch=max_batch)
    monkeypatch.delenv('GPMI_PANEL', raising=False)
    monkeypatch.delenv('GPMI_KLOOP', raising=False)
    pts, X, z, _ = _inputs(n)
    op.assemble_matern(pts, numpy.array([scale, scale]), nu)
    op.set_rhs(numpy.column_stack([X, z]))
    op.set_outer(outer)
    return op


class _Reference(object):
    """blocked_reference's values on one A, each computed when first asked for."""

    def __init__(self, A):
        self.A = A
        self._v = {}

    def _get(self, name, make):
        if name not in self._v:
            self._v[name] = make()
        return self._v[name]

    @property
    def blocked(self):
        return self._get('blocked', lambda: bw.blocked_reference(self.A))

    @property
    def chol(self):
        return self._get('chol', lambda: bw.omega_chol(self.A, self.blocked[0]))

    @property
    def inv(self):
        return self._get('inv', lambda: bw.omega_inv(*self.blocked))

    @property
    def kappa(self):
        return self._get('kappa', lambda: bw.kappa_max(self.blocked[0]))


_REF = {}


def _reference(n, nu, scale, eta, K):
    """The reference for A = K + eta I, K the device's; every operator of these inputs
    must have assembled the same K."""
    key = (n, nu, scale, eta)
    if key not in _REF:
        A = K.copy()
        A[numpy.diag_indices(n)] += eta
        A.setflags(write=False)
        _REF[key] = (K, _Reference(A))
    K0, ref = _REF[key]
    assert K0 is K or numpy.array_equal(K0, K), 'the assembly is not reproducible'
    return ref


_DEV = {}


def _device(hip, monkeypatch, case):
    """Everything the device computes for a case, read back once: one operator, closed
    before the host evaluates anything."""
    if case in _DEV:
        return _DEV[case]
    n, outer, panel, kloop, _ = case
    nu, scale, eta = _params(case)
    _, _, z, B = _inputs(n)
    d = dict(n=n, eta=eta)
    op = _operator(hip, monkeypatch, n, nu, scale, outer, panel, kloop)
    try:
        d['n_pad'] = op.n_pad
        K = op.get_matrix()
        d['logdet'] = op.logdet(eta)
        d['L'] = op.factor()
        # the cached factor: fwd_step_kernel, one and three 16-column passes
        d['x1_cached'] = op.solve(eta, z)
        d['x37_cached'] = op.solve(eta, B)
        d['tr1'] = op.traceinv(eta, 1)
        d['W'] = op.trinv()
        d['tr2'] = op.traceinv(eta, 2)
        d['T'] = op.inverse()
        d['dinv'] = op.loo_terms(eta)[0]
        # a fresh factorization per solve: the forward substitution fused into it
        op.logdet(2 * eta)
        d['x1_fresh'] = op.solve(eta, z)
        d['L_again'] = op.factor()
        op.logdet(2 * eta)
        d['x37_fresh'] = op.solve(eta, B)
    except numpy.linalg.LinAlgError as e:
        d['failed'] = str(e)
    finally:
        op.close()
    d['ref'] = _reference(n, nu, scale, eta, K)
    _DEV[case] = d
    return d


def _got(hip, monkeypatch, case):
    d = _device(hip, monkeypatch, case)
    assert 'failed' not in d, 'the device reports a pivot LAPACK does not: ' + d['failed']
    return d


def _worst(tiles):
    i, j = numpy.unravel_index(numpy.argmax(tiles), tiles.shape)
    return 'worst tile (%d, %d); per-tile maxima / u:\n%s' % (
        i, j, numpy.array2string(tiles / U, precision=1, max_line_width=200))


def _chol_bar(n, ref, omega):
    """max((n + 1) u, 16 omega_chol(ref)); the reference is evaluated only when the first
    term does not already decide."""
    return (n + 1) * U if omega <= (n + 1) * U else max((n + 1) * U, 16 * ref.chol)


def _check_factor(n, ref, L, label):
    """Structure and omega_chol of a factor of ref.A -> omega_chol."""
    assert not numpy.any(numpy.triu(L, 1)), 'the strict upper triangle is not zero'
    assert numpy.all(numpy.diag(L) > 0)
    o, tiles = bw.omega_chol(ref.A, L, tiles=True)
    nu1 = (n + 1) * U
    bar = _chol_bar(n, ref, o)
    print('%s: omega_chol %.3f (n+1)u, bar %.3f' % (label, o / nu1, bar / nu1))
    assert o <= bar, _worst(tiles)
    if o > nu1:
        assert o <= nu1 * (1 + ref.kappa), _worst(tiles)
    return o


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_factor(hip, monkeypatch, case):
    d = _got(hip, monkeypatch, case)
    n, L = d['n'], d['L']
    _check_factor(n, d['ref'], L, _id(case))
    # the same input gives the same bits
    assert numpy.array_equal(d['L_again'], L)
    ld, ld_abs = bw.logdet_from_factor(L)
    print('%s: logdet off by %.3g of (n+2)u sum|log|' %
          (_id(case), float(abs(d['logdet'] - ld) / ((n + 2) * U * ld_abs))))
    assert abs(d['logdet'] - ld) <= (n + 2) * U * ld_abs


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_trinv(hip, monkeypatch, case):
    d = _got(hip, monkeypatch, case)
    n, L, W = d['n'], d['L'], d['W']
    assert not numpy.any(numpy.tril(W, -1)), 'W is not upper triangular'
    assert numpy.all(numpy.diag(W) > 0)
    o, tiles = bw.omega_inv(L, W, tiles=True)
    nu1 = (n + 1) * U
    bar = nu1 if o <= nu1 else max(nu1, 16 * d['ref'].inv)
    print('%s: omega_inv %.3f (n+1)u, bar %.3f' % (_id(case), o / nu1, bar / nu1))
    assert o <= bar, _worst(tiles)
    fro = numpy.sum(W.astype(bw.LD) ** 2)
    assert abs(d['tr1'] - fro) <= (n + 2) * U * fro


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_inverse(hip, monkeypatch, case):
    d = _got(hip, monkeypatch, case)
    n, W, T = d['n'], d['W'], d['T']
    assert numpy.array_equal(T, T.T)
    o, tiles = bw.omega_gram(W, T, tiles=True)
    print('%s: omega_gram %.3f (n+1)u, bar %.3f' % (_id(case), o / ((n + 1) * U),
                                                    (d['n_pad'] + 1) / (n + 1)))
    assert o <= (d['n_pad'] + 1) * U, _worst(tiles)
    fro = numpy.sum(T.astype(bw.LD) ** 2)
    assert abs(d['tr2'] - fro) <= (n + 2) * U * fro
    dg = numpy.diag(T)
    assert numpy.all(numpy.abs(d['dinv'] - dg) <= 4 * (n + 1) * U * dg)


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_solve(hip, monkeypatch, case):
    d = _got(hip, monkeypatch, case)
    n, ref = d['n'], d['ref']
    _, _, z, B = _inputs(n)
    got = {k: bw.omega_solve(ref.A, d['L'], d[k], z if k.startswith('x1_') else B)
           for k in ('x1_fresh', 'x37_fresh', 'x1_cached', 'x37_cached')}
    worst = max(got.values())
    bar = (3 * n + 1) * U
    if worst > bar:
        bar *= max(1.0, 16 * ref.chol / ((n + 1) * U))
    print('%s: omega_solve %s (n+1)u, bar %.3f' % (
        _id(case), ' '.join('%s %.3f' % (k[1:], v / ((n + 1) * U)) for k, v in got.items()),
        bar / ((n + 1) * U)))
    for k, v in got.items():
        assert v <= bar, k


# ------------------------------------------------------------------- batch --

@pytest.mark.parametrize('n,outer,batch,slots', [(300, 16, 3, (0, 1, 2)),
                                                 (1000, 4, 3, (0, 1, 2)),
                                                 (300, 16, 33, (0, 16, 32))])
def test_batch_slots(hip, monkeypatch, n, outer, batch, slots):
    """Every member's own factor (both stream halves of a small batch; one stream at 33),
    and slot 0 bit for bit the factor of a handle that factors that eta alone."""
    etas = numpy.logspace(-2, 1, batch)
    op = _operator(hip, monkeypatch, n, 1.5, 0.2, outer, max_batch=batch)
    one = _operator(hip, monkeypatch, n, 1.5, 0.2, outer, max_batch=1)
    try:
        K = op.get_matrix()
        _, _, info = op.loglik_batch(etas)
        assert numpy.all(info == 0)
        Ls = {s: op.factor(s) for s in slots}
        with pytest.raises(hip.GPMIError):
            op.factor(batch)
        one.logdet(etas[0])
        alone = one.factor()
    finally:
        op.close()
        one.close()
    assert numpy.array_equal(Ls[0], alone)
    for s in slots:
        ref = _reference(n, 1.5, 0.2, float(etas[s]), K)
        _check_factor(n, ref, Ls[s], 'n %d batch %d slot %d' % (n, batch, s))


# ------------------------------------------------------------------- state --

def test_factor_needs_a_factorization_of_the_current_matrix(hip, monkeypatch):
    n = 300
    op = _operator(hip, monkeypatch, n, 1.5, 0.2, 16, max_batch=3)
    try:
        with pytest.raises(hip.GPMIError):
            op.factor()
        K = op.get_matrix()
        op.logdet(ETA)
        L = op.factor()
        with pytest.raises(hip.GPMIError):
            op.factor(1)
        with pytest.raises(hip.GPMIError):
            op.factor(-1)
        # a new K: nothing to read until it is factored, and then its own factor
        op.load_matrix(K + 0.5 * numpy.eye(n))
        for slot in (0, 1):
            with pytest.raises(hip.GPMIError):
                op.factor(slot)
        op.logdet(ETA)
        assert not numpy.array_equal(op.factor(), L)
        # the members of a batch last until the next factorization
        op.loglik_batch([0.1, 0.2, 0.3])
        op.factor(2)
        op.logdet(ETA)
        for slot in (1, 2):
            with pytest.raises(hip.GPMIError):
                op.factor(slot)
        op.factor(0)
    finally:
        op.close()


def test_a_member_that_failed_is_not_returned(hip, monkeypatch):
    n = 300
    op = _operator(hip, monkeypatch, n, 1.5, 0.2, 16, max_batch=2)
    try:
        _, _, info = op.loglik_batch([-2.0, ETA])
        assert info[0] > 0 and info[1] == 0
        with pytest.raises(hip.GPMIError):
            op.factor(0)
        op.factor(1)
    finally:
        op.close()


def test_trinv_and_inverse_need_their_stage(hip, monkeypatch):
    op = _operator(hip, monkeypatch, 300, 1.5, 0.2, 16)
    try:
        op.logdet(ETA)
        for get in (op.trinv, op.inverse):
            with pytest.raises(hip.GPMIError):
                get()
        op.traceinv(ETA, 1)
        op.trinv()
        with pytest.raises(hip.GPMIError):
            op.inverse()
        op.traceinv(ETA, 2)
        op.inverse()
        op.trinv()
        # a new factorization: W and A^-1 belong to the old one
        op.logdet(2 * ETA)
        for get in (op.trinv, op.inverse):
            with pytest.raises(hip.GPMIError):
                get()
    finally:
        op.close()


def test_read_backs_change_nothing(hip, monkeypatch):
    """The same calls with and without read-backs in between: the same bits."""
    n = 300
    _, _, z, _ = _inputs(n)
    out = []
    for read in (False, True):
        op = _operator(hip, monkeypatch, n, 1.5, 0.2, 16, max_batch=3)
        try:
            r = [op.logdet(ETA)]
            if read:
                op.factor()
            r.append(op.traceinv(ETA, 1))
            if read:
                op.trinv(), op.factor()
            r.append(op.traceinv(ETA, 2))
            if read:
                op.inverse(), op.trinv(), op.factor()
            r.append(op.solve(ETA, z))
            r.extend(op.loo_terms(ETA))
            r.append(op.traceinv(ETA, 2))
            r.extend(op.loglik_batch([0.1, 0.2, 0.3]))
            if read:
                op.factor(1), op.factor(2)
            r.append(op.solve(0.1, z))
            r.append(op.traceinv(0.1, 1))
            out.append(r)
        finally:
            op.close()
    for a, b in zip(*out):
        assert numpy.array_equal(a, b)


def test_leading_dimension_and_arguments(hip, monkeypatch):
    n = 300
    op = _operator(hip, monkeypatch, n, 1.5, 0.2, 16)
    try:
        op.traceinv(ETA, 2)
        for get in (op.factor, op.trinv, op.inverse):
            wide = get(ld=n + 3)
            assert wide.shape == (n, n + 3)
            assert numpy.all(numpy.isnan(wide[:, n:]))
            assert numpy.array_equal(wide[:, :n], get())
        buf = numpy.full((n, n), numpy.nan)
        null = ctypes.POINTER(ctypes.c_double)()
        lib = op.lib
        for call in (lambda p, ld: lib.gpmi_op_get_factor(op.h, 0, p, ld),
                     lambda p, ld: lib.gpmi_op_get_trinv(op.h, p, ld),
                     lambda p, ld: lib.gpmi_op_get_inverse(op.h, p, ld)):
            assert call(hip.dptr(buf), n - 1) < 0
            assert call(null, n) < 0
        assert numpy.all(numpy.isnan(buf))
        assert lib.gpmi_op_get_factor(None, 0, hip.dptr(buf), n) < 0
    finally:
        op.close()
