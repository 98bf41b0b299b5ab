"""Each stage of the band path held to a backward-error bar of its own, on what the device
left in memory: the reduction K_pad = Q B Q^T (Band.reduction: B, the reflectors V and the
compact-WY T of every panel), Y = Q^T R (rhs), x = (B + eta I)^-1 Y (solution), the
block-tridiagonal part of (B + eta I)^-1 (sinv_blocks) and the tridiagonal the bulge chase
left (tridiagonal). The metrics and the host arithmetic that evaluates them are in
_backward.py (test_backward_host.py shows what they can see); none of the bars depends on
cond(K + eta I), and a failure names the block.

The device assembles K itself (assemble_matern); K_pad is get_matrix() padded by the
identity, R = [X | z | 12 random columns] (the band's 16 columns).

Shapes, the smallest that reach each path (N = n_pad, nt = N / 128):
  300   nt 3  ragged: one CholeskyQR panel and a last Householder panel; the look-ahead
              "K-first" copy; cyclic-reduction levels 3 -> 2 -> 1
  640   nt 5  a multiple of 128: every panel CholeskyQR; odd level sizes
  1000  nt 8  power-of-two levels
  1100  nt 9  odd top level, one-block right edge
Variants at 640 and 1000: GPMI_BAND_PANEL=hh, GPMI_CQ_FO=0, GPMI_BAND_LA=0 (bit for bit the
default's B, V, T and Y); the per-eta stages under GPMI_BAND_BCR=0 and 1; the eigenvalue
stage under GPMI_CHASE_MODE unset / systolic / split with GPMI_BISECT unset / 1.
Conditioning ladder (LADDER, the dense file's): the reduction at n = 640 on its four
distinct K, the per-eta stages at n = 300 and 1000 on all five rungs.

Bars (u = 2^-53; none is taken from the code under test). Every backward-error bar is
max((N + 1) u, 16 x the same metric of the numpy restatement of the device's algorithm on
the same device K / B / Y), the 16 being the margin test_gpu_dense_stages.py grants the
device's other summation order; the restatement is evaluated only when the first term
does not already decide:
  omega_orth, omega_sim, omega_rhs   the larger of the Householder restatement
             (tools/band_proto.py) and the CholeskyQR one (tools/cholqr_proto.py): the
             device and numpy may choose differently on the same panel
  omega_solve   the sequential explicit-inverse band Cholesky with its back substitution
             (_backward.band_chol_solve), for both device paths
  G1 = Y^T x, G2 = x^T x   (N + 2) u of the sums of absolute values, on the arrays read back
  logdet     against a longdouble banded Cholesky of the device's B + eta I; the first-order
             bound eps tr(|A^-1| |L| |L^T|) of a Cholesky backward error eps = 16 (N + 1) u
  omega_sinv    _backward.bcr_sinv_reference (tools/bcr_sinv_proto.py); Zd_k symmetric to
             max(4 u, 16 x the restatement's asymmetry) max |Zd_k|: Z_pp = Linv^T Linv -
             X_l^T Z_lp - X_r^T Z_rp is a difference of rounded products and not symmetric
             to 4 u in numpy either (up to 3.7 x 4 u on the ladder; device 1.1 ... 2.7);
             tr1 = sum tr Zd_k over rows < n to (N + 2) u sum |diag|
  tangent    the same residual for Z + A dZ = 0 on the same blocks, normalised by
             |Z_kk| + sum |A_kj| |dZ_jk|, against tools/bcr_dsinv_proto.py; tr2 = -sum tr dZd_k
  eigenvalues   Sturm counts in longdouble on the tridiagonal read back:
             count(lam_i - delta) <= i < count(lam_i + delta), delta = m u max |lam|,
             m = max(8, 4 m_ref), m_ref the smallest power of two at which LAPACK's
             eigvalsh_tridiagonal of the same (d, e) passes the same test
  chase      tr T = tr B and ||T||_F = ||B||_F in longdouble, and max |lam(T) - lam(B)| /
             ||B||_2 with both spectra from LAPACK: max((N + 2) u, 16 x tools/chase_proto.py)
Not here: G3 (no read-back of the second forward elimination; test_gpu_band.py checks it
by parity) and the cyclic reduction's per-level factor blocks, whose backward error is what
omega_solve and omega_sinv measure.
Measured values: DESIGN section 6 (the tests print them under -s).
"""

import os
import sys

import numpy
import pytest
import scipy.linalg

import _backward as bw

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                'tools'))
import band_proto  # noqa: E402
import chase_proto  # noqa: E402
import cholqr_proto  # noqa: E402

pytestmark = pytest.mark.gpu

U = bw.U
TS = bw.TS
# (nu, scale, eta); nu = 100 is the Gaussian limit (test_gpu_dense_stages.LADDER)
LADDER = [(1.5, 0.2, 1e-2), (2.5, 0.2, 1e-6), (2.5, 1.0, 1e-6), (2.5, 1.0, 1e-10),
          (100, 0.5, 1e-10)]
KNOBS = ('GPMI_BAND_PANEL', 'GPMI_CQ_FO', 'GPMI_BAND_LA', 'GPMI_BAND_BCR', 'GPMI_CHASE_MODE',
         'GPMI_BISECT')

_CACHE = {}


def _inputs(n):
    """Points and R = [X | z | 12 random columns] for size n: computed once, never
    modified."""
    if n not in _CACHE:
        rng = numpy.random.RandomState(n)
        pts = rng.rand(n, 2)
        z = numpy.sin(3 * pts[:, 0]) + 0.1 * rng.randn(n)
        R = numpy.column_stack([numpy.ones(n), pts, z, rng.randn(n, 12)])
        pts.setflags(write=False)
        R.setflags(write=False)
        _CACHE[n] = (pts, R)
    return _CACHE[n]


@pytest.fixture(scope='module')
def hip():
    from gaussian_proc import _hip
    _hip.require_device(0)
    return _hip


class _Session(object):
    """An operator with K assembled on the device and its Band, created and used under
    the given GPMI_* knobs (the others unset); closed, and the knobs unset, on exit."""

    def __init__(self, hip, monkeypatch, n, nu, scale, env=None):
        self.hip, self.mp, self.n = hip, monkeypatch, n
        self.nu, self.scale, self.env = nu, scale, dict(env or {})

    def __enter__(self):
        for k in KNOBS:
            self.mp.delenv(k, raising=False)
        for k, v in self.env.items():
            self.mp.setenv(k, v)
        pts, R = _inputs(self.n)
        self.op = self.hip.Operator(self.n, device=0, max_batch=1)
        self.band = None
        try:
            self.op.assemble_matern(pts, numpy.array([self.scale, self.scale]), self.nu)
            self.band = self.hip.Band(self.op)
        except Exception:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        if self.band is not None:
            self.band.close()
        self.op.close()
        for k in KNOBS:
            self.mp.delenv(k, raising=False)
        return False

    def k_pad(self):
        N = self.op.n_pad
        K = numpy.eye(N)
        K[:self.n, :self.n] = self.op.get_matrix()
        return K


def _r_pad(n, N):
    R = numpy.zeros((N, 16))
    R[:n] = _inputs(n)[1]
    return R


def _bar(value, floor, reference):
    """max(floor, 16 reference()); the reference is evaluated only when the floor does
    not already decide."""
    return floor if value <= floor else max(floor, 16 * reference())


# ------------------------------------------------------------------ reduction --

# (n, nu, scale, knobs)
_V = [('hh', {'GPMI_BAND_PANEL': 'hh'}), ('fo0', {'GPMI_CQ_FO': '0'})]
RED_CASES = ([(n, 1.5, 0.2, ()) for n in (300, 640, 1000, 1100)] +
             [(n, 1.5, 0.2, tuple(env.items())) for n in (640, 1000) for _, env in _V] +
             [(640, nu, scale, ()) for nu, scale in ((2.5, 0.2), (2.5, 1.0), (100, 0.5))])


def _red_id(case):
    n, nu, scale, env = case
    return '%d-nu%g-s%g%s' % (n, nu, scale, ''.join('-%s=%s' % (k[5:], v) for k, v in env))


_RED = {}


def _reduction(hip, monkeypatch, case):
    """What the device left after the reduction of a case, read back once: after create +
    set_rhs, and again after refresh(R) (Q^T applied beside the reduction)."""
    if case not in _RED:
        n, nu, scale, env = case
        with _Session(hip, monkeypatch, n, nu, scale, dict(env)) as s:
            d = dict(n=n, N=s.op.n_pad, K=s.k_pad())
            s.band.set_rhs(_inputs(n)[1])
            d['B'], d['V'], d['T'] = s.band.reduction()
            d['Y'] = s.band.rhs()
            s.band.refresh(_inputs(n)[1])
            d['again'] = s.band.reduction()
            d['Y_refresh'] = s.band.rhs()
            d['stats'] = s.band.stats()
        _RED[case] = d
    return _RED[case]


_RED_REF = {}


def _reduction_reference(d, key):
    """The larger of the two restatements' metrics on the device's K."""
    if key not in _RED_REF:
        n, N, K = d['n'], d['N'], d['K']
        R = _r_pad(n, N)
        out = {}
        for name in ('householder', 'cholqr'):
            if name == 'householder':
                A, Vs, Ts = band_proto.band_reduce(K, TS)
            else:
                A, Vs, Ts = cholqr_proto.band_reduce_cholqr(K, TS, [], n_real=n, want_vt=True)
            Y = band_proto.apply_qt(Vs, Ts, R, TS)
            V, T = bw.panels_to_v(Vs, Ts, N)
            m = bw.reduction_metrics(K, bw.band_of(A), V, T, R, Y)
            for k, v in m.items():
                out[k] = max(out.get(k, 0.0), v[0])
        _RED_REF[key] = out
    return _RED_REF[key]


@pytest.mark.parametrize('case', RED_CASES, ids=_red_id)
def test_reduction(hip, monkeypatch, case):
    d = _reduction(hip, monkeypatch, case)
    n, N, K, B, V, T = d['n'], d['N'], d['K'], d['B'], d['V'], d['T']
    print('%s: %s' % (_red_id(case), d['stats']))
    assert d['stats']['cholqr_fallbacks'] == 0 and d['stats']['panel_fallbacks'] == 0
    assert bw.band_structure(B, V, n) == []
    for p in range(T.shape[0]):
        assert not numpy.any(numpy.tril(T[p], -1)), 'T of panel %d is not upper triangular' % p
    # the same input gives the same bits, with Q^T applied beside the reduction or after
    for a, b in zip(d['again'], (B, V, T)):
        assert numpy.array_equal(a, b)
    R = _r_pad(n, N)
    Q = bw.band_q(V, T)
    got = dict(orth=bw.omega_orth(Q), sim=bw.omega_sim(K, Q, B), rhs=bw.omega_rhs(Q, R, d['Y']),
               rhs_refresh=bw.omega_rhs(Q, R, d['Y_refresh']))
    floor = (N + 1) * U
    key = case[:3]
    bars = {k: _bar(v[0], floor, lambda k=k: _reduction_reference(d, key)[k[:3]])
            for k, v in got.items()}
    print('%s: (N+1)u multiples: %s' % (_red_id(case), ', '.join(
        '%s %.3f at %s (bar %.3f)' % (k, v[0] / floor, v[1], bars[k] / floor)
        for k, v in got.items())))
    for k, v in got.items():
        assert v[0] <= bars[k], '%s: worst block %s' % (k, v[1])


@pytest.mark.parametrize('n', [640, 1000])
def test_no_lookahead_is_bit_identical(hip, monkeypatch, n):
    d0 = _reduction(hip, monkeypatch, (n, 1.5, 0.2, ()))
    d1 = _reduction(hip, monkeypatch, (n, 1.5, 0.2, (('GPMI_BAND_LA', '0'),)))
    for k in ('B', 'V', 'T', 'Y', 'Y_refresh'):
        assert numpy.array_equal(d0[k], d1[k]), k


# -------------------------------------------------------------------- per eta --

# (n, rung, GPMI_BAND_BCR or None)
ETA_CASES = ([(n, r, None) for n in (300, 1000) for r in range(len(LADDER))] +
             [(n, 0, bcr) for n in (640, 1000) for bcr in ('0', '1')])


def _eta_id(case):
    n, r, bcr = case
    return '%d-rung%d%s' % (n, r, '' if bcr is None else '-bcr' + bcr)


_ETA = {}


def _per_eta(hip, monkeypatch, case):
    if case not in _ETA:
        n, r, bcr = case
        nu, scale, eta = LADDER[r]
        with _Session(hip, monkeypatch, n, nu, scale,
                      {} if bcr is None else {'GPMI_BAND_BCR': bcr}) as s:
            d = dict(n=n, N=s.op.n_pad, eta=eta)
            s.band.set_rhs(_inputs(n)[1])
            d['B'] = s.band.reduction()[0]
            d['Y'] = s.band.rhs()
            ld, g1, g2, _, info = s.band.der_terms([eta])
            d['logdet'], d['g1'], d['g2'], d['info'] = ld[0], g1[0], g2[0], info[0]
            d['x'] = s.band.solution(0)
            tr, info = s.band.traceinv([eta], 1)
            d['tr1'], d['info_tr'] = tr[0], info[0]
            d['Zd'], d['Zsub'] = s.band.sinv_blocks(0)
            # the traces beside the solves (selected inversion on the side stream)
            out = s.band.der_terms([eta], traceinv=True)
            d['tr1_der'] = out[4][0]
            d['x_der'] = s.band.solution(0)
            d['Zd_der'] = s.band.sinv_blocks(0)[0]
            # exponent 2: the eta-tangent rides on the primal recurrences
            tr, info = s.band.traceinv([eta], 2)
            d['tr2'] = tr[0]
            d['Zd_tan'], d['Zsub_tan'] = s.band.sinv_blocks(0)
            d['dZd'], d['dZsub'] = s.band.sinv_blocks(0, tangent=True)
        _ETA[case] = d
    return _ETA[case]


@pytest.mark.parametrize('case', ETA_CASES, ids=_eta_id)
def test_band_solve(hip, monkeypatch, case):
    d = _per_eta(hip, monkeypatch, case)
    N, B, Y, x, eta = d['N'], d['B'], d['Y'], d['x'], d['eta']
    assert d['info'] == 0
    A = B + eta * numpy.eye(N)
    floor = (N + 1) * U
    ref = lambda: bw.omega_band_solve(A, bw.band_chol_solve(A, Y), Y)[0]   # noqa: E731
    for name in ('x', 'x_der'):
        o, at = bw.omega_band_solve(A, d[name], Y)
        bar = _bar(o, floor, ref)
        print('%s: omega_solve(%s) %.3f (N+1)u at block %d, bar %.3f'
              % (_eta_id(case), name, o / floor, at, bar / floor))
        assert o <= bar, 'block row %d' % at
    r1 = bw.gram_residual(Y, x, d['g1'])
    r2 = bw.gram_residual(x, x, d['g2'])
    print('%s: G1 %.3f, G2 %.3f of (N+2)u' % (_eta_id(case), r1 / ((N + 2) * U),
                                               r2 / ((N + 2) * U)))
    assert r2 <= (N + 2) * U
    assert r1 <= (N + 2) * U


@pytest.mark.parametrize('case', ETA_CASES, ids=_eta_id)
def test_band_logdet(hip, monkeypatch, case):
    d = _per_eta(hip, monkeypatch, case)
    n, N, eta = d['n'], d['N'], d['eta']
    A = d['B'][:n, :n] + eta * numpy.eye(n)      # (the pad block is a decoupled identity)
    ld = bw.band_logdet(A)[0]
    bar = bw.logdet_bar(A, 16 * (N + 1) * U)
    print('%s: logdet off by %.3g, bar %.3g (relative %.3g, %.3g)'
          % (_eta_id(case), float(abs(d['logdet'] - ld)), bar,
             float(abs((d['logdet'] - ld) / ld)), float(abs(bar / ld))))
    assert abs(d['logdet'] - ld) <= bar


@pytest.mark.parametrize('case', ETA_CASES, ids=_eta_id)
def test_selected_inverse(hip, monkeypatch, case):
    d = _per_eta(hip, monkeypatch, case)
    n, N, B, eta, Zd, Zsub = d['n'], d['N'], d['B'], d['eta'], d['Zd'], d['Zsub']
    assert d['info_tr'] == 0
    floor = (N + 1) * U
    o, at = bw.omega_sinv(B, eta, Zd, Zsub)
    bar = _bar(o, floor, lambda: bw.omega_sinv(B, eta, *bw.bcr_sinv_reference(B, eta)[:2])[0])
    print('%s: omega_sinv %.3f (N+1)u at block %d, bar %.3f'
          % (_eta_id(case), o / floor, at, bar / floor))
    assert o <= bar, 'block column %d' % at
    a, at = bw.sinv_asymmetry(Zd)
    bar = _bar(a, 4 * U, lambda: bw.sinv_asymmetry(bw.bcr_sinv_reference(B, eta)[0])[0])
    print('%s: asymmetry of Zd %.3f of 4u max|Zd_k| at block %d, bar %.3f'
          % (_eta_id(case), a / (4 * U), at, bar / (4 * U)))
    assert a <= bar, 'block %d' % at
    dg = numpy.concatenate([numpy.diag(z) for z in Zd])[:n].astype(bw.LD)
    assert abs(d['tr1'] - numpy.sum(dg)) <= (N + 2) * U * numpy.sum(numpy.abs(dg))
    # the same selected inversion beside the derivative solves
    assert d['tr1_der'] == d['tr1']
    assert numpy.array_equal(d['Zd_der'], Zd)


@pytest.mark.parametrize('case', ETA_CASES, ids=_eta_id)
def test_selected_inverse_tangent(hip, monkeypatch, case):
    d = _per_eta(hip, monkeypatch, case)
    n, N, B, eta = d['n'], d['N'], d['B'], d['eta']
    Zd, Zsub, dZd, dZsub = d['Zd_tan'], d['Zsub_tan'], d['dZd'], d['dZsub']
    # the primal blocks of an exponent-2 call are those of an exponent-1 call
    assert numpy.array_equal(Zd, d['Zd']) and numpy.array_equal(Zsub, d['Zsub'])
    floor = (N + 1) * U

    def ref():
        rZd, rZsub, rdZd, rdZsub = bw.bcr_dsinv_reference(B, eta)
        return bw.omega_sinv(B, eta, rZd, rZsub, tangent=(rdZd, rdZsub))[0]
    o, at = bw.omega_sinv(B, eta, Zd, Zsub, tangent=(dZd, dZsub))
    bar = _bar(o, floor, ref)
    print('%s: tangent residual %.3f (N+1)u at block %d, bar %.3f'
          % (_eta_id(case), o / floor, at, bar / floor))
    assert o <= bar, 'block column %d' % at
    dg = numpy.concatenate([numpy.diag(z) for z in dZd])[:n].astype(bw.LD)
    assert abs(d['tr2'] + numpy.sum(dg)) <= (N + 2) * U * numpy.sum(numpy.abs(dg))


# ---------------------------------------------------------------- eigenvalues --

EIG_CASES = [(n, mode, bis) for n in (640, 1000) for mode in (None, 'systolic', 'split')
             for bis in (None, '1')]


def _eig_id(case):
    n, mode, bis = case
    return '%d-%s%s' % (n, mode or 'default', '-bisect' if bis else '')


_CHASE_REF = {}


def _chase_reference(n, B):
    """tools/chase_proto.py on the device's B: its invariants and its spectrum's distance
    from B's, the values the chase's bars are 16 times of."""
    if n not in _CHASE_REF:
        dd, e, _ = chase_proto.chase(B, TS)
        tr, fro = bw.chase_invariants(B, dd, e * e)
        _CHASE_REF[n] = (B, dict(tr=tr, fro=fro, lam=_spectrum_distance(B, dd, e * e)))
    B0, ref = _CHASE_REF[n]
    assert numpy.array_equal(B0, B), 'the reduction is not reproducible'
    return ref


def _spectrum_distance(B, dd, e2):
    lb = scipy.linalg.eigvals_banded(_band_storage(B), lower=True)
    lt = scipy.linalg.eigvalsh_tridiagonal(dd, numpy.sqrt(e2))
    return float(numpy.max(numpy.abs(lt - lb)) / max(abs(lb[0]), abs(lb[-1])))


def _band_storage(B):
    n = B.shape[0]
    ab = numpy.zeros((TS + 1, n))
    for k in range(TS + 1):
        ab[k, :n - k] = numpy.diag(B, -k)
    return ab


@pytest.mark.parametrize('case', EIG_CASES, ids=_eig_id)
def test_eigenvalues(hip, monkeypatch, case):
    n, mode, bis = case
    env = {}
    if mode:
        env['GPMI_CHASE_MODE'] = mode
    if bis:
        env['GPMI_BISECT'] = bis
    with _Session(hip, monkeypatch, n, 1.5, 0.2, env) as s:
        N = s.op.n_pad
        B = s.band.reduction()[0][:n, :n]
        lam = s.band.eigenvalues()
        dd, e2 = s.band.tridiagonal()
        info = s.band.chase_info()
        lam2 = s.band.eigenvalues()
        dd2, e22 = s.band.tridiagonal()
    print('%s: %s' % (_eig_id(case), info))
    assert info['fallbacks'] == 0
    assert numpy.array_equal(lam, lam2) and numpy.array_equal(dd, dd2) and \
        numpy.array_equal(e2, e22)
    assert numpy.all(e2 >= 0) and numpy.all(numpy.diff(lam) >= 0)
    # the bisection against the tridiagonal it read
    scale = float(numpy.max(numpy.abs(lam)))
    lapack = scipy.linalg.eigvalsh_tridiagonal(dd, numpy.sqrt(e2))
    m_ref = bw.sturm_margin(dd, e2, lapack, scale)
    m_dev = bw.sturm_margin(dd, e2, lam, scale)
    m = max(8, 4 * m_ref)
    print('%s: Sturm margin device %s, LAPACK %s, allowed %d (units of u max|lam|)'
          % (_eig_id(case), m_dev, m_ref, m))
    ok, at = bw.sturm_ok(dd, e2, lam, m * U * scale)
    assert ok, 'eigenvalue %d' % at
    # the chase against the band it read
    tr, fro = bw.chase_invariants(B, dd, e2)
    dist = _spectrum_distance(B, dd, e2)
    floor = (N + 2) * U
    ref = lambda: _chase_reference(n, B)   # noqa: E731
    bars = dict(tr=_bar(tr, floor, lambda: ref()['tr']), fro=_bar(fro, floor, lambda: ref()['fro']),
                lam=_bar(dist, floor, lambda: ref()['lam']))
    print('%s: (N+2)u multiples: tr %.3f (bar %.3f), fro %.3f (bar %.3f), spectrum %.3f (bar %.3f)'
          % (_eig_id(case), tr / floor, bars['tr'] / floor, fro / floor, bars['fro'] / floor,
             dist / floor, bars['lam'] / floor))
    assert tr <= bars['tr'] and fro <= bars['fro'] and dist <= bars['lam']


# ---------------------------------------------------------------------- state --

def test_refusals(hip, monkeypatch):
    n = 300
    R = _inputs(n)[1]
    with _Session(hip, monkeypatch, n, 1.5, 0.2) as s:
        band = s.band
        band.reduction()                       # always there
        for get in (band.rhs, band.solution, band.sinv_blocks, band.tridiagonal):
            with pytest.raises(hip.GPMIError):
                get()
        band.set_rhs(R)
        band.rhs()
        with pytest.raises(hip.GPMIError):
            band.solution(0)
        band.loglik([0.1])                     # not a der_terms call
        with pytest.raises(hip.GPMIError):
            band.solution(0)
        band.der_terms([0.1, 0.2])
        band.solution(1)
        for slot in (-1, 2):
            with pytest.raises(hip.GPMIError):
                band.solution(slot)
        with pytest.raises(hip.GPMIError):
            band.sinv_blocks(0)
        band.traceinv([0.1, 0.2], 1)
        band.sinv_blocks(1)
        with pytest.raises(hip.GPMIError):
            band.sinv_blocks(2)
        with pytest.raises(hip.GPMIError):
            band.sinv_raw(0, tangent=True)     # needs an exponent-2 call
        band.traceinv([0.1], 2)
        band.sinv_raw(0, tangent=True)
        with pytest.raises(hip.GPMIError):
            band.sinv_blocks(1)                # past the last call
        band.traceinv([0.1], 1)
        with pytest.raises(hip.GPMIError):
            band.sinv_raw(0, tangent=True)     # the last call carried no tangent
        # a failed pivot: that slot is refused, the other is not
        _, _, _, _, info = band.der_terms([-2.0, 0.1])
        assert info[0] > 0 and info[1] == 0
        with pytest.raises(hip.GPMIError):
            band.solution(0)
        band.solution(1)
        band.eigenvalues()
        band.tridiagonal()
        # a new RHS: the solution belonged to the old one
        band.set_rhs(R)
        with pytest.raises(hip.GPMIError):
            band.solution(1)
        band.der_terms([0.1])
        band.solution(0)
        # a new reduction: nothing per eta, no tridiagonal, and (without R) no RHS
        band.refresh()
        for get in (band.rhs, band.solution, band.sinv_blocks, band.tridiagonal):
            with pytest.raises(hip.GPMIError):
                get()
        band.refresh(R)
        band.rhs()
        for get in (band.solution, band.sinv_blocks, band.tridiagonal):
            with pytest.raises(hip.GPMIError):
                get()
        assert band.lib.gpmi_band_get_rhs(None, hip.dptr(numpy.empty((384, 16))), 16) < 0
        assert band.lib.gpmi_band_get_rhs(band.h, hip.dptr(numpy.empty((384, 16))), 15) < 0


@pytest.mark.parametrize('bcr', ['0', '1'])
def test_slots_and_replacement(hip, monkeypatch, bcr):
    """Slots 0, 1 and 7 of an 8-eta call each solve their own eta; a second der_terms call
    replaces what solution returns."""
    n = 300
    etas = numpy.logspace(-3, 1, 8)
    with _Session(hip, monkeypatch, n, 1.5, 0.2, {'GPMI_BAND_BCR': bcr}) as s:
        N = s.op.n_pad
        s.band.set_rhs(_inputs(n)[1])
        B = s.band.reduction()[0]
        Y = s.band.rhs()
        s.band.der_terms(etas)
        xs = {slot: s.band.solution(slot) for slot in (0, 1, 7)}
        with pytest.raises(hip.GPMIError):
            s.band.solution(8)
        s.band.der_terms(etas[5:7])
        x5 = s.band.solution(0)
        with pytest.raises(hip.GPMIError):
            s.band.solution(2)
    floor = (N + 1) * U
    for slot, x in list(xs.items()) + [(5, x5)]:
        A = B + etas[slot] * numpy.eye(N)
        o, at = bw.omega_band_solve(A, x, Y)
        bar = _bar(o, floor, lambda: bw.omega_band_solve(A, bw.band_chol_solve(A, Y), Y)[0])
        print('bcr %s slot %d: omega_solve %.3f (N+1)u, bar %.3f' % (bcr, slot, o / floor,
                                                                    bar / floor))
        assert o <= bar, (slot, at)
    assert not numpy.array_equal(x5, xs[0])


def test_read_backs_change_nothing(hip, monkeypatch):
    """The same calls with and without read-backs in between: the same bits."""
    n = 300
    R = _inputs(n)[1]
    out = []
    for read in (False, True):
        with _Session(hip, monkeypatch, n, 1.5, 0.2) as s:
            band = s.band
            band.set_rhs(R)
            if read:
                band.reduction(), band.rhs()
            r = list(band.loglik([0.1, 0.2]))
            r.extend(band.der_terms([0.1, 0.3]))
            if read:
                band.solution(1), band.reduction()
            r.extend(band.der_terms([0.1, 0.3], traceinv=2))
            if read:
                band.solution(0), band.sinv_blocks(1), band.sinv_raw(1, tangent=True)
            r.extend(band.traceinv([0.2, 0.4], 2))
            if read:
                band.sinv_raw(0, tangent=True), band.rhs()
            r.append(band.eigenvalues())
            if read:
                band.tridiagonal(), band.reduction()
            r.extend(band.loglik([0.1, 0.2]))
            r.extend(band.der_terms([0.5]))
            r.append(band.eigenvalues())
            band.refresh(R)
            if read:
                band.reduction(), band.rhs()
            r.extend(band.der_terms([0.1, 0.3], traceinv=1))
            out.append(r)
    for a, b in zip(*out):
        assert numpy.array_equal(a, b)
