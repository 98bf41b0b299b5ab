"""The sparse operator's handle (csrc/gpmi_sp.h) across calls: its lazy workspaces appear
and are regrown in whatever order the calls come, the multi-shift CG's second block buffer
and final-Gram buffer appear late and are reused, the timing events are recycled from one
window to the next, the Lanczos and the multi-shift CG run from two host threads at once,
and handles are created and destroyed in a row, the create path that fails included.

None of this may change a result: every comparison is bit for bit against a fresh handle
that makes only that one call. n = 625 (25^2 grid points) is ten 64-row blocks, the last
one ragged; 40 columns are a 32-column pass and an 8-column one.
"""

import threading

import numpy
import pytest

from oracle import data, matern, sparse as osp
from _util import load_json

pytestmark = pytest.mark.gpu

NU = 1.5
ETAS = numpy.array([3.0, 5.0, 40.0])   # > |lambda_min| of the (indefinite) tapered matrices
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _K625():
    return _cached('K625', lambda: osp.sparse_correlation(data.generate_points(25, 2, True),
                                                          0.08, NU, 0.03)[0])


def _blocks():
    """Read-only random blocks [625, w] by width."""
    def make():
        rng = numpy.random.RandomState(11)
        out = {w: rng.randn(625, w) for w in (3, 5, 7, 12, 40)}
        for a in out.values():
            a.setflags(write=False)
        return out
    return _cached('blocks', make)


def _compaction_inputs():
    """K (24^2 points) and B as in test_gpu_sparse.py::test_msgram_compaction_bit_identical:
    six columns stop within the first poll, the seventh does not."""
    def make():
        K = osp.sparse_correlation(data.generate_points(24, 2, True), 0.08, NU, 0.03)[0]
        _, U = numpy.linalg.eigh(K.toarray())
        B = numpy.empty((K.shape[0], 7))
        for c in range(6):
            B[:, c] = U[:, -1 - c] + 0.5 * U[:, -2 - c]
        B[:, 6] = numpy.random.RandomState(9).randn(K.shape[0])
        B.setflags(write=False)
        return K, B
    return _cached('compaction', make)


@pytest.fixture(scope='module')
def hip():
    from gaussian_proc import _hip
    _hip.require_device(0)
    return _hip


def _fresh(hip, call, K=None):
    """`call` on a handle of its own that makes no other call."""
    sop = hip.SparseOperator.from_csr(_K625() if K is None else K)
    try:
        return call(sop)
    finally:
        sop.close()


def _assert_same(got, ref):
    if not isinstance(got, tuple):
        got, ref = (got,), (ref,)
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        numpy.testing.assert_array_equal(a, b)


def _msgram(B, **kw):
    def call(sop):
        if kw.get('resident'):
            sop.set_rhs(B)
        G = sop.msgram(ETAS, None if kw.get('resident') else B, rtol=1e-10, cols=kw.get('cols'))
        return G, sop.last_cg_iterations
    return call


def test_workspaces_grow_across_calls(hip):
    X = _blocks()
    spmm = lambda w: (lambda sop: sop.spmm(0.3, X[w]))
    lanczos = lambda steps, orth: (lambda sop: sop.lanczos(5, steps, seed=3, orthogonalize=orth))

    def cg(sop):
        return sop.cg(3.0, X[3], rtol=1e-8), sop.last_cg_iterations

    calls = [spmm(5), spmm(40)]                                   # ws appears, regrows
    for orth in (0, 3, -1):                                       # lz / partial / lzd, ws
        calls += [lanczos(8, orth), lanczos(30, orth)]
    calls += [cg,
              _msgram(X[7]),                                      # ms.ws, cg2_buf, blk[0], pin
              _msgram(X[7], resident=True),                       # rhs_dev at 7 columns
              _msgram(X[12], resident=True),                      # ... freed and made anew at 12
              _msgram(X[12], cols=(1, 7)),
              # the small calls again, in the grown buffers
              spmm(5), lanczos(8, 0), lanczos(8, 3), lanczos(8, -1), cg,
              _msgram(X[7], resident=True), _msgram(X[7])]
    sop = hip.SparseOperator.from_csr(_K625())
    try:
        for i, call in enumerate(calls):
            got, ref = call(sop), _fresh(hip, call)
            try:
                _assert_same(got, ref)
            except AssertionError as e:
                raise AssertionError('call %d of the sequence differs: %s' % (i, e))
    finally:
        sop.close()


def test_compaction_buffers_appear_late_and_are_reused(hip, monkeypatch):
    K, B = _compaction_inputs()
    call = lambda sop: sop.msgram(ETAS, B, rtol=1e-12)
    monkeypatch.setenv('GPMI_MS_COMPACT', '0')
    ref = _fresh(hip, call, K)
    sop = hip.SparseOperator.from_csr(K)
    try:
        for compact in ('0', '1', '0', '1'):    # blk[1] and gfin appear at the second call
            monkeypatch.setenv('GPMI_MS_COMPACT', compact)
            G = call(sop)
            assert (sop.msgram_compactions() >= 1) == (compact == '1')
            numpy.testing.assert_array_equal(G, ref)
        monkeypatch.delenv('GPMI_MS_COMPACT')
        numpy.testing.assert_array_equal(_fresh(hip, call, K), ref)
    finally:
        sop.close()


def test_timing_windows_recycle_events(hip):
    X = _blocks()
    sop = hip.SparseOperator.from_csr(_K625())
    try:
        y5, y40 = sop.spmm(0.3, X[5]), sop.spmm(0.3, X[40])
        lanczos = lambda: sop.lanczos(5, 8, seed=3, orthogonalize=0)   # eight 5-column SpMMs
        lz = lanczos()
        assert sop.spmm_kernel(32) != 'csr_spmm_wing_kernel'    # logged by an event pair
        sop.set_timing(True)
        _assert_same(sop.spmm(0.3, X[5]), y5)
        _assert_same(sop.spmm(0.3, X[40]), y40)
        first = sop.spmm_timing()
        assert {w: c for w, (c, _) in first.items()} == {5: 1, 32: 1, 8: 1}
        sop.set_timing(True)                    # a new window: the pairs go back to the pool
        _assert_same(sop.spmm(0.3, X[40]), y40)
        _assert_same(sop.spmm(0.3, X[40]), y40)
        _assert_same(lanczos(), lz)
        for _ in range(2):                      # reading the log does not consume it
            second = sop.spmm_timing()
            assert {w: c for w, (c, _) in second.items()} == {32: 2, 8: 2, 5: 8}
            assert all(numpy.isfinite(ms) and ms > 0.0 for _, ms in second.values())
        sop.set_timing(False)
        _assert_same(sop.spmm(0.3, X[40]), y40)
    finally:
        sop.close()


def test_lanczos_beside_msgram_on_two_threads(hip):
    """As sweep.slq_gram_sweep runs them: the Lanczos on the calling thread and the main
    stream, the multi-shift CG on a second thread and its own stream, one handle."""
    X = _blocks()
    lanczos = lambda sop: sop.lanczos(20, 30, seed=5)
    gram = _msgram(X[7])
    ref_l, ref_g = _fresh(hip, lanczos), _fresh(hip, gram)
    sop = hip.SparseOperator.from_csr(_K625())
    try:
        for _ in range(3):      # the first round also builds the windows, from either thread
            box = {}

            def side():
                try:
                    box['g'] = gram(sop)
                except Exception as e:   # noqa: BLE001 (reported by the assert below)
                    box['error'] = e
            t = threading.Thread(target=side)
            t.start()
            got_l = lanczos(sop)
            t.join()
            assert 'error' not in box, box.get('error')
            _assert_same(got_l, ref_l)
            _assert_same(box['g'], ref_g)
    finally:
        sop.close()


def test_create_and_close_in_a_row(hip):
    X = _blocks()[5]
    vals = [_fresh(hip, lambda sop: sop.spmm(0.3, X)) for _ in range(20)]
    assert numpy.all(numpy.isfinite(vals[0])) and all(numpy.array_equal(v, vals[0]) for v in vals)
    pts = data.generate_points(20, 2, True)
    Xp = numpy.random.RandomState(2).randn(400, 5)
    vals = []
    for _ in range(20):
        sop = hip.SparseOperator.from_points(pts, numpy.full(2, 0.05), NU, 0.05)
        vals.append((sop.nnz, sop.spmm(0.3, Xp)))
        sop.close()
    assert numpy.all(numpy.isfinite(vals[0][1]))
    assert all(v[0] == vals[0][0] and numpy.array_equal(v[1], vals[0][1]) for v in vals)
    # a dense-mode handle borrows its Operator's K: closed first
    rng = numpy.random.RandomState(300)
    Kd = matern.dense_correlation(rng.rand(300, 2), 0.2, NU)
    Xd = rng.randn(300, 5)
    op = hip.Operator(300, device=0)
    op.load_matrix(Kd)
    sd = hip.SparseOperator.from_dense(op)
    Y = sd.spmm(0.3, Xd)
    sd.close()
    op.close()
    # (300-term fp64 sums of entries below 1 times normals: n eps sum |k x| < 1e-11)
    numpy.testing.assert_allclose(Y, Kd @ Xd + 0.3 * Xd, rtol=0, atol=1e-11)


def test_failed_create_leaves_nothing_behind(hip):
    """A taper threshold that is never reached fails gpmi_sp_create_matern (-1101) after
    the handle, its stream and its first buffer exist: fifty times in a row, then a valid
    operator. The ValueError of test_gpu_sparse.py::test_threshold_error_matches_reference
    comes from the host heuristic before the library is called; a threshold below every
    kernel value is what reaches the library's own check."""
    import gaussian_proc
    pts = data.generate_points(10, 2, True)
    for _ in range(50):
        with pytest.raises(ValueError):
            gaussian_proc.generate_correlation(pts, 0.1, NU, sparse=True, density=1e-3)
        with pytest.raises(hip.GPMIError, match='taper threshold not reached'):
            hip.SparseOperator.from_points(pts, numpy.full(2, 0.1), NU, -1.0)
    meta = load_json('sparse.json')[0]
    K = gaussian_proc.generate_correlation(
        data.generate_points(meta['num_points'], meta['dimension'], True),
        meta['correlation_scale'], meta['nu'], sparse=True, density=meta['density'])
    assert K.nnz == meta['nnz']
