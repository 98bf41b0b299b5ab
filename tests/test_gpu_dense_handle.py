"""The dense operator's handle (csrc/gpmi_op.h) across calls: its lazy workspaces appear
and are regrown in whatever order the calls come, the second stream of a batched call is
released and created again, the grouped tile orders are rebuilt by set_outer, and
handles are created and destroyed in a row.

None of this may change a result: every comparison is bit for bit against a fresh handle
that makes only that one call (inputs as test_gpu_dense_kloop.py). The one exception is a
solve on a cached factor: it runs the forward substitution as fwd_step_kernel launches,
a fresh handle's solve runs it fused into the factorization, and the two kernels differ
in the last bits (measured at n = 300, eta = 0.03: max 8.57e-14 absolute, 1.7e-11
relative, the same figure with the handle as it was before gpmi_op.h). That call is
compared, still bit for bit, with a fresh handle that factors first (logdet) and then
solves; a solve at a new eta, which factors, follows it and is compared as the others.
n = 300 is three tile rows, the last one ragged; n = 1000 at outer 4 is the smallest
shape of test_gpu_dense_kloop.py whose bulk update uses a grouped tile order.
"""

import numpy
import pytest

from oracle import matern

pytestmark = pytest.mark.gpu

SCALE, NU = 0.2, 1.5
_CACHE = {}


def _inputs(n):
    """K (Matern 3/2), points, R = [1 | points | z] for size n: computed once, read-only."""
    if n not in _CACHE:
        rng = numpy.random.RandomState(n)
        pts = rng.rand(n, 2)
        K = matern.dense_correlation(pts, SCALE, NU)
        z = numpy.sin(3 * pts[:, 0]) + 0.1 * rng.randn(n)
        R = numpy.column_stack([numpy.ones(n), pts, z])
        for a in (K, pts, R):
            a.setflags(write=False)
        _CACHE[n] = (K, pts, R)
    return _CACHE[n]


@pytest.fixture(scope='module')
def hip():
    from gaussian_proc import _hip
    _hip.require_device(0)
    return _hip


def _operator(hip, n, outer=16, max_batch=1):
    K, _, R = _inputs(n)
    op = hip.Operator(n, device=0, max_batch=max_batch)
    op.load_matrix(K)
    op.set_rhs(R)
    op.set_outer(outer)
    return op


def _fresh(hip, n, call, **kw):
    """`call` on a handle of its own that makes no other call."""
    op = _operator(hip, n, **kw)
    try:
        return call(op)
    finally:
        op.close()


def _assert_same(got, ref):
    if not isinstance(got, tuple):
        got, ref = (got,), (ref,)
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        numpy.testing.assert_array_equal(a, b)


def test_workspaces_grow_across_calls(hip):
    n, eta, eta2, eta3 = 300, 0.03, 2.0, 0.5
    _, pts, R = _inputs(n)
    scale = numpy.full(2, SCALE)
    rng = numpy.random.RandomState(7)
    t5, t200, t130 = rng.rand(5, 2), rng.rand(200, 2), rng.rand(130, 2)

    def terms(tst):
        return lambda op: op.predict_terms(eta, test_points=tst, points=pts, scale=scale, nu=NU)

    def cached_solve(op):
        op.logdet(eta)
        return op.solve(eta, R[:, 3])

    # (call on the one handle, the same on a fresh handle)
    calls = [
        (lambda op: op.traceinv(eta, 2), None),    # W, tpart, Td appear
        (terms(t5), None),                         # PY, Pgram, PT, Ppart, Pout at 128 columns
        (terms(t200), None),                       # ... regrown to 256
        (lambda op: op.predict_cov(eta, test_points=t130, points=pts, scale=scale, nu=NU), None),
        (terms(t5), None),                         # the small call again, in the grown workspace
        # the cached factor: forward substitution by fwd_step_kernel, over R slot 0 behind
        # the prediction's Y; the fresh handle factors first (see the top of the file)
        (lambda op: op.solve(eta, R[:, 3]), cached_solve),
        (lambda op: op.solve(eta3, R[:, 3]), None),   # a solve that factors, as a fresh one
        (lambda op: op.traceinv(eta2, 1), None),      # a new factor under the trace cache
    ]
    op = _operator(hip, n)
    try:
        for i, (call, alone) in enumerate(calls):
            got, ref = call(op), _fresh(hip, n, alone or call)
            try:
                _assert_same(got, ref)
            except AssertionError as e:
                raise AssertionError('call %d of the sequence differs: %s' % (i, e))
    finally:
        op.close()


def test_second_stream_released_and_created_again(hip):
    n = 300
    etas = numpy.array([0.03, 0.5, 2.0])     # two-stream halves 1 + 2
    batch = lambda op: op.loglik_batch(etas)
    ref = _fresh(hip, n, batch, max_batch=3)
    assert numpy.all(ref[2] == 0)
    op = _operator(hip, n, max_batch=3)
    try:
        first = batch(op)
        second = batch(op)                   # creates the released stream again
        ld0 = op.logdet(etas[0])             # single eta, on the batch's cached factor
    finally:
        op.close()
    _assert_same(first, ref)
    _assert_same(second, ref)
    assert ld0 == ref[0][0]
    assert ld0 == _fresh(hip, n, lambda o: o.logdet(etas[0]), max_batch=3)


def test_grouped_orders_rebuilt_by_set_outer(hip, monkeypatch):
    n = 1000
    etas = numpy.array([0.03, 0.5, 2.0])
    batch = lambda op: op.loglik_batch(etas)
    monkeypatch.setenv('GPMI_GROUPS', '1')   # read at create: the batch on one stream
    one = _operator(hip, n, outer=4, max_batch=3)
    monkeypatch.delenv('GPMI_GROUPS')
    two = _operator(hip, n, outer=4, max_batch=3)
    try:
        ref = batch(two)
        assert numpy.all(ref[2] == 0)
        _assert_same(batch(one), ref)
        one.set_outer(2)
        two.set_outer(2)
        ref2 = _fresh(hip, n, batch, outer=2, max_batch=3)
        _assert_same(batch(one), ref2)
        _assert_same(batch(two), ref2)
    finally:
        one.close()
        two.close()


def test_create_and_close_in_a_row(hip):
    vals = [_fresh(hip, 300, lambda op: op.logdet(0.03)) for _ in range(20)]
    assert numpy.isfinite(vals[0]) and all(v == vals[0] for v in vals)
