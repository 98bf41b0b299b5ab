"""Digests of the dense operator's results, to compare two builds of libgpmi bit for bit:
one SHA-256 per call over the raw bytes of what it returns, for loglik_batch, logdet,
solve, traceinv 1 and 2, predict_terms, predict_cov, matvec and trace, at the sizes,
outer panel widths and batches of tests/test_gpu_dense_kloop.py's CASES with
n = 300 / 1000 / 2100. Inputs are seeded; a refactor of the host side leaves every line
unchanged.

  python tools/dense_digest.py > new.txt
  GPMI_LIB_VARIANT=<name> python tools/dense_digest.py > old.txt    (libgpmi_<name>.so)
  diff old.txt new.txt
"""
import hashlib
import os
import sys

import numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'gaussian-process-param-estimation_amd')]
from gaussian_proc import _hip  # noqa: E402
from oracle import matern  # noqa: E402

CASES = [(300, 16, 1), (300, 16, 3), (300, 16, 33), (1000, 4, 1), (1000, 4, 3), (2100, 16, 2)]
SCALE, NU = 0.2, 1.5


def digest(result):
    h = hashlib.sha256()
    for a in result if isinstance(result, tuple) else (result,):
        h.update(numpy.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    _hip.require_device(0)
    inputs = {}
    for n, outer, batch in CASES:
        if n not in inputs:
            rng = numpy.random.RandomState(n)
            pts = rng.rand(n, 2)
            z = numpy.sin(3 * pts[:, 0]) + 0.1 * rng.randn(n)
            inputs[n] = (matern.dense_correlation(pts, SCALE, NU), pts,
                         numpy.column_stack([numpy.ones(n), pts, z]), rng.rand(200, 2))
        K, pts, R, tst = inputs[n]
        scale = numpy.full(2, SCALE)
        etas = numpy.logspace(-2, 1, batch)
        eta = 0.03
        op = _hip.Operator(n, device=0, max_batch=batch)
        op.load_matrix(K)
        op.set_rhs(R)
        op.set_outer(outer)
        calls = [
            ('loglik_batch', lambda: op.loglik_batch(etas)),
            ('logdet', lambda: numpy.float64(op.logdet(eta))),
            ('solve', lambda: op.solve(eta, R)),
            ('traceinv1', lambda: numpy.float64(op.traceinv(eta, 1))),
            ('traceinv2', lambda: numpy.float64(op.traceinv(eta, 2))),
            ('predict_terms', lambda: op.predict_terms(eta, test_points=tst, points=pts,
                                                       scale=scale, nu=NU)),
            ('predict_cov', lambda: op.predict_cov(eta, test_points=tst[:130], points=pts,
                                                   scale=scale, nu=NU)),
            ('matvec', lambda: op.matvec(R)),
            ('trace', lambda: numpy.array(op.trace())),
        ]
        for name, call in calls:
            print('n=%d outer=%d batch=%d %s %s' % (n, outer, batch, name, digest(call())),
                  flush=True)
        op.close()


if __name__ == '__main__':
    main()
