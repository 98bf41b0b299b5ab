"""Joint posterior draws at scale on one GPU: GaussianProcess.sample (resident covariance
C0 = K** - V V^T, C0 + U U^T handed to a second dense operator on the device, its batched
fp64-MFMA Cholesky, device normals, triangular product Y_t = Xi_t L^T on fp64 MFMA) against
the route that existed before it, predict(..., return_cov=True), numpy.linalg.cholesky of
the n* x n* covariance and a matmul on the host, in the same process. cfg3 inputs
(128 x 128 grid, N = 16384, scale 0.1), nu = 0.5, hyperparam (1, 0.1) so eta = 1e-2,
noise=True, n* = 4096 and 256 random points, 1024 and 128 draws. Both routes run on the
cached factor of K + eta I. Wall times are medians of repeated calls after warm-up, device
parts HIP events (gpmi_op_sample_ms). --depths lists piece depths (GPMI_SAMPLE_DEPTH; 0: the
plan's choice) whose product time is reported side by side. Prints one JSON line.

  python tools/sample_bench.py [--grid 128] [--nstar 4096,256] [--sizes 1024,128]
                               [--repeats 9] [--warmup 2] [--host-repeats 3]
                               [--depths 0,1,2,4,8,16,32]
"""
import argparse
import json
import os
import sys
import time

import numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'gaussian-process-param-estimation_amd')]
import gaussian_proc  # noqa: E402
from gaussian_proc import _hip  # noqa: E402
from gaussian_proc._likelihood._profile_likelihood import _sample_lowrank_from_terms  # noqa: E402
from oracle import data  # noqa: E402

FP64_MFMA_PEAK_TFLOPS = 78.6    # MI355X fp64 matrix, dense (AMD spec), as bench.py


def _ms(f):
    t0 = time.perf_counter()
    r = f()
    return 1e3 * (time.perf_counter() - t0), r


def _median_ms(f, a):
    for _ in range(a.warmup):
        f()
    t = [_ms(f)[0] for _ in range(a.repeats)]
    return round(float(numpy.median(t)), 3), [round(min(t), 3), round(max(t), 3)]


def _frac(t):
    return t['trmm_flops'] / (t['trmm_ms'] * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS \
        if t['trmm_ms'] > 0 else 0.0


def one_shape(g, z, hp, nstar, size, a):
    mc = g.likelihood.K_mixed
    X = numpy.asarray(g.X, dtype=float)
    tst = numpy.random.RandomState(nstar).rand(nstar, 2)
    Xs = data.generate_basis_functions(tst, 2)
    eta = (hp[1] / hp[0]) ** 2
    kw = dict(z=z, hyperparam=hp, noise=True)
    whole, whole_mm = _median_ms(lambda: g.sample(tst, Xs, size=size, seed=1, **kw), a)
    # the parts, each on its own
    mc.set_rhs(X, z)
    pk = dict(test_points=tst, points=mc.K.points, scale=numpy.asarray(
        mc.K.correlation_scale, dtype=float) * numpy.ones(2), nu=mc.K.nu)
    res, _ = _median_ms(lambda: mc.op.predict_cov_resident(eta, **pk), a)
    c, _, G = mc.op.predict_cov_resident(eta, **pk)
    U = _sample_lowrank_from_terms(c, G, Xs)
    child = _hip.Operator(nstar, device=mc.op.device)
    child.set_timing(True)
    load, _ = _median_ms(lambda: child.load_predict_cov(mc.op, U), a)

    def factor():
        child.load_predict_cov(mc.op, U)     # drops the cached factor
        return _ms(lambda: child.logdet(eta))[0]
    fac = round(float(numpy.median([factor() for _ in range(a.warmup + a.repeats)][a.warmup:])), 3)
    wall, nrm, prod, frac = [], [], [], []
    for i in range(a.warmup + a.repeats):
        w, _ = _ms(lambda: child.sample(eta, size, seed=1))
        t = child.sample_ms()
        if i >= a.warmup:
            wall.append(w), nrm.append(t['normal_ms']), prod.append(t['trmm_ms'])
            frac.append(_frac(t))
    draw = float(numpy.median(wall))
    ab = {}
    for d in [int(x) for x in a.depths.split(',') if x != '']:
        if d:
            os.environ['GPMI_SAMPLE_DEPTH'] = str(d)
        else:
            os.environ.pop('GPMI_SAMPLE_DEPTH', None)
        ts = []
        for i in range(a.warmup + a.repeats):
            child.sample(eta, size, seed=1)
            if i >= a.warmup:
                ts.append(child.sample_ms()['trmm_ms'])
        ab[str(d)] = round(float(numpy.median(ts)), 4)
    os.environ.pop('GPMI_SAMPLE_DEPTH', None)
    dev = child.sample(eta, size, seed=1)
    child.close()
    # the route that existed before, on the same cached factor
    host_cov, host_chol, host_mm = [], [], []
    for _ in range(a.host_repeats):
        t0, (mean, cov) = _ms(lambda: g.predict(tst, Xs, return_cov=True, **kw))
        t1, L = _ms(lambda: numpy.linalg.cholesky(cov))
        xi = numpy.random.RandomState(0).randn(nstar, size)
        t2, old = _ms(lambda: mean[None, :] + (L @ xi).T)
        host_cov.append(t0), host_chol.append(t1), host_mm.append(t2)
    host = [float(numpy.median(v)) for v in (host_cov, host_chol, host_mm)]
    # the device draws' second moments against the host covariance, in standard errors
    S = dev.T @ dev / size
    d = numpy.diag(cov) / hp[0] ** 2
    se = numpy.sqrt((numpy.outer(d, d) + (cov / hp[0] ** 2) ** 2) / size)
    return {
        'nstar': nstar, 'size': size,
        'sample_wall_ms_median': whole, 'sample_wall_ms_min_max': whole_mm,
        'resident_cov_ms': res, 'load_ms': load, 'child_factor_ms': fac,
        'draw_call_ms': round(draw, 3),
        'normals_ms': round(float(numpy.median(nrm)), 4),
        'product_ms': round(float(numpy.median(prod)), 4),
        'download_and_host_ms': round(draw - float(numpy.median(nrm)) -
                                      float(numpy.median(prod)), 3),
        'product_flops': t['trmm_flops'],
        'product_mfma_frac_median': round(float(numpy.median(frac)), 4),
        'product_ms_by_depth': ab,
        'host_route_predict_cov_ms': round(host[0], 2),
        'host_route_cholesky_ms': round(host[1], 2),
        'host_route_matmul_ms': round(host[2], 2),
        'host_route_ms': round(sum(host), 2),
        'host_route_over_sample': round(sum(host) / whole, 2),
        'max_second_moment_deviation_se': round(float(numpy.max(numpy.abs(S - cov / hp[0] ** 2)
                                                                / se)), 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=128)
    ap.add_argument('--nstar', default='4096,256')
    ap.add_argument('--sizes', default='1024,128')
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--depths', default='')
    a = ap.parse_args()
    nu, scale, hp = 0.5, 0.1, (1.0, 0.1)
    pts = data.generate_points(a.grid, 2, True)
    z = data.generate_data(pts, 0.2)
    X = data.generate_basis_functions(pts, 2)
    D = gaussian_proc.generate_correlation(pts, scale, nu, device_resident=True)
    g = gaussian_proc.GaussianProcess(X, D)
    t0 = time.perf_counter()
    g.predict(pts[:1], X[:1], z=z, hyperparam=hp)               # factorizes
    first_ms = 1e3 * (time.perf_counter() - t0)
    out = {
        'tool': 'sample_bench', 'n': pts.shape[0], 'nu': nu, 'eta': (hp[1] / hp[0]) ** 2,
        'repeats': a.repeats, 'warmup': a.warmup, 'host_repeats': a.host_repeats,
        'host_cpus': len(os.sched_getaffinity(0)),
        'omp_num_threads': os.environ.get('OMP_NUM_THREADS'),
        'first_call_with_factorization_ms': round(first_ms, 2),
        'fp64_mfma_peak_tflops': FP64_MFMA_PEAK_TFLOPS,
        'covariance_product_mfma_frac_at_4096': 0.78,
        'shapes': [one_shape(g, z, hp, int(s), int(k), a)
                   for s in a.nstar.split(',') for k in a.sizes.split(',')],
    }
    print(json.dumps(out))


if __name__ == '__main__':
    main()
