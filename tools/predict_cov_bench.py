"""Joint covariance of the new points at scale on one GPU: MixedCorrelation.predict_cov_terms
(cross assemblies, wide forward substitution keeping V = L^-1 K*^T, split-depth SYRK
C0 = K** - V V^T on fp64 MFMA) against the route that existed before it,
W = MixedCorrelation.solve(eta, K*^T) in 16-column passes and K** - K* W on the host, in
the same process. cfg3 inputs (128 x 128 grid, N = 16384, scale 0.1), nu = 0.5,
eta = 1e-2, n* = 4096 and n* = 256 random points. Both routes run on the cached factor.
Prints one JSON line.

  python tools/predict_cov_bench.py [--grid 128] [--nstar 4096,256] [--repeats 5]
                                    [--warmup 2]
                                    [--solve-cols N]  (columns of the old route's solve;
                                                       default all; its time is scaled)
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
from gaussian_proc._mixed_correlation import MixedCorrelation  # noqa: E402
from oracle import data  # noqa: E402

FP64_MFMA_PEAK_TFLOPS = 78.6    # MI355X fp64 matrix, dense (AMD spec), as bench.py


def one_size(mc, pts, X, z, nstar, a, nu, scale, eta):
    tst = numpy.random.RandomState(nstar).rand(nstar, 2)
    for _ in range(a.warmup):
        mc.predict_cov_terms(eta, X, z, test_points=tst)
    wall, prod, frac, terms = [], [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        c, q, G, C0 = mc.predict_cov_terms(eta, X, z, test_points=tst)
        wall.append(1e3 * (time.perf_counter() - t0))
        t = mc.op.predict_cov_ms()
        prod.append(t['product_ms'])
        frac.append(t['product_flops'] / (t['product_ms'] * 1e-3) / 1e12 /
                    FP64_MFMA_PEAK_TFLOPS if t['product_ms'] > 0 else 0.0)
        t0 = time.perf_counter()
        mc.predict_terms(eta, X, z, test_points=tst)
        terms.append(1e3 * (time.perf_counter() - t0))
    # the parent route on the same cached factor
    Ks = gaussian_proc.generate_cross_correlation(tst, pts, scale, nu)
    Kss = gaussian_proc.generate_cross_correlation(tst, tst, scale, nu)
    cols = min(a.solve_cols or nstar, nstar)
    B = numpy.ascontiguousarray(Ks.T[:, :cols])
    mc.solve(eta, B[:, :16])                                     # warm-up: one pass
    t0 = time.perf_counter()
    W = mc.solve(eta, B)
    solve_ms = 1e3 * (time.perf_counter() - t0) * nstar / cols
    t0 = time.perf_counter()
    C_old = Kss[:, :cols] - Ks @ W
    host_ms = 1e3 * (time.perf_counter() - t0) * nstar / cols
    med = float(numpy.median(wall))
    return {
        'nstar': nstar, 'split': t['split'],
        'predict_cov_wall_ms_median': round(med, 3),
        'predict_cov_wall_ms_min_max': [round(min(wall), 3), round(max(wall), 3)],
        'predict_terms_wall_ms_median': round(float(numpy.median(terms)), 3),
        'product_ms_median': round(float(numpy.median(prod)), 4),
        'product_flops': t['product_flops'],
        'product_mfma_frac_median': round(float(numpy.median(frac)), 4),
        'parent_route_solve_cols': cols,
        'parent_route_solve_ms': round(solve_ms, 2),
        'parent_route_host_product_ms': round(host_ms, 2),
        'parent_route_ms': round(solve_ms + host_ms, 2),
        'parent_route_over_predict_cov': round((solve_ms + host_ms) / med, 2),
        'max_abs_diff_vs_parent_route': float(numpy.max(numpy.abs(C0[:, :cols] - C_old))),
        'symmetric': bool(numpy.array_equal(C0, C0.T)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=128)
    ap.add_argument('--nstar', default='4096,256')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--solve-cols', type=int, default=0)
    a = ap.parse_args()
    nu, scale, eta = 0.5, 0.1, 1e-2
    pts = data.generate_points(a.grid, 2, True)
    z = data.generate_data(pts, 0.2)
    X = data.generate_basis_functions(pts, 2)
    D = gaussian_proc.generate_correlation(pts, scale, nu, device_resident=True)
    mc = MixedCorrelation(D, imate_method='cholesky')
    mc.op.set_timing(True)
    t0 = time.perf_counter()
    mc.predict_terms(eta, X, z, test_points=pts[:1])            # factorizes
    first_ms = 1e3 * (time.perf_counter() - t0)
    out = {
        'tool': 'predict_cov_bench', 'n': pts.shape[0], 'nu': nu, 'eta': eta,
        'repeats': a.repeats, 'warmup': a.warmup,
        'first_call_with_factorization_ms': round(first_ms, 2),
        'fp64_mfma_peak_tflops': FP64_MFMA_PEAK_TFLOPS,
        'sizes': [one_size(mc, pts, X, z, int(s), a, nu, scale, eta)
                  for s in a.nstar.split(',')],
    }
    print(json.dumps(out))


if __name__ == '__main__':
    main()
