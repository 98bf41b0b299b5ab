"""The likelihood's correlation-scale gradient at scale on one GPU:
MixedCorrelation.scale_grad_terms (the factor, W = L^-T, the tiles of A^-1 = W W^T, one
fused pass over them) timed with each of its ingredients cached or not, the pass's rate
beside the leave-one-out pass's in the same process (both read 8 * 128^2 * nt (nt + 1) / 2
bytes), and the route without it: central differences of the log-likelihood, 2 d
re-assemblies and factorizations. Then the same comparison at d = 8, and one
GaussianProcess.train_scale. cfg3 inputs (128 x 128 grid, N = 16384), nu = 1.5,
eta = 1e-2, m + 1 = 4 resident columns. Prints one JSON line.

  python tools/scale_grad_bench.py [--grid 128] [--repeats 5] [--no-train]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'gaussian-process-param-estimation_amd')]
import gaussian_proc  # noqa: E402
from gaussian_proc._mixed_correlation import MixedCorrelation  # noqa: E402
from gaussian_proc._likelihood._profile_likelihood import _scale_grad_from_terms  # noqa: E402
from oracle import data  # noqa: E402


def wall_ms(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def profiled_lp(mc, X, z, eta):
    n, m = X.shape
    ld, G = mc.loglik_terms([eta], X, z)
    G = G[0]
    zPz = G[m, m] - G[:m, m] @ numpy.linalg.solve(G[:m, :m], G[:m, m])
    return -0.5 * (n - m) * numpy.log(zPz / (n - m)) - 0.5 * ld[0] \
        - 0.5 * numpy.linalg.slogdet(G[:m, :m])[1]


def compare(pts, X, z, rho, nu, eta, repeats):
    """The analytic gradient and the central differences on one operator -> dict."""
    n, m = X.shape
    d = pts.shape[1]
    D = gaussian_proc.generate_correlation(pts, rho, nu, device_resident=True)
    mc = MixedCorrelation(D, imate_method='cholesky')
    mc.op.set_timing(True)
    mc.set_rhs(X, z)
    factor_ms, _ = wall_ms(lambda: mc.logdet(eta))
    cold_ms, T = wall_ms(lambda: mc.scale_grad_terms(eta, X, z))      # builds W and A^-1
    eta2 = eta * (1.0 + 1e-9)                                         # another factorization
    mc.logdet(eta2)
    w_ms, _ = wall_ms(lambda: mc.traceinv(eta2, 1))                   # builds W
    ainv_ms, _ = wall_ms(lambda: mc.scale_grad_terms(eta2, X, z))     # builds A^-1
    warm, dev, loo = [], [], []
    for _ in range(repeats):
        ms, T = wall_ms(lambda: mc.scale_grad_terms(eta2, X, z))
        warm.append(ms)
        dev.append(mc.op.scale_grad_ms()['pass_ms'])
        loo.append(mc.op.loo_ms()['pass_ms'])
    nbytes = mc.op.scale_grad_ms()['pass_bytes']
    grad = _scale_grad_from_terms(n, m, T['t'], T['qX'], T['qc'], T['G'])
    rho = numpy.asarray(rho, dtype=float)

    def differences():
        g = numpy.empty(d)
        for k in range(d):
            vals = []
            for sgn in (1.0, -1.0):
                r = rho.copy()
                r[k] *= 1.0 + sgn * 1e-5
                D.set_correlation_scale(r)
                vals.append((profiled_lp(mc, X, z, eta2), r[k]))
            g[k] = (vals[0][0] - vals[1][0]) / (vals[0][1] - vals[1][1])
        D.set_correlation_scale(rho)
        return g

    fd_ms, fd = wall_ms(differences)
    pass_ms, loo_ms = float(numpy.median(dev)), float(numpy.median(loo))
    return {
        'n': n, 'd': d, 'cols': m + 1, 'nu': nu, 'eta': eta,
        'factorization_ms': round(factor_ms, 2),
        'terms_ms_factor_cached_w_not': round(cold_ms, 2),
        'traceinv1_ms_builds_w': round(w_ms, 2),
        'terms_ms_w_cached_ainv_not': round(ainv_ms, 2),
        'terms_ms_all_cached_median': round(float(numpy.median(warm)), 3),
        'terms_ms_all_cached_min_max': [round(min(warm), 3), round(max(warm), 3)],
        'pass_ms_median': round(pass_ms, 4),
        'pass_ms_min_max': [round(min(dev), 4), round(max(dev), 4)],
        'pass_bytes': nbytes,
        'pass_gb_per_s': round(nbytes / (pass_ms * 1e-3) / 1e9, 1),
        'loo_pass_ms_median': round(loo_ms, 4),
        'loo_pass_gb_per_s': round(nbytes / (loo_ms * 1e-3) / 1e9, 1),
        'analytic_gradient_ms_from_nothing': round(factor_ms + cold_ms, 2),
        'central_differences_ms_2d_assemblies_and_factorizations': round(fd_ms, 2),
        'gradient': [float(v) for v in grad],
        'max_rel_diff_vs_central_differences': float(numpy.max(numpy.abs(grad - fd)) /
                                                     numpy.max(numpy.abs(fd))),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-train', action='store_true')
    a = ap.parse_args()
    nu, eta = 1.5, 1e-2
    pts = data.generate_points(a.grid, 2, True)
    z = data.generate_data(pts, 0.2)
    X = data.generate_basis_functions(pts, 1)          # m = 3: 1, x, y
    n = pts.shape[0]
    # discarded: the process's first use of the kernels and of 2 GB blocks of the allocator
    compare(pts, X, z, [0.1, 0.1], nu, eta, 1)
    out = {'tool': 'scale_grad_bench', 'repeats': a.repeats,
           'd2': compare(pts, X, z, [0.1, 0.1], nu, eta, a.repeats)}
    rng = numpy.random.RandomState(0)
    p8 = rng.rand(n, 8)
    z8 = numpy.sin(3 * p8[:, 0]) + p8[:, 7] + 0.1 * rng.randn(n)
    X8 = numpy.column_stack([numpy.ones(n), p8[:, 0], p8[:, 7]])
    out['d8'] = compare(p8, X8, z8, numpy.linspace(0.8, 1.5, 8), nu, eta, a.repeats)
    if not a.no_train:
        D = gaussian_proc.generate_correlation(pts, [0.05, 0.05], nu, device_resident=True)
        g = gaussian_proc.GaussianProcess(X, D)
        with contextlib.redirect_stdout(io.StringIO()):
            ms, _ = wall_ms(lambda: g.train_scale(z, eta0=1.0))
        r = g.results
        out['train_scale'] = {
            'n': n, 'd': 2, 'nu': nu, 'start_scale': [0.05, 0.05], 'start_eta': 1.0,
            'wall_ms': round(ms, 1), 'iterations': r['iterations'],
            'evaluations': r['evaluations'], 'success': r['success'],
            'ms_per_evaluation': round(ms / max(1, r['evaluations']), 1),
            'eta': r['eta'], 'correlation_scale': [float(v) for v in r['correlation_scale']],
            'sigma': r['sigma'], 'sigma0': r['sigma0'], 'max_lp': r['max_lp']}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
