"""Prediction on a sparse K at scale on one GPU: MixedCorrelation.predict_terms on a
DeviceSparseCorrelation K (cross assembly by cell list, device-resident CGs) against the
route that existed before it, in the same process: generate_cross_correlation's dense K*
thresholded on the host, MixedCorrelation.solve(eta, K*^T) with the same cg_rtol, host
products. BASELINE cfg 4 (256 x 256 grid, n = 65536) with 256 and 1024 new points and
cfg 5 (64^3 grid, n = 262144) with 256, basis and eta grid as bench.py's sparse configs
(the eta of index --eta-index of that grid, default its middle). Per case: the cross
assembly (cell list, all pairs), the mean-only call, and for each variance block width
(GPMI_SP_PREDICT_S) the device-resident SpMM per launch (gpmi_sp_bench_spmm) and the whole
call with its iterations and SpMM launches per width. Both routes: medians with [min, max] after a
warm-up. Prints one JSON line (--out FILE: also written there, indented).

  python tools/sparse_predict_bench.py [--cases sparse4:256,sparse4:1024,sparse5:256]
                                       [--widths 32,20,16] [--repeats 5] [--warmup 2]
                                       [--eta-index 16] [--old-cols N] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'gaussian-process-param-estimation_amd')]
import gaussian_proc  # noqa: E402
from gaussian_proc import _hip, _slq  # noqa: E402
from gaussian_proc._mixed_correlation import MixedCorrelation  # noqa: E402
from oracle import data  # noqa: E402

# bench.py's SPARSE_CONFIGS: points per axis, dimension, rho, nu, density, probes, steps, etas
CONFIGS = {
    'sparse4': (256, 2, 0.005, 1.5, 1e-3, 20, 30, 32),
    'sparse5': (64, 3, 0.02, 1.5, 6e-4, 20, 30, 32),
}


def stats(ms):
    return {'median_ms': round(float(numpy.median(ms)), 3),
            'min_max_ms': [round(float(min(ms)), 3), round(float(max(ms)), 3)]}


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


class Model(object):
    """One config's K, operator, basis and eta (shared by its cases)."""

    def __init__(self, config, eta_index):
        npts, dim, rho, nu, dens, nprobe, steps, neta = CONFIGS[config]
        self.config, self.dim, self.rho, self.nu = config, dim, rho, nu
        self.pts = data.generate_points(npts, dim, True)
        self.z = data.generate_data(self.pts, 0.2)
        self.X = data.generate_basis_functions(self.pts, 2)
        t0 = time.perf_counter()
        self.D = gaussian_proc.generate_correlation(self.pts, rho, nu, sparse=True, density=dens,
                                                    device_resident=True)
        self.create_ms = 1e3 * (time.perf_counter() - t0)
        self.mc = MixedCorrelation(self.D, imate_method='slq',
                                   imate_options={'num_samples': nprobe,
                                                  'lanczos_degree': steps})
        theta_min = _slq.min_ritz(self.mc.slq_nodes())
        self.shift = max(0.0, -1.1 * theta_min)
        self.eta = float((numpy.logspace(-2, 2, neta) + self.shift)[eta_index])
        self.R = numpy.column_stack([self.X, self.z])


def run_case(M, nstar, a):
    sop, mc = M.mc.sop, M.mc
    n = M.pts.shape[0]
    tst = numpy.ascontiguousarray(numpy.random.RandomState(0).rand(nstar, M.dim))
    nnz = ctypes.c_int64()

    def assemble():
        _hip.check(sop.lib.gpmi_sp_cross_matern(sop.h, _hip.dptr(tst), nstar, M.dim,
                                                ctypes.byref(nnz)), 'gpmi_sp_cross_matern')

    out = {'config': M.config, 'n': n, 'nnz': sop.nnz, 'nstar': nstar, 'eta': M.eta,
           'eta_shift': M.shift, 'basis_columns': M.X.shape[1], 'cg_rtol': mc.cg_rtol,
           'create_ms': round(M.create_ms, 1)}
    out['cross_cell_list'] = stats(timed(assemble, a.repeats, a.warmup))
    os.environ['GPMI_SPARSE_BRUTE'] = '1'
    out['cross_all_pairs'] = stats(timed(assemble, a.repeats, a.warmup))
    del os.environ['GPMI_SPARSE_BRUTE']
    out['cross_nnz'] = nnz.value
    out['cross_empty_rows'] = int(numpy.sum(numpy.diff(sop.cross(tst).indptr) == 0))
    def mean_only():
        w = stats(timed(
            lambda: mc.predict_terms(M.eta, M.X, M.z, test_points=tst, return_q=False),
            a.repeats, a.warmup))
        w['iterations'] = sop.last_predict_iterations[0]
        return w

    # (timed again after the full calls below: the first measurement of a process runs on
    # a device and a workspace that the full calls have not yet warmed and grown)
    out['mean_only_before_full_calls'] = mean_only()
    widths = {}
    for s in a.widths:
        os.environ['GPMI_SP_PREDICT_S'] = str(s)
        ms = timed(lambda: mc.predict_terms(M.eta, M.X, M.z, test_points=tst), a.repeats,
                   a.warmup)
        sop.set_timing(True)
        c, q, G = mc.predict_terms(M.eta, M.X, M.z, test_points=tst)
        sop.set_timing(False)
        w = stats(ms)
        w['iterations_R_solve_and_most_of_a_block'] = list(sop.last_predict_iterations)
        w['spmm_launches_and_ms_by_width'] = {str(k): [v[0], round(v[1], 3)]
                                              for k, v in sop.spmm_timing().items()}
        w['spmm_kernel'] = sop.spmm_kernel(s)
        w['bench_spmm_us_per_launch'] = round(1e3 * sop.bench_spmm(s, 50, M.eta), 2)
        widths[str(s)] = w
    del os.environ['GPMI_SP_PREDICT_S']
    out['full_call_by_block_width'] = widths
    out['mean_only'] = mean_only()
    c, q, G = mc.predict_terms(M.eta, M.X, M.z, test_points=tst)    # the default width
    # the route that existed before: dense K*, thresholded on the host, solve, products;
    # warmed up and repeated like the new route
    cols = min(nstar, a.old_cols or nstar)
    parts = []
    for run in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        Ks = gaussian_proc.generate_cross_correlation(tst[:cols], M.pts, M.rho, M.nu)
        Ks[Ks <= M.D.tau] = 0.0
        B = numpy.ascontiguousarray(Ks.T)
        t1 = time.perf_counter()
        W = mc.solve(M.eta, B)
        t2 = time.perf_counter()
        c_old = W.T @ M.R
        q_old = numpy.sum(B * W, axis=0)
        t3 = time.perf_counter()
        if run >= a.warmup:
            parts.append([1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t3 - t0)])
    parts = numpy.array(parts)
    old_ms = float(numpy.median(parts[:, 3]))
    out['old_route'] = {
        'columns': cols, 'cross_dense_and_threshold': stats(list(parts[:, 0])),
        'solve': stats(list(parts[:, 1])), 'host_products': stats(list(parts[:, 2])),
        'total': stats(list(parts[:, 3])),
        'total_median_ms_scaled_to_nstar': round(old_ms * nstar / cols, 1),
        'host_block_bytes': int(B.nbytes), 'runs': a.repeats, 'warmup': a.warmup,
        'max_abs_diff_c': float(numpy.max(numpy.abs(c[:cols] - c_old))),
        'max_abs_diff_q': float(numpy.max(numpy.abs(q[:cols] - q_old))),
        'max_abs_c': float(numpy.max(numpy.abs(c_old))),
        'max_abs_q': float(numpy.max(numpy.abs(q_old)))}
    best = min(widths.values(), key=lambda w: w['median_ms'])['median_ms']
    out['old_over_new_full_call'] = round(old_ms * nstar / cols / best, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='sparse4:256,sparse4:1024,sparse5:256')
    ap.add_argument('--widths', default='32,20,16')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--eta-index', type=int, default=16)
    ap.add_argument('--old-cols', type=int, default=0,
                    help='columns of the old route that are run (0: all; the time is scaled)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.widths = [int(s) for s in a.widths.split(',')]
    _hip.require_device(0)
    models, cases = {}, []
    for item in a.cases.split(','):
        config, nstar = item.split(':')
        if config not in models:
            models[config] = Model(config, a.eta_index)
        cases.append(run_case(models[config], int(nstar), a))
    out = {'tool': 'sparse_predict_bench', 'repeats': a.repeats, 'warmup': a.warmup,
           'widths': a.widths, 'default_width': 32, 'cases': cases}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
