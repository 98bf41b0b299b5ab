"""Leave-one-out terms at scale on one GPU: MixedCorrelation.loo_terms (W = L^-T from the
cached factor, one fused pass over its upper block triangle) with, from the same process,
the two yardsticks of the pass: a device-to-device hipMemcpy of the bytes of W the pass
reads (bandwidth), and gpmi_op_solve on the same columns with the factor cached, the
backward chain the pass replaces for S^-1 [X z]. cfg3 inputs (128 x 128 grid, N = 16384,
scale 0.1), nu = 0.5, eta = 1e-2, m + 1 = 4 resident columns. Prints one JSON line.

  python tools/loo_bench.py [--grid 128] [--repeats 7] [--warmup 2]
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
from gaussian_proc._mixed_correlation import MixedCorrelation  # noqa: E402
from oracle import data  # noqa: E402


def hip_runtime():
    """The HIP runtime libgpmi.so has loaded into this process (the same one, so that the
    copy below runs on the device context the operator uses)."""
    with open('/proc/self/maps') as fh:
        for line in fh:
            if 'libamdhip64' in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError('libgpmi.so has not loaded a HIP runtime')


def d2d_copy_ms(nbytes, repeats, warmup):
    """Median ms (HIP events) of a device-to-device hipMemcpy of nbytes."""
    hip = hip_runtime()
    vp = ctypes.c_void_p

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError('%s failed (%d)' % (what, rc))

    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    n = ctypes.c_size_t(int(nbytes))
    ok(hip.hipMalloc(ctypes.byref(src), n), 'hipMalloc')
    ok(hip.hipMalloc(ctypes.byref(dst), n), 'hipMalloc')
    ok(hip.hipMemset(src, 0, n), 'hipMemset')
    ok(hip.hipEventCreate(ctypes.byref(e0)), 'hipEventCreate')
    ok(hip.hipEventCreate(ctypes.byref(e1)), 'hipEventCreate')
    ms = []
    for i in range(warmup + repeats):
        ok(hip.hipEventRecord(e0, None), 'hipEventRecord')
        ok(hip.hipMemcpyAsync(dst, src, n, 3, None), 'hipMemcpyAsync')   # 3: device to device
        ok(hip.hipEventRecord(e1, None), 'hipEventRecord')
        ok(hip.hipEventSynchronize(e1), 'hipEventSynchronize')
        t = ctypes.c_float()
        ok(hip.hipEventElapsedTime(ctypes.byref(t), e0, e1), 'hipEventElapsedTime')
        if i >= warmup:
            ms.append(t.value)
    for ev in (e0, e1):
        ok(hip.hipEventDestroy(ev), 'hipEventDestroy')
    for p in (src, dst):
        ok(hip.hipFree(p), 'hipFree')
    return float(numpy.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    nu, scale, eta = 0.5, 0.1, 1e-2
    pts = data.generate_points(a.grid, 2, True)
    z = data.generate_data(pts, 0.2)
    X = data.generate_basis_functions(pts, 1)          # m = 3: 1, x, y
    n = pts.shape[0]
    R = numpy.column_stack([X, z])
    D = gaussian_proc.generate_correlation(pts, scale, nu, device_resident=True)
    mc = MixedCorrelation(D, imate_method='cholesky')
    mc.op.set_timing(True)
    mc.set_rhs(X, z)
    t0 = time.perf_counter()
    mc.logdet(eta)                                      # factorizes
    factor_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    dinv, sol, G = mc.loo_terms(eta, X, z)              # cold: builds W
    cold_ms = 1e3 * (time.perf_counter() - t0)
    for _ in range(a.warmup):
        mc.loo_terms(eta, X, z)
    wall, dev = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        dinv, sol, G = mc.loo_terms(eta, X, z)
        wall.append(1e3 * (time.perf_counter() - t0))
        t = mc.op.loo_ms()
        dev.append(t['pass_ms'])
    pass_ms = float(numpy.median(dev))
    nbytes = t['pass_bytes']
    copy_ms = d2d_copy_ms(nbytes, a.repeats, a.warmup)
    # the backward chain on the same cached factor and the same columns
    mc.solve(eta, R)
    solve = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        W = mc.solve(eta, R)
        solve.append(1e3 * (time.perf_counter() - t0))
    out = {
        'tool': 'loo_bench', 'n': n, 'cols': R.shape[1], 'nu': nu, 'eta': eta,
        'repeats': a.repeats, 'warmup': a.warmup,
        'factorization_ms': round(factor_ms, 2),
        'loo_terms_cold_ms_factor_cached_w_not': round(cold_ms, 2),
        'loo_terms_warm_wall_ms_median': round(float(numpy.median(wall)), 3),
        'loo_terms_warm_wall_ms_min_max': [round(min(wall), 3), round(max(wall), 3)],
        'pass_ms_median': round(pass_ms, 4),
        'pass_ms_min_max': [round(min(dev), 4), round(max(dev), 4)],
        'pass_bytes': nbytes,
        'pass_gb_per_s': round(nbytes / (pass_ms * 1e-3) / 1e9, 1),
        'd2d_copy_same_bytes_ms_median': round(copy_ms, 4),
        'd2d_copy_gb_per_s_read_plus_write': round(2 * nbytes / (copy_ms * 1e-3) / 1e9, 1),
        'solve_same_cols_factor_cached_wall_ms_median': round(float(numpy.median(solve)), 3),
        'solve_same_cols_wall_ms_min_max': [round(min(solve), 3), round(max(solve), 3)],
        'max_rel_diff_sol_vs_solve': float(numpy.max(numpy.abs(sol - W)) /
                                           numpy.max(numpy.abs(W))),
        'sum_dinv_minus_traceinv_rel': float(abs(numpy.sum(dinv) - mc.traceinv(eta, 1)) /
                                             mc.traceinv(eta, 1)),
    }
    print(json.dumps(out))


if __name__ == '__main__':
    main()
