// Prediction on a sparse K (include/gpmi.h: gpmi_sp_predict_terms, gpmi_sp_predict_terms_csr,
// gpmi_sp_cross_matern, gpmi_sp_get_cross): the cross CSR K* of the new points with the
// training points (assembled from the geometry the create kept, kernels: gpmi_matern.hip;
// or the caller's), then, with S = K + eta I and R = [X z],
//   Sol = S^-1 R (one CG), G = R^T Sol, c = K* Sol,
//   q_j = k*_j^T S^-1 k*_j by CGs on blocks of s <= 32 rows of K* scattered into B [n][s],
// every right-hand side and solution staying on the device (cg_block_device). Nothing of
// size n x nstar exists; only c, q, G and the iteration counts cross the bus. The handle:
// gpmi_sp.h (SpGeom, SpPredict).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <utility>
#include <vector>

#include "gpmi_sp.h"

using namespace gpmi;

namespace {

// Rows of K* per variance block. The window SpMM serves widths up to 20 and the gather
// by column pairs serves 32; measured in the whole call, GPMI_SP_PREDICT_S
// overrides.
constexpr int PREDICT_S_DEFAULT = 32;

int predict_block_width() {
  const char* e = std::getenv("GPMI_SP_PREDICT_S");
  const int s = e ? std::atoi(e) : PREDICT_S_DEFAULT;
  return std::min(MAXS, std::max(1, s));
}

// The row pointers from the host counts, the buffers of the cross CSR grown to hold it.
// (pr.nstar stays 0, "no cross CSR", until the caller's fill or upload has completed.)
int cross_reserve(gpmi_sp* sp, int64_t nstar, const std::vector<int>& cnt) {
  SpPredict& pr = sp->pred;
  pr.indptr_h.assign((size_t)nstar + 1, 0);
  for (int64_t j = 0; j < nstar; ++j) pr.indptr_h[j + 1] = pr.indptr_h[j] + cnt[j];
  pr.nnz = pr.indptr_h[nstar];
  HIP_TRY(pr.indptr.reserve((size_t)nstar + 1));
  HIP_TRY(pr.indices.reserve((size_t)std::max<int64_t>(1, pr.nnz)));
  HIP_TRY(pr.data.reserve((size_t)std::max<int64_t>(1, pr.nnz)));
  HIP_TRY(hipMemcpyAsync(pr.indptr, pr.indptr_h.data(), sizeof(int64_t) * (nstar + 1),
                        hipMemcpyHostToDevice, sp->stream));
  return 0;
}

// K* of the new points test [nstar][d] from the kept geometry: count, scan on the host,
// fill. The cell list when the create found a plan, unless GPMI_SPARSE_BRUTE=1 (read
// here, at the call) or a row holds more than CELL_CAP kept entries: then all pairs.
int cross_assemble(gpmi_sp* sp, const double* test, int64_t nstar, int d) {
  SpGeom& geo = sp->geom;
  SpPredict& pr = sp->pred;
  if (!geo.has)
    return set_error(-1108, "the handle keeps no geometry (not from gpmi_sp_create_matern): "
                            "pass the cross matrix (gpmi_sp_predict_terms_csr)");
  if (d != geo.d) return set_error(-1108, "test points of another dimension than the handle's");
  if (!test || nstar < 1 || nstar > ((int64_t)1 << 30))
    return set_error(-1100, "need 1 <= nstar <= 2^30 test points");
  hipStream_t st = sp->stream;
  pr.nstar = 0;   // (no cross CSR until this one is complete)
  HIP_TRY(pr.test.reserve((size_t)nstar * d));
  HIP_TRY(pr.cnt.reserve((size_t)nstar));
  HIP_TRY(hipMemcpyAsync(pr.test, test, sizeof(double) * nstar * d, hipMemcpyHostToDevice, st));
  const unsigned grid = (unsigned)((nstar + 3) / 4);
  const char* brute_env = std::getenv("GPMI_SPARSE_BRUTE");
  bool cells = geo.cells && !(brute_env && std::atoi(brute_env) != 0);
  if (cells) {
    hipLaunchKernelGGL(cross_cell_count_kernel, dim3(grid), dim3(256), 0, st, geo.points, nstar,
                       pr.test, d, geo.scale, geo.P, geo.tau, geo.xcut, geo.grid,
                       geo.cell_start, geo.cell_perm, pr.cnt);
    LAUNCH_CHECK("cross_cell_count_kernel");
  } else {
    hipLaunchKernelGGL(cross_count_kernel, dim3(grid), dim3(256), 0, st, geo.points, sp->n,
                       pr.test, nstar, d, geo.scale, geo.P, geo.tau, geo.xcut, pr.cnt);
    LAUNCH_CHECK("cross_count_kernel");
  }
  std::vector<int> cnt((size_t)nstar);
  HIP_TRY(hipMemcpyAsync(cnt.data(), pr.cnt, sizeof(int) * nstar, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // (the all-pairs count of a row equals its cell-list count: no recount)
  if (cells && *std::max_element(cnt.begin(), cnt.end()) > CELL_CAP_HOST) cells = false;
  if (int rc = cross_reserve(sp, nstar, cnt)) return rc;
  if (cells) {
    hipLaunchKernelGGL(cross_cell_fill_kernel, dim3(grid), dim3(256), 0, st, geo.points, nstar,
                       pr.test, d, geo.scale, geo.P, geo.tau, geo.xcut, geo.grid,
                       geo.cell_start, geo.cell_perm, geo.inv, pr.indptr, pr.indices, pr.data);
    LAUNCH_CHECK("cross_cell_fill_kernel");
  } else {
    hipLaunchKernelGGL(cross_fill_kernel, dim3(grid), dim3(256), 0, st, geo.points, sp->n,
                       pr.test, nstar, d, geo.scale, geo.P, geo.tau, geo.xcut,
                       sp->perm.empty() ? (const int*)nullptr : (const int*)sp->perm_d, pr.indptr,
                       pr.indices, pr.data);
    LAUNCH_CHECK("cross_fill_kernel");
  }
  HIP_TRY(hipStreamSynchronize(st));
  pr.nstar = nstar;
  return 0;
}

// The caller's K* (host CSR over original column indices, ascending per row): columns
// renamed to device rows and re-sorted per row, then uploaded.
int cross_upload(gpmi_sp* sp, int64_t nstar, const int64_t* indptr, const int* indices,
                 const double* data) {
  SpPredict& pr = sp->pred;
  const int64_t n = sp->n;
  if (!indptr || nstar < 1 || nstar > ((int64_t)1 << 30))
    return set_error(-1100, "need 1 <= nstar <= 2^30 rows of the cross matrix");
  if (indptr[0] != 0) return set_error(-1109, "cross CSR: indptr[0] != 0");
  for (int64_t j = 0; j < nstar; ++j)
    if (indptr[j + 1] < indptr[j] || indptr[j + 1] - indptr[j] > n)
      return set_error(-1109, "cross CSR: row pointers not ascending (or a row longer than n)");
  if (indptr[nstar] > 0 && (!indices || !data))
    return set_error(-1006, "cross CSR: null indices or data");
  for (int64_t j = 0; j < nstar; ++j) {
    for (int64_t e = indptr[j]; e < indptr[j + 1]; ++e) {
      if (indices[e] < 0 || indices[e] >= n)
        return set_error(-1109, "cross CSR: a column index outside [0, n)");
      if (e > indptr[j] && indices[e] <= indices[e - 1])
        return set_error(-1109, "cross CSR: a row's columns are not strictly ascending");
    }
  }
  pr.nstar = 0;
  std::vector<int> cnt((size_t)nstar);
  for (int64_t j = 0; j < nstar; ++j) cnt[j] = (int)(indptr[j + 1] - indptr[j]);
  const int64_t nnz = indptr[nstar];
  std::vector<int> ix((size_t)nnz);
  std::vector<double> dv((size_t)nnz);
  if (sp->perm.empty()) {
    std::copy(indices, indices + nnz, ix.begin());
    std::copy(data, data + nnz, dv.begin());
  } else {
    std::vector<int> inv((size_t)n);
    for (int64_t r = 0; r < n; ++r) inv[sp->perm[r]] = (int)r;
    std::vector<std::pair<int, double>> row;
    for (int64_t j = 0; j < nstar; ++j) {
      row.clear();
      for (int64_t e = indptr[j]; e < indptr[j + 1]; ++e)
        row.emplace_back(inv[indices[e]], data[e]);
      std::sort(row.begin(), row.end(),
                [](const std::pair<int, double>& a, const std::pair<int, double>& b) {
                  return a.first < b.first;
                });
      for (size_t e = 0; e < row.size(); ++e) {
        ix[(size_t)indptr[j] + e] = row[e].first;
        dv[(size_t)indptr[j] + e] = row[e].second;
      }
    }
  }
  if (int rc = cross_reserve(sp, nstar, cnt)) return rc;
  if (nnz > 0) {
    HIP_TRY(hipMemcpyAsync(pr.indices, ix.data(), sizeof(int) * nnz, hipMemcpyHostToDevice,
                          sp->stream));
    HIP_TRY(hipMemcpyAsync(pr.data, dv.data(), sizeof(double) * nnz, hipMemcpyHostToDevice,
                          sp->stream));
  }
  HIP_TRY(hipStreamSynchronize(sp->stream));   // (ix, dv leave with this scope)
  pr.nstar = nstar;
  return 0;
}

// c, q and G from the cross CSR in sp->pred (see the head of this file).
int predict_core(gpmi_sp* sp, double eta, const double* rhs, int64_t ld, int nrhs, int want_q,
                 double rtol, int maxiter, double* c, double* q, double* G, int* iterations) {
  SpPredict& pr = sp->pred;
  const int64_t n = sp->n, nstar = pr.nstar;
  hipStream_t st = sp->stream;
  if (!c || !G || (want_q && !q)) return set_error(-1006, "null output");
  if (!rhs && (!sp->ms.rhs_dev || nrhs != sp->ms.rhs_nrhs))
    return set_error(-1105, "predict_terms: rhs NULL needs a resident block of nrhs columns "
                            "(gpmi_sp_set_rhs)");
  if (nrhs < 1 || nrhs > MAXS || (rhs && ld < nrhs))
    return set_error(-1104, "predict_terms: need 1 <= nrhs <= 32 and ld >= nrhs");
  if (maxiter < 0 || !(rtol >= 0.0))
    return set_error(-1104, "predict_terms: need maxiter >= 0 and rtol >= 0 (not NaN)");
  const int s = nrhs;
  const int sb = predict_block_width();
  const int64_t ns = n * s;
  sp->last_converged = 0;
  bool converged = true;
  // every buffer before the first launch (reserve frees the old block)
  HIP_TRY(sp->work.ws.reserve((size_t)4 * n * std::max(s, want_q ? sb : 1)));
  HIP_TRY(pr.R.reserve((size_t)ns));
  HIP_TRY(pr.Sol.reserve((size_t)ns));
  HIP_TRY(pr.partial.reserve((size_t)NBLK * s * s));
  HIP_TRY(pr.out.reserve((size_t)nstar * s + (size_t)nstar + (size_t)s * s));
  double* cd = pr.out;
  double* qd = cd + nstar * s;
  double* Gd = qd + nstar;
  // 1. Sol = S^-1 R, G = R^T Sol
  {
    double* X = sp->work.ws;
    double* Rr = X + ns;
    if (rhs) {
      std::vector<double> h((size_t)ns);
      for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < s; ++k) h[(size_t)i * s + k] = rhs[orig_row(sp, i) * ld + k];
      HIP_TRY(hipMemcpyAsync(Rr, h.data(), sizeof(double) * ns, hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));
    } else {
      hipLaunchKernelGGL(rows_gather_kernel, dim3(grid_ns(n, s)), dim3(256), 0, st,
                         (const double*)sp->ms.rhs_dev, s,
                         sp->perm.empty() ? (const int*)nullptr : (const int*)sp->perm_d, n, s, Rr);
      LAUNCH_CHECK("rows_gather_kernel");
    }
    HIP_TRY(hipMemcpyAsync(pr.R, Rr, sizeof(double) * ns, hipMemcpyDeviceToDevice, st));
    int it = 0;
    if (int rc = cg_block_device(sp, eta, s, rtol, maxiter, &it, &converged)) return rc;
    if (iterations) iterations[0] = it, iterations[1] = 0;
    HIP_TRY(hipMemcpyAsync(pr.Sol, X, sizeof(double) * ns, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(gram_partial_kernel, dim3(NBLK), dim3((unsigned)((s * s + 63) / 64 * 64)), 0,
                       st, (const double*)pr.R, (const double*)pr.Sol, n, s, pr.partial);
    LAUNCH_CHECK("gram_partial_kernel");
    hipLaunchKernelGGL(col_dot_reduce_kernel, dim3((s * s + 3) / 4), dim3(256), 0, st,
                       (const double*)pr.partial, NBLK, s, s, Gd);
    LAUNCH_CHECK("col_dot_reduce_kernel");
  }
  // 2. c = K* Sol
  hipLaunchKernelGGL(cross_spmm_kernel, dim3((unsigned)((nstar + 3) / 4)), dim3(256), 0, st,
                     (const int64_t*)pr.indptr, (const int*)pr.indices, (const double*)pr.data,
                     nstar, (const double*)pr.Sol, s, cd);
  LAUNCH_CHECK("cross_spmm_kernel");
  // 3. q, block by block (a block of empty rows keeps its zeros without a CG)
  if (want_q) {
    HIP_TRY(hipMemsetAsync(qd, 0, sizeof(double) * nstar, st));
    int most = 0;
    for (int64_t j0 = 0; j0 < nstar; j0 += sb) {
      const int sw = (int)std::min<int64_t>(sb, nstar - j0);
      if (pr.indptr_h[j0 + sw] == pr.indptr_h[j0]) continue;
      const int64_t nw = n * sw;
      double* X = sp->work.ws;
      double* Rr = X + nw;
      HIP_TRY(hipMemsetAsync(Rr, 0, sizeof(double) * nw, st));
      hipLaunchKernelGGL(cross_scatter_kernel, dim3((sw + 3) / 4), dim3(256), 0, st,
                         (const int64_t*)pr.indptr, (const int*)pr.indices,
                         (const double*)pr.data, j0, sw, Rr);
      LAUNCH_CHECK("cross_scatter_kernel");
      int it = 0;
      if (int rc = cg_block_device(sp, eta, sw, rtol, maxiter, &it, &converged)) return rc;
      most = std::max(most, it);
      hipLaunchKernelGGL(cross_dot_kernel, dim3((sw + 3) / 4), dim3(256), 0, st,
                         (const int64_t*)pr.indptr, (const int*)pr.indices,
                         (const double*)pr.data, j0, sw, (const double*)X, qd);
      LAUNCH_CHECK("cross_dot_kernel");
    }
    if (iterations) iterations[1] = most;
  }
  HIP_TRY(hipMemcpyAsync(c, cd, sizeof(double) * nstar * s, hipMemcpyDeviceToHost, st));
  if (want_q) HIP_TRY(hipMemcpyAsync(q, qd, sizeof(double) * nstar, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(G, Gd, sizeof(double) * s * s, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  sp->last_converged = converged ? 1 : 0;
  return 0;
}

}  // namespace

extern "C" {

int gpmi_sp_cross_matern(gpmi_sp* sp, const double* test_points, int64_t nstar, int d,
                         int64_t* nnz) {
  if (!sp) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  if (int rc = cross_assemble(sp, test_points, nstar, d)) return rc;
  if (nnz) *nnz = sp->pred.nnz;
  return 0;
}

int gpmi_sp_get_cross(gpmi_sp* sp, int64_t* indptr, int* indices, double* data) {
  if (!sp) return set_error(-1006, "null handle");
  SpPredict& pr = sp->pred;
  if (pr.nstar < 1) return set_error(-1110, "no cross matrix has been assembled or given");
  if (!indptr || (pr.nnz > 0 && (!indices || !data))) return set_error(-1006, "null output");
  DeviceGuard g(sp->device);
  const int64_t nstar = pr.nstar, nnz = pr.nnz;
  std::vector<int> ix((size_t)nnz);
  std::vector<double> dv((size_t)nnz);
  if (nnz > 0) {
    HIP_TRY(hipMemcpy(ix.data(), pr.indices, sizeof(int) * nnz, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dv.data(), pr.data, sizeof(double) * nnz, hipMemcpyDeviceToHost));
  }
  // original column indices, ascending per row
  std::vector<std::pair<int, double>> row;
  for (int64_t j = 0; j < nstar; ++j) {
    const int64_t k0 = pr.indptr_h[j], k1 = pr.indptr_h[j + 1];
    indptr[j] = k0;
    row.clear();
    for (int64_t e = k0; e < k1; ++e) row.emplace_back((int)orig_row(sp, ix[e]), dv[e]);
    if (!sp->perm.empty())
      std::sort(row.begin(), row.end(),
                [](const std::pair<int, double>& a, const std::pair<int, double>& b) {
                  return a.first < b.first;
                });
    for (size_t e = 0; e < row.size(); ++e) {
      indices[k0 + (int64_t)e] = row[e].first;
      data[k0 + (int64_t)e] = row[e].second;
    }
  }
  indptr[nstar] = nnz;
  return 0;
}

int gpmi_sp_predict_terms(gpmi_sp* sp, double eta, const double* rhs, int64_t ld, int nrhs,
                          const double* test_points, int64_t nstar, int d, int want_q,
                          double rtol, int maxiter, double* c, double* q, double* G,
                          int* iterations) {
  if (!sp) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  if (int rc = cross_assemble(sp, test_points, nstar, d)) return rc;
  return predict_core(sp, eta, rhs, ld, nrhs, want_q, rtol, maxiter, c, q, G, iterations);
}

int gpmi_sp_predict_terms_csr(gpmi_sp* sp, double eta, const double* rhs, int64_t ld, int nrhs,
                              int64_t nstar, const int64_t* indptr, const int* indices,
                              const double* data, int want_q, double rtol, int maxiter,
                              double* c, double* q, double* G, int* iterations) {
  if (!sp) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  if (int rc = cross_upload(sp, nstar, indptr, indices, data)) return rc;
  return predict_core(sp, eta, rhs, ld, nrhs, want_q, rtol, maxiter, c, q, G, iterations);
}

}  // extern "C"
