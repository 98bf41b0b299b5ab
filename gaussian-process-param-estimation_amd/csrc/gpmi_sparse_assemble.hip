// gpmi_sp_create_matern: the tapered Matérn CSR assembled on the device (kernels:
// gpmi_matern.hip), as cutoff search, cell plan (gpmi_cell_plan.h), count, fill and the
// locality permutation.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "gpmi_sp.h"
#include "gpmi_cell_plan.h"

using namespace gpmi;

namespace gpmi {
int matern_params_host(double nu, MaternParams* P);   // gpmi_api.hip
}  // namespace gpmi

namespace {

// Scaled-distance cutoff: smallest grid x with matern(x) <= tau, with margin.
// matern is decreasing, so every pair beyond xcut has matern < tau.
int taper_cutoff(gpmi_sp* sp, const MaternParams& P, double tau, double* xcut_out) {
  hipStream_t st = sp->stream;
  const int M = 4096;
  double xmax = 1.0, xcut = 0.0;
  std::vector<double> hx(M), hv(M);
  double* dx = sp->work.small;
  double* dv = sp->work.small + M;
  for (int it = 0; it < 60; ++it) {
    for (int i = 0; i < M; ++i) hx[i] = xmax * (i + 1) / M;
    HIP_TRY(hipMemcpyAsync(dx, hx.data(), sizeof(double) * M, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(matern_eval_kernel, dim3(M / 256), dim3(256), 0, st, dx, (int64_t)M, P, dv);
    LAUNCH_CHECK("matern_eval_kernel");
    HIP_TRY(hipMemcpyAsync(hv.data(), dv, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int first = -1;
    for (int i = 0; i < M; ++i)
      if (hv[i] <= tau) {
        first = i;
        break;
      }
    if (first >= 0) {
      xcut = hx[first] * (1.0 + 1e-6) + xmax / M;
      break;
    }
    xmax *= 2.0;
  }
  if (xcut == 0.0) return set_error(-1101, "taper threshold not reached (tau too small)");
  *xcut_out = xcut;
  return 0;
}

// rows (and columns) renumbered in the locality order: K' = P K P^T
int permute_csr(gpmi_sp* sp, std::vector<int>& lorder, const std::vector<int>& cnt) {
  const int64_t n = sp->n;
  hipStream_t st = sp->stream;
  std::vector<int> inv(n);
  for (int64_t r = 0; r < n; ++r) inv[lorder[r]] = (int)r;
  std::vector<int64_t> ip2(n + 1, 0);
  for (int64_t r = 0; r < n; ++r) ip2[r + 1] = ip2[r] + cnt[lorder[r]];
  // (freed in reverse order: the old row starts, columns and values; the inverse stays
  // with the handle for the cross assembly's device columns)
  DevBuf<int>& dpi = sp->geom.inv;
  DevBuf<double> ddv2;
  DevBuf<int> dix2;
  DevBuf<int64_t> dip2;
  HIP_TRY(sp->perm_d.reserve(n));
  HIP_TRY(dpi.reserve(n));
  HIP_TRY(dip2.reserve(n + 1));
  HIP_TRY(dix2.reserve(std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(ddv2.reserve(std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(hipMemcpyAsync(sp->perm_d, lorder.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dpi, inv.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dip2, ip2.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(csr_permute_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st,
                     sp->indptr, sp->indices, sp->data, sp->perm_d, dpi, n, dip2, dix2, ddv2);
  LAUNCH_CHECK("csr_permute_kernel");
  HIP_TRY(hipStreamSynchronize(st));
  sp->indptr = std::move(dip2);   // (the old CSR leaves with the locals)
  sp->indices = std::move(dix2);
  sp->data = std::move(ddv2);
  sp->perm = std::move(lorder);
  return 0;
}

}  // namespace

extern "C" int gpmi_sp_create_matern(int device, const double* points, int64_t n, int d,
                                     const double* scale, double nu, double tau, gpmi_sp** out) {
  if (!out || n <= 0) return set_error(-1100, "invalid arguments");
  if (d < 1 || d > GPMI_MAX_DIM) return set_error(-1003, "dimension outside [1, 8]");
  MaternParams P;
  int rc = matern_params_host(nu, &P);
  if (rc) return rc;
  DeviceGuard g(device);
  SpPtr sp(new gpmi_sp());
  sp->device = device;
  sp->n = n;
  sp->tau = tau;
  HIP_TRY(hipStreamCreateWithFlags(&sp->stream.h, hipStreamNonBlocking));
  HIP_TRY(sp->work.small.reserve(16384));
  hipStream_t st = sp->stream;
  double xcut = 0.0;
  if ((rc = taper_cutoff(sp.get(), P, tau, &xcut))) return rc;
  DevBuf<int> dcnt;
  // the points and [scale | 1 / scale] stay with the handle (SpGeom: a later cross
  // assembly reads them), and with a plan its cell starts and cell order
  SpGeom& geo = sp->geom;
  DevBuf<double>&ds = geo.scale, &dp = geo.points;
  DevBuf<int> dcell;   // [n] cell of each point, then gdim [d]
  HIP_TRY(dp.reserve(n * d));
  HIP_TRY(ds.reserve(2 * GPMI_MAX_DIM));   // [scale | 1 / scale]
  HIP_TRY(dcnt.reserve(n));
  HIP_TRY(hipMemcpyAsync(dp, points, sizeof(double) * n * d, hipMemcpyHostToDevice, st));
  std::vector<double> hsc(2 * GPMI_MAX_DIM, 1.0);
  for (int k = 0; k < d; ++k) {
    hsc[k] = scale[k];
    hsc[GPMI_MAX_DIM + k] = 1.0 / scale[k];
  }
  HIP_TRY(hipMemcpyAsync(ds, hsc.data(), sizeof(double) * hsc.size(), hipMemcpyHostToDevice, st));
  const unsigned grid = (unsigned)((n + 3) / 4);
  // Cell list (d <= 3). GPMI_SPARSE_BRUTE=1 forces the all-pairs kernels (A/B and tests);
  // GPMI_SPARSE_REORDER=0 keeps the rows in the original order.
  const char* brute_env = std::getenv("GPMI_SPARSE_BRUTE");
  bool cells = d <= 3 && n < (int64_t)1 << 28 && !(brute_env && std::atoi(brute_env) != 0);
  int *dgdim = nullptr, *dstart = nullptr, *dperm = nullptr;
  CellPlan plan;       // (lorder: locality order of the rows, Morton order of the cells)
  if (cells) {
    const char* ro = std::getenv("GPMI_SPARSE_REORDER");
    cells = cell_plan(points, n, d, scale, xcut, !(ro && std::atoi(ro) == 0), &plan);
  }
  const bool planned = cells;
  if (cells) {
    const int64_t total = plan.total;
    HIP_TRY(dcell.reserve(n + d));
    HIP_TRY(geo.cell_start.reserve(total + 1));
    HIP_TRY(geo.cell_perm.reserve(n));
    dgdim = dcell + n;
    dstart = geo.cell_start;
    dperm = geo.cell_perm;
    HIP_TRY(hipMemcpyAsync(dcell, plan.cell.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dgdim, plan.gdim.data(), sizeof(int) * d, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dstart, plan.start.data(), sizeof(int) * (total + 1),
                          hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dperm, plan.perm.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    hipLaunchKernelGGL(csr_cell_count_kernel, dim3(grid), dim3(256), 0, st, dp, n, d, ds, P, tau,
                       xcut, dcell, dgdim, dstart, dperm, dcnt);
    LAUNCH_CHECK("csr_cell_count_kernel");
  } else {
    hipLaunchKernelGGL(csr_count_kernel, dim3(grid), dim3(256), 0, st, dp, n, d, ds, P, tau, xcut,
                       dcnt);
    LAUNCH_CHECK("csr_count_kernel");
  }
  std::vector<int> cnt(n);
  HIP_TRY(hipMemcpyAsync(cnt.data(), dcnt, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (cells && *std::max_element(cnt.begin(), cnt.end()) > CELL_CAP_HOST) cells = false;
  std::vector<int64_t> ip(n + 1, 0);
  for (int64_t i = 0; i < n; ++i) ip[i + 1] = ip[i] + cnt[i];
  sp->nnz = ip[n];
  HIP_TRY(sp->indptr.reserve(n + 1));
  HIP_TRY(sp->indices.reserve(std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(sp->data.reserve(std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(hipMemcpyAsync(sp->indptr, ip.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice,
                        st));
  if (cells) {
    hipLaunchKernelGGL(csr_cell_fill_kernel, dim3(grid), dim3(256), 0, st, dp, n, d, ds, P, tau,
                       xcut, dcell, dgdim, dstart, dperm, sp->indptr, sp->indices, sp->data);
    LAUNCH_CHECK("csr_cell_fill_kernel");
  } else {   // all pairs (d > 3, or a row holds more than CELL_CAP kept entries)
    hipLaunchKernelGGL(csr_fill_kernel, dim3(grid), dim3(256), 0, st, dp, n, d, ds, P, tau, xcut,
                       sp->indptr, sp->indices, sp->data);
    LAUNCH_CHECK("csr_fill_kernel");
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (cells && (int64_t)plan.lorder.size() == n)
    if ((rc = permute_csr(sp.get(), plan.lorder, cnt))) return rc;
  geo.d = d;
  geo.P = P;
  geo.tau = tau;
  geo.xcut = xcut;
  geo.cells = planned;
  if (planned) {
    for (int k = 0; k < 3; ++k) {
      geo.grid.pmin[k] = k < d ? plan.pmin[k] : 0.0;
      geo.grid.wid[k] = k < d ? plan.wid[k] : 1.0;
      geo.grid.gdim[k] = k < d ? plan.gdim[k] : 1;
    }
  } else {
    (void)geo.cell_start.release();
    (void)geo.cell_perm.release();
  }
  geo.has = true;
  *out = sp.release();
  return 0;
}
