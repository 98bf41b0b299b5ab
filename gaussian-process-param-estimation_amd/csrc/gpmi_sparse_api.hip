// C-ABI of the sparse path (include/gpmi.h, gpmi_sp_*), the handle's own part: create
// from a host CSR or over a dense operator, destroy, info, the CSR read-back and its
// dense scatter, the resident RHS block and the last status. The handle: gpmi_sp.h.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "gpmi_sp.h"
#include "gpmi_band.h"

using namespace gpmi;

namespace gpmi {
int op_view(const gpmi_op* op, OpView* v);   // gpmi_api.hip
}  // namespace gpmi

extern "C" {

int gpmi_sp_create_csr(int device, int64_t n, const int64_t* indptr, const int* indices,
                       const double* data, gpmi_sp** out) {
  if (!out || n <= 0) return set_error(-1100, "invalid arguments");
  DeviceGuard g(device);
  SpPtr sp(new gpmi_sp());
  sp->device = device;
  sp->n = n;
  sp->nnz = indptr[n];
  HIP_TRY(hipStreamCreateWithFlags(&sp->stream.h, hipStreamNonBlocking));
  HIP_TRY(sp->indptr.reserve(n + 1));
  HIP_TRY(sp->indices.reserve(std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(sp->data.reserve(std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(sp->work.small.reserve(16384));
  HIP_TRY(hipMemcpy(sp->indptr, indptr, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(sp->indices, indices, sizeof(int) * sp->nnz, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(sp->data, data, sizeof(double) * sp->nnz, hipMemcpyHostToDevice));
  *out = sp.release();
  return 0;
}

int gpmi_sp_create_dense(gpmi_op* op, gpmi_sp** out) {
  if (!out) return set_error(-1004, "null output handle");
  OpView v;
  int rc = op_view(op, &v);
  if (rc) return rc;
  if (!v.has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  DeviceGuard g(v.device);
  SpPtr sp(new gpmi_sp());
  sp->device = v.device;
  sp->n = v.n;
  sp->nnz = v.n * v.n;
  sp->dense.K = v.K;
  sp->dense.ld = v.n_pad;
  // k splits: about 1024 workgroups (row blocks x splits) keep the HBM stream busy
  const int64_t nch = (v.n + 63) / 64;
  int split = (int)std::min<int64_t>(16, std::max<int64_t>(1, (1024 + nch - 1) / nch));
  split = (int)std::min<int64_t>(split, nch);
  sp->dense.kcs = (int)((nch + split - 1) / split);
  sp->dense.split = (int)((nch + sp->dense.kcs - 1) / sp->dense.kcs);
  const size_t part = (size_t)sp->dense.split * (size_t)sp->n * MAXS;
  const char* what = "stream";
  hipError_t e = hipStreamCreateWithFlags(&sp->stream.h, hipStreamNonBlocking);
  if (e == hipSuccess) what = "small", e = sp->work.small.reserve(16384);
  if (e == hipSuccess) what = "dense partials", e = sp->dense.Yp.reserve(part);
  if (e == hipSuccess) e = sp->dense.Yp_ms.reserve(part);
  if (e != hipSuccess)
    return set_errorf(-(int)e, "%s failed: %s", what, hipGetErrorString(e));
  *out = sp.release();
  return 0;
}

int gpmi_sp_destroy(gpmi_sp* sp) {
  if (!sp) return 0;
  DeviceGuard g(sp->device);
  if (sp->stream) (void)hipStreamSynchronize(sp->stream);
  if (sp->ms.stream) (void)hipStreamSynchronize(sp->ms.stream);
  delete sp;
  return 0;
}

int gpmi_sp_info(const gpmi_sp* sp, int64_t* n, int64_t* nnz) {
  if (!sp) return set_error(-1006, "null handle");
  if (n) *n = sp->n;
  if (nnz) *nnz = sp->nnz;
  return 0;
}

int gpmi_sp_get_csr(gpmi_sp* sp, int64_t* indptr, int* indices, double* data) {
  if (!sp) return set_error(-1006, "null handle");
  if (sp->dense.K) return set_error(-1105, "a dense operator has no CSR");
  DeviceGuard g(sp->device);
  if (sp->perm.empty()) {
    HIP_TRY(hipMemcpy(indptr, sp->indptr, sizeof(int64_t) * (sp->n + 1), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(indices, sp->indices, sizeof(int) * sp->nnz, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(data, sp->data, sizeof(double) * sp->nnz, hipMemcpyDeviceToHost));
    return 0;
  }
  // the original order: row i = device row inv[i], columns renamed back and sorted
  const int64_t n = sp->n;
  std::vector<int64_t> ip(n + 1);
  std::vector<int> ix(sp->nnz);
  std::vector<double> dv(sp->nnz);
  HIP_TRY(hipMemcpy(ip.data(), sp->indptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ix.data(), sp->indices, sizeof(int) * sp->nnz, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(dv.data(), sp->data, sizeof(double) * sp->nnz, hipMemcpyDeviceToHost));
  std::vector<int> inv(n);
  for (int64_t r = 0; r < n; ++r) inv[sp->perm[r]] = (int)r;
  indptr[0] = 0;
  std::vector<std::pair<int, double>> row;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = inv[i];
    row.clear();
    for (int64_t q = ip[r]; q < ip[r + 1]; ++q) row.emplace_back(sp->perm[ix[q]], dv[q]);
    std::sort(row.begin(), row.end(),
              [](const std::pair<int, double>& a, const std::pair<int, double>& b) {
                return a.first < b.first;
              });
    const int64_t o = indptr[i];
    for (size_t q = 0; q < row.size(); ++q) {
      indices[o + q] = row[q].first;
      data[o + q] = row[q].second;
    }
    indptr[i + 1] = o + (int64_t)row.size();
  }
  return 0;
}

}  // extern "C"

namespace gpmi {

// K[perm[r]][perm[c]] = a_rc: one wavefront per device row (the dense copy is in
// the original point order).
__global__ void __launch_bounds__(256) csr_scatter_dense_kernel(
    const int64_t* __restrict__ indptr, const int* __restrict__ indices,
    const double* __restrict__ data, const int* __restrict__ perm, int64_t n,
    double* __restrict__ K, int64_t ldk) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int lane = threadIdx.x & 63;
  const int64_t i = perm ? perm[r] : r;
  double* Ki = K + i * ldk;
  for (int64_t q = indptr[r] + lane; q < indptr[r + 1]; q += 64) {
    const int c = indices[q];
    Ki[perm ? perm[c] : c] = data[q];
  }
}

// Scatter the operator's CSR into a zeroed dense [n][ldk] device matrix on the
// device `device` (stream st); the dense operator's exact methods on a sparse K.
int sp_scatter_dense(const gpmi_sp* sp, int device, double* K, int64_t ldk, hipStream_t st) {
  if (sp->device != device)
    return set_error(-1011, "sparse and dense operators live on different devices");
  if (sp->dense.K) return set_error(-1105, "a dense operator has no CSR");
  HIP_TRY(hipStreamSynchronize(sp->stream));
  const unsigned grid = (unsigned)((sp->n + 3) / 4);
  hipLaunchKernelGGL(csr_scatter_dense_kernel, dim3(grid), dim3(256), 0, st, sp->indptr,
                     sp->indices, sp->data, sp->perm.empty() ? nullptr : (int*)sp->perm_d, sp->n, K,
                     ldk);
  LAUNCH_CHECK("csr_scatter_dense_kernel");
  return 0;
}

}  // namespace gpmi

extern "C" {

int gpmi_sp_set_rhs(gpmi_sp* sp, const double* rhs, int64_t ld, int nrhs) {
  if (!sp) return set_error(-1006, "null handle");
  if (!rhs || nrhs < 1 || nrhs > MS_MAXS || ld < nrhs)
    return set_error(-1104, "set_rhs: need 1 <= nrhs <= 16 and ld >= nrhs");
  DeviceGuard g(sp->device);
  const int64_t n = sp->n;
  // (exactly [n][nrhs]: another width allocates afresh)
  if (sp->ms.rhs_dev && sp->ms.rhs_nrhs != nrhs) HIP_TRY(sp->ms.rhs_dev.release());
  if (!sp->ms.rhs_dev) HIP_TRY(sp->ms.rhs_dev.reserve((size_t)n * nrhs));
  sp->ms.rhs_nrhs = nrhs;
  if (ld == nrhs) {
    HIP_TRY(hipMemcpy(sp->ms.rhs_dev, rhs, sizeof(double) * (size_t)n * nrhs,
                      hipMemcpyHostToDevice));
  } else {
    std::vector<double> h((size_t)n * nrhs);
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < nrhs; ++c) h[(size_t)i * nrhs + c] = rhs[i * ld + c];
    HIP_TRY(hipMemcpy(sp->ms.rhs_dev, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  }
  return 0;
}

int gpmi_sp_last_status(const gpmi_sp* sp, int* converged) {
  if (!sp) return set_error(-1006, "null handle");
  if (converged) *converged = sp->last_converged;
  return 0;
}

}  // extern "C"
