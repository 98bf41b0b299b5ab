// The dense operator's second-order terms (include/gpmi.h: gpmi_op_fisher_terms;
// gpmi_op.h: DenseFisher) on the cached factor: the traces tr(M_a M_b) and the small Grams
// U[a], V[a][b] the expected information in (sigma, sigma0, rho) is made of. The lower
// tiles of A^-1 = W W^T are those gpmi_op_traceinv(.., 2) forms and caches
// (traceinv_build_ainv), S = A^-1 [X | z] that of the leave-one-out pass (loo_build_sol,
// left in loo.out); the d products M_k = A^-1 dK / d rho_k, the traces and the thin
// products are gpmi_fisher.hip's. The call reads tinv.W, tinv.Td, loo.out and rhs_src and
// writes only DenseFisher's buffers.

#include <hip/hip_runtime.h>

#include <vector>

#include "gpmi_op.h"

using namespace gpmi;

namespace {

// reserve() with a failure turned into the library's own code: the handle stays usable,
// and HIP's out-of-memory error is cleared.
template <class T>
int reserve_or_code(DevBuf<T>& b, size_t count, const char* what) {
  if (b.reserve(count) == hipSuccess) return 0;
  (void)hipGetLastError();
  return set_errorf(-1032, "gpmi_op_fisher_terms: no device memory for %s (%zu bytes)", what,
                    sizeof(T) * count);
}

}  // namespace

extern "C" {

int gpmi_op_fisher_terms(gpmi_op* op, double eta, const double* points, int d,
                         const double* scale, double nu, double* T_out, double* U_out,
                         double* V_out) {
  if (!op) return set_error(-1006, "null handle");
  if (!op->has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  if (op->nrhs < 1)
    return set_error(-1012, "no resident right-hand sides (gpmi_op_set_rhs)");
  if (d < 1 || d > GPMI_MAX_DIM)
    return set_errorf(-1003, "dimension %d outside [1, %d]", d, GPMI_MAX_DIM);
  if (!points || !scale) return set_error(-1004, "null argument");
  MaternParams MP;
  int rc = matern_params_host(nu, &MP);
  if (rc) return rc;
  if (MP.mode == MATERN_GENERAL)
    return set_errorf(-1031,
                      "the information has no form for a general nu (got %g): nu must be "
                      "0.5, 1.5, 2.5 or >= 100 (the Gaussian limit)", nu);
  const int64_t np = op->n_pad, n = op->n;
  const int nt = op->nt, m = op->nrhs, d1 = d + 1;
  const int ntile = nt * nt, npair = d1 * (d1 + 1) / 2, ngram = d1 + d1 * d1;
  DeviceGuard g(op->device);
  hipStream_t s = op->stream;
  DenseFisher& fi = op->fisher;
  fi.last_product_ms = fi.last_total_ms = 0.0;
  if (op->tim.on) {
    HIP_TRY(op->tim.fisher.reserve(4, timing_event_flags()));
    HIP_TRY(hipEventRecord(op->tim.fisher[0], s));
  }
  bool fresh;
  if ((rc = factor_ready(op, eta, op->rhs_src, &fresh))) return rc;
  if ((rc = traceinv_build_w(op))) return rc;
  if ((rc = traceinv_build_ainv(op))) return rc;
  if ((rc = loo_build_sol(op))) return rc;
  // the call's own buffers after the cached pieces exist (W, the tiles of A^-1, Sol keep
  // their memory either way), the large block first: when one does not fit, none of this
  // call's terms has been computed
  if ((rc = reserve_or_code(fi.M, (size_t)d * np * np, "the products M_k"))) return rc;
  if ((rc = reserve_or_code(fi.YZ, (size_t)2 * d1 * np * RLD, "the thin blocks"))) return rc;
  if ((rc = reserve_or_code(fi.part, (size_t)npair * ntile, "the trace partials"))) return rc;
  if ((rc = reserve_or_code(fi.out, (size_t)npair + (size_t)ngram * RLD * RLD, "the results")))
    return rc;
  if ((rc = reserve_or_code(fi.pts, (size_t)n * d, "the points"))) return rc;
  if ((rc = reserve_or_code(fi.scale, (size_t)GPMI_MAX_DIM, "the scale"))) return rc;
  HIP_TRY(hipMemcpyAsync(fi.pts, points, sizeof(double) * n * d, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(fi.scale, scale, sizeof(double) * d, hipMemcpyHostToDevice, s));
  // (the host blocks are the caller's: on the device before the call goes on)
  HIP_TRY(hipStreamSynchronize(s));
  const double* W = op->tinv.W;
  const double* Td = op->tinv.Td;
  double* Y = fi.YZ;
  double* Z = Y + (size_t)d1 * np * RLD;
  double* tr = fi.out;
  double* gram = tr + npair;
  // M_k = A^-1 N_k
  if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.fisher[1], s));
  launch_fisher_product(s, MP.mode, W, np, Td, fi.pts, n, d, fi.scale, nt, fi.M);
  LAUNCH_CHECK("fisher_product_kernel");
  if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.fisher[2], s));
  // T[a][b], a <= b
  hipLaunchKernelGGL(fisher_trace_kernel, dim3((unsigned)ntile, (unsigned)npair), dim3(256), 0, s,
                     fi.M, np, W, Td, n, d, nt, fi.part);
  LAUNCH_CHECK("fisher_trace_kernel");
  hipLaunchKernelGGL(fisher_trace_reduce_kernel, dim3((unsigned)npair), dim3(256), 0, s, fi.part,
                     ntile, tr);
  LAUNCH_CHECK("fisher_trace_reduce_kernel");
  // Y_0 = S, Y_k = M_k^T R; Z_a = M_a S
  hipLaunchKernelGGL(fisher_copy_sol_kernel, dim3((unsigned)((np * RLD + 255) / 256)), dim3(256),
                     0, s, op->loo.out, np, Y);
  LAUNCH_CHECK("fisher_copy_sol_kernel");
  launch_fisher_thin(s, true, 1, d, fi.M, np, W, Td, n, op->rhs_src, RLD, Y + (size_t)np * RLD);
  LAUNCH_CHECK("fisher_thin_kernel (Y)");
  launch_fisher_thin(s, false, 0, d1, fi.M, np, W, Td, n, op->loo.out, LOO_LD, Z);
  LAUNCH_CHECK("fisher_thin_kernel (Z)");
  hipLaunchKernelGGL(fisher_gram_kernel, dim3((unsigned)ngram), dim3(256), 0, s, fi.YZ, np, d,
                     gram);
  LAUNCH_CHECK("fisher_gram_kernel");
  if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.fisher[3], s));
  std::vector<double> ho((size_t)npair + (size_t)ngram * RLD * RLD);
  HIP_TRY(hipMemcpyAsync(ho.data(), fi.out, sizeof(double) * ho.size(), hipMemcpyDeviceToHost,
                         s));
  HIP_TRY(hipStreamSynchronize(s));
  if (T_out) {
    int y = 0;
    for (int a = 0; a < d1; ++a)
      for (int b = a; b < d1; ++b, ++y) T_out[a * d1 + b] = T_out[b * d1 + a] = ho[y];
  }
  const double* hg = ho.data() + npair;
  for (int gi = 0; gi < ngram; ++gi) {
    double* dst = gi < d1 ? U_out : V_out;
    if (!dst) continue;
    dst += (size_t)(gi < d1 ? gi : gi - d1) * m * m;
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b) dst[a * m + b] = hg[((size_t)gi * RLD + a) * RLD + b];
  }
  if (op->tim.on) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, op->tim.fisher[1], op->tim.fisher[2]));
    fi.last_product_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, op->tim.fisher[0], op->tim.fisher[3]));
    fi.last_total_ms = ms;
  }
  return 0;
}

int gpmi_op_fisher_ms(gpmi_op* op, double* product_ms, double* total_ms) {
  if (!op) return set_error(-1006, "null handle");
  if (product_ms) *product_ms = op->fisher.last_product_ms;
  if (total_ms) *total_ms = op->fisher.last_total_ms;
  return 0;
}

}  // extern "C"
