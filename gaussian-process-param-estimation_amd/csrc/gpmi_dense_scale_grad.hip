// The dense operator's correlation-scale gradient terms (include/gpmi.h:
// gpmi_op_scale_grad_terms; gpmi_op.h: DenseScaleGrad) on the cached factor. The lower
// tiles of A^-1 = W W^T are those gpmi_op_traceinv(.., 2) forms and caches
// (traceinv_build_ainv), Sol = A^-1 [X | z] that of the leave-one-out pass
// (loo_build_sol, left in loo.out), and one pass over the tiles (kernels:
// gpmi_scale_grad.hip) contracts both with dK / d rho_k formed from the points. The pass
// reads tinv.W, tinv.Td and loo.out and writes only DenseScaleGrad's buffers.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "gpmi_op.h"

using namespace gpmi;

extern "C" {

int gpmi_op_scale_grad_terms(gpmi_op* op, double eta, const double* points, int d,
                             const double* scale, double nu, const double* coef, int ncoef,
                             double* tr_out, double* quad_out) {
  if (!op) return set_error(-1006, "null handle");
  if (!op->has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  if (ncoef < 0 || ncoef > SG_MAX_COEF)
    return set_errorf(-1030, "ncoef %d outside [0, %d]", ncoef, SG_MAX_COEF);
  if (ncoef > 0 && op->nrhs < 1)
    return set_error(-1012, "no resident right-hand sides (gpmi_op_set_rhs)");
  if (d < 1 || d > GPMI_MAX_DIM)
    return set_errorf(-1003, "dimension %d outside [1, %d]", d, GPMI_MAX_DIM);
  if (!points || !scale || (ncoef > 0 && !coef)) return set_error(-1004, "null argument");
  MaternParams MP;
  int rc = matern_params_host(nu, &MP);
  if (rc) return rc;
  if (MP.mode == MATERN_GENERAL)
    return set_errorf(-1031,
                      "the scale gradient has no form for a general nu (got %g): nu must be "
                      "0.5, 1.5, 2.5 or >= 100 (the Gaussian limit)", nu);
  const int64_t np = op->n_pad, n = op->n;
  const int nt = op->nt, m = op->nrhs;
  const int ntile = nt * (nt + 1) / 2;
  const int nc = ncoef == 0 ? 0 : (ncoef <= 2 ? 2 : 4);   // the kernel's instantiations
  const int nval = (1 + ncoef) * GPMI_MAX_DIM;
  DeviceGuard g(op->device);
  hipStream_t s = op->stream;
  bool fresh;
  if ((rc = factor_ready(op, eta, op->rhs_src, &fresh))) return rc;
  if ((rc = traceinv_build_w(op))) return rc;
  if ((rc = traceinv_build_ainv(op))) return rc;
  if (ncoef > 0 && (rc = loo_build_sol(op))) return rc;
  DenseScaleGrad& sg = op->sgrad;
  HIP_TRY(sg.pts.reserve((size_t)n * d));
  HIP_TRY(sg.scale.reserve(GPMI_MAX_DIM));
  HIP_TRY(sg.coef.reserve((size_t)SG_MAX_COEF * RLD * RLD));
  HIP_TRY(sg.part.reserve((size_t)ntile * (1 + SG_MAX_COEF) * GPMI_MAX_DIM));
  HIP_TRY(sg.out.reserve((size_t)(1 + SG_MAX_COEF) * GPMI_MAX_DIM));
  // coef [ncoef][nrhs][nrhs] -> [nc][16][16], zero beyond
  std::vector<double> hc((size_t)SG_MAX_COEF * RLD * RLD, 0.0);
  for (int c = 0; c < ncoef; ++c)
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b)
        hc[((size_t)c * RLD + a) * RLD + b] = coef[((size_t)c * m + a) * m + b];
  HIP_TRY(hipMemcpyAsync(sg.pts, points, sizeof(double) * n * d, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(sg.scale, scale, sizeof(double) * d, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(sg.coef, hc.data(), sizeof(double) * hc.size(), hipMemcpyHostToDevice,
                         s));
  // (the host blocks are this call's locals: on the device before it goes on)
  HIP_TRY(hipStreamSynchronize(s));
  if (op->tim.on) {
    HIP_TRY(op->tim.sgrad.reserve(2, timing_event_flags()));
    HIP_TRY(hipEventRecord(op->tim.sgrad[0], s));
  }
  launch_scale_grad_pass(s, MP.mode, nc, op->tinv.W, np, op->tinv.Td, op->loo.out, sg.coef,
                         ncoef, sg.pts, n, d, sg.scale, nt, sg.part);
  LAUNCH_CHECK("scale_grad_pass_kernel");
  if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.sgrad[1], s));
  hipLaunchKernelGGL(scale_grad_reduce_kernel, dim3(1), dim3(64), 0, s, sg.part, ntile, nval, d,
                     sg.scale, sg.out);
  LAUNCH_CHECK("scale_grad_reduce_kernel");
  double ho[(1 + SG_MAX_COEF) * GPMI_MAX_DIM];
  HIP_TRY(hipMemcpyAsync(ho, sg.out, sizeof(double) * nval, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < d; ++k) {
    if (tr_out) tr_out[k] = ho[k];
    if (quad_out)
      for (int c = 0; c < ncoef; ++c) quad_out[c * d + k] = ho[(1 + c) * GPMI_MAX_DIM + k];
  }
  sg.last_ms = sg.last_bytes = 0.0;
  if (op->tim.on) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, op->tim.sgrad[0], op->tim.sgrad[1]));
    sg.last_ms = ms;
    sg.last_bytes = 8.0 * TS * TS * (double)ntile;   // the lower tiles of A^-1
  }
  return 0;
}

int gpmi_op_scale_grad_ms(gpmi_op* op, double* pass_ms, double* pass_bytes) {
  if (!op) return set_error(-1006, "null handle");
  if (pass_ms) *pass_ms = op->sgrad.last_ms;
  if (pass_bytes) *pass_bytes = op->sgrad.last_bytes;
  return 0;
}

}  // extern "C"
