// The dense operator's leave-one-out terms (include/gpmi.h: gpmi_op_loo_terms; gpmi_op.h:
// DenseLoo) on the cached factor: W = L^-T is the one gpmi_op_traceinv builds and caches
// (traceinv_build_w), Y = L^-1 [X | z] and G = Y^T Y those of the prediction
// (predict_refresh_y), and one chunked pass over W (kernels: gpmi_loo.hip) gives
// diag(S^-1) and S^-1 [X | z]. The pass reads pred.PY and writes only DenseLoo's buffers.
// The pass and its reduce are loo_build_sol, which the scale gradient
// (gpmi_dense_scale_grad.hip) calls too for S^-1 [X | z].

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "gpmi_op.h"

using namespace gpmi;

namespace {

// GPMI_LOO_CHUNK (read per call): the chunk width in columns, or -1.
int64_t loo_chunk_cols() {
  int64_t cw = LOO_CHUNK;
  if (const char* e = std::getenv("GPMI_LOO_CHUNK"))
    if (*e) cw = std::atoll(e);
  return (cw < TS || cw % TS || cw > (1 << 20)) ? -1 : cw;
}

}  // namespace

int gpmi::loo_build_sol(gpmi_op* op) {
  const int64_t np = op->n_pad;
  const int64_t cw = loo_chunk_cols();
  if (cw < 0) return set_error(-1021, "GPMI_LOO_CHUNK must be a positive multiple of 128");
  const int nchunk = (int)((np + cw - 1) / cw);
  hipStream_t s = op->stream;
  int rc;
  if ((rc = predict_refresh_y(op))) return rc;
  DenseLoo& lo = op->loo;
  HIP_TRY(lo.part.reserve((size_t)nchunk * np * LOO_LD));
  HIP_TRY(lo.out.reserve((size_t)np * LOO_LD));
  if (op->tim.on) {
    HIP_TRY(op->tim.loo.reserve(2, timing_event_flags()));
    HIP_TRY(hipEventRecord(op->tim.loo[0], s));
  }
  hipLaunchKernelGGL(loo_pass_kernel, dim3(nchunk, (unsigned)(np / LOO_ROWS)), dim3(256), 0, s,
                     op->tinv.W, np, op->pred.PY, np, (int)cw, lo.part);
  LAUNCH_CHECK("loo_pass_kernel");
  if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.loo[1], s));
  const int64_t cnt = np * LOO_LD;
  hipLaunchKernelGGL(loo_reduce_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s,
                     lo.part, np, (int)cw, nchunk, lo.out);
  LAUNCH_CHECK("loo_reduce_kernel");
  return 0;
}

extern "C" {

int gpmi_op_loo_terms(gpmi_op* op, double eta, double* dinv_out, double* sol_out,
                      int64_t ldsol, double* gram_out) {
  if (!op) return set_error(-1006, "null handle");
  if (!op->has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  if (op->nrhs < 1) return set_error(-1012, "no resident right-hand sides (gpmi_op_set_rhs)");
  if (sol_out && ldsol < op->nrhs)
    return set_errorf(-1020, "ldsol %lld below nrhs = %d", (long long)ldsol, op->nrhs);
  if (loo_chunk_cols() < 0)
    return set_error(-1021, "GPMI_LOO_CHUNK must be a positive multiple of 128");
  const int64_t n = op->n;
  DeviceGuard g(op->device);
  hipStream_t s = op->stream;
  bool fresh;
  int rc = factor_ready(op, eta, op->rhs_src, &fresh);
  if (rc) return rc;
  if ((rc = traceinv_build_w(op))) return rc;
  if ((rc = loo_build_sol(op))) return rc;
  DenseLoo& lo = op->loo;
  std::vector<double> h((size_t)n * LOO_LD);
  double hg[256];
  HIP_TRY(hipMemcpyAsync(h.data(), lo.out, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hg, op->pred.Pgram, sizeof(hg), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int m = op->nrhs;
  for (int64_t i = 0; i < n; ++i) {
    if (dinv_out) dinv_out[i] = h[(size_t)i * LOO_LD + 16];
    if (sol_out)
      for (int a = 0; a < m; ++a) sol_out[i * ldsol + a] = h[(size_t)i * LOO_LD + a];
  }
  if (gram_out)
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b) gram_out[a * m + b] = hg[a * RLD + b];
  lo.last_ms = lo.last_bytes = 0.0;
  if (op->tim.on) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, op->tim.loo[0], op->tim.loo[1]));
    lo.last_ms = ms;
    // the upper block triangle, diagonal tiles whole
    lo.last_bytes = 8.0 * TS * TS * (double)op->nt * (op->nt + 1) / 2.0;
  }
  return 0;
}

int gpmi_op_loo_ms(gpmi_op* op, double* pass_ms, double* pass_bytes) {
  if (!op) return set_error(-1006, "null handle");
  if (pass_ms) *pass_ms = op->loo.last_ms;
  if (pass_bytes) *pass_bytes = op->loo.last_bytes;
  return 0;
}

}  // extern "C"
