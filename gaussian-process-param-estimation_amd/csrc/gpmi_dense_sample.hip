// The dense operator's draws z = L xi from the cached factor of K + eta I = L L^T, and the
// hand-over of the prediction's joint covariance to a second operator (include/gpmi.h:
// gpmi_op_sample, gpmi_op_load_predict_cov; gpmi_op.h: DenseSample): chunking, work list
// and workspace sizes are gpmi_sample_plan.h, the kernels gpmi_sample.hip.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "gpmi_op.h"
#include "gpmi_sample_plan.h"

using namespace gpmi;

namespace {

// An integer knob read per call (0: unset or empty).
int64_t env_knob(const char* name) {
  const char* e = std::getenv(name);
  if (!e || !*e) return 0;
  const int64_t v = std::atoll(e);
  return v > 0 ? v : -1;
}

// The pieces of (nt, D), deepest first, on the device (kept until the shape changes).
int sample_ensure_order(gpmi_op* op, int D) {
  DenseSample& sm = op->samp;
  if (sm.order && sm.order_nt == op->nt && sm.order_depth == D) return 0;
  sm.order_nt = sm.order_depth = -1;
  const std::vector<uint32_t> h = sample_order(op->nt, D);
  HIP_TRY(sm.order.reserve(h.size()));
  HIP_TRY(hipMemcpyAsync(sm.order, h.data(), sizeof(uint32_t) * h.size(), hipMemcpyHostToDevice,
                         op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));   // (h goes out of scope)
  sm.order_nt = op->nt;
  sm.order_depth = D;
  return 0;
}

}  // namespace

extern "C" {

int gpmi_op_load_predict_cov(gpmi_op* dst, gpmi_op* src, const double* U, int64_t ldu, int m) {
  if (!dst || !src) return set_error(-1006, "null handle");
  if (dst->device != src->device)
    return set_errorf(-1022, "operators on different devices (%d and %d)", dst->device,
                      src->device);
  if (src->pred.cov_nstar < 1)
    return set_error(-1023, "the source holds no resident covariance "
                            "(gpmi_op_predict_cov or gpmi_op_predict_cov_resident first)");
  if (dst->n != src->pred.cov_nstar)
    return set_errorf(-1005, "resident covariance is of %lld points, the operator of %lld",
                      (long long)src->pred.cov_nstar, (long long)dst->n);
  if (m < 0 || m > RLD - 1) return set_errorf(-1024, "m %d outside [0, %d]", m, RLD - 1);
  if (m > 0 && !U) return set_error(-1004, "null argument");
  if (m > 0 && ldu < m) return set_errorf(-1025, "ldu %lld below m = %d", (long long)ldu, m);
  DeviceGuard g(dst->device);
  hipStream_t s = dst->stream;
  const int64_t np = dst->n_pad, n = dst->n;
  DenseSample& sm = dst->samp;
  if (m > 0) {
    HIP_TRY(sm.U.reserve((size_t)n * m));
    HIP_TRY(hipMemcpy2DAsync(sm.U, sizeof(double) * m, U, sizeof(double) * ldu,
                             sizeof(double) * m, n, hipMemcpyHostToDevice, s));
  }
  // after the source's work on its own stream
  if (!sm.ev_src) HIP_TRY(hipEventCreateWithFlags(&sm.ev_src.h, sync_event_flags()));
  HIP_TRY(hipEventRecord(sm.ev_src, src->stream));
  HIP_TRY(hipStreamWaitEvent(s, sm.ev_src, 0));
  hipLaunchKernelGGL(cov_lowrank_kernel, dim3((unsigned)(np * np / 256)), dim3(256), 0, s,
                     (const double*)src->pred.Pcov, np, (double*)dst->K, np, n,
                     (const double*)sm.U, m);
  LAUNCH_CHECK("cov_lowrank_kernel");
  HIP_TRY(hipStreamSynchronize(s));
  dst->has_K = true;
  dst->fac.drop();
  return 0;
}

int gpmi_op_sample(gpmi_op* op, double eta, const double* xi, int64_t ldxi,
                   unsigned long long seed, unsigned long long first, int64_t nsamp,
                   double* out, int64_t ldout) {
  if (!op) return set_error(-1006, "null handle");
  if (!op->has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  if (!out) return set_error(-1004, "null argument");
  if (nsamp < 1) return set_errorf(-1026, "nsamp must be positive (got %lld)", (long long)nsamp);
  if (ldout < op->n)
    return set_errorf(-1027, "ldout %lld below n = %lld", (long long)ldout, (long long)op->n);
  if (xi && ldxi < nsamp)
    return set_errorf(-1028, "ldxi %lld below nsamp = %lld", (long long)ldxi, (long long)nsamp);
  if (op->nt > SAMPLE_MAX_NT) return set_error(-1005, "matrix too large for gpmi_op_sample");
  const int cw = sample_chunk_draws(env_knob("GPMI_SAMPLE_CHUNK"));   // draws per chunk
  if (cw < 0) return set_error(-1029, "GPMI_SAMPLE_CHUNK must be a positive multiple of 128");
  const int64_t dknob = env_knob("GPMI_SAMPLE_DEPTH");   // the piece depth in tile rows
  DeviceGuard g(op->device);
  hipStream_t s = op->stream;
  bool fresh;
  int rc = factor_ready(op, eta, op->rhs_src, &fresh);
  if (rc) return rc;
  if (!op->pred.ncu)
    HIP_TRY(hipDeviceGetAttribute(&op->pred.ncu, hipDeviceAttributeMultiprocessorCount,
                                  op->device));
  DenseSample& sm = op->samp;
  const int64_t np = op->n_pad, n = op->n;
  const int nt = op->nt;
  sm.last_normal_ms = sm.last_trmm_ms = sm.last_trmm_flops = 0.0;
  size_t evi = 0;
  std::vector<double> hx;   // a chunk of the host normals, transposed
  for (int64_t j0 = 0; j0 < nsamp; j0 += cw) {
    const int64_t cs = std::min<int64_t>(cw, nsamp - j0);
    const int jt = (int)((cs + TS - 1) / TS);
    const int64_t rows = (int64_t)jt * TS;
    const int D = sample_depth(nt, jt, op->pred.ncu, dknob);
    const int split = D < nt ? 1 : 0;
    const int64_t items = sample_items(nt, D);
    if (items * jt > 0x7fffffff) return set_error(-1005, "too many workgroups in gpmi_op_sample");
    if ((rc = sample_ensure_order(op, D))) return rc;
    const SampleSizes sz = sample_sizes(np, nt, jt, D);
    HIP_TRY(sm.Xi.reserve(sz.xi));
    HIP_TRY(sm.Y.reserve(sz.y));
    HIP_TRY(sm.part.reserve(sz.part));
    if (op->tim.on) HIP_TRY(op->tim.samp.reserve(evi + 4, timing_event_flags()));
    if (xi) {
      hx.resize((size_t)cs * n);
      for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < cs; ++j) hx[(size_t)j * n + i] = xi[i * ldxi + j0 + j];
      HIP_TRY(hipMemsetAsync(sm.Xi, 0, sizeof(double) * rows * np, s));
      HIP_TRY(hipMemcpy2DAsync(sm.Xi, sizeof(double) * np, hx.data(), sizeof(double) * n,
                               sizeof(double) * n, cs, hipMemcpyHostToDevice, s));
    } else {
      if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.samp[evi], s));
      hipLaunchKernelGGL(sample_normal_kernel, dim3((unsigned)(rows * np / 256)), dim3(256), 0, s,
                         (double*)sm.Xi, np, rows, np, seed, first + (unsigned long long)j0);
      LAUNCH_CHECK("sample_normal_kernel");
      if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.samp[evi + 1], s));
    }
    if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.samp[evi + 2], s));
    hipLaunchKernelGGL(sample_trmm_kernel, dim3((unsigned)(items * jt)), dim3(256), 0, s,
                       (const double*)op->fac.A, np, (const double*)sm.Xi, np, jt, D, split,
                       (const uint32_t*)sm.order, (double*)sm.Y, np, (double*)sm.part);
    LAUNCH_CHECK("sample_trmm_kernel");
    if (split) {
      hipLaunchKernelGGL(sample_reduce_kernel, dim3((unsigned)(nt * jt), TS / 16), dim3(256), 0,
                         s, (const double*)sm.part, jt, D, (double*)sm.Y, np);
      LAUNCH_CHECK("sample_reduce_kernel");
    }
    if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.samp[evi + 3], s));
    HIP_TRY(hipMemcpy2DAsync(out + j0 * ldout, sizeof(double) * ldout, sm.Y, sizeof(double) * np,
                             sizeof(double) * n, cs, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (op->tim.on) {
      float ms = 0.f;
      if (!xi) {
        HIP_TRY(hipEventElapsedTime(&ms, op->tim.samp[evi], op->tim.samp[evi + 1]));
        sm.last_normal_ms += ms;
      }
      HIP_TRY(hipEventElapsedTime(&ms, op->tim.samp[evi + 2], op->tim.samp[evi + 3]));
      sm.last_trmm_ms += ms;
      // the tile products the grid runs (a diagonal tile counted whole)
      sm.last_trmm_flops += 2.0 * TS * TS * TS * (double)jt * nt * (nt + 1) / 2.0;
      evi += 4;
    }
  }
  return 0;
}

int gpmi_op_sample_ms(gpmi_op* op, double* normal_ms, double* trmm_ms, double* trmm_flops) {
  if (!op) return set_error(-1006, "null handle");
  if (normal_ms) *normal_ms = op->samp.last_normal_ms;
  if (trmm_ms) *trmm_ms = op->samp.last_trmm_ms;
  if (trmm_flops) *trmm_flops = op->samp.last_trmm_flops;
  return 0;
}

}  // extern "C"
