// The dense operator's prediction terms and joint covariance (include/gpmi.h:
// gpmi_op_predict_terms, gpmi_op_predict_cov, gpmi_op_predict_cov_resident; gpmi_op.h:
// DensePredict) on the cached
// factor: chunking, launch list and workspace sizes are gpmi_predict_plan.h, the kernels
// gpmi_predict.hip.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "gpmi_op.h"
#include "gpmi_predict_plan.h"

using namespace gpmi;

// Y = L^-1 rhs_src for the cached factor into PY, and G = Y^T Y into Pgram[0..256):
// from slot 0 of R when it still holds Y, else by forward substitution of rhs_src
// again (a solve since the factorization has overwritten R).
int gpmi::predict_refresh_y(gpmi_op* op) {
  DensePredict& p = op->pred;
  if (p.py_gen == op->factor_gen && p.py_rhs == op->rhs_gen) return 0;
  HIP_TRY(p.PY.reserve((size_t)op->n_pad * RLD));
  HIP_TRY(p.Pgram.reserve((size_t)(op->nt + 1) * 256));
  hipStream_t s = op->stream;
  BatchPtrs P = op->ptrs();
  if (p.ry_gen != op->factor_gen || p.ry_rhs != op->rhs_gen) {
    HIP_TRY(hipMemcpyAsync(op->fac.R, op->rhs_src, sizeof(double) * P.sR,
                           hipMemcpyDeviceToDevice, s));
    if (int rc = forward_substitute(op, P)) return rc;
    p.ry_gen = op->factor_gen;
    p.ry_rhs = op->rhs_gen;
  }
  HIP_TRY(hipMemcpyAsync(p.PY, op->fac.R, sizeof(double) * P.sR, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(pred_gram_kernel, dim3(op->nt), dim3(256), 0, s, p.PY, p.Pgram + 256);
  LAUNCH_CHECK("pred_gram_kernel");
  hipLaunchKernelGGL(pred_reduce_kernel, dim3(1), dim3(256), 0, s, p.Pgram + 256, op->nt,
                     (int64_t)256, p.Pgram);
  LAUNCH_CHECK("pred_reduce_kernel");
  p.py_gen = op->factor_gen;
  p.py_rhs = op->rhs_gen;
  return 0;
}

namespace {

// One call: its arguments, the shapes predict_check derives from them, and what the
// steps hand on.
struct PredictCall {
  double eta, nu;
  int d;
  const double *points, *scale, *test_points, *kstar;
  int64_t nstar, ldks;
  double *c_out, *q_out, *gram_out;
  bool cov;                    // gpmi_op_predict_cov: the joint covariance too
  const double* kss;           // K** that goes with an uploaded kstar
  int64_t ldkss, ldcov;
  double* cov_out;
  bool resident;               // gpmi_op_predict_cov_resident: C0 stays on the device only
  MaternParams MP;
  int NS;                      // chunk width in columns
  int wide;                    // the widest chunk of this call, in columns
  int64_t nsp;                 // nstar rounded up to a tile
  int cnct, csplit;            // covariance: column tiles of the whole block, depth pieces
  DevBuf<double> dp, dt, ds;   // points, test points and scale on the device (no kstar)
  size_t evi;                  // timing events recorded so far
  double trail_flops;
};

// Argument checks, the knobs (read per call) and the shapes they fix.
int predict_check(gpmi_op* op, PredictCall* c) {
  const int64_t nstar = c->nstar;
  if (!op->has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  if (op->nrhs < 1) return set_error(-1012, "no resident right-hand sides (gpmi_op_set_rhs)");
  if (nstar < 1) return set_errorf(-1013, "nstar must be positive (got %lld)", (long long)nstar);
  if (!c->kstar) {
    if (c->d < 1 || c->d > GPMI_MAX_DIM)
      return set_errorf(-1003, "dimension %d outside [1, %d]", c->d, GPMI_MAX_DIM);
    if (!c->points || !c->scale || !c->test_points) return set_error(-1004, "null argument");
    int rc = matern_params_host(c->nu, &c->MP);
    if (rc) return rc;
  } else if (c->ldks < op->n) {
    return set_errorf(-1014, "ldks %lld below n = %lld", (long long)c->ldks, (long long)op->n);
  }
  if (c->cov) {
    if (!c->cov_out && !c->resident) return set_error(-1004, "null argument");
    if (c->cov_out && c->ldcov < nstar)
      return set_errorf(-1016, "ldcov %lld below nstar = %lld", (long long)c->ldcov,
                        (long long)nstar);
    if (c->kstar && !c->kss)
      return set_error(-1017, "an uploaded kstar needs kss, the test points' own correlations");
    if (c->kstar && c->ldkss < nstar)
      return set_errorf(-1018, "ldkss %lld below nstar = %lld", (long long)c->ldkss,
                        (long long)nstar);
  }
  int64_t knob = 0;   // GPMI_PREDICT_CHUNK: the chunk width in columns
  if (const char* e = std::getenv("GPMI_PREDICT_CHUNK"))
    if (*e) knob = std::atoll(e) > 0 ? std::atoll(e) : -1;
  const int64_t np = op->n_pad;
  c->NS = predict_chunk_cols(np, knob);
  if (c->NS < 0)
    return set_error(-1015, "GPMI_PREDICT_CHUNK must be a positive multiple of 128");
  c->nsp = (nstar + TS - 1) / TS * TS;
  c->wide = (int)std::min<int64_t>(c->NS, c->nsp);
  // covariance: column tiles of the whole block, the depth split, and the cap
  c->cnct = 0;
  c->csplit = 1;
  if (c->cov) {
    c->cnct = (int)std::min<int64_t>(c->nsp / TS, 1 << 20);   // (beyond: over the cap in any case)
    if (!op->pred.ncu)
      HIP_TRY(hipDeviceGetAttribute(&op->pred.ncu, hipDeviceAttributeMultiprocessorCount,
                                    op->device));
    int64_t sknob = 0;   // GPMI_PREDICT_COV_SPLIT: the number of depth pieces
    if (const char* e = std::getenv("GPMI_PREDICT_COV_SPLIT"))
      if (*e) sknob = std::atoll(e);
    c->csplit = predict_cov_split(predict_cov_tiles(c->cnct), op->nt, 2 * op->pred.ncu, sknob);
    if (!predict_cov_fits(np, c->cnct, c->csplit))
      return set_errorf(-1019,
                        "covariance of %lld points at n_pad %lld, split %d is over the "
                        "%lld MiB cap",
                        (long long)nstar, (long long)np, c->csplit,
                        (long long)(PRED_COV_BYTES >> 20));
  }
  return 0;
}

// Workspace: grown to the widest chunk a call has needed, at most NS columns; PT holds
// one chunk, or, for the covariance, every test column. (PY and Pgram: predict_refresh_y.)
int predict_reserve(gpmi_op* op, const PredictCall& c) {
  DensePredict& p = op->pred;
  const int64_t np = op->n_pad;
  const PredictSizes sz = predict_sizes(np, op->nt, c.wide);
  const PredictCovSizes cz = predict_cov_sizes(np, c.cnct, c.csplit);
  HIP_TRY(p.PT.reserve(c.cov ? cz.T : sz.T));
  HIP_TRY(p.Ppart.reserve(sz.part));
  HIP_TRY(p.Pout.reserve(sz.out));
  if (c.cov) {
    p.cov_nstar = 0;   // (Pcov is about to be overwritten, or moved)
    HIP_TRY(p.Pcov.reserve(cz.cov));
    HIP_TRY(p.Pcpart.reserve(cz.part));
    if (op->tim.on) HIP_TRY(op->tim.cov.reserve(2, timing_event_flags()));
  }
  return 0;
}

// Chunk by chunk: k* of the chunk's test points into its rows of PT (the block itself,
// or the chunk's range of the whole block), T <- L^-1 T by the launch list, and the
// reduced partials back to the host.
int predict_chunks_run(gpmi_op* op, PredictCall* c) {
  DensePredict& p = op->pred;
  hipStream_t s = op->stream;
  const int64_t np = op->n_pad, n = op->n;
  const int nt = op->nt, m = op->nrhs;
  const std::vector<PredictLaunch> plan = predict_plan(nt, predict_outer(op->outer));
  std::vector<double> h((size_t)c->wide * PRED_LD);
  for (const PredictChunk& ch : predict_chunks(c->nstar, c->NS)) {
    const int nct = ch.nct;
    const int64_t rows = (int64_t)nct * TS;   // rows of T this chunk runs (<= wide)
    double* const PTc = p.PT + (c->cov ? predict_cov_row0(ch) * np : 0);
    if (c->kstar) {
      HIP_TRY(hipMemsetAsync(PTc, 0, sizeof(double) * rows * np, s));
      HIP_TRY(hipMemcpy2DAsync(PTc, sizeof(double) * np, c->kstar + ch.j0 * c->ldks,
                               sizeof(double) * c->ldks, sizeof(double) * n, ch.cols,
                               hipMemcpyHostToDevice, s));
    } else {
      launch_matern_cross(s, c->dp, n, c->dt + ch.j0 * c->d, ch.cols, c->d, c->ds, c->MP, PTc,
                          np, rows, np);
      LAUNCH_CHECK("matern_cross_kernel");
    }
    for (const PredictLaunch& L : plan) {
      if (L.kind == PRED_DIAG) {
        hipLaunchKernelGGL(pred_diag_kernel, dim3(nct), dim3(256), 0, s, op->fac.A, np,
                           op->fac.Linv, p.PY, PTc, np, L.r0, L.kb, p.Ppart, rows);
        LAUNCH_CHECK("pred_diag_kernel");
      } else {
        const int ni = L.r1 - L.r0;
        if (op->tim.on) {
          HIP_TRY(op->tim.pred.reserve(c->evi + 2, timing_event_flags()));
          HIP_TRY(hipEventRecord(op->tim.pred[c->evi++], s));
        }
        hipLaunchKernelGGL(pred_update_kernel, dim3(ni * nct), dim3(256), 0, s, op->fac.A, np,
                           PTc, np, L.r0, ni, nct, L.kb, L.ke);
        LAUNCH_CHECK("pred_update_kernel");
        if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.pred[c->evi++], s));
        c->trail_flops += 2.0 * TS * TS * (double)(L.ke - L.kb) * TS * ni * nct;
      }
    }
    const int64_t cnt = rows * PRED_LD;
    hipLaunchKernelGGL(pred_reduce_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s,
                       p.Ppart, nt, cnt, p.Pout);
    LAUNCH_CHECK("pred_reduce_kernel");
    HIP_TRY(hipMemcpyAsync(h.data(), p.Pout, sizeof(double) * ch.cols * PRED_LD,
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int j = 0; j < ch.cols; ++j) {
      if (c->c_out)
        for (int a = 0; a < m; ++a)
          c->c_out[(ch.j0 + j) * m + a] = h[(size_t)j * PRED_LD + a];
      if (c->q_out) c->q_out[ch.j0 + j] = h[(size_t)j * PRED_LD + 16];
    }
  }
  return 0;
}

// K** into Pcov [nsp][nsp] (pad rows / columns zero), then C0 = K** - V V^T in place
// from the whole block the chunks left in PT, and out to the host.
int predict_cov_tail(gpmi_op* op, const PredictCall& c) {
  DensePredict& p = op->pred;
  hipStream_t s = op->stream;
  const int64_t np = op->n_pad, nstar = c.nstar, ldc = c.nsp;
  if (c.kstar) {
    HIP_TRY(hipMemsetAsync(p.Pcov, 0, sizeof(double) * c.nsp * ldc, s));
    HIP_TRY(hipMemcpy2DAsync(p.Pcov, sizeof(double) * ldc, c.kss,
                             sizeof(double) * c.ldkss, sizeof(double) * nstar, nstar,
                             hipMemcpyHostToDevice, s));
  } else {
    launch_matern_cross(s, c.dt, nstar, c.dt, nstar, c.d, c.ds, c.MP, p.Pcov, ldc, c.nsp, c.nsp);
    LAUNCH_CHECK("matern_cross_kernel");
  }
  const int ntiles = (int)predict_cov_tiles(c.cnct);
  if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.cov[0], s));
  hipLaunchKernelGGL(pred_cov_partial_kernel, dim3((unsigned)(ntiles * c.csplit)), dim3(256), 0,
                     s, p.PT, np, c.cnct, op->nt, c.csplit, p.Pcpart);
  LAUNCH_CHECK("pred_cov_partial_kernel");
  if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.cov[1], s));
  hipLaunchKernelGGL(pred_cov_reduce_kernel, dim3(ntiles, TS / 16), dim3(256), 0, s, p.Pcpart,
                     c.csplit, c.cnct, p.Pcov, ldc);
  LAUNCH_CHECK("pred_cov_reduce_kernel");
  if (c.cov_out)
    HIP_TRY(hipMemcpy2DAsync(c.cov_out, sizeof(double) * c.ldcov, p.Pcov, sizeof(double) * ldc,
                             sizeof(double) * nstar, nstar, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  p.cov_nstar = nstar;   // Pcov holds C0 of this call (gpmi_op_load_predict_cov reads it)
  p.last_cov_ms = p.last_cov_flops = 0.0;
  p.last_cov_split = c.csplit;
  if (op->tim.on) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, op->tim.cov[0], op->tim.cov[1]));
    p.last_cov_ms = ms;
    p.last_cov_flops = 2.0 * TS * TS * (double)np * ntiles;
  }
  return 0;
}

// The call's end event, and the numbers of gpmi_op_predict_ms (0 without timing).
int predict_read_timing(gpmi_op* op, const PredictCall& c) {
  DensePredict& p = op->pred;
  p.last_pred_ms = p.last_pred_trail_ms = p.last_pred_trail_flops = 0.0;
  if (!op->tim.on) return 0;
  const EventPool& ev = op->tim.pred;
  HIP_TRY(hipEventRecord(ev[1], op->stream));
  HIP_TRY(hipEventSynchronize(ev[1]));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
  p.last_pred_ms = ms;
  double tr = 0.0;
  for (size_t e = 2; e + 1 < c.evi; e += 2) {
    HIP_TRY(hipEventElapsedTime(&ms, ev[e], ev[e + 1]));
    tr += ms;
  }
  p.last_pred_trail_ms = tr;
  p.last_pred_trail_flops = c.trail_flops;
  return 0;
}

// gpmi_op_predict_terms, gpmi_op_predict_cov and gpmi_op_predict_cov_resident. Without
// `cov` the working block holds one chunk at a time; with it every chunk keeps its rows of
// the whole block, and C0 = K** - V V^T follows the chunks (`resident`: the same launches
// without the download of C0).
int predict_run(gpmi_op* op, PredictCall* c) {
  if (!op) return set_error(-1006, "null handle");
  int rc = predict_check(op, c);
  if (rc) return rc;
  DeviceGuard g(op->device);
  hipStream_t s = op->stream;
  bool fresh;
  if ((rc = factor_ready(op, c->eta, op->rhs_src, &fresh))) return rc;
  if ((rc = predict_reserve(op, *c))) return rc;
  c->evi = 2;
  c->trail_flops = 0.0;
  if (op->tim.on) {
    HIP_TRY(op->tim.pred.reserve(2, timing_event_flags()));
    HIP_TRY(hipEventRecord(op->tim.pred[0], s));
  }
  if ((rc = predict_refresh_y(op))) return rc;
  if (!c->kstar) {
    const int64_t n = op->n, nstar = c->nstar;
    const int d = c->d;
    HIP_TRY(c->dp.reserve((size_t)n * d));
    HIP_TRY(c->dt.reserve((size_t)nstar * d));
    HIP_TRY(c->ds.reserve(d));
    HIP_TRY(hipMemcpyAsync(c->dp, c->points, sizeof(double) * n * d, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->dt, c->test_points, sizeof(double) * nstar * d,
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->ds, c->scale, sizeof(double) * d, hipMemcpyHostToDevice, s));
  }
  if ((rc = predict_chunks_run(op, c))) return rc;
  if (c->gram_out) {
    const int m = op->nrhs;
    double hg[256];
    HIP_TRY(hipMemcpyAsync(hg, op->pred.Pgram, sizeof(hg), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b) c->gram_out[a * m + b] = hg[a * RLD + b];
  }
  if (c->cov && (rc = predict_cov_tail(op, *c))) return rc;
  return predict_read_timing(op, *c);
}

}  // namespace

extern "C" {

int gpmi_op_predict_terms(gpmi_op* op, double eta, const double* points, int d,
                          const double* scale, double nu, const double* test_points,
                          int64_t nstar, const double* kstar, int64_t ldks, double* c_out,
                          double* q_out, double* gram_out) {
  PredictCall c = {eta,   nu,   d,     points, scale,    test_points, kstar,
                   nstar, ldks, c_out, q_out,  gram_out, false};
  return predict_run(op, &c);
}

int gpmi_op_predict_cov(gpmi_op* op, double eta, const double* points, int d,
                        const double* scale, double nu, const double* test_points,
                        int64_t nstar, const double* kstar, int64_t ldks, const double* kss,
                        int64_t ldkss, double* c_out, double* q_out, double* gram_out,
                        double* cov_out, int64_t ldcov) {
  PredictCall c = {eta,   nu,   d,     points, scale,    test_points, kstar,
                   nstar, ldks, c_out, q_out,  gram_out, true,        kss,
                   ldkss, ldcov, cov_out};
  return predict_run(op, &c);
}

int gpmi_op_predict_cov_resident(gpmi_op* op, double eta, const double* points, int d,
                                 const double* scale, double nu, const double* test_points,
                                 int64_t nstar, const double* kstar, int64_t ldks,
                                 const double* kss, int64_t ldkss, double* c_out,
                                 double* q_out, double* gram_out) {
  PredictCall c = {eta,   nu,   d,     points, scale,    test_points, kstar,
                   nstar, ldks, c_out, q_out,  gram_out, true,        kss,
                   ldkss, 0,    nullptr, true};
  return predict_run(op, &c);
}

int gpmi_op_predict_cov_ms(gpmi_op* op, double* product_ms, double* product_flops) {
  if (!op) return set_error(-1006, "null handle");
  if (product_ms) *product_ms = op->pred.last_cov_ms;
  if (product_flops) *product_flops = op->pred.last_cov_flops;
  return 0;
}

int gpmi_op_predict_cov_split(gpmi_op* op, int* split) {
  if (!op) return set_error(-1006, "null handle");
  if (split) *split = op->pred.last_cov_split;
  return 0;
}

int gpmi_op_predict_ms(gpmi_op* op, double* total_ms, double* trailing_ms,
                       double* trailing_flops) {
  if (!op) return set_error(-1006, "null handle");
  if (total_ms) *total_ms = op->pred.last_pred_ms;
  if (trailing_ms) *trailing_ms = op->pred.last_pred_trail_ms;
  if (trailing_flops) *trailing_flops = op->pred.last_pred_trail_flops;
  return 0;
}

}  // extern "C"
