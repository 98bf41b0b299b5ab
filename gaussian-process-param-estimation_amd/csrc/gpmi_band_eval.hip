// Evaluator of the band path: the likelihood terms of B + eta I for a batch of etas
// from the band Ab and Q^T R in Y: logdet and Gram blocks by block cyclic reduction or
// the sequential banded Cholesky, the eta-derivative terms, and trace((B + eta I)^-1),
// ^-2 by selected inversion and its eta-tangent (kernels: gpmi_bcr.hip, gpmi_band.hip).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "gpmi_band_host.h"

using namespace gpmi;

namespace {

// The caller's arrays of one call (null: not wanted), per eta: logdet, the Gram blocks
// [nrhs][nrhs] of exponents 1 to 3, the traces of exponents 1 and 2, info.
struct EvalOut {
  double *logdet, *g1, *g2, *g3, *tr1, *tr2;
  int* info;
  EvalOut at(int e, size_t mm) const {   // the arrays from eta e on (mm = nrhs^2)
    return {logdet ? logdet + e : nullptr, g1 ? g1 + e * mm : nullptr,
            g2 ? g2 + e * mm : nullptr,    g3 ? g3 + e * mm : nullptr,
            tr1 ? tr1 + e : nullptr,       tr2 ? tr2 + e : nullptr,
            info ? info + e : nullptr};
  }
};

// The etas of a call onto the device (the io group holds them), then ev0.
int eval_begin(gpmi_band* b, const double* etas, int neta) {
  HIP_TRY(hipMemcpyAsync(b->io.etas, etas, sizeof(double) * neta, hipMemcpyHostToDevice,
                         b->stream));
  HIP_TRY(hipEventRecord(b->ev0, b->stream));
  return 0;
}

// The device results of neta etas into the caller's arrays, behind what is queued on
// the main stream, which is waited for.
int copy_back(gpmi_band* b, int neta, const EvalOut& o) {
  hipStream_t s = b->stream;
  const size_t ne = (size_t)neta, dl = 2 * RLD * RLD;
  std::vector<double> hout(o.logdet || o.g1 ? ne * OUT_LD : 0), hder(o.g2 || o.g3 ? ne * dl : 0);
  if (o.tr1)
    HIP_TRY(hipMemcpyAsync(o.tr1, b->eval.sinv.Tr + ne * b->nt, sizeof(double) * ne,
                           hipMemcpyDeviceToHost, s));
  if (o.tr2)
    HIP_TRY(hipMemcpyAsync(o.tr2, b->eval.tan.Tr + ne * b->nt, sizeof(double) * ne,
                           hipMemcpyDeviceToHost, s));
  if (!hout.empty())
    HIP_TRY(hipMemcpyAsync(hout.data(), b->io.out, sizeof(double) * hout.size(),
                           hipMemcpyDeviceToHost, s));
  if (!hder.empty())
    HIP_TRY(hipMemcpyAsync(hder.data(), b->eval.der.der, sizeof(double) * hder.size(),
                           hipMemcpyDeviceToHost, s));
  if (o.info)
    HIP_TRY(hipMemcpyAsync(o.info, b->io.info, sizeof(int) * ne, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int m = b->nrhs;
  for (size_t e = 0; e < ne; ++e) {
    if (o.logdet) o.logdet[e] = hout[e * OUT_LD];
    for (int a = 0; a < m; ++a)
      for (int c = 0; c < m; ++c) {
        const size_t at = (e * m + a) * m + c;
        if (o.g1) o.g1[at] = hout[e * OUT_LD + 1 + a * RLD + c];
        if (o.g2) o.g2[at] = hder[e * dl + a * RLD + c];
        if (o.g3) o.g3[at] = hder[e * dl + RLD * RLD + a * RLD + c];
      }
  }
  return 0;
}

int elapsed_ms(hipEvent_t from, hipEvent_t to, double* ms) {
  float f = 0.f;
  HIP_TRY(hipEventElapsedTime(&f, from, to));
  *ms = f;
  return 0;
}

bool use_bcr(const gpmi_band* b, int neta) {
  return b->eval.bcr_mode == 1 || (b->eval.bcr_mode == 2 && neta <= 64);
}

// The likelihood terms of neta eta (b->io.etas on the device) by block cyclic
// reduction (gpmi_bcr.hip) into b->io.out / info, on stream s. With tan (neta <= the
// tangent group's capacity), also every eliminated block's dLinv and dW (bcr_dfac /
// bcr_dw / bcr_dupd) for band_sinv_bcr's exponent-2 trace.
int band_loglik_bcr(gpmi_band* b, int neta, hipStream_t s, bool tan = false) {
  BandEval& ev = b->eval;
  BandBcr& c = ev.bcr;
  BandTan& t = ev.tan;
  const BandPlan& p = ev.plan;
  const int nt = b->nt;
  const int64_t np = b->n_pad;
  if (neta > c.cap && ev.sol_path == 2) ev.sol_path = 0;   // X is released with the group
  HIP_TRY(c.reserve(neta, p));
  if (nt > 1) {
    HIP_TRY(ev.F0.reserve((size_t)(nt - 1) * TS * TS));
    hipLaunchKernelGGL(bcr_f0_kernel, dim3(nt - 1), dim3(256), 0, s, b->Ab, np, ev.F0);
    LAUNCH_CHECK("bcr_f0_kernel");
  }
  const double* Din = nullptr;
  const double* Yin = b->Y;
  const double* Fin = ev.F0;
  const double* dDin = nullptr;   // tangents of the level's D, F (level 0: I, 0)
  const double* dFin = nullptr;
  int64_t sD = 0, sY = 0, sF = 0;
  int cur = 0;
  bool dupd_pending = false;   // the last bcr_dupd_kernel (side stream) not yet waited for
  const int L = (int)ev.levels.size();
  for (int lvl = 0; lvl < L; ++lvl) {
    const int m = ev.levels[lvl], nodd = m / 2, neven = (m + 1) / 2;
    hipLaunchKernelGGL(bcr_chol_kernel, dim3(nodd, neta), dim3(256), 0, s, b->Ab, np, b->io.etas,
                       lvl, 1, Din, sD, Yin, sY, c.L, p.sL, 1, c.Z, p.sZ, c.Ld, c.G, c.Fail, nt,
                       b->n);
    LAUNCH_CHECK("bcr_chol_kernel");
    // W (and with tangents the level's dLinv beside it), then D', F', Y' (and dW),
    // then dD', dF' on the side stream beside the next level's Cholesky (the dLinv of
    // the next bcr_w_kernel launch waits for them)
    if (dupd_pending) HIP_TRY(hipStreamWaitEvent(s, b->red.ev_t, 0));
    dupd_pending = false;
    hipLaunchKernelGGL(bcr_w_kernel, dim3(2 * nodd + (tan ? nodd : 0), neta), dim3(256), 0, s,
                       c.L, p.sL, Fin, sF, c.W, p.sW, m, lvl, dDin, p.sH, t.X, t.L);
    LAUNCH_CHECK("bcr_w_kernel");
    hipLaunchKernelGGL(bcr_upd_kernel, dim3(3 * neven + (tan ? 2 * nodd : 0), neta), dim3(256), 0,
                       s, b->Ab, np, b->io.etas, lvl, Din, sD, Yin, sY, c.W, p.sW, c.Z, p.sZ,
                       c.D[cur], c.F[cur], c.Y[cur], p.sH, p.sHY, m, c.L, t.L, p.sL, Fin, sF, dFin,
                       p.sH, t.W);
    LAUNCH_CHECK("bcr_upd_kernel");
    if (tan) {
      HIP_TRY(hipEventRecord(b->red.ev_v, s));
      HIP_TRY(hipStreamWaitEvent(b->side, b->red.ev_v, 0));
      hipLaunchKernelGGL(bcr_dupd_kernel, dim3(2 * neven, neta), dim3(256), 0, b->side, c.W, t.W,
                         p.sW, dDin, p.sH, t.D[cur], t.F[cur], p.sH, m, lvl);
      LAUNCH_CHECK("bcr_dupd_kernel");
      HIP_TRY(hipEventRecord(b->red.ev_t, b->side));
      dupd_pending = true;
      dDin = t.D[cur];
      dFin = t.F[cur];
    }
    Din = c.D[cur];
    Yin = c.Y[cur];
    Fin = c.F[cur];
    sD = p.sH;
    sY = p.sHY;
    sF = p.sH;
    cur ^= 1;
  }
  hipLaunchKernelGGL(bcr_chol_kernel, dim3(1, neta), dim3(256), 0, s, b->Ab, np, b->io.etas, L, 0,
                     Din, sD, Yin, sY, c.L, p.sL, 1, c.Z, p.sZ, c.Ld, c.G, c.Fail, nt, b->n);
  LAUNCH_CHECK("bcr_chol_kernel");
  if (tan) {   // the last level's dLinv (bcr_w_kernel with m = 1: its dfac role only)
    if (dupd_pending) HIP_TRY(hipStreamWaitEvent(s, b->red.ev_t, 0));
    hipLaunchKernelGGL(bcr_w_kernel, dim3(1, neta), dim3(256), 0, s, c.L, p.sL, nullptr, 0,
                       nullptr, p.sW, 1, L, dDin, p.sH, t.X, t.L);
    LAUNCH_CHECK("bcr_w_kernel");
  }
  hipLaunchKernelGGL(bcr_final_kernel, dim3(neta), dim3(256), 0, s, c.Ld, c.G, c.Fail, nt,
                     b->io.out, OUT_LD, b->io.info);
  LAUNCH_CHECK("bcr_final_kernel");
  return 0;
}

// Derivative terms by cyclic reduction (after band_loglik_bcr, whose levels stay
// stored): X = (B + eta I)^-1 Y by back substitution from the last level down, then
// the forward elimination of X; G2, G3 into the der group's der (gpmi_bcr.hip).
int band_der_solves(gpmi_band* b, int neta, hipStream_t s) {
  BandBcr& c = b->eval.bcr;
  const BandPlan& p = b->eval.plan;
  const std::vector<int>& ms = b->eval.levels;
  const int nt = b->nt, L = (int)ms.size();
  hipLaunchKernelGGL(bcr_back_kernel, dim3(1, neta), dim3(256), 0, s, c.L, p.sL, c.W, p.sW, c.Z,
                     p.sZ, c.X, c.G2, nt, L, 0, 1);
  LAUNCH_CHECK("bcr_back_kernel");
  for (int l = L - 1; l >= 0; --l) {
    hipLaunchKernelGGL(bcr_back_kernel, dim3(ms[l] / 2, neta), dim3(256), 0, s, c.L, p.sL, c.W,
                       p.sW, c.Z, p.sZ, c.X, c.G2, nt, l, 1, ms[l]);
    LAUNCH_CHECK("bcr_back_kernel");
  }
  const double* Yin = c.X;
  int64_t sY = p.sZ;
  int cur = 0;
  for (int l = 0; l < L; ++l) {
    hipLaunchKernelGGL(bcr_rhs_odd_kernel, dim3(ms[l] / 2, neta), dim3(256), 0, s, c.L, p.sL, Yin,
                       sY, c.Zp, p.sZ, c.G3, nt, l, 1);
    LAUNCH_CHECK("bcr_rhs_odd_kernel");
    hipLaunchKernelGGL(bcr_rhs_even_kernel, dim3((ms[l] + 1) / 2, neta), dim3(256), 0, s, c.W,
                       p.sW, c.Zp, p.sZ, Yin, sY, c.Y[cur], p.sHY, l, ms[l]);
    LAUNCH_CHECK("bcr_rhs_even_kernel");
    Yin = c.Y[cur];
    sY = p.sHY;
    cur ^= 1;
  }
  hipLaunchKernelGGL(bcr_rhs_odd_kernel, dim3(1, neta), dim3(256), 0, s, c.L, p.sL, Yin, sY, c.Zp,
                     p.sZ, c.G3, nt, L, 0);
  LAUNCH_CHECK("bcr_rhs_odd_kernel");
  hipLaunchKernelGGL(bcr_der_final_kernel, dim3(neta), dim3(256), 0, s, c.G2, c.G3, nt,
                     b->eval.der.der);
  LAUNCH_CHECK("bcr_der_final_kernel");
  return 0;
}

// tr((B + eta_e I)^-1) for the neta etas whose cyclic-reduction factor band_loglik_bcr
// left in the bcr group's L / W: selected inversion down the tree, top-down
// (gpmi_bcr.hip bcr_sinv_*), into sinv.Tr[nt * neta + e] (device). With tan (the
// factor's tangents computed by band_loglik_bcr(.., tan)) also tr((B + eta_e I)^-2)
// into tan.Tr[nt * neta + e] (bcr_dsinv_*).
int band_sinv_bcr(gpmi_band* b, int neta, hipStream_t s, bool tan = false) {
  BandBcr& c = b->eval.bcr;
  BandSinv& v = b->eval.sinv;
  BandTan& t = b->eval.tan;
  const BandPlan& p = b->eval.plan;
  const std::vector<int>& ms = b->eval.levels;
  const int nt = b->nt, L = (int)ms.size();
  b->eval.sinv_neta = 0;   // (the read-back's bookkeeping: nothing until this call is queued)
  b->eval.sinv_tan = false;
  HIP_TRY(v.reserve(neta, p));
  const int64_t sZd = p.sL, sZo = p.sW, sX = p.sW;
  const int nt_ = tan ? 1 : 0;
  b->eval.sinv_neta = neta;
  b->eval.sinv_tan = tan;
  // every block's X_l, X_r, Linv^T Linv (and tangents), the root's trace
  hipLaunchKernelGGL(bcr_sinv_pre_kernel, dim3(nt * (3 + 3 * nt_), neta), dim3(256), 0, s, c.L,
                     t.L, p.sL, c.W, t.W, p.sW, v.X, t.X, sX, v.Zd, t.Zd, sZd, v.Tr, t.Tr, nt, L,
                     b->n, nt_);
  LAUNCH_CHECK("bcr_sinv_pre_kernel");
  for (int l = L - 1; l >= 0; --l) {
    const int nodd = ms[l] / 2;
    hipLaunchKernelGGL(bcr_sinv_off_kernel, dim3((2 + 2 * nt_) * nodd, neta), dim3(256), 0, s,
                       v.Zd, t.Zd, sZd, v.Zo, t.Zo, sZo, v.X, t.X, sX, ms[l], l, nt_);
    LAUNCH_CHECK("bcr_sinv_off_kernel");
    hipLaunchKernelGGL(bcr_sinv_diag_kernel, dim3((1 + nt_) * nodd, neta), dim3(256), 0, s, v.X,
                       t.X, sX, v.Zo, t.Zo, sZo, v.Zd, t.Zd, sZd, v.Tr, t.Tr, nt, b->n, ms[l], l,
                       nt_);
    LAUNCH_CHECK("bcr_sinv_diag_kernel");
  }
  hipLaunchKernelGGL(bcr_sinv_final_kernel, dim3((neta + 63) / 64), dim3(64), 0, s, v.Tr, nt,
                     v.Tr + (size_t)nt * neta, neta);
  LAUNCH_CHECK("bcr_sinv_final_kernel");
  if (tan) {
    hipLaunchKernelGGL(bcr_sinv_final_kernel, dim3((neta + 63) / 64), dim3(64), 0, s, t.Tr, nt,
                       t.Tr + (size_t)nt * neta, neta);
    LAUNCH_CHECK("bcr_sinv_final_kernel");
  }
  return 0;
}

// The derivative terms of one chunk of etas (o.tr2: at most GPMI_BAND_TAN_MAX).
int der_terms_chunk(gpmi_band* b, const double* etas, int neta, const EvalOut& o) {
  BandEval& ev = b->eval;
  const bool tr = o.tr1 || o.tr2, tan = o.tr2 != nullptr;
  HIP_TRY(b->io.reserve(neta));
  HIP_TRY(ev.der.reserve(neta, ev.plan));
  if (tan) {
    ev.sinv_tan = false;
    HIP_TRY(ev.tan.reserve(neta, ev.plan));
  }
  hipStream_t s = b->stream;
  ev.sol_path = 0;
  int rc = eval_begin(b, etas, neta);
  if (rc) return rc;
  // the traces need the cyclic-reduction factor (the tree they invert along); the
  // selected inversion (side stream) and the G2 / G3 solves (s) both read only the
  // factor, so they run side by side
  if (tr) {
    if ((rc = band_loglik_bcr(b, neta, s, tan))) return rc;
    HIP_TRY(hipEventRecord(b->red.ev_q, s));
    HIP_TRY(hipStreamWaitEvent(b->side, b->red.ev_q, 0));
    HIP_TRY(hipEventRecord(b->ev2, b->side));
    if ((rc = band_sinv_bcr(b, neta, b->side, tan))) return rc;
    HIP_TRY(hipEventRecord(b->ev3, b->side));
    if ((rc = band_der_solves(b, neta, s))) return rc;
    HIP_TRY(hipStreamWaitEvent(s, b->ev3, 0));
  } else if (use_bcr(b, neta)) {
    if ((rc = band_loglik_bcr(b, neta, s))) return rc;
    if ((rc = band_der_solves(b, neta, s))) return rc;
  } else {
    hipLaunchKernelGGL(band_chol_kernel, dim3(neta), dim3(256), 0, s, b->Ab, b->n_pad, b->nt,
                       b->n, b->Y, b->io.etas, b->io.out, OUT_LD, b->io.info, ev.der.fac,
                       ev.der.ysol);
    LAUNCH_CHECK("band_chol_kernel");
    hipLaunchKernelGGL(band_der_kernel, dim3(neta), dim3(256), 0, s, ev.der.fac, b->nt,
                       ev.der.ysol, ev.der.der);
    LAUNCH_CHECK("band_der_kernel");
  }
  HIP_TRY(hipEventRecord(b->ev1, s));
  if ((rc = copy_back(b, neta, o))) return rc;
  // what gpmi_band_get_solution may return (host bookkeeping; the info of a caller
  // that did not ask for it is read here)
  ev.sol_info.assign((size_t)neta, 0);
  if (o.info)
    std::copy(o.info, o.info + neta, ev.sol_info.begin());
  else
    HIP_TRY(hipMemcpy(ev.sol_info.data(), b->io.info, sizeof(int) * neta, hipMemcpyDeviceToHost));
  ev.sol_neta = neta;
  ev.sol_path = (tr || use_bcr(b, neta)) ? 2 : 1;
  if ((rc = elapsed_ms(b->ev0, b->ev1, &ev.der_ms))) return rc;
  return tr ? elapsed_ms(b->ev2, b->ev3, &ev.sinv_ms) : 0;
}

// The traces alone of one chunk: everything on the main stream.
int traceinv_chunk(gpmi_band* b, const double* etas, int neta, const EvalOut& o) {
  BandEval& ev = b->eval;
  const bool tan = o.tr2 != nullptr;
  HIP_TRY(b->io.reserve(neta));
  if (tan) {
    ev.sinv_tan = false;
    HIP_TRY(ev.tan.reserve(neta, ev.plan));
  }
  hipStream_t s = b->stream;
  int rc = eval_begin(b, etas, neta);
  if (rc) return rc;
  if ((rc = band_loglik_bcr(b, neta, s, tan))) return rc;
  HIP_TRY(hipEventRecord(b->ev2, s));
  if ((rc = band_sinv_bcr(b, neta, s, tan))) return rc;
  HIP_TRY(hipEventRecord(b->ev1, s));
  if ((rc = copy_back(b, neta, o))) return rc;
  return elapsed_ms(b->ev2, b->ev1, &ev.sinv_ms);
}

// `chunk` over the etas of a call: with tr2 in ranges of at most GPMI_BAND_TAN_MAX
// (the tangent group is sized per chunk), else all at once.
int eval_chunks(gpmi_band* b, const double* etas, int neta, const EvalOut& o,
                int (*chunk)(gpmi_band*, const double*, int, const EvalOut&)) {
  DeviceGuard g(b->device);
  const size_t mm = (size_t)b->nrhs * b->nrhs;
  for (const EtaChunk& c : eta_chunks(neta, o.tr2 ? GPMI_BAND_TAN_MAX : neta)) {
    int rc = chunk(b, etas + c.begin, c.count, o.at(c.begin, mm));
    if (rc) return rc;
  }
  return 0;
}

}  // namespace

extern "C" {

int gpmi_band_loglik(gpmi_band* b, const double* etas, int neta, double* logdet, double* gram,
                     int* info) {
  if (!b) return set_error(-1006, "null handle");
  if (neta <= 0) return 0;
  DeviceGuard g(b->device);
  HIP_TRY(b->io.reserve(neta));
  hipStream_t s = b->stream;
  int rc = eval_begin(b, etas, neta);
  if (rc) return rc;
  if (use_bcr(b, neta)) {
    if ((rc = band_loglik_bcr(b, neta, s))) return rc;
  } else {
    hipLaunchKernelGGL(band_chol_kernel, dim3(neta), dim3(256), 0, s, b->Ab, b->n_pad, b->nt,
                       b->n, b->Y, b->io.etas, b->io.out, OUT_LD, b->io.info, nullptr, nullptr);
    LAUNCH_CHECK("band_chol_kernel");
  }
  HIP_TRY(hipEventRecord(b->ev1, s));
  if ((rc = copy_back(b, neta, {logdet, gram, nullptr, nullptr, nullptr, nullptr, info})))
    return rc;
  return elapsed_ms(b->ev0, b->ev1, &b->loglik_ms);
}

int gpmi_band_der_terms(gpmi_band* b, const double* etas, int neta, double* logdet,
                        double* g1, double* g2, double* g3, int* info) {
  return gpmi_band_der_terms_ex2(b, etas, neta, logdet, g1, g2, g3, nullptr, nullptr, info);
}

int gpmi_band_der_terms_ex(gpmi_band* b, const double* etas, int neta, double* logdet,
                           double* g1, double* g2, double* g3, double* tr1, int* info) {
  return gpmi_band_der_terms_ex2(b, etas, neta, logdet, g1, g2, g3, tr1, nullptr, info);
}

int gpmi_band_der_terms_ex2(gpmi_band* b, const double* etas, int neta, double* logdet,
                            double* g1, double* g2, double* g3, double* tr1, double* tr2,
                            int* info) {
  if (!b) return set_error(-1006, "null handle");
  if (neta <= 0) return 0;
  if (neta > GPMI_BAND_DER_MAX)
    return set_error(-1203, "gpmi_band_der_terms: at most GPMI_BAND_DER_MAX etas per call");
  return eval_chunks(b, etas, neta, {logdet, g1, g2, g3, tr1, tr2, info}, der_terms_chunk);
}

int gpmi_band_traceinv(gpmi_band* b, const double* etas, int neta, double* tr, int* info) {
  return gpmi_band_traceinv2(b, etas, neta, tr, nullptr, info);
}

int gpmi_band_traceinv2(gpmi_band* b, const double* etas, int neta, double* tr1, double* tr2,
                        int* info) {
  if (!b) return set_error(-1006, "null handle");
  if (neta <= 0) return 0;
  if (neta > GPMI_BAND_DER_MAX)
    return set_error(-1203, "gpmi_band_traceinv: at most GPMI_BAND_DER_MAX etas per call");
  if (!tr1) return set_error(-1006, "gpmi_band_traceinv2: tr1 is required");
  return eval_chunks(b, etas, neta, {nullptr, nullptr, nullptr, nullptr, tr1, tr2, info},
                     traceinv_chunk);
}

}  // extern "C"
