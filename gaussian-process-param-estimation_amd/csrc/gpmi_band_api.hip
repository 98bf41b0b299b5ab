// C-ABI of the band path (include/gpmi.h, gpmi_band_*): the handle's life (create,
// refresh, destroy), the resident RHS, the getters and the GPMI_* knobs. The reduction,
// the evaluator and the eigenvalues are gpmi_band_reduce.hip, gpmi_band_eval.hip and
// gpmi_band_eig.hip; the handle itself is gpmi_band_host.h.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "gpmi_band_host.h"

using namespace gpmi;

namespace {

// RHS [n][ld] (nrhs columns) -> the padded [n_pad][16] host layout of Y.
std::vector<double> pack_rhs(const gpmi_band* b, const double* rhs, int64_t ld, int nrhs) {
  std::vector<double> h((size_t)b->n_pad * RLD, 0.0);
  for (int64_t i = 0; i < b->n; ++i)
    for (int c = 0; c < nrhs; ++c) h[(size_t)i * RLD + c] = rhs[i * ld + c];
  return h;
}

}  // namespace

extern "C" {

int gpmi_band_create(gpmi_op* op, gpmi_band** out) {
  if (!out) return set_error(-1004, "null output handle");
  OpView v;
  int rc = op_view(op, &v);
  if (rc) return rc;
  if (!v.has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  if (v.n_pad > BAND_MAX_NPAD) return set_error(-1200, "band path supports n <= 32768");
  DeviceGuard g(v.device);
  std::unique_ptr<gpmi_band> owner(new gpmi_band());   // (a failed create just deletes it)
  gpmi_band* b = owner.get();
  BandReduce& r = b->red;
  b->device = v.device;
  b->n = v.n;
  b->n_pad = v.n_pad;
  b->nt = (int)(v.n_pad / TS);
  const int64_t np = b->n_pad;
  const int nt = b->nt;
  b->eval.plan = BandPlan(nt);
  b->eval.levels = bcr_levels(nt);
  HIP_TRY(hipDeviceGetAttribute(&b->ncu, hipDeviceAttributeMultiprocessorCount, v.device));
  const size_t nch = (size_t)std::max<int64_t>(1, (np + TN_CH - 1) / TN_CH);
  const size_t blk = (size_t)TS * TS;
  HIP_TRY(hipStreamCreateWithFlags(&b->stream.h, hipStreamNonBlocking));
  for (Event* ev : {&b->ev0, &b->ev1, &b->ev2, &b->ev3}) HIP_TRY(hipEventCreate(&ev->h));
  HIP_TRY(hipStreamCreateWithFlags(&b->side.h, hipStreamNonBlocking));
  if (const char* la = std::getenv("GPMI_BAND_LA")) r.lookahead = std::atoi(la);
  if (const char* po = std::getenv("GPMI_BAND_POISON")) r.poison = std::atoi(po) != 0;
  if (const char* v = std::getenv("GPMI_LA_FREE")) r.la_free = std::max(1, std::atoi(v));
  if (const char* v = std::getenv("GPMI_LA_FREE_LATE")) r.la_free_late = std::max(1, std::atoi(v));
  if (const char* v = std::getenv("GPMI_LA_LATE_MT")) r.la_late_mt = std::atoi(v);
  if (const char* pm = std::getenv("GPMI_BAND_PANEL")) r.panel_mode = std::strcmp(pm, "hh") == 0;
  if (const char* bm = std::getenv("GPMI_BAND_BCR"))
    b->eval.bcr_mode = std::max(0, std::min(2, std::atoi(bm)));
  // GPMI_CQ_FO=0: every CholeskyQR pass by an exact Cholesky (no first-order passes)
  if (const char* fo = std::getenv("GPMI_CQ_FO"))
    if (std::atoi(fo) == 0) r.cq_fo[1] = r.cq_fo[2] = 0.0;
  // test hook: GPMI_CHASE_SPIN_LIMIT=0 times the systolic chase out at its first wait
  if (const char* sl = std::getenv("GPMI_CHASE_SPIN_LIMIT"))
    b->eig.chase_spin = (unsigned)std::strtoul(sl, nullptr, 10);
  // test hook: GPMI_HH_SPIN_LIMIT=0 makes the first unsuccessful poll a timeout
  if (const char* sl = std::getenv("GPMI_HH_SPIN_LIMIT"))
    r.spin_limit = (unsigned)std::strtoul(sl, nullptr, 10);

  if (r.lookahead) {
    // s_pan at the high dispatch priority. Alone, the priorities do not matter (135.5
    // ms all normal, 135.9-136.3 with one stream high); in a process that holds other
    // operators' streams (the bench line: the dense operator's) a high-priority stream
    // gets a hardware queue of its own, while normal-priority streams beyond the
    // process's GPU_MAX_HW_QUEUES (4) share queues and serialise: the bench line's
    // reduction took 165.4 ms with all three at normal priority, 137 with this one high
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(hipStreamCreateWithPriority(&r.s_pan.h, hipStreamNonBlocking, hi));
    for (Event* ev : {&r.ev_col, &r.ev_pan})
      HIP_TRY(hipEventCreateWithFlags(&ev->h, sync_event_flags()));
  }
  for (Event* ev : {&r.ev_q, &r.ev_v, &r.ev_t, &r.ev_rc})
    HIP_TRY(hipEventCreateWithFlags(&ev->h, sync_event_flags()));
  HIP_TRY(b->Ab.reserve(np * np));
  HIP_TRY(r.U.reserve(np * BAND_ULD));
  HIP_TRY(r.X.reserve(np * TS));
  HIP_TRY(r.X2.reserve(np * TS));
  HIP_TRY(r.Xp.reserve(xp_tiles(nt, b->ncu) * blk));
  HIP_TRY(r.part.reserve(2 * HH_MAXG * HH_PART_LD));
  HIP_TRY(r.pivrow.reserve(2 * TS));
  HIP_TRY(r.tau.reserve((size_t)nt * TS));
  HIP_TRY(r.Tm.reserve(nt * blk));
  HIP_TRY(r.tnp.reserve(nch * blk));
  HIP_TRY(r.tnp2.reserve(nch * blk));
  HIP_TRY(r.VtV.reserve(blk));
  HIP_TRY(r.M.reserve(blk));
  HIP_TRY(r.Zh.reserve(blk));
  HIP_TRY(b->Y.reserve(np * RLD));
  HIP_TRY(r.qtp.reserve((size_t)(np / QT_ROWS + 1) * TS * RLD));
  HIP_TRY(r.qa.reserve(TS * RLD));
  HIP_TRY(r.qb.reserve(TS * RLD));
  HIP_TRY(r.Qb.reserve(np * TS));
  HIP_TRY(r.cqpart.reserve((size_t)(np / 64) * CQ_GPK));
  HIP_TRY(r.cqG.reserve(blk));
  HIP_TRY(r.cqL.reserve(nt * 3 * blk));
  HIP_TRY(r.cqLinv.reserve(nt * 3 * blk));
  HIP_TRY(r.cqMinv.reserve(blk));
  HIP_TRY(r.cqUS.reserve(nt * blk));
  HIP_TRY(r.cqW.reserve(nt * blk));
  r.t_from_q.assign((size_t)nt, 0);
  r.v_in_u.assign((size_t)nt, 0);
  HIP_TRY(r.cqS.reserve((size_t)nt * TS));
  HIP_TRY(r.cqscr.reserve(nt * blk));
  HIP_TRY(r.cqflag.reserve((size_t)8 * nt));
  if (nt > 2) {
    const std::vector<uint32_t> h = syr2k_tile_order(nt, &r.rorder_off);
    HIP_TRY(r.rorder.reserve(h.size()));
    HIP_TRY(hipMemcpy(r.rorder, h.data(), sizeof(uint32_t) * h.size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(r.ctr.reserve(512 / sizeof(unsigned)));
  HIP_TRY(r.err.reserve(16 / sizeof(int)));
  HIP_TRY(hipMemsetAsync(r.err, 0, 16, b->stream));
  // per device (this one is current): cheap, so set on every create
  for (const void* f : {reinterpret_cast<const void*>(&cq_gram_kernel),
                        reinterpret_cast<const void*>(&cq_apply_kernel)})
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, CQ_DYN_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&hh_panel_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, HH_PANEL_LDS));
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, reinterpret_cast<const void*>(&hh_panel_kernel), HH_THREADS, HH_PANEL_LDS));
  r.panel_maxg = std::min(HH_PANEL_MAXG, std::max(0, per_cu) * b->ncu);
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, reinterpret_cast<const void*>(&chase_systolic_kernel), CHASE_THREADS, 0));
  b->eig.chase_maxg = std::max(0, per_cu) * b->ncu;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, reinterpret_cast<const void*>(&chase_split_kernel), CHASE_SPLIT_THREADS, 0));
  b->eig.split_maxg = std::max(0, per_cu) * b->ncu;
  HIP_TRY(hipMemsetAsync(r.U, 0, sizeof(double) * np * BAND_ULD, b->stream));
  HIP_TRY(hipMemsetAsync(b->Y, 0, sizeof(double) * np * RLD, b->stream));
  rc = band_reduce(b, v.K);
  if (rc) return rc;
  *out = owner.release();
  return 0;
}

int gpmi_band_refresh(gpmi_band* b, gpmi_op* op) {
  if (!b) return set_error(-1006, "null handle");
  OpView v;
  int rc = op_view(op, &v);
  if (rc) return rc;
  if (!v.has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  if (v.n != b->n || v.device != b->device)
    return set_error(-1202, "operator size or device differs from the band's");
  DeviceGuard g(b->device);
  b->nrhs = 0;
  return band_reduce(b, v.K);
}

int gpmi_band_refresh_rhs(gpmi_band* b, gpmi_op* op, const double* rhs, int64_t ld, int nrhs) {
  if (!b) return set_error(-1006, "null handle");
  if (nrhs < 0 || nrhs > RLD) return set_error(-1007, "nrhs outside [0, 16]");
  OpView v;
  int rc = op_view(op, &v);
  if (rc) return rc;
  if (!v.has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  if (v.n != b->n || v.device != b->device)
    return set_error(-1202, "operator size or device differs from the band's");
  DeviceGuard g(b->device);
  b->nrhs = 0;
  const std::vector<double> h = pack_rhs(b, rhs, ld, nrhs);
  rc = band_reduce(b, v.K, &h);
  if (rc) return rc;
  b->nrhs = nrhs;
  b->rhs_ms = 0.0;   // overlapped with the reduction
  return 0;
}

int gpmi_band_destroy(gpmi_band* b) {
  if (!b) return 0;
  DeviceGuard g(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  delete b;
  return 0;
}

int gpmi_band_set_rhs(gpmi_band* b, const double* rhs, int64_t ld, int nrhs) {
  if (!b) return set_error(-1006, "null handle");
  if (nrhs < 0 || nrhs > RLD) return set_error(-1007, "nrhs outside [0, 16]");
  DeviceGuard g(b->device);
  hipStream_t s = b->stream;
  const std::vector<double> h = pack_rhs(b, rhs, ld, nrhs);
  b->eval.sol_path = 0;   // a solution read back would belong to the old RHS
  HIP_TRY(hipEventRecord(b->ev0, s));
  HIP_TRY(hipMemcpyAsync(b->Y, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, s));
  for (int j = 0; j + 1 < b->nt; ++j) {
    int rc = qt_panel(b, j, s);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(b->ev1, s));
  HIP_TRY(hipEventSynchronize(b->ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  b->rhs_ms = ms;
  b->nrhs = nrhs;
  return 0;
}

int gpmi_band_get(gpmi_band* b, double* B_out, int64_t ld) {
  if (!b) return set_error(-1006, "null handle");
  DeviceGuard g(b->device);
  const int64_t np = b->n_pad, n = b->n;
  std::vector<double> h((size_t)np * np);
  HIP_TRY(hipMemcpyAsync(h.data(), b->Ab, sizeof(double) * h.size(), hipMemcpyDeviceToHost,
                        b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j) {
      const int64_t hi = std::max(i, j), lo = std::min(i, j);
      B_out[i * ld + j] = (hi - lo <= TS) ? h[(size_t)hi * np + lo] : 0.0;
    }
  return 0;
}

// ---------------------------------------------------------------------------
// Read-backs of what the stages left on the device (tests and diagnostics): each is
// a copy on the handle's stream and a rearrangement on the host; none launches a
// kernel or changes what a later call computes.
// ---------------------------------------------------------------------------

int gpmi_band_get_reduction(gpmi_band* b, double* B_out, double* V_out, double* T_out,
                            int64_t ld) {
  if (!b) return set_error(-1006, "null handle");
  if (!B_out || !V_out || !T_out) return set_error(-1004, "null output");
  if (ld < b->n_pad) return set_error(-1003, "ld < n_pad");
  DeviceGuard g(b->device);
  const int64_t np = b->n_pad;
  const int nt = b->nt;
  std::vector<double> h((size_t)np * np);
  HIP_TRY(hipMemcpyAsync(h.data(), b->Ab, sizeof(double) * h.size(), hipMemcpyDeviceToHost,
                        b->stream));
  if (nt > 1)
    HIP_TRY(hipMemcpyAsync(T_out, b->red.Tm, sizeof(double) * (size_t)(nt - 1) * TS * TS,
                          hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int64_t i = 0; i < np; ++i)
    for (int64_t j = 0; j < np; ++j) {
      const int64_t hi = std::max(i, j), lo = std::min(i, j);
      B_out[i * ld + j] = (hi - lo <= TS) ? h[(size_t)hi * np + lo] : 0.0;
      V_out[i * ld + j] = 0.0;
    }
  // panel j: rows from 128 (j + 1), columns [128 j, +128), unit lower trapezoidal
  for (int j = 0; j + 1 < nt; ++j) {
    const int64_t r0 = (int64_t)(j + 1) * TS, c0 = (int64_t)j * TS;
    for (int64_t i = 0; r0 + i < np; ++i)
      for (int64_t q = 0; q < TS && q <= i; ++q)
        V_out[(r0 + i) * ld + c0 + q] = (i == q) ? 1.0 : h[(size_t)(r0 + i) * np + c0 + q];
  }
  return 0;
}

int gpmi_band_get_rhs(gpmi_band* b, double* Y_out, int64_t ld) {
  if (!b) return set_error(-1006, "null handle");
  if (!Y_out) return set_error(-1004, "null output");
  if (b->nrhs <= 0) return set_error(-1204, "no right-hand side is resident");
  if (ld < b->nrhs) return set_error(-1003, "ld < nrhs");
  DeviceGuard g(b->device);
  std::vector<double> h((size_t)b->n_pad * RLD);
  HIP_TRY(hipMemcpyAsync(h.data(), b->Y, sizeof(double) * h.size(), hipMemcpyDeviceToHost,
                        b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int64_t i = 0; i < b->n_pad; ++i)
    for (int c = 0; c < b->nrhs; ++c) Y_out[i * ld + c] = h[(size_t)i * RLD + c];
  return 0;
}

int gpmi_band_get_solution(gpmi_band* b, int slot, double* X_out, int64_t ld) {
  if (!b) return set_error(-1006, "null handle");
  if (!X_out) return set_error(-1004, "null output");
  const BandEval& ev = b->eval;
  if (ev.sol_path == 0 || b->nrhs <= 0)
    return set_error(-1204, "no solution: gpmi_band_der_terms has not run on this band and RHS");
  if (slot < 0 || slot >= ev.sol_neta)
    return set_error(-1205, "slot outside the last gpmi_band_der_terms call");
  if (ev.sol_info[(size_t)slot] != 0) return set_error(-1206, "that eta's factorization failed");
  if (ld < b->nrhs) return set_error(-1003, "ld < nrhs");
  DeviceGuard g(b->device);
  const int64_t sZ = ev.plan.sZ;
  const double* src = (ev.sol_path == 1 ? static_cast<const double*>(ev.der.ysol) : static_cast<const double*>(ev.bcr.X)) + (int64_t)slot * sZ;
  std::vector<double> h((size_t)sZ);
  HIP_TRY(hipMemcpyAsync(h.data(), src, sizeof(double) * h.size(), hipMemcpyDeviceToHost,
                        b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int64_t i = 0; i < b->n_pad; ++i)
    for (int c = 0; c < b->nrhs; ++c) X_out[i * ld + c] = h[(size_t)i * RLD + c];
  return 0;
}

int gpmi_band_get_sinv(gpmi_band* b, int slot, int tangent, double* Zd_out, double* Zo_out) {
  if (!b) return set_error(-1006, "null handle");
  if (!Zd_out || !Zo_out) return set_error(-1004, "null output");
  const BandEval& ev = b->eval;
  if (ev.sinv_neta == 0) return set_error(-1204, "no selected inversion has run on this band");
  if (tangent && !ev.sinv_tan)
    return set_error(-1204, "the last selected inversion carried no tangent (exponent 2)");
  if (slot < 0 || slot >= ev.sinv_neta)
    return set_error(-1205, "slot outside the last selected-inversion call");
  DeviceGuard g(b->device);
  const int nt = b->nt;
  const size_t blk = (size_t)TS * TS;
  const double* zd = (tangent ? static_cast<const double*>(ev.tan.Zd) : static_cast<const double*>(ev.sinv.Zd)) + (int64_t)slot * ev.plan.sL;
  const double* zo = (tangent ? static_cast<const double*>(ev.tan.Zo) : static_cast<const double*>(ev.sinv.Zo)) + (int64_t)slot * ev.plan.sW;
  HIP_TRY(hipMemcpyAsync(Zd_out, zd, sizeof(double) * nt * blk, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipMemcpyAsync(Zo_out, zo, sizeof(double) * 2 * nt * blk, hipMemcpyDeviceToHost,
                        b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  // slots no kernel writes: the root's (block 0), and the right one of a level's last
  // block when that block is odd there
  for (int o = 0; o < nt; ++o) {
    int lvl = 0, m = nt;
    if (o > 0)
      for (; !((o >> lvl) & 1); ++lvl) m = (m + 1) >> 1;
    const int p = o >> lvl;
    for (int side = 0; side < 2; ++side)
      if (o == 0 || (side == 1 && p + 1 >= m))
        std::fill_n(Zo_out + ((size_t)o * 2 + side) * blk, blk, 0.0);
  }
  return 0;
}

int gpmi_band_get_tridiagonal(gpmi_band* b, double* d_out, double* e2_out) {
  if (!b) return set_error(-1006, "null handle");
  if (!d_out || !e2_out) return set_error(-1004, "null output");
  if (!b->eig.td_valid) return set_error(-1204, "gpmi_band_eigenvalues has not run on this band");
  DeviceGuard g(b->device);
  const int64_t np = b->n_pad, n = b->n;
  HIP_TRY(hipMemcpyAsync(d_out, b->eig.td, sizeof(double) * n, hipMemcpyDeviceToHost, b->stream));
  if (n > 1)
    HIP_TRY(hipMemcpyAsync(e2_out, b->eig.td + np, sizeof(double) * (n - 1), hipMemcpyDeviceToHost,
                          b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int gpmi_band_last_timing(gpmi_band* b, double* reduce_ms, double* rhs_ms, double* loglik_ms) {
  if (!b) return set_error(-1006, "null handle");
  if (std::getenv("GPMI_BAND_TRACE")) fprintf(stderr, "[gpmi band] eigenvalues %.3f ms\n", b->eig.eig_ms);
  if (reduce_ms) *reduce_ms = b->reduce_ms;
  if (rhs_ms) *rhs_ms = b->rhs_ms;
  if (loglik_ms) *loglik_ms = b->loglik_ms;
  return 0;
}

int gpmi_band_chase_info(gpmi_band* b, int* systolic, int* fallbacks, int* maxg) {
  if (!b) return set_error(-1006, "null handle");
  if (systolic) *systolic = b->eig.chase_systolic;
  if (fallbacks) *fallbacks = b->eig.chase_fallbacks;
  if (maxg) *maxg = b->eig.chase_maxg;
  return 0;
}

int gpmi_band_cq_stats(gpmi_band* b, int* panel_mode, int* cq_fallbacks,
                       int* cq_panel_fallbacks) {
  if (!b) return set_error(-1006, "null handle");
  if (panel_mode) *panel_mode = b->red.panel_mode;
  if (cq_fallbacks) *cq_fallbacks = b->red.cq_fallbacks;
  if (cq_panel_fallbacks) *cq_panel_fallbacks = b->red.cq_panel_fallbacks;
  return 0;
}

int gpmi_band_stats(gpmi_band* b, int* panel_fallbacks, int* panel_maxg) {
  if (!b) return set_error(-1006, "null handle");
  if (panel_fallbacks) *panel_fallbacks = b->red.panel_fallbacks;
  if (panel_maxg) *panel_maxg = b->red.panel_maxg;
  return 0;
}

int gpmi_band_sinv_ms(gpmi_band* b, double* ms) {
  if (!b || !ms) return set_error(-1006, "null handle");
  *ms = b->eval.sinv_ms;
  return 0;
}

int gpmi_band_der_ms(gpmi_band* b, double* der_ms) {
  if (!b) return set_error(-1006, "null handle");
  if (der_ms) *der_ms = b->eval.der_ms;
  return 0;
}

}  // extern "C"
