// Reduction of the band path: an operator's K to symmetric band form (bandwidth 128)
// on the device, panel by panel on three streams, with Q^T applied to a resident RHS
// block beside it (kernels: gpmi_band.hip, gpmi_cholqr.hip).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpmi_band_host.h"

using namespace gpmi;

namespace gpmi {

int qt_panel(gpmi_band* b, int j, hipStream_t st) {
  BandReduce& r = b->red;
  const int64_t np = b->n_pad;
  const int64_t r0 = (int64_t)(j + 1) * TS, c0 = (int64_t)j * TS;
  const int m = (int)(np - r0);
  const int G = (m + QT_ROWS - 1) / QT_ROWS;
  const double* P = b->Ab + r0 * np + c0;
  double* Yr = b->Y + r0 * RLD;
  hipLaunchKernelGGL(qt_partial_kernel, dim3(G), dim3(256), 0, st, P, np, m, Yr, r.qtp);
  LAUNCH_CHECK("qt_partial_kernel");
  hipLaunchKernelGGL(qt_reduce_kernel, dim3(TS * RLD / 256), dim3(256), 0, st, r.qtp, G, r.qa);
  LAUNCH_CHECK("qt_reduce_kernel");
  hipLaunchKernelGGL(qt_tb_kernel, dim3(1), dim3(256), 0, st, r.qa, r.Tm + (int64_t)j * TS * TS,
                     r.qb);
  LAUNCH_CHECK("qt_tb_kernel");
  hipLaunchKernelGGL(qt_apply_kernel, dim3(G), dim3(256), 0, st, P, np, m, Yr, r.qb);
  LAUNCH_CHECK("qt_apply_kernel");
  return 0;
}

namespace {

// CholeskyQR panel j (gpmi_cholqr.hip): shifted CholeskyQR3 of the m x 128 panel,
// then Householder reconstruction into V (the panel below its top block), tau and
// S R (the top block). A failure sets the panel's flag [4] before anything is written
// to the panel, and the guarded Householder panel factors it instead.
int cq_guard(gpmi_band* b, int j, hipStream_t st);

// guard: launch the guarded Householder panel right behind the chain (false: the
// caller launches it, cq_guard, where every CU is free again)
int cq_panel(gpmi_band* b, int j, hipStream_t st, bool guard = true) {
  BandReduce& r = b->red;
  const int64_t np = b->n_pad;
  const int64_t r0 = (int64_t)(j + 1) * TS, c0 = (int64_t)j * TS;
  const int m = (int)(np - r0);
  const int mt = m / TS;
  double* P = b->Ab + r0 * np + c0;
  const double coef = 11.0 * ((double)m * TS + (double)TS * (TS + 1)) * 1.1102230246251565e-16;
  const int64_t pt = (int64_t)j * 3 * TS * TS;   // this panel's factor slots
  int* fl = r.cqflag + 8 * j;
  // Gram partials of P (64-row tiles), then per pass: reduce -> factor -> apply
  // (+ the next Gram)
  const int rt = m / 64;
  hipLaunchKernelGGL(cq_gram_kernel, dim3(rt), dim3(256), CQ_DYN_LDS, st, P, np, r.cqpart);
  LAUNCH_CHECK("cq_gram_kernel");
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(cq_reduce_kernel, dim3(CQ_GPK / 64), dim3(256), 0, st, r.cqpart, rt,
                       r.cqG);
    LAUNCH_CHECK("cq_reduce_kernel");
    double* L = r.cqL + pt + (int64_t)pass * TS * TS;
    double* Li = r.cqLinv + pt + (int64_t)pass * TS * TS;
    hipLaunchKernelGGL(cq_chol_kernel, dim3(1), dim3(256), 0, st, r.cqG, pass, coef,
                       r.cq_fo[pass], L, Li, fl, fl + 4, r.ctr);
    LAUNCH_CHECK("cq_chol_kernel");
    const double* src = pass == 0 ? P : r.Qb;
    hipLaunchKernelGGL(cq_apply_kernel, dim3(rt), dim3(256), CQ_DYN_LDS, st, src,
                       pass == 0 ? np : (int64_t)TS, r.Qb, (int64_t)TS, Li, r.cqpart,
                       nullptr);
    LAUNCH_CHECK("cq_apply_kernel");
  }
  hipLaunchKernelGGL(cq_reduce_kernel, dim3(CQ_GPK / 64), dim3(256), 0, st, r.cqpart, rt,
                     r.cqG);
  LAUNCH_CHECK("cq_reduce_kernel");
  // third factor, reconstruction: V1 into P, tau, S, C = U^-T M3
  hipLaunchKernelGGL(cq_recon_kernel, dim3(1), dim3(256), 0, st, r.Qb, r.cqG, r.cq_fo[2], P,
                     np, r.cqS + (int64_t)j * TS, r.tau + (int64_t)j * TS,
                     r.cqL + pt + 2 * TS * TS, r.cqLinv + pt + 2 * TS * TS, r.cqMinv, fl,
                     fl + 4, r.cqUS + (int64_t)j * TS * TS);
  LAUNCH_CHECK("cq_recon_kernel");
  // T = -U S V1^-T on the side stream beside the rest of the chain (exits when the
  // panel failed); the side stream's later work for this panel is behind it
  HIP_TRY(hipEventRecord(r.ev_rc, st));
  HIP_TRY(hipStreamWaitEvent(b->side, r.ev_rc, 0));
  hipLaunchKernelGGL(cq_t_kernel, dim3(1), dim3(256), 0, b->side, P, np,
                     r.cqUS + (int64_t)j * TS * TS, r.cqW + (int64_t)j * TS * TS,
                     r.Tm + (int64_t)j * TS * TS, fl + 4);
  LAUNCH_CHECK("cq_t_kernel");
  r.t_from_q[j] = 1;
  // V2 = Q2 C^T below the top block
  if (mt > 1) {
    hipLaunchKernelGGL(cq_apply_kernel, dim3(rt - 2), dim3(256), CQ_DYN_LDS, st, r.Qb + TS * TS,
                       (int64_t)TS, P + TS * np, np, r.cqMinv, nullptr, fl + 4);
    LAUNCH_CHECK("cq_apply_kernel");
  }
  return guard ? cq_guard(b, j, st) : 0;
}

// A failed CholeskyQR panel j (flag fl[4], P untouched) by the Householder panel in
// one launch, guarded on the device (it exits at once when the flag is clear); past
// that launch's size (G > panel_maxg workgroups cannot all be co-resident) the host
// reads the flag after the chain and, only for a failed panel, runs the per-column
// Householder launches on the same stream: that panel alone falls back, the
// reduction goes on (one host round trip per such panel). The guarded launch needs
// its G workgroups co-resident, so it runs where no SYR2K holds CUs.
int cq_guard(gpmi_band* b, int j, hipStream_t st) {
  BandReduce& r = b->red;
  const int64_t np = b->n_pad;
  const int64_t r0 = (int64_t)(j + 1) * TS, c0 = (int64_t)j * TS;
  const int m = (int)(np - r0);
  double* P = b->Ab + r0 * np + c0;
  int* fl = r.cqflag + 8 * j;
  const int G = (m + HH_ROWS - 1) / HH_ROWS;
  if (G <= r.panel_maxg) {
    // (it also copies the panel's reflectors into U, vcopy_kernel's work)
    hipLaunchKernelGGL(hh_panel_kernel, dim3(G), dim3(HH_THREADS), HH_PANEL_LDS, st, P, np, m,
                       r.part, r.pivrow, r.ctr, r.tau + (int64_t)j * TS, r.err,
                       r.spin_limit, fl + 4, r.U + r0 * BAND_ULD, (int64_t)BAND_ULD);
    LAUNCH_CHECK("hh_panel_kernel");
    r.v_in_u[j] = 1;
  } else {
    int failed = 0;
    HIP_TRY(hipMemcpyAsync(&failed, fl + 4, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ++r.cq_host_checks;
    if (failed) {
      for (int c = -1; c < TS; ++c) {
        hipLaunchKernelGGL(hh_col_kernel, dim3(G), dim3(HH_THREADS), 0, st, P, np, m, c, r.part,
                           r.pivrow, r.tau + (int64_t)j * TS);
        LAUNCH_CHECK("hh_col_kernel");
      }
    }
  }
  return 0;
}

// Panel j (columns [128 j, +128), rows from 128 (j + 1)) on st. mode 0: CholeskyQR;
// 1: Householder, one launch per panel where its workgroups fit; 2: Householder,
// one launch per column.
int panel_qr(gpmi_band* b, int j, hipStream_t st, int mode, bool* guard_deferred = nullptr) {
  BandReduce& r = b->red;
  const int64_t np = b->n_pad;
  const int64_t r0 = (int64_t)(j + 1) * TS, c0 = (int64_t)j * TS;
  if (guard_deferred) *guard_deferred = false;
  // a last panel with fewer than 128 real rows (ragged n: the rest is the zero
  // pad) has rank < 128, which CholeskyQR cannot orthonormalise: Householder
  if (mode == 0 && b->n - r0 >= TS) {
    if (guard_deferred) *guard_deferred = true;
    return cq_panel(b, j, st, guard_deferred == nullptr);
  }
  if (mode == 0) mode = 1;
  const int m = (int)(np - r0);
  const int G = (m + HH_ROWS - 1) / HH_ROWS;
  double* P = b->Ab + r0 * np + c0;
  double* tau = r.tau + (int64_t)j * TS;
  if (mode == 1 && G <= r.panel_maxg) {
    // one launch per panel (rows in registers, in-launch reductions)
    HIP_TRY(hipMemsetAsync(r.ctr, 0, 512, st));
    hipLaunchKernelGGL(hh_panel_kernel, dim3(G), dim3(HH_THREADS), HH_PANEL_LDS, st, P, np, m,
                       r.part, r.pivrow, r.ctr, tau, r.err, r.spin_limit, nullptr, nullptr,
                       (int64_t)0);
    LAUNCH_CHECK("hh_panel_kernel");
  } else {
    for (int c = -1; c < TS; ++c) {
      hipLaunchKernelGGL(hh_col_kernel, dim3(G), dim3(HH_THREADS), 0, st, P, np, m, c, r.part,
                         r.pivrow, tau);
      LAUNCH_CHECK("hh_col_kernel");
    }
  }
  return 0;
}

// Dense -> band: panels j = 0 .. nt-2 of 128 columns (see gpmi_band.hip).
// With yh (the packed RHS), Y = Q^T R is applied panel by panel on the side
// stream as soon as each panel's T exists, beside the rest of the reduction.
// mode: the panel algorithm (panel_qr); mode 2 runs without look-ahead.
int band_reduce_pass(gpmi_band* b, const double* K, const std::vector<double>* yh, int mode) {
  BandReduce& r = b->red;
  hipStream_t s = b->stream;
  const int64_t np = b->n_pad;
  const int nt = b->nt;
  HIP_TRY(hipMemsetAsync(r.err, 0, 16, s));
  if (mode == 0) HIP_TRY(hipMemsetAsync(r.cqflag, 0, sizeof(int) * 8 * nt, s));
  HIP_TRY(hipEventRecord(b->ev0, s));
  const auto host_t0 = std::chrono::steady_clock::now();
  if (yh) {
    HIP_TRY(hipMemcpyAsync(b->Y, yh->data(), sizeof(double) * yh->size(), hipMemcpyHostToDevice,
                          b->side));
  }
  std::fill(r.t_from_q.begin(), r.t_from_q.end(), 0);
  std::fill(r.v_in_u.begin(), r.v_in_u.end(), 0);
  const bool la = mode != 2 && r.lookahead && r.s_pan;
  // The pipelined CholeskyQR form copies only tile column 0 of K into the working matrix:
  // the first panel's SYMM reads A22 from K, and its update (the tile column and the
  // pipelined SYR2K) reads its C tiles from K and writes them to Ab, which holds the
  // lower triangle from then on (the upper one is never read). 2 GB -> 16 MB at N = 16384
  // (the copy took 0.8 ms). Every other form copies all of K.
  const bool k_first = mode == 0 && la && nt > 2;
  if (k_first && r.poison)   // (tests: NaN wherever the reduction would read unwritten Ab)
    HIP_TRY(hipMemsetAsync(b->Ab, 0xff, sizeof(double) * np * np, s));
  if (k_first)
    HIP_TRY(hipMemcpy2DAsync(b->Ab, sizeof(double) * np, K, sizeof(double) * np,
                            sizeof(double) * TS, np, hipMemcpyDeviceToDevice, s));
  else
    HIP_TRY(hipMemcpyAsync(b->Ab, K, sizeof(double) * np * np, hipMemcpyDeviceToDevice, s));
  bool ahead = false;   // panel j already factored by the previous look-ahead
  for (int j = 0; j + 1 < nt; ++j) {
    const int64_t r0 = (int64_t)(j + 1) * TS, c0 = (int64_t)j * TS;
    const int m = (int)(np - r0), mt = nt - j - 1;
    double* P = b->Ab + r0 * np + c0;
    double* tau = r.tau + (int64_t)j * TS;
    double* T = r.Tm + (int64_t)j * TS * TS;
    if (!ahead) {
      int rc = panel_qr(b, j, s, mode);
      if (rc) return rc;
    }
    ahead = false;
    double* Ur = r.U + r0 * BAND_ULD;
    if (!r.v_in_u[j]) {   // (the guarded Householder panel copied them already)
      hipLaunchKernelGGL(vcopy_kernel, dim3((unsigned)((int64_t)m * TS / 256)), dim3(256), 0, s,
                         P, np, m, Ur, (int64_t)BAND_ULD);
      LAUNCH_CHECK("vcopy_kernel");
    }
    const int nch = (m + TN_CH - 1) / TN_CH;
    // T from V^T V on the side stream, beside the SYMM (which needs only V)
    HIP_TRY(hipEventRecord(r.ev_v, s));
    HIP_TRY(hipStreamWaitEvent(b->side, r.ev_v, 0));
    if (r.t_from_q[j]) {
      // a CholeskyQR panel's T came from cq_t_kernel; only if it fell back does this
      // one-workgroup launch form it (it exits at once otherwise)
      hipLaunchKernelGGL(t_fallback_kernel, dim3(1), dim3(256), 0, b->side, Ur + TS,
                         (int64_t)BAND_ULD, m, tau, r.VtV, T, r.cqflag + 8 * j + 4);
      LAUNCH_CHECK("t_fallback_kernel");
    } else {
      hipLaunchKernelGGL(tn_partial_kernel, dim3(nch), dim3(256), 0, b->side, Ur + TS,
                         (int64_t)BAND_ULD, Ur + TS, (int64_t)BAND_ULD, m, r.tnp2, nullptr);
      LAUNCH_CHECK("tn_partial_kernel");
      hipLaunchKernelGGL(tn_reduce_kernel, dim3(TS * TS / 64), dim3(256), 0, b->side, r.tnp2,
                         nch, r.VtV, 1.0, nullptr);
      LAUNCH_CHECK("tn_reduce_kernel");
      hipLaunchKernelGGL(tbuild_kernel, dim3(1), dim3(256), 0, b->side, r.VtV, tau, T, nullptr);
      LAUNCH_CHECK("tbuild_kernel");
    }
    r.t_from_q[j] = 0;
    HIP_TRY(hipEventRecord(r.ev_t, b->side));
    if (yh) {
      // Q_j^T on the side stream right after T_j (a stream of its own measured the
      // same, and a fourth stream of the reduction costs more elsewhere: DESIGN 5)
      int rc = qt_panel(b, j, b->side);
      if (rc) return rc;
    }
    const int chunk = symm_chunk(mt, 2 * b->ncu);
    const int sch = (mt + chunk - 1) / chunk;
    const double* ksrc = (k_first && j == 0) ? K : nullptr;   // panel 0: C and A22 from K
    hipLaunchKernelGGL(symm_kernel, dim3(mt, sch), dim3(256), 0, s, ksrc ? ksrc : b->Ab, np,
                       r.U, (int64_t)BAND_ULD, j + 1, mt, chunk, r.Xp);
    LAUNCH_CHECK("symm_kernel");
    hipLaunchKernelGGL(psum_kernel, dim3(TS * TS / 512, mt), dim3(256), 0, s, r.Xp, sch, r.X);
    LAUNCH_CHECK("psum_kernel");
    HIP_TRY(hipStreamWaitEvent(s, r.ev_t, 0));
    // the serial 128^3 steps on quadrant workgroups (gemm_quad2, gpmi_tile.h; one
    // launch summing the split-K partials and forming X T per half tile instead:
    // slower, 139.0 against 138.2 ms, its 34-234 workgroups each read 1/2 of a row
    // tile's partials)
    hipLaunchKernelGGL(xt_q_kernel, dim3(mt, 4), dim3(256), 0, s, r.X, T, r.X2);
    LAUNCH_CHECK("xt_q_kernel");
    hipLaunchKernelGGL(tn_partial_q_kernel, dim3(nch, 4), dim3(256), 0, s, Ur + TS,
                       (int64_t)BAND_ULD, r.X2, (int64_t)TS, m, r.tnp);
    LAUNCH_CHECK("tn_partial_q_kernel");
    hipLaunchKernelGGL(tn_reduce_kernel, dim3(TS * TS / 64), dim3(256), 0, s, r.tnp, nch, r.M,
                       1.0, nullptr);
    LAUNCH_CHECK("tn_reduce_kernel");
    hipLaunchKernelGGL(z_q_kernel, dim3(4), dim3(256), 0, s, T, r.M, r.Zh);
    LAUNCH_CHECK("z_q_kernel");
    hipLaunchKernelGGL(w_q_kernel, dim3(mt, 4), dim3(256), 0, s, r.X2, Ur, (int64_t)BAND_ULD,
                       r.Zh);
    LAUNCH_CHECK("w_q_kernel");
    const int next_g = (int)((np - r0 - TS + HH_ROWS - 1) / HH_ROWS);   // panel j + 1's grid
    if (la && j + 2 < nt && (mode == 0 || next_g <= r.panel_maxg)) {
      // tile column 0 of the update (panel j + 1's columns) first; then that
      // panel's QR beside the rest of the update on a grid capped to la_grid
      // workgroups, so that the panel's workgroups find free CUs
      hipLaunchKernelGGL(syr2k_col_q_kernel, dim3(mt, 4), dim3(256), 0, s, b->Ab, np, r.U,
                         (int64_t)BAND_ULD, j + 1, ksrc);
      LAUNCH_CHECK("syr2k_col_q_kernel");
      HIP_TRY(hipEventRecord(r.ev_col, s));
      HIP_TRY(hipStreamWaitEvent(r.s_pan, r.ev_col, 0));
      const bool pipe = mode == 0;
      const int rest = (mt - 1) * mt / 2;
      const int la_free = mt < r.la_late_mt ? r.la_free_late : r.la_free;
      const int nmain = std::min(rest, std::max(1, b->ncu - la_free));
      int* tcnt = pipe ? r.cqflag + 8 * j + 6 : nullptr;
      // The rest of the update on s_pan, panel j + 1's QR on s right behind the tile
      // column it needs (round 5: the chain used to run on s_pan between two cross-stream
      // waits, ~12 us before it and ~10 us after it on every chain-bound late panel)
      if (pipe) {
        // one SYR2K workgroup per CU on all but la_free CUs, which the chain (its
        // single-workgroup kernels need a whole CU) has to itself
        hipLaunchKernelGGL(syr2k_pipe_kernel, dim3(nmain), dim3(256), 0, r.s_pan, b->Ab, np,
                           r.U, (int64_t)BAND_ULD, j + 1, mt, tcnt, nmain, 0, ksrc);
        LAUNCH_CHECK("syr2k_pipe_kernel");
      } else {
        // the Householder panel (its workgroups must be co-resident) beside a capped
        // grid; la_grid 0: leave exactly the panel's workgroup count of CUs free
        // (measured: slower than a fixed 128-workgroup cap at N = 16384, 302 vs 262 ms)
        const int cap = r.la_grid > 0 ? r.la_grid : std::max(64, b->ncu - next_g);
        hipLaunchKernelGGL(syr2k_rest_kernel, dim3(std::min(rest, cap)), dim3(256), 0, r.s_pan,
                           b->Ab, np, r.U, (int64_t)BAND_ULD, j + 1,
                           mt, r.rorder ? r.rorder + r.rorder_off[mt - 1] : nullptr);
        LAUNCH_CHECK("syr2k_rest_kernel");
      }
      HIP_TRY(hipEventRecord(r.ev_pan, r.s_pan));
      bool guard = false;
      int rc = panel_qr(b, j + 1, s, mode, pipe ? &guard : nullptr);
      if (rc) return rc;
      if (tcnt && rest > nmain) {
        // the chain's CUs join the update once the chain ends (tickets of tcnt;
        // 139.2 against 141.0 ms at N = 16384; launched only from panels whose
        // update outlasts the chain: no difference)
        hipLaunchKernelGGL(syr2k_pipe_kernel, dim3(std::min(la_free, rest - nmain)), dim3(256),
                           0, s, b->Ab, np, r.U, (int64_t)BAND_ULD, j + 1, mt, tcnt, nmain, 1,
                           ksrc);
        LAUNCH_CHECK("syr2k_pipe_kernel");
      }
      HIP_TRY(hipStreamWaitEvent(s, r.ev_pan, 0));
      if (guard) {
        // the guarded Householder panel behind the SYR2K (its workgroups must be
        // co-resident: every CU is free again here)
        rc = cq_guard(b, j + 1, s);
        if (rc) return rc;
      }
      ahead = true;
    } else {
      const int tiles = mt * (mt + 1) / 2;
      hipLaunchKernelGGL(syr2k_kernel, dim3(tiles), dim3(256), 0, s, b->Ab, np, r.U,
                         (int64_t)BAND_ULD, j + 1, mt);
      LAUNCH_CHECK("syr2k_kernel");
    }
  }
  if (yh) {
    HIP_TRY(hipEventRecord(r.ev_q, b->side));
    HIP_TRY(hipStreamWaitEvent(s, r.ev_q, 0));
  }
  if (mode == 0 && nt > 1) {
    // R (the band's subdiagonal blocks) of every CholeskyQR panel
    hipLaunchKernelGGL(cq_top_kernel, dim3(nt - 1), dim3(256), 0, s, r.cqL, r.cqLinv, r.cqflag,
                       r.cqS, r.cqscr, b->Ab, np);
    LAUNCH_CHECK("cq_top_kernel");
  }
  HIP_TRY(hipEventRecord(b->ev1, s));
  // host time to enqueue the whole reduction (GPMI_BAND_TRACE: against its device time,
  // printed below; a device span not far above it would mean the host's launches bound it)
  const double host_enqueue_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
  int herr = 0;
  std::vector<int> hflag(mode == 0 ? 8 * nt : 0);
  HIP_TRY(hipMemcpyAsync(&herr, r.err, sizeof(int), hipMemcpyDeviceToHost, s));
  if (mode == 0)
    HIP_TRY(hipMemcpyAsync(hflag.data(), r.cqflag, sizeof(int) * hflag.size(),
                          hipMemcpyDeviceToHost, s));
  HIP_TRY(hipEventSynchronize(b->ev1));
  HIP_TRY(hipStreamSynchronize(s));
  if (herr) return set_error(-1201, "band reduction: panel hand-off timed out (workgroups not co-resident?)");
  if (mode == 0) {
    // failed CholeskyQR panels, each refactored in place during the pass (cq_panel)
    for (int j = 0; j + 1 < nt; ++j)
      if (hflag[8 * j + 4]) ++r.cq_panel_fallbacks;
  }
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  b->reduce_ms = ms;
  if (std::getenv("GPMI_BAND_TRACE"))
    fprintf(stderr, "[gpmi band] reduction %.3f ms on the device, enqueued in %.3f ms\n", ms,
            host_enqueue_ms);
  return 0;
}

}  // namespace

// The reduction with the single-launch panel QR; if a hand-off times out (its
// workgroups were not all resident, e.g. the GPU is shared or partitioned), the
// whole reduction is redone from K with the per-column panel launches.
// CholeskyQR panels first (unless GPMI_BAND_PANEL=hh); if one of them reports a
// breakdown (a numerically rank-deficient panel) the reduction is redone with
// Householder panels.
int band_reduce(gpmi_band* b, const double* K, const std::vector<double>* yh) {
  BandReduce& r = b->red;
  int rc;
  // a new band: what the evaluator and the chase left belongs to the old one
  b->eval.sol_path = 0;
  b->eval.sol_neta = 0;
  b->eval.sinv_neta = 0;
  b->eval.sinv_tan = false;
  b->eig.td_valid = false;
  if (r.panel_mode == 0) {
    // a failed CholeskyQR panel is refactored in place (cq_panel); only a timed-out
    // guarded Householder panel (its workgroups not co-resident on a shared GPU)
    // sends the reduction back, straight to the per-column launches
    rc = band_reduce_pass(b, K, yh, 0);
    if (rc != -1201) return rc;
    ++r.cq_fallbacks;
    ++r.panel_fallbacks;
    return band_reduce_pass(b, K, yh, 2);
  }
  rc = band_reduce_pass(b, K, yh, 1);
  if (rc != -1201) return rc;
  ++r.panel_fallbacks;
  return band_reduce_pass(b, K, yh, 2);
}

}  // namespace gpmi
