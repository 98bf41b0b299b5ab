// The dense operator's blocked Cholesky (include/gpmi.h, gpmi_op.h): the schedule of a
// batched factorization of K + eta_b I (launch list: gpmi_dense_plan.h; kernels in
// gpmi_chol.hip, gpmi_diag.hip), its HIP-event timing, the cached single-eta factor,
// and the entry points that consume a factor: loglik_batch, logdet, solve, traceinv
// (kernels in gpmi_trinv.hip), and the read-backs of L, W = L^-T and A^-1 (tests).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <map>
#include <vector>

#include "gpmi_op.h"

using namespace gpmi;

namespace {

// Lower-triangular tiles of a band (w tile columns over t tile rows) in row
// groups of G rows, column-major inside a group, packed (i << 16) | j. The
// 32 CUs x 2 workgroups in flight on one XCD then cover ~G rows x (64/G)
// columns, so each operand slab is re-read from that XCD's L2, not from the
// Infinity Cache / HBM.
void grouped_order(int w, int t, int G, std::vector<uint32_t>* out) {
  for (int r0 = 0; r0 < t; r0 += G) {
    const int r1 = std::min(t, r0 + G);
    const int jmax = std::min(r1 - 1, w - 1);
    for (int j = 0; j <= jmax; ++j)
      for (int i = std::max(r0, j); i < r1; ++i) out->push_back(((uint32_t)i << 16) | j);
  }
}

int launch_syrk(gpmi_op* op, hipStream_t st, int b0, int nb, int tc0, int w, int t, int p0,
                int kdim, bool from_k = false) {
  // b0: first batch member of the launch (a batch group's offset)
  const int tri = w * (w + 1) / 2;
  const int tiles = tri + (t - w) * w;
  if (tiles <= 0 || nb <= 0) return 0;
  int evi = -1;
  if (op->tim.on) {
    evi = (int)op->tim.syrk_log.size() * 2;
    HIP_TRY(op->tim.syrk.reserve(evi + 2, timing_event_flags()));
    HIP_TRY(hipEventRecord(op->tim.syrk[evi], st));
  }
  const uint32_t* order = nullptr;
  if (op->fac.order && w > 1) {
    auto it = op->fac.order_off.find({w, t});
    if (it != op->fac.order_off.end()) order = op->fac.order + it->second;
  }
  hipLaunchKernelGGL(op->kloop == KLOOP_LATE ? syrk_kernel<KLOOP_LATE> : syrk_kernel<KLOOP_EARLY>,
                     dim3(tiles, nb), dim3(256), 0, st,
                     op->fac.A + (int64_t)b0 * op->n_pad * op->n_pad, (int64_t)op->n_pad,
                     op->n_pad * op->n_pad, tc0, w, t, p0, kdim, order,
                     from_k ? (const double*)op->K : nullptr, op->fac.etas + b0, (int64_t)op->n);
  LAUNCH_CHECK("syrk_kernel");
  if (op->tim.on) {
    HIP_TRY(hipEventRecord(op->tim.syrk[evi + 1], st));
    // algorithmic flops: lower triangle only (diagonal tiles count 128*129/2 entries)
    const double offd = (double)(tiles - std::min(tiles, w)) * TS * TS;
    const double diag = (double)std::min(tiles, w) * TS * (TS + 1) / 2.0;
    const double fl = 2.0 * (offd + diag) * kdim * nb;
    op->tim.syrk_log.push_back({evi, fl});
    op->tim.syrk_shape.push_back({w, t, kdim});
  }
  return 0;
}

// One launch of an outer panel's factorization (gpmi_dense_plan.h): the diagonal-block
// kernel of a column (Cholesky, inverse, fused forward solve, logdet / Gram partials),
// then either the left-looking column kernel (column update, L_ik and r_i updates, next
// diagonal tile) or, in the recursive schedule, the panel kernel (L_ik and r_i updates).
int factor_panel(gpmi_op* op, const BatchPtrs& P, int nb, hipStream_t st,
                 const DenseLaunch& L) {
  const int64_t lda = op->n_pad;
  if (L.kind == DENSE_DIAG) {
    hipLaunchKernelGGL(diag_block_kernel, dim3(nb), dim3(256), 0, st, P, lda, L.col, op->nt);
    LAUNCH_CHECK("diag_block_kernel");
  } else if (L.kind == DENSE_PANEL) {
    hipLaunchKernelGGL(panel_kernel, dim3(L.r1 - L.r0, nb), dim3(256), 0, st, P, lda, L.col);
    LAUNCH_CHECK("panel_kernel");
  } else {
    // (its events only under GPMI_SYRK_TRACE: the default timed run records none here)
    const bool ev = op->tim.on && op->tim.trace;
    size_t evi = op->tim.colpanel_used;
    if (ev) {
      HIP_TRY(op->tim.colpanel.reserve(evi + 2, timing_event_flags()));
      HIP_TRY(hipEventRecord(op->tim.colpanel[evi], st));
    }
    // block 0 is row tile col + 1, the one that goes on to the next diagonal tile
    hipLaunchKernelGGL(colpanel_kernel, dim3(L.r1 - L.r0, nb), dim3(256), 0, st, P, lda, L.col,
                       L.p0 / TS, L.next_diag ? 1 : 0);
    LAUNCH_CHECK("colpanel_kernel");
    if (ev) {
      HIP_TRY(hipEventRecord(op->tim.colpanel[evi + 1], st));
      op->tim.colpanel_used = evi + 2;
    }
  }
  return 0;
}

// The blocked factorization schedule over outer panels P_k of `outer` tile
// columns, in order on one stream: factor P_k (the recursive panel factorization, or
// left-looking by column under GPMI_PANEL=col), then
// one trailing SYRK over all columns right of it (kdim = 128 * outer). (Round 5
// removed the look-ahead form, the panel chain of P_{k+1} on a second high-priority
// stream beside the bulk update of P_k: at the batch-64 headline 1441.8 against
// 1442.9 ms per 64-eta step, and within +-1 % at 8 and 16 eta in round 3: the batched
// SYRK keeps every CU busy, so the chain beside it gains nothing.)
// P points at batch member b0 (a batch group); `main` replaces op->stream.
int schedule(gpmi_op* op, const BatchPtrs& P, int b0, int nb, hipStream_t main = nullptr) {
  hipStream_t A = main ? main : op->stream;
  for (const DenseLaunch& L : dense_plan(op->nt, op->outer, op->panel_mode)) {
    // SYRK: a band update of the recursive schedule, or the bulk trailing update; the
    // first bulk update reads its C tiles from K (run_factor copies only the first
    // outer panel's tile columns into the members)
    const int rc = L.kind == DENSE_SYRK
                       ? launch_syrk(op, A, b0, nb, L.col, L.w, L.r1 - L.r0, L.p0, L.kdim,
                                     L.from_k)
                       : factor_panel(op, P, nb, A, L);
    if (rc) return rc;
  }
  return 0;
}

// One grouped tile order per trailing-update shape (w, t) the schedule launches, in
// launch order; rebuilt when the schedule changes (gpmi_op_set_outer).
int ensure_order(gpmi_op* op) {
  DenseFactor& f = op->fac;
  if (f.group <= 0) return 0;
  if (f.order && f.order_nt == op->nt && f.order_outer == op->outer) return 0;
  f.order_nt = f.order_outer = -1;
  f.order_off.clear();
  std::vector<uint32_t> h;
  for (const DenseLaunch& L : dense_plan(op->nt, op->outer, op->panel_mode)) {
    const std::pair<int, int> wt(L.w, L.r1 - L.r0);
    if (L.kind != DENSE_SYRK || wt.first < 2 || f.order_off.count(wt)) continue;
    f.order_off[wt] = (int64_t)h.size();
    grouped_order(wt.first, wt.second, f.group, &h);
  }
  if (h.empty()) h.push_back(0);
  HIP_TRY(f.order.release());
  HIP_TRY(f.order.reserve(h.size()));
  HIP_TRY(hipMemcpy(f.order, h.data(), sizeof(uint32_t) * h.size(), hipMemcpyHostToDevice));
  f.order_nt = op->nt;
  f.order_outer = op->outer;
  return 0;
}

BatchPtrs shifted(const BatchPtrs& P, int b0) {
  BatchPtrs q = P;
  q.A += b0 * P.sA;
  q.R += b0 * P.sR;
  q.U += b0 * P.sU;
  q.Linv += b0 * P.sL;
  q.logdiag += b0 * P.sLD;
  q.gram += b0 * P.sG;
  q.info += b0;
  return q;
}

// Factor K + eta_b I for b < nb, with the fused forward substitution of the
// RHS block (copied from rhs_src). Results stay on the device.
int run_factor(gpmi_op* op, const double* etas_host, int nb, const double* rhs_dev) {
  if (!op->has_K) return set_errorf(-1000, "operator has no matrix (load or assemble first)");
  if (nb < 1 || nb > op->max_batch)
    return set_errorf(-1001, "batch %d outside [1, %d]", nb, op->max_batch);
  DeviceGuard g(op->device);
  hipStream_t s = op->stream;
  const int nt = op->nt;
  const int64_t lda = op->n_pad;
  BatchPtrs P = op->ptrs();
  int rc = ensure_order(op);
  if (rc) return rc;
  op->tim.syrk_log.clear();
  op->tim.syrk_shape.clear();
  op->tim.colpanel_used = 0;
  op->fac.cache_valid = false;
  op->fac.last_nb = 0;
  ++op->factor_gen;
  // slot 0 of R ends as L^-1 rhs_src only when that block is what is factored along
  op->pred.ry_gen = rhs_dev == op->rhs_src ? op->factor_gen : ~0ull;
  op->pred.ry_rhs = op->rhs_gen;
  if (op->tim.on) {
    HIP_TRY(op->tim.span.reserve(2, timing_event_flags()));
    HIP_TRY(hipEventRecord(op->tim.span[0], s));
  }
  HIP_TRY(hipMemcpyAsync(op->fac.etas, etas_host, sizeof(double) * nb, hipMemcpyHostToDevice, s));
  // K + eta_b I into the members' tile columns of the first outer panel only; the
  // rest is formed by the first trailing SYRK from K (schedule)
  const int wc = std::min(op->outer, nt);
  hipLaunchKernelGGL(shift_copy_kernel, dim3(wc * (wc + 1) / 2 + (nt - wc) * wc), dim3(256), 0,
                     s, op->K, lda, op->fac.A, lda, P.sA, op->fac.etas, nb, op->n, wc);
  LAUNCH_CHECK("shift_copy_kernel");
  for (int b = 0; b < nb; ++b)
    HIP_TRY(hipMemcpyAsync(op->fac.R + b * P.sR, rhs_dev, sizeof(double) * P.sR,
                           hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(op->fac.info, 0, sizeof(int) * nb, s));
  // auto: a small batch (the per-rank block of a strong-scaled curve) keeps more CUs
  // busy with its halves overlapped (batch 8: +2.3 %); a large one is all SYRK
  // already (batch 64: +0.2 %) and keeps one stream (clean per-launch timing)
  const int groups = op->groups ? op->groups : (nb <= 32 ? 2 : 1);
  if (groups == 2 && nb >= 2) {
    // two independent halves of the batch on two streams: one half's
    // latency-bound diagonal-block / panel kernels run beside the other's SYRK.
    // Only batched callers (nb >= 2) get here, and the one batched caller,
    // gpmi_op_loglik_batch, releases stream3 after its synchronisation
    // (the single-eta factor calls never create it)
    const int h = nb / 2;
    if (!op->fac.stream3)
      HIP_TRY(hipStreamCreateWithFlags(&op->fac.stream3.h, hipStreamNonBlocking));
    HIP_TRY(hipEventRecord(op->fac.ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(op->fac.stream3, op->fac.ev_fork, 0));
    if ((rc = schedule(op, P, 0, h, s))) return rc;
    if ((rc = schedule(op, shifted(P, h), h, nb - h, op->fac.stream3))) return rc;
    HIP_TRY(hipEventRecord(op->fac.ev_g, op->fac.stream3));
    HIP_TRY(hipStreamWaitEvent(s, op->fac.ev_g, 0));
  } else {
    rc = schedule(op, P, 0, nb);
  }
  if (rc) return rc;
  hipLaunchKernelGGL(finalize_kernel, dim3(nb), dim3(256), 0, s, P, nt, op->fac.out, OUT_LD);
  LAUNCH_CHECK("finalize_kernel");
  if (op->tim.on) HIP_TRY(hipEventRecord(op->tim.span[1], s));
  op->fac.last_nb = nb;
  return 0;
}

int collect_timing(gpmi_op* op) {
  if (!op->tim.on) return 0;
  HIP_TRY(hipEventSynchronize(op->tim.span[1]));
  double tot = 0.0, fl = 0.0;
  std::vector<std::pair<double, double>> iv;
  for (auto& pr : op->tim.syrk_log) {
    float ms = 0.f, t0 = 0.f, t1 = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, op->tim.syrk[pr.first], op->tim.syrk[pr.first + 1]));
    HIP_TRY(hipEventElapsedTime(&t0, op->tim.span[0], op->tim.syrk[pr.first]));
    HIP_TRY(hipEventElapsedTime(&t1, op->tim.span[0], op->tim.syrk[pr.first + 1]));
    iv.push_back({t0, t1});
    tot += ms;
    fl += pr.second;
  }
  if (op->tim.trace) {
    // dev aid: SYRK time by class (bulk trailing update w == t vs band w < t) and kdim,
    // then the colpanel_kernel launches' total
    std::map<std::pair<int, int>, std::array<double, 3>> cls;
    for (size_t i = 0; i < op->tim.syrk_log.size(); ++i) {
      const auto& sh = op->tim.syrk_shape[i];
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, op->tim.syrk[op->tim.syrk_log[i].first],
                                  op->tim.syrk[op->tim.syrk_log[i].first + 1]));
      auto& c = cls[{sh[0] == sh[1] ? 1 : 0, sh[2]}];
      c[0] += 1;
      c[1] += ms;
      c[2] += op->tim.syrk_log[i].second;
    }
    for (auto& kv : cls)
      fprintf(stderr, "[gpmi syrk] %s kdim=%4d launches=%3.0f ms=%8.3f TF/s=%6.2f\n",
              kv.first.first ? "bulk" : "band", kv.first.second, kv.second[0], kv.second[1],
              kv.second[2] / (kv.second[1] * 1e-3) / 1e12);
    double cp = 0.0;
    for (size_t i = 0; i + 1 < op->tim.colpanel_used; i += 2) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, op->tim.colpanel[i], op->tim.colpanel[i + 1]));
      cp += ms;
    }
    if (op->tim.colpanel_used)
      fprintf(stderr, "[gpmi syrk] colpanel_kernel launches=%3zu ms=%8.3f\n",
              op->tim.colpanel_used / 2, cp);
  }
  std::sort(iv.begin(), iv.end());
  double busy = 0.0, cs = -1.0, ce = -1.0;
  for (auto& x : iv) {
    if (x.first > ce) {
      if (ce > cs) busy += ce - cs;
      cs = x.first;
      ce = x.second;
    } else if (x.second > ce) {
      ce = x.second;
    }
  }
  if (ce > cs) busy += ce - cs;
  float all = 0.f;
  HIP_TRY(hipEventElapsedTime(&all, op->tim.span[0], op->tim.span[1]));
  op->tim.last_syrk_ms = tot;
  op->tim.last_syrk_busy_ms = busy;
  op->tim.last_syrk_flops = fl;
  op->tim.last_syrk_launches = (int)op->tim.syrk_log.size();
  op->tim.last_total_ms = all;
  return 0;
}

int ensure_factor(gpmi_op* op, double eta, const double* rhs_dev, bool* fresh) {
  *fresh = false;
  if (op->fac.cache_valid && op->fac.cached_eta == eta) return 0;
  int rc = run_factor(op, &eta, 1, rhs_dev);
  if (rc) return rc;
  op->fac.cache_valid = true;
  op->fac.cached_eta = eta;
  *fresh = true;
  return 0;
}

}  // namespace

namespace gpmi {

int factor_ready(gpmi_op* op, double eta, const double* rhs_dev, bool* fresh) {
  int rc = ensure_factor(op, eta, rhs_dev, fresh);
  if (rc) return rc;
  int inf = 0;
  HIP_TRY(hipMemcpyAsync(&inf, op->fac.info, sizeof(int), hipMemcpyDeviceToHost, op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  if (inf) {
    op->fac.cache_valid = false;
    return set_errorf(inf, "matrix K + eta I is not positive definite (pivot %d)", inf);
  }
  return 0;
}

int forward_substitute(gpmi_op* op, const BatchPtrs& P) {
  for (int kb = 0; kb < op->nt; ++kb) {
    hipLaunchKernelGGL(fwd_step_kernel, dim3(op->nt - kb, 1), dim3(256), 0, op->stream, P,
                       op->n_pad, kb);
    LAUNCH_CHECK("fwd_step_kernel");
  }
  return 0;
}

int traceinv_build_w(gpmi_op* op) {
  DenseTraceInv& ti = op->tinv;
  if (ti.gen != op->factor_gen) {
    ti.gen = op->factor_gen;
    ti.have = 0;
  }
  if (ti.have & 1) return 0;
  const int nt = op->nt;
  const int64_t np = op->n_pad;
  const int ntri = nt * (nt + 1) / 2;
  HIP_TRY(ti.W.reserve((size_t)np * np));
  HIP_TRY(ti.tpart.reserve((size_t)(ntri + nt * nt)));
  hipStream_t s = op->stream;
  double* p1 = ti.tpart + ntri;   // [nt][nt]: ||Y_kj||^2 at [k * nt + j]
  for (int kb = 0; kb < nt; kb += op->outer) {
    const int ke = std::min(nt, kb + op->outer);
    for (int k = kb; k < ke; ++k) {
      if (k > kb) {
        hipLaunchKernelGGL(trinv_update_kernel, dim3(k), dim3(256), 0, s, op->fac.A, np, ti.W,
                           np, k, k, kb, k);
        LAUNCH_CHECK("trinv_update_kernel");
      }
      hipLaunchKernelGGL(trinv_diag_kernel, dim3(k + 1), dim3(256), 0, s, op->fac.Linv, ti.W,
                         np, k, p1 + (int64_t)k * nt);
      LAUNCH_CHECK("trinv_diag_kernel");
    }
    if (ke < nt) {
      hipLaunchKernelGGL(trinv_update_kernel, dim3((nt - ke) * ke), dim3(256), 0, s, op->fac.A,
                         np, ti.W, np, ke, ke, kb, ke);
      LAUNCH_CHECK("trinv_update_kernel");
    }
  }
  std::vector<double> h((size_t)nt * nt);
  HIP_TRY(hipMemcpyAsync(h.data(), p1, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  double acc = 0.0;
  for (int k = 0; k < nt; ++k)
    for (int j = 0; j <= k; ++j) acc += h[(size_t)k * nt + j];
  // the identity pad contributes n_pad - n
  ti.value[0] = acc - (double)(np - op->n);
  ti.have |= 1;
  return 0;
}

int traceinv_build_ainv(gpmi_op* op) {
  DenseTraceInv& ti = op->tinv;
  if (ti.have & 2) return 0;
  const int nt = op->nt;
  const int64_t np = op->n_pad;
  HIP_TRY(ti.Td.reserve((size_t)nt * TS * TS));
  hipStream_t s = op->stream;
  // T = W W^T over k-panels of 4 tiles; panel [p0, p0 + kd) updates tile rows I < imax
  for (int p0 = 0; p0 < (int)np; p0 += 4 * TS) {
    const int kd = std::min<int>(4 * TS, (int)np - p0);
    const int imax = (p0 + kd) / TS;
    hipLaunchKernelGGL(gram_panel_kernel, dim3(imax * (imax + 1) / 2), dim3(256), 0, s,
                       ti.W, np, ti.Td, p0, kd, imax);
    LAUNCH_CHECK("gram_panel_kernel");
  }
  hipLaunchKernelGGL(gram_sumsq_kernel, dim3(nt), dim3(256), 0, s, ti.W, np, ti.Td,
                     ti.tpart);
  LAUNCH_CHECK("gram_sumsq_kernel");
  std::vector<double> h((size_t)nt);
  HIP_TRY(hipMemcpyAsync(h.data(), ti.tpart, sizeof(double) * h.size(),
                         hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  double acc = 0.0;
  for (int q = 0; q < nt; ++q) acc += h[q];
  ti.value[1] = acc - (double)(np - op->n);
  ti.have |= 2;
  return 0;
}

}  // namespace gpmi

extern "C" {

int gpmi_op_loglik_batch(gpmi_op* op, const double* etas, int neta, double* logdet,
                         double* gram, int* info) {
  if (!op) return set_errorf(-1006, "null handle");
  DeviceGuard g(op->device);
  int rc = run_factor(op, etas, neta, op->rhs_src);
  if (rc) return rc;
  std::vector<double> hout((size_t)neta * OUT_LD);
  std::vector<int> hinfo(neta);
  HIP_TRY(hipMemcpyAsync(hout.data(), op->fac.out, sizeof(double) * hout.size(),
                         hipMemcpyDeviceToHost, op->stream));
  HIP_TRY(hipMemcpyAsync(hinfo.data(), op->fac.info, sizeof(int) * neta, hipMemcpyDeviceToHost,
                         op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  // the batch-halves stream is joined and idle: release it, so that it does not hold
  // one of the process's hardware queues while other objects run (a band reduction
  // after a batch-8 call here: 181 ms with it alive, 162 ms without)
  HIP_TRY(op->fac.stream3.release());
  rc = collect_timing(op);
  if (rc) return rc;
  const int m = op->nrhs;
  int status = 0;
  for (int e = 0; e < neta; ++e) {
    if (logdet) logdet[e] = hout[(size_t)e * OUT_LD];
    if (gram)
      for (int a = 0; a < m; ++a)
        for (int c = 0; c < m; ++c)
          gram[((size_t)e * m + a) * m + c] = hout[(size_t)e * OUT_LD + 1 + a * RLD + c];
    if (info) info[e] = hinfo[e];
    if (hinfo[e] && !status) status = hinfo[e];
  }
  op->fac.cache_valid = (neta >= 1 && hinfo[0] == 0);
  op->fac.cached_eta = etas[0];
  if (status) set_errorf(status, "matrix K + eta I is not positive definite (pivot %d)", status);
  return 0;
}

int gpmi_op_logdet(gpmi_op* op, double eta, double* logdet) {
  if (!op) return set_errorf(-1006, "null handle");
  DeviceGuard g(op->device);
  bool fresh;
  int rc = factor_ready(op, eta, op->rhs_src, &fresh);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(logdet, op->fac.out, sizeof(double), hipMemcpyDeviceToHost,
                         op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  return 0;
}

int gpmi_op_solve(gpmi_op* op, double eta, const double* rhs, int64_t ld, int nrhs,
                  double* sol, int64_t ldsol) {
  if (!op) return set_errorf(-1006, "null handle");
  DeviceGuard g(op->device);
  const int nt = op->nt;
  const int64_t lda = op->n_pad;
  BatchPtrs P = op->ptrs();
  std::vector<double> h((size_t)op->n_pad * RLD);
  for (int c0 = 0; c0 < nrhs; c0 += RLD) {
    const int nc = std::min(RLD, nrhs - c0);
    int rc = upload_rhs(op, op->scratch, rhs, ld, nc, c0);
    if (rc) return rc;
    bool fresh;
    op->pred.ry_gen = ~0ull;   // R is overwritten below (gpmi_op_predict_terms keeps its own Y)
    rc = factor_ready(op, eta, op->scratch, &fresh);
    if (rc) return rc;
    if (!fresh) {
      // cached factor: forward substitution of the new RHS block
      HIP_TRY(hipMemcpyAsync(op->fac.R, op->scratch, sizeof(double) * P.sR,
                             hipMemcpyDeviceToDevice, op->stream));
      if ((rc = forward_substitute(op, P))) return rc;
    }
    for (int kb = nt - 1; kb >= 0; --kb) {
      hipLaunchKernelGGL(bwd_step_kernel, dim3(std::max(kb, 1), 1), dim3(256), 0, op->stream, P,
                         lda, kb, op->fac.X, P.sR);
      LAUNCH_CHECK("bwd_step_kernel");
    }
    HIP_TRY(hipMemcpyAsync(h.data(), op->fac.X, sizeof(double) * h.size(), hipMemcpyDeviceToHost,
                           op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    for (int64_t i = 0; i < op->n; ++i)
      for (int c = 0; c < nc; ++c) sol[i * ldsol + c0 + c] = h[(size_t)i * RLD + c];
  }
  return 0;
}

int gpmi_op_traceinv(gpmi_op* op, double eta, int exponent, double* value) {
  if (!op) return set_errorf(-1006, "null handle");
  if (!value) return set_errorf(-1004, "null output");
  if (exponent < 1 || exponent > 2)
    return set_errorf(-1010, "traceinv exponent %d outside [1, 2]", exponent);
  DeviceGuard g(op->device);
  bool fresh;
  int rc = factor_ready(op, eta, op->rhs_src, &fresh);
  if (rc) return rc;
  // W = L^-T from the cached factor in slot 0 (needed by both exponents)
  if ((rc = traceinv_build_w(op))) return rc;
  if (exponent == 2 && (rc = traceinv_build_ainv(op))) return rc;
  *value = op->tinv.value[exponent - 1];
  return 0;
}

// The read-backs below launch no kernel and change no cache state: a copy on the
// operator's stream, a synchronisation, and the masking on the host.

int gpmi_op_get_factor(gpmi_op* op, int slot, double* L_out, int64_t ldl) {
  if (!op) return set_errorf(-1006, "null handle");
  if (!L_out) return set_errorf(-1004, "null output");
  if (ldl < op->n) return set_errorf(-1005, "ldl %lld < n", (long long)ldl);
  const DenseFactor& f = op->fac;
  if (!op->has_K || f.last_nb < 1)
    return set_errorf(-1032, "no factorization since the matrix was loaded");
  if (slot < 0 || slot >= f.last_nb)
    return set_errorf(-1033, "slot %d outside the last batch [0, %d)", slot, f.last_nb);
  if (slot == 0 && !f.cache_valid) return set_errorf(-1032, "slot 0 holds no valid factor");
  DeviceGuard g(op->device);
  const int64_t n = op->n, np = op->n_pad;
  int inf = 0;
  HIP_TRY(hipMemcpyAsync(&inf, f.info + slot, sizeof(int), hipMemcpyDeviceToHost, op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  if (inf) return set_errorf(-1032, "slot %d: not positive definite (pivot %d)", slot, inf);
  HIP_TRY(hipMemcpy2DAsync(L_out, sizeof(double) * ldl, f.A + (int64_t)slot * np * np,
                           sizeof(double) * np, sizeof(double) * n, n, hipMemcpyDeviceToHost,
                           op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  // the strictly upper tiles hold working data
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = i + 1; j < n; ++j) L_out[i * ldl + j] = 0.0;
  return 0;
}

int gpmi_op_get_trinv(gpmi_op* op, double* W_out, int64_t ldw) {
  if (!op) return set_errorf(-1006, "null handle");
  if (!W_out) return set_errorf(-1004, "null output");
  if (ldw < op->n) return set_errorf(-1005, "ldw %lld < n", (long long)ldw);
  const DenseTraceInv& ti = op->tinv;
  if (!op->fac.cache_valid || ti.gen != op->factor_gen || !(ti.have & 1))
    return set_errorf(-1034, "no triangular inverse of the current factor (traceinv first)");
  DeviceGuard g(op->device);
  const int64_t n = op->n, np = op->n_pad;
  HIP_TRY(hipMemcpy2DAsync(W_out, sizeof(double) * ldw, ti.W, sizeof(double) * np,
                           sizeof(double) * n, n, hipMemcpyDeviceToHost, op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  // the lower block triangle may hold tiles of A^-1
  for (int64_t i = TS; i < n; ++i)
    for (int64_t j = 0; j < i / TS * TS; ++j) W_out[i * ldw + j] = 0.0;
  return 0;
}

int gpmi_op_get_inverse(gpmi_op* op, double* Ainv_out, int64_t lda) {
  if (!op) return set_errorf(-1006, "null handle");
  if (!Ainv_out) return set_errorf(-1004, "null output");
  if (lda < op->n) return set_errorf(-1005, "lda %lld < n", (long long)lda);
  const DenseTraceInv& ti = op->tinv;
  if (!op->fac.cache_valid || ti.gen != op->factor_gen || !(ti.have & 2))
    return set_errorf(-1035, "no inverse of the current factor (traceinv, exponent 2, first)");
  DeviceGuard g(op->device);
  const int64_t n = op->n, np = op->n_pad;
  std::vector<double> td((size_t)op->nt * TS * TS);
  HIP_TRY(hipMemcpy2DAsync(Ainv_out, sizeof(double) * lda, ti.W, sizeof(double) * np,
                           sizeof(double) * n, n, hipMemcpyDeviceToHost, op->stream));
  HIP_TRY(hipMemcpyAsync(td.data(), ti.Td, sizeof(double) * td.size(), hipMemcpyDeviceToHost,
                         op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  // strictly lower tiles as they are; the lower triangle of a diagonal tile from Td
  for (int64_t i = 0; i < n; ++i) {
    const int64_t c0 = i / TS * TS;
    const double* row = td.data() + (size_t)c0 * TS + (i - c0) * TS;
    for (int64_t j = c0; j <= i; ++j) Ainv_out[i * lda + j] = row[j - c0];
  }
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = i + 1; j < n; ++j) Ainv_out[i * lda + j] = Ainv_out[j * lda + i];
  return 0;
}

int gpmi_op_last_timing(gpmi_op* op, double* syrk_ms, int* syrk_launches, double* syrk_flops,
                        double* total_ms, double* syrk_busy_ms) {
  if (!op) return set_errorf(-1006, "null handle");
  if (syrk_busy_ms) *syrk_busy_ms = op->tim.last_syrk_busy_ms;
  if (syrk_ms) *syrk_ms = op->tim.last_syrk_ms;
  if (syrk_launches) *syrk_launches = op->tim.last_syrk_launches;
  if (syrk_flops) *syrk_flops = op->tim.last_syrk_flops;
  if (total_ms) *total_ms = op->tim.last_total_ms;
  return 0;
}

}  // extern "C"
