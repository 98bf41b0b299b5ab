// The sparse operator's solvers: the blocked CG (gpmi_sp_cg) on the main stream, and the
// multi-shift CG's Gram blocks (gpmi_sp_msgram*) on a stream of their own, scheduled by
// gpmi_ms_sched.h (handle: gpmi_sp.h).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpmi_sp.h"
#include "gpmi_ms_sched.h"

using namespace gpmi;

namespace gpmi {

int cg_block_device(gpmi_sp* sp, double eta, int s, double rtol, int maxiter, int* it_used_out,
                    bool* converged) {
  const int64_t n = sp->n;
  const int64_t ns = n * s;
  double* X = sp->work.ws;
  double* Rr = X + ns;
  double* Pp = Rr + ns;
  double* Q = Pp + ns;
  // device scalars: pq, rr (double-buffered by iteration parity), thr = rtol ||b||,
  // the active flags (double-buffered), the error flag and the iteration count
  double* pq = sp->work.small;
  double* rrb[2] = {sp->work.small + MAXS, sp->work.small + 2 * MAXS};
  double* thr = sp->work.small + 3 * MAXS;
  int* actb[2] = {reinterpret_cast<int*>(sp->work.small + 4 * MAXS),
                  reinterpret_cast<int*>(sp->work.small + 5 * MAXS)};
  int* err = reinterpret_cast<int*>(sp->work.small + 6 * MAXS);
  int* iters = err + 1;
  HIP_TRY(hipMemcpyAsync(Pp, Rr, sizeof(double) * ns, hipMemcpyDeviceToDevice, sp->stream));
  HIP_TRY(hipMemsetAsync(X, 0, sizeof(double) * ns, sp->stream));
  if (int rc = col_dots(sp, Rr, 0, 1, Rr, s, rrb[0])) return rc;
  hipLaunchKernelGGL(cg_init_kernel, dim3(1), dim3(64), 0, sp->stream, rrb[0], rtol, s, thr,
                     actb[0], err, iters);
  LAUNCH_CHECK("cg_init_kernel");
  // The host reads the flags every CG_POLL iterations (one round trip each, not two per
  // iteration): iterations queued after the last column stopped do no vector work.
  constexpr int CG_POLL = 8;
  std::vector<int> flags(MAXS + 2);
  const unsigned grid = grid_ns(n, s);
  for (int it = 0; it < maxiter; ++it) {
    const int cur = it & 1;
    if (int rc = spmm(sp, Pp, Q, s, eta)) return rc;
    if (int rc = col_dots(sp, Pp, 0, 1, Q, s, pq)) return rc;
    hipLaunchKernelGGL(cg_xr_kernel, dim3(grid), dim3(256), 0, sp->stream, Pp, Q, X, Rr,
                       rrb[cur], pq, actb[cur], n, s, err);   // x += a p, r -= a q
    LAUNCH_CHECK("cg_xr_kernel");
    if (int rc = col_dots(sp, Rr, 0, 1, Rr, s, rrb[cur ^ 1])) return rc;
    hipLaunchKernelGGL(cg_p_kernel, dim3(grid), dim3(256), 0, sp->stream, Rr, Pp, rrb[cur],
                       rrb[cur ^ 1], actb[cur], actb[cur ^ 1], thr, it, iters, n, s);
    LAUNCH_CHECK("cg_p_kernel");   // p = r + b p
    if ((it + 1) % CG_POLL == 0 || it + 1 == maxiter) {
      HIP_TRY(hipMemcpyAsync(flags.data(), actb[cur ^ 1], sizeof(int) * s, hipMemcpyDeviceToHost,
                            sp->stream));
      HIP_TRY(hipMemcpyAsync(flags.data() + MAXS, err, sizeof(int), hipMemcpyDeviceToHost,
                            sp->stream));
      HIP_TRY(hipStreamSynchronize(sp->stream));
      if (flags[MAXS])
        return set_error(1, "CG: p^T (K + eta I) p <= 0 (K + eta I is not positive definite)");
      bool any = false;
      for (int c = 0; c < s; ++c) any = any || flags[c];
      if (!any) break;
    }
  }
  // the residual norms after the last iteration that ran sit in rrb[it_used & 1] (rrb[0]
  // when none ran); the no-op iterations queued after it rewrite the same values
  std::vector<double> rr(s), bnt(s);
  HIP_TRY(hipMemcpyAsync(flags.data() + MAXS, err, sizeof(int) * 2, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  if (flags[MAXS])
    return set_error(1, "CG: p^T (K + eta I) p <= 0 (K + eta I is not positive definite)");
  const int it_used = flags[MAXS + 1];
  *it_used_out = it_used;
  HIP_TRY(hipMemcpyAsync(bnt.data(), thr, sizeof(double) * s, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipMemcpyAsync(rr.data(), rrb[it_used & 1], sizeof(double) * s, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  for (int c = 0; c < s; ++c)
    if (!(std::sqrt(rr[c]) <= bnt[c])) *converged = false;
  return 0;
}

}  // namespace gpmi

extern "C" {

// Upload a block of at most MAXS columns (permuted into the device row order), the CG on
// the device (cg_block_device), download.
int gpmi_sp_cg(gpmi_sp* sp, double eta, const double* rhs, int64_t ld, int nrhs, double rtol,
               int maxiter, double* sol, int64_t ldsol, int* iterations) {
  if (!sp) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  const int64_t n = sp->n;
  int max_it_used = 0;
  bool converged = true;
  sp->last_converged = 0;
  for (int c0 = 0; c0 < nrhs; c0 += MAXS) {
    const int s = std::min(MAXS, nrhs - c0);
    const int64_t ns = n * s;
    HIP_TRY(sp->work.ws.reserve((size_t)4 * ns));
    double* X = sp->work.ws;
    double* Rr = X + ns;
    std::vector<double> h((size_t)ns);
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < s; ++c) h[(size_t)i * s + c] = rhs[orig_row(sp, i) * ld + c0 + c];
    HIP_TRY(hipMemcpyAsync(Rr, h.data(), sizeof(double) * ns, hipMemcpyHostToDevice, sp->stream));
    int it_used = 0;
    if (int rc = cg_block_device(sp, eta, s, rtol, maxiter, &it_used, &converged)) return rc;
    max_it_used = std::max(max_it_used, it_used);
    HIP_TRY(hipMemcpyAsync(h.data(), X, sizeof(double) * ns, hipMemcpyDeviceToHost, sp->stream));
    HIP_TRY(hipStreamSynchronize(sp->stream));
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < s; ++c) sol[orig_row(sp, i) * ldsol + c0 + c] = h[(size_t)i * s + c];
  }
  if (iterations) *iterations = max_it_used;
  sp->last_converged = converged ? 1 : 0;
  return 0;
}

// The multi-shift CG in the Chronopoulos-Gear form (round 5): per iteration the SpMM
// w = (K + eta_0 I) r with the r . w / r . r block rows in its epilogue (window SpMM;
// other kinds: + ms_dots2_kernel), ms_cg2_reduce_kernel (those rows and the previous
// update's B^T r rows summed), then ms_cg2_update_kernel (the scalars, p, s, r, the
// B^T r rows, and the shift step of the previous iteration): three dependent launches
// per iteration against the standard form's five (round 4: SpMM, its p . q sum, the r
// update with B^T r, its sum, the tail), and six vector passes against seven: cfg 4
// 4.80 -> 4.31 ms, cfg 5 13.44 -> 12.81 ms per step on one box (tools/sparse_ab.sh).
// (A two-launch form that summed the rows inside the SpMM and the update by group
// last-arriver tickets was slower: every block then drains its stores before its
// ticket, 12.6 -> 25 us per cfg 4 SpMM.)
//
// Three phases (msgram_cg2): setup (ms_alloc, ms_start), the iterations (ms_schedule of
// gpmi_ms_sched.h decides the batches, the slot reads and the compactions; MsDev below
// only queues what it is told to), and the read-back (ms_finish).

// One block of the multi-shift CG, s columns wide: the vectors, the update's B^T r
// block partials [nbd s][MS_UB] and the scalar state.
struct MsBlock {
  double *R, *W, *S, *bpart;
  MsScal sc[2];   // by iteration parity
  MsShift sh;     // (flags and it_stop belong to the run: every block's point to the same)
  int s;
};

// The one layout of a block: carves *b (all but sh.flags and sh.it_stop) out of base and
// returns the doubles it takes; base == nullptr: the size only. R, W and S start on 16
// bytes (the window SpMM loads their rows 16 bytes at a time).
static size_t ms_carve(double* base, int64_t n, int s, int nbd, int S, MsBlock* b) {
  size_t off = 0;
  auto take = [&](size_t d) {
    double* p = base ? base + off : nullptr;
    off += d;
    return p;
  };
  auto even = [](size_t d) { return (d + 1) & ~(size_t)1; };
  MsBlock k{};
  k.s = s;
  k.R = take(even((size_t)n * s));
  k.W = take(even((size_t)n * s));
  k.S = take(even((size_t)n * s));
  k.bpart = take((size_t)MS_UB * nbd * s);
  for (MsScal& c : k.sc) {
    c.rr = take(s);
    c.a = take(s);
    c.a_prev = take(s);
    c.beta = take(s);
    c.active = reinterpret_cast<int*>(take(s));
  }
  k.sh.bn2 = take(s);
  k.sh.z = take((size_t)S * s);
  k.sh.z_prev = take((size_t)S * s);
  k.sh.bp = take((size_t)S * nbd * s);
  k.sh.g = take((size_t)S * nbd * s);
  if (base) {
    k.sh.flags = b->sh.flags;
    k.sh.it_stop = b->sh.it_stop;
    *b = k;
  }
  return off;
}

// The device side of the iterations (the Dev of ms_schedule): the current block, one
// iteration's launches, the two slots' events, and the compaction's gather.
struct MsDev {
  gpmi_sp* sp;
  hipStream_t str;
  int64_t n;
  int S, nbd, s0;         // shifts, columns of B, the block's width at the start
  double eta0, rtol;
  double *Bd, *Hs;        // B [n][nbd], the host staging [n][nrhs]
  // dot rows: the SpMM's per-block [nblk][2s]; their sums and the B^T r sums [2s + nbd s]
  // (ms_cg2_reduce_kernel); the init partials [MS_NBLK][ne]
  double *spart, *dred, *ipart;
  double* dshift;         // [S] eta_j - eta_0
  MsPin *pin_host, *pin_dev;
  MsBlock blk;            // the current block, carved out of sp->ms.blk[buf]
  int buf;

  MsPin* pin() { return pin_host; }
  int mark(int slot) {
    HIP_TRY(hipEventRecord(sp->ms.ev[slot], str));
    return 0;
  }
  int wait(int slot) {
    HIP_TRY(hipEventSynchronize(sp->ms.ev[slot]));
    return 0;
  }

  // one iteration's launches on str (parity k & 1 picks the scalar buffers)
  int iterate(int k, int slot) {
    const int s = blk.s, neb = nbd * s;
    int rows = 0;
    if (int rc = spmm(sp, blk.R, blk.W, s, eta0, str, spart, &rows, 1)) return rc;
    if (rows == 0) {
      hipLaunchKernelGGL(ms_dots2_kernel, dim3(MS_DOT_BLK), dim3(256), 0, str,
                         (const double*)blk.R, (const double*)blk.W, n, s, spart);
      LAUNCH_CHECK("ms_dots2_kernel");
      rows = MS_DOT_BLK;
    }
    hipLaunchKernelGGL(ms_cg2_reduce_kernel, dim3(2 * s + neb), dim3(256), 0, str,
                       (const double*)spart, rows, s, (const double*)blk.bpart, MS_UB, neb, dred);
    LAUNCH_CHECK("ms_cg2_reduce_kernel");
    hipLaunchKernelGGL(ms_cg2_update_kernel, dim3(MS_UB + 1), dim3(256), 0, str,
                       (const double*)Bd, blk.R, (const double*)blk.W, blk.S, blk.sc[k & 1],
                       blk.sc[(k + 1) & 1], blk.sh, (const double*)dred, blk.bpart,
                       (const double*)dshift, S, s, nbd, rtol * rtol, k, n,
                       slot >= 0 ? pin_dev + slot : (MsPin*)nullptr);
    LAUNCH_CHECK("ms_cg2_update_kernel");
    return 0;
  }

  // One launch on the CG's stream gathers the kept columns' state (r, s, the scalars of
  // parity it & 1, the shift recurrences, the B^T r block partials) into a block of
  // width a and scatters the dropped columns' final Grams into ms_gfin; the host only
  // switches its block. The new block is carved out of the buffer the current one is
  // NOT in (the start block took ms_blk[0], compaction k takes ms_blk[k & 1]): the
  // gather never writes the buffer it reads.
  int compact(const int* map, int a, const int* drop, const int* drop_orig, int nd, int it) {
    const int nbuf = buf ^ 1;
    HIP_TRY(sp->ms.blk[nbuf].reserve(ms_carve(nullptr, n, a, nbd, S, nullptr)));
    MsBlock nw = blk;   // (the run's flags and it_stop)
    ms_carve(sp->ms.blk[nbuf], n, a, nbd, S, &nw);
    const MsScal &cur = blk.sc[it & 1], &ncur = nw.sc[it & 1];
    MsCompactArgs A{};
    auto job = [&](const double* src, int64_t rows, int L, double* dst) {
      A.job[A.njob++] = MsCompactJob{src, dst, rows, L, 0};
    };
    job(blk.R, n, 1, nw.R);
    job(blk.S, n, 1, nw.S);
    job(blk.bpart, nbd, MS_UB, nw.bpart);   // [cp s + c][vb] -> [cp a + c'][vb]
    job(cur.rr, 1, 1, ncur.rr);
    job(cur.a, 1, 1, ncur.a);
    job(cur.a_prev, 1, 1, ncur.a_prev);
    job(cur.beta, 1, 1, ncur.beta);
    job(blk.sh.bn2, 1, 1, nw.sh.bn2);
    job(blk.sh.z, S, 1, nw.sh.z);
    job(blk.sh.z_prev, S, 1, nw.sh.z_prev);
    job(blk.sh.bp, (int64_t)S * nbd, 1, nw.sh.bp);
    job(blk.sh.g, (int64_t)S * nbd, 1, nw.sh.g);
    A.s = blk.s;
    A.a = a;
    A.nd = nd;
    A.s0 = s0;
    std::copy(map, map + a, A.map);
    std::copy(drop, drop + nd, A.drop);
    std::copy(drop_orig, drop_orig + nd, A.drop_orig);
    A.g = blk.sh.g;
    A.gfin = sp->ms.gfin;
    A.SN = (int64_t)S * nbd;
    A.act_src = cur.active;
    A.act = ncur.active;
    int64_t most = A.SN * nd;
    for (int q = 0; q < A.njob; ++q)
      most = std::max<int64_t>(most, A.job[q].rows * a * A.job[q].L);
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (most + 255) / 256));
    hipLaunchKernelGGL(ms_compact_kernel, dim3(gx, A.njob + 1), dim3(256), 0, str, A);
    LAUNCH_CHECK("ms_compact_kernel");
    blk = nw;
    buf = nbuf;
    return 0;
  }
};

// The run's workspaces (grown on demand) and the start block of width s in ms_blk[0].
static int ms_alloc(MsDev& d, int s, int nrhs, int kind, bool gfin) {
  gpmi_sp* sp = d.sp;
  const int64_t n = d.n;
  const int S = d.S, nbd = d.nbd;
  auto even = [](size_t x) { return (x + 1) & ~(size_t)1; };
  HIP_TRY(sp->ms.ws.reserve(even((size_t)n * nbd) + even((size_t)n * nrhs)));
  d.Bd = sp->ms.ws;
  d.Hs = d.Bd + even((size_t)n * nbd);
  const size_t c_sp = (size_t)(kind == 5 ? sp->win.nblk : MS_DOT_BLK) * 2 * s;
  const size_t c_red = 2 * (size_t)s + (size_t)nbd * s;
  const size_t c_init = (size_t)MS_NBLK * ((size_t)nbd * s + s);
  HIP_TRY(sp->ms.cg2_buf.reserve(c_sp + c_red + c_init + S + 2));
  d.spart = sp->ms.cg2_buf;
  d.dred = d.spart + c_sp;
  d.ipart = d.dred + c_red;
  d.dshift = d.ipart + c_init;
  HIP_TRY(sp->ms.blk[0].reserve(ms_carve(nullptr, n, s, nbd, S, nullptr)));
  d.buf = 0;
  d.blk.sh.flags = reinterpret_cast<int*>(d.dshift + S);
  d.blk.sh.it_stop = reinterpret_cast<int*>(d.dshift + S + 1);
  ms_carve(sp->ms.blk[0], n, s, nbd, S, &d.blk);
  // the dropped columns' final Grams, on the device until the end
  if (gfin) HIP_TRY(sp->ms.gfin.reserve((size_t)S * nbd * s));
  if (!sp->ms.pin.p) {
    // coherent: the batch's last update kernel stores the end state into it directly
    HIP_TRY(sp->ms.pin.alloc(2 * sizeof(MsPin), hipHostMallocCoherent | hipHostMallocMapped));
    for (Event& e : sp->ms.ev) HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
  }
  d.pin_host = reinterpret_cast<MsPin*>(sp->ms.pin.p);
  d.pin_dev = nullptr;
  HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d.pin_dev), sp->ms.pin.p, 0));
  return 0;
}

// B (every column of the host block, in device row order), r_0 = its columns from c_lo,
// s_{-1} = 0, the shifts, and the scalars' start (ms_init_kernel).
static int ms_start(MsDev& d, const double* etas, const double* rhs, int64_t ld, int nrhs,
                    int c_lo, bool full) {
  gpmi_sp* sp = d.sp;
  hipStream_t str = d.str;
  const int64_t n = d.n;
  const int S = d.S, nbd = d.nbd, s = d.blk.s;
  const int64_t ns = n * s;
  const double* Hsrc = d.Hs;
  if (!rhs) {
    Hsrc = sp->ms.rhs_dev;
  } else if (ld == nrhs) {
    HIP_TRY(hipMemcpyAsync(d.Hs, rhs, sizeof(double) * n * nrhs, hipMemcpyHostToDevice, str));
  } else {
    std::vector<double> h((size_t)n * nrhs);
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < nrhs; ++c) h[(size_t)i * nrhs + c] = rhs[i * ld + c];
    HIP_TRY(hipMemcpyAsync(d.Hs, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, str));
    HIP_TRY(hipStreamSynchronize(str));
  }
  hipLaunchKernelGGL(rows_gather_kernel, dim3(grid_ns(n, nbd)), dim3(256), 0, str, Hsrc, nrhs,
                     (const int*)sp->perm_d, n, nbd, d.Bd);
  LAUNCH_CHECK("rows_gather_kernel");
  std::vector<double> hd(S);
  for (int j = 0; j < S; ++j) hd[j] = etas[j] - d.eta0;
  HIP_TRY(hipMemcpyAsync(d.dshift, hd.data(), sizeof(double) * S, hipMemcpyHostToDevice, str));
  if (full) {
    HIP_TRY(hipMemcpyAsync(d.blk.R, d.Bd, sizeof(double) * ns, hipMemcpyDeviceToDevice, str));
  } else {
    hipLaunchKernelGGL(rows_gather_kernel, dim3(grid_ns(n, s)), dim3(256), 0, str, d.Bd + c_lo,
                       nbd, (const int*)nullptr, n, s, d.blk.R);
    LAUNCH_CHECK("rows_gather_kernel");
  }
  // s_{-1} = 0 (beta_{-1} = 0 multiplies it: no NaN may stand there)
  HIP_TRY(hipMemsetAsync(d.blk.S, 0, sizeof(double) * ns, str));
  launch_ms_dots(d.Bd, d.blk.R, n, s, d.ipart, MS_NBLK, str, nbd);
  LAUNCH_CHECK("ms_dots_partial_kernel");
  hipLaunchKernelGGL(ms_init_kernel, dim3(1), dim3(1024), 0, str, d.blk.sc[0], d.blk.sh,
                     (const double*)d.ipart, MS_NBLK, S, s, nbd, d.pin_dev);
  LAUNCH_CHECK("ms_init_kernel");
  return 0;
}

// The last step of columns still active at maxiter (a no-op when all stopped), then G:
// each original column from the final block, or from the final Grams its compaction
// scattered when it was dropped.
static int ms_finish(MsDev& d, const MsRun& run, int nrhs, int nsub, bool trace, double* G,
                     int* iterations) {
  gpmi_sp* sp = d.sp;
  hipStream_t str = d.str;
  const int S = d.S, nbd = d.nbd, s0 = d.s0, s = d.blk.s, it = run.launched;
  const MsScal& cur = d.blk.sc[it & 1];
  const MsShift& sh = d.blk.sh;
  hipLaunchKernelGGL(ms_cg2_close_kernel, dim3(1), dim3(256), 0, str, cur, sh,
                     (const double*)d.dshift, S, s, nbd);
  LAUNCH_CHECK("ms_cg2_close_kernel");
  int flag = 0, it_stop = -1;
  std::vector<int> hact(s);
  HIP_TRY(hipMemcpyAsync(hact.data(), cur.active, sizeof(int) * s, hipMemcpyDeviceToHost, str));
  HIP_TRY(hipMemcpyAsync(&flag, sh.flags, sizeof(int), hipMemcpyDeviceToHost, str));
  HIP_TRY(hipMemcpyAsync(&it_stop, sh.it_stop, sizeof(int), hipMemcpyDeviceToHost, str));
  std::vector<double> hg((size_t)S * nbd * s);
  HIP_TRY(hipMemcpyAsync(hg.data(), sh.g, sizeof(double) * hg.size(), hipMemcpyDeviceToHost, str));
  std::vector<double> g_final;   // [j][cp][c original], the dropped columns' entries
  if (run.compactions > 0) {
    g_final.resize((size_t)S * nbd * s0);
    HIP_TRY(hipMemcpyAsync(g_final.data(), sp->ms.gfin, sizeof(double) * g_final.size(),
                          hipMemcpyDeviceToHost, str));
  }
  HIP_TRY(hipStreamSynchronize(str));
  sp->ms.last_compactions = run.compactions;
  sp->ms.last_segments = run.segments;
  if (flag)
    return set_error(1, "multi-shift CG: p^T (K + min(eta) I) p <= 0 (not positive definite)");
  bool any = false;
  for (int c = 0; c < s; ++c) any = any || hact[c];
  sp->last_converged = any ? 0 : 1;
  std::vector<int> where(s0, -1);
  for (int c = 0; c < s; ++c) where[run.orig[c]] = c;
  for (int j = 0; j < S; ++j)
    for (int a = 0; a < nrhs; ++a)
      for (int c = 0; c < nsub; ++c) {
        const size_t jc = (size_t)j * nbd + a;
        G[((size_t)j * nrhs + a) * nsub + c] =
            where[c] >= 0 ? hg[jc * s + where[c]] : g_final[jc * s0 + c];
      }
  if (trace)
    std::fprintf(stderr, "[ms] all stopped at %d, %d compactions\n", it_stop, run.compactions);
  if (iterations) *iterations = it_stop >= 0 ? it_stop : it;
  return 0;
}

static int msgram_cg2(gpmi_sp* sp, const double* etas, int neta, const double* rhs,
                      int64_t ld, int nrhs, int c_lo, int c_hi, double rtol, int maxiter,
                      double* G, int* iterations) {
  const int nsub = c_hi - c_lo;
  const bool full = nsub == nrhs;
  DeviceGuard g(sp->device);
  int s = nsub;
  int kind = 0;
  if (int rc = spmm_kind(sp, s, &kind)) return rc;
  // Padding (the Gram of the real columns is unchanged by a zero column, inactive
  // from the start: ||b|| = 0): the window SpMM at s = 11 stages 12-column rows with
  // 16-byte loads: cfg 5 s = 11 88 -> 73 us per launch (round 3)
  if (full && kind == 5 && s == 11 && neta * (s + 1) <= 1024) ++s;
  if (int rc = spmm_kind(sp, s, &kind)) return rc;
  if (!sp->ms.stream) {
    // the CG's own stream, at the same (normal) dispatch priority as the Lanczos's.
    // Round 5 gave it the high priority (cfg 5 11.85 -> 11.46 ms, when the CG alone took
    // 8.8 ms); since the compaction the CG alone takes 6.4 ms and a starved Lanczos (4.1
    // ms alone) plus its host-side quadrature became the step's tail: round 6 alternating
    // runs, high / normal / low: cfg 5 9.80-9.92 / 9.40-9.44 / 9.77-10.05 ms, cfg 4
    // 2.86-2.90 / 2.80-2.82 / 2.83-2.86 ms.
    HIP_TRY(hipStreamCreateWithFlags(&sp->ms.stream.h, hipStreamNonBlocking));
  }
  // GPMI_MS_COMPACT=0: no active-column compaction
  const char* cenv = std::getenv("GPMI_MS_COMPACT");
  const bool compact_on = !(cenv && std::atoi(cenv) == 0);
  // GPMI_MS_TRACE=1: each batch's size and each read's prediction on stderr (diagnostic)
  const bool trace = std::getenv("GPMI_MS_TRACE") != nullptr;
  MsDev dev{};
  dev.sp = sp;
  dev.str = sp->ms.stream;
  dev.n = sp->n;
  dev.S = neta;
  dev.nbd = full ? s : nrhs;
  dev.s0 = s;
  dev.eta0 = *std::min_element(etas, etas + neta);
  dev.rtol = rtol;
  sp->last_converged = 0;
  if (int rc = ms_alloc(dev, s, nrhs, kind, compact_on && s > 1)) return rc;
  if (int rc = ms_start(dev, etas, rhs, ld, nrhs, c_lo, full)) return rc;
  MsRun run;
  const int rc = ms_schedule(dev, s, rtol, maxiter, compact_on, trace, &run);
  if (run.indefinite) {
    HIP_TRY(hipStreamSynchronize(dev.str));
    return set_error(1, "multi-shift CG: p^T (K + min(eta) I) p <= 0 (not positive definite)");
  }
  if (rc) return rc;
  return ms_finish(dev, run, nrhs, nsub, trace, G, iterations);
}

// Multi-shift CG Gram blocks for the right-hand sides B[:, c_lo:c_hi] of the nb-column
// host block B (every eta): G[j][a][c] = b_a^T (K + eta_j I)^-1 b_{c_lo + c}, a < nb
// (the dots run over all of B, so a shard of columns gives complete G columns).
static int msgram_impl(gpmi_sp* sp, const double* etas, int neta, const double* rhs,
                       int64_t ld, int nrhs, int c_lo, int c_hi, double rtol, int maxiter,
                       double* G, int* iterations) {
  if (!sp) return set_error(-1006, "null handle");
  // rhs == NULL: the resident block of gpmi_sp_set_rhs (already in HBM: no upload)
  if (!rhs && (!sp->ms.rhs_dev || nrhs != sp->ms.rhs_nrhs))
    return set_error(-1105, "msgram: rhs NULL needs a resident block of nrhs columns "
                            "(gpmi_sp_set_rhs)");
  if (neta < 1 || nrhs < 1 || nrhs > MS_MAXS || c_lo < 0 || c_hi > nrhs || c_lo >= c_hi ||
      neta * (c_hi - c_lo) > 1024)
    return set_error(-1104, "msgram: need 1 <= nrhs <= 16, 0 <= c_lo < c_hi <= nrhs and "
                            "neta * (c_hi - c_lo) <= 1024");
  return msgram_cg2(sp, etas, neta, rhs, ld, nrhs, c_lo, c_hi, rtol, maxiter, G, iterations);
}

int gpmi_sp_msgram(gpmi_sp* sp, const double* etas, int neta, const double* rhs, int64_t ld,
                   int nrhs, double rtol, int maxiter, double* G, int* iterations) {
  return msgram_impl(sp, etas, neta, rhs, ld, nrhs, 0, nrhs, rtol, maxiter, G, iterations);
}

int gpmi_sp_msgram_cols(gpmi_sp* sp, const double* etas, int neta, const double* rhs, int64_t ld,
                        int nrhs, int c_lo, int c_hi, double rtol, int maxiter, double* G,
                        int* iterations) {
  return msgram_impl(sp, etas, neta, rhs, ld, nrhs, c_lo, c_hi, rtol, maxiter, G, iterations);
}

int gpmi_sp_msgram_compactions(const gpmi_sp* sp, int* count) {
  if (!sp || !count) return set_error(-1006, "null handle");
  *count = sp->ms.last_compactions;
  return 0;
}

int gpmi_sp_msgram_segments(const gpmi_sp* sp, int cap, int* widths, int* iterations,
                            int* count) {
  if (!sp || !count) return set_error(-1006, "null handle");
  const int m = (int)sp->ms.last_segments.size();
  *count = m;
  if (m > 0 && cap < m) return set_error(-1003, "gpmi_sp_msgram_segments: cap < segments");
  if (m > 0 && (!widths || !iterations)) return set_error(-1006, "null output");
  for (int q = 0; q < m; ++q) {
    widths[q] = sp->ms.last_segments[q].first;
    iterations[q] = sp->ms.last_segments[q].second;
  }
  return 0;
}

}  // extern "C"
