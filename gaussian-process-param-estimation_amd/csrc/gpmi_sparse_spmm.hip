// The sparse operator's SpMM: the lazy X windows, the choice of kernel and its launch,
// gpmi_sp_spmm, and the in-step timing of the launches (handle: gpmi_sp.h).

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "gpmi_sp.h"

using namespace gpmi;

namespace gpmi {
constexpr int WING_MAX_LDS = 80 * 1024;   // two workgroups per CU

// csr_spmm_wing_kernel<s> for s in [1, WING_MAXS] (index s - 1)
template <int... I>
constexpr std::array<decltype(&csr_spmm_wing_kernel<1, WING_U, WING_TPR>), sizeof...(I)>
wing_table(std::integer_sequence<int, I...>) {
  return {{&csr_spmm_wing_kernel<I + 1, WING_U, WING_TPR>...}};
}
const auto kWing = wing_table(std::make_integer_sequence<int, WING_MAXS>{});

static int build_window(gpmi_sp* sp);

int ensure_window(gpmi_sp* sp) {
  if (sp->win.maxu.load(std::memory_order_acquire) >= 0) return 0;
  std::lock_guard<std::mutex> lock(sp->win.mu);
  if (sp->win.maxu.load(std::memory_order_acquire) >= 0) return 0;
  const int rc = build_window(sp);
  if (rc) {
    (void)sp->win.cols.release();
    (void)sp->win.u.release();
    (void)sp->win.lidx.release();
  }
  return rc;
}

static int build_window(gpmi_sp* sp) {
  const int64_t nblk = (sp->n + WIN_ROWS - 1) / WIN_ROWS;
  HIP_TRY(sp->win.cols.reserve((size_t)nblk * WIN_MAXU));
  HIP_TRY(sp->win.u.reserve((size_t)nblk));
  HIP_TRY(sp->win.lidx.reserve((size_t)std::max<int64_t>(1, sp->nnz)));
  hipLaunchKernelGGL(spmm_window_build_kernel, dim3((unsigned)nblk), dim3(256), 0, sp->stream,
                     sp->indptr, sp->indices, sp->n, sp->win.cols, sp->win.u, sp->win.lidx);
  LAUNCH_CHECK("spmm_window_build_kernel");
  std::vector<int> hu((size_t)nblk);
  HIP_TRY(hipMemcpyAsync(hu.data(), sp->win.u, sizeof(int) * nblk, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  int mu = 0;
  for (int v : hu) mu = std::max(mu, v);
  {
    double su = 0.0;
    for (int v : hu) su += v;
    sp->win.mean = su / (double)nblk;
  }
  std::vector<int64_t> hp((size_t)sp->n + 1);
  HIP_TRY(hipMemcpy(hp.data(), sp->indptr, sizeof(int64_t) * (sp->n + 1), hipMemcpyDeviceToHost));
  int mm = 0;
  for (int64_t b = 0; b < nblk; ++b)
    if (hu[(size_t)b] > 0) {
      const int64_t r0 = b * WIN_ROWS, r1 = std::min<int64_t>(r0 + WIN_ROWS, sp->n);
      mm = std::max<int>(mm, (int)(hp[(size_t)r1] - hp[(size_t)r0]));
    }
  sp->win.maxm = mm;
  if (std::getenv("GPMI_SPMM_TRACE")) {
    double su = 0.0;
    int nz = 0;
    for (int v : hu) {
      su += v;
      nz += v == 0;
    }
    fprintf(stderr, "[gpmi spmm] %lld blocks of %d rows: window mean %.1f max %d, %d unwindowed, "
            "max block nnz %d\n", (long long)nblk, WIN_ROWS, su / (double)nblk, mu, nz, mm);
  }
  const size_t lds = (size_t)std::max(1, mu) * WIN_CS * 8 + 10 * (size_t)mm + 4 +
                     4 * (WIN_ROWS + 1);
  // the windowed kernel pays off while several workgroups fit a CU (2D tapered
  // Matern: windows of ~160 columns, 24 KB, 6 per CU: 1.2x); with 3D windows
  // (~350 columns, 49 KB, 3 per CU) it is slower than gathering from X
  sp->win.use = lds <= 32 * 1024;
  if (lds > 160 * 1024) return set_error(-1104, "spmm window exceeds LDS");
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&csr_spmm_win_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (auto f : kWing)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(f),
                               hipFuncAttributeMaxDynamicSharedMemorySize, WING_MAX_LDS));
  sp->win.nblk = nblk;
  sp->win.maxu.store(mu, std::memory_order_release);
  return 0;
}

// The SpMM kernel for an s-column block (0 gather, 1 windowed chunks, 3 gather by
// column pairs, 5 window with latency-hidden staging; 2, the round-2 one-pass
// window, is superseded by 5). GPMI_SPMM_WINDOW: 0 the gather-from-X kernel, 2 the windowed
// kernel, unset or 1 the faster one for this matrix (win.use); GPMI_SPMM_PAIR=0 keeps the
// one-column gather for even s. The alignment of a given block: spmm_resolve.
int spmm_kind(gpmi_sp* sp, int s, int* kind) {
  if (sp->dense.K) {
    *kind = 4;
    return 0;
  }
  const char* wenv = std::getenv("GPMI_SPMM_WINDOW");
  const int wmode = wenv ? std::atoi(wenv) : 1;
  if (wmode != 0)
    if (int rc = ensure_window(sp)) return rc;
  *kind = 0;
  // the window with latency-hidden staging (csr_spmm_wing_kernel) at every width up to
  // 20 (the Lanczos and multi-shift CG blocks and their N-rank shards) while the widest
  // window fits two workgroups per CU (GPMI_SPMM_WING=0: off)
  const char* genv = std::getenv("GPMI_SPMM_WING");
  if (wmode != 0 && !(genv && std::atoi(genv) == 0) && s >= 1 && s <= WING_MAXS &&
      sp->win.maxu.load(std::memory_order_acquire) > 0 &&
      sizeof(double) * (size_t)std::max(sp->win.maxu.load(std::memory_order_acquire),
                                        WIN_ROWS) * s <= (size_t)WING_MAX_LDS) {
    *kind = 5;
    return 0;
  }
  if (wmode == 2 || (wmode != 0 && sp->win.use)) *kind = 1;
  const char* penv = std::getenv("GPMI_SPMM_PAIR");
  if (*kind == 0 && s % 2 == 0 && s <= 64 && !(penv && std::atoi(penv) == 0)) *kind = 3;
  return 0;
}

// The kernel that runs for this block: spmm_kind, but the window kernel (5) stages
// even-width rows of X with 16-byte loads and the pair kernel (3) loads column pairs: an
// 8-byte aligned block handed in directly takes the one-column gather (0) instead.
static int spmm_resolve(gpmi_sp* sp, int s, const double* X, const double* Y, int* kind) {
  if (int rc = spmm_kind(sp, s, kind)) return rc;
  const bool aligned =
      ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 15) == 0;
  if (!aligned && (*kind == 3 || (*kind == 5 && s % 2 == 0))) *kind = 0;
  return 0;
}

// Y = (K + eta I) X by the kernel `kind` (spmm_resolve); pqp, pq_blocks: spmm.
static int spmm_launch(gpmi_sp* sp, int kind, const double* X, double* Y, int s, double eta,
                       hipStream_t st, double* pqp, int* pq_blocks, int dots2,
                       unsigned long long* stamp) {
  if (pq_blocks) *pq_blocks = 0;
  if (kind == 4) {
    // dense: split partials of K X on fp64 MFMA, summed in split order (+ eta X)
    double* Yp = st == sp->ms.stream ? sp->dense.Yp_ms : sp->dense.Yp;
    const dim3 grid((unsigned)((sp->n + 63) / 64), (unsigned)sp->dense.split);
    hipLaunchKernelGGL(s <= 16 ? dense_mm_kernel<1> : dense_mm_kernel<2>, grid, dim3(256), 0, st,
                       sp->dense.K, sp->dense.ld, sp->n, X, s, sp->dense.kcs, Yp);
    LAUNCH_CHECK("dense_mm_kernel");
    const int64_t ns = sp->n * s;
    hipLaunchKernelGGL(dense_mm_reduce_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st,
                       Yp, sp->dense.split, ns, X, eta, Y);
    LAUNCH_CHECK("dense_mm_reduce_kernel");
    return 0;
  }
  if (kind == 5) {
    // the window, and the epilogue's [64][s] rows of X . Y (pqp), with dots2 its
    // [64][2s] rows of X . Y and X . X (the Chronopoulos-Gear multi-shift CG)
    const size_t lds = sizeof(double) * (size_t)s *
                       (size_t)std::max(sp->win.maxu.load(std::memory_order_acquire),
                                        (dots2 ? 2 : 1) * WIN_ROWS);
    auto kfn = kWing[s - 1];
    const int tpr = WING_TPR;
    hipLaunchKernelGGL(kfn, dim3((unsigned)sp->win.nblk), dim3(64 * tpr), lds, st, sp->indptr,
                       sp->indices, sp->win.lidx, sp->data, sp->n, sp->win.cols, sp->win.u, X, Y,
                       eta, pqp, dots2, stamp);
    LAUNCH_CHECK("csr_spmm_wing_kernel");
    if (pqp && pq_blocks) *pq_blocks = (int)sp->win.nblk;
    return 0;
  }
  if (kind == 1) {
    // window + the largest windowed block's values, positions and row starts
    const size_t lds = sizeof(double) * WIN_CS *
                           (size_t)std::max(1, sp->win.maxu.load(std::memory_order_acquire)) +
                       10 * (size_t)sp->win.maxm + 4 + sizeof(int) * (WIN_ROWS + 1);
    hipLaunchKernelGGL(csr_spmm_win_kernel,
                       dim3((unsigned)sp->win.nblk),
                       dim3(256), lds, st, sp->indptr, sp->indices, sp->win.lidx, sp->data,
                       sp->n, sp->win.cols, sp->win.u, X, (int64_t)s, Y, (int64_t)s, s, eta);
    LAUNCH_CHECK("csr_spmm_win_kernel");
    return 0;
  }
  if (kind == 3) {
    // three gathers in flight per lane (measured at cfg 5: two 126.4, three 125.9, four
    // 132.5 us per s = 20 launch)
    hipLaunchKernelGGL(csr_spmm_pair_kernel<3>, dim3((unsigned)((sp->n + 3) / 4)), dim3(256), 0, st,
                       sp->indptr, sp->indices, sp->data, sp->n, X, Y, s, 64 / (s / 2), eta);
    LAUNCH_CHECK("csr_spmm_pair_kernel");
    return 0;
  }
  hipLaunchKernelGGL(csr_spmm_kernel, dim3((unsigned)((sp->n + 3) / 4)), dim3(256), 0,
                     st, sp->indptr, sp->indices, sp->data, sp->n, X, (int64_t)s, Y,
                     (int64_t)s, s, 64 / s, eta);
  LAUNCH_CHECK("csr_spmm_kernel");
  return 0;
}

// A free event, or a new one (owned by tim.events either way); under tim.mu.
static int take_event(gpmi_sp* sp, hipEvent_t* e) {
  if (sp->tim.free_ev.empty()) {
    HIP_TRY(sp->tim.events.reserve(sp->tim.events.ev.size() + 1, gpmi::timing_event_flags()));
    sp->tim.free_ev.push_back(sp->tim.events.ev.back());
  }
  *e = sp->tim.free_ev.back();
  sp->tim.free_ev.pop_back();
  return 0;
}

constexpr int STAMP_CAP = 8192;            // stamped window-SpMM launches per timing window
constexpr size_t STAMP_BYTES = 256u << 20;   // at most this much stamp buffer

// With in-step timing on (gpmi_sp_set_timing) the window SpMM stamps its span into the
// next slot, other kinds are bracketed by a HIP event pair on their stream.
int spmm(gpmi_sp* sp, const double* X, double* Y, int s, double eta, hipStream_t st, double* pqp,
         int* pq_blocks, int dots2) {
  if (!st) st = sp->stream;
  int kind = 0;
  if (int rc = spmm_resolve(sp, s, X, Y, &kind)) return rc;
  if (!sp->tim.on) return spmm_launch(sp, kind, X, Y, s, eta, st, pqp, pq_blocks, dots2, nullptr);
  SpTiming::SpmmRec rec{nullptr, nullptr, s, -1};
  {
    std::lock_guard<std::mutex> lock(sp->tim.mu);
    if (kind == 5 && sp->tim.stamps_used < sp->tim.stamp_cap) {
      rec.slot = sp->tim.stamps_used++;
    } else {
      if (int rc = take_event(sp, &rec.e0)) return rc;
      if (int rc = take_event(sp, &rec.e1)) return rc;
    }
  }
  if (rec.slot < 0) HIP_TRY(hipEventRecord(rec.e0, st));
  if (int rc = spmm_launch(sp, kind, X, Y, s, eta, st, pqp, pq_blocks, dots2,
                           rec.slot >= 0 ? sp->tim.stamps + 2 * sp->win.nblk * rec.slot : nullptr))
    return rc;
  if (rec.slot < 0) HIP_TRY(hipEventRecord(rec.e1, st));
  std::lock_guard<std::mutex> lock(sp->tim.mu);
  sp->tim.log.push_back(rec);
  return 0;
}

}  // namespace gpmi

extern "C" {

int gpmi_sp_spmm(gpmi_sp* sp, double eta, const double* X, int64_t ld, int ncol, double* Y,
                 int64_t ldy) {
  if (!sp) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  const int64_t n = sp->n;
  for (int c0 = 0; c0 < ncol; c0 += MAXS) {
    const int s = std::min(MAXS, ncol - c0);
    HIP_TRY(sp->work.ws.reserve((size_t)2 * n * s));
    std::vector<double> h((size_t)n * s);
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < s; ++c) h[(size_t)i * s + c] = X[orig_row(sp, i) * ld + c0 + c];
    HIP_TRY(hipMemcpyAsync(sp->work.ws, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice,
                          sp->stream));
    if (int rc = spmm(sp, sp->work.ws, sp->work.ws + n * s, s, eta)) return rc;
    HIP_TRY(hipMemcpyAsync(h.data(), sp->work.ws + n * s, sizeof(double) * h.size(),
                          hipMemcpyDeviceToHost, sp->stream));
    HIP_TRY(hipStreamSynchronize(sp->stream));
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < s; ++c) Y[orig_row(sp, i) * ldy + c0 + c] = h[(size_t)i * s + c];
  }
  return 0;
}

int gpmi_sp_spmm_info(gpmi_sp* sp, int* windowed, double* mean_window, int* max_window) {
  if (!sp) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  if (sp->dense.K) {   // dense: no window
    if (windowed) *windowed = 0;
    if (mean_window) *mean_window = 0.0;
    if (max_window) *max_window = 0;
    return 0;
  }
  if (int rc = ensure_window(sp)) return rc;
  const char* wenv = std::getenv("GPMI_SPMM_WINDOW");
  const int wmode = wenv ? std::atoi(wenv) : 1;
  if (windowed) *windowed = wmode == 2 || (wmode != 0 && sp->win.use);
  if (mean_window) *mean_window = sp->win.mean;
  if (max_window) *max_window = sp->win.maxu.load(std::memory_order_acquire);
  return 0;
}

int gpmi_sp_spmm_kernel(gpmi_sp* sp, int s, int* kind) {
  if (!sp || !kind) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  return spmm_kind(sp, s, kind);
}

}  // extern "C"

namespace gpmi {
// An empty launch that marks the start / end of a timing window in a rocprofv3
// kernel trace (tools/trace_summary.py --timed-spmm takes the SpMM launches
// between two marks as the timed ones).
__global__ void timing_mark_kernel(int on) { (void)on; }

// Holds its stream until the host sets *flag (pinned, coherent host memory), or at
// most max_ticks of the wall clock: the launches queued behind it then run back to
// back, not at the host's enqueue rate (gpmi_sp_bench_spmm).
__global__ void gate_kernel(const int* flag, unsigned long long max_ticks) {
  if (threadIdx.x != 0) return;
  const unsigned long long t0 = wall_clock64();
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0 &&
         wall_clock64() - t0 < max_ticks)
    __builtin_amdgcn_s_sleep(8);
}

// out[l] = (earliest start, latest end) over the nblk workgroup pairs of stamped
// launch l (one workgroup per launch).
__global__ void stamp_span_kernel(const unsigned long long* __restrict__ st, int64_t nblk,
                                  unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s0[256], s1[256];
  const int t = threadIdx.x;
  const unsigned long long* p = st + 2 * nblk * blockIdx.x;
  unsigned long long lo = ~0ull, hi = 0ull;
  for (int64_t i = t; i < nblk; i += 256) {
    lo = min(lo, p[2 * i]);
    hi = max(hi, p[2 * i + 1]);
  }
  s0[t] = lo;
  s1[t] = hi;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) {
      s0[t] = min(s0[t], s0[t + off]);
      s1[t] = max(s1[t], s1[t + off]);
    }
    __syncthreads();
  }
  if (t == 0) {
    out[2 * blockIdx.x] = s0[0];
    out[2 * blockIdx.x + 1] = s1[0];
  }
}
}  // namespace gpmi

extern "C" {

int gpmi_sp_set_timing(gpmi_sp* sp, int enable) {
  if (!sp) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  std::lock_guard<std::mutex> lock(sp->tim.mu);
  if (enable && !sp->tim.stamps && !sp->dense.K) {
    if (int rc = ensure_window(sp)) return rc;
    const size_t per = sizeof(unsigned long long) * 2 * (size_t)std::max<int64_t>(1, sp->win.nblk);
    sp->tim.stamp_cap = (int)std::min<size_t>(STAMP_CAP, STAMP_BYTES / per);
    HIP_TRY(sp->tim.stamps.reserve_bytes(per * sp->tim.stamp_cap));
    HIP_TRY(hipDeviceGetAttribute(&sp->tim.wall_khz, hipDeviceAttributeWallClockRate, sp->device));
  }
  hipLaunchKernelGGL(gpmi::timing_mark_kernel, dim3(1), dim3(64), 0, sp->stream, enable);
  LAUNCH_CHECK("timing_mark_kernel");
  if (enable) {
    // the pairs of an earlier window go back to the pool (their streams are idle
    // once the caller synchronised; wait for them anyway)
    for (auto& r : sp->tim.log) {
      if (r.slot >= 0) continue;
      HIP_TRY(hipEventSynchronize(r.e1));
      sp->tim.free_ev.push_back(r.e0);
      sp->tim.free_ev.push_back(r.e1);
    }
    sp->tim.log.clear();
    sp->tim.stamps_used = 0;
  }
  // (disabling keeps the window's log for gpmi_sp_spmm_timing)
  sp->tim.on = enable != 0;
  return 0;
}

int gpmi_sp_spmm_timing(gpmi_sp* sp, int max_widths, int* n_widths, int* widths, int* launches,
                        double* total_ms) {
  if (!sp || !n_widths) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  std::lock_guard<std::mutex> lock(sp->tim.mu);
  std::map<int, std::pair<int, double>> acc;
  std::vector<unsigned long long> st;
  if (sp->tim.stamps_used > 0) {
    // every stamped launch's span, reduced on the device (after the logged work)
    HIP_TRY(hipDeviceSynchronize());
    DevBuf<unsigned long long> span;
    HIP_TRY(span.reserve((size_t)2 * sp->tim.stamps_used));
    hipLaunchKernelGGL(gpmi::stamp_span_kernel, dim3(sp->tim.stamps_used), dim3(256), 0, sp->stream,
                       sp->tim.stamps, sp->win.nblk, span);
    LAUNCH_CHECK("stamp_span_kernel");
    st.resize((size_t)2 * sp->tim.stamps_used);
    HIP_TRY(hipMemcpyAsync(st.data(), span, sizeof(unsigned long long) * st.size(),
                          hipMemcpyDeviceToHost, sp->stream));
    HIP_TRY(hipStreamSynchronize(sp->stream));
  }
  for (auto& r : sp->tim.log) {
    double ms = 0.0;
    if (r.slot >= 0) {
      const unsigned long long t0 = st[2 * r.slot], t1 = st[2 * r.slot + 1];
      if (t1 < t0 || sp->tim.wall_khz <= 0) return set_error(-1107, "SpMM timing: a stamp slot was not written");
      ms = (double)(t1 - t0) / (double)sp->tim.wall_khz;
    } else {
      HIP_TRY(hipEventSynchronize(r.e1));
      float fms = 0.f;
      HIP_TRY(hipEventElapsedTime(&fms, r.e0, r.e1));
      ms = fms;
    }
    auto& a = acc[r.s];
    a.first += 1;
    a.second += ms;
  }
  *n_widths = (int)acc.size();
  int k = 0;
  for (auto& kv : acc) {
    if (k >= max_widths) break;
    if (widths) widths[k] = kv.first;
    if (launches) launches[k] = kv.second.first;
    if (total_ms) total_ms[k] = kv.second.second;
    ++k;
  }
  return 0;
}

int gpmi_sp_bench_spmm(gpmi_sp* sp, int s, int reps, double eta, double* avg_ms) {
  if (!sp) return set_error(-1006, "null handle");
  if (s < 1 || s > 64 || reps < 1) return set_error(-1103, "s in [1, 64], reps >= 1");
  DeviceGuard g(sp->device);
  const int64_t ns = sp->n * s;
  HIP_TRY(sp->work.ws.reserve((size_t)2 * ns));
  hipLaunchKernelGGL(rademacher_kernel, dim3(grid_ns(sp->n, s)), dim3(256), 0, sp->stream,
                     (double*)sp->work.ws, sp->n, s, 12345ull, 0, 1.0, (const int*)nullptr);
  LAUNCH_CHECK("rademacher_kernel");
  Event e0, e1;
  HIP_TRY(hipEventCreate(&e0.h));
  HIP_TRY(hipEventCreate(&e1.h));
  // warm-up, kept out of the in-step timing log (a logged warm-up made
  // the log 51 spans for the 50 timed launches, mixing a cold launch into the mean
  // span the bench subtracts from the gated period)
  bool timing_was;
  {
    std::lock_guard<std::mutex> lock(sp->tim.mu);
    timing_was = sp->tim.on;
    sp->tim.on = false;
  }
  int rc = spmm(sp, sp->work.ws, sp->work.ws + ns, s, eta);
  {
    std::lock_guard<std::mutex> lock(sp->tim.mu);
    sp->tim.on = timing_was;
  }
  if (rc) return rc;
  // the timed launches wait behind a gate until all of them are queued (at most 2 s)
  PinnedMem gate;
  HIP_TRY(gate.alloc(sizeof(int), hipHostMallocCoherent));
  int* flag = static_cast<int*>(gate.p);
  *flag = 0;
  int khz = 0;
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, sp->device));
  struct Open {   // on every way out: the gate opened, the stream drained, then the flag freed
    int* flag;
    hipStream_t st;
    ~Open() { __atomic_store_n(flag, 1, __ATOMIC_SEQ_CST), (void)hipStreamSynchronize(st); }
  } open{flag, sp->stream};
  hipLaunchKernelGGL(gpmi::gate_kernel, dim3(1), dim3(64), 0, sp->stream, flag,
                     (unsigned long long)std::max(khz, 1) * 2000ull);
  LAUNCH_CHECK("gate_kernel");
  HIP_TRY(hipEventRecord(e0, sp->stream));
  for (int r = 0; r < reps && rc == 0; ++r) rc = spmm(sp, sp->work.ws, sp->work.ws + ns, s, eta);
  __atomic_store_n(flag, 1, __ATOMIC_SEQ_CST);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(e1, sp->stream));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  *avg_ms = ms / reps;
  return 0;
}

}  // extern "C"
