// C-ABI of the sparse path (include/gpmi.h, gpmi_sp_*): tapered Matérn CSR
// assembly, SpMM, blocked Lanczos with full (CGS2) reorthogonalisation for
// stochastic Lanczos quadrature, and blocked CG.

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <utility>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <map>
#include <vector>

#include "gpmi_internal.h"
#include "gpmi_host.h"
#include "gpmi_sparse.h"
#include "gpmi_ms_sched.h"
#include "gpmi_band.h"
#include "../../include/gpmi.h"

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
int op_view(const gpmi_op* op, OpView* v);            // gpmi_api.hip
int matern_params_host(double nu, MaternParams* P);   // gpmi_api.hip
}  // namespace gpmi

namespace {

constexpr int NBLK = 256;   // fixed reduction grid (deterministic sums)
constexpr int MAXS = 32;    // vector-block width per device pass

}  // namespace

struct gpmi_sp {
  int device = 0;
  int64_t n = 0, nnz = 0;
  double tau = 0.0;
  hipStream_t stream = nullptr;
  int64_t* indptr = nullptr;
  int* indices = nullptr;
  double* data = nullptr;
  // workspace (grown on demand)
  size_t ws_doubles = 0;
  double* ws = nullptr;
  double* partial = nullptr;   // [NBLK][J][s]
  size_t partial_doubles = 0;
  double* small = nullptr;     // coefficient / reduction arrays
  double* lz = nullptr;        // Lanczos scalars (lanczos_block)
  size_t lz_doubles = 0;
  double* lzd = nullptr;       // DCGS2 Lanczos scalars (lanczos_block_dcgs2)
  size_t lzd_doubles = 0;
  int lanczos_cgs2_reruns = 0; // DCGS2 blocks rerun with CGS2 (cancellation in rho)
  // the multi-shift CG (gpmi_sp_msgram) has a stream and workspaces of its own, so
  // that it may run from another host thread beside a Lanczos on `stream` (the
  // sparse step's two independent halves overlap on the device)
  hipStream_t ms_stream = nullptr;
  double* ms_ws = nullptr;                 // B [n][nb] and the host staging [n][nrhs]
  double* rhs_dev = nullptr;               // resident RHS block [n][rhs_nrhs] (gpmi_sp_set_rhs)
  int rhs_nrhs = 0;
  size_t ms_ws_doubles = 0;
  void* ms_pin = nullptr;                  // pinned flags / r.r of two CG batches
  // the Chronopoulos-Gear form's dot rows (sized for the start width), the shifts and
  // the two flags
  double* cg2_buf = nullptr;
  // the block's state (MsBlock: R, W, S, the B^T r partials, the scalars), two buffers,
  // alternating: the start block in [0], compaction k (1-based) gathers the active
  // columns from the current one into [k & 1]
  double* ms_blk[2] = {nullptr, nullptr};
  size_t ms_blk_doubles[2] = {0, 0};
  double* ms_gfin = nullptr;   // the stopped columns' final Grams [S nb][s0]
  size_t ms_gfin_doubles = 0;
  size_t cg2_doubles = 0;
  hipEvent_t ms_ev[2] = {nullptr, nullptr};
  std::mutex win_mu;           // the lazy X-window build (ensure_window)
  int last_converged = 1;      // last gpmi_sp_cg / gpmi_sp_msgram met rtol in every column
  int last_compactions = 0;    // active-column compactions of the last multi-shift CG
  // its launch segments: (block width, iterations launched at that width), in order
  std::vector<std::pair<int, int>> last_segments;
  // Locality order (gpmi_sp_create_matern, d <= 3): device row r is original point
  // perm[r] (cells in Morton order), so the rows a CU streams through have their X
  // gathers in a compact window that stays in its XCD's L2. Host inputs and
  // outputs of every call stay in the original order (permuted at the boundary).
  std::vector<int> perm;       // empty: identity
  int* perm_d = nullptr;
  // X windows of the default SpMM (csr_spmm_win_kernel), built on first use
  int* win_cols = nullptr;             // [nblk][WIN_MAXU] sorted window columns
  int* win_u = nullptr;                // [nblk] window sizes (0: block gathers from X)
  unsigned short* win_lidx = nullptr;  // [nnz] window position of every nonzero
  // -1: not built. Published (release) after every other window field, so a reader
  // that sees it >= 0 (acquire; the Lanczos and the multi-shift CG may run on two
  // host threads) sees the whole window
  std::atomic<int> win_maxu{-1};
  int win_maxm = 0;                    // most nonzeros in a windowed block
  double win_mean = 0.0;               // mean window columns per block
  bool win_use = false;                // the windowed kernel is the faster one here
  int64_t win_nblk = 0;
  // dense mode (gpmi_sp_create_dense): K borrowed from a gpmi_op, no CSR
  const double* dK = nullptr;
  int64_t dld = 0;
  int dsplit = 1, dkcs = 1;            // k splits of dense_mm_kernel, 64-column chunks each
  double* dYp = nullptr;               // split partials [dsplit][n][MAXS] of `stream`
  double* dYp_ms = nullptr;            // ... of ms_stream (the CG beside the Lanczos)
  // In-step SpMM timing (gpmi_sp_set_timing), logged per launch with its width;
  // gpmi_sp_spmm_timing sums the spans per width. The window SpMM (every SpMM of
  // the sparse sweeps) stamps each workgroup's start and end on the device's
  // constant wall clock into the launch's slot of `stamps` (win_nblk pairs, plain
  // stores at the workgroup's end: the timed steps themselves carry the timing);
  // stamp_span_kernel reduces a slot to the launch's span (earliest start, latest
  // end). Other kinds get a HIP event pair on their stream. The two host threads
  // of a sweep both launch SpMMs: the log is under timing_mu.
  std::mutex timing_mu;
  bool timing = false;
  std::vector<hipEvent_t> ev_pool;     // free events
  unsigned long long* stamps = nullptr;   // [stamp_cap][win_nblk][2]
  int stamp_cap = 0;                   // launches the buffer holds
  int stamps_used = 0;
  int wall_khz = 0;                    // wall clock rate (hipDeviceAttributeWallClockRate)
  struct SpmmRec {
    hipEvent_t e0, e1;
    int s;
    int slot;                          // stamps slot, or -1 (events)
  };
  std::vector<SpmmRec> spmm_log;
};

namespace {

// A workspace grown on demand: at least `need` doubles behind *buf (*have of them
// now; the contents do not survive a growth).
int grow(double** buf, size_t* have, size_t need) {
  if (*have >= need) return 0;
  if (*buf) HIP_TRY(hipFree(*buf));
  *buf = nullptr;
  *have = 0;
  HIP_TRY(hipMalloc(buf, sizeof(double) * need));
  *have = need;
  return 0;
}

int build_window(gpmi_sp* sp);

// The X windows of the window SpMMs, built once (under win_mu); a failed build
// frees its buffers, so a retry allocates afresh.
int ensure_window(gpmi_sp* sp) {
  if (sp->win_maxu.load(std::memory_order_acquire) >= 0) return 0;
  std::lock_guard<std::mutex> lock(sp->win_mu);
  if (sp->win_maxu.load(std::memory_order_acquire) >= 0) return 0;
  const int rc = build_window(sp);
  if (rc) {
    if (sp->win_cols) (void)hipFree(sp->win_cols);
    if (sp->win_u) (void)hipFree(sp->win_u);
    if (sp->win_lidx) (void)hipFree(sp->win_lidx);
    sp->win_cols = nullptr;
    sp->win_u = nullptr;
    sp->win_lidx = nullptr;
  }
  return rc;
}

int build_window(gpmi_sp* sp) {
  const int64_t nblk = (sp->n + WIN_ROWS - 1) / WIN_ROWS;
  HIP_TRY(hipMalloc(&sp->win_cols, sizeof(int) * (size_t)nblk * WIN_MAXU));
  HIP_TRY(hipMalloc(&sp->win_u, sizeof(int) * (size_t)nblk));
  HIP_TRY(hipMalloc(&sp->win_lidx, sizeof(unsigned short) * (size_t)std::max<int64_t>(1, sp->nnz)));
  hipLaunchKernelGGL(spmm_window_build_kernel, dim3((unsigned)nblk), dim3(256), 0, sp->stream,
                     sp->indptr, sp->indices, sp->n, sp->win_cols, sp->win_u, sp->win_lidx);
  LAUNCH_CHECK("spmm_window_build_kernel");
  std::vector<int> hu((size_t)nblk);
  HIP_TRY(hipMemcpyAsync(hu.data(), sp->win_u, sizeof(int) * nblk, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  int mu = 0;
  for (int v : hu) mu = std::max(mu, v);
  {
    double su = 0.0;
    for (int v : hu) su += v;
    sp->win_mean = su / (double)nblk;
  }
  std::vector<int64_t> hp((size_t)sp->n + 1);
  HIP_TRY(hipMemcpy(hp.data(), sp->indptr, sizeof(int64_t) * (sp->n + 1), hipMemcpyDeviceToHost));
  int mm = 0;
  for (int64_t b = 0; b < nblk; ++b)
    if (hu[(size_t)b] > 0) {
      const int64_t r0 = b * WIN_ROWS, r1 = std::min<int64_t>(r0 + WIN_ROWS, sp->n);
      mm = std::max<int>(mm, (int)(hp[(size_t)r1] - hp[(size_t)r0]));
    }
  sp->win_maxm = mm;
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
  sp->win_use = lds <= 32 * 1024;
  if (lds > 160 * 1024) return set_error(-1104, "spmm window exceeds LDS");
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&csr_spmm_win_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (auto f : kWing)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(f),
                               hipFuncAttributeMaxDynamicSharedMemorySize, WING_MAX_LDS));
  sp->win_nblk = nblk;
  sp->win_maxu.store(mu, std::memory_order_release);
  return 0;
}

// The SpMM kernel for an s-column block (0 gather, 1 windowed chunks, 3 gather by
// column pairs, 5 window with latency-hidden staging; 2, the round-2 one-pass
// window, is superseded by 5). GPMI_SPMM_WINDOW: 0 the gather-from-X
// kernel, 2 the windowed kernel, unset or 1 the faster one for this matrix
// (win_use); GPMI_SPMM_PAIR=0
// keeps the one-column gather for even s (the pair kernel also needs 16-byte
// aligned blocks, else the one-column gather runs).
int spmm_kind(gpmi_sp* sp, int s, int* kind) {
  if (sp->dK) {
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
      sp->win_maxu.load(std::memory_order_acquire) > 0 &&
      sizeof(double) * (size_t)std::max(sp->win_maxu.load(std::memory_order_acquire),
                                        WIN_ROWS) * s <= (size_t)WING_MAX_LDS) {
    *kind = 5;
    return 0;
  }
  if (wmode == 2 || (wmode != 0 && sp->win_use)) *kind = 1;
  const char* penv = std::getenv("GPMI_SPMM_PAIR");
  if (*kind == 0 && s % 2 == 0 && s <= 64 && !(penv && std::atoi(penv) == 0)) *kind = 3;
  return 0;
}

// Y = (K + eta I) X. With pqp, a kernel that can also writes the per-block partials
// X . Y per column (pqp[block][s], the multi-shift CG's p . q) and sets *pq_blocks to
// their count; otherwise *pq_blocks = 0 and the caller forms them.
int spmm_launch(gpmi_sp* sp, const double* X, double* Y, int s, double eta, hipStream_t st,
                double* pqp, int* pq_blocks, int dots2, unsigned long long* stamp = nullptr) {
  if (pq_blocks) *pq_blocks = 0;
  if (sp->dK) {
    // dense: split partials of K X on fp64 MFMA, summed in split order (+ eta X)
    double* Yp = st == sp->ms_stream ? sp->dYp_ms : sp->dYp;
    const dim3 grid((unsigned)((sp->n + 63) / 64), (unsigned)sp->dsplit);
    if (s <= 16)
      hipLaunchKernelGGL(dense_mm_kernel<1>, grid, dim3(256), 0, st, sp->dK, sp->dld, sp->n, X, s,
                         sp->dkcs, Yp);
    else
      hipLaunchKernelGGL(dense_mm_kernel<2>, grid, dim3(256), 0, st, sp->dK, sp->dld, sp->n, X, s,
                         sp->dkcs, Yp);
    LAUNCH_CHECK("dense_mm_kernel");
    const int64_t ns = sp->n * s;
    hipLaunchKernelGGL(dense_mm_reduce_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st,
                       Yp, sp->dsplit, ns, X, eta, Y);
    LAUNCH_CHECK("dense_mm_reduce_kernel");
    return 0;
  }
  int kind = 0;
  if (int rc = spmm_kind(sp, s, &kind)) return rc;
  // the window kernel stages even-width rows of X with 16-byte loads: an 8-byte
  // aligned block handed in directly takes the one-column gather instead
  if (kind == 5 && s % 2 == 0 &&
      ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 15) != 0)
    kind = 0;
  if (kind == 5) {
    // the window, and the epilogue's [64][s] rows of X . Y (pqp), with dots2 its
    // [64][2s] rows of X . Y and X . X (the Chronopoulos-Gear multi-shift CG)
    const size_t lds = sizeof(double) * (size_t)s *
                       (size_t)std::max(sp->win_maxu.load(std::memory_order_acquire),
                                        (dots2 ? 2 : 1) * WIN_ROWS);
    auto kfn = kWing[s - 1];
    const int tpr = WING_TPR;
    hipLaunchKernelGGL(kfn, dim3((unsigned)sp->win_nblk), dim3(64 * tpr), lds, st, sp->indptr,
                       sp->indices, sp->win_lidx, sp->data, sp->n, sp->win_cols, sp->win_u, X, Y,
                       eta, pqp, dots2, stamp);
    LAUNCH_CHECK("csr_spmm_wing_kernel");
    if (pqp && pq_blocks) *pq_blocks = (int)sp->win_nblk;
    return 0;
  }
  if (kind == 1) {
    // window + the largest windowed block's values, positions and row starts
    const size_t lds = sizeof(double) * WIN_CS *
                           (size_t)std::max(1, sp->win_maxu.load(std::memory_order_acquire)) +
                       10 * (size_t)sp->win_maxm + 4 + sizeof(int) * (WIN_ROWS + 1);
    hipLaunchKernelGGL(csr_spmm_win_kernel,
                       dim3((unsigned)sp->win_nblk),
                       dim3(256), lds, st, sp->indptr, sp->indices, sp->win_lidx, sp->data,
                       sp->n, sp->win_cols, sp->win_u, X, (int64_t)s, Y, (int64_t)s, s, eta);
    LAUNCH_CHECK("csr_spmm_win_kernel");
    return 0;
  }
  if (kind == 3 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 &&
      (reinterpret_cast<uintptr_t>(Y) & 15) == 0) {
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

int take_event(gpmi_sp* sp, hipEvent_t* e) {
  if (!sp->ev_pool.empty()) {
    *e = sp->ev_pool.back();
    sp->ev_pool.pop_back();
    return 0;
  }
  HIP_TRY(hipEventCreateWithFlags(e, gpmi::timing_event_flags()));
  return 0;
}

constexpr int STAMP_CAP = 8192;            // stamped window-SpMM launches per timing window
constexpr size_t STAMP_BYTES = 256u << 20;   // at most this much stamp buffer

// Y = (K + eta I) X (spmm_launch); with in-step timing on (gpmi_sp_set_timing) the
// window SpMM stamps its span into the next slot, other kinds are bracketed by a
// HIP event pair on their stream.
int spmm(gpmi_sp* sp, const double* X, double* Y, int s, double eta, hipStream_t st = nullptr,
         double* pqp = nullptr, int* pq_blocks = nullptr, int dots2 = 0) {
  if (!st) st = sp->stream;
  if (!sp->timing) return spmm_launch(sp, X, Y, s, eta, st, pqp, pq_blocks, dots2);
  gpmi_sp::SpmmRec rec{nullptr, nullptr, s, -1};
  int kind = 0;
  if (int rc = spmm_kind(sp, s, &kind)) return rc;
  const bool stamped =
      kind == 5 && !sp->dK &&
      !(s % 2 == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 15));
  {
    std::lock_guard<std::mutex> lock(sp->timing_mu);
    if (stamped && sp->stamps_used < sp->stamp_cap) {
      rec.slot = sp->stamps_used++;
    } else {
      if (int rc = take_event(sp, &rec.e0)) return rc;
      if (int rc = take_event(sp, &rec.e1)) return rc;
    }
  }
  if (rec.slot < 0) HIP_TRY(hipEventRecord(rec.e0, st));
  if (int rc = spmm_launch(sp, X, Y, s, eta, st, pqp, pq_blocks, dots2,
                           rec.slot >= 0 ? sp->stamps + 2 * sp->win_nblk * rec.slot : nullptr))
    return rc;
  if (rec.slot < 0) HIP_TRY(hipEventRecord(rec.e1, st));
  std::lock_guard<std::mutex> lock(sp->timing_mu);
  sp->spmm_log.push_back(rec);
  return 0;
}

// out[j][c] = sum_i A_j[i][c] B[i][c], j < J  (device out)
int col_dots(gpmi_sp* sp, const double* A, int64_t strideA, int J, const double* B, int s,
             double* out, double* partial = nullptr, hipStream_t st = nullptr) {
  if (!partial) {
    int rc = grow(&sp->partial, &sp->partial_doubles, (size_t)NBLK * J * s);
    if (rc) return rc;
    partial = sp->partial;
  }
  if (!st) st = sp->stream;
  hipLaunchKernelGGL(col_dot_partial_kernel, dim3(NBLK, J), dim3(256), 0, st, A, strideA,
                     B, sp->n, s, partial);
  LAUNCH_CHECK("col_dot_partial_kernel");
  hipLaunchKernelGGL(col_dot_reduce_kernel, dim3((J * s + 3) / 4), dim3(256), 0, st,
                     partial, NBLK, J, s, out);
  LAUNCH_CHECK("col_dot_reduce_kernel");
  return 0;
}

unsigned grid_ns(int64_t n, int s) { return (unsigned)((n * s + 255) / 256); }

// device row r <- original row orig(r)
inline int64_t orig_row(const gpmi_sp* sp, int64_t r) {
  return sp->perm.empty() ? r : (int64_t)sp->perm[r];
}

// Morton (Z-order) key of a cell's integer coordinates (d <= 3, 21 bits each).
uint64_t morton3(const int64_t (&q)[3], int d) {
  uint64_t key = 0;
  for (int b = 20; b >= 0; --b)
    for (int k = 0; k < d; ++k) key = (key << 1) | (uint64_t)((q[k] >> b) & 1);
  return key;
}

// Lanczos of K on s probe columns starting from V0 (already in V block 0).
// alpha/beta: host [s][steps] (column-major by probe). orth < 0: CGS2 against every
// previous vector (full reorthogonalisation); orth = 0: the plain three-term
// recurrence (one projection on v_k after subtracting beta v_{k-1}: imate's
// orthogonalize=0); orth > 0: CGS2 against the last orth vectors and v_k.
int lanczos_block(gpmi_sp* sp, double* V, double* W, int s, int steps, double* h_alpha,
                  double* h_beta, int orth = -1) {
  const int64_t ns = sp->n * s;
  // device scalars: H1, H2 [(steps+1)][MAXS] (the two CGS2 passes), norms, the
  // alpha/beta tables [s][steps], two axpby coefficient pairs and the dead flags
  const size_t need = (size_t)2 * (steps + 1) * MAXS + MAXS + (size_t)2 * MAXS * steps +
                      4 * MAXS + MAXS;
  if (int rc = grow(&sp->lz, &sp->lz_doubles, need)) return rc;
  double* H1 = sp->lz;
  double* H2 = H1 + (size_t)(steps + 1) * MAXS;
  double* nrm = H2 + (size_t)(steps + 1) * MAXS;
  double* dalpha = nrm + MAXS;
  double* dbeta = dalpha + (size_t)MAXS * steps;
  double* ca = dbeta + (size_t)MAXS * steps;
  double* cb = ca + MAXS;
  double* na = cb + MAXS;
  double* nb = na + MAXS;
  int* dead = reinterpret_cast<int*>(nb + MAXS);
  // one pass (orth = 0): the second pass's coefficients stay zero
  if (orth == 0) HIP_TRY(hipMemsetAsync(H2, 0, sizeof(double) * MAXS, sp->stream));
  for (int k = 0; k < steps; ++k) {
    double* Vk = V + (int64_t)k * ns;
    const int jlo = orth < 0 ? 0 : std::max(0, k - orth);   // projection window [jlo, k]
    const int J = k + 1 - jlo;
    int rc = spmm(sp, Vk, W, s, 0.0);
    if (rc) return rc;
    if (k > 0) {   // W -= beta_{k-1} V_{k-1}
      hipLaunchKernelGGL(col_axpby_kernel, dim3(grid_ns(sp->n, s)), dim3(256), 0, sp->stream,
                         V + (int64_t)(k - 1) * ns, W, na, nb, sp->n, s);
      LAUNCH_CHECK("col_axpby_kernel");
    }
    for (int pass = 0; pass < (orth == 0 ? 1 : 2); ++pass) {   // CGS(2) against V_jlo .. V_k
      double* H = pass == 0 ? H1 : H2;
      rc = col_dots(sp, V + (int64_t)jlo * ns, ns, J, W, s, H);
      if (rc) return rc;
      hipLaunchKernelGGL(col_gs_update_kernel, dim3((unsigned)((ns + 511) / 512)), dim3(256), 0,
                         sp->stream, W, V + (int64_t)jlo * ns, ns, H, J, sp->n, s);
      LAUNCH_CHECK("col_gs_update_kernel");
    }
    rc = col_dots(sp, W, 0, 1, W, s, nrm);
    if (rc) return rc;
    hipLaunchKernelGGL(lanczos_scalar_kernel, dim3(1), dim3(64), 0, sp->stream,
                       H1 + (size_t)(k - jlo) * s, orth == 0 ? H2 : H2 + (size_t)(k - jlo) * s,
                       nrm, s, k, steps, dead, dalpha, dbeta, ca, cb, na, nb);
    LAUNCH_CHECK("lanczos_scalar_kernel");
    if (k + 1 < steps) {
      // V_{k+1} = W / beta  (b = 0 -> X * 0 + 0 * Y; Y is zero-initialised below)
      double* Vn = V + (int64_t)(k + 1) * ns;
      HIP_TRY(hipMemsetAsync(Vn, 0, sizeof(double) * ns, sp->stream));
      hipLaunchKernelGGL(col_axpby_kernel, dim3(grid_ns(sp->n, s)), dim3(256), 0, sp->stream, W,
                         Vn, ca, cb, sp->n, s);
      LAUNCH_CHECK("col_axpby_kernel");
    }
  }
  HIP_TRY(hipMemcpyAsync(h_alpha, dalpha, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipMemcpyAsync(h_beta, dbeta, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

// Lanczos of K on s probe columns by the plain three-term recurrence (imate's
// orthogonalize = 0; lz0_*_kernel in gpmi_sparse.hip): three launches per step (the
// SpMM with u . Ku in its epilogue, the per-column scalars, one update pass over three
// vectors with the next norm and overlap partials), the vectors unnormalised. U:
// three rotating blocks [n][s] (U[0] = the normalised probes), Y one block.
// alpha / beta: host [s][steps].
int lanczos_block_plain(gpmi_sp* sp, double* U, double* Y, int s, int steps, double* h_alpha,
                        double* h_beta) {
  const int64_t n = sp->n, ns = n * s;
  const int nb = (int)((n + 63) / 64);
  const size_t need = 5 * (size_t)s + 2 * (size_t)s * steps + s;
  if (int rc = grow(&sp->lz, &sp->lz_doubles, need)) return rc;
  double* st = sp->lz;
  double* coef = st + 2 * s;
  double* dal = coef + 3 * s;
  double* dbe = dal + (size_t)s * steps;
  int* dead = reinterpret_cast<int*>(dbe + (size_t)s * steps);
  int rc = grow(&sp->partial, &sp->partial_doubles, (size_t)nb * 3 * s);
  if (rc) return rc;
  double* pq = sp->partial;                 // [s][nb]: u_k . y
  double* pv = pq + (size_t)nb * s;         // [2][s][nb]: ||u_{k+1}||^2, u_{k+1} . u_k
  HIP_TRY(hipMemsetAsync(dbe, 0, sizeof(double) * s * steps, sp->stream));
  // u_{-1}: zero (its coefficient is 0 at k = 0; 0 * garbage could be NaN)
  HIP_TRY(hipMemsetAsync(U + 2 * ns, 0, sizeof(double) * ns, sp->stream));
  const unsigned sgrid = (unsigned)s;   // lz0_alpha_kernel: one workgroup per column
  for (int k = 0; k < steps; ++k) {
    double* Uc = U + (int64_t)(k % 3) * ns;
    double* Un = U + (int64_t)((k + 1) % 3) * ns;
    double* Up = U + (int64_t)((k + 2) % 3) * ns;
    int pqb = 0;
    rc = spmm(sp, Uc, Y, s, 0.0, sp->stream, pq, &pqb);
    if (rc) return rc;
    if (pqb != nb) {
      hipLaunchKernelGGL(lz0_dot64_kernel, dim3((unsigned)nb), dim3(256), 0, sp->stream, Uc, Y, n,
                         s, pq);
      LAUNCH_CHECK("lz0_dot64_kernel");
    }
    hipLaunchKernelGGL(lz0_alpha_kernel, dim3(sgrid), dim3(256), 0, sp->stream, pq, pv, nb, s, k,
                       steps, st, dead, dal, dbe, coef);
    LAUNCH_CHECK("lz0_alpha_kernel");
    hipLaunchKernelGGL(lz0_update_kernel, dim3((unsigned)nb), dim3(256), 0, sp->stream, Y, Up, Uc,
                       Un, coef, n, s, pv);
    LAUNCH_CHECK("lz0_update_kernel");
  }
  hipLaunchKernelGGL(lz0_alpha_kernel, dim3(sgrid), dim3(256), 0, sp->stream, pq, pv, nb, s, steps,
                     steps, st, dead, dal, dbe, coef);
  LAUNCH_CHECK("lz0_alpha_kernel");
  HIP_TRY(hipMemcpyAsync(h_alpha, dal, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipMemcpyAsync(h_beta, dbe, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

constexpr int LZ_NB = 512;   // row blocks of the DCGS2 dot partials (fixed: deterministic)

// Lanczos of K on s probe columns from V block 0 (normalised probes) with DCGS2
// reorthogonalisation (lz_*_kernel in gpmi_sparse.hip): per step one SpMM, one dot
// pass and one update pass over the basis. V: steps blocks [n][s]; U, Y: one block
// each. alpha / beta: host [s][steps]. *inexact: a column lost more than six digits
// of rho to cancellation (the caller reruns the block with CGS2).
int lanczos_block_dcgs2(gpmi_sp* sp, double* V, double* U, double* Y, int s, int steps,
                        double* h_alpha, double* h_beta, bool* inexact) {
  const int64_t n = sp->n, ns = n * s;
  const size_t hsz = (size_t)(steps + 2) * (steps + 1);
  const size_t need = (size_t)s * hsz + (size_t)(2 * steps + 2) * s + (size_t)steps * s +
                      (size_t)(steps + 1) * s + 2 * (size_t)s + 2 * (size_t)s * steps + 2 * s;
  if (int rc = grow(&sp->lzd, &sp->lzd_doubles, need)) return rc;
  double* H = sp->lzd;
  double* d = H + (size_t)s * hsz;
  double* cv = d + (size_t)(2 * steps + 2) * s;
  double* cu = cv + (size_t)steps * s;
  double* ir = cu + (size_t)(steps + 1) * s;
  double* rho = ir + s;
  double* dal = rho + s;
  double* dbe = dal + (size_t)s * steps;
  int* dead = reinterpret_cast<int*>(dbe + (size_t)s * steps);
  int* inex = dead + s;
  // row blocks of the dot partials (fixed: deterministic; 256 / 1024 / 2048 measured
  // 2-5 % slower at cfg 5)
  const int lz_nb = LZ_NB;
  int rc = grow(&sp->partial, &sp->partial_doubles, (size_t)lz_nb * (2 * steps + 2) * s);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(H, 0, sizeof(double) * s * hsz, sp->stream));
  HIP_TRY(hipMemsetAsync(dal, 0, sizeof(double) * 2 * s * steps, sp->stream));
  HIP_TRY(hipMemcpyAsync(U, V, sizeof(double) * ns, hipMemcpyDeviceToDevice, sp->stream));
  // non-temporal basis reads for a basis over twice the 256 MB Infinity Cache (cfg 5
  // Lanczos 13.0 -> 11.2 ms; at cfg 4's 0.3 GB they measured slower, 6.8 -> 7.0 ms)
  const bool lz_nt = sizeof(double) * (double)ns * (steps + 1) > 512.0 * 1024 * 1024;
  for (int k = 0; k <= steps; ++k) {
    const bool last = k == steps;
    if (!last) {
      rc = spmm(sp, U, Y, s, 0.0);
      if (rc) return rc;
    }
    const int nv = 2 * k + 2;
    for (int j0 = 0; j0 == 0 || j0 < k; j0 += LZ_JC) {
      // (column pairs with 16-byte loads measured slower: 15.9 against 13.1 ms per
      // cfg 5 Lanczos, at half the occupancy for the doubled accumulators)
      hipLaunchKernelGGL(lz_nt ? lz_dots_kernel<true> : lz_dots_kernel<false>, dim3(lz_nb),
                         dim3(256), 0, sp->stream, V, ns, k, j0, U,
                         last ? (const double*)nullptr : Y, n, s, nv, sp->partial);
      LAUNCH_CHECK("lz_dots_kernel");
    }
    hipLaunchKernelGGL(col_dot_reduce_kernel, dim3((nv * s + 3) / 4), dim3(256), 0, sp->stream,
                       sp->partial, lz_nb, nv, s, d);
    LAUNCH_CHECK("col_dot_reduce_kernel");
    const size_t sdb = sizeof(double) * (size_t)(2 * k + 2) * s;   // the dots in LDS
    const int stage = sdb <= 64 * 1024 ? 1 : 0;
    hipLaunchKernelGGL(lz_scalar_kernel, dim3(1), dim3(1024), stage ? sdb : 0, sp->stream, d, k,
                       steps, s, H, cv, cu, ir, rho, dead, inex, dal, dbe, stage);
    LAUNCH_CHECK("lz_scalar_kernel");
    if (!last) {
      // four row chunks per thread sharing its two columns' coefficients (cfg 5 Lanczos
      // 13.7 -> 12.65 ms against one): the grid's thread-pair count P with 2 P a
      // multiple of s
      const int64_t q = s / std::__gcd(512, s);
      int64_t g = (ns / 2 + 1023) / 1024;
      g = (g + q - 1) / q * q;
      auto kfn = lz_nt ? lz_update_kernel<4, true> : lz_update_kernel<4, false>;
      hipLaunchKernelGGL(kfn, dim3((unsigned)g), dim3(256), 0, sp->stream, V, ns, k, U, Y, cv, cu,
                         ir, s);
      LAUNCH_CHECK("lz_update_kernel");
    }
  }
  std::vector<int> hin(s);
  HIP_TRY(hipMemcpyAsync(h_alpha, dal, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipMemcpyAsync(h_beta, dbe, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipMemcpyAsync(hin.data(), inex, sizeof(int) * s, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  *inexact = false;
  for (int c = 0; c < s; ++c) *inexact = *inexact || hin[c];
  return 0;
}

}  // namespace

extern "C" {

int gpmi_sp_create_csr(int device, int64_t n, const int64_t* indptr, const int* indices,
                       const double* data, gpmi_sp** out) {
  if (!out || n <= 0) return set_error(-1100, "invalid arguments");
  DeviceGuard g(device);
  gpmi_sp* sp = new gpmi_sp();
  sp->device = device;
  sp->n = n;
  sp->nnz = indptr[n];
  HIP_TRY(hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc(&sp->indptr, sizeof(int64_t) * (n + 1)));
  HIP_TRY(hipMalloc(&sp->indices, sizeof(int) * std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(hipMalloc(&sp->data, sizeof(double) * std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(hipMalloc(&sp->small, sizeof(double) * 16384));
  HIP_TRY(hipMemcpy(sp->indptr, indptr, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(sp->indices, indices, sizeof(int) * sp->nnz, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(sp->data, data, sizeof(double) * sp->nnz, hipMemcpyHostToDevice));
  *out = sp;
  return 0;
}

int gpmi_sp_create_matern(int device, const double* points, int64_t n, int d,
                          const double* scale, double nu, double tau, gpmi_sp** out) {
  if (!out || n <= 0) return set_error(-1100, "invalid arguments");
  if (d < 1 || d > GPMI_MAX_DIM) return set_error(-1003, "dimension outside [1, 8]");
  MaternParams P;
  int rc = matern_params_host(nu, &P);
  if (rc) return rc;
  DeviceGuard g(device);
  gpmi_sp* sp = new gpmi_sp();
  sp->device = device;
  sp->n = n;
  sp->tau = tau;
  HIP_TRY(hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc(&sp->small, sizeof(double) * 16384));
  hipStream_t st = sp->stream;
  // Scaled-distance cutoff: smallest grid x with matern(x) <= tau, with margin.
  // matern is decreasing, so every pair beyond xcut has matern < tau.
  const int M = 4096;
  double xmax = 1.0, xcut = 0.0;
  std::vector<double> hx(M), hv(M);
  double* dx = sp->small;
  double* dv = sp->small + M;
  for (int it = 0; it < 60; ++it) {
    for (int i = 0; i < M; ++i) hx[i] = xmax * (i + 1) / M;
    HIP_TRY(hipMemcpyAsync(dx, hx.data(), sizeof(double) * M, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(matern_eval_kernel, dim3(M / 256), dim3(256), 0, st, dx, (int64_t)M, P, dv);
    LAUNCH_CHECK("matern_eval_kernel");
    HIP_TRY(hipMemcpyAsync(hv.data(), dv, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int first = -1;
    for (int i = 0; i < M; ++i)
      if (hv[i] <= tau) {
        first = i;
        break;
      }
    if (first >= 0) {
      xcut = hx[first] * (1.0 + 1e-6) + xmax / M;
      break;
    }
    xmax *= 2.0;
  }
  if (xcut == 0.0) return set_error(-1101, "taper threshold not reached (tau too small)");
  double *dp = nullptr, *ds = nullptr;
  int* dcnt = nullptr;
  HIP_TRY(hipMalloc(&dp, sizeof(double) * n * d));
  HIP_TRY(hipMalloc(&ds, sizeof(double) * 2 * GPMI_MAX_DIM));   // [scale | 1 / scale]
  HIP_TRY(hipMalloc(&dcnt, sizeof(int) * n));
  HIP_TRY(hipMemcpyAsync(dp, points, sizeof(double) * n * d, hipMemcpyHostToDevice, st));
  std::vector<double> hsc(2 * GPMI_MAX_DIM, 1.0);
  for (int k = 0; k < d; ++k) {
    hsc[k] = scale[k];
    hsc[GPMI_MAX_DIM + k] = 1.0 / scale[k];
  }
  HIP_TRY(hipMemcpyAsync(ds, hsc.data(), sizeof(double) * hsc.size(), hipMemcpyHostToDevice, st));
  const unsigned grid = (unsigned)((n + 3) / 4);
  // Cell list (d <= 3): cells of width >= xcut * scale_k, so a kept pair is in the
  // same or an adjacent cell; coarsened while there are more cells than 4 n.
  // GPMI_SPARSE_BRUTE=1 forces the all-pairs kernels (A/B and tests).
  const char* brute_env = std::getenv("GPMI_SPARSE_BRUTE");
  bool cells = d <= 3 && n < (int64_t)1 << 28 && !(brute_env && std::atoi(brute_env) != 0);
  int* dcell = nullptr;   // [n] cell of each point, then gdim [d], cell_start, perm
  int *dgdim = nullptr, *dstart = nullptr, *dperm = nullptr;
  std::vector<int> lorder;   // locality order of the rows (Morton order of the cells)
  if (cells) {
    double pmin[3], pmax[3], wid[3];
    int64_t G[3] = {1, 1, 1};
    for (int k = 0; k < d; ++k) {
      pmin[k] = pmax[k] = points[k];
      for (int64_t i = 0; i < n; ++i) {
        const double v = points[i * d + k];
        if (!std::isfinite(v)) cells = false;   // NaN / inf points: all-pairs kernels
        pmin[k] = std::min(pmin[k], v);
        pmax[k] = std::max(pmax[k], v);
      }
      wid[k] = xcut * std::fabs(scale[k]) * (1.0 + 1e-9);
      if (!(wid[k] > 0.0) || !std::isfinite(wid[k])) cells = false;
    }
    int64_t total = 0;
    for (int it = 0; cells && it < 64; ++it) {
      total = 1;
      for (int k = 0; k < d; ++k) {
        const double g = std::floor((pmax[k] - pmin[k]) / wid[k]) + 1.0;
        G[k] = g > 1e9 ? (int64_t)1e9 : (int64_t)g;
        total = std::min<int64_t>(total * G[k], (int64_t)1 << 40);
      }
      if (total <= std::max<int64_t>(4 * n, 1024)) break;
      for (int k = 0; k < d; ++k) wid[k] *= 2.0;
    }
    if (cells && total > std::max<int64_t>(4 * n, 1024)) cells = false;
    if (cells) {
      std::vector<int> hcell(n), hstart(total + 1, 0), hperm(n), hg(d);
      for (int k = 0; k < d; ++k) hg[k] = (int)G[k];
      for (int64_t i = 0; i < n; ++i) {
        int64_t c = 0, mul = 1;
        for (int k = 0; k < d; ++k) {
          int64_t q = (int64_t)std::floor((points[i * d + k] - pmin[k]) / wid[k]);
          q = std::min<int64_t>(std::max<int64_t>(q, 0), G[k] - 1);
          c += q * mul;
          mul *= G[k];
        }
        hcell[i] = (int)c;
        ++hstart[c + 1];
      }
      for (int64_t c = 0; c < total; ++c) hstart[c + 1] += hstart[c];
      std::vector<int> fillp(hstart.begin(), hstart.end() - 1);
      for (int64_t i = 0; i < n; ++i) hperm[fillp[hcell[i]]++] = (int)i;   // ascending i per cell
      // GPMI_SPARSE_REORDER=0 keeps the rows in the original order
      const char* ro = std::getenv("GPMI_SPARSE_REORDER");
      if (!(ro && std::atoi(ro) == 0) && n > 1) {
        std::vector<std::pair<uint64_t, int64_t>> keys;
        keys.reserve(total);
        for (int64_t c = 0; c < total; ++c) {
          if (hstart[c + 1] == hstart[c]) continue;
          int64_t q[3] = {0, 0, 0}, cc = c;
          for (int k = 0; k < d; ++k) {
            q[k] = cc % G[k];
            cc /= G[k];
          }
          keys.emplace_back(morton3(q, d), c);
        }
        std::sort(keys.begin(), keys.end());
        lorder.reserve(n);
        for (const auto& kc : keys)
          for (int q = hstart[kc.second]; q < hstart[kc.second + 1]; ++q) lorder.push_back(hperm[q]);
      }
      HIP_TRY(hipMalloc(&dcell, sizeof(int) * (2 * n + d + total + 1)));
      dgdim = dcell + n;
      dstart = dgdim + d;
      dperm = dstart + total + 1;
      HIP_TRY(hipMemcpyAsync(dcell, hcell.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dgdim, hg.data(), sizeof(int) * d, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dstart, hstart.data(), sizeof(int) * (total + 1),
                            hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dperm, hperm.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));   // host vectors go out of scope
    }
  }
  if (cells) {
    hipLaunchKernelGGL(csr_cell_count_kernel, dim3(grid), dim3(256), 0, st, dp, n, d, ds, P, tau,
                       xcut, dcell, dgdim, dstart, dperm, dcnt);
    LAUNCH_CHECK("csr_cell_count_kernel");
  } else {
    hipLaunchKernelGGL(csr_count_kernel, dim3(grid), dim3(256), 0, st, dp, n, d, ds, P, tau, xcut,
                       dcnt);
    LAUNCH_CHECK("csr_count_kernel");
  }
  std::vector<int> cnt(n);
  HIP_TRY(hipMemcpyAsync(cnt.data(), dcnt, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (cells && *std::max_element(cnt.begin(), cnt.end()) > CELL_CAP_HOST) cells = false;
  std::vector<int64_t> ip(n + 1, 0);
  for (int64_t i = 0; i < n; ++i) ip[i + 1] = ip[i] + cnt[i];
  sp->nnz = ip[n];
  HIP_TRY(hipMalloc(&sp->indptr, sizeof(int64_t) * (n + 1)));
  HIP_TRY(hipMalloc(&sp->indices, sizeof(int) * std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(hipMalloc(&sp->data, sizeof(double) * std::max<int64_t>(1, sp->nnz)));
  HIP_TRY(hipMemcpyAsync(sp->indptr, ip.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice,
                        st));
  if (cells) {
    hipLaunchKernelGGL(csr_cell_fill_kernel, dim3(grid), dim3(256), 0, st, dp, n, d, ds, P, tau,
                       xcut, dcell, dgdim, dstart, dperm, sp->indptr, sp->indices, sp->data);
    LAUNCH_CHECK("csr_cell_fill_kernel");
  } else {   // all pairs (d > 3, or a row holds more than CELL_CAP kept entries)
    hipLaunchKernelGGL(csr_fill_kernel, dim3(grid), dim3(256), 0, st, dp, n, d, ds, P, tau, xcut,
                       sp->indptr, sp->indices, sp->data);
    LAUNCH_CHECK("csr_fill_kernel");
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (cells && (int64_t)lorder.size() == n) {
    // rows (and columns) renumbered in the locality order: K' = P K P^T
    std::vector<int> inv(n);
    for (int64_t r = 0; r < n; ++r) inv[lorder[r]] = (int)r;
    std::vector<int64_t> ip2(n + 1, 0);
    for (int64_t r = 0; r < n; ++r) ip2[r + 1] = ip2[r] + cnt[lorder[r]];
    int* dpi = nullptr;
    int64_t* dip2 = nullptr;
    int* dix2 = nullptr;
    double* ddv2 = nullptr;
    HIP_TRY(hipMalloc(&sp->perm_d, sizeof(int) * n));
    HIP_TRY(hipMalloc(&dpi, sizeof(int) * n));
    HIP_TRY(hipMalloc(&dip2, sizeof(int64_t) * (n + 1)));
    HIP_TRY(hipMalloc(&dix2, sizeof(int) * std::max<int64_t>(1, sp->nnz)));
    HIP_TRY(hipMalloc(&ddv2, sizeof(double) * std::max<int64_t>(1, sp->nnz)));
    HIP_TRY(hipMemcpyAsync(sp->perm_d, lorder.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dpi, inv.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dip2, ip2.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(csr_permute_kernel, dim3(grid), dim3(256), 0, st, sp->indptr, sp->indices,
                       sp->data, sp->perm_d, dpi, n, dip2, dix2, ddv2);
    LAUNCH_CHECK("csr_permute_kernel");
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipFree(sp->indptr));
    HIP_TRY(hipFree(sp->indices));
    HIP_TRY(hipFree(sp->data));
    HIP_TRY(hipFree(dpi));
    sp->indptr = dip2;
    sp->indices = dix2;
    sp->data = ddv2;
    sp->perm = std::move(lorder);
  }
  if (dcell) HIP_TRY(hipFree(dcell));
  HIP_TRY(hipFree(dp));
  HIP_TRY(hipFree(ds));
  HIP_TRY(hipFree(dcnt));
  *out = sp;
  return 0;
}

int gpmi_sp_create_dense(gpmi_op* op, gpmi_sp** out) {
  if (!out) return set_error(-1004, "null output handle");
  OpView v;
  int rc = op_view(op, &v);
  if (rc) return rc;
  if (!v.has_K) return set_error(-1000, "operator has no matrix (load or assemble first)");
  DeviceGuard g(v.device);
  gpmi_sp* sp = new gpmi_sp();
  sp->device = v.device;
  sp->n = v.n;
  sp->nnz = v.n * v.n;
  sp->dK = v.K;
  sp->dld = v.n_pad;
  // k splits: about 1024 workgroups (row blocks x splits) keep the HBM stream busy
  const int64_t nch = (v.n + 63) / 64;
  int split = (int)std::min<int64_t>(16, std::max<int64_t>(1, (1024 + nch - 1) / nch));
  split = (int)std::min<int64_t>(split, nch);
  sp->dkcs = (int)((nch + split - 1) / split);
  sp->dsplit = (int)((nch + sp->dkcs - 1) / sp->dkcs);
  auto fail = [&](hipError_t e, const char* what) {
    char b[300];
    snprintf(b, sizeof(b), "%s failed: %s", what, hipGetErrorString(e));
    gpmi_sp_destroy(sp);
    return set_error(-(int)e, b);
  };
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking)) != hipSuccess)
    return fail(e, "stream");
  const size_t part = sizeof(double) * (size_t)sp->dsplit * (size_t)sp->n * MAXS;
  if ((e = hipMalloc(&sp->small, sizeof(double) * 16384)) != hipSuccess) return fail(e, "small");
  if ((e = hipMalloc(&sp->dYp, part)) != hipSuccess) return fail(e, "dense partials");
  if ((e = hipMalloc(&sp->dYp_ms, part)) != hipSuccess) return fail(e, "dense partials");
  *out = sp;
  return 0;
}

int gpmi_sp_destroy(gpmi_sp* sp) {
  if (!sp) return 0;
  DeviceGuard g(sp->device);
  if (sp->stream) (void)hipStreamSynchronize(sp->stream);
  if (sp->dYp) (void)hipFree(sp->dYp);
  if (sp->dYp_ms) (void)hipFree(sp->dYp_ms);
  if (sp->perm_d) (void)hipFree(sp->perm_d);
  if (sp->indptr) (void)hipFree(sp->indptr);
  if (sp->indices) (void)hipFree(sp->indices);
  if (sp->data) (void)hipFree(sp->data);
  if (sp->ws) (void)hipFree(sp->ws);
  if (sp->partial) (void)hipFree(sp->partial);
  if (sp->small) (void)hipFree(sp->small);
  if (sp->lz) (void)hipFree(sp->lz);
  if (sp->lzd) (void)hipFree(sp->lzd);
  if (sp->ms_ws) (void)hipFree(sp->ms_ws);
  if (sp->rhs_dev) (void)hipFree(sp->rhs_dev);
  if (sp->ms_pin) (void)hipHostFree(sp->ms_pin);
  if (sp->cg2_buf) (void)hipFree(sp->cg2_buf);
  for (double* cb : sp->ms_blk)
    if (cb) (void)hipFree(cb);
  if (sp->ms_gfin) (void)hipFree(sp->ms_gfin);
  for (hipEvent_t e : sp->ev_pool) (void)hipEventDestroy(e);
  for (auto& r : sp->spmm_log) {
    if (r.e0) (void)hipEventDestroy(r.e0);
    if (r.e1) (void)hipEventDestroy(r.e1);
  }
  if (sp->stamps) (void)hipFree(sp->stamps);
  for (hipEvent_t e : sp->ms_ev)
    if (e) (void)hipEventDestroy(e);
  if (sp->ms_stream) (void)hipStreamDestroy(sp->ms_stream);
  if (sp->win_cols) (void)hipFree(sp->win_cols);
  if (sp->win_u) (void)hipFree(sp->win_u);
  if (sp->win_lidx) (void)hipFree(sp->win_lidx);
  if (sp->stream) (void)hipStreamDestroy(sp->stream);
  delete sp;
  return 0;
}

int gpmi_sp_info(const gpmi_sp* sp, int64_t* n, int64_t* nnz) {
  if (!sp) return set_error(-1006, "null handle");
  if (n) *n = sp->n;
  if (nnz) *nnz = sp->nnz;
  return 0;
}

int gpmi_sp_get_csr(gpmi_sp* sp, int64_t* indptr, int* indices, double* data) {
  if (!sp) return set_error(-1006, "null handle");
  if (sp->dK) return set_error(-1105, "a dense operator has no CSR");
  DeviceGuard g(sp->device);
  if (sp->perm.empty()) {
    HIP_TRY(hipMemcpy(indptr, sp->indptr, sizeof(int64_t) * (sp->n + 1), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(indices, sp->indices, sizeof(int) * sp->nnz, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(data, sp->data, sizeof(double) * sp->nnz, hipMemcpyDeviceToHost));
    return 0;
  }
  // the original order: row i = device row inv[i], columns renamed back and sorted
  const int64_t n = sp->n;
  std::vector<int64_t> ip(n + 1);
  std::vector<int> ix(sp->nnz);
  std::vector<double> dv(sp->nnz);
  HIP_TRY(hipMemcpy(ip.data(), sp->indptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ix.data(), sp->indices, sizeof(int) * sp->nnz, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(dv.data(), sp->data, sizeof(double) * sp->nnz, hipMemcpyDeviceToHost));
  std::vector<int> inv(n);
  for (int64_t r = 0; r < n; ++r) inv[sp->perm[r]] = (int)r;
  indptr[0] = 0;
  std::vector<std::pair<int, double>> row;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = inv[i];
    row.clear();
    for (int64_t q = ip[r]; q < ip[r + 1]; ++q) row.emplace_back(sp->perm[ix[q]], dv[q]);
    std::sort(row.begin(), row.end(),
              [](const std::pair<int, double>& a, const std::pair<int, double>& b) {
                return a.first < b.first;
              });
    const int64_t o = indptr[i];
    for (size_t q = 0; q < row.size(); ++q) {
      indices[o + q] = row[q].first;
      data[o + q] = row[q].second;
    }
    indptr[i + 1] = o + (int64_t)row.size();
  }
  return 0;
}

}  // extern "C"

namespace gpmi {

// K[perm[r]][perm[c]] = a_rc: one wavefront per device row (the dense copy is in
// the original point order).
__global__ void __launch_bounds__(256) csr_scatter_dense_kernel(
    const int64_t* __restrict__ indptr, const int* __restrict__ indices,
    const double* __restrict__ data, const int* __restrict__ perm, int64_t n,
    double* __restrict__ K, int64_t ldk) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int lane = threadIdx.x & 63;
  const int64_t i = perm ? perm[r] : r;
  double* Ki = K + i * ldk;
  for (int64_t q = indptr[r] + lane; q < indptr[r + 1]; q += 64) {
    const int c = indices[q];
    Ki[perm ? perm[c] : c] = data[q];
  }
}

// Scatter the operator's CSR into a zeroed dense [n][ldk] device matrix on the
// device `device` (stream st); the dense operator's exact methods on a sparse K.
int sp_scatter_dense(const gpmi_sp* sp, int device, double* K, int64_t ldk, hipStream_t st) {
  if (sp->device != device)
    return set_error(-1011, "sparse and dense operators live on different devices");
  if (sp->dK) return set_error(-1105, "a dense operator has no CSR");
  HIP_TRY(hipStreamSynchronize(sp->stream));
  const unsigned grid = (unsigned)((sp->n + 3) / 4);
  hipLaunchKernelGGL(csr_scatter_dense_kernel, dim3(grid), dim3(256), 0, st, sp->indptr,
                     sp->indices, sp->data, sp->perm.empty() ? nullptr : sp->perm_d, sp->n, K,
                     ldk);
  LAUNCH_CHECK("csr_scatter_dense_kernel");
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
    int rc = grow(&sp->ws, &sp->ws_doubles, (size_t)2 * n * s);
    if (rc) return rc;
    std::vector<double> h((size_t)n * s);
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < s; ++c) h[(size_t)i * s + c] = X[orig_row(sp, i) * ld + c0 + c];
    HIP_TRY(hipMemcpyAsync(sp->ws, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice,
                          sp->stream));
    rc = spmm(sp, sp->ws, sp->ws + n * s, s, eta);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h.data(), sp->ws + n * s, sizeof(double) * h.size(),
                          hipMemcpyDeviceToHost, sp->stream));
    HIP_TRY(hipStreamSynchronize(sp->stream));
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < s; ++c) Y[orig_row(sp, i) * ldy + c0 + c] = h[(size_t)i * s + c];
  }
  return 0;
}

int gpmi_sp_lanczos(gpmi_sp* sp, int nprobe, int steps, uint64_t seed, int probe_offset,
                    double* alpha, double* beta) {
  return gpmi_sp_lanczos_ex(sp, nprobe, steps, seed, probe_offset, -1, alpha, beta);
}

int gpmi_sp_lanczos_ex(gpmi_sp* sp, int nprobe, int steps, uint64_t seed, int probe_offset,
                       int orthogonalize, double* alpha, double* beta) {
  if (!sp) return set_error(-1006, "null handle");
  if (steps < 1 || steps > 256 || nprobe < 1)
    return set_error(-1102, "steps must be in [1, 256] and nprobe >= 1");
  DeviceGuard g(sp->device);
  const int64_t n = sp->n;
  for (int p0 = 0; p0 < nprobe; p0 += MAXS) {
    const int s = std::min(MAXS, nprobe - p0);
    // the basis and a work block (the plain recurrence: three rotating blocks + one)
    int rc = grow(&sp->ws, &sp->ws_doubles, (size_t)std::max(steps + 2, 4) * n * s);
    if (rc) return rc;
    double* V = sp->ws;
    double* W = sp->ws + (size_t)(steps + 1) * n * s;
    auto probes = [&]() -> int {
      hipLaunchKernelGGL(rademacher_kernel, dim3(grid_ns(n, s)), dim3(256), 0, sp->stream, V, n,
                         s, (unsigned long long)seed, probe_offset + p0,
                         1.0 / std::sqrt((double)n), (const int*)sp->perm_d);
      LAUNCH_CHECK("rademacher_kernel");
      return 0;
    };
    if ((rc = probes())) return rc;
    if (orthogonalize == 0) {
      // the plain three-term recurrence (imate's default)
      rc = lanczos_block_plain(sp, V, sp->ws + 3 * (size_t)n * s, s, steps,
                               alpha + (size_t)p0 * steps, beta + (size_t)p0 * steps);
      if (rc) return rc;
      continue;
    }
    if (orthogonalize > 0) {
      // windowed reorthogonalisation (imate's orthogonalize = k)
      rc = lanczos_block(sp, V, W, s, steps, alpha + (size_t)p0 * steps,
                         beta + (size_t)p0 * steps, orthogonalize);
      if (rc) return rc;
      continue;
    }
    // DCGS2 (default; GPMI_LANCZOS=cgs2 selects CGS2). A block whose rho lost
    // precision to cancellation (near an invariant subspace) is redone with CGS2.
    const char* lenv = std::getenv("GPMI_LANCZOS");
    bool cgs2 = lenv && std::strcmp(lenv, "cgs2") == 0;
    if (!cgs2) {
      bool inexact = false;
      rc = lanczos_block_dcgs2(sp, V, sp->ws + (size_t)steps * n * s, W, s, steps,
                               alpha + (size_t)p0 * steps, beta + (size_t)p0 * steps, &inexact);
      if (rc) return rc;
      if (inexact) {
        ++sp->lanczos_cgs2_reruns;
        cgs2 = true;
        if ((rc = probes())) return rc;
      }
    }
    if (cgs2) {
      rc = lanczos_block(sp, V, W, s, steps, alpha + (size_t)p0 * steps,
                         beta + (size_t)p0 * steps);
      if (rc) return rc;
    }
  }
  return 0;
}

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
    int rc = grow(&sp->ws, &sp->ws_doubles, (size_t)4 * ns);
    if (rc) return rc;
    double* X = sp->ws;
    double* Rr = X + ns;
    double* Pp = Rr + ns;
    double* Q = Pp + ns;
    // device scalars: pq, rr (double-buffered by iteration parity), thr = rtol ||b||,
    // the active flags (double-buffered), the error flag and the iteration count
    double* pq = sp->small;
    double* rrb[2] = {sp->small + MAXS, sp->small + 2 * MAXS};
    double* thr = sp->small + 3 * MAXS;
    int* actb[2] = {reinterpret_cast<int*>(sp->small + 4 * MAXS),
                    reinterpret_cast<int*>(sp->small + 5 * MAXS)};
    int* err = reinterpret_cast<int*>(sp->small + 6 * MAXS);
    int* iters = err + 1;
    std::vector<double> h((size_t)ns);
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < s; ++c) h[(size_t)i * s + c] = rhs[orig_row(sp, i) * ld + c0 + c];
    HIP_TRY(hipMemcpyAsync(Rr, h.data(), sizeof(double) * ns, hipMemcpyHostToDevice, sp->stream));
    HIP_TRY(hipMemcpyAsync(Pp, Rr, sizeof(double) * ns, hipMemcpyDeviceToDevice, sp->stream));
    HIP_TRY(hipMemsetAsync(X, 0, sizeof(double) * ns, sp->stream));
    rc = col_dots(sp, Rr, 0, 1, Rr, s, rrb[0]);
    if (rc) return rc;
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
      rc = spmm(sp, Pp, Q, s, eta);
      if (rc) return rc;
      rc = col_dots(sp, Pp, 0, 1, Q, s, pq);
      if (rc) return rc;
      hipLaunchKernelGGL(cg_xr_kernel, dim3(grid), dim3(256), 0, sp->stream, Pp, Q, X, Rr,
                         rrb[cur], pq, actb[cur], n, s, err);   // x += a p, r -= a q
      LAUNCH_CHECK("cg_xr_kernel");
      rc = col_dots(sp, Rr, 0, 1, Rr, s, rrb[cur ^ 1]);
      if (rc) return rc;
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
    max_it_used = std::max(max_it_used, it_used);
    HIP_TRY(hipMemcpyAsync(bnt.data(), thr, sizeof(double) * s, hipMemcpyDeviceToHost, sp->stream));
    HIP_TRY(hipMemcpyAsync(rr.data(), rrb[it_used & 1], sizeof(double) * s, hipMemcpyDeviceToHost,
                          sp->stream));
    HIP_TRY(hipStreamSynchronize(sp->stream));
    for (int c = 0; c < s; ++c)
      if (!(std::sqrt(rr[c]) <= bnt[c])) converged = false;
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
  MsBlock blk;            // the current block, carved out of sp->ms_blk[buf]
  int buf;

  MsPin* pin() { return pin_host; }
  int mark(int slot) {
    HIP_TRY(hipEventRecord(sp->ms_ev[slot], str));
    return 0;
  }
  int wait(int slot) {
    HIP_TRY(hipEventSynchronize(sp->ms_ev[slot]));
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
    if (int rc = grow(&sp->ms_blk[nbuf], &sp->ms_blk_doubles[nbuf],
                      ms_carve(nullptr, n, a, nbd, S, nullptr)))
      return rc;
    MsBlock nw = blk;   // (the run's flags and it_stop)
    ms_carve(sp->ms_blk[nbuf], n, a, nbd, S, &nw);
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
    A.gfin = sp->ms_gfin;
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
  if (int rc = grow(&sp->ms_ws, &sp->ms_ws_doubles,
                    even((size_t)n * nbd) + even((size_t)n * nrhs)))
    return rc;
  d.Bd = sp->ms_ws;
  d.Hs = d.Bd + even((size_t)n * nbd);
  const size_t c_sp = (size_t)(kind == 5 ? sp->win_nblk : MS_DOT_BLK) * 2 * s;
  const size_t c_red = 2 * (size_t)s + (size_t)nbd * s;
  const size_t c_init = (size_t)MS_NBLK * ((size_t)nbd * s + s);
  if (int rc = grow(&sp->cg2_buf, &sp->cg2_doubles, c_sp + c_red + c_init + S + 2)) return rc;
  d.spart = sp->cg2_buf;
  d.dred = d.spart + c_sp;
  d.ipart = d.dred + c_red;
  d.dshift = d.ipart + c_init;
  if (int rc = grow(&sp->ms_blk[0], &sp->ms_blk_doubles[0],
                    ms_carve(nullptr, n, s, nbd, S, nullptr)))
    return rc;
  d.buf = 0;
  d.blk.sh.flags = reinterpret_cast<int*>(d.dshift + S);
  d.blk.sh.it_stop = reinterpret_cast<int*>(d.dshift + S + 1);
  ms_carve(sp->ms_blk[0], n, s, nbd, S, &d.blk);
  // the dropped columns' final Grams, on the device until the end
  if (gfin)
    if (int rc = grow(&sp->ms_gfin, &sp->ms_gfin_doubles, (size_t)S * nbd * s)) return rc;
  if (!sp->ms_pin) {
    // coherent: the batch's last update kernel stores the end state into it directly
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&sp->ms_pin), 2 * sizeof(MsPin),
                         hipHostMallocCoherent | hipHostMallocMapped));
    for (hipEvent_t* e : {&sp->ms_ev[0], &sp->ms_ev[1]})
      HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  d.pin_host = reinterpret_cast<MsPin*>(sp->ms_pin);
  d.pin_dev = nullptr;
  HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d.pin_dev), sp->ms_pin, 0));
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
    Hsrc = sp->rhs_dev;
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
    HIP_TRY(hipMemcpyAsync(g_final.data(), sp->ms_gfin, sizeof(double) * g_final.size(),
                          hipMemcpyDeviceToHost, str));
  }
  HIP_TRY(hipStreamSynchronize(str));
  sp->last_compactions = run.compactions;
  sp->last_segments = run.segments;
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
  if (!sp->ms_stream) {
    // the CG's own stream, at the same (normal) dispatch priority as the Lanczos's.
    // Round 5 gave it the high priority (cfg 5 11.85 -> 11.46 ms, when the CG alone took
    // 8.8 ms); since the compaction the CG alone takes 6.4 ms and a starved Lanczos (4.1
    // ms alone) plus its host-side quadrature became the step's tail: round 6 alternating
    // runs, high / normal / low: cfg 5 9.80-9.92 / 9.40-9.44 / 9.77-10.05 ms, cfg 4
    // 2.86-2.90 / 2.80-2.82 / 2.83-2.86 ms.
    HIP_TRY(hipStreamCreateWithFlags(&sp->ms_stream, hipStreamNonBlocking));
  }
  // GPMI_MS_COMPACT=0: no active-column compaction
  const char* cenv = std::getenv("GPMI_MS_COMPACT");
  const bool compact_on = !(cenv && std::atoi(cenv) == 0);
  // GPMI_MS_TRACE=1: each batch's size and each read's prediction on stderr (diagnostic)
  const bool trace = std::getenv("GPMI_MS_TRACE") != nullptr;
  MsDev dev{};
  dev.sp = sp;
  dev.str = sp->ms_stream;
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
  if (!rhs && (!sp->rhs_dev || nrhs != sp->rhs_nrhs))
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

int gpmi_sp_set_rhs(gpmi_sp* sp, const double* rhs, int64_t ld, int nrhs) {
  if (!sp) return set_error(-1006, "null handle");
  if (!rhs || nrhs < 1 || nrhs > MS_MAXS || ld < nrhs)
    return set_error(-1104, "set_rhs: need 1 <= nrhs <= 16 and ld >= nrhs");
  DeviceGuard g(sp->device);
  const int64_t n = sp->n;
  if (sp->rhs_dev && sp->rhs_nrhs != nrhs) {
    HIP_TRY(hipFree(sp->rhs_dev));
    sp->rhs_dev = nullptr;
  }
  if (!sp->rhs_dev) HIP_TRY(hipMalloc(&sp->rhs_dev, sizeof(double) * (size_t)n * nrhs));
  sp->rhs_nrhs = nrhs;
  if (ld == nrhs) {
    HIP_TRY(hipMemcpy(sp->rhs_dev, rhs, sizeof(double) * (size_t)n * nrhs, hipMemcpyHostToDevice));
  } else {
    std::vector<double> h((size_t)n * nrhs);
    for (int64_t i = 0; i < n; ++i)
      for (int c = 0; c < nrhs; ++c) h[(size_t)i * nrhs + c] = rhs[i * ld + c];
    HIP_TRY(hipMemcpy(sp->rhs_dev, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  }
  return 0;
}

int gpmi_sp_spmm_info(gpmi_sp* sp, int* windowed, double* mean_window, int* max_window) {
  if (!sp) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  if (sp->dK) {   // dense: no window
    if (windowed) *windowed = 0;
    if (mean_window) *mean_window = 0.0;
    if (max_window) *max_window = 0;
    return 0;
  }
  if (int rc = ensure_window(sp)) return rc;
  const char* wenv = std::getenv("GPMI_SPMM_WINDOW");
  const int wmode = wenv ? std::atoi(wenv) : 1;
  if (windowed) *windowed = wmode == 2 || (wmode != 0 && sp->win_use);
  if (mean_window) *mean_window = sp->win_mean;
  if (max_window) *max_window = sp->win_maxu.load(std::memory_order_acquire);
  return 0;
}

int gpmi_sp_spmm_kernel(gpmi_sp* sp, int s, int* kind) {
  if (!sp || !kind) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  return spmm_kind(sp, s, kind);
}

int gpmi_sp_last_status(const gpmi_sp* sp, int* converged) {
  if (!sp) return set_error(-1006, "null handle");
  if (converged) *converged = sp->last_converged;
  return 0;
}

int gpmi_sp_msgram_compactions(const gpmi_sp* sp, int* count) {
  if (!sp || !count) return set_error(-1006, "null handle");
  *count = sp->last_compactions;
  return 0;
}

int gpmi_sp_msgram_segments(const gpmi_sp* sp, int cap, int* widths, int* iterations,
                            int* count) {
  if (!sp || !count) return set_error(-1006, "null handle");
  const int m = (int)sp->last_segments.size();
  *count = m;
  if (m > 0 && cap < m) return set_error(-1003, "gpmi_sp_msgram_segments: cap < segments");
  if (m > 0 && (!widths || !iterations)) return set_error(-1006, "null output");
  for (int q = 0; q < m; ++q) {
    widths[q] = sp->last_segments[q].first;
    iterations[q] = sp->last_segments[q].second;
  }
  return 0;
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
  std::lock_guard<std::mutex> lock(sp->timing_mu);
  if (enable && !sp->stamps && !sp->dK) {
    if (int rc = ensure_window(sp)) return rc;
    const size_t per = sizeof(unsigned long long) * 2 * (size_t)std::max<int64_t>(1, sp->win_nblk);
    sp->stamp_cap = (int)std::min<size_t>(STAMP_CAP, STAMP_BYTES / per);
    HIP_TRY(hipMalloc(&sp->stamps, per * sp->stamp_cap));
    HIP_TRY(hipDeviceGetAttribute(&sp->wall_khz, hipDeviceAttributeWallClockRate, sp->device));
  }
  hipLaunchKernelGGL(gpmi::timing_mark_kernel, dim3(1), dim3(64), 0, sp->stream, enable);
  LAUNCH_CHECK("timing_mark_kernel");
  if (enable) {
    // the pairs of an earlier window go back to the pool (their streams are idle
    // once the caller synchronised; wait for them anyway)
    for (auto& r : sp->spmm_log) {
      if (r.slot >= 0) continue;
      HIP_TRY(hipEventSynchronize(r.e1));
      sp->ev_pool.push_back(r.e0);
      sp->ev_pool.push_back(r.e1);
    }
    sp->spmm_log.clear();
    sp->stamps_used = 0;
  }
  // (disabling keeps the window's log for gpmi_sp_spmm_timing)
  sp->timing = enable != 0;
  return 0;
}

int gpmi_sp_spmm_timing(gpmi_sp* sp, int max_widths, int* n_widths, int* widths, int* launches,
                        double* total_ms) {
  if (!sp || !n_widths) return set_error(-1006, "null handle");
  DeviceGuard g(sp->device);
  std::lock_guard<std::mutex> lock(sp->timing_mu);
  std::map<int, std::pair<int, double>> acc;
  std::vector<unsigned long long> st;
  if (sp->stamps_used > 0) {
    // every stamped launch's span, reduced on the device (after the logged work)
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long* span = nullptr;
    HIP_TRY(hipMalloc(&span, sizeof(unsigned long long) * 2 * sp->stamps_used));
    hipLaunchKernelGGL(gpmi::stamp_span_kernel, dim3(sp->stamps_used), dim3(256), 0, sp->stream,
                       sp->stamps, sp->win_nblk, span);
    LAUNCH_CHECK("stamp_span_kernel");
    st.resize((size_t)2 * sp->stamps_used);
    HIP_TRY(hipMemcpyAsync(st.data(), span, sizeof(unsigned long long) * st.size(),
                          hipMemcpyDeviceToHost, sp->stream));
    HIP_TRY(hipStreamSynchronize(sp->stream));
    HIP_TRY(hipFree(span));
  }
  for (auto& r : sp->spmm_log) {
    double ms = 0.0;
    if (r.slot >= 0) {
      const unsigned long long t0 = st[2 * r.slot], t1 = st[2 * r.slot + 1];
      if (t1 < t0 || sp->wall_khz <= 0) return set_error(-1107, "SpMM timing: a stamp slot was not written");
      ms = (double)(t1 - t0) / (double)sp->wall_khz;
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
  int rc = grow(&sp->ws, &sp->ws_doubles, (size_t)2 * ns);
  if (rc) return rc;
  hipLaunchKernelGGL(rademacher_kernel, dim3(grid_ns(sp->n, s)), dim3(256), 0, sp->stream, sp->ws,
                     sp->n, s, 12345ull, 0, 1.0, (const int*)nullptr);
  LAUNCH_CHECK("rademacher_kernel");
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  // warm-up, kept out of the in-step timing log (a logged warm-up made
  // the log 51 spans for the 50 timed launches, mixing a cold launch into the mean
  // span the bench subtracts from the gated period)
  bool timing_was;
  {
    std::lock_guard<std::mutex> lock(sp->timing_mu);
    timing_was = sp->timing;
    sp->timing = false;
  }
  rc = spmm(sp, sp->ws, sp->ws + ns, s, eta);
  {
    std::lock_guard<std::mutex> lock(sp->timing_mu);
    sp->timing = timing_was;
  }
  if (rc) return rc;
  // the timed launches wait behind a gate until all of them are queued (at most 2 s)
  int* flag = nullptr;
  HIP_TRY(hipHostMalloc(&flag, sizeof(int), hipHostMallocCoherent));
  *flag = 0;
  int khz = 0;
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, sp->device));
  hipLaunchKernelGGL(gpmi::gate_kernel, dim3(1), dim3(64), 0, sp->stream, flag,
                     (unsigned long long)std::max(khz, 1) * 2000ull);
  LAUNCH_CHECK("gate_kernel");
  HIP_TRY(hipEventRecord(e0, sp->stream));
  for (int r = 0; r < reps && rc == 0; ++r) rc = spmm(sp, sp->ws, sp->ws + ns, s, eta);
  __atomic_store_n(flag, 1, __ATOMIC_SEQ_CST);
  if (rc) {
    (void)hipStreamSynchronize(sp->stream);
    (void)hipHostFree(flag);
    return rc;
  }
  HIP_TRY(hipEventRecord(e1, sp->stream));
  HIP_TRY(hipEventSynchronize(e1));
  HIP_TRY(hipHostFree(flag));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  *avg_ms = ms / reps;
  HIP_TRY(hipEventDestroy(e0));
  HIP_TRY(hipEventDestroy(e1));
  return 0;
}

}  // extern "C"
