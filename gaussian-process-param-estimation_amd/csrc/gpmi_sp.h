// The sparse operator's handle (include/gpmi.h, gpmi_sp_*) and what its host translation
// units share. One gpmi_sp = one device-resident CSR of a tapered correlation matrix (or a
// dense K borrowed from a gpmi_op) plus the Krylov workspaces. The handle is a core (the
// size, the main stream, the CSR, the locality permutation) and one state per component:
//   gpmi_sparse_api.hip       create from CSR / dense, destroy, info, the CSR read-back and
//                             its dense scatter, the resident RHS block, the last status
//   gpmi_sparse_assemble.hip  gpmi_sp_create_matern (cell plan: gpmi_cell_plan.h)
//   gpmi_sparse_spmm.hip      the X windows, the SpMM and its in-step timing
//                             (SpDense, SpWindow, SpTiming)
//   gpmi_sparse_lanczos.hip   the three Lanczos forms (SpWork)
//   gpmi_sparse_cg.hip        the blocked CG (SpWork) and the multi-shift CG (SpMs)
//   gpmi_sparse_predict.hip   prediction on a sparse K: the cross CSR of new points and the
//                             terms c, q, G (SpPredict; reads SpGeom, which
//                             gpmi_sp_create_matern fills once)
// Every device buffer is a DevBuf, every stream and event an owner (gpmi_host.h): streams
// are declared before the buffers their work touches, gpmi_sp_destroy synchronises both.
//
// Threading. A sweep uses a handle from two host threads at once: the "main" thread calls
// spmm / lanczos / cg / bench_spmm (work on `stream`), the "ms" thread msgram* / set_rhs
// (work on ms.stream). The core, SpDense's K and a published SpWindow are read-only for
// both; SpWork and dense.Yp belong to the main thread, SpMs and dense.Yp_ms to the ms
// thread; SpTiming is shared under its mutex. Two threads in one role, or create / destroy
// beside any call, are not supported. The prediction (main thread: SpPredict, SpGeom) with
// rhs == NULL reads ms.rhs_dev: set_rhs must not run beside it.
#pragma once

#include <atomic>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "gpmi_internal.h"
#include "gpmi_host.h"
#include "gpmi_sparse.h"
#include "../../include/gpmi.h"

#pragma GCC visibility push(hidden)

namespace gpmi {

constexpr int NBLK = 256;   // fixed reduction grid (deterministic sums)
constexpr int MAXS = 32;    // vector-block width per device pass

// Dense mode (gpmi_sp_create_dense): K borrowed from a gpmi_op, no CSR. Read-only after
// create; each partial buffer is written by its own stream's thread only.
struct SpDense {
  const double* K = nullptr;
  int64_t ld = 0;
  int split = 1, kcs = 1;      // k splits of dense_mm_kernel, 64-column chunks each
  DevBuf<double> Yp;           // split partials [split][n][MAXS] of `stream`
  DevBuf<double> Yp_ms;        // ... of ms.stream (the CG beside the Lanczos)
};

// X windows of the default SpMM (csr_spmm_win_kernel), built on first use under mu
// (ensure_window) and read-only from both threads once published.
struct SpWindow {
  std::mutex mu;               // the lazy build
  DevBuf<int> cols;            // [nblk][WIN_MAXU] sorted window columns
  DevBuf<int> u;               // [nblk] window sizes (0: block gathers from X)
  DevBuf<unsigned short> lidx; // [nnz] window position of every nonzero
  // -1: not built. Published (release) after every other window field, so a reader
  // that sees it >= 0 (acquire) sees the whole window
  std::atomic<int> maxu{-1};
  int maxm = 0;                // most nonzeros in a windowed block
  double mean = 0.0;           // mean window columns per block
  bool use = false;            // the windowed kernel is the faster one here
  int64_t nblk = 0;
};

// Workspaces of the calls on `stream` (grown to the largest call so far): main thread only.
struct SpWork {
  DevBuf<double> ws;           // vector blocks
  DevBuf<double> partial;      // [NBLK][J][s]
  DevBuf<double> small;        // coefficient / reduction arrays
  DevBuf<double> lz;           // Lanczos scalars (lanczos_block, lanczos_block_plain)
  DevBuf<double> lzd;          // DCGS2 Lanczos scalars (lanczos_block_dcgs2)
  int lanczos_cgs2_reruns = 0; // DCGS2 blocks rerun with CGS2 (cancellation in rho)
};

// The multi-shift CG (gpmi_sp_msgram) has a stream and workspaces of its own, so that it
// may run from another host thread beside a Lanczos on `stream` (the sparse step's two
// independent halves overlap on the device): ms thread only.
struct SpMs {
  Stream stream;               // created at the first msgram
  DevBuf<double> ws;           // B [n][nb] and the host staging [n][nrhs]
  DevBuf<double> rhs_dev;      // resident RHS block [n][rhs_nrhs] (gpmi_sp_set_rhs)
  int rhs_nrhs = 0;
  PinnedMem pin;               // pinned flags / r.r of two CG batches
  // the Chronopoulos-Gear form's dot rows (sized for the start width), the shifts and
  // the two flags
  DevBuf<double> cg2_buf;
  // the block's state (MsBlock: R, W, S, the B^T r partials, the scalars), two buffers,
  // alternating: the start block in [0], compaction k (1-based) gathers the active
  // columns from the current one into [k & 1]
  DevBuf<double> blk[2];
  DevBuf<double> gfin;         // the stopped columns' final Grams [S nb][s0]
  Event ev[2];
  int last_compactions = 0;    // active-column compactions of the last multi-shift CG
  // its launch segments: (block width, iterations launched at that width), in order
  std::vector<std::pair<int, int>> last_segments;
};

// In-step SpMM timing (gpmi_sp_set_timing), logged per launch with its width;
// gpmi_sp_spmm_timing sums the spans per width. The window SpMM (every SpMM of the sparse
// sweeps) stamps each workgroup's start and end on the device's constant wall clock into
// the launch's slot of `stamps` (win.nblk pairs, plain stores at the workgroup's end);
// stamp_span_kernel reduces a slot to the launch's span. Other kinds get a HIP event pair
// on their stream. Both threads launch SpMMs: all but `on` is touched under mu only.
struct SpTiming {
  std::mutex mu;
  bool on = false;
  EventPool events;            // every event created, in the log or free
  std::vector<hipEvent_t> free_ev;
  DevBuf<unsigned long long> stamps;   // [stamp_cap][win.nblk][2]
  int stamp_cap = 0;           // launches the buffer holds
  int stamps_used = 0;
  int wall_khz = 0;            // wall clock rate (hipDeviceAttributeWallClockRate)
  struct SpmmRec {
    hipEvent_t e0, e1;
    int s;
    int slot;                  // stamps slot, or -1 (events)
  };
  std::vector<SpmmRec> log;
};

// What gpmi_sp_create_matern keeps for a later cross assembly (gpmi_sparse_predict.hip):
// about n (d + 2) words, read-only after create. Handles from a CSR or a dense K have
// none (has = false): they take the cross matrix from the caller.
struct SpGeom {
  bool has = false;
  int d = 0;
  MaternParams P{};
  double tau = 0.0, xcut = 0.0;
  bool cells = false;          // the create found a plan: grid, cell_start, cell_perm
  CrossGrid grid{};            // gdim, pmin, wid
  DevBuf<double> points;       // [n][d], original order
  DevBuf<double> scale;        // [scale | 1 / scale]
  DevBuf<int> cell_start;      // [cells + 1]
  DevBuf<int> cell_perm;       // [n] the points cell by cell
  DevBuf<int> inv;             // [n] device row of each original point (perm's inverse)
};

// The sparse prediction (main thread): the last cross CSR (columns = device rows) and the
// blocks that outlive a CG on work.ws.
struct SpPredict {
  int64_t nstar = 0, nnz = 0;
  std::vector<int64_t> indptr_h;   // host copy of the row pointers
  DevBuf<int64_t> indptr;
  DevBuf<int> indices;
  DevBuf<double> data;
  DevBuf<double> test;         // [nstar][d] new points
  DevBuf<int> cnt;             // [nstar] row counts
  DevBuf<double> R, Sol;       // [n][s] R = [X z] in device order, S^-1 R
  DevBuf<double> out;          // c [nstar][s], q [nstar], G [s][s]
  DevBuf<double> partial;      // [NBLK][s][s] Gram partials
};

}  // namespace gpmi

struct gpmi_sp {
  int device = 0;
  int64_t n = 0, nnz = 0;
  double tau = 0.0;
  gpmi::Stream stream;
  gpmi::SpMs ms;                 // (here: its stream, too, outlives the buffers below)
  gpmi::DevBuf<int64_t> indptr;
  gpmi::DevBuf<int> indices;
  gpmi::DevBuf<double> data;
  // Locality order (gpmi_sp_create_matern, d <= 3): device row r is original point
  // perm[r] (cells in Morton order), so the rows a CU streams through have their X
  // gathers in a compact window that stays in its XCD's L2. Host inputs and
  // outputs of every call stay in the original order (permuted at the boundary).
  std::vector<int> perm;         // empty: identity
  gpmi::DevBuf<int> perm_d;
  // The last gpmi_sp_cg (main thread) or gpmi_sp_msgram (ms thread) met rtol in every
  // column. In the core, and atomic, because both roles write it: the last to finish wins.
  std::atomic<int> last_converged{1};
  gpmi::SpDense dense;
  gpmi::SpWindow win;
  gpmi::SpWork work;
  gpmi::SpTiming tim;
  gpmi::SpGeom geom;
  gpmi::SpPredict pred;
};

namespace gpmi {

// create paths: the handle until *out takes it (synchronises, then deletes)
struct SpDelete {
  void operator()(gpmi_sp* sp) const { (void)gpmi_sp_destroy(sp); }
};
using SpPtr = std::unique_ptr<gpmi_sp, SpDelete>;

// gpmi_sparse_spmm.hip
// The X windows of the window SpMMs, built once (under win.mu); a failed build frees
// its buffers, so a retry allocates afresh.
int ensure_window(gpmi_sp* sp);
// The SpMM kernel for an s-column block, before the alignment of a given block is known
// (gpmi_sp_spmm_kernel; the kinds: gpmi_sparse_spmm.hip).
int spmm_kind(gpmi_sp* sp, int s, int* kind);
// Y = (K + eta I) X on st (nullptr: the main stream). With pqp, a kernel that can also
// writes the per-block partials X . Y per column (pqp[block][s], the multi-shift CG's
// p . q) and sets *pq_blocks to their count; otherwise *pq_blocks = 0 and the caller
// forms them. With in-step timing on, the launch is logged.
int spmm(gpmi_sp* sp, const double* X, double* Y, int s, double eta, hipStream_t st = nullptr,
         double* pqp = nullptr, int* pq_blocks = nullptr, int dots2 = 0);

// gpmi_sparse_lanczos.hip
// out[j][c] = sum_i A_j[i][c] B[i][c], j < J  (device out)
int col_dots(gpmi_sp* sp, const double* A, int64_t strideA, int J, const double* B, int s,
             double* out, double* partial = nullptr, hipStream_t st = nullptr);

// gpmi_sparse_cg.hip
// The blocked CG of gpmi_sp_cg on a block already on the device: work.ws holds
// [X | R | P | Q], n * s doubles each, with the right-hand sides b in R (device row order).
// Leaves the solutions in X. *it_used: iterations of the slowest column; *converged is
// cleared when a column stopped at maxiter. Status 1: p^T (K + eta I) p <= 0.
int cg_block_device(gpmi_sp* sp, double eta, int s, double rtol, int maxiter, int* it_used,
                    bool* converged);

inline unsigned grid_ns(int64_t n, int s) { return (unsigned)((n * s + 255) / 256); }

// device row r <- original row orig(r)
inline int64_t orig_row(const gpmi_sp* sp, int64_t r) {
  return sp->perm.empty() ? r : (int64_t)sp->perm[r];
}

}  // namespace gpmi

#pragma GCC visibility pop
