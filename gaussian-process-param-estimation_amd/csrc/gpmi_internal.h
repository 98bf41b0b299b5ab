// Internal declarations shared by the gpmi HIP translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "gpmi_ms_sched.h"   // MS_MAXS, MsPin (HIP-free: shared with the host scheduler)

#define GPMI_MAX_DIM 8     // max point dimension handled by the assembly kernel
#define GPMI_TS 128        // tile / diagonal-block size of the blocked Cholesky
#define GPMI_RHS_LD 16     // leading dimension (max columns) of a resident RHS block

struct gpmi_sp;   // include/gpmi.h

namespace gpmi {

// Flags of the events that only order one device's streams (never read by the host):
// no timing, and no system-scope fence on record (the default release writes back and
// invalidates caches for host visibility, which a consumer kernel on the same device
// does not need). GPMI_EV_SYSFENCE=1 restores the system-scope fence (A/B).
inline unsigned sync_event_flags() {
  static const unsigned f = [] {
    const char* e = getenv("GPMI_EV_SYSFENCE");
    return (unsigned)hipEventDisableTiming |
           ((e && e[0] == '1') ? 0u : (unsigned)hipEventDisableSystemFence);
  }();
  return f;
}
// Timing events (elapsed time only; the host never reads memory behind them): timing
// kept, the system-scope fence dropped the same way.
inline unsigned timing_event_flags() {
  return sync_event_flags() & ~(unsigned)hipEventDisableTiming;
}

enum MaternMode { MATERN_HALF = 0, MATERN_3HALF = 1, MATERN_5HALF = 2,
                  MATERN_GENERAL = 3, MATERN_GAUSS = 4 };

struct MaternParams {
  int mode;
  double nu;
  double sqrt2nu;     // sqrt(2 nu)
  double mu;          // general nu >= 2: starting order nu - floor(nu) + 1 in [1, 2)
  double lp0, lp1;    // log(2^(1-a) / Gamma(a)) at a = mu, mu + 1 (a = nu when nu < 2)
};

// Dense Matérn assembly: lower-triangular 64 x 64 tiles (grid = T (T + 1) / 2,
// T = ceil(n_pad / 64)), each mirrored (gpmi_matern.hip).
void launch_matern_dense(dim3 grid, hipStream_t s, const double* points, int64_t n, int d,
                         const double* scale, const MaternParams& P, double* K, int64_t ldk,
                         int64_t n_pad);

// Batched factorization kernels (gpmi_chol.hip). All matrices are row-major
// n_pad x n_pad with leading dimension lda; batch member b lives at base + b*stride.
struct BatchPtrs {
  double* A;        int64_t sA;       // working matrices K + eta_b I -> L
  double* R;        int64_t sR;       // RHS blocks [n_pad][16] -> L^-1 R
  double* U;        int64_t sU;       // per-step u_k = A_kk^-1 r_k  [128][16]
  double* Linv;     int64_t sL;       // inverses of the diagonal blocks [nt][128][128]
  double* logdiag;  int64_t sLD;      // per diagonal block: 2 sum log L_ii  [nt]
  double* gram;     int64_t sG;       // per diagonal block Gram partials [nt][16][16]
  int* info;                          // first non-positive pivot (1-based), per member
};

__global__ void shift_copy_kernel(const double* K, int64_t ldk, double* A, int64_t lda,
                                  int64_t sA, const double* etas, int nb, int64_t n,
                                  int wc);
__global__ void diag_block_kernel(BatchPtrs P, int64_t lda, int kb, int nt);
__global__ void panel_kernel(BatchPtrs P, int64_t lda, int kb);
__global__ void colpanel_kernel(BatchPtrs P, int64_t lda, int kb, int c0, int next_diag);
// The two pipeline forms of tile_mma's k-loop (gpmi_device.h). Both run, per accumulator,
// the same MFMA sequence in the same k order: the same results, bit for bit.
//   KLOOP_LATE : the next slab's global loads at the start of a stage, its LDS writes
//                after the stage's last MFMA, one barrier per stage.
//   KLOOP_EARLY: the LDS hand-off off the MFMA path (tile_mma_early).
enum { KLOOP_LATE = 0, KLOOP_EARLY = 1 };
template <int KL>
__global__ void syrk_kernel(double* A, int64_t lda, int64_t sA, int tc0, int w, int t,
                            int p0, int kdim, const uint32_t* order, const double* Ksrc,
                            const double* etas, int64_t n);
__global__ void finalize_kernel(BatchPtrs P, int nt, double* out, int out_ld);
__global__ void bwd_step_kernel(BatchPtrs P, int64_t lda, int kb, double* X, int64_t sX);
__global__ void fwd_step_kernel(BatchPtrs P, int64_t lda, int kb);
__global__ void gemv_sym_kernel(const double* K, int64_t ldk, int64_t n,
                                const double* x, int64_t ldx, int ncol, double* y,
                                double eta, int exponent);
__global__ void trace_kernel(const double* K, int64_t ldk, int64_t n, double* out);
__global__ void trinv_diag_kernel(const double* Linv, double* W, int64_t ldw, int k,
                                  double* partial);
__global__ void trinv_update_kernel(const double* L, int64_t lda, double* W, int64_t ldw, int i0,
                                    int nj, int kb, int ke);
__global__ void gram_panel_kernel(double* W, int64_t ldw, double* Td, int p0, int kdim,
                                  int imax);
__global__ void gram_sumsq_kernel(const double* W, int64_t ldw, const double* Td,
                                  double* partial);
__global__ void matern_eval_kernel(const double* x, int64_t m, MaternParams P, double* out);

// Cross Matérn assembly C[j][i] = matern(test_j, points_i), zero for j >= ns or i >= n;
// rows x cols entries are written (gpmi_matern.hip).
void launch_matern_cross(hipStream_t s, const double* points, int64_t n, const double* test,
                         int64_t ns, int d, const double* scale, const MaternParams& P,
                         double* C, int64_t ldc, int64_t rows, int64_t cols);

// Prediction terms (gpmi_predict.hip; launch list in gpmi_predict_plan.h).
__global__ void pred_update_kernel(const double* L, int64_t lda, double* T, int64_t ldt, int i0,
                                   int ni, int nct, int kb, int ke);
__global__ void pred_diag_kernel(const double* L, int64_t lda, const double* Linv,
                                 const double* Y, double* T, int64_t ldt, int k, int kb,
                                 double* part, int64_t ns_ld);
__global__ void pred_reduce_kernel(const double* part, int nt, int64_t cnt, double* out);
__global__ void pred_gram_kernel(const double* Y, double* gpart);
__global__ void pred_cov_partial_kernel(const double* T, int64_t ldt, int nct, int nt, int S,
                                        double* part);
__global__ void pred_cov_reduce_kernel(const double* part, int S, int nct, double* C,
                                       int64_t ldc);

// Leave-one-out terms (gpmi_loo.hip): per row 16 entries of W Y, then the row's sum of
// squares of W. One workgroup per LOO_ROWS rows and chunk of LOO_CHUNK columns (three
// tiles: chunk starts 3 KB apart, not a power of two), Y staged in LDS in sub-blocks of
// LOO_STAGE columns (32 KB).
constexpr int LOO_LD = 17;
constexpr int LOO_CHUNK = 384;
constexpr int LOO_STAGE = 256;
constexpr int LOO_ROWS = 64;
__global__ void loo_pass_kernel(const double* W, int64_t ldw, const double* Y, int64_t n_pad,
                                int cw, double* part);
__global__ void loo_reduce_kernel(const double* part, int64_t n_pad, int cw, int nchunk,
                                  double* out);

// Correlation-scale gradient terms (gpmi_scale_grad.hip): one workgroup per lower tile of
// A^-1 -> part[tile][1 + ncoef][8], reduced over the tiles in ascending order into
// out[1 + ncoef][8]. mode: a closed form or MATERN_GAUSS; nc: ncoef rounded up to 0, 2 or
// 4, the coefficient matrices coef[nc][16][16] the pass multiplies (zero beyond ncoef).
constexpr int SG_MAX_COEF = 4;
void launch_scale_grad_pass(hipStream_t s, int mode, int nc, const double* W, int64_t ldw,
                            const double* Td, const double* sol, const double* coef, int ncoef,
                            const double* points, int64_t n, int d, const double* scale, int nt,
                            double* part);
__global__ void scale_grad_reduce_kernel(const double* part, int ntile, int nval, int d,
                                         const double* scale_dev, double* out);

// Second-order (expected information) terms (gpmi_fisher.hip): M_k = A^-1 dK / d rho_k on
// fp64 MFMA into M[d][np][np], the traces tr(M_a M_b) tile by tile and reduced in a fixed
// order, the thin products with [np][16] blocks and their 16 x 16 Grams. a = 0 stands for
// A^-1 itself, read from the tiles (W, Td) with the pad masked.
void launch_fisher_product(hipStream_t s, int mode, const double* W, int64_t np, const double* Td,
                           const double* points, int64_t n, int d, const double* scale, int nt,
                           double* M);
__global__ void fisher_trace_kernel(const double* M, int64_t np, const double* W,
                                    const double* Td, int64_t n, int d, int nt, double* part);
__global__ void fisher_trace_reduce_kernel(const double* part, int ntile, double* out);
__global__ void fisher_copy_sol_kernel(const double* sol, int64_t np, double* Y0);
void launch_fisher_thin(hipStream_t s, bool trans, int a0, int count, const double* M, int64_t np,
                        const double* W, const double* Td, int64_t n, const double* X, int ldx,
                        double* out);
__global__ void fisher_gram_kernel(const double* YZ, int64_t np, int d, double* out);

// Draws from the cached factor and the covariance hand-over (gpmi_sample.hip; work list in
// gpmi_sample_plan.h).
__global__ void sample_normal_kernel(double* Xi, int64_t ld, int64_t rows, int64_t cols,
                                     unsigned long long seed, unsigned long long first);
__global__ void sample_trmm_kernel(const double* L, int64_t lda, const double* Xi, int64_t ldx,
                                   int jt, int D, int split, const uint32_t* order, double* Y,
                                   int64_t ldy, double* part);
__global__ void sample_reduce_kernel(const double* part, int jt, int D, double* Y, int64_t ldy);
__global__ void cov_lowrank_kernel(const double* src, int64_t lds, double* dst, int64_t np,
                                   int64_t n, const double* U, int m);

// Multi-shift CG Gram state (gpmi_sparse.hip, gpmi_sparse_cg.hip); device pointers.
#ifndef GPMI_LZ_JC
#define GPMI_LZ_JC 16
#endif
constexpr int LZ_JC = GPMI_LZ_JC;   // basis vectors per lz_dots_kernel launch (DCGS2 Lanczos)

// The Chronopoulos-Gear multi-shift CG (ms_cg2_update_kernel): the seed scalars,
// double-buffered by iteration parity (every block of iteration k reads cur, block 0
// writes nxt), and the shift state only block 0 touches.
struct MsScal {
  double* rr;      // [s] gamma_{k-1} = r_{k-1} . r_{k-1} (cur at iteration k)
  double* a;       // [s] alpha_{k-1}
  double* a_prev;  // [s] alpha_{k-2}
  double* beta;    // [s] beta_{k-2}
  int* active;     // [s] the column took step k-1
};
struct MsShift {
  double* bn2;     // [s] ||b_c||^2
  double* z;       // [S][s] zeta_j
  double* z_prev;  // [S][s]
  double* bp;      // [S][s'][s] b_c' . p_{j,c}
  double* g;       // [S][s'][s] accumulated G_j[c'][c]
  int* flags;      // [1] p^T (K + eta_0 I) p <= 0 in an active column
  int* it_stop;    // [1] the first iteration with no active column (-1: none yet)
};
constexpr int MS_UB = 512;      // vector blocks of ms_cg2_update_kernel (256 / 1024: cfg 5
                                // 12.37 / 12.12 against 11.91 ms per step)
constexpr int MS_DOT_BLK = 256; // blocks of ms_dots2_kernel (SpMM kinds without the epilogue)

// One active-column compaction of the multi-shift CG as ONE launch (round 6): up to
// MS_CJOBS column gathers src[r][s][L] -> dst[r][a][L] by the map, the stopped columns'
// Grams scattered into their final slots (gfin[jc][s0], by original column), and the
// compacted block's active flags set. Everything by value: no host copy, no sync.
constexpr int MS_CJOBS = 12;
struct MsCompactJob {
  const double* src;
  double* dst;
  int64_t rows;
  int L;
  int pad;
};
struct MsCompactArgs {
  MsCompactJob job[MS_CJOBS];
  int njob, s, a, nd, s0, pad;
  int map[MS_MAXS];         // the kept columns (old block index), in order
  int drop[MS_MAXS];        // the dropped columns (old block index)
  int drop_orig[MS_MAXS];   // their original column
  const double* g;          // [SN][s] the old block's Grams
  double* gfin;             // [SN][s0]
  int64_t SN;               // S * nbd
  const int* act_src;       // [s] the old block's active flags at the compaction
  int* act;                 // [a] the compacted block's (a kept column may have stopped
                            //     since the slot the map came from was written)
};

// Scatter a sparse operator's CSR (original point order) into a zeroed dense
// [n][ldk] matrix on the same device (gpmi_sparse_api.hip).
int sp_scatter_dense(const ::gpmi_sp* sp, int device, double* K, int64_t ldk,
                     hipStream_t st);

}  // namespace gpmi
