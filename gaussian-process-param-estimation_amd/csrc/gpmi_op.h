// The dense operator's handle (include/gpmi.h, gpmi_op_*) and what its host translation
// units share. One gpmi_op = one device-resident correlation matrix K (padded to n_pad,
// a multiple of 128, identity in the pad) plus workspace for max_batch concurrent
// factorizations of K + eta_b I. All work of an op runs in order on the op's own HIP
// stream; the host blocks only when it reads results back. The handle is a core (K, the
// resident RHS, the stream, the knobs) and one state per component:
//   gpmi_api.hip            create / destroy, loading K, RHS, matvec, trace, the knobs
//   gpmi_dense_factor.hip   the Cholesky schedule, its timing, and the calls that consume
//                           a factor (DenseFactor, DenseTiming, DenseTraceInv)
//   gpmi_dense_predict.hip  the prediction terms and the joint covariance (DensePredict)
//   gpmi_dense_loo.hip      the leave-one-out terms (DenseLoo)
//   gpmi_dense_scale_grad.hip  the correlation-scale gradient terms (DenseScaleGrad)
//   gpmi_dense_fisher.hip   the second-order terms of the expected information (DenseFisher)
//   gpmi_dense_sample.hip   draws from the cached factor, and the hand-over of the joint
//                           covariance to a second operator (DenseSample)
// Every device buffer is a DevBuf, every stream and event an owner (gpmi_host.h):
// destruction is member order, streams after the buffers their work may touch.
#pragma once

#include <array>
#include <map>
#include <utility>
#include <vector>

#include "gpmi_internal.h"
#include "gpmi_dense_plan.h"
#include "gpmi_host.h"
#include "../../include/gpmi.h"

namespace gpmi {
int matern_params_host(double nu, MaternParams* P);   // gpmi_api.hip
}  // namespace gpmi

#pragma GCC visibility push(hidden)

namespace gpmi {

constexpr int TS = GPMI_TS;
constexpr int RLD = GPMI_RHS_LD;
constexpr int OUT_LD = 1 + RLD * RLD;

// The batch workspace of the factorization and the cached factor.
struct DenseFactor {
  Stream stream3;          // second batch group (groups == 2); alive only inside a
                           // batched call (gpmi_op_loglik_batch releases it)
  Event ev_fork, ev_g;     // stream -> stream3 at the start of the halves, and back
  DevBuf<double> A;        // [max_batch][n_pad][n_pad]
  DevBuf<double> R, X;     // [max_batch][n_pad][16] each
  DevBuf<double> U;        // [max_batch][128][16]
  DevBuf<double> Linv;     // [max_batch][nt][128][128]
  DevBuf<double> logdiag;  // [max_batch][nt]
  DevBuf<double> gram;     // [max_batch][nt][256]
  DevBuf<double> out;      // [max_batch][OUT_LD]
  DevBuf<double> etas;     // [max_batch]
  DevBuf<int> info;        // [max_batch]
  // grouped syrk tile orders, one per trailing-update shape (w, t) of the schedule
  DevBuf<uint32_t> order;
  int order_nt = -1, order_outer = -1, group = 8;
  std::map<std::pair<int, int>, int64_t> order_off;
  // factor cache: batch slot 0 holds the factor of K + cached_eta I
  bool cache_valid = false;
  double cached_eta = 0.0;
  // members of the last factorization of the current K (0: none since K was loaded);
  // slots 1 .. last_nb - 1 hold their factors until the next one (gpmi_op_get_factor)
  int last_nb = 0;

  // K changed: no slot holds a factor of it.
  void drop() {
    cache_valid = false;
    last_nb = 0;
  }

  BatchPtrs ptrs(int64_t n_pad, int nt) const {
    BatchPtrs p;
    p.A = A, p.sA = n_pad * n_pad;
    p.R = R, p.sR = n_pad * RLD;
    p.U = U, p.sU = (int64_t)TS * RLD;
    p.Linv = Linv, p.sL = (int64_t)nt * TS * TS;
    p.logdiag = logdiag, p.sLD = nt;
    p.gram = gram, p.sG = (int64_t)nt * 256;
    p.info = info;
    return p;
  }
};

// HIP-event timing of the factorization and of the prediction (gpmi_op_set_timing).
struct DenseTiming {
  bool on = false;
  bool trace = false;      // GPMI_SYRK_TRACE: per-class breakdown
  EventPool span;          // begin, end of a factorization
  EventPool syrk;          // (begin, end) per logged syrk_kernel launch
  EventPool colpanel;      // (begin, end) per colpanel_kernel launch (trace only)
  size_t colpanel_used = 0;
  EventPool pred;          // begin, end of a prediction call; (begin, end) per trailing product
  EventPool cov;           // begin, end of the covariance's partial-product launch
  EventPool loo;           // begin, end of the leave-one-out pass over W
  EventPool sgrad;         // begin, end of the scale gradient's pass over the tiles of A^-1
  EventPool fisher;        // begin of the call, begin and end of the product stage, end of the call
  EventPool samp;          // per chunk of draws: begin, end of the normals and of the product
  std::vector<std::pair<int, double>> syrk_log;  // (event index, flops)
  std::vector<std::array<int, 3>> syrk_shape;    // (w, t, kdim) per logged launch
  double last_syrk_ms = 0.0, last_syrk_flops = 0.0, last_total_ms = 0.0;
  double last_syrk_busy_ms = 0.0;                // union of syrk launch intervals
  int last_syrk_launches = 0;
};

// gpmi_op_traceinv: the workspace (allocated at the first call) and the trace cache.
struct DenseTraceInv {
  DevBuf<double> W;        // [n_pad][n_pad] L^-T
  DevBuf<double> tpart;    // [nt * (nt + 1) / 2 + nt * nt] partials
  DevBuf<double> Td;       // [nt][128][128] diagonal tiles of A^-1 (exponent 2)
  uint64_t gen = ~0ull;    // the factor generation the cache is valid for
  int have = 0;            // bit 0: W and tr(A^-1), bit 1: the tiles of A^-1 and tr(A^-2)
  double value[2] = {0.0, 0.0};
};

// gpmi_op_predict_terms / gpmi_op_predict_cov: workspace grown to the largest call so
// far (sizes: gpmi_predict_plan.h), and where Y = L^-1 rhs_src currently is.
struct DensePredict {
  DevBuf<double> PY;       // [n_pad][16] Y, kept where solve does not write
  DevBuf<double> Pgram;    // [nt][256] partials, then [256] G = Y^T Y
  DevBuf<double> PT;       // [wide][n_pad] the chunk's working block, transposed; a
                           // covariance call widens it to every test column
  DevBuf<double> Ppart;    // [nt][wide][17] per-tile-row partials
  DevBuf<double> Pout;     // [wide][17]
  DevBuf<double> Pcov;     // [nsp][nsp] K**, then C0 = K** - V V^T
  DevBuf<double> Pcpart;   // [tiles][S][128][128] depth pieces of the product
  int ncu = 0;             // compute units (read at the first covariance call)
  int64_t cov_nstar = 0;   // Pcov holds C0 of this many points, leading dimension their
                           // count rounded up to a tile (0: nothing resident)
  uint64_t ry_gen = ~0ull; // factor generation for which R slot 0 holds L^-1 rhs_src
  uint64_t ry_rhs = ~0ull; // ... and the rhs generation
  uint64_t py_gen = ~0ull, py_rhs = ~0ull;   // the same for PY / Pgram
  double last_pred_ms = 0.0, last_pred_trail_ms = 0.0, last_pred_trail_flops = 0.0;
  double last_cov_ms = 0.0, last_cov_flops = 0.0;
  int last_cov_split = 0;  // depth pieces of the last covariance call
};

// gpmi_op_loo_terms: workspace grown to the largest call so far.
struct DenseLoo {
  DevBuf<double> part;     // [nchunk][n_pad][17] per-chunk partials
  DevBuf<double> out;      // [n_pad][17] (W Y)_i, then d_i
  double last_ms = 0.0, last_bytes = 0.0;
};

// gpmi_op_scale_grad_terms: the points, scale and coefficient matrices of the call on the
// device, and the per-tile partials (grown to the largest call so far).
struct DenseScaleGrad {
  DevBuf<double> pts;      // [n][d]
  DevBuf<double> scale;    // [8]
  DevBuf<double> coef;     // [4][16][16]
  DevBuf<double> part;     // [nt (nt + 1) / 2][1 + ncoef][8]
  DevBuf<double> out;      // [1 + ncoef][8]
  double last_ms = 0.0, last_bytes = 0.0;
};

// gpmi_op_fisher_terms: the points and scale of the call on the device, the d products
// M_k = A^-1 dK / d rho_k, the thin blocks and the partials (grown to the largest call so far).
struct DenseFisher {
  DevBuf<double> pts;      // [n][d]
  DevBuf<double> scale;    // [8]
  DevBuf<double> M;        // [d][n_pad][n_pad]
  DevBuf<double> YZ;       // [2][d + 1][n_pad][16] Y_a = N_a S, then Z_a = A^-1 Y_a
  DevBuf<double> part;     // [(d + 1)(d + 2) / 2][nt * nt] per-tile partials of the traces
  DevBuf<double> out;      // [(d + 1)(d + 2) / 2] traces, then [(d + 1) + (d + 1)^2][16][16] Grams
  double last_product_ms = 0.0, last_total_ms = 0.0;
};

// gpmi_op_sample / gpmi_op_load_predict_cov: workspace of one chunk of draws, grown to
// the largest so far (sizes and work list: gpmi_sample_plan.h).
struct DenseSample {
  DevBuf<double> Xi;       // [chunk][n_pad] the normals, sample-major
  DevBuf<double> Y;        // [chunk][n_pad] the draws
  DevBuf<double> part;     // [pieces][draw tiles][128][128] depth pieces of the product
  DevBuf<uint32_t> order;  // the pieces, deepest first, for (order_nt, order_depth)
  int order_nt = -1, order_depth = -1;
  DevBuf<double> U;        // [n][m] the low-rank factor of gpmi_op_load_predict_cov
  Event ev_src;            // the source operator's work -> this operator's stream
  double last_normal_ms = 0.0, last_trmm_ms = 0.0, last_trmm_flops = 0.0;
};

}  // namespace gpmi

struct gpmi_op {
  int device = 0;
  int64_t n = 0, n_pad = 0;
  int nt = 0;
  int max_batch = 1;
  int outer = 16;                      // outer panel width in 128-column tiles
  int panel_mode = gpmi::DENSE_REC;    // schedule inside an outer panel (GPMI_PANEL)
  int kloop = gpmi::KLOOP_EARLY;       // k-loop form of syrk_kernel (GPMI_KLOOP)
  int groups = 0;                      // 2: the batch runs as two halves on two streams;
                                       // 0: auto (2 for batches of 2..32, 1 above)
  gpmi::Stream stream;
  gpmi::DenseFactor fac;          // (here: its second stream, too, outlives the buffers below)
  gpmi::DevBuf<double> K;         // [n_pad][n_pad]
  gpmi::DevBuf<double> rhs_src;   // [n_pad][16] the resident RHS
  gpmi::DevBuf<double> scratch;   // [n_pad][16] (matvec input, solve's RHS block)
  gpmi::DevBuf<double> scratch2;  // [n_pad][16] (matvec output)
  gpmi::DevBuf<double> tracebuf;  // [n_pad][2]
  int nrhs = 0;
  bool has_K = false;
  uint64_t factor_gen = 0;        // bumped by every factorization
  uint64_t rhs_gen = 0;           // bumped by gpmi_op_set_rhs
  gpmi::DenseTiming tim;
  gpmi::DenseTraceInv tinv;
  gpmi::DensePredict pred;
  gpmi::DenseLoo loo;
  gpmi::DenseScaleGrad sgrad;
  gpmi::DenseFisher fisher;
  gpmi::DenseSample samp;

  gpmi::BatchPtrs ptrs() const { return fac.ptrs(n_pad, nt); }
};

namespace gpmi {

// gpmi_api.hip: columns [col0, col0 + nrhs) of an [n][ld] host block into dst [n_pad][16]
int upload_rhs(gpmi_op* op, double* dst, const double* rhs, int64_t ld, int nrhs, int col0);

// gpmi_dense_factor.hip
// The factor of K + eta I in batch slot 0, from the cache or by a factorization with
// the fused forward substitution of rhs_dev (*fresh); read back as positive definite,
// else the cache is dropped and the pivot is the error.
int factor_ready(gpmi_op* op, double eta, const double* rhs_dev, bool* fresh);
// R slot 0 <- L^-1 R slot 0 with the factor in slot 0.
int forward_substitute(gpmi_op* op, const BatchPtrs& P);
// W = L^-T of the cached factor in slot 0 into tinv.W, with tr((K + eta I)^-1) from the
// same launches; nothing when tinv already holds them for this factorization.
int traceinv_build_w(gpmi_op* op);
// The lower tiles of A^-1 = W W^T (strict lower tiles in W's lower block triangle,
// diagonal tiles in tinv.Td) and tr(A^-2) from them, after traceinv_build_w; nothing when
// tinv already holds them for this factorization.
int traceinv_build_ainv(gpmi_op* op);

// gpmi_dense_loo.hip
// loo.out [n_pad][17] <- row i of A^-1 rhs_src, then (A^-1)_ii, by the chunked pass over W
// and its reduce (GPMI_LOO_CHUNK read per call), after traceinv_build_w.
int loo_build_sol(gpmi_op* op);

// gpmi_dense_predict.hip
// Y = L^-1 rhs_src for the cached factor into pred.PY, and G = Y^T Y into pred.Pgram[0..256).
int predict_refresh_y(gpmi_op* op);

}  // namespace gpmi

#pragma GCC visibility pop
