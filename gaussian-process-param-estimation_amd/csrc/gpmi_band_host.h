// The band handle (include/gpmi.h, gpmi_band_*) and what its host translation units
// share. The handle is a core (the band Ab, Q^T R in Y, the streams every part uses)
// and one state per component:
//   gpmi_band_reduce.hip  dense -> band, Q^T on the RHS          (BandReduce)
//   gpmi_band_eval.hip    the likelihood terms of B + eta I       (BandEval; reads Ab, Y)
//   gpmi_band_eig.hip     bulge chase + bisection                 (BandEig; reads Ab)
//   gpmi_band_api.hip     create / destroy / refresh, RHS, getters, the GPMI_* knobs
// Every device buffer is a DevBuf, every stream and event an owner (gpmi_host.h):
// destruction is member order. Sizes come from gpmi_band_plan.h.
#pragma once

#include <vector>

#include "gpmi_internal.h"
#include "gpmi_band.h"
#include "gpmi_band_plan.h"
#include "gpmi_host.h"
#include "../../include/gpmi.h"

static_assert(gpmi::BAND_TS == GPMI_TS && gpmi::BAND_RLD == GPMI_RHS_LD &&
                  gpmi::BAND_TAN_MAX == GPMI_BAND_TAN_MAX,
              "gpmi_band_plan.h restates these");

namespace gpmi {
int op_view(const gpmi_op* op, OpView* v);   // gpmi_api.hip
}  // namespace gpmi

#pragma GCC visibility push(hidden)

namespace gpmi {

constexpr int TS = GPMI_TS;
constexpr int RLD = GPMI_RHS_LD;
constexpr int OUT_LD = BAND_OUT_LD;

// Dense -> band (see gpmi_band.hip). The ordering events ev_v, ev_t, ev_q also order
// the evaluator's work on the side stream.
struct BandReduce {
  // look-ahead: the next panel's QR (high-priority stream) beside the rest of the
  // SYR2K: a CholeskyQR panel beside syr2k_pipe_kernel on all but LA_FREE CUs, a
  // Householder panel beside syr2k_rest_kernel on la_grid workgroups
  int lookahead = 1, la_grid = 128;
  Stream s_pan;
  Event ev_col, ev_pan, ev_v, ev_t, ev_q;
  DevBuf<double> U;        // [n_pad][384] = [W | V | W] of the current panel
  DevBuf<double> X;        // [n_pad][128] (rows relative to the panel's trailing block)
  DevBuf<double> X2;       // [n_pad][128] X T (quadrant steps: out of place)
  DevBuf<double> Xp;       // symm split-K partials
  DevBuf<double> part;     // [2][HH_MAXG][HH_PART_LD] column partials
  DevBuf<double> pivrow;   // [2][128]
  DevBuf<double> tau;      // [nt][128]
  DevBuf<double> Tm;       // [nt][128][128] compact-WY T per panel
  DevBuf<double> tnp;      // tn partials [nch][128][128]
  DevBuf<double> tnp2;     // tn partials of V^T V (side stream) [nch][128][128]
  DevBuf<double> VtV, M, Zh;   // [128][128] each
  DevBuf<double> qtp;      // [HH_MAXG][128][16]
  DevBuf<double> qa, qb;   // [128][16] each
  DevBuf<unsigned> ctr;    // hh_panel hand-off counter: 8 shards, 64 B apart (512 bytes)
  DevBuf<int> err;         // hh_panel timeout flag
  // hh_panel_kernel needs all G workgroups co-resident: used only for G <= panel_maxg
  // (CU count x resident workgroups per CU, at most HH_PANEL_MAXG); a timed-out
  // hand-off makes band_reduce redo the reduction with hh_col_kernel launches
  int panel_maxg = HH_PANEL_MAXG;
  unsigned spin_limit = 1u << 24;
  int panel_fallbacks = 0;
  // CholeskyQR panel (gpmi_cholqr.hip; default, GPMI_BAND_PANEL=hh selects the
  // Householder panel): Q [n_pad][128], Gram partials, the three Cholesky factors
  // and inverses, the reconstruction's U^-T, V1, signs, scratch, failure flag
  int panel_mode = 0;        // 0 CholeskyQR, 1 Householder (single launch)
  int cq_fallbacks = 0;      // reductions redone with Householder panels
  DevBuf<double> Qb, cqpart, cqG;
  // per panel (cq_top_kernel forms every panel's R after the reduction):
  DevBuf<double> cqL;      // [nt][3][128][128] exact factors (first-order passes: by top)
  DevBuf<double> cqLinv;   // [nt][3][128][128] applied inverses
  DevBuf<double> cqS;      // [nt][128] reconstruction signs
  DevBuf<double> cqscr;    // [nt][128][128]
  DevBuf<int> cqflag;      // [nt][8]: [0..2] first-order flag per pass, [3] CholeskyQR
                           // succeeded, [4] failed (the guarded Householder panel ran),
                           // [6] the look-ahead SYR2K's tile tickets
  int la_free = LA_FREE, la_free_late = LA_FREE_LATE, la_late_mt = LA_LATE_MT;   // GPMI_LA_*
  bool poison = false;          // GPMI_BAND_POISON=1: Ab set to NaN before a K-first copy
  int cq_panel_fallbacks = 0;   // panels factored by the guarded Householder panel, or
                                // (past its single-launch size) by per-column launches
  int cq_host_checks = 0;       // panels past the single-launch size whose flag the host read
  // grouped tile orders of the look-ahead SYR2K (syr2k_tile_order)
  DevBuf<uint32_t> rorder;
  std::vector<int64_t> rorder_off;
  DevBuf<double> cqMinv;   // C = U^-T M3 of the current panel
  // T of a CholeskyQR panel from its reconstruction (cq_t_kernel) on the side stream
  // (not a stream of its own: the process's streams share GPU_MAX_HW_QUEUES hardware
  // queues, and two streams on one queue serialise): U S and V1^-1 per panel;
  // t_from_q[j]: panel j's T comes from there (the side stream's V^T V / tbuild_kernel
  // then run only if the panel fell back)
  DevBuf<double> cqUS;     // [nt][128][128]
  DevBuf<double> cqW;      // [nt][128][128]
  Event ev_rc;
  std::vector<char> t_from_q;
  std::vector<char> v_in_u;   // v_in_u[j]: panel j's reflectors are in U already
  double cq_fo[3] = {0.0, 1e-4, 3e-8};   // first-order thresholds on ||G - I||_F
};

// The evaluator's buffers, in four groups that each grow on demand to the etas of a
// call (per eta: BandPlan), and the io group of the core. reserve(neta) frees a group
// before it allocates it again (regrow, gpmi_host.h).
struct BandIo {
  int cap = 0;
  DevBuf<double> etas;   // [cap]
  DevBuf<double> out;    // [cap][OUT_LD]
  DevBuf<int> info;      // [cap]
  hipError_t reserve(int neta) {
    const int c = BandPlan::io_capacity(neta);
    return regrow(&cap, c, {sized(etas, c), sized(out, (size_t)c * OUT_LD), sized(info, c)});
  }
};

// block cyclic reduction of B + eta I (gpmi_bcr.hip)
struct BandBcr {
  int cap = 0;
  DevBuf<double> D[2], F[2];   // [cap][half][128][128] a level's reduced blocks, two in turn
  DevBuf<double> Y[2];         // [cap][half][128][16]
  DevBuf<double> L;    // [cap][nt][128][128]     every level's Linv, by original block
  DevBuf<double> W;    // [cap][nt][2][128][128]  every level's W_l, W_r, likewise
  DevBuf<double> Z;    // [cap][nt][128][16]
  DevBuf<double> X;    // [cap][nt][128][16]      derivative terms: X, then Z'
  DevBuf<double> Zp;
  DevBuf<double> G, G2, G3;   // [cap][nt][16][16]
  DevBuf<double> Ld;   // [cap][nt]
  DevBuf<int> Fail;    // [cap][nt]
  hipError_t reserve(int neta, const BandPlan& p) {
    const size_t e = (size_t)neta;
    return regrow(&cap, neta,
                  {sized(D[0], e * p.sH), sized(F[0], e * p.sH), sized(Y[0], e * p.sHY),
                   sized(D[1], e * p.sH), sized(F[1], e * p.sH), sized(Y[1], e * p.sHY),
                   sized(L, e * p.sL), sized(W, e * p.sW), sized(Z, e * p.sZ), sized(X, e * p.sZ),
                   sized(Zp, e * p.sZ), sized(G, e * p.sG), sized(G2, e * p.sG),
                   sized(G3, e * p.sG), sized(Ld, e * p.nt), sized(Fail, e * p.nt)});
  }
};

// selected inversion down the reduction tree (traceinv without eigenvalues)
struct BandSinv {
  int cap = 0;
  DevBuf<double> Zd;   // [cap][nt][128][128]     diagonal blocks of (B + eta I)^-1
  DevBuf<double> Zo;   // [cap][nt][2][128][128]  Z_lp, Z_rp of every eliminated block
  DevBuf<double> X;    // [cap][nt][2][128][128]  X_l, X_r
  DevBuf<double> Tr;   // [cap][nt] per-block traces, then [cap] sums
  hipError_t reserve(int neta, const BandPlan& p) {
    const size_t e = (size_t)neta;
    return regrow(&cap, neta, {sized(Zd, e * p.sL), sized(Zo, e * p.sW), sized(X, e * p.sW),
                               sized(Tr, e * p.sT)});
  }
};

// eta-tangents of the cyclic-reduction factor and of the selected inversion (traceinv
// of exponent 2, gpmi_bcr.hip bcr_d*): per eta of a chunk of at most BAND_TAN_MAX,
// strides per eta as the primal blocks
struct BandTan {
  int cap = 0;
  DevBuf<double> L;    // [cap][nt][128][128]     dLinv
  DevBuf<double> W;    // [cap][nt][2][128][128]  dW_l, dW_r
  DevBuf<double> X;    // [cap][nt][2][128][128]  dX_l, dX_r (bcr_dfac's scratch first)
  DevBuf<double> Zd;   // [cap][nt][128][128]
  DevBuf<double> Zo;   // [cap][nt][2][128][128]
  DevBuf<double> D[2], F[2];   // [cap][half][128][128]
  DevBuf<double> Tr;   // [cap][nt] per-block -tr dZ_pp, then [cap] sums
  hipError_t reserve(int neta, const BandPlan& p) {
    const size_t e = (size_t)neta;
    return regrow(&cap, neta,
                  {sized(L, e * p.sL), sized(W, e * p.sW), sized(X, e * p.sW), sized(Zd, e * p.sL),
                   sized(Zo, e * p.sW), sized(D[0], e * p.sH), sized(F[0], e * p.sH),
                   sized(D[1], e * p.sH), sized(F[1], e * p.sH), sized(Tr, e * p.sT)});
  }
};

// eta-derivative terms: the sequential kernel's banded factor blocks and solution
// block, and the two higher Grams (of either path)
struct BandDer {
  int cap = 0;
  DevBuf<double> fac;    // [cap][nt][2][128][128]
  DevBuf<double> ysol;   // [cap][n_pad][16]
  DevBuf<double> der;    // [cap][2][16][16]
  hipError_t reserve(int neta, const BandPlan& p) {
    const size_t e = (size_t)neta;
    return regrow(&cap, neta, {sized(fac, e * p.sW), sized(ysol, e * p.sZ),
                               sized(der, e * 2 * RLD * RLD)});
  }
};

struct BandEval {
  BandPlan plan{0};
  std::vector<int> levels;   // bcr_levels(nt)
  int bcr_mode = 2;   // 0 sequential band_chol_kernel, 1 cyclic reduction, 2 auto:
                      // cyclic reduction up to 64 eta per call (measured at N = 16384:
                      // 1 eta 9.97 -> 1.30 ms, 8 eta 10.05 -> 1.85, 64 eta 9.9 -> 8.8;
                      // the sequential kernel's time is flat up to the CU count)
  BandBcr bcr;
  DevBuf<double> F0;   // [nt - 1][128][128] the band's subdiagonal blocks (first use)
  BandSinv sinv;
  BandTan tan;
  BandDer der;
  double sinv_ms = 0.0, der_ms = 0.0;
  // what the read-backs (gpmi_band_get_solution / _get_sinv) may return: host
  // bookkeeping of the last der_terms / selected-inversion chunk, cleared by a reduction
  int sol_path = 0;            // 0 nothing, 1 der.ysol (sequential), 2 bcr.X
  int sol_neta = 0;
  std::vector<int> sol_info;   // that chunk's info per eta
  int sinv_neta = 0;
  bool sinv_tan = false;       // the tangents dZd, dZo belong to the same chunk
};

// eigenvalues (bulge chase + bisection), computed on request
struct BandEig {
  DevBuf<double> Ac;   // [n_pad][n_pad] chase copy of the band (lower), launch form only
  DevBuf<double> td;   // td_doubles(n_pad): diagonal, squared subdiagonal, eigenvalues, slots
  double eig_ms = 0.0;
  bool td_valid = false;   // td holds the tridiagonal of the current band (read-back)
  // systolic chase (chase_systolic_kernel): one workgroup per position, all
  // co-resident; used when chase_maxg (CU count x resident workgroups per CU)
  // covers the positions, else (and after a timed-out hand-off) the launch form
  DevBuf<unsigned long long> cmsg;   // reflector, column slots [2][K + 1][2][2 CHASE_MSG], err
  int chase_maxg = 0;
  int split_maxg = 0;        // the same for chase_split_kernel (2K workgroups)
  unsigned chase_spin = 1u << 24;
  int chase_systolic = 0;    // the last eigenvalues(): 2 split, 1 one-per-position, 0 launches
  int chase_fallbacks = 0;   // systolic attempts that timed out and reran the launch form
};

int band_reduce(gpmi_band* b, const double* K, const std::vector<double>* yh = nullptr);
// Y <- Q_j^T Y for panel j (Y = b->Y, rows from 128 (j + 1)) on stream st.
int qt_panel(gpmi_band* b, int j, hipStream_t st);

}  // namespace gpmi

struct gpmi_band {
  int device = 0;
  int64_t n = 0, n_pad = 0;
  int nt = 0, ncu = 256;
  gpmi::Stream stream;
  gpmi::Stream side;   // V^T V and T of a panel beside its SYMM; the selected inversion
                       // beside the derivative solves
  gpmi::Event ev0, ev1, ev2, ev3;   // timing
  gpmi::DevBuf<double> Ab;   // [n_pad][n_pad]: band (diagonal tiles, triu of subdiagonal
                             // tiles) + Householder vectors below the band
  gpmi::DevBuf<double> Y;    // [n_pad][16] = Q^T R
  int nrhs = 0;
  gpmi::BandIo io;
  double reduce_ms = 0.0, rhs_ms = 0.0, loglik_ms = 0.0;
  gpmi::BandReduce red;
  gpmi::BandEval eval;
  gpmi::BandEig eig;
};

#pragma GCC visibility pop
