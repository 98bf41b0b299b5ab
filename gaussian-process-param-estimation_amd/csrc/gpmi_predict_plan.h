// Chunking, launch list and workspace sizes of the prediction terms (gpmi_dense_predict.hip:
// gpmi_op_predict_terms; kernels in gpmi_predict.hip). Plain arithmetic, no HIP here, so
// that the list is replayed on the host (tests/host/predict_plan_check.cpp).
//
// The working block T holds one chunk of NS test columns TRANSPOSED: T[j][i], row j a
// test column, i the training index, leading dimension n_pad (the layout of a
// cross-correlation [n*][n]). The forward substitution T <- L^-1 T runs in place over
// outer panels [kb, ke) of `outer` tile rows, in stream order:
//   PRED_DIAG  k   one workgroup per column tile: inside the panel, left-looking,
//                  T_k -= L_{k,[kb,k)} V_[kb,k) (nothing at k == kb), then
//                  V_k = Linv_kk T_k and, with the tile on chip, the partials
//                  Y_k^T V_k and the column sums of squares into part[k][NS][17];
//   PRED_TRAIL     after the panel, T_i -= L_{i,[kb,ke)} V_[kb,ke) for every tile row
//                  i >= ke and every column tile (k-depth 128 (ke - kb)).
// A tile row thus receives its operand range once, in ascending contiguous chunks with
// tile boundaries, from finished V tiles, before its diagonal step.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define GPMI_PLAN_HD __host__ __device__
#else
#define GPMI_PLAN_HD
#endif

#pragma GCC visibility push(hidden)   // (inline helpers: no exported symbols)

namespace gpmi {

constexpr int PRED_TS = 128;          // = GPMI_TS
constexpr int PRED_LD = 17;           // per test column: 16 entries of Y^T v, then v^T v
constexpr int PRED_MAX_CHUNK = 4096;  // widest chunk (columns)
constexpr int64_t PRED_T_BYTES = (int64_t)512 << 20;   // the working block's budget
constexpr int PRED_GROUP = 8;         // column tiles per group of the trailing product
constexpr int PRED_OUTER = 4;         // widest outer panel of the solve (tile rows)

// Outer panel width of the solve: the factorization's (gpmi_op_set_outer), but at most
// PRED_OUTER. Inside a panel only the chunk's column tiles run side by side (32 workgroups
// for 4096 columns on 256 CUs), so the in-panel share of the flops, ~ width / nt, costs
// eight times its weight: N = 16384, n* = 4096 measured 38.5 / 29.1 / 25.6 / 25.6 ms at
// widths 16 / 8 / 4 / 2 (the trailing product at 0.77 / 0.81 / 0.77 / 0.69 of peak).
inline int predict_outer(int op_outer) { return std::max(1, std::min(op_outer, PRED_OUTER)); }

// Chunk width in columns (a multiple of 128): `override_cols` (GPMI_PREDICT_CHUNK; 0:
// none) or as many as the budget holds, at least one tile and at most PRED_MAX_CHUNK.
// < 0: the override is not a positive multiple of 128.
inline int predict_chunk_cols(int64_t n_pad, int64_t override_cols) {
  if (override_cols != 0) {
    if (override_cols < 0 || override_cols % PRED_TS || override_cols > (1 << 20)) return -1;
    return (int)override_cols;
  }
  int64_t c = PRED_T_BYTES / (8 * n_pad) / PRED_TS * PRED_TS;
  c = std::max<int64_t>(PRED_TS, std::min<int64_t>(PRED_MAX_CHUNK, c));
  return (int)c;
}

struct PredictChunk {
  int64_t j0;   // first test point
  int cols;     // test points in the chunk (<= NS)
  int nct;      // column tiles the chunk runs: ceil(cols / 128)
};

inline std::vector<PredictChunk> predict_chunks(int64_t nstar, int NS) {
  std::vector<PredictChunk> out;
  for (int64_t j0 = 0; j0 < nstar; j0 += NS) {
    const int cols = (int)std::min<int64_t>(NS, nstar - j0);
    out.push_back({j0, cols, (cols + PRED_TS - 1) / PRED_TS});
  }
  return out;
}

// Workspace in doubles for chunks of NS columns, the widest used being `wide` columns
// (the call's min(NS, nstar) rounded up to a tile): T [wide][n_pad],
// part [nt][wide][17], out [wide][17].
struct PredictSizes {
  size_t T, part, out;
};

inline PredictSizes predict_sizes(int64_t n_pad, int nt, int wide) {
  return {(size_t)wide * (size_t)n_pad, (size_t)nt * wide * PRED_LD, (size_t)wide * PRED_LD};
}

enum PredictKind { PRED_DIAG = 0, PRED_TRAIL = 1 };

struct PredictLaunch {
  int kind;
  int r0, r1;   // tile rows [r0, r1) the launch updates (DIAG: [k, k + 1))
  int kb, ke;   // operand tile rows [kb, ke) of the update it applies (empty: none)
};

inline std::vector<PredictLaunch> predict_plan(int nt, int outer) {
  std::vector<PredictLaunch> out;
  for (int kb = 0; kb < nt; kb += outer) {
    const int ke = std::min(nt, kb + outer);
    for (int k = kb; k < ke; ++k) out.push_back({PRED_DIAG, k, k + 1, kb, k});
    if (ke < nt) out.push_back({PRED_TRAIL, ke, nt, kb, ke});
  }
  return out;
}

// Tile (i, j) of workgroup q of a trailing product over ni tile rows and nct column
// tiles: column groups of PRED_GROUP tiles, row-major inside a group, so that the 64
// workgroups in flight on one XCD cover 8 rows x 8 columns and share 8 + 8 operand
// slabs in its L2. A bijection of [0, ni * nct).
GPMI_PLAN_HD inline void predict_tile(int q, int ni, int nct, int* pi, int* pj) {
  const int full = nct / PRED_GROUP;            // whole column groups
  const int per = ni * PRED_GROUP;              // tiles of one
  if (q < full * per) {
    const int g = q / per, r = q % per;
    *pi = r / PRED_GROUP;
    *pj = g * PRED_GROUP + r % PRED_GROUP;
  } else {
    const int w = nct - full * PRED_GROUP;      // the ragged last group
    const int r = q - full * per;
    *pi = r / w;
    *pj = full * PRED_GROUP + r % w;
  }
}

// ---------------------------------------------------------------------------
// Joint covariance of the test points (gpmi_dense_predict.hip: gpmi_op_predict_cov; kernels
// pred_cov_partial_kernel / pred_cov_reduce_kernel in gpmi_predict.hip):
//   C0 = K** - V V^T,  V = L^-1 K*^T kept for ALL test points.
// The working block is then the whole T [nsp][n_pad], nsp = n* rounded up to a tile;
// the forward substitution still runs chunk by chunk on the row range of each chunk
// (T is transposed: a chunk is a contiguous row range), part / out stay chunk-wide.
// C0's lower tiles (J, L), J >= L, are SYRK-shaped products of depth n_pad; the depth is
// split into S pieces of whole tile rows, one workgroup per (tile, piece) writing a
// partial tile, summed in ascending piece order by the second kernel.
// ---------------------------------------------------------------------------
constexpr int64_t PRED_COV_BYTES = (int64_t)8 << 30;   // cap on T + K** + the partials

// First row of a chunk's range inside the whole block (chunk widths are whole tiles).
inline int64_t predict_cov_row0(const PredictChunk& ch) { return ch.j0; }

inline int64_t predict_cov_tiles(int nct) { return (int64_t)nct * (nct + 1) / 2; }

// Workspace in doubles: T [nsp][n_pad], cov [nsp][nsp], part [tiles][S][128][128].
struct PredictCovSizes {
  size_t T, cov, part;
};

inline PredictCovSizes predict_cov_sizes(int64_t n_pad, int nct, int S) {
  const size_t nsp = (size_t)nct * PRED_TS;
  return {nsp * (size_t)n_pad, nsp * nsp,
          (size_t)predict_cov_tiles(nct) * (size_t)S * PRED_TS * PRED_TS};
}

// Whether a covariance call of nct column tiles at split S stays within the cap
// (in tiles, so that no product overflows for any int nct).
inline bool predict_cov_fits(int64_t n_pad, int nct, int S) {
  const int64_t tile_bytes = (int64_t)8 * PRED_TS * PRED_TS;
  const int64_t nt = n_pad / PRED_TS;
  const int64_t tiles = (int64_t)nct * nt + (int64_t)nct * nct + predict_cov_tiles(nct) * S;
  return tiles <= PRED_COV_BYTES / tile_bytes;
}

// Tile rows [begin(p), begin(p + 1)) of depth piece p of S, 1 <= S <= nt: balanced,
// ragged where S does not divide nt, never empty.
GPMI_PLAN_HD inline int predict_cov_piece_begin(int nt, int S, int p) {
  return (int)((int64_t)p * nt / S);
}

// First double of the partial tile of (lower tile q, piece p).
GPMI_PLAN_HD inline int64_t predict_cov_part_off(int64_t q, int S, int p) {
  return (q * S + p) * (int64_t)(PRED_TS * PRED_TS);
}

// Number of depth pieces for `ntiles` lower tiles of depth nt tile rows on `slots`
// resident workgroups (two per CU); `override_split` (GPMI_PREDICT_COV_SPLIT; <= 0:
// none) replaces the choice, clipped to [1, nt]. In units of one 128^3 product per
// slot the ntiles * S workgroups run ceil(ntiles S / slots) rounds of ceil(nt / S)
// products, so (as symm_chunk, gpmi_band_plan.h) the S minimising rounds x depth ends
// the grid in whole rounds; each partial tile adds a 128 KB write and read, about one
// product's time per slot when all slots stream at once (128 KB x 2 at HBM rate / slots
// against 2 x 128^3 flops at the fp64 MFMA rate / slots), counted as 1 / slots each.
// Ties go to the smaller S. n* = 256, N = 16384: 3 tiles -> S = 128 (384 workgroups, one
// round); n* = 4096: 528 tiles -> S = 8 (4224 workgroups, 8.25 rounds run as 9 of
// depth 16: 144 + 8, against 2 rounds of depth 128 unsplit). Measured there, product ms
// at S = 1 / 2 / 4 / 8 / 16 / 32: 6.40 / 5.30 / 4.82 / 4.61 / 4.43 / 4.61, the whole
// call within 0.3 ms of each other from S = 2 on.
inline int predict_cov_split(int64_t ntiles, int nt, int slots, int64_t override_split = 0) {
  if (nt < 1) return 1;
  if (override_split > 0) return (int)std::min<int64_t>(override_split, nt);
  slots = std::max(slots, 1);
  int best = 1;
  double bc = -1.0;
  for (int S = 1; S <= nt; ++S) {
    const int64_t w = ntiles * S;
    const int64_t rounds = (w + slots - 1) / slots;
    const int depth = (nt + S - 1) / S;
    const double c = (double)rounds * depth + (double)w / slots;
    if (bc < 0.0 || c < bc) {
      bc = c;
      best = S;
    }
  }
  return best;
}

}  // namespace gpmi

#pragma GCC visibility pop
