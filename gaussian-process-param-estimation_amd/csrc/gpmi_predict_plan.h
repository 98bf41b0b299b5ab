// Chunking, launch list and workspace sizes of the prediction terms (gpmi_api.hip:
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

}  // namespace gpmi

#pragma GCC visibility pop
