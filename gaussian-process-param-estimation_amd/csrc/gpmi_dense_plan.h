// Launch list of the dense blocked Cholesky (gpmi_dense_factor.hip: schedule): which kernel runs
// on which tiles with which operand range, in stream order, for nt tile rows, outer
// panels of `outer` tile columns and one of two panel schedules. Plain arithmetic, no
// HIP here, so that the list is replayed on the host (tests/host/dense_plan_check.cpp).
//
// Both schedules factor the outer panel [c0, c0 + W) and then run one bulk trailing SYRK
// (kdim = 128 W) over everything right of it. Inside the panel:
//   DENSE_REC  recursive halving: factor the left half, one band SYRK (kdim = 128 x half
//              width) onto the right half, factor the right half; a single column is
//              DIAG then PANEL.
//   DENSE_COL  left-looking: per column k, DIAG then one COLPANEL launch that brings
//              column k up to date from the panel's columns [c0, k) (kdim = 128 (k - c0)),
//              runs the panel step on it and, while k + 1 is inside the panel, completes
//              the next diagonal tile.
// Either way a tile receives its updates in ascending operand order, in chunks whose
// boundaries are multiples of 128: the fp64 operation sequence per element is the same.
#pragma once

#include <algorithm>
#include <vector>

#pragma GCC visibility push(hidden)   // (inline helpers: no exported symbols)

namespace gpmi {

constexpr int DENSE_TS = 128;   // = GPMI_TS

enum DenseMode { DENSE_REC = 0, DENSE_COL = 1 };
enum DenseKind { DENSE_DIAG = 0, DENSE_PANEL = 1, DENSE_COLPANEL = 2, DENSE_SYRK = 3 };

struct DenseLaunch {
  int kind;
  int col;         // DIAG / PANEL / COLPANEL: the tile column k; SYRK: its first tile column
  int w;           // tile columns the launch writes (SYRK: the band's width; else 1)
  int r0, r1;      // tile rows [r0, r1) the launch writes in those columns
  int p0, kdim;    // operand element columns [p0, p0 + kdim) of the update it applies
                   // (DIAG, PANEL: none, kdim = 0)
  bool next_diag;  // COLPANEL: also completes diagonal tile (k + 1, k + 1) from
                   // [p0, p0 + kdim + 128)
  bool from_k;     // SYRK: the factorization's first bulk update (C is read from K)
};

inline void dense_plan_rec(int nt, int c0, int W, std::vector<DenseLaunch>* out) {
  if (W == 1) {
    out->push_back({DENSE_DIAG, c0, 1, c0, c0 + 1, 0, 0, false, false});
    if (c0 + 1 < nt) out->push_back({DENSE_PANEL, c0, 1, c0 + 1, nt, 0, 0, false, false});
    return;
  }
  const int h = W / 2;
  dense_plan_rec(nt, c0, h, out);
  out->push_back({DENSE_SYRK, c0 + h, W - h, c0 + h, nt, c0 * DENSE_TS, h * DENSE_TS, false,
                  false});
  dense_plan_rec(nt, c0 + h, W - h, out);
}

inline std::vector<DenseLaunch> dense_plan(int nt, int outer, int mode) {
  std::vector<DenseLaunch> out;
  for (int c0 = 0; c0 < nt; c0 += outer) {
    const int W = std::min(outer, nt - c0);
    if (mode == DENSE_REC) {
      dense_plan_rec(nt, c0, W, &out);
    } else {
      for (int k = c0; k < c0 + W; ++k) {
        out.push_back({DENSE_DIAG, k, 1, k, k + 1, 0, 0, false, false});
        if (k + 1 < nt)
          out.push_back({DENSE_COLPANEL, k, 1, k + 1, nt, c0 * DENSE_TS, (k - c0) * DENSE_TS,
                         k + 1 < c0 + W, false});
      }
    }
    const int c1 = c0 + W;
    if (c1 >= nt) break;
    out.push_back({DENSE_SYRK, c1, nt - c1, c1, nt, c0 * DENSE_TS, W * DENSE_TS, false,
                   c0 == 0});
  }
  return out;
}

}  // namespace gpmi

#pragma GCC visibility pop
