// The cell list of the tapered Matérn assembly (gpmi_sp_create_matern, d <= 3), HIP-free:
// cells of width >= xcut * scale_k, so a kept pair is in the same or an adjacent cell;
// coarsened while there are more cells than max(4 n, 1024). The points are counting-sorted
// into cells, and the rows' locality order is the Morton order of the occupied cells.
// Host check: tests/host/cell_plan_check.cpp.
// A new point (the cross assembly of the sparse prediction) is not in the plan: its cell
// comes from its coordinates (cross_cell_coord, cross_cell_range), compiled by the host and
// by cross_cell_*_kernel alike. Host check: tests/host/cross_plan_check.cpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define GPMI_CELL_HD __host__ __device__
#else
#define GPMI_CELL_HD
#endif

namespace gpmi {

// The unclamped cell coordinate floor((t - pmin) / wid) of a new point in one dimension,
// limited to [-2, gdim + 1] before the integer conversion (so +-inf and huge coordinates
// do not overflow; NaN gives -2). A training point p with |t - p| <= xcut |scale| < wid has
// a cell coordinate (in [0, gdim - 1]) within 1 of it: the kept-pair guarantee of cell_plan.
GPMI_CELL_HD inline int cross_cell_coord(double t, double pmin, double wid, int gdim) {
  double x = std::floor((t - pmin) / wid);
  if (!(x >= -2.0)) x = -2.0;
  if (x > (double)gdim + 1.0) x = (double)gdim + 1.0;
  return (int)x;
}

// The neighbour cells q - 1 .. q + 1 of that coordinate inside the grid: [*lo, *hi], empty
// (*lo > *hi) for a point more than one cell outside the training box.
GPMI_CELL_HD inline void cross_cell_range(int q, int gdim, int* lo, int* hi) {
  *lo = q - 1 < 0 ? 0 : q - 1;
  *hi = q + 1 > gdim - 1 ? gdim - 1 : q + 1;
}

struct CellPlan {
  double pmin[3], wid[3];      // the grid's origin and cell widths
  int64_t total = 0;           // cells
  std::vector<int> gdim;       // [d] cells per dimension
  std::vector<int> cell;       // [n] cell of each point (dimension 0 fastest)
  std::vector<int> start;      // [total + 1] prefix sum of the cell populations
  std::vector<int> perm;       // [n] the points cell by cell, ascending index per cell
  std::vector<int> lorder;     // [n] locality order of the rows; empty: original order
};

// Morton (Z-order) key of a cell's integer coordinates (d <= 3, 21 bits each).
inline uint64_t morton3(const int64_t (&q)[3], int d) {
  uint64_t key = 0;
  for (int b = 20; b >= 0; --b)
    for (int k = 0; k < d; ++k) key = (key << 1) | (uint64_t)((q[k] >> b) & 1);
  return key;
}

// The plan for n points [n][d], d <= 3. False (all-pairs kernels instead): NaN / inf
// points, a cell width that is not positive and finite, or more than max(4 n, 1024) cells
// after 64 doublings. reorder: fill lorder (n > 1).
inline bool cell_plan(const double* points, int64_t n, int d, const double* scale, double xcut,
                      bool reorder, CellPlan* out) {
  CellPlan& p = *out;
  double pmax[3];
  int64_t G[3] = {1, 1, 1};
  bool cells = true;
  for (int k = 0; k < d; ++k) {
    p.pmin[k] = pmax[k] = points[k];
    for (int64_t i = 0; i < n; ++i) {
      const double v = points[i * d + k];
      if (!std::isfinite(v)) cells = false;
      p.pmin[k] = std::min(p.pmin[k], v);
      pmax[k] = std::max(pmax[k], v);
    }
    p.wid[k] = xcut * std::fabs(scale[k]) * (1.0 + 1e-9);
    if (!(p.wid[k] > 0.0) || !std::isfinite(p.wid[k])) cells = false;
  }
  int64_t total = 0;
  for (int it = 0; cells && it < 64; ++it) {
    total = 1;
    for (int k = 0; k < d; ++k) {
      const double g = std::floor((pmax[k] - p.pmin[k]) / p.wid[k]) + 1.0;
      G[k] = g > 1e9 ? (int64_t)1e9 : (int64_t)g;
      total = std::min<int64_t>(total * G[k], (int64_t)1 << 40);
    }
    if (total <= std::max<int64_t>(4 * n, 1024)) break;
    for (int k = 0; k < d; ++k) p.wid[k] *= 2.0;
  }
  if (!cells || total > std::max<int64_t>(4 * n, 1024)) return false;
  p.total = total;
  p.cell.assign(n, 0);
  p.start.assign(total + 1, 0);
  p.perm.assign(n, 0);
  p.gdim.assign(d, 0);
  p.lorder.clear();
  for (int k = 0; k < d; ++k) p.gdim[k] = (int)G[k];
  for (int64_t i = 0; i < n; ++i) {
    int64_t c = 0, mul = 1;
    for (int k = 0; k < d; ++k) {
      int64_t q = (int64_t)std::floor((points[i * d + k] - p.pmin[k]) / p.wid[k]);
      q = std::min<int64_t>(std::max<int64_t>(q, 0), G[k] - 1);
      c += q * mul;
      mul *= G[k];
    }
    p.cell[i] = (int)c;
    ++p.start[c + 1];
  }
  for (int64_t c = 0; c < total; ++c) p.start[c + 1] += p.start[c];
  std::vector<int> fillp(p.start.begin(), p.start.end() - 1);
  for (int64_t i = 0; i < n; ++i) p.perm[fillp[p.cell[i]]++] = (int)i;   // ascending i per cell
  if (reorder && n > 1) {
    std::vector<std::pair<uint64_t, int64_t>> keys;
    keys.reserve(total);
    for (int64_t c = 0; c < total; ++c) {
      if (p.start[c + 1] == p.start[c]) continue;
      int64_t q[3] = {0, 0, 0}, cc = c;
      for (int k = 0; k < d; ++k) {
        q[k] = cc % G[k];
        cc /= G[k];
      }
      keys.emplace_back(morton3(q, d), c);
    }
    std::sort(keys.begin(), keys.end());
    p.lorder.reserve(n);
    for (const auto& kc : keys)
      for (int q = p.start[kc.second]; q < p.start[kc.second + 1]; ++q)
        p.lorder.push_back(p.perm[q]);
  }
  return true;
}

}  // namespace gpmi
