// The cell rule for a new point of csrc/gpmi_cell_plan.h (cross_cell_coord,
// cross_cell_range; what cross_cell_count_kernel / cross_cell_fill_kernel visit) on the
// host. For plans in d = 1, 2, 3 and new points inside, on the faces of, just outside and
// far outside the training box:
//   * every training point within xcut * |scale_k| of the new point in every dimension lies
//     in a visited cell (the kept-pair guarantee);
//   * the visited cells are inside the grid and distinct, at most 3^d of them;
//   * a point more than one cell outside the box visits none;
//   * +-inf, NaN and huge coordinates give a coordinate in [-2, gdim + 1] (no overflow in
//     the integer conversion) and never a cell out of range.
// Exit status 0: all held. Build: c++ -std=c++17 -I <csrc> cross_plan_check.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <set>
#include <vector>

#include "gpmi_cell_plan.h"

using namespace gpmi;

static int failures = 0;
static const char* ctx = "";

#define CHECK(cond)                                                                \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      if (++failures <= 20) std::fprintf(stderr, "%s: line %d: %s\n", ctx, __LINE__, #cond); \
    }                                                                              \
  } while (0)

static uint64_t rng_state = 98765;
static double uniform() {   // xorshift64*, in [0, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (double)((rng_state * 2685821657736338717ull) >> 11) / 9007199254740992.0;
}

// The cells a new point visits: per dimension [lo, hi]; returns their ids (dimension 0
// fastest), empty when a dimension's range is empty.
static std::vector<int64_t> visited(const CellPlan& p, int d, const double* t, int* lo, int* hi) {
  std::vector<int64_t> ids;
  for (int k = 0; k < 3; ++k) lo[k] = hi[k] = 0;
  for (int k = 0; k < d; ++k) {
    const int q = cross_cell_coord(t[k], p.pmin[k], p.wid[k], p.gdim[k]);
    CHECK(q >= -2 && q <= p.gdim[k] + 1);
    cross_cell_range(q, p.gdim[k], &lo[k], &hi[k]);
    if (lo[k] > hi[k]) return ids;
    CHECK(lo[k] >= 0 && hi[k] <= p.gdim[k] - 1 && hi[k] - lo[k] <= 2);
  }
  const int g0 = p.gdim[0], g1 = d > 1 ? p.gdim[1] : 1;
  for (int c2 = lo[2]; c2 <= hi[2]; ++c2)
    for (int c1 = lo[1]; c1 <= hi[1]; ++c1)
      for (int c0 = lo[0]; c0 <= hi[0]; ++c0) ids.push_back(c0 + (int64_t)g0 * (c1 + (int64_t)g1 * c2));
  return ids;
}

static void check_point(const CellPlan& p, const std::vector<double>& pts, int64_t n, int d,
                        const double* scale, double xcut, const double* t, bool expect_none) {
  int lo[3], hi[3];
  const std::vector<int64_t> ids = visited(p, d, t, lo, hi);
  std::set<int64_t> uniq(ids.begin(), ids.end());
  CHECK(uniq.size() == ids.size());
  CHECK(ids.size() <= (size_t)(d == 1 ? 3 : d == 2 ? 9 : 27));
  for (int64_t id : ids) CHECK(id >= 0 && id < p.total);
  if (expect_none) CHECK(ids.empty());
  for (int64_t i = 0; i < n; ++i) {
    bool close = true;
    for (int k = 0; k < d; ++k)
      close = close && std::fabs(t[k] - pts[i * d + k]) <= xcut * std::fabs(scale[k]);
    if (!close) continue;
    CHECK(uniq.count(p.cell[i]) == 1);
  }
}

static void check_plan(const char* name, int64_t n, int d, const double* scale, double xcut) {
  ctx = name;
  const double span[3] = {1.7, 0.9, 1.3};
  std::vector<double> pts((size_t)n * d);
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < d; ++k) pts[i * d + k] = -0.3 + span[k] * uniform();
  CellPlan p;
  const bool ok = cell_plan(pts.data(), n, d, scale, xcut, true, &p);
  CHECK(ok);
  if (!ok) return;
  double pmax[3] = {0, 0, 0};
  for (int k = 0; k < d; ++k) {
    pmax[k] = pts[k];
    for (int64_t i = 0; i < n; ++i) pmax[k] = std::max(pmax[k], pts[i * d + k]);
  }
  double t[3];
  // inside the box, and the training points themselves
  for (int r = 0; r < 200; ++r) {
    for (int k = 0; k < d; ++k) t[k] = p.pmin[k] + (pmax[k] - p.pmin[k]) * uniform();
    check_point(p, pts, n, d, scale, xcut, t, false);
  }
  for (int64_t i = 0; i < n; i += 7) check_point(p, pts, n, d, scale, xcut, &pts[i * d], false);
  // on the faces and the corners, and just outside them (within one cutoff, then within
  // one cell: still visiting), in every combination of dimensions
  const double off[7] = {0.0, 1e-15, 1e-9, 0.5, 0.999, 1.0, 1.0 + 1e-12};
  for (int m = 0; m < 27; ++m)
    for (double f : off) {
      int mm = m;
      for (int k = 0; k < d; ++k) {
        const int side = mm % 3;
        mm /= 3;
        const double cut = xcut * std::fabs(scale[k]);
        t[k] = side == 0 ? p.pmin[k] - f * cut
                         : side == 1 ? pmax[k] + f * cut
                                     : p.pmin[k] + (pmax[k] - p.pmin[k]) * uniform();
      }
      check_point(p, pts, n, d, scale, xcut, t, false);
    }
  // far outside in one dimension (more than one cell beyond the box): no cell
  for (int k = 0; k < d; ++k)
    for (double far : {-1.0, 1.0})
      for (double mult : {2.01, 3.0, 17.0, 1e6, 1e300}) {
        for (int j = 0; j < d; ++j) t[j] = p.pmin[j] + (pmax[j] - p.pmin[j]) * uniform();
        // (beyond the last cell's far edge, which may lie past pmax)
        t[k] = far < 0 ? p.pmin[k] - mult * p.wid[k]
                       : p.pmin[k] + (p.gdim[k] + mult) * p.wid[k];
        check_point(p, pts, n, d, scale, xcut, t, true);
      }
  // non-finite and huge coordinates
  const double inf = std::numeric_limits<double>::infinity();
  const double bad[6] = {inf, -inf, std::nan(""), std::numeric_limits<double>::max(),
                         -std::numeric_limits<double>::max(), 1e308};
  for (int k = 0; k < d; ++k)
    for (double b : bad) {
      for (int j = 0; j < d; ++j) t[j] = p.pmin[j] + (pmax[j] - p.pmin[j]) * uniform();
      t[k] = b;
      check_point(p, pts, n, d, scale, xcut, t, true);
    }
}

int main() {
  const double scale[3] = {0.05, -0.08, 0.11};
  const double fine[3] = {0.02, 0.02, 0.02};
  int cases = 0;
  for (int d = 1; d <= 3; ++d)
    for (int64_t n : {1, 2, 97, 700}) {
      check_plan("scattered", n, d, scale, 1.3);
      ++cases;
    }
  check_plan("coarsened", 50, 3, fine, 1.0);   // widths doubled until the grid fits
  ++cases;
  if (failures) {
    std::fprintf(stderr, "cross_plan_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("cross_plan_check: %d cases OK\n", cases);
  return 0;
}
