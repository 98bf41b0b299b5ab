// csrc/gpmi_cell_plan.h on the host. For scattered 1D / 2D / 3D points, one case whose grid
// is coarsened and one that falls back to all pairs:
//   * every point is in the cell its coordinates say (pmin, wid, gdim; dimension 0 fastest);
//   * start is the prefix sum of the cell populations and ends at n;
//   * perm lists each cell's points in ascending index, every point once;
//   * lorder is a permutation of 0 .. n-1 that keeps each cell's points together (and is
//     empty when the order is not asked for);
//   * any two points closer than xcut * |scale_k| in every dimension lie in the same or in
//     adjacent cells (what csr_cell_count_kernel relies on);
//   * there are at most max(4 n, 1024) cells;
//   * non-finite points, a width that is not positive and too many cells give no plan.
// Exit status 0: all held. Build: c++ -std=c++17 -I <csrc> cell_plan_check.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

static uint64_t rng_state = 12345;
static double uniform() {   // xorshift64*, in [0, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (double)((rng_state * 2685821657736338717ull) >> 11) / 9007199254740992.0;
}

static std::vector<double> scatter(int64_t n, int d, const double* span) {
  std::vector<double> p((size_t)n * d);
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < d; ++k) p[i * d + k] = -0.3 + span[k] * uniform();
  return p;
}

static void cell_coords(const CellPlan& p, int d, int c, int64_t* q) {
  for (int k = 0; k < d; ++k) {
    q[k] = c % p.gdim[k];
    c /= p.gdim[k];
  }
}

// a plan for these points, checked; returns the number of width doublings it took
static int check_plan(const char* name, const std::vector<double>& pts, int64_t n, int d,
                      const double* scale, double xcut, bool reorder) {
  ctx = name;
  CellPlan p;
  const bool ok = cell_plan(pts.data(), n, d, scale, xcut, reorder, &p);
  CHECK(ok);
  if (!ok) return -1;
  CHECK((int)p.gdim.size() == d && (int64_t)p.cell.size() == n && (int64_t)p.perm.size() == n);
  int64_t total = 1;
  for (int k = 0; k < d; ++k) {
    CHECK(p.gdim[k] >= 1);
    total *= p.gdim[k];
    CHECK(p.wid[k] >= xcut * std::fabs(scale[k]));
  }
  CHECK(total == p.total && (int64_t)p.start.size() == total + 1);
  CHECK(total <= std::max<int64_t>(4 * n, 1024));
  const int doublings = (int)std::lround(std::log2(p.wid[0] / (xcut * std::fabs(scale[0]))));
  // every point in the cell its coordinates say
  std::vector<int> pop((size_t)total, 0);
  for (int64_t i = 0; i < n; ++i) {
    CHECK(p.cell[i] >= 0 && p.cell[i] < total);
    int64_t q[3] = {0, 0, 0};
    cell_coords(p, d, p.cell[i], q);
    for (int k = 0; k < d; ++k) {
      const double x = (pts[i * d + k] - p.pmin[k]) / p.wid[k];
      CHECK(x >= 0.0);
      // (the last cell also takes a point that rounds onto the upper edge)
      CHECK((double)q[k] <= x && (x < (double)(q[k] + 1) || q[k] == p.gdim[k] - 1));
    }
    ++pop[(size_t)p.cell[i]];
  }
  // prefix sums, and each cell's points in ascending index, every point once
  CHECK(p.start[0] == 0 && p.start[(size_t)total] == n);
  std::vector<char> seen((size_t)n, 0);
  for (int64_t c = 0; c < total; ++c) {
    CHECK(p.start[c + 1] - p.start[c] == pop[(size_t)c]);
    for (int q = p.start[c]; q < p.start[c + 1]; ++q) {
      const int i = p.perm[q];
      CHECK(i >= 0 && i < n && !seen[(size_t)i] && p.cell[i] == c);
      if (i >= 0 && i < n) seen[(size_t)i] = 1;
      if (q > p.start[c]) CHECK(p.perm[q - 1] < i);
    }
  }
  // the locality order: a permutation, cell by cell
  if (!reorder || n <= 1) {
    CHECK(p.lorder.empty());
  } else {
    CHECK((int64_t)p.lorder.size() == n);
    std::vector<char> in((size_t)n, 0);
    std::vector<char> closed((size_t)total, 0);
    for (int64_t r = 0; r < (int64_t)p.lorder.size(); ++r) {
      const int i = p.lorder[r];
      CHECK(i >= 0 && i < n && !in[(size_t)i]);
      if (!(i >= 0 && i < n)) continue;
      in[(size_t)i] = 1;
      if (r > 0 && p.cell[p.lorder[r - 1]] != p.cell[i]) closed[(size_t)p.cell[p.lorder[r - 1]]] = 1;
      CHECK(!closed[(size_t)p.cell[i]]);
    }
  }
  // close pairs lie in the same or adjacent cells
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = i + 1; j < n; ++j) {
      bool close = true;
      for (int k = 0; k < d; ++k)
        close = close && std::fabs(pts[i * d + k] - pts[j * d + k]) < xcut * std::fabs(scale[k]);
      if (!close) continue;
      int64_t qi[3] = {0, 0, 0}, qj[3] = {0, 0, 0};
      cell_coords(p, d, p.cell[i], qi);
      cell_coords(p, d, p.cell[j], qj);
      for (int k = 0; k < d; ++k) CHECK(std::llabs(qi[k] - qj[k]) <= 1);
    }
  return doublings;
}

int main() {
  const double span[3] = {1.7, 0.9, 1.3}, scale[3] = {0.05, -0.08, 0.11};
  int cases = 0;
  for (int d = 1; d <= 3; ++d)
    for (int64_t n : {1, 2, 97, 700})
      for (bool reorder : {true, false}) {
        const std::vector<double> pts = scatter(n, d, span);
        CHECK(check_plan("scattered", pts, n, d, scale, 1.3, reorder) >= 0);
        ++cases;
      }
  {
    // widths far below the spacing: 40 x 40 x 40 cells for 50 points, coarsened to <= 1024
    const double fine[3] = {0.02, 0.02, 0.02};
    const std::vector<double> pts = scatter(50, 3, span);
    CHECK(check_plan("coarsened", pts, 50, 3, fine, 1.0, true) >= 1);
    ++cases;
  }
  {
    ctx = "fallback";
    CellPlan p;
    std::vector<double> pts = scatter(100, 2, span);
    const double zero[2] = {0.05, 0.0};
    CHECK(!cell_plan(pts.data(), 100, 2, zero, 1.3, true, &p));        // a width of 0
    CHECK(!cell_plan(pts.data(), 100, 2, scale, std::nan(""), true, &p));
    // cells that 64 doublings do not bring under the cap (the range overflows to inf)
    std::vector<double> far = {0.0, std::numeric_limits<double>::max(),
                               -std::numeric_limits<double>::max()};
    const double one[1] = {1.0};
    CHECK(!cell_plan(far.data(), 3, 1, one, 1e-300, true, &p));
    pts[57] = std::numeric_limits<double>::infinity();
    CHECK(!cell_plan(pts.data(), 100, 2, scale, 1.3, true, &p));       // a non-finite point
    pts[57] = std::nan("");
    CHECK(!cell_plan(pts.data(), 100, 2, scale, 1.3, true, &p));
    cases += 5;
  }
  if (failures) {
    std::fprintf(stderr, "cell_plan_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("cell_plan_check: %d cases OK\n", cases);
  return 0;
}
