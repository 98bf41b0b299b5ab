// The dense Cholesky's launch list (csrc/gpmi_dense_plan.h) replayed symbolically: per
// tile, which operand element columns it has received so far. Checked for both panel
// schedules, for nt in {1, 2, 3, 8, 9, 17, 128} x outer in {1, 4, 16, 32}:
//   * every lower tile (I, k) receives [0, 128 k) exactly once, ascending and contiguous,
//     from operand tiles that are final, before its panel step (TRSM);
//   * every diagonal tile is complete before its diag-block launch;
//   * the recursive and the left-looking schedule cover identical ranges, and the
//     left-looking one launches no band SYRK (w < rows) at all.
// Exit status 0: all held. Build: c++ -std=c++17 -I <csrc> dense_plan_check.cpp
#include <cstdio>
#include <utility>
#include <vector>

#include "gpmi_dense_plan.h"

using namespace gpmi;

static int failures = 0;
static int ctx_nt = 0, ctx_outer = 0, ctx_mode = 0;

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      if (++failures <= 20)                                                              \
        std::fprintf(stderr, "nt = %d outer = %d mode = %d: line %d: %s\n", ctx_nt,      \
                     ctx_outer, ctx_mode, __LINE__, #cond);                              \
    }                                                                                    \
  } while (0)

struct Tile {
  int done = 0;          // operand element columns [0, done) applied
  bool final_ = false;   // lower tile: panel step done; diagonal tile: factored
  std::vector<std::pair<int, int>> chunks;   // (p0, kdim) in the order applied
};

struct Replay {
  int nt;
  std::vector<Tile> tiles;
  explicit Replay(int nt_) : nt(nt_), tiles((size_t)nt_ * nt_) {}
  Tile& at(int i, int j) { return tiles[(size_t)i * nt + j]; }

  // tile (i, j) -= A_i,[p0, p0 + kdim) A_j,[p0, p0 + kdim)^T
  void update(int i, int j, int p0, int kdim) {
    Tile& t = at(i, j);
    CHECK(!t.final_);
    CHECK(t.done == p0);   // ascending, contiguous, nothing twice
    CHECK(kdim > 0 && p0 % DENSE_TS == 0 && kdim % DENSE_TS == 0);
    CHECK(p0 + kdim <= j * DENSE_TS);
    for (int q = p0 / DENSE_TS; q < (p0 + kdim) / DENSE_TS; ++q) {
      CHECK(at(i, q).final_);   // the operand tiles are finished L tiles
      CHECK(at(j, q).final_);
    }
    t.done = p0 + kdim;
    t.chunks.push_back({p0, kdim});
  }
  void trsm(int i, int k) {
    Tile& t = at(i, k);
    CHECK(!t.final_);
    CHECK(t.done == k * DENSE_TS);
    CHECK(at(k, k).final_);
    t.final_ = true;
  }
  void diag(int k) {
    Tile& t = at(k, k);
    CHECK(!t.final_);
    CHECK(t.done == k * DENSE_TS);
    t.final_ = true;
  }
};

static Replay replay(int nt, int outer, int mode) {
  ctx_nt = nt, ctx_outer = outer, ctx_mode = mode;
  Replay R(nt);
  int n_diag = 0, n_bulk = 0;
  bool seen_from_k = false;
  for (const DenseLaunch& L : dense_plan(nt, outer, mode)) {
    CHECK(L.r0 >= 0 && L.r0 < L.r1 && L.r1 <= nt && L.col >= 0 && L.col + L.w <= nt);
    switch (L.kind) {
      case DENSE_DIAG:
        CHECK(L.r0 == L.col && L.r1 == L.col + 1);
        R.diag(L.col);
        ++n_diag;
        break;
      case DENSE_PANEL:
        CHECK(mode == DENSE_REC);
        CHECK(L.r0 == L.col + 1 && L.r1 == nt);
        for (int i = L.r0; i < L.r1; ++i) R.trsm(i, L.col);
        break;
      case DENSE_COLPANEL: {
        CHECK(mode == DENSE_COL);
        CHECK(L.r0 == L.col + 1 && L.r1 == nt);
        const int c0 = L.p0 / DENSE_TS;
        CHECK(c0 % outer == 0 && c0 <= L.col && L.col < c0 + outer);
        CHECK(L.kdim == (L.col - c0) * DENSE_TS);
        CHECK(L.next_diag == (L.col + 1 < c0 + outer && L.col + 1 < nt));
        for (int i = L.r0; i < L.r1; ++i) {
          if (L.kdim > 0) R.update(i, L.col, L.p0, L.kdim);
          R.trsm(i, L.col);
        }
        if (L.next_diag) R.update(L.col + 1, L.col + 1, L.p0, L.kdim + DENSE_TS);
        break;
      }
      case DENSE_SYRK: {
        CHECK(L.r0 == L.col && L.r1 == nt);
        // (a band SYRK of the recursion applies at most half a panel)
        const bool bulk = L.kdim == outer * DENSE_TS;
        if (mode == DENSE_COL) CHECK(bulk);
        if (bulk) {
          ++n_bulk;
          CHECK(L.w == L.r1 - L.r0 && L.p0 + L.kdim == L.col * DENSE_TS);
        } else {
          CHECK(L.w < outer && L.p0 + L.kdim == L.col * DENSE_TS);
        }
        CHECK(L.from_k == (bulk && L.p0 == 0));
        if (L.from_k) {
          CHECK(!seen_from_k);
          seen_from_k = true;
        }
        for (int j = L.col; j < L.col + L.w; ++j)
          for (int i = j; i < nt; ++i) R.update(i, j, L.p0, L.kdim);
        break;
      }
      default:
        CHECK(false);
    }
  }
  CHECK(n_diag == nt);
  CHECK(n_bulk == (nt - 1) / outer);
  for (int i = 0; i < nt; ++i)
    for (int j = 0; j <= i; ++j) {
      CHECK(R.at(i, j).final_);
      CHECK(R.at(i, j).done == j * DENSE_TS);
    }
  return R;
}

int main() {
  const int nts[] = {1, 2, 3, 8, 9, 17, 128};
  const int outers[] = {1, 4, 16, 32};
  for (int nt : nts)
    for (int outer : outers) {
      Replay rec = replay(nt, outer, DENSE_REC);
      Replay col = replay(nt, outer, DENSE_COL);
      ctx_mode = -1;
      for (int i = 0; i < nt; ++i)
        for (int j = 0; j <= i; ++j) {
          // the same range, cut at multiples of 128 either way; the left-looking chunks
          // are unions of the recursive ones inside a panel, identical outside it
          const auto& a = rec.at(i, j).chunks;
          const auto& b = col.at(i, j).chunks;
          CHECK(rec.at(i, j).done == col.at(i, j).done);
          size_t ia = 0;
          for (const auto& cb : b) {
            int p = cb.first;
            while (ia < a.size() && p < cb.first + cb.second) {
              CHECK(a[ia].first == p);
              p += a[ia].second;
              ++ia;
            }
            CHECK(p == cb.first + cb.second);
          }
          CHECK(ia == a.size());
        }
    }
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("dense plan: ok\n");
  return 0;
}
