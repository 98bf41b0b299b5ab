// csrc/gpmi_sample_plan.h replayed the way gpmi_op_sample and its kernels walk it. Over
// nt = 1..40, every piece depth D = 1..nt and jt = 1, 3, 8 draw tiles:
//   * sample_piece_base is the running sum of sample_pieces, sample_items its total;
//   * the pieces of a row tile cover the tile columns [0, I] once, ascending, none empty
//     and none deeper than D, and exactly the last one holds the diagonal tile;
//   * sample_order lists every (row tile, piece) once, no piece deeper than the one before;
//   * distinct (row tile, piece, draw tile) get distinct partial tiles inside the size
//     sample_sizes reserves, and an unsplit list (D = nt) reserves none;
//   * sample_depth lies in [1, nt], honours and clips its override, never exceeds the
//     cap on partial tiles, and is what the header quotes at the benchmark shapes;
//   * sample_chunk_draws accepts multiples of 128 only.
// Exit status 0: all held. Build: c++ -std=c++17 -I <csrc> sample_plan_check.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpmi_sample_plan.h"

using namespace gpmi;

static int failures = 0;
static int ctx_nt = 0, ctx_d = 0, ctx_jt = 0;

#define CHECK(cond)                                                                           \
  do {                                                                                        \
    if (!(cond)) {                                                                            \
      if (++failures <= 20)                                                                   \
        std::fprintf(stderr, "nt = %d D = %d jt = %d: line %d: %s\n", ctx_nt, ctx_d, ctx_jt,  \
                     __LINE__, #cond);                                                        \
    }                                                                                         \
  } while (0)

static void check_pieces(int nt, int D) {
  int64_t run = 0;
  for (int I = 0; I < nt; ++I) {
    CHECK(sample_piece_base(I, D) == run);
    const int np = sample_pieces(I, D);
    CHECK(np >= 1);
    int next = 0;
    for (int p = 0; p < np; ++p) {
      int k0, k1;
      sample_piece_range(I, D, p, &k0, &k1);
      CHECK(k0 == next);                    // ascending, no gap, no overlap
      CHECK(k1 > k0 && k1 - k0 <= D);       // never empty, never deeper than D
      CHECK((k1 == I + 1) == (p == np - 1));   // the diagonal tile is in the last piece only
      next = k1;
    }
    CHECK(next == I + 1);
    run += np;
  }
  CHECK(sample_items(nt, D) == run);
  if (D >= nt) CHECK(run == nt);            // unsplit: one piece per row tile
}

static void check_order(int nt, int D) {
  const std::vector<uint32_t> ord = sample_order(nt, D);
  CHECK((int64_t)ord.size() == sample_items(nt, D));
  std::vector<char> seen((size_t)sample_items(nt, D), 0);
  int prev = 1 << 30;
  for (uint32_t w : ord) {
    const int I = (int)(w >> 16), p = (int)(w & 0xffff);
    CHECK(I >= 0 && I < nt && p >= 0 && p < sample_pieces(I, D));
    if (!(I >= 0 && I < nt && p >= 0 && p < sample_pieces(I, D))) continue;
    const int64_t slot = sample_piece_base(I, D) + p;
    CHECK(!seen[(size_t)slot]);
    seen[(size_t)slot] = 1;
    int k0, k1;
    sample_piece_range(I, D, p, &k0, &k1);
    CHECK(k1 - k0 <= prev);                 // deepest first
    prev = k1 - k0;
  }
  if (!ord.empty()) CHECK((int)(ord[0] >> 16) == nt - 1);   // the heaviest row tile leads
}

static void check_sizes(int nt, int D, int jt) {
  const int64_t n_pad = (int64_t)nt * SAMPLE_TS;
  const SampleSizes sz = sample_sizes(n_pad, nt, jt, D);
  CHECK(sz.xi == (size_t)jt * SAMPLE_TS * (size_t)n_pad && sz.y == sz.xi);
  if (D >= nt) {
    CHECK(sz.part == 0);
    return;
  }
  const int64_t tile = (int64_t)SAMPLE_TS * SAMPLE_TS;
  std::vector<char> seen((size_t)(sample_items(nt, D) * jt), 0);
  for (int I = 0; I < nt; ++I)
    for (int p = 0; p < sample_pieces(I, D); ++p)
      for (int J = 0; J < jt; ++J) {
        const int64_t slot = (sample_piece_base(I, D) + p) * jt + J;
        CHECK(slot >= 0 && (size_t)((slot + 1) * tile) <= sz.part);
        if (slot >= 0 && slot < (int64_t)seen.size()) {
          CHECK(!seen[(size_t)slot]);
          seen[(size_t)slot] = 1;
        }
      }
}

int main() {
  int cases = 0;
  for (int nt = 1; nt <= 40; ++nt) {
    for (int D = 1; D <= nt; ++D) {
      ctx_nt = nt, ctx_d = D, ctx_jt = 0;
      check_pieces(nt, D);
      check_order(nt, D);
      for (int jt : {1, 3, 8}) {
        ctx_jt = jt;
        check_sizes(nt, D, jt);
        CHECK(sample_depth(nt, jt, 256, D) == D);   // the override
        ++cases;
      }
    }
    ctx_d = 0;
    for (int jt : {1, 3, 8})
      for (int slots : {1, 64, 256}) {
        ctx_jt = jt;
        const int D = sample_depth(nt, jt, slots);
        CHECK(D >= 1 && D <= nt);
        CHECK(D == nt || sample_items(nt, D) * jt <= SAMPLE_PART_TILES);
        CHECK(sample_depth(nt, jt, slots, 0) == D && sample_depth(nt, jt, slots, -3) == D);
        CHECK(sample_depth(nt, jt, slots, 99) == std::min(99, nt));
        CHECK(sample_depth(nt, jt, slots, (int64_t)1 << 40) == nt);
      }
    // one slot: nothing to balance, so no split
    CHECK(sample_depth(nt, 1, 1) == nt);
  }
  ctx_nt = ctx_d = ctx_jt = 0;
  // the benchmark shapes on 256 CUs (header), and a tall operator under the cap
  CHECK(sample_depth(32, 1, 256) == 3);
  CHECK(sample_depth(32, 8, 256) == 5);
  CHECK(sample_depth(2, 1, 256) == 1);
  CHECK(sample_depth(1, 8, 256) == 1);
  for (int nt : {128, 512, 4096}) {
    const int D = sample_depth(nt, 8, 256);
    CHECK(D >= 1 && D <= nt);
    CHECK(D == nt || sample_items(nt, D) * 8 <= SAMPLE_PART_TILES);
  }
  CHECK(sample_chunk_draws(0) == SAMPLE_CHUNK && SAMPLE_CHUNK % SAMPLE_TS == 0);
  CHECK(sample_chunk_draws(128) == 128 && sample_chunk_draws(2048) == 2048);
  CHECK(sample_chunk_draws(-1) < 0 && sample_chunk_draws(100) < 0 && sample_chunk_draws(129) < 0);
  CHECK(sample_chunk_draws((int64_t)1 << 30) < 0);
  if (failures) {
    std::fprintf(stderr, "sample_plan_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("sample_plan_check: %d cases OK\n", cases);
  return 0;
}
