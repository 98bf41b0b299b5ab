// The covariance additions of csrc/gpmi_predict_plan.h replayed the way
// gpmi_op_predict_cov and its two kernels walk them. Over nt = 1..9, n* = 1..1100 and
// chunk widths 128 / 256 / the default:
//   * the chunk row ranges tile [0, n*_pad) exactly, in order, inside the block size;
//   * the pieces of every split S = 1..nt cover [0, nt) once, ascending, none empty;
//   * predict_cov_split lies in [1, nt], honours the override and clips it to nt;
//   * the partial-buffer size bounds every (tile, piece) index, and distinct
//     (tile, piece) pairs get distinct partial tiles;
//   * the cap rejects a block one tile over it and accepts one at it.
// Exit status 0: all held. Build: c++ -std=c++17 -I <csrc> predict_cov_plan_check.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpmi_predict_plan.h"

using namespace gpmi;

static int failures = 0;
static int ctx_nt = 0, ctx_ns = 0;
static long long ctx_nstar = 0;

#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      if (++failures <= 20)                                                                \
        std::fprintf(stderr, "nt = %d NS = %d nstar = %lld: line %d: %s\n", ctx_nt, ctx_ns, \
                     ctx_nstar, __LINE__, #cond);                                          \
    }                                                                                      \
  } while (0)

static void check_pieces(int nt) {
  for (int S = 1; S <= nt; ++S) {
    CHECK(predict_cov_piece_begin(nt, S, 0) == 0);
    CHECK(predict_cov_piece_begin(nt, S, S) == nt);
    int next = 0, longest = 0;
    for (int p = 0; p < S; ++p) {
      const int k0 = predict_cov_piece_begin(nt, S, p), k1 = predict_cov_piece_begin(nt, S, p + 1);
      CHECK(k0 == next);   // ascending, no gap, no overlap
      CHECK(k1 > k0);      // never empty
      longest = std::max(longest, k1 - k0);
      next = k1;
    }
    CHECK(next == nt);
    CHECK(longest == (nt + S - 1) / S);   // balanced: the depth predict_cov_split counts
  }
}

static void check_case(int nt, int NS, int64_t nstar) {
  ctx_nt = nt, ctx_ns = NS, ctx_nstar = nstar;
  const int64_t n_pad = (int64_t)nt * PRED_TS;
  const int64_t nsp = (nstar + PRED_TS - 1) / PRED_TS * PRED_TS;
  const int nct = (int)(nsp / PRED_TS);
  const int64_t ntiles = predict_cov_tiles(nct);
  CHECK(ntiles == (int64_t)nct * (nct + 1) / 2);
  // chunk row ranges inside the whole block
  {
    const PredictCovSizes cap = predict_cov_sizes(n_pad, nct, 1);
    CHECK(cap.T == (size_t)nsp * (size_t)n_pad && cap.cov == (size_t)nsp * (size_t)nsp);
    int64_t next_row = 0;
    for (const PredictChunk& ch : predict_chunks(nstar, NS)) {
      const int64_t r0 = predict_cov_row0(ch), rows = (int64_t)ch.nct * PRED_TS;
      CHECK(r0 == next_row);            // in order, no gap, no overlap
      CHECK(r0 % PRED_TS == 0);
      CHECK((size_t)((r0 + rows) * n_pad) <= cap.T);   // the last element the solve touches
      next_row = r0 + rows;
    }
    CHECK(next_row == nsp);
  }
  // every split: partial indices, and the choice
  for (int S = 1; S <= nt; ++S) {
    const PredictCovSizes cap = predict_cov_sizes(n_pad, nct, S);
    std::vector<char> seen((size_t)ntiles * S, 0);
    for (int64_t q = 0; q < ntiles; ++q)
      for (int p = 0; p < S; ++p) {
        const int64_t off = predict_cov_part_off(q, S, p);
        CHECK(off >= 0 && off % (PRED_TS * PRED_TS) == 0);
        CHECK((size_t)(off + PRED_TS * PRED_TS) <= cap.part);
        const int64_t slot = off / (PRED_TS * PRED_TS);
        if (slot >= 0 && slot < ntiles * S) {
          CHECK(!seen[(size_t)slot]);
          seen[(size_t)slot] = 1;
        }
      }
    CHECK(predict_cov_fits(n_pad, nct, S));   // (far below the cap at these sizes)
    CHECK(predict_cov_split(ntiles, nt, 512, S) == S);           // the override
  }
  for (int slots : {1, 64, 512}) {
    const int S = predict_cov_split(ntiles, nt, slots);
    CHECK(S >= 1 && S <= nt);
  }
  CHECK(predict_cov_split(ntiles, nt, 512, 99) == std::min(99, nt));   // clipped to nt
  CHECK(predict_cov_split(ntiles, nt, 512, (int64_t)1 << 40) == nt);
  const int free_choice = predict_cov_split(ntiles, nt, 512);
  CHECK(predict_cov_split(ntiles, nt, 512, 0) == free_choice);         // 0 and below: none
  CHECK(predict_cov_split(ntiles, nt, 512, -3) == free_choice);
}

int main() {
  int cases = 0;
  for (int nt = 1; nt <= 9; ++nt) {
    ctx_nt = nt, ctx_ns = 0, ctx_nstar = 0;
    check_pieces(nt);
    const int widths[] = {128, 256, predict_chunk_cols((int64_t)nt * PRED_TS, 0)};
    for (int NS : widths)
      for (int64_t nstar = 1; nstar <= 1100; ++nstar) {
        check_case(nt, NS, nstar);
        ++cases;
      }
  }
  ctx_nt = ctx_ns = 0, ctx_nstar = 0;
  // the choice at the two benchmark shapes (N = 16384 on 256 CUs), and whole rounds
  CHECK(predict_cov_split(predict_cov_tiles(2), 128, 512) == 128);
  CHECK(predict_cov_split(predict_cov_tiles(32), 128, 512) == 8);
  CHECK(predict_cov_split(1, 1, 512) == 1);
  // the cap: for several depths, the widest block that fits and the one a tile wider
  const int64_t cap_tiles = PRED_COV_BYTES / ((int64_t)8 * PRED_TS * PRED_TS);
  for (int nt : {1, 9, 128, 512}) {
    ctx_nt = nt;
    const int64_t n_pad = (int64_t)nt * PRED_TS;
    for (int S : {1, nt}) {
      int nct = 1;
      while (predict_cov_fits(n_pad, nct + 1, S)) ++nct;
      CHECK(predict_cov_fits(n_pad, nct, S));
      CHECK(!predict_cov_fits(n_pad, nct + 1, S));
      const PredictCovSizes at = predict_cov_sizes(n_pad, nct, S);
      const PredictCovSizes over = predict_cov_sizes(n_pad, nct + 1, S);
      CHECK((int64_t)(8 * (at.T + at.cov + at.part)) <= PRED_COV_BYTES);
      CHECK((int64_t)(8 * (over.T + over.cov + over.part)) > PRED_COV_BYTES);
      // a grid of tiles x pieces stays far inside an int
      CHECK(predict_cov_tiles(nct) * S <= cap_tiles);
    }
    CHECK(!predict_cov_fits(n_pad, 1 << 20, 1));
  }
  if (failures) {
    std::fprintf(stderr, "predict_cov_plan_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("predict_cov_plan_check: %d cases OK\n", cases);
  return 0;
}
