// The prediction's launch list, chunking and workspace sizes (csrc/gpmi_predict_plan.h)
// replayed symbolically, the way gpmi_op_predict_terms walks them. For
// nt in {1, 2, 3, 17} x outer in {1, 2, 4, 16} x chunk widths of one and several column
// tiles x test-point counts around the tile and chunk edges:
//   * every T tile (tile row i, column tile j) receives the operand tile rows [0, i)
//     exactly once, ascending and contiguous, from V tiles that are final, before its
//     diagonal step; every tile gets exactly one diagonal step, which writes its
//     partials row part[i][column][0..16];
//   * the workgroup -> tile map of each trailing product is a bijection of its tiles;
//   * the chunks cover [0, nstar) exactly, in order, each within the chunk width;
//   * every index the kernels form into T, part and out lies inside predict_sizes();
//   * the chunk width of the default budget and of the override, and the panel width.
// Exit status 0: all held. Build: c++ -std=c++17 -I <csrc> predict_plan_check.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpmi_predict_plan.h"

using namespace gpmi;

static int failures = 0;
static int ctx_nt = 0, ctx_outer = 0, ctx_ns = 0;
static long long ctx_nstar = 0;

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      if (++failures <= 20)                                                              \
        std::fprintf(stderr, "nt = %d outer = %d NS = %d nstar = %lld: line %d: %s\n",   \
                     ctx_nt, ctx_outer, ctx_ns, ctx_nstar, __LINE__, #cond);             \
    }                                                                                    \
  } while (0)

struct Tile {
  int done = 0;          // operand tile rows [0, done) applied
  bool final_ = false;   // the diagonal step has run: the tile holds V
};

// One chunk of nct column tiles through the launch list, with the buffers' capacities.
static void replay_chunk(int nt, int outer, int nct, int64_t n_pad, const PredictSizes& cap) {
  std::vector<Tile> tiles((size_t)nt * nct);
  std::vector<int> part_written((size_t)nt * nct, 0);
  auto at = [&](int i, int j) -> Tile& { return tiles[(size_t)i * nct + j]; };
  const int64_t rows = (int64_t)nct * PRED_TS;   // rows of T the chunk runs (= part's ns_ld)
  CHECK((size_t)(rows * n_pad) <= cap.T);
  CHECK((size_t)(rows * PRED_LD) <= cap.out);
  auto update = [&](int i, int j, int kb, int ke) {
    Tile& t = at(i, j);
    CHECK(!t.final_);
    CHECK(kb < ke && ke <= i);
    CHECK(t.done == kb);   // ascending, contiguous, nothing twice
    for (int k = kb; k < ke; ++k) CHECK(at(k, j).final_);   // operands are finished V tiles
    t.done = ke;
    // the last element of the C tile and of the V operand slab, in T
    const int64_t last_row = (int64_t)j * PRED_TS + PRED_TS - 1;
    CHECK((size_t)(last_row * n_pad + (int64_t)i * PRED_TS + PRED_TS - 1) < cap.T);
    CHECK((size_t)(last_row * n_pad + (int64_t)ke * PRED_TS - 1) < cap.T);
    CHECK((int64_t)i * PRED_TS + PRED_TS <= n_pad);   // L's rows
  };
  int last_diag = -1;
  for (const PredictLaunch& L : predict_plan(nt, outer)) {
    CHECK(L.kb <= L.ke && L.ke - L.kb <= outer);
    if (L.kind == PRED_DIAG) {
      const int k = L.r0;
      CHECK(L.r1 == k + 1 && L.ke == k && k == last_diag + 1);
      last_diag = k;
      for (int j = 0; j < nct; ++j) {
        if (k > L.kb) update(k, j, L.kb, k);
        Tile& t = at(k, j);
        CHECK(!t.final_);
        CHECK(t.done == k);   // everything above it applied
        t.final_ = true;
        // partials: part[(k * rows + col) * 17 + 0..16] for the tile's 128 columns
        const int64_t last = ((int64_t)k * rows + (int64_t)j * PRED_TS + PRED_TS - 1) * PRED_LD +
                             PRED_LD - 1;
        CHECK((size_t)last < cap.part);
        ++part_written[(size_t)k * nct + j];
      }
    } else {
      CHECK(L.kind == PRED_TRAIL);
      CHECK(L.r0 == L.ke && L.r1 == nt && L.r0 < L.r1);
      CHECK(last_diag == L.ke - 1);
      const int ni = L.r1 - L.r0;
      std::vector<int> seen((size_t)ni * nct, 0);
      for (int q = 0; q < ni * nct; ++q) {
        int i = -1, j = -1;
        predict_tile(q, ni, nct, &i, &j);
        CHECK(i >= 0 && i < ni && j >= 0 && j < nct);
        if (i < 0 || i >= ni || j < 0 || j >= nct) continue;
        ++seen[(size_t)i * nct + j];
        update(L.r0 + i, j, L.kb, L.ke);
      }
      for (int v : seen) CHECK(v == 1);
    }
  }
  CHECK(last_diag == nt - 1);
  for (int i = 0; i < nt; ++i)
    for (int j = 0; j < nct; ++j) {
      CHECK(at(i, j).final_ && at(i, j).done == i);
      CHECK(part_written[(size_t)i * nct + j] == 1);
    }
}

static void check_case(int nt, int outer, int NS, int64_t nstar) {
  ctx_nt = nt, ctx_outer = outer, ctx_ns = NS, ctx_nstar = nstar;
  const int64_t n_pad = (int64_t)nt * PRED_TS;
  // the workspace a call allocates: its widest chunk, rounded up to a tile
  int64_t wide = (nstar + PRED_TS - 1) / PRED_TS * PRED_TS;
  if (wide > NS) wide = NS;
  const PredictSizes cap = predict_sizes(n_pad, nt, (int)wide);
  int64_t next = 0;
  int seen_nct = -1;
  for (const PredictChunk& ch : predict_chunks(nstar, NS)) {
    CHECK(ch.j0 == next);                       // in order, no gap, no overlap
    CHECK(ch.cols >= 1 && ch.cols <= NS);
    CHECK(ch.nct == (ch.cols + PRED_TS - 1) / PRED_TS);
    CHECK((int64_t)ch.nct * PRED_TS <= wide);
    CHECK((size_t)ch.cols * PRED_LD <= cap.out);   // the host copy of the chunk's results
    next = ch.j0 + ch.cols;
    if (ch.nct != seen_nct) {                   // (equal chunks replay identically)
      replay_chunk(nt, outer, ch.nct, n_pad, cap);
      seen_nct = ch.nct;
    }
  }
  CHECK(next == nstar);
}

int main() {
  const int nts[] = {1, 2, 3, 17};
  const int outers[] = {1, 2, 4, 16};
  const int widths[] = {128, 384, 1152};   // 1, 3 and 9 column tiles (one whole group + 1)
  int cases = 0;
  for (int nt : nts)
    for (int outer : outers)
      for (int NS : widths) {
        const int64_t counts[] = {1, 127, 128, 129, NS - 1, NS, NS + 1, 2 * NS + 130, 3 * NS};
        for (int64_t nstar : counts) {
          if (nstar < 1) continue;
          check_case(nt, outer, NS, nstar);
          ++cases;
        }
      }
  // chunk width: the budget's default, clamped, and the override
  ctx_nt = ctx_outer = ctx_ns = 0, ctx_nstar = 0;
  CHECK(predict_chunk_cols(16384, 0) == 4096);
  CHECK(predict_chunk_cols(128, 0) == PRED_MAX_CHUNK);
  CHECK(predict_chunk_cols(65536, 0) == 1024);
  CHECK(predict_chunk_cols((int64_t)1 << 22, 0) == PRED_TS);
  for (int64_t np : {128, 384, 16384, 65536, 1 << 20}) {
    const int c = predict_chunk_cols(np, 0);
    CHECK(c >= PRED_TS && c <= PRED_MAX_CHUNK && c % PRED_TS == 0);
    CHECK(c == PRED_TS || (int64_t)c * np * 8 <= PRED_T_BYTES);
  }
  CHECK(predict_outer(16) == PRED_OUTER && predict_outer(32) == PRED_OUTER);
  CHECK(predict_outer(1) == 1 && predict_outer(2) == 2 && predict_outer(PRED_OUTER) == PRED_OUTER);
  CHECK(predict_chunk_cols(16384, 128) == 128);
  CHECK(predict_chunk_cols(16384, 256) == 256);
  CHECK(predict_chunk_cols(16384, 100) < 0);
  CHECK(predict_chunk_cols(16384, -128) < 0);
  if (failures) {
    std::fprintf(stderr, "predict_plan_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("predict_plan_check: %d cases OK\n", cases);
  return 0;
}
