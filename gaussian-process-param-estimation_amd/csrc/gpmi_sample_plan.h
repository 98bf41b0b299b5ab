// Chunking, work list and workspace sizes of the draws z = L xi from the cached factor
// (gpmi_dense_sample.hip: gpmi_op_sample; kernels in gpmi_sample.hip). Plain arithmetic, no
// HIP here, so that the list is replayed on the host (tests/host/sample_plan_check.cpp).
//
// The normals and the draws are held sample-major, Xi_t / Y_t [draws][n_pad]: one draw is
// one contiguous row, and both MFMA operands of Y_t = Xi_t L^T are [row][k] slabs. Output
// tile (draw tile J, row tile I) is the triangular sum over k <= I of Xi_t_Jk L_Ik^T, of
// depth I + 1 tile products. The depth is cut into pieces of at most D tile rows: piece p
// of row tile I covers the tile columns [p D, min((p + 1) D, I + 1)), so a row tile has
// I / D + 1 pieces and the last one holds the diagonal tile. D >= nt leaves every row
// tile whole (no partials, no second kernel). One workgroup per (piece, draw tile); the
// pieces are listed deepest first (sample_order), the draw tiles of a piece side by side.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define GPMI_SPLAN_HD __host__ __device__
#else
#define GPMI_SPLAN_HD
#endif

#pragma GCC visibility push(hidden)   // (inline helpers: no exported symbols)

namespace gpmi {

constexpr int SAMPLE_TS = 128;              // = GPMI_TS
constexpr int SAMPLE_CHUNK = 1024;          // draws per chunk
constexpr int SAMPLE_MAX_NT = 1 << 15;      // a row tile and a piece share one 32-bit word
constexpr int64_t SAMPLE_PART_TILES = 8192; // cap on the partial tiles of a chunk (1 GiB)

// Chunk width in draws: `override_draws` (GPMI_SAMPLE_CHUNK; 0: none) or SAMPLE_CHUNK.
// < 0: the override is not a positive multiple of 128.
inline int sample_chunk_draws(int64_t override_draws) {
  if (override_draws == 0) return SAMPLE_CHUNK;
  if (override_draws < 0 || override_draws % SAMPLE_TS || override_draws > (1 << 20)) return -1;
  return (int)override_draws;
}

// Pieces of row tile I at piece depth D.
GPMI_SPLAN_HD inline int sample_pieces(int I, int D) { return I / D + 1; }

// Pieces of the row tiles before I: sum over i < I of (i / D + 1). The partial tile of
// (row tile I, piece p, draw tile J of jt) is number (sample_piece_base(I, D) + p) jt + J.
GPMI_SPLAN_HD inline int64_t sample_piece_base(int I, int D) {
  const int64_t a = I / D, b = I % D;
  return (int64_t)I + (int64_t)D * a * (a - 1) / 2 + a * b;
}

inline int64_t sample_items(int nt, int D) { return sample_piece_base(nt, D); }

// Tile columns [k0, k1) of piece p of row tile I.
GPMI_SPLAN_HD inline void sample_piece_range(int I, int D, int p, int* k0, int* k1) {
  *k0 = p * D;
  *k1 = (p + 1) * D < I + 1 ? (p + 1) * D : I + 1;
}

// The pieces, (I << 16) | p, deepest first (a stable sort of the row tiles descending):
// the long pieces start first and the short ones fill the tail of the grid.
inline std::vector<uint32_t> sample_order(int nt, int D) {
  std::vector<uint32_t> out;
  out.reserve((size_t)sample_items(nt, D));
  for (int I = nt - 1; I >= 0; --I)
    for (int p = 0; p < sample_pieces(I, D); ++p) out.push_back(((uint32_t)I << 16) | (uint32_t)p);
  std::stable_sort(out.begin(), out.end(), [D](uint32_t a, uint32_t b) {
    int a0, a1, b0, b1;
    sample_piece_range((int)(a >> 16), D, (int)(a & 0xffff), &a0, &a1);
    sample_piece_range((int)(b >> 16), D, (int)(b & 0xffff), &b0, &b1);
    return a1 - a0 > b1 - b0;
  });
  return out;
}

// Piece depth D in [1, nt] for nt row tiles and jt draw tiles on `slots` workgroups at a
// time, one per CU: two are resident, but they share the CU's MFMA pipe, and the
// measurements below follow one slot per CU, not two. D == nt: unsplit. `override_depth`
// (GPMI_SAMPLE_DEPTH; <= 0: none) replaces the choice, clipped to [1, nt]. In units of one
// 128^3 product per slot: unsplit, the row tiles run deepest first and the grid ends after
// about max(nt, work / slots), work = jt nt (nt + 1) / 2; split, the w = items jt pieces
// of depth <= D run ceil(w / slots) rounds of D, and each partial tile adds a 128 KB write
// and read, counted as 1 / slots as predict_cov_split does (gpmi_predict_plan.h). Ties go
// to the larger D (fewer partials), and a D whose partials exceed SAMPLE_PART_TILES is
// left out. n* = 4096 (nt = 32) on 256 CUs, product ms measured at D = 1 / 2 / 4 / 8 / 16 /
// 32 (profiles/r12/sample_depth_ab.txt): 1024 draws (jt = 8) 0.517 / 0.416 / 0.388 / 0.430 /
// 0.545 / 0.570, the rule's costs 33.5 / 26.5 / 24.5 / 26.5 / 33.5 / 32, least at D = 5
// (23.7; measured 0.384); 128 draws (jt = 1) 0.124 / 0.101 / 0.092 / 0.145 / 0.266 / 0.506,
// costs 5.1 / 5.1 / 4.6 / 8.3 / 16.2 / 32, least at D = 3 (3.7; measured 0.083).
inline int sample_depth(int nt, int jt, int slots, int64_t override_depth = 0) {
  if (nt < 1) return 1;
  if (override_depth > 0) return (int)std::min<int64_t>(override_depth, nt);
  slots = std::max(slots, 1);
  jt = std::max(jt, 1);
  const double work = (double)jt * nt * (nt + 1) / 2.0 / slots;
  int best = nt;
  double bc = std::max((double)nt, work);
  for (int D = nt - 1; D >= 1; --D) {
    const int64_t w = sample_items(nt, D) * jt;
    if (w > SAMPLE_PART_TILES) break;   // (w grows as D falls)
    const double c = (double)((w + slots - 1) / slots) * D + (double)w / slots;
    if (c < bc) {
      bc = c;
      best = D;
    }
  }
  return best;
}

// Workspace in doubles of one chunk of jt draw tiles: Xi_t and Y_t [128 jt][n_pad] each,
// part [items jt][128][128] when the depth is split (D < nt), else nothing.
struct SampleSizes {
  size_t xi, y, part;
};

inline SampleSizes sample_sizes(int64_t n_pad, int nt, int jt, int D) {
  const size_t blk = (size_t)jt * SAMPLE_TS * (size_t)n_pad;
  const size_t part = D < nt ? (size_t)sample_items(nt, D) * jt * SAMPLE_TS * SAMPLE_TS : 0;
  return {blk, blk, part};
}

}  // namespace gpmi

#pragma GCC visibility pop
