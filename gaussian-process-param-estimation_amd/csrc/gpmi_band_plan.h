// Shapes and sizes of the band path's host side (gpmi_band_*.hip): the cyclic
// reduction's level list and per-eta strides, what every buffer of a capacity group
// holds per eta, the create-time sizes, and the eta chunking. Plain arithmetic, no HIP
// here, so that it is checked on the host (tests/host/band_plan_check.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)   // (inline helpers: no exported symbols)

namespace gpmi {

constexpr int BAND_TS = 128;    // = GPMI_TS: the band's block size
constexpr int BAND_RLD = 16;    // = GPMI_RHS_LD: columns of the resident RHS block
constexpr int BAND_OUT_LD = 1 + BAND_RLD * BAND_RLD;   // per eta: logdet, then the Gram block
constexpr int BAND_TAN_MAX = 64;   // = GPMI_BAND_TAN_MAX (include/gpmi.h): etas per tangent chunk
constexpr int BAND_IO_MIN = 64;    // the io group's smallest capacity

// Blocks per cyclic-reduction level, from the band's nt down; a level of m blocks
// eliminates its m / 2 odd ones and hands (m + 1) / 2 on. The last level's single
// block (the root) is implied.
inline std::vector<int> bcr_levels(int nt) {
  std::vector<int> ms;
  for (int m = nt; m > 1; m = (m + 1) / 2) ms.push_back(m);
  return ms;
}

// What the evaluator's buffers hold per eta, in doubles: the strides its kernels are
// given, and the sizes its capacity groups allocate (BandEval, gpmi_band_host.h).
struct BandPlan {
  int nt, half;          // blocks of the band; of a reduced level, at most
  int64_t sL, sW, sZ;    // by original block: [nt][128][128], [nt][2][128][128], [nt][128][16]
  int64_t sH, sHY;       // by a level's even block: [half][128][128], [half][128][16]
  int64_t sG, sT;        // [nt][16][16] Gram partials; [nt] per-block traces + their sum

  explicit BandPlan(int nt_) : nt(nt_), half((nt_ + 1) / 2) {
    const int64_t blk = (int64_t)BAND_TS * BAND_TS, yb = (int64_t)BAND_TS * BAND_RLD;
    sL = nt * blk, sW = 2 * sL, sZ = nt * yb;
    sH = half * blk, sHY = half * yb;
    sG = (int64_t)nt * BAND_RLD * BAND_RLD, sT = nt + 1;
  }

  // cyclic reduction: D, F, Y of two levels in turn, every level's Linv, W, Z, the
  // derivative solves' X, Z', the Gram partials G, G2, G3 and the log-determinants
  // (and nt ints: the failed pivots)
  int64_t bcr_doubles() const { return 2 * (2 * sH + sHY) + sL + sW + 3 * sZ + 3 * sG + nt; }
  // selected inversion: Zd, Zo, X, Tr
  int64_t sinv_doubles() const { return sL + 2 * sW + sT; }
  // eta-tangents: dL, dW, dX, dZd, dZo, dD and dF of two levels in turn, Tr
  int64_t tan_doubles() const { return 2 * sL + 3 * sW + 4 * sH + sT; }
  // the sequential kernel's derivative terms: the factor, the solution, G2 and G3
  int64_t der_doubles() const { return sW + sZ + 2 * BAND_RLD * BAND_RLD; }
  // io: eta, the output record (and one int: info)
  static constexpr int64_t io_doubles() { return 1 + BAND_OUT_LD; }
  static int io_capacity(int neta) { return std::max(neta, BAND_IO_MIN); }
};

constexpr int SY_CH = 16;          // tile columns per symm split-K chunk (at most)
// symm split-K chunk for an mt-tile trailing block on `slots` resident workgroups (two
// per CU): the mt x ceil(mt / chunk) workgroups run in ceil(W / slots) rounds of chunk
// 128^3 products each, so the chunk minimising rounds x chunk (+ the partial sums'
// reads, ~1/620 of a product each) ends the grid in full rounds: at mt = 117, chunk 9
// (1521 workgroups, 2.97 rounds of 512) instead of mt^2 / 1024 = 13 (1053, 2.06 rounds
// run as 3: the third nearly empty, 1.06 ms against ~0.73).
inline int symm_chunk(int mt, int slots) {
  int best = 1;
  long long bc = -1;
  for (int ch = 1; ch <= SY_CH; ++ch) {
    const long long w = (long long)mt * ((mt + ch - 1) / ch);
    const long long c = (w + slots - 1) / slots * ch * 620 + w;
    if (bc < 0 || c <= bc) {
      bc = c;
      best = ch;
    }
  }
  return best;
}

// Tiles of the symm split-K partials Xp: the largest mt x chunks over the panels.
inline int64_t xp_tiles(int nt, int ncu) {
  int64_t tiles = 1;
  for (int mt = 1; mt < nt; ++mt) {
    const int ch = symm_chunk(mt, 2 * ncu);
    tiles = std::max<int64_t>(tiles, (int64_t)mt * ((mt + ch - 1) / ch));
  }
  return tiles;
}

constexpr int RGROUP = 8;   // tile rows per group of the look-ahead SYR2K's tile order
// The grouped tile orders of the look-ahead SYR2K, one per (w x w)-triangle, w < nt,
// from off[w]: row groups of RGROUP tile rows, column-major inside a group, a tile
// packed as (i << 16) | j (measured within +-0.5 % of the plain triangle order).
inline std::vector<uint32_t> syr2k_tile_order(int nt, std::vector<int64_t>* off) {
  std::vector<uint32_t> h;
  off->assign(std::max(nt, 0), 0);
  for (int w = 1; w < nt; ++w) {
    (*off)[w] = (int64_t)h.size();
    for (int r0 = 0; r0 < w; r0 += RGROUP) {
      const int r1 = std::min(w, r0 + RGROUP);
      for (int j = 0; j < r1; ++j)
        for (int i = std::max(r0, j); i < r1; ++i) h.push_back(((uint32_t)i << 16) | (uint32_t)j);
    }
  }
  return h;
}

constexpr int CHASE_MSG = 136;   // = CMSG (gpmi_chase.hip): values per hand-off slot
// Positions of the systolic chase, and its message slots (8-byte granules): per slot
// CHASE_MSG values as two tagged granules each; four message kinds (the
// one-per-position kernel uses two) of chase_msg_slots each.
inline int chase_positions(int64_t n) { return (int)((n - 1 + BAND_TS - 1) / BAND_TS); }
inline int64_t chase_msg_slots(int64_t n) {
  return (int64_t)(chase_positions(n) + 1) * 2 * 2 * CHASE_MSG;
}
// cmsg in granules: the four kinds' slots, then the error flag (64 bytes) and the
// profile records of a GPMI_CHASE_PROF build (8192 bytes)
inline int64_t chase_msg_granules(int64_t n) { return 4 * chase_msg_slots(n) + 8 + 1024; }
// td: [n_pad] diagonal, squared subdiagonal and eigenvalues each, then the launch
// form's reflector slots (two wavefront parities x ((n_pad - 2) / 128 + 3) slots of 130)
inline int64_t td_doubles(int64_t n_pad) {
  return 3 * n_pad + 2 * ((n_pad - 2) / BAND_TS + 3) * (BAND_TS + 2);
}

// [begin, begin + count) ranges of at most `chunk` etas covering [0, neta), in order.
struct EtaChunk {
  int begin, count;
};
inline std::vector<EtaChunk> eta_chunks(int neta, int chunk) {
  std::vector<EtaChunk> c;
  for (int b = 0; b < neta; b += chunk) c.push_back({b, std::min(chunk, neta - b)});
  return c;
}

}  // namespace gpmi

#pragma GCC visibility pop
