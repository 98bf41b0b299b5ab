// The band path's shapes and sizes (csrc/gpmi_band_plan.h) against what the host code
// computed before they were gathered there: the cyclic reduction's level walk, every
// capacity group's allocation per eta (the literal hipMalloc arguments), the look-ahead
// SYR2K's tile orders, the split-K partials' tile count and the eta chunking.
// Exit status 0: all held. Build: c++ -std=c++17 -I <csrc> band_plan_check.cpp
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "gpmi_band_plan.h"

using namespace gpmi;

static int failures = 0;
static int ctx_nt = 0;

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      ++failures;                                                                      \
      std::fprintf(stderr, "nt = %d: line %d: %s\n", ctx_nt, __LINE__, #cond);         \
    }                                                                                  \
  } while (0)

static void check_levels(int nt) {
  const std::vector<int> ms = bcr_levels(nt);
  // the walk of the level loop as it stood in the cyclic reduction
  std::vector<int> walk;
  int m = nt, lvl = 0, odd = 0;
  while (m > 1) {
    const int nodd = m / 2, neven = (m + 1) / 2;
    walk.push_back(m);
    odd += nodd;
    m = neven;
    ++lvl;
  }
  CHECK(ms == walk);
  CHECK((int)ms.size() == lvl);
  for (size_t l = 1; l < ms.size(); ++l) CHECK(ms[l] < ms[l - 1]);
  CHECK(odd + 1 == nt);   // every block is eliminated once; the root is left
  int log2 = 0;
  while ((1 << log2) < nt) ++log2;
  CHECK((int)ms.size() == log2);
  if (nt == 1) CHECK(ms.empty());
}

static void check_sizes(int nt) {
  const BandPlan p(nt);
  const int64_t TS = 128, RLD = 16, OUT_LD = 1 + 16 * 16;
  const int64_t half = (nt + 1) / 2, blk = TS * TS, yb = TS * RLD, np = nt * TS;
  CHECK(p.nt == nt && p.half == half);
  CHECK(p.sL == nt * blk && p.sW == 2 * nt * blk && p.sZ == nt * yb);
  CHECK(p.sH == half * blk && p.sHY == half * yb);
  // cyclic reduction: bcrD/F/Y[2], L, W, Z, X, Zp, G, G2, G3, Ld (Fail: nt ints)
  CHECK(p.bcr_doubles() == 2 * (half * blk + half * blk + half * yb) + nt * blk + nt * 2 * blk +
                               3 * (nt * yb) + 3 * (nt * RLD * RLD) + nt);
  // selected inversion: sinvZd, Zo, X, Tr
  CHECK(p.sinv_doubles() == nt * blk + nt * 2 * blk + nt * 2 * blk + (nt + 1));
  // tangents: tanL, W, X, Zd, Zo, tanD/F[2], tanTr
  CHECK(p.tan_doubles() == nt * blk + nt * 2 * blk + nt * 2 * blk + nt * blk + nt * 2 * blk +
                               2 * (half * blk + half * blk) + (nt + 1));
  // derivative terms: fac, ysol, der
  CHECK(p.der_doubles() == nt * 2 * TS * TS + np * RLD + 2 * RLD * RLD);
  // io: etas, out (info: one int), capacity max(neta, 64)
  CHECK(BandPlan::io_doubles() == 1 + OUT_LD);
  CHECK(BAND_OUT_LD == OUT_LD);
  for (int neta : {1, 63, 64, 65, 300}) CHECK(BandPlan::io_capacity(neta) == std::max(neta, 64));
  if (nt == 128) {
    CHECK(p.tan_doubles() == (8 * 128 + 4 * 64) * 128 * 128 + 129);
    CHECK(p.tan_doubles() == 20971649);
    CHECK(p.tan_doubles() * 8 == 167773192);   // the "about 168 MB" per eta at N = 16384
  }
  // the eigenvalue path's fixed sizes, for n = n_pad and a ragged n
  for (int64_t n : {np, np - 37}) {
    if (n < 1) continue;
    const int64_t K = (n - 1 + TS - 1) / TS;
    CHECK(chase_positions(n) == K);
    CHECK(chase_msg_slots(n) == (K + 1) * 2 * 2 * 136);
    CHECK(chase_msg_granules(n) * 8 == 8 * 4 * chase_msg_slots(n) + 64 + 8192);
  }
  CHECK(td_doubles(np) == 3 * np + 2 * ((np - 2) / TS + 3) * (TS + 2));
}

static void check_tile_order(int nt) {
  std::vector<int64_t> off;
  const std::vector<uint32_t> h = syr2k_tile_order(nt, &off);
  CHECK((int)off.size() == nt);
  int64_t at = 0;
  for (int w = 1; w < nt; ++w) {
    CHECK(off[w] == at);
    const int64_t cnt = (int64_t)w * (w + 1) / 2;
    CHECK(at + cnt <= (int64_t)h.size());
    if (at + cnt > (int64_t)h.size()) return;
    std::set<std::pair<int, int>> seen;
    for (int64_t k = at; k < at + cnt; ++k) {
      const int i = (int)(h[k] >> 16), j = (int)(h[k] & 0xffff);
      CHECK(j <= i && i < w);
      seen.insert({i, j});
    }
    CHECK((int64_t)seen.size() == cnt);   // each tile exactly once
    at += cnt;
  }
  CHECK(at == (int64_t)h.size());
}

static void check_xp_tiles(int nt) {
  for (int ncu : {64, 256, 304}) {
    int64_t tiles = 1;   // the loop as it stood in gpmi_band_create
    for (int mt = 1; mt < nt; ++mt) {
      const int ch = symm_chunk(mt, 2 * ncu);
      tiles = std::max<int64_t>(tiles, (int64_t)mt * ((mt + ch - 1) / ch));
    }
    CHECK(xp_tiles(nt, ncu) == tiles);
  }
}

static void check_chunks() {
  for (int neta : {1, 64, 65, 128, 130, 256}) {
    ctx_nt = -neta;   // (reported as a negative "nt")
    const std::vector<EtaChunk> c = eta_chunks(neta, 64);
    int at = 0;
    for (const EtaChunk& k : c) {
      CHECK(k.begin == at);
      CHECK(k.count > 0 && k.count <= 64);
      at += k.count;
    }
    CHECK(at == neta);
    CHECK((int)c.size() == (neta + 63) / 64);
  }
  const std::vector<EtaChunk> c = eta_chunks(130, 64);
  CHECK(c.size() == 3 && c[0].count == 64 && c[1].count == 64 && c[2].count == 2);
  CHECK(eta_chunks(200, 200).size() == 1);   // unchunked calls: one range
  CHECK(BAND_TAN_MAX == 64);
}

int main() {
  for (int nt : {1, 2, 3, 4, 5, 8, 9, 17, 18, 128, 256}) {
    ctx_nt = nt;
    check_levels(nt);
    check_sizes(nt);
    check_tile_order(nt);
    check_xp_tiles(nt);
  }
  ctx_nt = 0;
  CHECK(symm_chunk(117, 512) == 9);
  check_chunks();
  if (failures) {
    std::fprintf(stderr, "band_plan_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("band_plan_check: ok\n");
  return 0;
}
