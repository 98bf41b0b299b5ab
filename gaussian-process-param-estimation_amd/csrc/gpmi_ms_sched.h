// Host scheduling of the multi-shift CG (gpmi_sp_msgram): batch sizes, when to wait
// for a pinned slot, the per-column stop prediction, and when and what to compact.
// Plain arithmetic on the two pinned MsPin slots: no HIP here, so that the loop runs
// against a CPU model of the device (tests/host/ms_sched_check.cpp). The device side
// (the launches, the event pair, the buffers) is the Dev the loop is given:
//   int iterate(int k, int slot)  queue iteration k's launches; slot >= 0: its update
//                                 kernel writes the end state into that pinned slot
//   int mark(int slot)            record the slot's event behind what is queued
//   int wait(int slot)            wait for that event (the slot is then readable)
//   MsPin* pin()                  the two slots (host pointer)
//   int compact(const int* map, int a, const int* drop, const int* drop_orig, int nd,
//               int it)           gather the kept columns map[0, a) into a block of
//                                 width a (the state before iteration `it`), keep the
//                                 nd dropped columns' Grams, and iterate there from now
// Each returns 0, or an error code that ends the run.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

namespace gpmi {

constexpr int MS_MAXS = 16;   // RHS columns per multi-shift block
constexpr int MS_BATCH = 8;   // multi-shift CG iterations between host polls

// A multi-shift CG batch's end state, written by the batch's last
// ms_cg2_update_kernel (block 0) straight into host-mapped pinned memory: the host
// reads it after an event behind that kernel (no copy launches; round 4 copied the
// three fields with three hipMemcpyAsync blits, ~75 us per batch with their gaps).
struct MsPin {
  int act[MS_MAXS];
  int flag;
  int pad;
  double rr[MS_MAXS];
  double bn2[MS_MAXS];   // ||b_c||^2, written by ms_init_kernel into both slots
};

struct MsRun {
  int launched = 0;        // iterations queued
  int compactions = 0;
  int forced_reads = 0;    // compaction reads that found too few columns stopped
  bool indefinite = false; // a slot carried the negative-curvature flag (run ended)
  // the launch segments: (block width, iterations launched at that width), in order
  std::vector<std::pair<int, int>> segments;
  std::vector<int> orig;   // each final column's index in the original block
};

// Iterations run in batches between host reads of the stop flags. Each batch's last
// update kernel writes its end state (active flags, the negative-curvature flag,
// gamma) into host-mapped pinned memory, read while the NEXT batch is already
// queued, so the device does not wait for the host between batches. The next
// batch's size comes from the residuals' decay: the iterations the slowest active
// column still needs at its rate since the previous read, beyond what is queued (at
// most MS_BATCH); when the queued iterations should suffice the host waits for them
// instead. Iterations past a column's stop leave it unchanged (zero steps).
//
// Active-column compaction (round 6). The block iterates until its slowest column
// converges, and a stopped column still costs its share of every SpMM and vector
// pass (zero steps). BASELINE cfg 5: the ten basis columns of [X z] stop at ~42
// iterations, the data column z runs to ~90. Once at most half of the columns are
// still active, their state is gathered into a block of their width (Dev::compact)
// and the loop goes on there. Every column's arithmetic is unchanged (the SpMM, the
// dots and the updates are per column): the Grams are bit-identical to the
// uncompacted block (test_msgram_compaction_*).
template <class Dev>
struct MsSched {
  Dev& dev;
  int s;   // the block's current width (compaction narrows it)
  const double rtol;
  const int maxiter;
  const bool compact_on, trace;
  MsPin* const pin;
  int it = 0;   // iterations queued
  int slot_it[2] = {0, 0};
  std::vector<double> rr_seen;
  int it_seen = 0;
  bool prev = false;   // the other slot holds a batch not yet read
  std::vector<int> orig;   // each current column's index in the original block
  int compactions = 0;
  int seg_start = 0;   // the iteration the current block width began at
  std::vector<std::pair<int, int>> segments;
  // Predictions from each read (round 6): need_after, the iterations the slowest active
  // column still needs beyond those queued (it; unknown at first: a batch at a time), and
  // compact_at, the iteration by which at most half of the block's columns should still
  // iterate (each column's stop from its own rate; -1: none predicted). A batch sized to
  // end where the prediction says the CG stops, or where the block can be compacted, is
  // read as soon as it ends instead of after the next batch is queued: before, the
  // iterations queued past the stop ran at full cost (cfg 4: 111 launched for 102) and
  // the compaction waited a batch at the full width.
  int need_after;
  int compact_at = -1;
  int forced_reads = 0;   // compaction reads that found too few columns stopped
  bool indefinite = false;
  std::vector<double> stops;

  MsSched(Dev& d, int s_, double rtol_, int maxiter_, bool compact_on_, bool trace_)
      : dev(d), s(s_), rtol(rtol_), maxiter(maxiter_), compact_on(compact_on_), trace(trace_),
        pin(d.pin()), rr_seen(s_, -1.0), orig(s_), need_after(maxiter_) {
    for (int c = 0; c < s; ++c) orig[c] = c;
  }

  // narrow the block once at most half of its columns still iterate (one column left
  // always qualifies; waiting for three quarters measured the same at cfg 4 and 5)
  int keep_target() const { return std::max(1, s / 2); }

  bool compactable(int q) const {
    int nact = 0;
    for (int c = 0; c < s; ++c) nact += pin[q].act[c] ? 1 : 0;
    return nact <= keep_target();
  }

  // 0: columns still active; 2: all stopped; else an error
  int read_slot(int qs) {
    if (int rc = dev.wait(qs)) return rc;
    if (pin[qs].flag) {
      indefinite = true;
      return 1;
    }
    bool any = false;
    double needm = 0.0;
    const int at = slot_it[qs];
    int nact = 0;
    stops.clear();
    for (int c = 0; c < s; ++c) {
      if (!pin[qs].act[c]) continue;
      any = true;
      ++nact;
      // (at the first read the rate is from r_0 = b: ||r_0||^2 = ||b||^2, so the first
      // batches need no wait for a second read)
      const double r1 = pin[qs].rr[c], target = rtol * rtol * pin[qs].bn2[c];
      const double r0 = rr_seen[c] < 0.0 && it_seen == 0 ? pin[qs].bn2[c] : rr_seen[c];
      double m = (double)MS_BATCH;
      bool rated = false;
      if (r0 > 0.0 && r1 > 0.0 && r1 < r0 && at > it_seen && target > 0.0) {
        m = std::log(target / r1) / (std::log(r1 / r0) / (double)(at - it_seen));
        rated = true;
      }
      needm = std::max(needm, m);
      stops.push_back(rated ? (double)at + std::max(0.0, m) : 1e300);
      rr_seen[c] = r1;
    }
    it_seen = at;
    // clamped before the conversion: a stagnating residual (r1 / r0 -> 1) gives a huge m
    const double rem = std::min((double)maxiter, std::ceil((double)at + needm)) - (double)it;
    need_after = (int)std::max(-1.0, rem);
    compact_at = -1;
    const int k = nact - keep_target();   // columns that must stop before the block narrows
    if (compact_on && s > 1 && any && k >= 1 && forced_reads < 2) {
      std::nth_element(stops.begin(), stops.begin() + (k - 1), stops.end());
      const double tk = stops[k - 1];
      if (tk < (double)maxiter) compact_at = (int)std::ceil(tk);
    }
    if (trace)
      std::fprintf(stderr,
                   "[ms] read slot at %d (queued %d, width %d, active %d): need %.1f more, "
                   "after %d, compact at %d%s\n",
                   at, it, s, nact, needm, need_after, compact_at, any ? "" : " (all stopped)");
    return any ? 0 : 2;
  }

  // The compaction, asynchronous (round 6): the kept columns are those active in the
  // pinned slot rd the host has just read (a column that stopped since idles in the new
  // block until the next compaction or the end). The slot rd was written by the last
  // batch or the one before it; the device's gathers are queued behind every iteration,
  // so they see the state at iteration `it` whichever it was.
  int compact(int rd) {
    int map[MS_MAXS], drop[MS_MAXS], drop_orig[MS_MAXS];
    int a = 0, nd = 0;
    for (int c = 0; c < s; ++c) {
      if (pin[rd].act[c]) map[a++] = c;
      else drop[nd++] = c;
    }
    if (a == 0 || a > keep_target() || nd == 0) return 0;
    for (int d = 0; d < nd; ++d) drop_orig[d] = orig[drop[d]];
    if (int rc = dev.compact(map, a, drop, drop_orig, nd, it)) return rc;
    // host-side state in the new column order (pin's bn2 is written once, at the start;
    // a batch still in flight writes its old-order end state into the slot after rd's,
    // which is rewritten by the next batch before it is read)
    std::vector<int> norig(a);
    std::vector<double> nrr(a);
    for (int q = 0; q < a; ++q) {
      norig[q] = orig[map[q]];
      nrr[q] = rr_seen[map[q]];
    }
    for (int qs = 0; qs < 2; ++qs) {
      double bn[MS_MAXS];
      for (int q = 0; q < a; ++q) bn[q] = pin[qs].bn2[map[q]];
      for (int q = 0; q < a; ++q) pin[qs].bn2[q] = bn[q];
    }
    orig.swap(norig);
    rr_seen.swap(nrr);
    segments.emplace_back(s, it - seg_start);
    seg_start = it;
    s = a;
    prev = false;
    ++compactions;
    return 0;
  }

  int run() {
    int nb = MS_BATCH;
    int kb = 0;
    int rc = 0;
    while (it < maxiter) {
      nb = std::max(1, std::min(nb, maxiter - it));
      const int qs = kb & 1;
      for (int i = 0; i < nb; ++i, ++it)
        if ((rc = dev.iterate(it, i + 1 == nb ? qs : -1))) return rc;
      if ((rc = dev.mark(qs))) return rc;
      slot_it[qs] = it;
      ++kb;
      need_after -= nb;
      int read = -1;   // the slot read this round (its flags drive the compaction)
      if (prev) {
        const int r = read_slot(qs ^ 1);
        if (r == 2) break;
        if (r) return r;
        read = qs ^ 1;
      }
      prev = true;
      const bool can_compact = compact_on && s > 1 && it < maxiter;
      // the stop, or the compaction, predicted within the iterations queued: read them now
      const bool due = can_compact && compact_at >= 0 && compact_at <= it &&
                       !(read >= 0 && compactable(read));
      if (need_after <= 0 || due) {
        const int r = read_slot(qs);
        if (r == 2) break;
        if (r) return r;
        prev = false;
        read = qs;
        if (due && !compactable(qs)) ++forced_reads;
      }
      if (can_compact && read >= 0 && compactable(read)) {
        if ((rc = compact(read))) return rc;
        compact_at = -1;   // (a prediction for the old block)
      }
      nb = std::max(1, std::min(MS_BATCH, need_after));
      // end the batch where the block is predicted to narrow
      if (compact_on && s > 1 && compact_at > it && compact_at < it + nb) nb = compact_at - it;
    }
    if (trace) std::fprintf(stderr, "[ms] loop end: launched %d\n", it);
    return 0;
  }
};

// The multi-shift CG's iterations on dev, from a block of width s, until every column
// has stopped or maxiter iterations are queued. *out: what ran (also on an error).
template <class Dev>
int ms_schedule(Dev& dev, int s, double rtol, int maxiter, bool compact_on, bool trace,
                MsRun* out) {
  MsSched<Dev> sch(dev, s, rtol, maxiter, compact_on, trace);
  const int rc = sch.run();
  out->launched = sch.it;
  out->compactions = sch.compactions;
  out->forced_reads = sch.forced_reads;
  out->indefinite = sch.indefinite;
  sch.segments.emplace_back(sch.s, sch.it - sch.seg_start);
  out->segments = std::move(sch.segments);
  out->orig = std::move(sch.orig);
  return rc;
}

}  // namespace gpmi
