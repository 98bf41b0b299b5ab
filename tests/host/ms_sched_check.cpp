// The multi-shift CG's host scheduler (csrc/gpmi_ms_sched.h) against a CPU model of
// the device: columns whose residuals decay at given rates. Every scenario runs with
// the compaction off and on; the invariants of a run are checked as it goes, and the
// outcome (iterations launched, segments, forced reads) against the recorded table
// (the scheduler before it was split from the HIP code, on the same model).
// Exit status 0: all held. Build: c++ -std=c++17 -I <csrc> ms_sched_check.cpp
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "gpmi_ms_sched.h"

using gpmi::MS_BATCH;
using gpmi::MsPin;
using gpmi::MsRun;

static int failures = 0;
static std::string context;

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      ++failures;                                                                        \
      std::fprintf(stderr, "%s: line %d: %s\n", context.c_str(), __LINE__, #cond);       \
    }                                                                                    \
  } while (0)

typedef std::vector<std::pair<int, int>> Segments;

struct Scenario {
  const char* name;
  double rtol;
  int maxiter;
  std::vector<double> bn2, rho;   // per original column
  int k0;                         // the decay slows after iteration k0 (< 0: never)
  double slow;
  int off_launched;               // expected, compaction off
  int on_launched;                // expected, compaction on
  Segments on_segments;
  int on_forced;
};

static double rate(double rtol, double K) { return std::pow(rtol * rtol, 1.0 / K); }

struct Model {
  const Scenario& sc;
  int maxiter;
  MsPin slots[2];
  std::vector<int> cols;   // the current block's original columns, in order
  bool marked[2] = {false, false};
  int launched = 0;
  int compactions = 0;

  explicit Model(const Scenario& s) : sc(s), maxiter(s.maxiter), slots() {
    const int n = (int)sc.bn2.size();
    for (int c = 0; c < n; ++c) cols.push_back(c);
    for (MsPin& p : slots)   // (ms_init_kernel)
      for (int c = 0; c < n; ++c) p.bn2[c] = sc.bn2[c];
  }

  double rr(int c, int k) const {
    const double e = sc.k0 < 0 || k <= sc.k0 ? (double)k : sc.k0 + sc.slow * (k - sc.k0);
    return sc.bn2[c] * std::pow(sc.rho[c], e) * (1.0 + 0.3 * std::sin(0.7 * k + c));
  }
  // the first iteration column c does not take (its residual met the tolerance before)
  int stop(int c) const {
    if (!(sc.bn2[c] > 0.0)) return 0;
    int k = 0;
    while (k <= maxiter && rr(c, k) > sc.rtol * sc.rtol * sc.bn2[c]) ++k;
    return k;
  }
  bool active(int c, int k) const { return k < stop(c); }

  MsPin* pin() { return slots; }
  int iterate(int k, int slot) {
    CHECK(k == launched);
    CHECK(k < maxiter);
    ++launched;
    if (slot >= 0) {
      CHECK(slot < 2);
      marked[slot] = false;
      for (size_t q = 0; q < cols.size(); ++q) {
        slots[slot].act[q] = active(cols[q], k + 1) ? 1 : 0;
        slots[slot].rr[q] = rr(cols[q], k + 1);
      }
      slots[slot].flag = 0;
    }
    return 0;
  }
  int mark(int slot) {
    marked[slot] = true;
    return 0;
  }
  int wait(int slot) {
    CHECK(marked[slot]);
    return 0;
  }
  int compact(const int* map, int a, const int* drop, const int* drop_orig, int nd, int it) {
    const int s = (int)cols.size();
    CHECK(it == launched);
    CHECK(a >= 1 && a <= std::max(1, s / 2));
    CHECK(nd >= 1);
    CHECK(a + nd == s);
    std::vector<int> kept(s, 0), ncols;
    for (int q = 0; q < a; ++q) {
      CHECK(map[q] >= 0 && map[q] < s && (q == 0 || map[q] > map[q - 1]));
      kept[map[q]] = 1;
      ncols.push_back(cols[map[q]]);
    }
    for (int d = 0; d < nd; ++d) {
      CHECK(drop[d] >= 0 && drop[d] < s && !kept[drop[d]]);
      CHECK(!active(cols[drop[d]], it));       // only stopped columns leave
      CHECK(drop_orig[d] == cols[drop[d]]);
    }
    for (int q = 0; q < s; ++q)
      if (active(cols[q], it)) CHECK(kept[q]);   // every active column stays
    cols.swap(ncols);
    ++compactions;
    return 0;
  }
};

static void run(const Scenario& sc, bool compact_on) {
  context = std::string(sc.name) + (compact_on ? " (compaction on)" : " (compaction off)");
  Model m(sc);
  const int s = (int)sc.bn2.size();
  MsRun out;
  const int rc = gpmi::ms_schedule(m, s, sc.rtol, sc.maxiter, compact_on, false, &out);
  CHECK(rc == 0 && !out.indefinite);
  CHECK(out.launched == m.launched);
  CHECK(out.compactions == m.compactions);
  CHECK(compact_on || out.compactions == 0);
  int last_stop = 0;
  for (int c = 0; c < s; ++c) last_stop = std::max(last_stop, m.stop(c));
  CHECK(out.launched <= sc.maxiter);
  if (last_stop > sc.maxiter) {   // a column still active at maxiter
    CHECK(out.launched == sc.maxiter);
  } else {
    // (a stop at the start of a batch still runs that batch and the one queued behind it)
    CHECK(out.launched >= last_stop);
    CHECK(out.launched <= last_stop + 2 * MS_BATCH - 1);
  }
  CHECK((int)out.segments.size() == out.compactions + 1);
  int sum = 0;
  for (size_t q = 0; q < out.segments.size(); ++q) {
    sum += out.segments[q].second;
    if (q == 0) CHECK(out.segments[q].first == s);
    else CHECK(2 * out.segments[q].first <= out.segments[q - 1].first);
  }
  CHECK(sum == out.launched);
  CHECK(out.orig == m.cols);
  // the recorded outcome
  std::printf("%-10s compaction %s: launched %d, forced reads %d, segments", sc.name,
              compact_on ? "on " : "off", out.launched, out.forced_reads);
  for (const auto& g : out.segments) std::printf(" (%d,%d)", g.first, g.second);
  std::printf("\n");
  if (compact_on) {
    CHECK(out.launched == sc.on_launched);
    CHECK(out.segments == sc.on_segments);
    CHECK(out.forced_reads == sc.on_forced);
  } else {
    CHECK(out.launched == sc.off_launched);
    CHECK(out.segments == Segments({{s, sc.off_launched}}));
  }
}

int main() {
  std::vector<Scenario> all;
  {
    Scenario c{"cfg5like", 1e-6, 1000, std::vector<double>(12, 3.0),
               std::vector<double>(12, rate(1e-6, 42)), -1, 1.0,
               91, 92, {{12, 42}, {5, 16}, {1, 34}}, 0};
    c.rho[10] = rate(1e-6, 90);
    c.bn2[11] = 0.0;   // the padding column
    all.push_back(c);
  }
  {
    Scenario c{"waves", 1e-12, 1000, std::vector<double>(8, 2.0), {}, -1, 1.0,
               36, 36, {{8, 16}, {4, 16}, {2, 3}, {1, 1}}, 0};
    for (double K : {2, 2, 2, 2, 21, 21, 35, 35}) c.rho.push_back(rate(1e-12, K));
    all.push_back(c);
  }
  for (int maxiter : {17, 24}) {
    Scenario c{maxiter == 17 ? "maxiter17" : "maxiter24", 1e-13, maxiter,
               std::vector<double>(6, 2.0), {}, -1, 1.0, maxiter, maxiter,
               {{6, 16}, {2, maxiter - 16}}, 0};
    for (double K : {3, 3, 3, 3, 60, 60}) c.rho.push_back(rate(1e-13, K));
    all.push_back(c);
  }
  all.push_back(Scenario{"one", 1e-6, 1000, {1.0}, {rate(1e-6, 30)}, -1, 1.0,
                         31, 31, {{1, 31}}, 0});
  all.push_back(Scenario{"stagnate", 1e-6, 50, std::vector<double>(7, 1.0),
                         std::vector<double>(7, 0.999999), -1, 1.0, 50, 50, {{7, 50}}, 0});
  {
    Scenario c{"ladder16", 1e-8, 1000, std::vector<double>(16, 1.0), {}, -1, 1.0,
               96, 96, {{16, 48}, {8, 23}, {4, 16}, {2, 9}}, 0};
    for (int q = 0; q < 16; ++q) c.rho.push_back(rate(1e-8, 5 + 6 * q));
    all.push_back(c);
  }
  {
    // the decay slows tenfold after iteration 12: a compaction prediction misses
    Scenario c{"plateau", 1e-8, 1000, std::vector<double>(8, 1.0), {}, 12, 0.1,
               170, 167, {{8, 137}, {4, 16}, {2, 14}}, 1};
    for (int q = 0; q < 8; ++q) c.rho.push_back(rate(1e-8, 20 + q));
    all.push_back(c);
  }
  for (const Scenario& sc : all)
    for (bool on : {false, true}) run(sc, on);
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  return failures ? 1 : 0;
}
