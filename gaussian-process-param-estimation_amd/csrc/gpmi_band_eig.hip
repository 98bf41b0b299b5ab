// Eigenvalues of the band path: the band's bulge chase to tridiagonal form (systolic
// in one launch, or wavefront launches) and bisection (kernels: gpmi_chase.hip).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpmi_band_host.h"

using namespace gpmi;

namespace {

// The systolic chase (one launch): d, e2 of the tridiagonal. Returns 0 when done,
// 1 when the positions cannot all be co-resident, 2 after a timed-out hand-off.
int chase_systolic_run(gpmi_band* b, hipStream_t s, double* d, double* e2, bool split) {
  const int n = (int)b->n;
  const int K = chase_positions(n);
  if (split ? 2 * K > b->eig.split_maxg : K > b->eig.chase_maxg) return 1;
  const size_t slots = (size_t)chase_msg_slots(n), all = (size_t)chase_msg_granules(n);
  HIP_TRY(b->eig.cmsg.reserve(all));
  int* err = reinterpret_cast<int*>(b->eig.cmsg + 4 * slots);
  HIP_TRY(hipMemsetAsync(b->eig.cmsg, 0, sizeof(unsigned long long) * all, s));
  if (split) {
    hipLaunchKernelGGL(chase_split_kernel, dim3(2 * K), dim3(CHASE_SPLIT_THREADS), 0, s, b->Ab,
                       (int64_t)b->n_pad, n, b->eig.cmsg, K, err, b->eig.chase_spin, d, e2);
    LAUNCH_CHECK("chase_split_kernel");
  } else {
    hipLaunchKernelGGL(chase_systolic_kernel, dim3(K), dim3(CHASE_THREADS), 0, s, b->Ab,
                       (int64_t)b->n_pad, n, b->eig.cmsg, b->eig.cmsg + slots, err,
                       b->eig.chase_spin, d, e2);
    LAUNCH_CHECK("chase_systolic_kernel");
  }
  int herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
#ifdef GPMI_CHASE_PROF
  {
    std::vector<long long> st(4 * 16 * 8);
    HIP_TRY(hipMemcpy(st.data(), err + 16, sizeof(long long) * st.size(), hipMemcpyDeviceToHost));
    for (int q = 0; q < 4; ++q)
      for (int i = 0; i < 16; ++i) {
        const long long* t = st.data() + (q * 16 + i) * 8;
        const long long* tn = (i + 1 < 16) ? t + 8 : nullptr;
        fprintf(stderr, "[chase prof] k=%d s=%d dt(10ns): recvR %lld prod %lld post %lld upd %lld "
                "F %lld recvC %lld shift %lld\n", q + 1, 1000 + i, t[1] - t[0], t[2] - t[1],
                t[3] - t[2], t[4] - t[3], t[5] - t[4], t[6] - t[5], tn ? tn[0] - t[6] : 0LL);
      }
  }
#endif
  return herr ? 2 : 0;
}

}  // namespace

extern "C" {

int gpmi_band_eigenvalues(gpmi_band* b, double* lam) {
  if (!b) return set_error(-1006, "null handle");
  DeviceGuard g(b->device);
  hipStream_t s = b->stream;
  const int64_t np = b->n_pad;
  const int n = (int)b->n;
  HIP_TRY(b->eig.td.reserve(td_doubles(np)));
  b->eig.td_valid = false;
  double* d = b->eig.td;
  double* e2 = b->eig.td + np;
  double* dl = b->eig.td + 2 * np;
  HIP_TRY(hipEventRecord(b->ev0, s));
  // GPMI_CHASE_MODE: unset = the systolic chase with a D and an E workgroup per
  // position if its 2K workgroups fit, else one workgroup per position (K), else the
  // launch form; "systolic" = one workgroup per position; "split" (reflector +
  // per-block launches per wavefront t = 3 s + k) / "task" (one workgroup per task per
  // wavefront) = the launch forms
  const char* mode_env = std::getenv("GPMI_CHASE_MODE");
  const int chase_mode = !mode_env ? 0 : std::strcmp(mode_env, "split") == 0 ? 1
                                     : std::strcmp(mode_env, "task") == 0    ? 2
                                     : std::strcmp(mode_env, "systolic") == 0 ? 3 : 0;
  bool done = false;
  b->eig.chase_systolic = 0;
  if ((chase_mode == 0 || chase_mode == 3) && n > 2) {
    int rc = 1;
    if (chase_mode == 0) {
      rc = chase_systolic_run(b, s, d, e2, true);
      if (rc < 0) return rc;
      if (rc == 2) ++b->eig.chase_fallbacks;
      if (rc == 0) b->eig.chase_systolic = 2;
    }
    if (rc != 0) {
      rc = chase_systolic_run(b, s, d, e2, false);
      if (rc < 0) return rc;
      if (rc == 2) ++b->eig.chase_fallbacks;
      if (rc == 0) b->eig.chase_systolic = 1;
    }
    done = rc == 0;
  }
  if (!done) {
  HIP_TRY(b->eig.Ac.reserve(np * np));
  hipLaunchKernelGGL(chase_copy_kernel, dim3(n), dim3(256), 0, s, b->Ab, b->eig.Ac, np, n);
  LAUNCH_CHECK("chase_copy_kernel");
  const bool chase_split = chase_mode != 2;
  const int kmax = (n - 2) / TS + 1;
  const int tmax = 3 * std::max(0, n - 3) + kmax;
  for (int t = 0; t <= tmax && n > 2; ++t) {
    const int s_hi = std::min(t / 3, n - 3);
    const int s_lo = std::max(0, (t - kmax + 2) / 3);
    if (s_hi < s_lo) continue;
    if (chase_split) {
      // reflector slots by sweep (s % ns), double-buffered by wavefront parity: the
      // E workgroup of (s, k) writes the reflector of (s, k + 1) for wavefront t + 1;
      // a sweep's first task (t = 3 s) gets its own small launch
      const int ns = kmax + 2;
      double* scr = b->eig.td + 3 * np;
      double* rd = scr + (int64_t)(t & 1) * ns * (TS + 2);
      double* wr = scr + (int64_t)((t + 1) & 1) * ns * (TS + 2);
      if (t % 3 == 0 && t / 3 >= s_lo && t / 3 <= s_hi) {
        const int s0 = t / 3;
        hipLaunchKernelGGL(chase_reflect_kernel, dim3(1), dim3(TS), 0, s, b->eig.Ac, np, n, s0,
                           rd + (int64_t)(s0 % ns) * (TS + 2));
        LAUNCH_CHECK("chase_reflect_kernel");
      }
      hipLaunchKernelGGL(chase_apply_kernel, dim3(3 * (s_hi - s_lo + 1)), dim3(512), 0, s, b->eig.Ac,
                         np, n, t, s_hi, rd, wr, ns);
      LAUNCH_CHECK("chase_apply_kernel");
    } else {
      hipLaunchKernelGGL(chase_task_kernel, dim3(s_hi - s_lo + 1), dim3(512), 0, s, b->eig.Ac, np, n,
                         t, s_hi);
      LAUNCH_CHECK("chase_task_kernel");
    }
  }
  hipLaunchKernelGGL(tridiag_extract_kernel, dim3((n + 255) / 256), dim3(256), 0, s, b->eig.Ac, np, n,
                     d, e2);
  LAUNCH_CHECK("tridiag_extract_kernel");
  }
  std::vector<double> hd(n), he2(n);
  HIP_TRY(hipMemcpyAsync(hd.data(), d, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(he2.data(), e2, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // Gershgorin interval and the dstebz pivot floor
  double lo = hd[0], hi = hd[0], emax = 0.0;
  for (int i = 0; i < n; ++i) {
    const double el = i > 0 ? std::sqrt(he2[i - 1]) : 0.0;
    const double er = i + 1 < n ? std::sqrt(he2[i]) : 0.0;
    lo = std::min(lo, hd[i] - el - er);
    hi = std::max(hi, hd[i] + el + er);
    emax = std::max(emax, he2[i]);
  }
  const double span = std::max(hi - lo, std::fabs(hi)) * 1e-15 + 1e-300;
  lo -= span;
  hi += span;
  const double pivmin = 2.2250738585072014e-308 * std::max(1.0, emax);
  // GPMI_BISECT=1: one thread per eigenvalue (plain bisection) instead of multisection
  const char* bis = std::getenv("GPMI_BISECT");
  if (bis && std::atoi(bis) == 1) {
    hipLaunchKernelGGL(bisect_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d, e2, n, lo, hi,
                       pivmin, dl);
    LAUNCH_CHECK("bisect_kernel");
  } else {
    const int64_t lanes = (int64_t)n * BISECT_LANES;
    hipLaunchKernelGGL(bisect_multi_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s,
                       d, e2, n, lo, hi, pivmin, dl);
    LAUNCH_CHECK("bisect_multi_kernel");
  }
  HIP_TRY(hipMemcpyAsync(lam, dl, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipEventRecord(b->ev1, s));
  HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  b->eig.eig_ms = ms;
  b->eig.td_valid = true;
  return 0;
}

}  // extern "C"
