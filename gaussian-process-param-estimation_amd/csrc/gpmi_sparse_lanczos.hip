// The sparse operator's Lanczos for stochastic Lanczos quadrature: blocked, with full or
// windowed (CGS2), delayed (DCGS2) or no reorthogonalisation (handle: gpmi_sp.h).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpmi_sp.h"

using namespace gpmi;

namespace gpmi {

int col_dots(gpmi_sp* sp, const double* A, int64_t strideA, int J, const double* B, int s,
             double* out, double* partial, hipStream_t st) {
  if (!partial) {
    HIP_TRY(sp->work.partial.reserve((size_t)NBLK * J * s));
    partial = sp->work.partial;
  }
  if (!st) st = sp->stream;
  hipLaunchKernelGGL(col_dot_partial_kernel, dim3(NBLK, J), dim3(256), 0, st, A, strideA,
                     B, sp->n, s, partial);
  LAUNCH_CHECK("col_dot_partial_kernel");
  hipLaunchKernelGGL(col_dot_reduce_kernel, dim3((J * s + 3) / 4), dim3(256), 0, st,
                     partial, NBLK, J, s, out);
  LAUNCH_CHECK("col_dot_reduce_kernel");
  return 0;
}

}  // namespace gpmi

namespace {

// Lanczos of K on s probe columns starting from V0 (already in V block 0).
// alpha/beta: host [s][steps] (column-major by probe). orth < 0: CGS2 against every
// previous vector (full reorthogonalisation); orth = 0: the plain three-term
// recurrence (one projection on v_k after subtracting beta v_{k-1}: imate's
// orthogonalize=0); orth > 0: CGS2 against the last orth vectors and v_k.
int lanczos_block(gpmi_sp* sp, double* V, double* W, int s, int steps, double* h_alpha,
                  double* h_beta, int orth = -1) {
  const int64_t ns = sp->n * s;
  // device scalars: H1, H2 [(steps+1)][MAXS] (the two CGS2 passes), norms, the
  // alpha/beta tables [s][steps], two axpby coefficient pairs and the dead flags
  const size_t need = (size_t)2 * (steps + 1) * MAXS + MAXS + (size_t)2 * MAXS * steps +
                      4 * MAXS + MAXS;
  HIP_TRY(sp->work.lz.reserve(need));
  double* H1 = sp->work.lz;
  double* H2 = H1 + (size_t)(steps + 1) * MAXS;
  double* nrm = H2 + (size_t)(steps + 1) * MAXS;
  double* dalpha = nrm + MAXS;
  double* dbeta = dalpha + (size_t)MAXS * steps;
  double* ca = dbeta + (size_t)MAXS * steps;
  double* cb = ca + MAXS;
  double* na = cb + MAXS;
  double* nb = na + MAXS;
  int* dead = reinterpret_cast<int*>(nb + MAXS);
  // one pass (orth = 0): the second pass's coefficients stay zero
  if (orth == 0) HIP_TRY(hipMemsetAsync(H2, 0, sizeof(double) * MAXS, sp->stream));
  for (int k = 0; k < steps; ++k) {
    double* Vk = V + (int64_t)k * ns;
    const int jlo = orth < 0 ? 0 : std::max(0, k - orth);   // projection window [jlo, k]
    const int J = k + 1 - jlo;
    if (int rc = spmm(sp, Vk, W, s, 0.0)) return rc;
    if (k > 0) {   // W -= beta_{k-1} V_{k-1}
      hipLaunchKernelGGL(col_axpby_kernel, dim3(grid_ns(sp->n, s)), dim3(256), 0, sp->stream,
                         V + (int64_t)(k - 1) * ns, W, na, nb, sp->n, s);
      LAUNCH_CHECK("col_axpby_kernel");
    }
    for (int pass = 0; pass < (orth == 0 ? 1 : 2); ++pass) {   // CGS(2) against V_jlo .. V_k
      double* H = pass == 0 ? H1 : H2;
      if (int rc = col_dots(sp, V + (int64_t)jlo * ns, ns, J, W, s, H)) return rc;
      hipLaunchKernelGGL(col_gs_update_kernel, dim3((unsigned)((ns + 511) / 512)), dim3(256), 0,
                         sp->stream, W, V + (int64_t)jlo * ns, ns, H, J, sp->n, s);
      LAUNCH_CHECK("col_gs_update_kernel");
    }
    if (int rc = col_dots(sp, W, 0, 1, W, s, nrm)) return rc;
    hipLaunchKernelGGL(lanczos_scalar_kernel, dim3(1), dim3(64), 0, sp->stream,
                       H1 + (size_t)(k - jlo) * s, orth == 0 ? H2 : H2 + (size_t)(k - jlo) * s,
                       nrm, s, k, steps, dead, dalpha, dbeta, ca, cb, na, nb);
    LAUNCH_CHECK("lanczos_scalar_kernel");
    if (k + 1 < steps) {
      // V_{k+1} = W / beta  (b = 0 -> X * 0 + 0 * Y; Y is zero-initialised below)
      double* Vn = V + (int64_t)(k + 1) * ns;
      HIP_TRY(hipMemsetAsync(Vn, 0, sizeof(double) * ns, sp->stream));
      hipLaunchKernelGGL(col_axpby_kernel, dim3(grid_ns(sp->n, s)), dim3(256), 0, sp->stream, W,
                         Vn, ca, cb, sp->n, s);
      LAUNCH_CHECK("col_axpby_kernel");
    }
  }
  HIP_TRY(hipMemcpyAsync(h_alpha, dalpha, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipMemcpyAsync(h_beta, dbeta, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

// Lanczos of K on s probe columns by the plain three-term recurrence (imate's
// orthogonalize = 0; lz0_*_kernel in gpmi_sparse.hip): three launches per step (the
// SpMM with u . Ku in its epilogue, the per-column scalars, one update pass over three
// vectors with the next norm and overlap partials), the vectors unnormalised. U:
// three rotating blocks [n][s] (U[0] = the normalised probes), Y one block.
// alpha / beta: host [s][steps].
int lanczos_block_plain(gpmi_sp* sp, double* U, double* Y, int s, int steps, double* h_alpha,
                        double* h_beta) {
  const int64_t n = sp->n, ns = n * s;
  const int nb = (int)((n + 63) / 64);
  const size_t need = 5 * (size_t)s + 2 * (size_t)s * steps + s;
  HIP_TRY(sp->work.lz.reserve(need));
  double* st = sp->work.lz;
  double* coef = st + 2 * s;
  double* dal = coef + 3 * s;
  double* dbe = dal + (size_t)s * steps;
  int* dead = reinterpret_cast<int*>(dbe + (size_t)s * steps);
  HIP_TRY(sp->work.partial.reserve((size_t)nb * 3 * s));
  double* pq = sp->work.partial;            // [s][nb]: u_k . y
  double* pv = pq + (size_t)nb * s;         // [2][s][nb]: ||u_{k+1}||^2, u_{k+1} . u_k
  HIP_TRY(hipMemsetAsync(dbe, 0, sizeof(double) * s * steps, sp->stream));
  // u_{-1}: zero (its coefficient is 0 at k = 0; 0 * garbage could be NaN)
  HIP_TRY(hipMemsetAsync(U + 2 * ns, 0, sizeof(double) * ns, sp->stream));
  const unsigned sgrid = (unsigned)s;   // lz0_alpha_kernel: one workgroup per column
  for (int k = 0; k < steps; ++k) {
    double* Uc = U + (int64_t)(k % 3) * ns;
    double* Un = U + (int64_t)((k + 1) % 3) * ns;
    double* Up = U + (int64_t)((k + 2) % 3) * ns;
    int pqb = 0;
    if (int rc = spmm(sp, Uc, Y, s, 0.0, sp->stream, pq, &pqb)) return rc;
    if (pqb != nb) {
      hipLaunchKernelGGL(lz0_dot64_kernel, dim3((unsigned)nb), dim3(256), 0, sp->stream, Uc, Y, n,
                         s, pq);
      LAUNCH_CHECK("lz0_dot64_kernel");
    }
    hipLaunchKernelGGL(lz0_alpha_kernel, dim3(sgrid), dim3(256), 0, sp->stream, pq, pv, nb, s, k,
                       steps, st, dead, dal, dbe, coef);
    LAUNCH_CHECK("lz0_alpha_kernel");
    hipLaunchKernelGGL(lz0_update_kernel, dim3((unsigned)nb), dim3(256), 0, sp->stream, Y, Up, Uc,
                       Un, coef, n, s, pv);
    LAUNCH_CHECK("lz0_update_kernel");
  }
  hipLaunchKernelGGL(lz0_alpha_kernel, dim3(sgrid), dim3(256), 0, sp->stream, pq, pv, nb, s, steps,
                     steps, st, dead, dal, dbe, coef);
  LAUNCH_CHECK("lz0_alpha_kernel");
  HIP_TRY(hipMemcpyAsync(h_alpha, dal, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipMemcpyAsync(h_beta, dbe, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

constexpr int LZ_NB = 512;   // row blocks of the DCGS2 dot partials (fixed: deterministic)

// Lanczos of K on s probe columns from V block 0 (normalised probes) with DCGS2
// reorthogonalisation (lz_*_kernel in gpmi_sparse.hip): per step one SpMM, one dot
// pass and one update pass over the basis. V: steps blocks [n][s]; U, Y: one block
// each. alpha / beta: host [s][steps]. *inexact: a column lost more than six digits
// of rho to cancellation (the caller reruns the block with CGS2).
int lanczos_block_dcgs2(gpmi_sp* sp, double* V, double* U, double* Y, int s, int steps,
                        double* h_alpha, double* h_beta, bool* inexact) {
  const int64_t n = sp->n, ns = n * s;
  const size_t hsz = (size_t)(steps + 2) * (steps + 1);
  const size_t need = (size_t)s * hsz + (size_t)(2 * steps + 2) * s + (size_t)steps * s +
                      (size_t)(steps + 1) * s + 2 * (size_t)s + 2 * (size_t)s * steps + 2 * s;
  HIP_TRY(sp->work.lzd.reserve(need));
  double* H = sp->work.lzd;
  double* d = H + (size_t)s * hsz;
  double* cv = d + (size_t)(2 * steps + 2) * s;
  double* cu = cv + (size_t)steps * s;
  double* ir = cu + (size_t)(steps + 1) * s;
  double* rho = ir + s;
  double* dal = rho + s;
  double* dbe = dal + (size_t)s * steps;
  int* dead = reinterpret_cast<int*>(dbe + (size_t)s * steps);
  int* inex = dead + s;
  // row blocks of the dot partials (fixed: deterministic; 256 / 1024 / 2048 measured
  // 2-5 % slower at cfg 5)
  const int lz_nb = LZ_NB;
  HIP_TRY(sp->work.partial.reserve((size_t)lz_nb * (2 * steps + 2) * s));
  HIP_TRY(hipMemsetAsync(H, 0, sizeof(double) * s * hsz, sp->stream));
  HIP_TRY(hipMemsetAsync(dal, 0, sizeof(double) * 2 * s * steps, sp->stream));
  HIP_TRY(hipMemcpyAsync(U, V, sizeof(double) * ns, hipMemcpyDeviceToDevice, sp->stream));
  // non-temporal basis reads for a basis over twice the 256 MB Infinity Cache (cfg 5
  // Lanczos 13.0 -> 11.2 ms; at cfg 4's 0.3 GB they measured slower, 6.8 -> 7.0 ms)
  const bool lz_nt = sizeof(double) * (double)ns * (steps + 1) > 512.0 * 1024 * 1024;
  for (int k = 0; k <= steps; ++k) {
    const bool last = k == steps;
    if (!last)
      if (int rc = spmm(sp, U, Y, s, 0.0)) return rc;
    const int nv = 2 * k + 2;
    for (int j0 = 0; j0 == 0 || j0 < k; j0 += LZ_JC) {
      // (column pairs with 16-byte loads measured slower: 15.9 against 13.1 ms per
      // cfg 5 Lanczos, at half the occupancy for the doubled accumulators)
      hipLaunchKernelGGL(lz_nt ? lz_dots_kernel<true> : lz_dots_kernel<false>, dim3(lz_nb),
                         dim3(256), 0, sp->stream, V, ns, k, j0, U,
                         last ? (const double*)nullptr : Y, n, s, nv, sp->work.partial);
      LAUNCH_CHECK("lz_dots_kernel");
    }
    hipLaunchKernelGGL(col_dot_reduce_kernel, dim3((nv * s + 3) / 4), dim3(256), 0, sp->stream,
                       sp->work.partial, lz_nb, nv, s, d);
    LAUNCH_CHECK("col_dot_reduce_kernel");
    const size_t sdb = sizeof(double) * (size_t)(2 * k + 2) * s;   // the dots in LDS
    const int stage = sdb <= 64 * 1024 ? 1 : 0;
    hipLaunchKernelGGL(lz_scalar_kernel, dim3(1), dim3(1024), stage ? sdb : 0, sp->stream, d, k,
                       steps, s, H, cv, cu, ir, rho, dead, inex, dal, dbe, stage);
    LAUNCH_CHECK("lz_scalar_kernel");
    if (!last) {
      // four row chunks per thread sharing its two columns' coefficients (cfg 5 Lanczos
      // 13.7 -> 12.65 ms against one): the grid's thread-pair count P with 2 P a
      // multiple of s
      const int64_t q = s / std::__gcd(512, s);
      int64_t g = (ns / 2 + 1023) / 1024;
      g = (g + q - 1) / q * q;
      auto kfn = lz_nt ? lz_update_kernel<4, true> : lz_update_kernel<4, false>;
      hipLaunchKernelGGL(kfn, dim3((unsigned)g), dim3(256), 0, sp->stream, V, ns, k, U, Y, cv, cu,
                         ir, s);
      LAUNCH_CHECK("lz_update_kernel");
    }
  }
  std::vector<int> hin(s);
  HIP_TRY(hipMemcpyAsync(h_alpha, dal, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipMemcpyAsync(h_beta, dbe, sizeof(double) * s * steps, hipMemcpyDeviceToHost,
                        sp->stream));
  HIP_TRY(hipMemcpyAsync(hin.data(), inex, sizeof(int) * s, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  *inexact = false;
  for (int c = 0; c < s; ++c) *inexact = *inexact || hin[c];
  return 0;
}

}  // namespace

extern "C" {

int gpmi_sp_lanczos(gpmi_sp* sp, int nprobe, int steps, uint64_t seed, int probe_offset,
                    double* alpha, double* beta) {
  return gpmi_sp_lanczos_ex(sp, nprobe, steps, seed, probe_offset, -1, alpha, beta);
}

int gpmi_sp_lanczos_ex(gpmi_sp* sp, int nprobe, int steps, uint64_t seed, int probe_offset,
                       int orthogonalize, double* alpha, double* beta) {
  if (!sp) return set_error(-1006, "null handle");
  if (steps < 1 || steps > 256 || nprobe < 1)
    return set_error(-1102, "steps must be in [1, 256] and nprobe >= 1");
  DeviceGuard g(sp->device);
  const int64_t n = sp->n;
  for (int p0 = 0; p0 < nprobe; p0 += MAXS) {
    const int s = std::min(MAXS, nprobe - p0);
    // the basis and a work block (the plain recurrence: three rotating blocks + one)
    HIP_TRY(sp->work.ws.reserve((size_t)std::max(steps + 2, 4) * n * s));
    double* V = sp->work.ws;
    double* W = sp->work.ws + (size_t)(steps + 1) * n * s;
    double *al = alpha + (size_t)p0 * steps, *be = beta + (size_t)p0 * steps;
    auto probes = [&]() -> int {
      hipLaunchKernelGGL(rademacher_kernel, dim3(grid_ns(n, s)), dim3(256), 0, sp->stream, V, n,
                         s, (unsigned long long)seed, probe_offset + p0,
                         1.0 / std::sqrt((double)n), (const int*)sp->perm_d);
      LAUNCH_CHECK("rademacher_kernel");
      return 0;
    };
    if (int rc = probes()) return rc;
    if (orthogonalize == 0) {
      // the plain three-term recurrence (imate's default)
      if (int rc = lanczos_block_plain(sp, V, sp->work.ws + 3 * (size_t)n * s, s, steps, al, be))
        return rc;
      continue;
    }
    if (orthogonalize > 0) {
      // windowed reorthogonalisation (imate's orthogonalize = k)
      if (int rc = lanczos_block(sp, V, W, s, steps, al, be, orthogonalize)) return rc;
      continue;
    }
    // DCGS2 (default; GPMI_LANCZOS=cgs2 selects CGS2). A block whose rho lost
    // precision to cancellation (near an invariant subspace) is redone with CGS2.
    const char* lenv = std::getenv("GPMI_LANCZOS");
    bool cgs2 = lenv && std::strcmp(lenv, "cgs2") == 0;
    if (!cgs2) {
      bool inexact = false;
      if (int rc = lanczos_block_dcgs2(sp, V, sp->work.ws + (size_t)steps * n * s, W, s, steps, al,
                                       be, &inexact))
        return rc;
      if (inexact) {
        ++sp->work.lanczos_cgs2_reruns;
        cgs2 = true;
        if (int rc = probes()) return rc;
      }
    }
    if (cgs2)
      if (int rc = lanczos_block(sp, V, W, s, steps, al, be)) return rc;
  }
  return 0;
}

}  // extern "C"
