// Device-side pieces of the Matérn kernel shared by the assembly (gpmi_matern.hip) and the
// correlation-scale gradient (gpmi_scale_grad.hip): the scaled distance, bit for bit the
// same in both, and the derivative of a correlation entry in the scale.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "gpmi_internal.h"

namespace gpmi {

// (p_i - p_j) / scale, correctly rounded as the reference's division, from the
// correctly rounded reciprocal rs = RN(1 / scale): q0 = RN(a rs), the exact
// remainder a - q0 scale (FMA), q = RN(q0 + rem rs) (Markstein's final step:
// RN(a / scale) whenever rs is within half an ulp of 1 / scale and q0 within one
// ulp of a / scale, no overflow / underflow; 2e8 random cases checked equal on
// the host). One multiply and two FMAs instead of the ~10-instruction IEEE
// division sequence.
__device__ __forceinline__ double div_by_scale(double a, double sc, double rs) {
  const double q0 = a * rs;
  const double rem = fma(-q0, sc, a);
  return fma(rem, rs, q0);
}

// Scaled Euclidean distance, summed in dimension order (_kernels.pyx:130-136).
// Unrolled to GPMI_MAX_DIM so p_j stays in registers.
__device__ __forceinline__ double scaled_distance(const double* __restrict__ pi,
                                                  const double (&pj)[GPMI_MAX_DIM],
                                                  const double* __restrict__ scale,
                                                  const double* __restrict__ rscale, int d) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < GPMI_MAX_DIM; ++k) {
    if (k < d) {
      const double v = div_by_scale(pi[k] - pj[k], scale[k], rscale[k]);
      acc += v * v;
    }
  }
  return sqrt(acc);
}

// The derivative of a correlation entry in the scale of dimension k. With
// u_k = (p_i - p_j)_k / rho_k and x = sqrt(sum_k u_k^2), M the Matérn correlation,
//   dK_ij / d rho_k = h(x) u_k^2 / rho_k,   h(x) = -M'(x) / x:
//   nu = 1/2   h = exp(-x) / x
//   nu = 3/2   h = 3 exp(-sqrt(3) x)
//   nu = 5/2   h = (5 / 3) (1 + sqrt(5) x) exp(-sqrt(5) x)
//   Gaussian   h = exp(-x^2 / 2)
// matern_dscale_factor is the part evaluated once per entry (for nu = 1/2 without the
// 1 / x), matern_dscale_term the entry's h(x) u_k^2. For nu = 1/2 the term is formed as
// exp(-x) (u_k^2 / x), finite because u_k^2 <= x^2, and is exactly 0 at x = 0
// (duplicated points). The closed forms and the Gaussian limit only: a general nu
// (MATERN_GENERAL) has no form here (for nu > 1, h = nu / (nu - 1) M_{nu-1}(t) at the
// same t = sqrt(2 nu) x: DESIGN.md section 2h).
template <int MODE>
__device__ __forceinline__ double matern_dscale_factor(double x) {
  switch (MODE) {
    case MATERN_HALF:
      return exp(-x);
    case MATERN_3HALF: {
      const double s3 = 1.7320508075688772;   // sqrt(3.0), correctly rounded
      return 3.0 * exp(-s3 * x);
    }
    case MATERN_5HALF: {
      const double s5 = 2.23606797749979;     // sqrt(5.0), correctly rounded
      return (5.0 / 3.0) * (1.0 + s5 * x) * exp(-s5 * x);
    }
    default:
      return exp(-0.5 * (x * x));
  }
}

template <int MODE>
__device__ __forceinline__ double matern_dscale_term(double f, double x, double u2) {
  if (MODE == MATERN_HALF) return x == 0.0 ? 0.0 : f * (u2 / x);
  return f * u2;
}

}  // namespace gpmi
