// Correlation-scale gradient terms of the likelihood from the dense factor: with
// A = K(rho) + eta I, T = A^-1 (lower tiles: strict lower T_IJ in W's lower block triangle,
// diagonal T_II in Td, as gram_panel_kernel of gpmi_trinv.hip leaves them) and
// Sol = A^-1 [X | z] ([n_pad][17], gpmi_loo.hip), one pass contracts both with
// dK/d rho_k, formed entry by entry from the point coordinates and never stored:
//   t_k      = sum_ij T_ij             dK_ij / d rho_k
//   q_k(C_c) = sum_ij (Sol C_c Sol^T)_ij dK_ij / d rho_k,   C_c symmetric 16 x 16
// (dK_ij / d rho_k = h(x) u_k^2 / rho_k: gpmi_matern_dev.h).
//   scale_grad_pass_kernel    one workgroup per lower tile (I >= J) -> part[tile][1 + ncoef][8]:
//                             the tile's sums of V_ij h(x_ij) u_k^2, V = T, E_0, .., over
//                             the entries that count
//   scale_grad_reduce_kernel  out[v][k] = 2 / rho_k * sum over the tiles, ascending
// The matrices are symmetric and the diagonal contributes nothing (u = 0), so an
// off-diagonal tile stands for its mirror image too and a diagonal tile counts its strict
// lower triangle only, twice: the factor 2 of the reduce. Entries with i >= n or j >= n
// (the identity pad of A^-1) are skipped, points beyond n never read. Nothing is atomic:
// the same input gives the same bits.
//
// A wave owns a 64 x 64 quadrant (wr, wc) of the tile as 16 blocks of 16 x 16, each held
// as gram_panel_kernel's accumulators were: lane (fk, fr) has rows fk + 4 r, column fr.
// Per block the T values are loaded with that map (the loads mirror the stores), and
// E_c = (Sol_I C_c) Sol_J^T comes from v_mfma_f64_16x16x4f64 in two steps. First
// P^T = C_c Sol_I^T (16 x 16 rows of the block, depth 16, operands from LDS): its
// accumulators are P[row fr][fk + 4 r]. They are, as they stand, the A operands of the
// second product if step r of its depth loop takes the depth indices fk + 4 r in place of
// 4 r + fk, so the B operand of step r is Sol_J[column fr][fk + 4 r] from LDS and P never
// goes through memory. Neither T nor E is held whole in registers: one block at a time.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpmi_internal.h"
#include "gpmi_device.h"
#include "gpmi_matern_dev.h"

namespace gpmi {

namespace {

constexpr int SG_LD = 17;    // LDS row stride of the staged Sol rows and of C_c (odd: the
                             // fragment reads, 16 rows apart per lane, spread over the banks)
constexpr int SG_K = GPMI_MAX_DIM;

// Sum over the wave's 64 lanes, the same on every lane (xor butterfly: a fixed order).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace

// Grid: nt (nt + 1) / 2 workgroups of 256. NC: coefficient matrices computed (ncoef <= NC;
// the host rounds ncoef up to 0, 2 or 4 and pads coef with zero matrices). coef:
// [NC][16][16]; sol: [n_pad][LOO_LD] (not read when NC == 0). Two workgroups per CU up to
// NC = 2; the 5 x 8 running sums of NC = 4 fit one workgroup's register budget only.
template <int MODE, int NC>
__global__ __launch_bounds__(256, NC > 2 ? 1 : 2) void scale_grad_pass_kernel(
    const double* __restrict__ W, int64_t ldw, const double* __restrict__ Td,
    const double* __restrict__ sol, const double* __restrict__ coef, int ncoef,
    const double* __restrict__ points, int64_t n, int d, const double* __restrict__ scale_dev,
    int nt, double* __restrict__ part) {
  constexpr int NCS = NC > 0 ? NC : 1;
  __shared__ double sPI[TS * SG_K], sPJ[TS * SG_K];
  __shared__ double sSI[NC > 0 ? TS * SG_LD : 1], sSJ[NC > 0 ? TS * SG_LD : 1];
  __shared__ double sC[NCS * RLD * SG_LD];
  __shared__ double sscale[SG_K], srs[SG_K];
  __shared__ double sred[4][(1 + NCS) * SG_K];
  const int q = xcd_remap(blockIdx.x, gridDim.x);
  int I, J;
  tri_decode(q, nt, &I, &J);
  const int t = threadIdx.x, lane = t & 63;
  // the wave index as a scalar: the skipped blocks of a diagonal tile are scalar branches
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = w >> 1, wc = w & 1, fr = lane & 15, fk = lane >> 4;
  const int64_t i0 = (int64_t)I * TS, j0 = (int64_t)J * TS;
  if (t < SG_K) {
    const double sc = t < d ? scale_dev[t] : 1.0;
    sscale[t] = sc;
    srs[t] = 1.0 / sc;
  }
  for (int e = t; e < TS * SG_K; e += 256) {
    const int r = e >> 3, k = e & 7;
    sPI[e] = (k < d && i0 + r < n) ? points[(i0 + r) * d + k] : 0.0;
    sPJ[e] = (k < d && j0 + r < n) ? points[(j0 + r) * d + k] : 0.0;
  }
  if (NC > 0) {
    for (int e = t; e < TS * RLD; e += 256) {
      const int r = e >> 4, c = e & 15;
      sSI[r * SG_LD + c] = sol[(i0 + r) * LOO_LD + c];
      sSJ[r * SG_LD + c] = sol[(j0 + r) * LOO_LD + c];
    }
    for (int e = t; e < NC * RLD * RLD; e += 256)
      sC[(e >> 4) * SG_LD + (e & 15)] = coef[e];
  }
  __syncthreads();
  const double* C;
  int64_t ldc;
  if (I == J) {
    C = Td + (int64_t)I * TS * TS;
    ldc = TS;
  } else {
    C = W + i0 * ldw + j0;
    ldc = ldw;
  }
  const bool diag = I == J;
  double accT[SG_K], accE[NCS][SG_K];
#pragma unroll
  for (int k = 0; k < SG_K; ++k) {
    accT[k] = 0.0;
#pragma unroll
    for (int c = 0; c < NCS; ++c) accE[c][k] = 0.0;
  }
#pragma unroll 1
  for (int a = 0; a < 4; ++a) {
    const int rb = wr * 64 + a * 16;   // first tile row of the block row
    // P^T = C_c Sol_I^T for the 16 rows: pt[c][r] = (Sol_I C_c)[rb + fr][fk + 4 r]
    d4 pt[NCS];
    if (NC > 0) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        pt[c] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          pt[c] = mfma64(sC[(c * RLD + fr) * SG_LD + 4 * kk + fk],
                         sSI[(rb + fr) * SG_LD + 4 * kk + fk], pt[c]);
      }
    }
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
      const int cb = wc * 64 + b * 16;   // first tile column of the block
      // a diagonal tile counts row > column only: blocks above the diagonal hold none
      if (diag && rb + 15 <= cb) continue;
      d4 tv;
#pragma unroll
      for (int r = 0; r < 4; ++r) tv[r] = C[(int64_t)(rb + fk + 4 * r) * ldc + cb + fr];
      d4 ev[NCS];
      if (NC > 0) {
        double sj[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) sj[r] = sSJ[(cb + fr) * SG_LD + fk + 4 * r];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          ev[c] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int r = 0; r < 4; ++r) ev[c] = mfma64(pt[c][r], sj[r], ev[c]);
        }
      }
      const int col = cb + fr;
      double pj[SG_K];
#pragma unroll
      for (int k = 0; k < SG_K; ++k) pj[k] = sPJ[col * SG_K + k];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rb + fk + 4 * r;
        const bool ok = i0 + row < n && j0 + col < n && (!diag || row > col);
        if (ok) {
          const double* pi = &sPI[row * SG_K];
          const double x = scaled_distance(pi, pj, sscale, srs, d);
          const double f = matern_dscale_factor<MODE>(x);
#pragma unroll
          for (int k = 0; k < SG_K; ++k) {
            if (k < d) {
              const double u = div_by_scale(pi[k] - pj[k], sscale[k], srs[k]);
              const double g = matern_dscale_term<MODE>(f, x, u * u);
              accT[k] = fma(tv[r], g, accT[k]);
#pragma unroll
              for (int c = 0; c < NC; ++c) accE[c][k] = fma(ev[c][r], g, accE[c][k]);
            }
          }
        }
      }
    }
  }
  // the workgroup's sums: over each wave's lanes, then the four waves in order
#pragma unroll
  for (int k = 0; k < SG_K; ++k) {
    const double s = wave_sum(accT[k]);
    if (lane == 0) sred[w][k] = s;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double sc = wave_sum(accE[c][k]);
      if (lane == 0) sred[w][(1 + c) * SG_K + k] = sc;
    }
  }
  __syncthreads();
  const int nval = (1 + ncoef) * SG_K;
  if (t < nval)
    part[(int64_t)q * nval + t] = ((sred[0][t] + sred[1][t]) + sred[2][t]) + sred[3][t];
}

// out[v][k] = 2 / rho_k * sum_q part[q][v][k], q ascending; 0 for k >= d. One workgroup of
// (1 + ncoef) * 8 <= 64 threads.
__global__ __launch_bounds__(64) void scale_grad_reduce_kernel(const double* __restrict__ part,
                                                               int ntile, int nval, int d,
                                                               const double* __restrict__ scale_dev,
                                                               double* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= nval) return;
  const int k = t & (SG_K - 1);
  double s = 0.0;
  int q = 0;
  for (; q + 8 <= ntile; q += 8) {
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = part[(int64_t)(q + j) * nval + t];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; q < ntile; ++q) s += part[(int64_t)q * nval + t];
  out[t] = k < d ? 2.0 * s / scale_dev[k] : 0.0;
}

void launch_scale_grad_pass(hipStream_t s, int mode, int nc, const double* W, int64_t ldw,
                            const double* Td, const double* sol, const double* coef, int ncoef,
                            const double* points, int64_t n, int d, const double* scale, int nt,
                            double* part) {
  const dim3 grid((unsigned)(nt * (nt + 1) / 2)), block(256);
#define GPMI_SG_LAUNCH(M, C)                                                                  \
  hipLaunchKernelGGL((scale_grad_pass_kernel<M, C>), grid, block, 0, s, W, ldw, Td, sol, coef, \
                     ncoef, points, n, d, scale, nt, part)
#define GPMI_SG_MODE(M)                \
  do {                                 \
    if (nc == 0) GPMI_SG_LAUNCH(M, 0); \
    else if (nc == 2) GPMI_SG_LAUNCH(M, 2); \
    else GPMI_SG_LAUNCH(M, 4);         \
  } while (0)
  switch (mode) {
    case MATERN_HALF: GPMI_SG_MODE(MATERN_HALF); break;
    case MATERN_3HALF: GPMI_SG_MODE(MATERN_3HALF); break;
    case MATERN_5HALF: GPMI_SG_MODE(MATERN_5HALF); break;
    default: GPMI_SG_MODE(MATERN_GAUSS); break;
  }
#undef GPMI_SG_MODE
#undef GPMI_SG_LAUNCH
}

}  // namespace gpmi
