// Second-order terms of the likelihood in the hyperparameters (the expected information)
// from the dense factor. With A = K(rho) + eta I, N_0 = I, N_k = dK / d rho_k (k = 1..d),
// R = [X | z] the resident block, S = A^-1 R, M_0 = A^-1, M_k = A^-1 N_k, Y_a = N_a S and
// Z_a = A^-1 Y_a = M_a S:
//   T[a][b] = tr(M_a M_b)          U[a] = S^T Y_a          V[a][b] = Y_a^T Z_b.
// A^-1 is read from the tiles traceinv_build_ainv leaves (strict lower tiles in W's lower
// block triangle, diagonal tiles in Td, of which the lower triangle is read; the upper
// part is the mirror), N_k is formed from the point coordinates (gpmi_matern_dev.h) and
// never stored, M_k is.
//   fisher_product_kernel  M_k tile (I, J) = sum_p A^-1(I, p) N_k(p, J) on
//                          v_mfma_f64_16x16x4f64: per 16-deep slab, A^-1 rows go from the
//                          tiles to LDS and the slab of N_k is generated into LDS
//   fisher_trace_kernel    part[pair][tile (I, J)] = sum M_a(I, J) o M_b(J, I)^T, a <= b
//   fisher_trace_reduce_kernel   T[pair] = sum of the tiles, a fixed tree
//   fisher_thin_kernel     Z_a = M_a S (rows) and Y_k = M_k^T R (columns), one workgroup
//                          per 16 rows / columns running over the whole depth in order
//   fisher_gram_kernel     the 16 x 16 Grams U[a], V[a][b], rows ascending
// Rows and columns >= n (the identity pad of A^-1) are masked out, points beyond n never
// read, so M_k, Y and Z are zero in the pad. Nothing is atomic and every sum has a fixed
// order: the same input gives the same bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpmi_internal.h"
#include "gpmi_device.h"
#include "gpmi_matern_dev.h"

namespace gpmi {

namespace {

constexpr int FI_K = GPMI_MAX_DIM;

// Entry (i, j), i, j < n, of A^-1 from the tile storage.
__device__ __forceinline__ double ainv_at(const double* __restrict__ W, int64_t ldw,
                                          const double* __restrict__ Td, int64_t i, int64_t j) {
  const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
  const int64_t th = hi / TS, tl = lo / TS;
  if (th == tl) return Td[th * TS * TS + (hi - th * TS) * TS + (lo - tl * TS)];
  return W[hi * ldw + lo];
}

// Entry (i, j) of M_a: a = 0 is A^-1 with its pad masked, a >= 1 the stored product.
__device__ __forceinline__ double fisher_at(int a, const double* __restrict__ M, int64_t np,
                                            const double* __restrict__ W,
                                            const double* __restrict__ Td, int64_t n, int64_t i,
                                            int64_t j) {
  if (a == 0) return (i < n && j < n) ? ainv_at(W, np, Td, i, j) : 0.0;
  return M[((int64_t)(a - 1) * np + i) * np + j];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// The 8 entries of the slab A^-1[i0 .. i0 + 128)[p0 .. p0 + 16) this thread stages, and
// where they go: element e = q * 256 + t is (row, k) = (e >> 4, e & 15) where rows are
// contiguous in memory (tile below the diagonal, or the diagonal tile) and (e & 127, e >> 7)
// where the mirror is read (tile above the diagonal): full lines either way.
__device__ __forceinline__ void ainv_slab_load(const double* __restrict__ W, int64_t ldw,
                                               const double* __restrict__ Td, int I, int64_t p0,
                                               double (&v)[8]) {
  const int t = threadIdx.x;
  const int P = (int)(p0 / TS);
  const int64_t i0 = (int64_t)I * TS;
  // a uniform base and one 32-bit element offset per thread (at most 128 rows of ldw), the
  // 8 elements a uniform step apart
  if (I > P) {
    const double* base = W + i0 * ldw + p0;
    const uint32_t off = (uint32_t)((t >> 4) * ldw + (t & 15)), step = (uint32_t)(16 * ldw);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = base[off + q * step];
  } else if (I < P) {
    const double* base = W + p0 * ldw + i0;
    const uint32_t off = (uint32_t)((t >> 7) * ldw + (t & 127)), step = (uint32_t)(2 * ldw);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = base[off + q * step];
  } else {
    const double* td = Td + (int64_t)I * TS * TS;
    const int c = (int)(p0 - i0) + (t & 15);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = q * 16 + (t >> 4);
      v[q] = r >= c ? td[r * TS + c] : td[c * TS + r];
    }
  }
}

__device__ __forceinline__ void ainv_slab_store(double* s, int I, int64_t p0,
                                                const double (&v)[8]) {
  const int t = threadIdx.x;
  const bool mirror = I < (int)(p0 / TS);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = q * 256 + t;
    const int row = mirror ? (e & 127) : (e >> 4), k = mirror ? (e >> 7) : (e & 15);
    s[slab_off(row, k)] = v[q];
  }
}

}  // namespace

// Grid: (nt * nt, d) workgroups of 256; blockIdx.y = k - 1 is the dimension. M: [d][np][np].
// Thread t generates the slab's entries N_k[p0 + (t & 15)][j0 + (t >> 4) + 16 r], r < 8,
// straight into the buffer of the next stage: its depth point sits in registers, the
// tile's column points in LDS.
template <int MODE>
__global__ __launch_bounds__(256, 2) void fisher_product_kernel(
    const double* __restrict__ W, int64_t np, const double* __restrict__ Td,
    const double* __restrict__ points, int64_t n, int d, const double* __restrict__ scale_dev,
    int nt, double* __restrict__ M) {
  __shared__ double smem[4 * STAGE];
  __shared__ double sPJ[TS * FI_K];
  __shared__ double sscale[FI_K], srs[FI_K];
  double* sA = smem;
  double* sB = smem + 2 * STAGE;
  const int q = xcd_remap(blockIdx.x, gridDim.x);
  const int I = q / nt, J = q % nt, kd = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1, fr = lane & 15, fk = lane >> 4;
  const int64_t i0 = (int64_t)I * TS, j0 = (int64_t)J * TS;
  if (t < FI_K) {
    const double sc = t < d ? scale_dev[t] : 1.0;
    sscale[t] = sc;
    srs[t] = 1.0 / sc;
  }
  for (int e = t; e < TS * FI_K; e += 256) {
    const int r = e >> 3, k = e & 7;
    sPJ[e] = (k < d && j0 + r < n) ? points[(j0 + r) * d + k] : 0.0;
  }
  __syncthreads();
  const double rsk = srs[kd], sck = sscale[kd];
  const int gk = t & 15, gc = t >> 4;

  // the slab of N_k at depth p0 into the staged buffer s (two entries in flight: the
  // accumulators leave room for no more)
  auto generate = [&](int64_t p0, double* s) {
    const int64_t p = p0 + gk;
    double pp[FI_K];
#pragma unroll
    for (int k = 0; k < FI_K; ++k) pp[k] = (k < d && p < n) ? points[p * d + k] : 0.0;
    const double ppk = p < n ? points[p * d + kd] : 0.0;
#pragma unroll 2
    for (int r = 0; r < 8; ++r) {
      const int col = gc + 16 * r;
      double v = 0.0;
      if (p < n && j0 + col < n) {
        const double* pj = &sPJ[col * FI_K];
        const double x = scaled_distance(pj, pp, sscale, srs, d);
        const double f = matern_dscale_factor<MODE>(x);
        const double u = div_by_scale(pj[kd] - ppk, sck, rsk);
        v = matern_dscale_term<MODE>(f, x, u * u) * rsk;
      }
      s[slab_off(col, gk)] = v;
    }
  };

  d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
  // depth slabs that hold a point: N_k is zero beyond
  const int nslab = (int)((n + BK - 1) / BK);
  double av[8];
  ainv_slab_load(W, np, Td, I, 0, av);
  generate(0, sB);
  ainv_slab_store(sA, I, 0, av);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    const int cur = s & 1;
    const double* cA = sA + cur * STAGE;
    const double* cB = sB + cur * STAGE;
    const int64_t pn = (int64_t)(s + 1) * BK;
    // the other buffers were last read before the barrier that ended stage s - 1
    if (s + 1 < nslab) {
      ainv_slab_load(W, np, Td, I, pn, av);
      generate(pn, sB + (cur ^ 1) * STAGE);
    }
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = cA[slab_off(wr * 64 + i * 16 + fr, kk * 4 + fk)];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = cB[slab_off(wc * 64 + j * 16 + fr, kk * 4 + fk)];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma64(a[i], b[j], acc[i][j]);
    }
    if (s + 1 < nslab) ainv_slab_store(sA + (cur ^ 1) * STAGE, I, pn, av);
    __syncthreads();
  }
  double* C = M + ((int64_t)kd * np + i0) * np + j0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr * 64 + a * 16 + fk + 4 * r, col = wc * 64 + c * 16 + fr;
        // (rows >= n of A^-1 are its pad: masked, as everywhere)
        C[(int64_t)row * np + col] = i0 + row < n ? acc[a][c][r] : 0.0;
      }
}

// Grid: (nt * nt, npair) workgroups of 256; pair y is (a, b), a <= b, in row-major order of
// the upper triangle of (d + 1) x (d + 1). part[y][tile] = sum over the tile (I, J) of
// M_a[i][j] M_b[j][i], by 32 x 32 blocks of M_b transposed through LDS.
__global__ __launch_bounds__(256) void fisher_trace_kernel(const double* __restrict__ M,
                                                           int64_t np,
                                                           const double* __restrict__ W,
                                                           const double* __restrict__ Td,
                                                           int64_t n, int d, int nt,
                                                           double* __restrict__ part) {
  __shared__ double sT[32 * 33];
  __shared__ double sred[4];
  const int q = blockIdx.x, I = q / nt, J = q % nt;
  int a = 0, b = (int)blockIdx.y;
  while (b > d - a) {
    b -= d - a + 1;
    ++a;
  }
  b += a;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t i0 = (int64_t)I * TS, j0 = (int64_t)J * TS;
  double acc = 0.0;
  for (int bi = 0; bi < 4; ++bi)
    for (int bj = 0; bj < 4; ++bj) {
      const int64_t ib = i0 + bi * 32, jb = j0 + bj * 32;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = u * 256 + t, r = e >> 5, c = e & 31;
        sT[r * 33 + c] = fisher_at(b, M, np, W, Td, n, jb + r, ib + c);
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = u * 256 + t, r = e >> 5, c = e & 31;
        acc = fma(fisher_at(a, M, np, W, Td, n, ib + r, jb + c), sT[c * 33 + r], acc);
      }
    }
  const double s = wave_sum(acc);
  if (lane == 0) sred[w] = s;
  __syncthreads();
  if (t == 0)
    part[(int64_t)blockIdx.y * gridDim.x + q] = ((sred[0] + sred[1]) + sred[2]) + sred[3];
}

// Grid: npair workgroups of 256. out[y] = sum_q part[y][q]: thread t adds q = t, t + 256, ..
// in order, then a fixed tree over the threads.
__global__ __launch_bounds__(256) void fisher_trace_reduce_kernel(const double* __restrict__ part,
                                                                  int ntile,
                                                                  double* __restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const double* p = part + (int64_t)blockIdx.x * ntile;
  double s = 0.0;
  for (int q = t; q < ntile; q += 256) s += p[q];
  red[t] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) out[blockIdx.x] = red[0];
}

// Y_0[i][c] = sol[i][c] (the leave-one-out pass's block, leading dimension 17).
__global__ __launch_bounds__(256) void fisher_copy_sol_kernel(const double* __restrict__ sol,
                                                              int64_t np,
                                                              double* __restrict__ Y0) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < np * RLD) Y0[e] = sol[(e >> 4) * LOO_LD + (e & 15)];
}

// Grid: (np / 16, count) workgroups of 256; matrix a = a0 + blockIdx.y.
//   TRANS false: out[y][i][c] = sum_j M_a[i][j] X[j][c]   (16 rows i per workgroup)
//   TRANS true : out[y][j][c] = sum_i M_a[i][j] X[i][c]   (16 columns j per workgroup)
// X: [np][ldx], 16 columns read. The depth runs in chunks of 128 through LDS, ascending.
template <bool TRANS>
__global__ __launch_bounds__(256) void fisher_thin_kernel(int a0, const double* __restrict__ M,
                                                          int64_t np,
                                                          const double* __restrict__ W,
                                                          const double* __restrict__ Td,
                                                          int64_t n, const double* __restrict__ X,
                                                          int ldx, double* __restrict__ out) {
  __shared__ double sM[16 * 129];
  __shared__ double sX[128 * 17];
  const int a = a0 + (int)blockIdx.y;
  const int t = threadIdx.x, r = t >> 4, c = t & 15;
  const int64_t b0 = (int64_t)blockIdx.x * 16;
  double acc = 0.0;
  for (int64_t c0 = 0; c0 < np; c0 += 128) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = u * 256 + t;
      if (TRANS) {
        const int dd = e >> 4, rr = e & 15;
        sM[rr * 129 + dd] = fisher_at(a, M, np, W, Td, n, c0 + dd, b0 + rr);
      } else {
        const int rr = e >> 7, dd = e & 127;
        sM[rr * 129 + dd] = fisher_at(a, M, np, W, Td, n, b0 + rr, c0 + dd);
      }
      sX[(e >> 4) * 17 + (e & 15)] = X[(c0 + (e >> 4)) * ldx + (e & 15)];
    }
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < 128; ++j) acc = fma(sM[r * 129 + j], sX[j * 17 + c], acc);
  }
  out[((int64_t)blockIdx.y * np + b0 + r) * RLD + c] = acc;
}

// Grid: (d + 1) + (d + 1)^2 workgroups of 256. YZ: [2][d + 1][np][16], Y then Z.
//   g <  d + 1: out[g] = Y_0^T Y_g                        (U[g])
//   g >= d + 1: out[g] = Y_a^T Z_b, (a, b) = divmod(g - (d + 1), d + 1)   (V[a][b])
// each [16][16]; rows in chunks of 128 through LDS, ascending.
__global__ __launch_bounds__(256) void fisher_gram_kernel(const double* __restrict__ YZ,
                                                          int64_t np, int d,
                                                          double* __restrict__ out) {
  __shared__ double sP[128 * 17], sQ[128 * 17];
  const int g = blockIdx.x, d1 = d + 1;
  const int64_t blk = np * RLD;
  const double *P, *Q;
  if (g < d1) {
    P = YZ;
    Q = YZ + (int64_t)g * blk;
  } else {
    P = YZ + (int64_t)((g - d1) / d1) * blk;
    Q = YZ + (int64_t)(d1 + (g - d1) % d1) * blk;
  }
  const int t = threadIdx.x, r = t >> 4, c = t & 15;
  double acc = 0.0;
  for (int64_t c0 = 0; c0 < np; c0 += 128) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = u * 256 + t;
      sP[(e >> 4) * 17 + (e & 15)] = P[c0 * RLD + e];
      sQ[(e >> 4) * 17 + (e & 15)] = Q[c0 * RLD + e];
    }
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < 128; ++j) acc = fma(sP[j * 17 + r], sQ[j * 17 + c], acc);
  }
  out[(int64_t)g * RLD * RLD + t] = acc;
}

void launch_fisher_product(hipStream_t s, int mode, const double* W, int64_t np, const double* Td,
                           const double* points, int64_t n, int d, const double* scale, int nt,
                           double* M) {
  const dim3 grid((unsigned)(nt * nt), (unsigned)d), block(256);
#define GPMI_FI_LAUNCH(MD)                                                                   \
  hipLaunchKernelGGL((fisher_product_kernel<MD>), grid, block, 0, s, W, np, Td, points, n, d, \
                     scale, nt, M)
  switch (mode) {
    case MATERN_HALF: GPMI_FI_LAUNCH(MATERN_HALF); break;
    case MATERN_3HALF: GPMI_FI_LAUNCH(MATERN_3HALF); break;
    case MATERN_5HALF: GPMI_FI_LAUNCH(MATERN_5HALF); break;
    default: GPMI_FI_LAUNCH(MATERN_GAUSS); break;
  }
#undef GPMI_FI_LAUNCH
}

void launch_fisher_thin(hipStream_t s, bool trans, int a0, int count, const double* M, int64_t np,
                        const double* W, const double* Td, int64_t n, const double* X, int ldx,
                        double* out) {
  const dim3 grid((unsigned)(np / 16), (unsigned)count), block(256);
  if (trans)
    hipLaunchKernelGGL(fisher_thin_kernel<true>, grid, block, 0, s, a0, M, np, W, Td, n, X, ldx,
                       out);
  else
    hipLaunchKernelGGL(fisher_thin_kernel<false>, grid, block, 0, s, a0, M, np, W, Td, n, X, ldx,
                       out);
}

}  // namespace gpmi
