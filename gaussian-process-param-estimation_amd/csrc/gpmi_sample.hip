// Draws z = L xi, xi ~ N(0, I), from the cached Cholesky factor of K + eta I = L L^T, so
// that z ~ N(0, K + eta I) (gpmi_dense_sample.hip: gpmi_op_sample), and the hand-over of the
// prediction's joint covariance to a second operator (gpmi_op_load_predict_cov).
//
// The normals and the draws are sample-major, Xi_t / Y_t [draws][n_pad] (one draw is one
// contiguous row), so both MFMA operands of Y_t = Xi_t L^T are [row][k] slabs (tile_mma, as
// in the prediction's trailing product). Work list and depth pieces: gpmi_sample_plan.h.
//   sample_normal_kernel   Xi_t: counter-based standard normals (Box-Muller on splitmix64)
//   sample_trmm_kernel     one (row tile I, depth piece, draw tile J) per workgroup:
//                            sum over the piece's k of Xi_t_Jk L_Ik^T from zero, the
//                            diagonal tile L_II masked to its lower triangle on the way
//                            into LDS; into Y_t, or into a partial tile when split
//   sample_reduce_kernel   Y_t tile = its pieces in ascending order (nothing atomic)
//   cov_lowrank_kernel     K of the second operator <- C0 + U U^T, identity in the pad
// Pad columns of Xi_t meet the zero columns i >= n of L's first n rows, pad rows of Xi_t
// only produce pad rows of Y_t: neither reaches a returned value.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpmi_internal.h"
#include "gpmi_device.h"
#include "gpmi_sample_plan.h"

namespace gpmi {

namespace {

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// ((x >> 11) + 0.5) 2^-53: in (0, 1], never zero.
__device__ __forceinline__ double unit_open(unsigned long long x) {
  return ((double)(x >> 11) + 0.5) * 0x1.0p-53;
}

__device__ __forceinline__ void store_c(double* C, int64_t ldc, const d4 (&acc)[4][4]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = wv >> 1, wc = wv & 1, fr = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        C[(int64_t)(wr * 64 + a * 16 + fk + 4 * r) * ldc + wc * 64 + c * 16 + fr] = acc[a][c][r];
}

// The entries k > row of the slab gload_slab(base, ld, p, r) has loaded from a diagonal
// tile, replaced by zero: what is left is the lower triangle, diagonal included.
__device__ __forceinline__ void mask_upper(int p, d2 (&r)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = i * 256 + t;
    const int row = idx >> 3, k = p + 2 * (idx & 7);
    if (k > row) r[i][0] = 0.0;
    if (k + 1 > row) r[i][1] = 0.0;
  }
}

// acc += P1[0:128, 0:128] tril(P2[0:128, 0:128])^T: tile_mma's KLOOP_LATE loop over a
// depth of 128 with P2's slabs masked between the global load and the LDS store, so that
// nothing above the diagonal of P2 reaches an MFMA, whatever the tile holds there.
__device__ __forceinline__ void tile_mma_tril(const double* __restrict__ P1, int64_t ld1,
                                              const double* __restrict__ P2, int64_t ld2,
                                              double* sA, double* sB, d4 (&acc)[4][4]) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int fr = lane & 15, fk = lane >> 4;
  d2 ra[4], rb[4];
  gload_slab(P1, ld1, 0, ra);
  gload_slab(P2, ld2, 0, rb);
  mask_upper(0, rb);
  sstore_slab(sA, ra);
  sstore_slab(sB, rb);
  __syncthreads();
  constexpr int nsteps = TS / BK;
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    const double* cA = sA + cur * STAGE;
    const double* cB = sB + cur * STAGE;
    if (s + 1 < nsteps) {
      gload_slab(P1, ld1, (s + 1) * BK, ra);
      gload_slab(P2, ld2, (s + 1) * BK, rb);
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
    if (s + 1 < nsteps) {
      mask_upper((s + 1) * BK, rb);
      sstore_slab(sA + (cur ^ 1) * STAGE, ra);
      sstore_slab(sB + (cur ^ 1) * STAGE, rb);
    }
    __syncthreads();
  }
}

}  // namespace

// Xi[j][i], j < rows, i < cols (cols <= ld): the standard normal of (seed, draw first + j,
// row i), a function of those three alone (gaussian_proc/_normal.py states it on the host):
//   key = seed G + (first + j) H,  x1 = splitmix64(key + 2 i),  x2 = splitmix64(key + 2 i + 1)
//   u = ((x >> 11) + 0.5) 2^-53,   xi = sqrt(-2 ln u1) cos(2 pi u2)
// with G, H the constants of rademacher_kernel (gpmi_sparse.hip).
__global__ __launch_bounds__(256) void sample_normal_kernel(double* __restrict__ Xi, int64_t ld,
                                                            int64_t rows, int64_t cols,
                                                            unsigned long long seed,
                                                            unsigned long long first) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * cols) return;
  const int64_t j = e / cols, i = e - j * cols;
  const unsigned long long key = seed * 0x9E3779B97F4A7C15ull +
                                 (first + (unsigned long long)j) * 0xD1B54A32D192ED03ull;
  const double u1 = unit_open(splitmix64(key + 2ull * (unsigned long long)i));
  const double u2 = unit_open(splitmix64(key + 2ull * (unsigned long long)i + 1ull));
  const double rad = sqrt(-2.0 * log(u1));
  const double ang = 6.283185307179586 * u2;
  Xi[j * ld + i] = rad * cos(ang);
}

// Grid: items * jt workgroups, items = sample_items(nt, D); workgroup q runs piece
// order[q / jt] = (I << 16) | p for draw tile J = q % jt, so that the workgroups in flight
// on one XCD (xcd_remap) share the piece's slabs of L in its L2. Reads L's lower tiles
// (I, k), k <= I, and Xi; writes tile (J, I) of Y [128 jt][ldy] (split == 0: the piece is
// the whole row tile) or the partial tile (sample_piece_base(I, D) + p) jt + J of part.
// Each workgroup writes a tile of its own and reads nothing another writes.
__global__ __launch_bounds__(256, 2) void sample_trmm_kernel(const double* __restrict__ L,
                                                             int64_t lda,
                                                             const double* __restrict__ Xi,
                                                             int64_t ldx, int jt, int D, int split,
                                                             const uint32_t* __restrict__ order,
                                                             double* __restrict__ Y, int64_t ldy,
                                                             double* __restrict__ part) {
  __shared__ double smem[4 * STAGE];
  const int q = xcd_remap(blockIdx.x, gridDim.x);
  const int item = q / jt;
  // (the tile indices as scalars: the operand bases of the k-loop's slab loads live in SGPRs)
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)order[item]);
  const int J = __builtin_amdgcn_readfirstlane(q - item * jt);
  const int I = (int)(w >> 16), p = (int)(w & 0xffffu);
  int k0, k1;
  sample_piece_range(I, D, p, &k0, &k1);
  const bool diag = k1 == I + 1;          // the piece ends in the diagonal tile
  const int nfull = k1 - k0 - (diag ? 1 : 0);
  const double* rowX = Xi + (int64_t)J * TS * ldx;
  const double* rowL = L + (int64_t)I * TS * lda;
  d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
  d4 dummy[2];
  if (nfull > 0)
    tile_mma<false, false, KLOOP_EARLY>(rowX + (int64_t)k0 * TS, ldx, rowL + (int64_t)k0 * TS, lda,
                                        nfull * TS, smem, smem + 2 * STAGE, acc, nullptr, dummy);
  if (diag)
    tile_mma_tril(rowX + (int64_t)I * TS, ldx, rowL + (int64_t)I * TS, lda, smem,
                  smem + 2 * STAGE, acc);
  if (split)
    store_c(part + ((sample_piece_base(I, D) + p) * jt + J) * (int64_t)(TS * TS), TS, acc);
  else
    store_c(Y + (int64_t)J * TS * ldy + (int64_t)I * TS, ldy, acc);
}

// Y tile (J, I) = sum over p < sample_pieces(I, D) of its partial tiles, p ascending.
// Grid: (nt * jt, 8), a workgroup takes 16 rows of its tile.
__global__ __launch_bounds__(256) void sample_reduce_kernel(const double* __restrict__ part,
                                                            int jt, int D, double* __restrict__ Y,
                                                            int64_t ldy) {
  const int I = blockIdx.x / jt, J = blockIdx.x - I * jt;
  const int np = sample_pieces(I, D);
  const double* pt = part + (sample_piece_base(I, D) * jt + J) * (int64_t)(TS * TS);
  const int64_t pstride = (int64_t)jt * TS * TS;
  const int t = threadIdx.x, c = t & (TS - 1);
  double* Yji = Y + (int64_t)J * TS * ldy + (int64_t)I * TS;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = blockIdx.y * 16 + (t >> 7) + 2 * i;
    double s = 0.0;
    for (int p = 0; p < np; ++p) s += pt[p * pstride + r * TS + c];
    Yji[(int64_t)r * ldy + c] = s;
  }
}

// dst [np][ldd = np] <- src[j][l] + sum_a U[j][a] U[l][a] for j, l < n (a ascending, one
// fma each, so that (j, l) and (l, j) get the same bits from a symmetric src), the
// identity elsewhere. src: [.][lds] with lds >= n; U: [n][m] packed, m <= 15. m == 0 is a
// plain copy.
__global__ __launch_bounds__(256) void cov_lowrank_kernel(const double* __restrict__ src,
                                                          int64_t lds, double* __restrict__ dst,
                                                          int64_t np, int64_t n,
                                                          const double* __restrict__ U, int m) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= np * np) return;
  const int64_t j = e / np, l = e - j * np;
  double v;
  if (j < n && l < n) {
    v = src[j * lds + l];
    for (int a = 0; a < m; ++a) v = fma(U[j * m + a], U[l * m + a], v);
  } else {
    v = j == l ? 1.0 : 0.0;
  }
  dst[e] = v;
}

}  // namespace gpmi
