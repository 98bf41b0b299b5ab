// Prediction terms at new points from the cached Cholesky factor of S = K + eta I = L L^T:
// for a chunk of test columns v_j = L^-1 k*_j (k*_j the correlations of test point j with
// the n training points) the device returns per column
//   c_j = Y^T v_j  (16 numbers, Y = L^-1 [X | z] forward-substituted, resident)
//   q_j = v_j^T v_j
// from which the host forms the posterior mean and variance (gaussian_proc:
// _predict_from_terms). V never leaves the device.
//
// The working block holds the chunk TRANSPOSED, T[j][i] (row j a test column, i the
// training index, leading dimension ldt = n_pad): both MFMA operands of every product
// are then [row][k] slabs (tile_mma, as in the factorization), and the trailing product's
// C tiles load and store as contiguous rows. Launch list: gpmi_predict_plan.h.
//   pred_diag_kernel    tile row k, one workgroup per column tile j:
//                         T_jk -= V_j,[kb,k) L_k,[kb,k)^T   (inside the outer panel)
//                         V_k = Linv_kk T_k  (MFMA, accumulators [training][test]),
//                         stored transposed in place; and with V_k still in registers
//                         its accumulator fragments ARE the B operands of
//                         Y_k^T V_k (16 x 128 x 128 on MFMA), plus the column sums of
//                         squares: part[k][col][0..15 | 16]
//   pred_update_kernel  T_ji -= V_j,[kb,ke) L_i,[kb,ke)^T for the tile rows below a panel
//   pred_reduce_kernel  out[e] = sum_k part[k][e], k ascending (deterministic)
//   pred_gram_kernel    per tile row, Y_k^T Y_k (16 x 16) -> summed by pred_reduce_kernel
// Rows i >= n of T are zero and L's pad is the identity, so V's pad rows stay zero and
// contribute nothing.
//
// The joint covariance (gpmi_op_predict_cov) keeps every chunk's rows of T, so that V^T for
// all test points is one [nsp][ldt] block, and forms C0 = K** - V V^T from it:
//   pred_cov_partial_kernel  one (lower tile, depth piece) per workgroup, -T_J T_L^T
//   pred_cov_reduce_kernel   K** + the pieces in ascending order, stored with its mirror

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpmi_internal.h"
#include "gpmi_device.h"
#include "gpmi_predict_plan.h"

namespace gpmi {

namespace {

// C tile <-> accumulators (wave tile 64 x 64 at (wr, wc); C/D map of
// v_mfma_f64_16x16x4f64: row = (lane >> 4) + 4 r, col = lane & 15).
__device__ __forceinline__ void load_c(const double* C, int64_t ldc, d4 (&acc)[4][4]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = wv >> 1, wc = wv & 1, fr = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[a][c][r] = C[(int64_t)(wr * 64 + a * 16 + fk + 4 * r) * ldc + wc * 64 + c * 16 + fr];
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

// Transposed tile store: acc element (row R, col C) -> T[C * ldt + R].
__device__ __forceinline__ void store_transposed(double* T, int64_t ldt, const d4 (&acc)[4][4]) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1, fr = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        T[(int64_t)(wc * 64 + c * 16 + fr) * ldt + wr * 64 + a * 16 + fk + 4 * r] = acc[a][c][r];
}

// Workgroup barrier that orders this workgroup's global stores before its later global
// loads (a tile stored by some threads is read back by others).
__device__ __forceinline__ void wg_global_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace

// Grid: ni * nct workgroups; tile (i0 + i, j) by predict_tile. Reads V_j,[kb,ke) (final)
// and L_i,[kb,ke); writes T_ji, i >= ke: no workgroup reads what another writes.
__global__ __launch_bounds__(256, 2) void pred_update_kernel(const double* __restrict__ L,
                                                             int64_t lda, double* T,
                                                             int64_t ldt, int i0, int ni,
                                                             int nct, int kb, int ke) {
  __shared__ double smem[4 * STAGE];
  const int q = xcd_remap(blockIdx.x, gridDim.x);
  int i, j;
  predict_tile(q, ni, nct, &i, &j);
  // (the tile indices as scalars: the operand bases of the k-loop's slab loads live in SGPRs)
  i = __builtin_amdgcn_readfirstlane(i) + i0;
  j = __builtin_amdgcn_readfirstlane(j);
  double* rowJ = T + (int64_t)j * TS * ldt;
  double* C = rowJ + (int64_t)i * TS;
  d4 acc[4][4];
  load_c(C, ldt, acc);
  d4 dummy[2];
  tile_mma<false, true, KLOOP_EARLY>(rowJ + (int64_t)kb * TS, ldt,
                                     L + (int64_t)i * TS * lda + (int64_t)kb * TS, lda,
                                     (ke - kb) * TS, smem, smem + 2 * STAGE, acc, nullptr, dummy);
  store_c(C, ldt, acc);
}

// Grid: nct workgroups (column tile j = blockIdx.x). Y: the resident [n_pad][16] block
// L^-1 [X | z]; part: [nt][ns_ld][17] with ns_ld = 128 nct.
__global__ __launch_bounds__(256, 2) void pred_diag_kernel(const double* __restrict__ L,
                                                           int64_t lda,
                                                           const double* __restrict__ Linv,
                                                           const double* __restrict__ Y,
                                                           double* T, int64_t ldt, int k, int kb,
                                                           double* __restrict__ part,
                                                           int64_t ns_ld) {
  __shared__ double smem[4 * STAGE + TS * RLD];
  double* sA = smem;
  double* sB = smem + 2 * STAGE;
  double* sY = smem + 4 * STAGE;
  const int j = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1, fr = lane & 15, fk = lane >> 4;
  double* rowJ = T + (int64_t)j * TS * ldt;
  double* Tjk = rowJ + (int64_t)k * TS;
  {
    // Y_k into LDS (read after the barriers of the operand pipeline)
    const double* Yk = Y + (int64_t)k * TS * RLD;
    d2 v[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) v[it] = *reinterpret_cast<const d2*>(Yk + 2 * (it * 256 + t));
#pragma unroll
    for (int it = 0; it < 4; ++it) *reinterpret_cast<d2*>(&sY[2 * (it * 256 + t)]) = v[it];
  }
  d4 acc[4][4];
  d4 dummy[2];
  if (k > kb) {
    load_c(Tjk, ldt, acc);
    tile_mma<false, true>(rowJ + (int64_t)kb * TS, ldt,
                          L + (int64_t)k * TS * lda + (int64_t)kb * TS, lda, (k - kb) * TS, sA, sB,
                          acc, nullptr, dummy);
    store_c(Tjk, ldt, acc);
    wg_global_barrier();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
  // acc[r][c] = sum_q Linv_kk[r][q] T_k[q][c], T_k[q][c] = Tjk[c * ldt + q]
  tile_mma<false>(Linv + (int64_t)k * TS * TS, TS, Tjk, ldt, TS, sA, sB, acc, nullptr, dummy);
  store_transposed(Tjk, ldt, acc);
  // Epilogue. Accumulator fragment acc[a][c][r] holds V[R0 + fk][C0 + fr] with
  // R0 = wr*64 + a*16 + 4 r, C0 = wc*64 + c*16: the B operand (B[k = fk][j = fr]) of
  // ep_c += Y[R0 .. R0+3][0:16]^T V[R0 .. R0+3][C0 .. C0+15], whose A operand
  // A[i = fr][k = fk] = Y[R0 + fk][fr] comes from LDS. ep[c][r2] = entry fk + 4 r2 of
  // column C0 + fr, over the wave's 64 rows, rows ascending.
  d4 ep[4];
  double qs[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    ep[c] = d4{0.0, 0.0, 0.0, 0.0};
    qs[c] = 0.0;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double y = sY[(wr * 64 + a * 16 + 4 * r + fk) * RLD + fr];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        ep[c] = mfma64(y, acc[a][c][r], ep[c]);
        qs[c] = fma(acc[a][c][r], acc[a][c][r], qs[c]);
      }
    }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    qs[c] += __shfl_xor(qs[c], 16);
    qs[c] += __shfl_xor(qs[c], 32);
  }
  // the two row halves (wr) are added in a fixed order: wr = 1 hands over through LDS
  // (the operand stages are free: tile_mma ended with a barrier)
  double* red = smem;   // [wc][c][17][16]
  if (wr == 1) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double* o = red + (wc * 4 + c) * PRED_LD * 16;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(fk + 4 * r) * 16 + fr] = ep[c][r];
      if (fk == 0) o[16 * 16 + fr] = qs[c];
    }
  }
  __syncthreads();
  if (wr == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double* o = red + (wc * 4 + c) * PRED_LD * 16;
      double* out = part + ((int64_t)k * ns_ld + (int64_t)j * TS + wc * 64 + c * 16 + fr) * PRED_LD;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[fk + 4 * r] = ep[c][r] + o[(fk + 4 * r) * 16 + fr];
      if (fk == 0) out[16] = qs[c] + o[16 * 16 + fr];
    }
  }
}

// out[e] = sum over k < nt of part[k * cnt + e], k ascending.
__global__ __launch_bounds__(256) void pred_reduce_kernel(const double* __restrict__ part,
                                                          int nt, int64_t cnt,
                                                          double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cnt) return;
  double s = 0.0;
  for (int k = 0; k < nt; ++k) s += part[(int64_t)k * cnt + e];
  out[e] = s;
}

// gpart[k][a][c] = sum_r Y_k[r][a] Y_k[r][c], r ascending (one workgroup per tile row).
__global__ __launch_bounds__(256) void pred_gram_kernel(const double* __restrict__ Y,
                                                        double* __restrict__ gpart) {
  __shared__ double sY[TS * RLD];
  const int k = blockIdx.x, t = threadIdx.x;
  for (int e = t; e < TS * RLD; e += 256) sY[e] = Y[(int64_t)k * TS * RLD + e];
  __syncthreads();
  const int a = t >> 4, c = t & 15;
  double s = 0.0;
  for (int r = 0; r < TS; ++r) s = fma(sY[r * RLD + a], sY[r * RLD + c], s);
  gpart[(int64_t)k * 256 + t] = s;
}

// Joint covariance C0 = K** - V V^T of the test points, V^T = T [nsp][ldt] whole
// (every chunk's rows kept). Grid: ntiles * S workgroups, ntiles = nct (nct + 1) / 2
// lower tiles (J, L), J >= L, by tri_decode; workgroup q = piece * ntiles + tile, so
// the workgroups in flight on one XCD (xcd_remap) run consecutive tiles of one depth
// piece and share its row slabs in L2. Piece p covers the tile rows
// [p nt / S, (p + 1) nt / S) (predict_cov_piece_begin). Both operands are [row][k] slabs
// of T; the partial, -T_J,[k0,k1) T_L,[k0,k1)^T from zero accumulators, goes to
// part[tile][p][128][128]. Reads T only; each workgroup writes its own partial tile.
__global__ __launch_bounds__(256, 2) void pred_cov_partial_kernel(const double* __restrict__ T,
                                                                  int64_t ldt, int nct, int nt,
                                                                  int S,
                                                                  double* __restrict__ part) {
  __shared__ double smem[4 * STAGE];
  const int ntiles = nct * (nct + 1) / 2;
  const int q = xcd_remap(blockIdx.x, gridDim.x);
  const int p = q / ntiles, tile = q - p * ntiles;
  int J, L;
  tri_decode(tile, nct, &J, &L);
  const int k0 = predict_cov_piece_begin(nt, S, p), k1 = predict_cov_piece_begin(nt, S, p + 1);
  d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
  d4 dummy[2];
  tile_mma<false, true>(T + (int64_t)J * TS * ldt + (int64_t)k0 * TS, ldt,
                        T + (int64_t)L * TS * ldt + (int64_t)k0 * TS, ldt, (k1 - k0) * TS, smem,
                        smem + 2 * STAGE, acc, nullptr, dummy);
  store_c(part + predict_cov_part_off(tile, S, p), TS, acc);
}

// C tile (J, L) = K**_JL + sum_p part[tile][p], p ascending, in place in C [nsp][ldc]
// (which holds K** on entry), stored as tile (J, L) and transposed as tile (L, J). Only
// the lower tiles of K**, and of a diagonal tile only the entries r >= c, are read, and
// what is written besides is read by nobody: C comes out exactly symmetric whatever the
// upper half held. Grid: (ntiles, 8), a workgroup takes 16 rows of its tile; the
// transposed store goes through LDS so that 16 lanes write one 128-B row segment.
__global__ __launch_bounds__(256) void pred_cov_reduce_kernel(const double* __restrict__ part,
                                                              int S, int nct, double* C,
                                                              int64_t ldc) {
  __shared__ double sm[16][TS + 1];
  int J, L;
  tri_decode((int)blockIdx.x, nct, &J, &L);
  const int t = threadIdx.x, r0 = blockIdx.y * 16;
  const bool diag = J == L;
  const double* pt = part + predict_cov_part_off(blockIdx.x, S, 0);
  double* Cjl = C + (int64_t)J * TS * ldc + (int64_t)L * TS;
  {
    const int c = t & (TS - 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rl = (t >> 7) + 2 * i, r = r0 + rl;
      if (!diag || r >= c) {
        double s = 0.0;
        for (int p = 0; p < S; ++p) s += pt[(int64_t)p * TS * TS + r * TS + c];
        const double v = Cjl[(int64_t)r * ldc + c] + s;
        Cjl[(int64_t)r * ldc + c] = v;
        sm[rl][c] = v;
      }
    }
  }
  __syncthreads();
  double* Clj = C + (int64_t)L * TS * ldc + (int64_t)J * TS;
  const int rl = t & 15, r = r0 + rl;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = (t >> 4) + 16 * i;
    if (!diag || r > c) Clj[(int64_t)c * ldc + r] = sm[rl][c];
  }
}

}  // namespace gpmi
