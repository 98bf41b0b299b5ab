// Leave-one-out terms from W = L^-T (gpmi_trinv.hip; S = K + eta I = L L^T, S^-1 = W W^T,
// W upper triangular, row-major [n_pad][ldw]) and Y = L^-1 [X | z] ([n_pad][16]): one
// streaming read of W's upper block triangle gives, for every row i,
//   d_i       = sum_k W_ik^2           = (S^-1)_ii
//   x_i[0:16] = sum_k W_ik Y_k[0:16]   = row i of S^-1 [X | z]
// from the same loaded values (gaussian_proc: _loo_from_terms turns them into the
// leave-one-out predictions).
//   loo_pass_kernel    one workgroup per (column chunk c, 64 rows of tile row j): the
//                      columns [max(c CW, 128 j), min((c + 1) CW, n_pad)) of those rows
//                      -> part[c][row][0..15 | 16]. Column tiles left of the diagonal tile
//                      are never read (after tr(S^-2) they hold tiles of S^-1); the
//                      diagonal tile is read whole (its lower half is zero).
//   loo_reduce_kernel  out[row] = sum_c part[c][row], c ascending from the row's first
//                      chunk (deterministic, no atomics)
// A wave owns 16 rows over the workgroup's column range. The thin product is
// v_mfma_f64_16x16x4f64 with A = W (16 rows x 4 columns, straight from the 16-byte global
// loads: lane l holds W[l & 15][2 (l >> 4) + {0, 1}] of an 8-column step) and B = Y from
// LDS; the squares are VALU FMAs on the same registers. 64 columns are in flight per wave
// (eight 16-byte loads per lane) while the previous 64 are consumed. The shape (16 rows
// per wave, 64-column steps, 256-column LDS stage, four workgroups per CU) and the chunk
// width are measured choices: DESIGN.md, leave-one-out.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpmi_internal.h"
#include "gpmi_device.h"

namespace gpmi {

namespace {

constexpr int LOO_STEP = 64;          // columns a wave loads ahead
constexpr int NJ = LOO_STEP / 8;      // 16-byte loads per lane in a step

// LOO_STEP columns of 16 rows: v[j] = W[row + (l & 15)][8 j + 2 (l >> 4) + {0, 1}]
__device__ __forceinline__ void loo_load(const double* __restrict__ p, d2 (&v)[NJ]) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) v[j] = *reinterpret_cast<const d2*>(p + 8 * j);
}

}  // namespace

// Grid: (nchunk, n_pad / 64) workgroups of 256. sY holds the sub-block's rows of Y in
// pairs, [k / 2][col][k & 1]: the B operands of the two MFMAs that consume one 16-byte
// load of W (columns k, k + 1) are then one 16-byte LDS read.
__global__ __launch_bounds__(256, 4) void loo_pass_kernel(const double* __restrict__ W,
                                                          int64_t ldw,
                                                          const double* __restrict__ Y,
                                                          int64_t n_pad, int cw,
                                                          double* __restrict__ part) {
  __shared__ double sY[LOO_STAGE * RLD];
  const int c = blockIdx.x;
  const int64_t wg0 = (int64_t)blockIdx.y * LOO_ROWS;   // first row of the workgroup
  const int64_t d0 = wg0 / TS * TS;                     // first column of its diagonal tile
  const int64_t c0 = (int64_t)c * cw;
  const int64_t kb = c0 > d0 ? c0 : d0;
  const int64_t ke = c0 + cw < n_pad ? c0 + cw : n_pad;
  if (kb >= ke) return;   // the chunk lies left of the diagonal tile (or past the matrix)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int64_t row0 = wg0 + w * 16;
  const double* Wl = W + (row0 + fr) * ldw + 2 * fk;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
  double sq = 0.0;
  for (int64_t s0 = kb; s0 < ke; s0 += LOO_STAGE) {
    const int cols = (int)(ke - s0 < LOO_STAGE ? ke - s0 : LOO_STAGE);   // a multiple of 128
    d2 cur[NJ], nxt[NJ];
    loo_load(Wl + s0, cur);
    __syncthreads();   // (the previous sub-block's reads of sY are done)
    for (int e = t; e < cols * 4; e += 256) {
      const int p = e >> 3, cp = e & 7;
      const d2 a = *reinterpret_cast<const d2*>(Y + (s0 + 2 * p) * RLD + 2 * cp);
      const d2 b = *reinterpret_cast<const d2*>(Y + (s0 + 2 * p + 1) * RLD + 2 * cp);
      *reinterpret_cast<d2*>(&sY[p * 32 + 4 * cp]) = d2{a.x, b.x};
      *reinterpret_cast<d2*>(&sY[p * 32 + 4 * cp + 2]) = d2{a.y, b.y};
    }
    __syncthreads();
    for (int k0 = 0; k0 < cols; k0 += LOO_STEP) {
      const bool more = k0 + LOO_STEP < cols;
      if (more) loo_load(Wl + s0 + k0 + LOO_STEP, nxt);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        // columns k0 + 8 j + 2 fk + {0, 1}: pair row k0 / 2 + 4 j + fk of sY
        const d2 y = *reinterpret_cast<const d2*>(&sY[(k0 / 2 + 4 * j + fk) * 32 + 2 * fr]);
        acc = mfma64(cur[j].x, y.x, acc);
        acc = mfma64(cur[j].y, y.y, acc);
        sq = fma(cur[j].x, cur[j].x, sq);
        sq = fma(cur[j].y, cur[j].y, sq);
      }
      if (more) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) cur[j] = nxt[j];
      }
    }
  }
  // acc[r] = x[row0 + fk + 4 r][fr]; sq = this lane's share of row row0 + fr, summed over
  // the four lanes fk in a fixed order
  double* out = part + ((int64_t)c * n_pad + row0) * LOO_LD;
  sq += __shfl_xor(sq, 16);
  sq += __shfl_xor(sq, 32);
#pragma unroll
  for (int r = 0; r < 4; ++r) out[(fk + 4 * r) * LOO_LD + fr] = acc[r];
  if (fk == 0) out[fr * LOO_LD + 16] = sq;
}

// out[row][e] = sum over the row's chunks c >= (128 (row / 128)) / cw of part[c][row][e],
// c ascending. Grid: ceil(n_pad * 17 / 256).
__global__ __launch_bounds__(256) void loo_reduce_kernel(const double* __restrict__ part,
                                                         int64_t n_pad, int cw, int nchunk,
                                                         double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t cnt = n_pad * LOO_LD;
  if (e >= cnt) return;
  const int64_t row = e / LOO_LD;
  double s = 0.0;
  for (int c = (int)(row / TS * TS / cw); c < nchunk; ++c) s += part[(int64_t)c * cnt + e];
  out[e] = s;
}

}  // namespace gpmi
