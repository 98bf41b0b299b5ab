// Device-side helpers shared by the gpmi HIP translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpmi_internal.h"

namespace gpmi {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int TS = GPMI_TS;      // 128
constexpr int BK = 16;           // k-depth of one LDS stage
constexpr int STAGE = TS * BK;   // doubles per staged operand buffer (128 rows x 16, 16 KB)

// Staged slabs are stored unpadded, [row][16 doubles], with the 16-byte chunk c
// of row r placed at chunk position c ^ ((r >> 1) & 7); the staging
// ds_write_b128 of a row stays one contiguous 128-byte line. The compiler merges
// fragment reads 16 rows apart into ds_read2st64_b64, whose 16-lane groups see
// this layout 2-way conflicted; measured faster than the conflict-free
// k ^ (r & 15) layout (with or without the merge) all the same.
__device__ __forceinline__ int slab_off(int row, int k) {
  return row * BK + 2 * ((k >> 1) ^ ((row >> 1) & 7)) + (k & 1);
}
constexpr int RLD = GPMI_RHS_LD; // 16

// Hand-off words between co-resident workgroups: agent-scope relaxed atomic
// stores / loads (write-through to L2, loads that bypass the non-coherent caches).
__device__ __forceinline__ void st_sc1(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p),
                     (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(
      reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
      __HIP_MEMORY_SCOPE_AGENT));
}

__device__ __forceinline__ d4 mfma64(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// c - a b: for f64 MFMA the BLGP field is the NEG modifier (bit 0 negates A),
// so the subtraction costs no VALU op.
__device__ __forceinline__ d4 mfma64_neg(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 1);
}


// 128 x 16 slab of rows base[row * ld + p .. p + 15]: each wave-instruction
// reads 32 full 128-B row segments (16 B / lane).
__device__ __forceinline__ void gload_slab(const double* __restrict__ base, int64_t ld,
                                           int p, d2 (&r)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = i * 256 + t;
    const int row = idx >> 3, c2 = idx & 7;
    r[i] = *reinterpret_cast<const d2*>(base + (int64_t)row * ld + p + 2 * c2);
  }
}

__device__ __forceinline__ void sstore_slab(double* s, const d2 (&r)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = i * 256 + t;
    const int row = idx >> 3, c2 = idx & 7;
    *reinterpret_cast<d2*>(s + row * BK + 2 * (c2 ^ ((row >> 1) & 7))) = r[i];
  }
}


// gload_slab through a buffer descriptor: the address split as the hardware takes it, a
// wave-uniform descriptor on the operand's base (base uniform), a scalar byte offset per
// load (row block i, k offset p: SALU) and one 32-bit byte offset per thread,
// slab_voff(ld). No 64-bit VALU add and no VGPR pair of address per load. Every offset
// stays below 2^32 for ld < 2^22 (128 rows of 8 ld bytes).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slab_rsrc(const double* base) {
  // raw buffer (stride 0), no range limit (the callers' tiles lie inside their matrices)
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(base), 0, 0xffffffff, 0x00020000);
}
__device__ __forceinline__ uint32_t slab_voff(int64_t ld) {
  const int t = threadIdx.x;
  return (uint32_t)(((t >> 3) * ld + 2 * (t & 7)) * 8);
}
__device__ __forceinline__ void gload_slab_u(__amdgpu_buffer_rsrc_t rs, int64_t ld, int p,
                                             uint32_t voff, d2 (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t soff = (uint32_t)(((int64_t)(i * 32) * ld + p) * 8);
    r[i] = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
  }
}

// The interleave of a stage of the KLOOP_EARLY form, pinned by sched_group_barrier
// (masks: 0x8 MFMA, 0x100 DS read, 0x200 DS write). The scheduler left to itself issues
// a k-step's fragment reads after its last MFMA, straight in front of the barrier's
// lgkmcnt(0). N MFMAs, each followed by PER LDS instructions of the kind MASK:
template <int MASK, int N, int PER>
__device__ __forceinline__ void pin_behind_mfma() {
#pragma unroll
  for (int q = 0; q < N; ++q) {
    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
    __builtin_amdgcn_sched_group_barrier(MASK, PER, 0);
  }
}
// one k-step (16 MFMAs): LEAD MFMAs, the four fragment reads for the next k-step one
// behind each of the next four MFMAs, then the rest.
template <int LEAD>
__device__ __forceinline__ void pin_kstep() {
  if (LEAD > 0) __builtin_amdgcn_sched_group_barrier(0x8, LEAD, 0);
  pin_behind_mfma<0x100, 4, 1>();
  __builtin_amdgcn_sched_group_barrier(0x8, 12 - LEAD, 0);
}

// One stage (slab s, 16 k) of the KLOOP_EARLY form, the slab in buffer CUR. On entry
// ra / rb hold slab s + 1, a / b the fragments of the stage's first k-step, and every
// wave has passed the barrier E that ended stage s - 1. In program order:
//   slab s + 1 goes from ra / rb to the other buffer behind the first four MFMAs, and the
//   global loads of slab s + 2 follow into the same registers (has2; a uniform branch, the
//   only one of the stage): a prefetch distance of two with one register set;
//   the rest of k-step 0, k-step 1; barrier M; k-steps 2, 3, the last one reading the
//   first fragments of stage s + 1 from the other buffer; barrier E.
// Which barrier orders what:
//   E (of stage s - 1) orders that stage's fragment reads of the other buffer, the
//     pre-read of this stage's first fragments included, before the writes here (WAR);
//   M orders the writes of slab s + 1 before its first fragment reads, the pre-read of
//     k-step 3 (RAW). The writes were issued 28 MFMAs earlier, so the lgkmcnt(0) in front
//     of M finds them done, and so does the one in front of E the pre-read (12 MFMAs);
//   E (of this stage) also leaves the buffers free for the caller after the last stage.
// No wave waits behind E for an LDS read: a and b are complete there. The last stage
// runs the same code: it writes ra / rb (slab s, again) to the other buffer and reads
// fragments from it that nothing uses.
template <bool WITH_RHS, bool NEG, int CUR>
__device__ __forceinline__ void tile_mma_early_stage(
    __amdgpu_buffer_rsrc_t R1, int64_t ld1, __amdgpu_buffer_rsrc_t R2, int64_t ld2,
    uint32_t vo1, uint32_t vo2, int s, bool has2, double* sA, double* sB, d4 (&acc)[4][4],
    const double* sU, d4 (&racc)[2], d2 (&ra)[4], d2 (&rb)[4], double (&a)[4],
    double (&b)[4]) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int fr = lane & 15, fk = lane >> 4;
  const double* cA = sA + CUR * STAGE;
  const double* cB = sB + CUR * STAGE;
  double* nA = sA + (CUR ^ 1) * STAGE;
  double* nB = sB + (CUR ^ 1) * STAGE;
  sstore_slab(nA, ra);
  sstore_slab(nB, rb);
#pragma unroll
  for (int kk = 0; kk < BK / 4; ++kk) {
    double an[4], bn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (kk == 0 && i == 1) {
        pin_behind_mfma<0x200, 4, 2>();
        if (has2) {
          gload_slab_u(R1, ld1, (s + 2) * BK, vo1, ra);
          gload_slab_u(R2, ld2, (s + 2) * BK, vo2, rb);
        }
      }
      if ((kk == 0 && i == 1) || (kk > 0 && i == 0)) {
        // the next k-step's fragments (the next stage's first, after k-step 3)
        const double* fA = kk + 1 < BK / 4 ? cA : nA;
        const double* fB = kk + 1 < BK / 4 ? cB : nB;
        const int kn = ((kk + 1) * 4) % BK + fk;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) an[ii] = fA[slab_off(wr * 64 + ii * 16 + fr, kn)];
#pragma unroll
        for (int j = 0; j < 4; ++j) bn[j] = fB[slab_off(wc * 64 + j * 16 + fr, kn)];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = NEG ? mfma64_neg(a[i], b[j], acc[i][j]) : mfma64(a[i], b[j], acc[i][j]);
    }
    if (WITH_RHS) {
      const double u = sU[(s * BK + kk * 4 + fk) * RLD + fr];
      const double a0 = wc ? a[2] : a[0];
      const double a1 = wc ? a[3] : a[1];
      racc[0] = mfma64(a0, u, racc[0]);
      racc[1] = mfma64(a1, u, racc[1]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = an[i];
      b[i] = bn[i];
    }
    if (kk == 1) {
      // k-step 0's remaining 12 MFMAs (its reads behind the 9th to 12th), then k-step 1
      __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
      pin_behind_mfma<0x100, 4, 1>();
      __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
      pin_kstep<0>();
      __builtin_amdgcn_sched_barrier(0);   // (every MFMA of k-steps 0, 1 ahead of M)
      __syncthreads();                     // M
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  pin_kstep<8>();
  pin_kstep<0>();
  __builtin_amdgcn_sched_barrier(0);   // (every MFMA of the stage ahead of E)
  __syncthreads();                     // E
  __builtin_amdgcn_sched_barrier(0);   // (no MFMA of the next stage moves up past E)
}

// kdim: a positive multiple of 2 BK (the stages run in pairs, so that the buffer parity,
// and with it every LDS offset, is static).
template <bool WITH_RHS, bool NEG>
__device__ __forceinline__ void tile_mma_early(const double* __restrict__ P1, int64_t ld1,
                                               const double* __restrict__ P2, int64_t ld2,
                                               int kdim, double* sA, double* sB,
                                               d4 (&acc)[4][4], const double* sU,
                                               d4 (&racc)[2]) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int fr = lane & 15, fk = lane >> 4;
  const int nsteps = kdim / BK;
  const uint32_t vo1 = slab_voff(ld1), vo2 = slab_voff(ld2);
  const __amdgpu_buffer_rsrc_t R1 = slab_rsrc(P1), R2 = slab_rsrc(P2);
  d2 ra[4], rb[4];
  gload_slab_u(R1, ld1, 0, vo1, ra);
  gload_slab_u(R2, ld2, 0, vo2, rb);
  sstore_slab(sA, ra);
  sstore_slab(sB, rb);
  // Drain every global load issued before the loop (the caller's accumulator preload)
  // here, once, as the KLOOP_LATE form does, and before slab 1 is requested.
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) expcnt(7) lgkmcnt(15)
  gload_slab_u(R1, ld1, BK, vo1, ra);
  gload_slab_u(R2, ld2, BK, vo2, rb);
  __syncthreads();   // slab 0 written -> its fragment reads
  double a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = sA[slab_off(wr * 64 + i * 16 + fr, fk)];
#pragma unroll
  for (int j = 0; j < 4; ++j) b[j] = sB[slab_off(wc * 64 + j * 16 + fr, fk)];
  __builtin_amdgcn_sched_barrier(0);
  for (int s = 0; s < nsteps; s += 2) {
    tile_mma_early_stage<WITH_RHS, NEG, 0>(R1, ld1, R2, ld2, vo1, vo2, s, s + 2 < nsteps, sA, sB,
                                           acc, sU, racc, ra, rb, a, b);
    tile_mma_early_stage<WITH_RHS, NEG, 1>(R1, ld1, R2, ld2, vo1, vo2, s + 1, s + 3 < nsteps, sA,
                                           sB, acc, sU, racc, ra, rb, a, b);
  }
}

// acc (wave tile 64 x 64 at (wr, wc)) += P1[0:128, 0:kdim] * P2[0:128, 0:kdim]^T.
// f64 MFMA 16x16x4 operand maps: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15].
// WITH_RHS additionally accumulates racc (rows wr*64 + wc*32 + [0,32), 16 cols)
// += P1 * U with U[kdim][16] staged in LDS. KL: the k-loop's pipeline form (gpmi_internal.h;
// KLOOP_EARLY needs wave-uniform P1 / P2 and kdim a multiple of 32). The same results either way.
template <bool WITH_RHS, bool NEG = false, int KL = KLOOP_LATE>
__device__ __forceinline__ void tile_mma(const double* __restrict__ P1, int64_t ld1,
                                         const double* __restrict__ P2, int64_t ld2,
                                         int kdim, double* sA, double* sB,
                                         d4 (&acc)[4][4], const double* sU,
                                         d4 (&racc)[2]) {
  if constexpr (KL == KLOOP_EARLY) {
    tile_mma_early<WITH_RHS, NEG>(P1, ld1, P2, ld2, kdim, sA, sB, acc, sU, racc);
    return;
  }
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int fr = lane & 15, fk = lane >> 4;
  d2 ra[4], rb[4];
  gload_slab(P1, ld1, 0, ra);
  gload_slab(P2, ld2, 0, rb);
  sstore_slab(sA, ra);
  sstore_slab(sB, rb);
  __syncthreads();
  // Drain every global load issued before the loop (the caller's accumulator
  // preload) here, once. Otherwise the waitcnt pass places vmcnt(3..0) waits
  // on the first accumulator uses INSIDE the loop, which also drain the
  // next-stage prefetch every iteration (vmcnt counts in order).
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) expcnt(7) lgkmcnt(15)
  const int nsteps = kdim / BK;
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
        for (int j = 0; j < 4; ++j)
          acc[i][j] = NEG ? mfma64_neg(a[i], b[j], acc[i][j]) : mfma64(a[i], b[j], acc[i][j]);
      if (WITH_RHS) {
        const double u = sU[(s * BK + kk * 4 + fk) * RLD + fr];
        const double a0 = wc ? a[2] : a[0];
        const double a1 = wc ? a[3] : a[1];
        racc[0] = mfma64(a0, u, racc[0]);
        racc[1] = mfma64(a1, u, racc[1]);
      }
    }
    if (s + 1 < nsteps) {
      sstore_slab(sA + (cur ^ 1) * STAGE, ra);
      sstore_slab(sB + (cur ^ 1) * STAGE, rb);
    }
    __syncthreads();
  }
}

// Output column block (16 wide, 0..7) that wave column wc computes as its j-th in
// tile_trsm: {0, 3, 4, 7} and {1, 2, 5, 6}. Column block cb needs the k-slabs s <= cb,
// so both wave columns run 18 of the 32 (slab, column block) steps.
__device__ __forceinline__ int trsm_cb(int wc, int j) { return 2 * j + ((j ^ wc) & 1); }

// acc += P1[0:128, 0:128] * Linv[0:128, 0:128]^T for a lower-triangular Linv (row-major,
// ld 128), the wave's 64 rows (wr) x column blocks trsm_cb(wc, 0..3). Same slab pipeline
// and, per accumulator, the same MFMA sequence as tile_mma over kdim = 128, except that
// the steps whose Linv operand is identically zero (k-slab s > column block) are left
// out: they add a * (+0) to a finite accumulator that started at +0. The racc update
// (WITH_RHS, as in tile_mma) runs over every k.
template <bool WITH_RHS>
__device__ __forceinline__ void tile_trsm(const double* P1, int64_t ld1, const double* Linv,
                                          double* sA, double* sB, d4 (&acc)[4][4],
                                          const double* sU, d4 (&racc)[2]) {
  const int t = threadIdx.x, lane = t & 63;
  // the wave index as a scalar: the skips below are scalar branches
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int fr = lane & 15, fk = lane >> 4;
  d2 ra[4], rb[4];
  gload_slab(P1, ld1, 0, ra);
  gload_slab(Linv, TS, 0, rb);
  sstore_slab(sA, ra);
  sstore_slab(sB, rb);
  __syncthreads();
  constexpr int nsteps = TS / BK;
#pragma unroll
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    const double* cA = sA + cur * STAGE;
    const double* cB = sB + cur * STAGE;
    if (s + 1 < nsteps) {
      gload_slab(P1, ld1, (s + 1) * BK, ra);
      gload_slab(Linv, TS, (s + 1) * BK, rb);
    }
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      double a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = cA[slab_off(wr * 64 + i * 16 + fr, kk * 4 + fk)];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // s <= 2 j: both wave columns; s == 2 j + 1: the one whose block is 2 j + 1
        if (s <= 2 * j || (s == 2 * j + 1 && ((j ^ wc) & 1))) {
          const double bj = cB[slab_off(trsm_cb(wc, j) * 16 + fr, kk * 4 + fk)];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i][j] = mfma64(a[i], bj, acc[i][j]);
        }
      }
      if (WITH_RHS) {
        const double u = sU[(s * BK + kk * 4 + fk) * RLD + fr];
        const double a0 = wc ? a[2] : a[0];
        const double a1 = wc ? a[3] : a[1];
        racc[0] = mfma64(a0, u, racc[0]);
        racc[1] = mfma64(a1, u, racc[1]);
      }
    }
    if (s + 1 < nsteps) {
      sstore_slab(sA + (cur ^ 1) * STAGE, ra);
      sstore_slab(sB + (cur ^ 1) * STAGE, rb);
    }
    __syncthreads();
  }
}

// Bijective XCD-aware remap (consecutive logical tiles -> one XCD's L2).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// Lower-triangular tile enumeration of a band of w tile columns over t tile
// rows (row-major): rows i < w hold a triangle, rows i >= w hold w tiles.
__device__ __forceinline__ void tri_decode(int q, int w, int* pi, int* pj) {
  const int tri = w * (w + 1) / 2;
  int i, j;
  if (q < tri) {
    i = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= q) ++i;
    while (i * (i + 1) / 2 > q) --i;
    j = q - i * (i + 1) / 2;
  } else {
    const int r = q - tri;
    i = w + r / w;
    j = r % w;
  }
  *pi = i;
  *pj = j;
}

}  // namespace gpmi
