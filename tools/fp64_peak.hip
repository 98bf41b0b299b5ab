// Dev microbenchmark: the achievable fp64 MFMA rate on this MI355X, to price the syrk
// roofline against a measured ceiling next to the 78.6 TFLOP/s spec figure. Two kernels,
// both the dense kernels' 4 x 4 block of v_mfma_f64_16x16x4f64 accumulators per wave,
// every CU busy, at 1 / 2 / 4 workgroups per CU (two are resident: 256 registers):
//   peak_kernel    : the MFMAs alone. Operands in registers; the timed loop holds no
//                    other instruction (check the -S listing: no v_accvgpr_*, no v_mov).
//   lds_fed_kernel : the same MFMAs fed by tile_mma's fragment reads (slab_off, the
//                    swizzled [row][16] slab) from an LDS slab pair that stays resident:
//                    no global traffic and no barrier. It prices the fragment scheme
//                    alone, which bounds what the dense k-loop can reach.
// Build:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/fp64_peak.hip -o tools/fp64_peak
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "../gaussian-process-param-estimation_amd/csrc/gpmi_device.h"

using gpmi::BK;
using gpmi::d4;
using gpmi::STAGE;

// 128 MFMAs per trip (the 4 x 4 block eight times)
__global__ __launch_bounds__(256, 2) void peak_kernel(double* out, int trips, double seed) {
  d4 acc[4][4];
  double a[4], b[4];
  for (int i = 0; i < 4; ++i) {
    a[i] = seed + (threadIdx.x + i) * 1e-3;
    b[i] = seed - (threadIdx.x + i) * 1e-3;
    for (int j = 0; j < 4; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  }
  for (int it = 0; it < trips; ++it) {
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = gpmi::mfma64(a[i], b[j], acc[i][j]);
  }
  double s = 0.0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) s += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

// 128 MFMAs per trip: two stages of BK = 16 (4 k-steps of 16 MFMAs), the fragments of
// every k-step read from the resident slab pair as tile_mma reads them
__global__ __launch_bounds__(256, 2) void lds_fed_kernel(double* out, int trips, double seed) {
  __shared__ double smem[2 * STAGE];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1, fr = lane & 15, fk = lane >> 4;
  for (int e = t; e < 2 * STAGE; e += 256) smem[e] = seed + (e & 1023) * 1e-6;
  __syncthreads();
  const double* sA = smem;
  const double* sB = smem + STAGE;
  d4 acc[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < trips; ++it) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      // (the slab never changes: without this the reads leave the loop)
      asm volatile("" ::: "memory");
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk) {
        double a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = sA[gpmi::slab_off(wr * 64 + i * 16 + fr, kk * 4 + fk)];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = sB[gpmi::slab_off(wc * 64 + j * 16 + fr, kk * 4 + fk)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = gpmi::mfma64(a[i], b[j], acc[i][j]);
      }
    }
  }
  double s = 0.0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) s += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

typedef void (*kernel_t)(double*, int, double);

#define CHECK(call)                                                          \
  do {                                                                       \
    hipError_t e_ = (call);                                                  \
    if (e_ != hipSuccess) {                                                  \
      fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));             \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

int main() {
  int ncu = 0;
  CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
  const kernel_t kernels[] = {peak_kernel, lds_fed_kernel};
  const char* names[] = {"fp64_mfma_16x16x4_peak", "fp64_mfma_16x16x4_lds_fed"};
  const int wgs_per_cu[] = {1, 2, 4};
  for (int k = 0; k < 2; ++k) {
    for (int wps : wgs_per_cu) {
      const int nblk = ncu * wps;   // 256 threads = 4 waves = one per SIMD
      double* out;
      CHECK(hipMalloc(&out, (size_t)nblk * 256 * sizeof(double)));
      const int trips = 500;        // x 128 MFMAs per wave
      hipEvent_t e0, e1;
      CHECK(hipEventCreate(&e0));
      CHECK(hipEventCreate(&e1));
      kernels[k]<<<nblk, 256>>>(out, 2, 1.0);
      CHECK(hipDeviceSynchronize());
      CHECK(hipEventRecord(e0));
      const int reps = 5;
      for (int r = 0; r < reps; ++r) kernels[k]<<<nblk, 256>>>(out, trips, 1.0 + r);
      CHECK(hipEventRecord(e1));
      CHECK(hipEventSynchronize(e1));
      float ms = 0.f;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      const double flops = (double)reps * nblk * 4 * (double)trips * 128 * 2048.0;
      printf("{\"kernel\": \"%s\", \"cus\": %d, \"waves_per_simd\": %d, "
             "\"tflops\": %.2f, \"ms\": %.3f}\n", names[k], ncu, wps,
             flops / (ms * 1e-3) / 1e12, ms);
      CHECK(hipEventDestroy(e0));
      CHECK(hipEventDestroy(e1));
      CHECK(hipFree(out));
    }
  }
  return 0;
}
