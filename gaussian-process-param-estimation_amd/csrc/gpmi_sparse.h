// Kernels and constants of the sparse path shared by their definitions
// (gpmi_sparse.hip; the CSR assembly in gpmi_matern.hip) and the host side that
// launches them (gpmi_sparse_assemble.hip, gpmi_sparse_spmm.hip, gpmi_sparse_lanczos.hip,
// gpmi_sparse_cg.hip; the handle: gpmi_sp.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpmi_internal.h"

namespace gpmi {

// X-window SpMM (gpmi_sparse.hip)
constexpr int WIN_ROWS = 64;     // rows per block
constexpr int WIN_MAXM = 4096;   // most nonzeros of a windowed block
constexpr int WIN_MAXU = 1024;   // most window columns of a windowed block
constexpr int WIN_CS = 8;        // columns staged at a time (csr_spmm_win_kernel)
constexpr int WING_MAXS = 20;    // widths 1 .. WING_MAXS have a window kernel
// nonzeros in flight per thread and threads per row of csr_spmm_wing_kernel (measured:
// 8 in flight best at cfg 5, within 0.3 us of 4 at cfg 4; 8 threads per row in
// 512-thread blocks faster only at cfg 5 s = 11, 55 against 59 us, slower elsewhere)
constexpr int WING_U = 8, WING_TPR = 4;
constexpr int MS_NBLK = 128;     // row blocks of the multi-shift dot partials

// CSR assembly (gpmi_matern.hip)
__global__ void csr_count_kernel(const double*, int64_t, int, const double*, MaternParams, double,
                                 double, int*);
__global__ void csr_fill_kernel(const double*, int64_t, int, const double*, MaternParams, double,
                                double, const int64_t*, int*, double*);
__global__ void csr_cell_count_kernel(const double*, int64_t, int, const double*, MaternParams,
                                      double, double, const int*, const int*, const int*,
                                      const int*, int*);
__global__ void csr_cell_fill_kernel(const double*, int64_t, int, const double*, MaternParams,
                                     double, double, const int*, const int*, const int*,
                                     const int*, const int64_t*, int*, double*);
constexpr int CELL_CAP_HOST = 512;   // = CELL_CAP (gpmi_matern.hip)

// Cross assembly of new points against the training points (gpmi_matern.hip): the cell
// grid by value, the training points in original order, perm_dev / inv the locality
// permutation and its inverse (null: identity), columns in device order
struct CrossGrid {
  double pmin[3], wid[3];
  int gdim[3];   // 1 past d
};
__global__ void cross_count_kernel(const double*, int64_t, const double*, int64_t, int,
                                   const double*, MaternParams, double, double, int*);
__global__ void cross_fill_kernel(const double*, int64_t, const double*, int64_t, int,
                                  const double*, MaternParams, double, double, const int*,
                                  const int64_t*, int*, double*);
__global__ void cross_cell_count_kernel(const double*, int64_t, const double*, int,
                                        const double*, MaternParams, double, double, CrossGrid,
                                        const int*, const int*, int*);
__global__ void cross_cell_fill_kernel(const double*, int64_t, const double*, int,
                                       const double*, MaternParams, double, double, CrossGrid,
                                       const int*, const int*, const int*, const int64_t*, int*,
                                       double*);

// SpMM
__global__ void csr_spmm_kernel(const int64_t*, const int*, const double*, int64_t, const double*,
                                int64_t, double*, int64_t, int, int, double);
template <int U>
__global__ void csr_spmm_pair_kernel(const int64_t*, const int*, const double*, int64_t,
                                     const double*, double*, int, int, double);
__global__ void spmm_window_build_kernel(const int64_t*, const int*, int64_t, int*, int*,
                                         unsigned short*);
__global__ void csr_spmm_win_kernel(const int64_t*, const int*, const unsigned short*,
                                    const double*, int64_t, const int*, const int*, const double*,
                                    int64_t, double*, int64_t, int, double);
template <int S, int U, int TPR>
__global__ void csr_spmm_wing_kernel(const int64_t*, const int*, const unsigned short*,
                                     const double*, int64_t, const int*, const int*,
                                     const double*, double*, double, double*, int,
                                     unsigned long long*);
template <int CT>
__global__ void dense_mm_kernel(const double*, int64_t, int64_t, const double*, int, int, double*);
__global__ void dense_mm_reduce_kernel(const double*, int, int64_t, const double*, double, double*);
__global__ void csr_permute_kernel(const int64_t*, const int*, const double*, const int*,
                                   const int*, int64_t, const int64_t*, int*, double*);
__global__ void rows_gather_kernel(const double*, int, const int*, int64_t, int, double*);

// column-blocked vector kernels, the standard-form CG
__global__ void col_dot_partial_kernel(const double*, int64_t, const double*, int64_t, int,
                                       double*);
__global__ void col_dot_reduce_kernel(const double*, int, int, int, double*);
__global__ void col_gs_update_kernel(double*, const double*, int64_t, const double*, int, int64_t,
                                     int);
__global__ void col_axpby_kernel(const double*, double*, const double*, const double*, int64_t,
                                 int);
__global__ void cg_xr_kernel(const double*, const double*, double*, double*, const double*,
                             const double*, const int*, int64_t, int, int*);
__global__ void cg_p_kernel(const double*, double*, const double*, const double*, const int*, int*,
                            const double*, int, int*, int64_t, int);
__global__ void cg_init_kernel(const double*, double, int, double*, int*, int*, int*);

// the sparse prediction's products with the cross CSR
__global__ void cross_spmm_kernel(const int64_t*, const int*, const double*, int64_t,
                                  const double*, int, double*);
__global__ void cross_scatter_kernel(const int64_t*, const int*, const double*, int64_t, int,
                                     double*);
__global__ void cross_dot_kernel(const int64_t*, const int*, const double*, int64_t, int,
                                 const double*, double*);
__global__ void gram_partial_kernel(const double*, const double*, int64_t, int, double*);

// Lanczos
template <bool NT>
__global__ void lz_dots_kernel(const double*, int64_t, int, int, const double*, const double*,
                               int64_t, int, int, double*);
__global__ void lz_scalar_kernel(const double*, int, int, int, double*, double*, double*, double*,
                                 double*, int*, int*, double*, double*, int);
template <int NR, bool NT>
__global__ void lz_update_kernel(double*, int64_t, int, double*, const double*, const double*,
                                 const double*, const double*, int);
__global__ void rademacher_kernel(double*, int64_t, int, unsigned long long, int, double,
                                  const int*);
__global__ void lz0_dot64_kernel(const double*, const double*, int64_t, int, double*);
__global__ void lz0_alpha_kernel(const double*, const double*, int, int, int, int, double*, int*,
                                 double*, double*, double*);
__global__ void lz0_update_kernel(const double*, const double*, const double*, double*,
                                  const double*, int64_t, int, double*);
__global__ void lanczos_scalar_kernel(const double*, const double*, const double*, int, int, int,
                                      int*, double*, double*, double*, double*, double*,
                                      double*);

// multi-shift CG
void launch_ms_dots(const double* B, const double* R, int64_t n, int s, double* partial, int nblk,
                    hipStream_t st, int sa);
__global__ void ms_init_kernel(MsScal, MsShift, const double*, int, int, int, int, MsPin*);
__global__ void ms_cg2_update_kernel(const double*, double*, const double*, double*,
                                     MsScal, MsScal, MsShift, const double*, double*,
                                     const double*, int, int, int, double, int, int64_t, MsPin*);
__global__ void ms_cg2_reduce_kernel(const double*, int, int, const double*, int, int, double*);
__global__ void ms_cg2_close_kernel(MsScal, MsShift, const double*, int, int, int);
__global__ void ms_compact_kernel(MsCompactArgs);
__global__ void ms_dots2_kernel(const double*, const double*, int64_t, int, double*);

}  // namespace gpmi
