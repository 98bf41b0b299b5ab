/*
 * gpmi — MI355X-native (gfx950) Gaussian-process log-likelihood evaluator.
 * C ABI of libgpmi.so: plain pointers and sizes, int status codes, no C++
 * exceptions and no framework types across the boundary.
 *
 * Status: 0 = OK; > 0 = LAPACK-style info (1-based index of the first
 * non-positive pivot of K + eta I, i.e. "not positive definite");
 * < 0 = error (message via gpmi_last_error).
 *
 * The reference (ameli/gaussian-process-param-estimation v0.0.1) has no FFI on
 * this path: its hot path is Python calling Cython/scipy/imate. Each entry point
 * below replaces the reference interface cited next to it; the Python package
 * gaussian_proc (gaussian-process-param-estimation_amd/gaussian_proc) binds them
 * with ctypes.
 *
 * Layouts: host matrices are row-major (C order) fp64. Device state lives in an
 * opaque gpmi_op handle (one per GPU per operator); calls on one handle must be
 * serialised by the caller.
 */
#ifndef GPMI_H_
#define GPMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpmi_op gpmi_op;
typedef struct gpmi_sp gpmi_sp;   /* sparse operator (below) */

#define GPMI_MAX_RHS 16   /* columns of the resident RHS block (m + 1 <= 16) */

/* Library version (major*10000 + minor*100 + patch). */
int gpmi_version(void);

/* Copy the calling thread's last error message into buf (always NUL-terminated). */
int gpmi_last_error(char* buf, size_t len);

/* Number of visible HIP devices. */
int gpmi_device_count(int* count);

/* Dense Matérn correlation matrix, host in / host out.
 * Replaces generate_correlation(points, correlation_scale, nu, sparse=False)
 *   gaussian_proc/generate_correlation/generate_correlation.py:32-222
 *   -> _generate_dense_correlation.pyx:98-162 -> _kernels.pyx:17-136.
 * points: [n][d] (d <= 8); scale: [d] (already broadcast); K_out: [n][ldk]. */
int gpmi_matern_dense(int device, const double* points, int64_t n, int d,
                      const double* scale, double nu, double* K_out, int64_t ldk);

/* Device ms of the calling thread's last dense Matérn assembly kernel
 * (gpmi_matern_dense / gpmi_op_assemble_matern; HIP events around the launch):
 * the lower-triangular tiles evaluated once and stored mirrored, 8 n_pad^2
 * bytes written. */
int gpmi_last_assembly_ms(double* ms);

/* Create the device-resident K + eta I operator for an n x n correlation matrix,
 * with workspace for max_batch concurrent eta values.
 * Replaces MixedCorrelation.__init__  mixed_correlation.py:34-79. */
int gpmi_op_create(int device, int64_t n, int max_batch, gpmi_op** out);
int gpmi_op_destroy(gpmi_op* op);
/* n and the padded size (multiple of 128) used on the device. */
int gpmi_op_size(const gpmi_op* op, int64_t* n, int64_t* n_pad);

/* Fill K from a host matrix [n][ldk] (symmetric; the lower triangle is used). */
int gpmi_op_load_matrix(gpmi_op* op, const double* K_host, int64_t ldk);
/* Fill K from a sparse operator on the same device (device-side scatter of its
 * CSR, original point order): the exact ('cholesky' / 'eigenvalue') methods on a
 * sparse K. Replaces imate's sparse Cholesky (CHOLMOD) call at
 * mixed_correlation.py:250-261 and the eigh of a sparse K (:76-79, which raises
 * in the reference) with the dense device paths; needs 8 n_pad^2 bytes per copy. */
int gpmi_op_load_sparse(gpmi_op* op, const gpmi_sp* sp);
/* Assemble K on the device from points (no host round trip):
 * generate_correlation(points, scale, nu) fused into the operator. */
int gpmi_op_assemble_matern(gpmi_op* op, const double* points, int d,
                            const double* scale, double nu);
/* Copy K back to the host ([n][ldk]). */
int gpmi_op_get_matrix(gpmi_op* op, double* K_out, int64_t ldk);
/* Read-backs of the dense path's intermediates (tests, diagnostics). Each copies
 * on the operator's stream and synchronises; none launches a kernel or changes a
 * cache. < 0: null handle or output, ld < n, or the state named below is absent
 * (nothing is written then).
 * The n x n lower-triangular factor L of K + eta_slot I in batch slot `slot` of the
 * last factorization ([n][ldl]; the strict upper triangle is written as zeros).
 * Slot 0 is the cached factor (gpmi_op_logdet, _solve, _traceinv, ... or member 0 of
 * gpmi_op_loglik_batch); slots >= 1 hold the other members of a gpmi_op_loglik_batch
 * until the next factorization. Refused when K was loaded or assembled since, when
 * slot is outside the last batch, or when that member's info is non-zero. */
int gpmi_op_get_factor(gpmi_op* op, int slot, double* L_out, int64_t ldl);
/* W = L^-T of the cached factor ([n][ldw], upper triangular; the lower block
 * triangle is written as zeros), after gpmi_op_traceinv (or gpmi_op_loo_terms,
 * gpmi_op_scale_grad_terms) on the current factorization. */
int gpmi_op_get_trinv(gpmi_op* op, double* W_out, int64_t ldw);
/* (K + eta I)^-1 = W W^T of the cached factor, full and exactly symmetric
 * ([n][lda]: the lower tiles the device holds, mirrored), after
 * gpmi_op_traceinv(.., 2) (or gpmi_op_scale_grad_terms) on the current
 * factorization. */
int gpmi_op_get_inverse(gpmi_op* op, double* Ainv_out, int64_t lda);

/* Upload the resident RHS block R = [X | z] ([n][ld], nrhs <= 16 columns). */
int gpmi_op_set_rhs(gpmi_op* op, const double* rhs, int64_t ld, int nrhs);

/* Batched likelihood terms for neta <= max_batch values of eta, one dense
 * Cholesky per eta (K + eta I = L L^T) on fp64 MFMA:
 *   logdet[e]            = log det(K + eta_e I)
 *   gram[e][nrhs][nrhs]  = (L^-1 R)^T (L^-1 R) = R^T (K + eta_e I)^-1 R
 *   info[e]              = 0, or 1-based first non-positive pivot.
 * Replaces the logdet + 2 x solve of DirectLikelihood.log_likelihood
 * (_direct_likelihood.py:59,62,332 -> mixed_correlation.py:221-299). */
int gpmi_op_loglik_batch(gpmi_op* op, const double* etas, int neta,
                         double* logdet, double* gram, int* info);

/* logdet(K + eta I) (mixed_correlation.py:221-274, exact). Caches the factor. */
int gpmi_op_logdet(gpmi_op* op, double eta, double* logdet);

/* Solve (K + eta I) X = RHS for an [n][ld] host RHS with nrhs columns
 * (any count; processed in blocks of 16). Reuses the cached factor for eta.
 * Replaces MixedCorrelation.solve mixed_correlation.py:280-299
 *   -> linear_solver _linear_solver.py:24-73 (scipy.linalg.solve, assume_a='pos'). */
int gpmi_op_solve(gpmi_op* op, double eta, const double* rhs, int64_t ld, int nrhs,
                  double* sol, int64_t ldsol);

/* y = K x for an [n][ld] host block with ncol columns.
 * Building block of MixedCorrelation.dot mixed_correlation.py:305-335. */
int gpmi_op_matvec(gpmi_op* op, const double* x, int64_t ld, int ncol, double* y,
                   int64_t ldy);

/* trace(K) and trace(K^2) = ||K||_F^2 (K symmetric).
 * Building blocks of MixedCorrelation.trace mixed_correlation.py:96-149. */
int gpmi_op_trace(gpmi_op* op, double* trace_k, double* trace_k2);

/* Exact tr((K + eta I)^-exponent), exponent 1 or 2, from the (cached) Cholesky
 * factor: tr(A^-1) = ||L^-1||_F^2 and tr(A^-2) = ||L^-T L^-1||_F^2, with L^-1
 * built by a blocked triangular solve on the device (n_pad^2 extra doubles,
 * allocated on first use). Results are cached per factorization.
 * Replaces MixedCorrelation.traceinv mixed_correlation.py:155-215 for
 * imate_method 'eigenvalue' / 'cholesky' (imate.traceinv, exact). */
int gpmi_op_traceinv(gpmi_op* op, double eta, int exponent, double* value);

/* Kernel-level timing of the last gpmi_op_loglik_batch when enabled:
 * dominant kernel (trailing-update SYRK) total device ms, launches and
 * algorithmic flops; whole-call device ms. HIP events on the op's stream. */
int gpmi_op_set_timing(gpmi_op* op, int enable);
int gpmi_op_last_timing(gpmi_op* op, double* syrk_ms, int* syrk_launches,
                        double* syrk_flops, double* total_ms, double* syrk_busy_ms);

/* Outer panel width in 128-column tiles (trailing update depth = 128*S, 1..32,
 * default 16); each outer panel is factorized recursively (halves). */
int gpmi_op_set_outer(gpmi_op* op, int s);

/* ------------------------------------------------------------- prediction --
 * The reference stops at training (its GaussianProcess has no predict); these
 * entry points serve gaussian_proc.GaussianProcess.predict of this build. */

/* Matérn cross-correlation of two point sets, host in / host out: the
 * counterpart of gpmi_matern_dense. points: [n][d], test_points: [nstar][d],
 * C_out[j][i] = matern(test_j, points_i), [nstar][ldc]. A test point equal to a
 * training point gives bit for bit the entry gpmi_matern_dense produces. */
int gpmi_matern_cross(int device, const double* points, int64_t n,
                      const double* test_points, int64_t nstar, int d,
                      const double* scale, double nu, double* C_out, int64_t ldc);

/* Prediction terms at nstar new points from the cached factor of
 * K + eta I = L L^T (factorized if absent) and the resident RHS block R of
 * gpmi_op_set_rhs. With k*_j the correlations of test point j with the n training
 * points, v_j = L^-1 k*_j and Y = L^-1 R:
 *   c_out[nstar][nrhs]    c_j = Y^T v_j = R^T (K + eta I)^-1 k*_j
 *   q_out[nstar]          q_j = v_j^T v_j = k*_j^T (K + eta I)^-1 k*_j
 *   gram_out[nrhs][nrhs]  Y^T Y = R^T (K + eta I)^-1 R
 * (any may be NULL). k* is assembled on the device from points [n][d] (the points
 * K was assembled from), scale [d], nu and test_points [nstar][d]; or, when
 * kstar != NULL, uploaded from the host block kstar[nstar][ldks] (a K that did not
 * come from this library's Matérn; points, scale, test_points may then be NULL).
 * A wide forward substitution on fp64 MFMA in chunks of test columns; the solved
 * block never leaves the device. The environment variable GPMI_PREDICT_CHUNK
 * (columns, a multiple of 128) overrides the chunk width.
 * > 0: first non-positive pivot; < 0: null handle, no resident RHS, d outside
 * 1..8 (device assembly), nstar < 1. */
int gpmi_op_predict_terms(gpmi_op* op, double eta, const double* points, int d,
                          const double* scale, double nu, const double* test_points,
                          int64_t nstar, const double* kstar, int64_t ldks,
                          double* c_out, double* q_out, double* gram_out);

/* HIP-event timing of the last gpmi_op_predict_terms when gpmi_op_set_timing is
 * on: the whole call, the trailing products' total device ms and their flops. */
int gpmi_op_predict_ms(gpmi_op* op, double* total_ms, double* trailing_ms,
                       double* trailing_flops);

/* gpmi_op_predict_terms plus the joint covariance block of the nstar new points,
 *   cov_out[nstar][ldcov]  C0 = K** - K* (K + eta I)^-1 K*^T = K** - V V^T,
 * K** the correlations of the new points with each other and V = L^-1 K*^T, which
 * this call keeps on the device for all nstar columns (the forward substitution
 * still runs in chunks, on row ranges of the one block). C0 is a lower-tile SYRK
 * on fp64 MFMA whose depth n_pad is split into S pieces, summed in ascending order
 * without atomics: for a given S the result does not depend on the chunk width,
 * and it is exactly symmetric. S is chosen from the tile count and the device's
 * compute units; the environment variable GPMI_PREDICT_COV_SPLIT overrides it
 * (read per call, clipped to n_pad / 128). K** is assembled on the device with k*,
 * or, when kstar != NULL, uploaded from kss[nstar][ldkss] (only its lower triangle
 * is read). c_out, q_out, gram_out are bit for bit those of gpmi_op_predict_terms
 * and may be NULL; cov_out may not.
 * > 0: first non-positive pivot; < 0: as gpmi_op_predict_terms, and ldcov < nstar,
 * kstar without kss, ldkss < nstar, or a call whose working block, K** and
 * partial products together exceed 8 GiB (nothing is allocated then). */
int gpmi_op_predict_cov(gpmi_op* op, double eta, const double* points, int d,
                        const double* scale, double nu, const double* test_points,
                        int64_t nstar, const double* kstar, int64_t ldks,
                        const double* kss, int64_t ldkss, double* c_out, double* q_out,
                        double* gram_out, double* cov_out, int64_t ldcov);

/* HIP-event timing of the partial-product launch of the last gpmi_op_predict_cov
 * when gpmi_op_set_timing is on (device ms and flops; 0 otherwise), and the number
 * of depth pieces S that call used. */
int gpmi_op_predict_cov_ms(gpmi_op* op, double* product_ms, double* product_flops);
int gpmi_op_predict_cov_split(gpmi_op* op, int* split);

/* ---------------------------------------------------------- leave-one-out --
 * Like the prediction, an extension beyond the reference; serves
 * gaussian_proc.GaussianProcess.leave_one_out / cross_validate of this build. */

/* Leave-one-out terms from the cached factor of K + eta I (factorized if absent)
 * and the resident RHS block R: dinv_out[n] = diag((K+eta I)^-1),
 * sol_out[n][ldsol] = (K+eta I)^-1 R (nrhs columns), gram_out[nrhs][nrhs] = R^T (K+eta I)^-1 R.
 * With W = L^-T (the block gpmi_op_traceinv builds and caches per factorization;
 * either call reuses the other's) and Y = L^-1 R, one pass over the upper block
 * triangle of W gives d_i = sum_k W_ik^2 and row i of W Y together. The column
 * range is cut into chunks of 384 columns whose partial sums are added in
 * ascending order (no atomics: the same input gives the same bits); the
 * environment variable GPMI_LOO_CHUNK (columns, a multiple of 128, read per
 * call) overrides the width. gram_out is bit for bit that of gpmi_op_predict_terms.
 * Any output may be NULL. > 0: first non-positive pivot; < 0: null handle, no resident RHS,
 * ldsol < nrhs. */
int gpmi_op_loo_terms(gpmi_op* op, double eta, double* dinv_out, double* sol_out,
                      int64_t ldsol, double* gram_out);
/* HIP-event ms of the last call's fused pass and the bytes of W it read
 * (when gpmi_op_set_timing is on). */
int gpmi_op_loo_ms(gpmi_op* op, double* pass_ms, double* pass_bytes);

/* ---------------------------------------------- correlation-scale gradient --
 * Like the prediction, an extension beyond the reference; serves
 * gaussian_proc's log_likelihood_der1_scale, GaussianProcess.scale_gradient and
 * train_scale of this build. */

/* The terms of the likelihood's gradient in the correlation scale rho (d entries)
 * of a Matérn K, from the cached factor of A = K + eta I (factorized if absent).
 * With u_k = (p_i - p_j)_k / rho_k, x = |u| and h(x) = -M'(x) / x,
 *   dK_ij / d rho_k = h(x) u_k^2 / rho_k            (0 on the diagonal),
 * and, with Sol = A^-1 R for the resident RHS block R,
 *   tr_out[k]          = sum_ij (A^-1)_ij            dK_ij / d rho_k = tr(A^-1 dK_k)
 *   quad_out[c * d + k] = sum_ij (Sol C_c Sol^T)_ij dK_ij / d rho_k
 * for the ncoef (0..4) symmetric matrices coef[c][nrhs][nrhs]. dK is never
 * formed: one pass reads the lower tiles of A^-1 = W W^T (those
 * gpmi_op_traceinv(.., 2) forms and caches per factorization; either call reuses
 * the other's), forms Sol C_c Sol^T tile by tile on fp64 MFMA from the
 * leave-one-out pass's Sol, and evaluates h from points[n][d], scale[d] and nu,
 * which must be those K was assembled with. Per-tile sums are added in
 * ascending tile order (no atomics: the same input gives the same bits).
 * tr_out and quad_out may be NULL. nu must be 0.5, 1.5, 2.5 or >= 100 (the
 * Gaussian limit).
 * > 0: first non-positive pivot; < 0: null handle (-1006), no matrix (-1000),
 * ncoef outside 0..4 (-1030), ncoef > 0 without a resident RHS (-1012), d outside
 * 1..8 (-1003), a null argument (-1004), a general nu (-1031). */
int gpmi_op_scale_grad_terms(gpmi_op* op, double eta, const double* points, int d,
                             const double* scale, double nu, const double* coef, int ncoef,
                             double* tr_out, double* quad_out);
/* HIP-event ms of the last call's pass over the tiles and the bytes of A^-1 it
 * read (when gpmi_op_set_timing is on). */
int gpmi_op_scale_grad_ms(gpmi_op* op, double* pass_ms, double* pass_bytes);

/* ------------------------------------------------------ expected information --
 * Like the prediction, an extension beyond the reference; serves
 * gaussian_proc.GaussianProcess.fisher_information, hyperparam_covariance and
 * standard_errors of this build. */

/* The second-order terms of the likelihood in (sigma, sigma0, rho) of a Matérn K,
 * from the cached factor of A = K + eta I (factorized if absent) and the resident
 * RHS block R (s = nrhs columns). With N_0 = I, N_k = dK / d rho_k (k = 1..d, as in
 * gpmi_op_scale_grad_terms), S = A^-1 R, M_0 = A^-1, M_k = A^-1 N_k and Y_a = N_a S:
 *   T_out[a * (d + 1) + b]             = tr(M_a M_b)        exactly symmetric
 *   U_out[a][s][s]                     = S^T Y_a
 *   V_out[a * (d + 1) + b][s][s]       = Y_a^T A^-1 Y_b
 * for a, b = 0..d. The d products M_k run on fp64 MFMA: A^-1 is read from the lower
 * tiles gpmi_op_traceinv(.., 2) forms and caches (the upper part as the mirror),
 * N_k is generated slab by slab from points[n][d], scale[d] and nu, which must be
 * those K was assembled with, and is never stored. The traces are summed per tile
 * and the tiles in a fixed order, the thin products and Grams run in ascending row
 * order (no atomics: the same input gives the same bits). The call keeps
 * d n_pad^2 + 32 (d + 1) n_pad doubles (and O(d^2 (n_pad / 128)^2) of partials) of its
 * own on the device, n_pad = n rounded up to 128, and changes no other cache. Any
 * output may be NULL. nu must be 0.5, 1.5, 2.5 or >= 100.
 * > 0: first non-positive pivot; < 0: null handle (-1006), no matrix (-1000), no
 * resident RHS (-1012), d outside 1..8 (-1003), a null argument (-1004), a general
 * nu (-1031), no device memory for the call's own buffers (-1032: they are reserved
 * after the factor, W, the tiles of A^-1 and Sol exist, which stay cached; none of
 * the terms was computed and the handle stays usable). */
int gpmi_op_fisher_terms(gpmi_op* op, double eta, const double* points, int d,
                         const double* scale, double nu, double* T_out, double* U_out,
                         double* V_out);
/* HIP-event ms of the last call's product stage (the d products M_k, 2 n_pad^3 d
 * flops) and of the whole call on the device (when gpmi_op_set_timing is on). */
int gpmi_op_fisher_ms(gpmi_op* op, double* product_ms, double* total_ms);

/* ---------------------------------------------------------------- sampling --
 * Like the prediction, an extension beyond the reference; serves
 * gaussian_proc.GaussianProcess.sample and MixedCorrelation.sample of this build. */

/* gpmi_op_predict_cov without the download of C0: the same launches, c_out, q_out
 * and gram_out bit for bit those of gpmi_op_predict_cov (any may be NULL). C0 of the
 * nstar points stays in the operator's covariance block, marked resident (as after
 * gpmi_op_predict_cov) until the next covariance call replaces it, for
 * gpmi_op_load_predict_cov. Status as gpmi_op_predict_cov. */
int gpmi_op_predict_cov_resident(gpmi_op* op, double eta, const double* points, int d,
                                 const double* scale, double nu, const double* test_points,
                                 int64_t nstar, const double* kstar, int64_t ldks,
                                 const double* kss, int64_t ldkss, double* c_out,
                                 double* q_out, double* gram_out);

/* K of dst <- C0 + U U^T, C0 the resident covariance of src's last covariance call
 * (nstar points) and U the host block U[nstar][ldu] of m <= 15 columns (NULL with
 * m = 0), without a host round trip of C0: one elementwise kernel on dst's stream after
 * src's work, the update as sum over a ascending of fma(U[j][a], U[l][a], .), so that
 * the result is exactly symmetric and, with m = 0, C0 bit for bit. The pad is the
 * identity. Like gpmi_op_load_matrix it drops dst's cached factor.
 * < 0: null handle, different devices, dst's size not nstar, no resident C0, m outside
 * 0..15, ldu < m. */
int gpmi_op_load_predict_cov(gpmi_op* dst, gpmi_op* src, const double* U, int64_t ldu,
                             int m);

/* nsamp draws of N(0, K + eta I): out[nsamp][ldout], row j = (L xi_j)^T with
 * K + eta I = L L^T the cached factor (factorized if absent; no resident RHS needed).
 * xi_j is column j of the host block xi[n][ldxi] when xi != NULL, else it is generated
 * on the device for the global draw indices first .. first + nsamp: entry i of draw j
 * is a function of (seed, j, i) alone (splitmix64 counters and Box-Muller;
 * gaussian_proc/_normal.py restates it), whatever the chunking or nsamp. The product
 * runs on fp64 MFMA in chunks of 1024 draws (GPMI_SAMPLE_CHUNK, a multiple of 128, read
 * per call); within a chunk the triangular depth is cut into pieces chosen from the
 * tile counts and the device's compute units (GPMI_SAMPLE_DEPTH, tile rows, overrides),
 * summed in ascending order without atomics: the same call gives the same bits, and
 * calls that differ in nsamp or the chunk width agree to rounding.
 * > 0: first non-positive pivot; < 0: null handle, no matrix, nsamp < 1, ldout < n,
 * ldxi < nsamp. */
int gpmi_op_sample(gpmi_op* op, double eta, const double* xi, int64_t ldxi,
                   unsigned long long seed, unsigned long long first, int64_t nsamp,
                   double* out, int64_t ldout);
/* HIP-event ms of the last gpmi_op_sample's normal generation and of its product
 * (with the sum of the pieces), and the product's flops, summed over the chunks
 * (when gpmi_op_set_timing is on; 0 otherwise). */
int gpmi_op_sample_ms(gpmi_op* op, double* normal_ms, double* trmm_ms, double* trmm_flops);

/* ------------------------------------------------------------------ sparse --
 * Tapered (compact-support) Matérn correlation in CSR on the device, and the
 * Krylov primitives of the sparse likelihood path. Replaces
 *   generate_correlation(sparse=True)  -> _generate_sparse_correlation.pyx:472-594
 *     (with the two argument fixes of SURVEY §0.4; the threshold heuristic
 *      :294-465 runs on the host, gaussian_proc/generate_correlation)
 *   MixedCorrelation.logdet / traceinv with imate 'slq'
 *     (mixed_correlation.py:138-143,204-209,263-268)
 *   linear_solver for sparse A: scipy.sparse.linalg.cg (_linear_solver.py:57-68).
 */

/* matern(x_i) for m scaled distances (the device kernel the assembly uses). */
int gpmi_matern_values(int device, const double* x, int64_t m, double nu, double* out);

/* CSR of the entries with matern(x_ij) > tau (x_ij the scaled distance), sorted
 * columns, deterministic; int64 row pointers, int32 columns. */
int gpmi_sp_create_matern(int device, const double* points, int64_t n, int d,
                          const double* scale, double nu, double tau, gpmi_sp** out);
/* From a host CSR (indptr[n+1] int64, indices int32, data fp64). */
int gpmi_sp_create_csr(int device, int64_t n, const int64_t* indptr, const int* indices,
                       const double* data, gpmi_sp** out);
/* The Krylov primitives below (spmm, lanczos, cg, msgram) on a DENSE operator's
 * K: a handle that borrows op's device matrix (op must outlive it, and its K must
 * not change while the handle is used). Products run on fp64 MFMA
 * (dense_mm_kernel); nnz reports n * n; gpmi_sp_get_csr is refused (-1105).
 * Replaces imate 'slq' on a dense K (mixed_correlation.py:138-143,204-209,263-268:
 * the reference's branch passes the misspelt self.K_afm and raises
 * AttributeError, so there is no reference value; the estimator is the same as
 * on a sparse K). */
int gpmi_sp_create_dense(gpmi_op* op, gpmi_sp** out);
int gpmi_sp_destroy(gpmi_sp* sp);
int gpmi_sp_info(const gpmi_sp* sp, int64_t* n, int64_t* nnz);
int gpmi_sp_get_csr(gpmi_sp* sp, int64_t* indptr, int* indices, double* data);

/* Y = (K + eta I) X for an [n][ld] host block with ncol columns. */
int gpmi_sp_spmm(gpmi_sp* sp, double eta, const double* X, int64_t ld, int ncol, double* Y,
                 int64_t ldy);

/* Lanczos tridiagonals of K for nprobe Rademacher probes (counter-based,
 * probe index probe_offset + p, seed), full CGS2 reorthogonalisation.
 * alpha, beta: [nprobe][steps]; a column that reaches an invariant subspace is
 * padded with zeros (beta = 0 marks the end of its tridiagonal). */
int gpmi_sp_lanczos(gpmi_sp* sp, int nprobe, int steps, uint64_t seed, int probe_offset,
                    double* alpha, double* beta);
/* The same with imate's `orthogonalize` option: -1 full reorthogonalisation (as
 * gpmi_sp_lanczos), 0 the plain three-term recurrence (imate's default), k > 0
 * CGS2 against the last k vectors. Replaces the Lanczos inside imate.logdet /
 * traceinv(method='slq', orthogonalize=...) (mixed_correlation.py:138-143,
 * 204-209,263-268 pass imate_options through). */
int gpmi_sp_lanczos_ex(gpmi_sp* sp, int nprobe, int steps, uint64_t seed, int probe_offset,
                       int orthogonalize, double* alpha, double* beta);

/* Blocked CG for (K + eta I) X = RHS, per-column stop ||r|| <= rtol ||b||. */
int gpmi_sp_cg(gpmi_sp* sp, double eta, const double* rhs, int64_t ld, int nrhs, double rtol,
               int maxiter, double* sol, int64_t ldsol, int* iterations);

/* Multi-shift CG Gram: G[j] = RHS^T (K + etas[j] I)^-1 RHS for every eta from
 * ONE blocked CG on K + min(etas) I (shifted systems share its Krylov space;
 * the Gram entries follow scalar recurrences, no per-eta vectors). Per-column
 * stop ||r|| <= rtol ||b|| on the base (slowest) system. nrhs <= 16,
 * neta * nrhs <= 1024; G: [neta][nrhs][nrhs]. Every K + eta_j I must be SPD.
 * Replaces the per-eta sparse solves of DirectLikelihood.log_likelihood
 * _direct_likelihood.py:59,62 -> MixedCorrelation.solve mixed_correlation.py:280-299
 * -> _linear_solver.py:57-68 (scipy.sparse.linalg.cg, tol 1e-6). */
int gpmi_sp_msgram(gpmi_sp* sp, const double* etas, int neta, const double* rhs, int64_t ld,
                   int nrhs, double rtol, int maxiter, double* G, int* iterations);
/* (rhs == NULL: the block made resident by gpmi_sp_set_rhs.) */
/* The same for a shard of the right-hand sides: the columns [c_lo, c_hi) of the
 * nrhs-column block solved (every eta), dotted with all nrhs columns:
 * G[neta][nrhs][c_hi - c_lo], G[j][a][c] = b_a^T (K + eta_j I)^-1 b_{c_lo + c}. Ranks
 * holding different column shards together form the whole Gram with a fraction of
 * the multi-shift CG's SpMMs each (the eta shard alone divides only its per-shift
 * scalars). */
int gpmi_sp_msgram_cols(gpmi_sp* sp, const double* etas, int neta, const double* rhs, int64_t ld,
                        int nrhs, int c_lo, int c_hi, double rtol, int maxiter, double* G,
                        int* iterations);
/* Keep the nrhs-column block [n][ld] (host, original row order) resident in HBM:
 * gpmi_sp_msgram / gpmi_sp_msgram_cols with rhs == NULL (ld ignored, nrhs equal to
 * this block's) then read it there instead of uploading the host block per call (the
 * likelihood's [X z] is fixed across evaluations; at cfg 5, 262144 x 11 doubles,
 * the per-call upload from pageable memory took ~1.9 ms of a ~14 ms step). Replaces
 * nothing in the reference (its CG reads the numpy arrays in place). */
int gpmi_sp_set_rhs(gpmi_sp* sp, const double* rhs, int64_t ld, int nrhs);

/* The SpMM kernel this operator uses (1: X-window staged in LDS, 64-row blocks;
 * 0: gathers from X, one wave per row) and its window sizes (columns per block:
 * mean, max). */
int gpmi_sp_spmm_info(gpmi_sp* sp, int* windowed, double* mean_window, int* max_window);
/* The SpMM kernel gpmi_sp_spmm runs for an s-column block on this operator:
 * 0 gather from X (csr_spmm_kernel), 1 X-window in 8-column chunks
 * (csr_spmm_win_kernel), 3 gather from X by column pairs (csr_spmm_pair_kernel,
 * even s), 4 dense (dense_mm_kernel, gpmi_sp_create_dense), 5 window with
 * latency-hidden staging (csr_spmm_wing_kernel, s = 7, 8, 11, 12, 20 while the
 * widest window fits 80 KB of LDS); a 16-byte-wide kernel handed a block that is
 * not 16-byte aligned runs csr_spmm_kernel. (2, the round-2 one-pass window, is no
 * longer returned.) Diagnostic; no reference counterpart. */
int gpmi_sp_spmm_kernel(gpmi_sp* sp, int s, int* kind);
/* Whether the last gpmi_sp_cg / gpmi_sp_msgram met rtol in every column before
 * maxiter (1) or stopped at maxiter (0). scipy's cg, which the reference calls
 * (_linear_solver.py:64,68), returns the unconverged iterate silently; the
 * Python layer warns. (A non-positive p^T A p makes those calls return 1, "not
 * positive definite".) */
int gpmi_sp_last_status(const gpmi_sp* sp, int* converged);
/* Active-column compactions of the last gpmi_sp_msgram(_cols) call: once at most
 * half of the block's columns still iterate, their state moves into a block of
 * their width (the Grams are unchanged, bit for bit; GPMI_MS_COMPACT=0 disables
 * it). Diagnostic. */
int gpmi_sp_msgram_compactions(const gpmi_sp* sp, int* count);
/* The launch segments of the last gpmi_sp_msgram(_cols) call, in order: segment q
 * ran iterations[q] iterations (each one SpMM + reduce + update launch) at block
 * width widths[q] (the full block, then each compacted block). count = segments
 * (compactions + 1); cap = room in widths / iterations. Diagnostic (bench.py's
 * algorithmic-byte count of the step). */
int gpmi_sp_msgram_segments(const gpmi_sp* sp, int cap, int* widths, int* iterations,
                            int* count);

/* Device-resident SpMM timing: reps launches of Y = (K + eta I) X with an
 * [n][s] block already in HBM, queued behind a gate kernel that holds the stream
 * until all of them are enqueued (so they run back to back, not at the host's
 * launch rate); average ms per launch (HIP events). */
int gpmi_sp_bench_spmm(gpmi_sp* sp, int s, int reps, double eta, double* avg_ms);
/* In-step SpMM timing (measurement; no reference counterpart): while enabled,
 * every SpMM this operator launches (Lanczos, CG, multi-shift CG; either
 * stream) is timed: the window SpMM stamps its own span (earliest workgroup start
 * to latest workgroup end on the device wall clock, up to 8192 launches per
 * window), other kinds get a HIP event pair on their stream. set_timing(1) starts
 * a window (clears the log), set_timing(0) ends it and keeps the log. spmm_timing
 * sums the logged spans by block width s: widths[k], launches[k], total_ms[k] for
 * k < min(*n_widths, max_widths), ascending s (it waits for the device). */
int gpmi_sp_set_timing(gpmi_sp* sp, int enable);
int gpmi_sp_spmm_timing(gpmi_sp* sp, int max_widths, int* n_widths, int* widths,
                        int* launches, double* total_ms);

/* ------------------------------------------------- prediction on a sparse K --
 * The model on a sparse K is the tapered kernel k_tau(x) = matern(x) if matern(x) > tau,
 * else 0, so k*_j, the correlations of new point j with the training points, follows the
 * same rule: K* [nstar][n] is sparse. With S = K + eta I and R = [X z] (nrhs <= 32
 * columns):
 *   c[nstar][nrhs] = K* S^-1 R,   q[nstar] = diag(K* S^-1 K*^T),   G[nrhs][nrhs] = R^T S^-1 R,
 * the terms gpmi_op_predict_terms returns from a dense factor. Here: one blocked CG for
 * S^-1 R, one gather product for c, and for q one CG per block of <= 32 rows of K*
 * (GPMI_SP_PREDICT_S, default 32) scattered into a device block; right-hand sides and
 * solutions never leave the device. The CGs stop per column at ||r|| <= rtol ||b|| or at
 * maxiter (gpmi_sp_last_status then reports 0); p^T S p <= 0 returns 1. Empty rows of K*
 * are legal and give c = 0 and q = 0 exactly.
 * No reference counterpart (the reference stops at training). */

/* c, q (when want_q; else q may be NULL and is not touched) and G for the nstar new points
 * test_points [nstar][d], K* assembled on the device from the geometry
 * gpmi_sp_create_matern kept (same kernel arithmetic: a new point equal to training point
 * i reproduces row i of K bit for bit). -1108: the handle has no geometry (from a CSR or
 * a dense K), or d is not its dimension. rhs [n][ld], original row order; rhs == NULL:
 * the block of gpmi_sp_set_rhs (nrhs equal to its width). iterations[2] = {the R solve,
 * the most of any variance block}. -1104: nrhs outside [1, 32], maxiter < 0, rtol negative
 * or NaN. No reference counterpart. */
int gpmi_sp_predict_terms(gpmi_sp* sp, double eta, const double* rhs, int64_t ld, int nrhs,
                          const double* test_points, int64_t nstar, int d, int want_q,
                          double rtol, int maxiter, double* c, double* q, double* G,
                          int* iterations);
/* The same with the caller's K*: a host CSR [nstar][n] over original column indices
 * (indptr int64, indices int32 strictly ascending per row, data fp64), for any handle.
 * It is permuted to the device's row order and re-sorted per row at upload. -1109:
 * row pointers not ascending, a column outside [0, n) or a row's columns not strictly
 * ascending. No reference counterpart. */
int gpmi_sp_predict_terms_csr(gpmi_sp* sp, double eta, const double* rhs, int64_t ld, int nrhs,
                              int64_t nstar, const int64_t* indptr, const int* indices,
                              const double* data, int want_q, double rtol, int maxiter,
                              double* c, double* q, double* G, int* iterations);
/* Assemble K* of test_points [nstar][d] only (kept on the device until the next cross
 * assembly or prediction on this handle); *nnz its entries. The cell list of the create
 * when it found a plan; all pairs for d > 3, under GPMI_SPARSE_BRUTE=1 (read at this
 * call) or when a row holds more than 512 kept entries: the CSR is identical either way.
 * -1108 as above. No reference counterpart. */
int gpmi_sp_cross_matern(gpmi_sp* sp, const double* test_points, int64_t nstar, int d,
                         int64_t* nnz);
/* The last cross CSR (assembled or given) back on the host: indptr[nstar + 1], and
 * indices / data of *nnz entries, original column indices ascending per row. -1110: there
 * is none. No reference counterpart. */
int gpmi_sp_get_cross(gpmi_sp* sp, int64_t* indptr, int* indices, double* data);

/* -------------------------------------------------------------------- band --
 * One-time orthogonal reduction of an operator's K to symmetric band form,
 * K = Q B Q^T with bandwidth 128 (blocked Householder panels, two-sided
 * updates on fp64 MFMA, 4/3 n^3 flops), after which every eta costs one banded
 * Cholesky of B + eta I, O(n 128^2), since K + eta I = Q (B + eta I) Q^T.
 * This is the device form of the reference's one-time spectral setup:
 *   MixedCorrelation.__init__ with imate_method='eigenvalue' runs eigh(K) once
 *   (mixed_correlation.py:76-79) so that logdet(eta) is cheap for every eta
 *   (:239-248); Likelihood builds its operator that way (likelihood.py:41-49).
 * n <= 32768. */
typedef struct gpmi_band gpmi_band;

/* Reduce the operator's current K (the operator stays usable; the band form is
 * a copy). Blocks until the reduction is done. */
int gpmi_band_create(gpmi_op* op, gpmi_band** out);
int gpmi_band_destroy(gpmi_band* b);
/* Re-run the reduction on the operator's current K (same n and device), reusing
 * the band's buffers; the resident RHS must be set again afterwards. */
int gpmi_band_refresh(gpmi_band* b, gpmi_op* op);
/* gpmi_band_refresh + gpmi_band_set_rhs in one call: Y = Q^T R is applied panel by
 * panel on a separate stream while the reduction proceeds (same results). */
int gpmi_band_refresh_rhs(gpmi_band* b, gpmi_op* op, const double* rhs, int64_t ld,
                          int nrhs);

/* Y = Q^T R for an [n][ld] host block R with nrhs <= 16 columns (resident). */
int gpmi_band_set_rhs(gpmi_band* b, const double* rhs, int64_t ld, int nrhs);

/* For any number of eta values (one workgroup per eta, all concurrent):
 *   logdet[e]           = log det(K + eta_e I) = log det(B + eta_e I)
 *   gram[e][nrhs][nrhs] = R^T (K + eta_e I)^-1 R = Y^T (B + eta_e I)^-1 Y
 *   info[e]             = 0, or 1-based first non-positive pivot.
 * Replaces the logdet + 2 x solve of DirectLikelihood.log_likelihood
 * (_direct_likelihood.py:59,62,332) on the 'eigenvalue' operator. */
int gpmi_band_loglik(gpmi_band* b, const double* etas, int neta, double* logdet,
                     double* gram, int* info);

/* Most etas per gpmi_band_der_terms call (its factor store is
 * 2 * n_pad * 128 doubles per eta: 33.5 MB at n = 16384). */
#define GPMI_BAND_DER_MAX 256

/* The eta-derivative terms of the profiled likelihood for neta <= GPMI_BAND_DER_MAX
 * etas (one workgroup per eta): logdet and info as gpmi_band_loglik, and
 *   g1[e] = R^T (K + eta_e I)^-1 R,  g2[e] = R^T (K + eta_e I)^-2 R,
 *   g3[e] = R^T (K + eta_e I)^-3 R   (each [nrhs][nrhs]),
 * from the banded factor (forward solve, backward solve, forward solve).
 * With traceinv from gpmi_band_eigenvalues these give
 * ProfileLikelihood.log_likelihood_der1_eta / der2_eta
 * (_profile_likelihood.py:91-192), which the reference evaluates with 2-5
 * dense solves per eta. Any output pointer may be NULL. */
int gpmi_band_der_terms(gpmi_band* b, const double* etas, int neta, double* logdet,
                        double* g1, double* g2, double* g3, int* info);
/* gpmi_band_der_terms plus, when tr1 != NULL, tr1[e] = trace((K + eta_e I)^-1) =
 * trace((B + eta_e I)^-1) by selected inversion of the block-cyclic-reduction
 * factor down its reduction tree (the Takahashi recurrences: only the inverse's
 * blocks on the factor's pattern, O(n 128^2) per eta, every block of a level in
 * parallel). With these the profiled likelihood's der1
 * (_profile_likelihood.py:91-132) needs no eigenvalues: it replaces the
 * eigenvalue sums of MixedCorrelation.traceinv ('eigenvalue', exponent 1,
 * mixed_correlation.py:172-181) and the eigh they come from (:76-79). */
int gpmi_band_der_terms_ex(gpmi_band* b, const double* etas, int neta, double* logdet,
                           double* g1, double* g2, double* g3, double* tr1, int* info);
/* tr[e] = trace((K + eta_e I)^-1) for neta <= GPMI_BAND_DER_MAX etas by the same
 * selected inversion (a cyclic-reduction factorization per eta first); info as
 * gpmi_band_loglik. Replaces MixedCorrelation.traceinv(eta) on the 'eigenvalue'
 * operator (mixed_correlation.py:172-181) without the eigenvalues. */
int gpmi_band_traceinv(gpmi_band* b, const double* etas, int neta, double* tr, int* info);
/* Most etas per device chunk of the exponent-2 trace below (its eta-tangent store
 * is 10 n_pad * 128 doubles per eta: 168 MB at n = 16384); larger calls run in
 * chunks of this size. */
#define GPMI_BAND_TAN_MAX 64

/* gpmi_band_der_terms_ex plus, when tr2 != NULL, tr2[e] = trace((K + eta_e I)^-2)
 * = -d/deta trace((B + eta_e I)^-1): the cyclic-reduction factor and the selected
 * inversion above differentiated in eta in forward mode (every block carries its
 * eta-tangent; about three times the selected inversion's products). tr2 needs tr1
 * (the tangent rides on the primal recurrences); tr1 != NULL is then implied.
 * With it the direct Hessian (_direct_likelihood.py:224) and the profiled der2
 * (_profile_likelihood.py:168) need no eigenvalues: it replaces the eigenvalue
 * sums of MixedCorrelation.traceinv(eta, exponent=2) on the 'eigenvalue' operator
 * (mixed_correlation.py:172-181) and the eigh they come from (:76-79). */
int gpmi_band_der_terms_ex2(gpmi_band* b, const double* etas, int neta, double* logdet,
                            double* g1, double* g2, double* g3, double* tr1, double* tr2,
                            int* info);
/* tr1[e] = trace((K + eta_e I)^-1) and, when tr2 != NULL, tr2[e] =
 * trace((K + eta_e I)^-2) for neta <= GPMI_BAND_DER_MAX etas (selected inversion
 * and its eta-tangent, as gpmi_band_der_terms_ex2); info as gpmi_band_loglik.
 * Replaces MixedCorrelation.traceinv(eta, exponent in {1, 2}) on the 'eigenvalue'
 * operator (mixed_correlation.py:172-181). */
int gpmi_band_traceinv2(gpmi_band* b, const double* etas, int neta, double* tr1, double* tr2,
                        int* info);
/* Device ms of the selected-inversion part of the last gpmi_band_traceinv /
 * gpmi_band_traceinv2 / gpmi_band_der_terms_ex(2) call (tr1 or tr2 requested).
 * Diagnostic. */
int gpmi_band_sinv_ms(gpmi_band* b, double* ms);

/* Reduction diagnostics: how many reductions of this band fell back to the
 * per-column panel launches after a timed-out single-launch panel hand-off, and
 * the largest panel grid (workgroups) run as one launch on this device
 * (CU count x resident hh_panel workgroups per CU, at most 128). */
int gpmi_band_stats(gpmi_band* b, int* panel_fallbacks, int* panel_maxg);
/* The panel algorithm of this band's reductions (0: CholeskyQR panels, shifted
 * CholeskyQR3 + Householder reconstruction, the default; 1: Householder panels,
 * GPMI_BAND_PANEL=hh), how many reductions were redone with Householder panels
 * (a CholeskyQR panel broke down past the single-launch Householder panel's
 * size) and how many panels broke down (numerically rank-deficient) and were
 * factored on the device by the Householder panel instead. Replaces nothing in
 * the reference: the panel QR is inside its one-time eigh
 * (mixed_correlation.py:76-79). */
int gpmi_band_cq_stats(gpmi_band* b, int* panel_mode, int* cq_fallbacks,
                       int* cq_panel_fallbacks);
/* Which form the last gpmi_band_eigenvalues took (2: the one-launch systolic chase
 * with a D and an E workgroup per position, 1: one workgroup per position, 0: the
 * per-wavefront launches), how many systolic attempts timed out and were redone by
 * another form, and how many workgroups of the one-per-position form can be
 * co-resident. */
int gpmi_band_chase_info(gpmi_band* b, int* systolic, int* fallbacks, int* maxg);

/* Device ms of the last gpmi_band_der_terms call (HIP events). */
int gpmi_band_der_ms(gpmi_band* b, double* der_ms);

/* The n eigenvalues of K (ascending): B -> tridiagonal by bulge chasing on the
 * device (one launch per wavefront of 128-row tasks), then bisection on Sturm
 * counts (one thread per eigenvalue). Completes the eigenvalue operator:
 * trace / traceinv / logdet of K + eta I as sums over lambda_i + eta
 * (mixed_correlation.py:127-133,172-181,239-248). Allocates n_pad^2 doubles. */
int gpmi_band_eigenvalues(gpmi_band* b, double* lam);

/* The band matrix B as a dense symmetric [n][ld] host matrix (tests). */
int gpmi_band_get(gpmi_band* b, double* B_out, int64_t ld);

/* Read-backs of what each stage of the band path left on the device (tests and
 * diagnostics; tests/test_gpu_band_stages.py holds each to a backward-error bar). Each is
 * a copy on the handle's stream: no kernel runs and no later result changes. While what
 * one reads does not exist it returns -1204; a slot outside the last call -1205; a slot
 * whose factorization failed -1206; a leading dimension too small -1003; a null output
 * -1004. No reference counterpart.
 *
 * The reduction K_pad = Q B Q^T, Q = prod_j (I - V_j T_j V_j^T) over the nt - 1 panels
 * (nt = n_pad / 128), everything at n_pad size: B_out [n_pad][ld] symmetric (the stored
 * lower band mirrored, as gpmi_band_get, the pad block as the device holds it: the
 * identity); V_out [n_pad][ld] with panel j's unit lower trapezoid in columns
 * [128 j, +128) and rows from 128 (j + 1), the unit diagonal written, zero elsewhere;
 * T_out [nt - 1][128][128] the compact-WY T of every panel as stored. ld >= n_pad. */
int gpmi_band_get_reduction(gpmi_band* b, double* B_out, double* V_out, double* T_out,
                            int64_t ld);
/* Y = Q^T R of the resident RHS, Y_out [n_pad][ld], nrhs columns written. */
int gpmi_band_get_rhs(gpmi_band* b, double* Y_out, int64_t ld);
/* x = (B + eta_slot I)^-1 Y as the last gpmi_band_der_terms(_ex, _ex2) call left it
 * (the sequential kernel's or the cyclic reduction's, whichever ran), X_out [n_pad][ld],
 * nrhs columns written. slot counts within that call's last device chunk (a call with
 * tr2 runs in chunks of GPMI_BAND_TAN_MAX). A new RHS or reduction discards it. */
int gpmi_band_get_solution(gpmi_band* b, int slot, double* X_out, int64_t ld);
/* The blocks of (B + eta_slot I)^-1 the last selected inversion (gpmi_band_traceinv,
 * _traceinv2, _der_terms_ex, _ex2 with tr1; its last chunk) left, by original block
 * index o: Zd_out [nt][128][128] = Z_oo; Zo_out [nt][2][128][128] = Z_lo, Z_ro for
 * the neighbours l, r of o at the level that eliminated it (level 0: o - 1 and o + 1 for
 * odd o); slots no neighbour fills are zeroed. tangent = 1: the eta-derivatives dZd,
 * dZo, present after a call with tr2. */
int gpmi_band_get_sinv(gpmi_band* b, int slot, int tangent, double* Zd_out, double* Zo_out);
/* The tridiagonal the last gpmi_band_eigenvalues' bulge chase left and its bisection
 * read: d_out [n] the diagonal, e2_out [n - 1] the squared subdiagonal. */
int gpmi_band_get_tridiagonal(gpmi_band* b, double* d_out, double* e2_out);

/* Device ms of the last reduction, Q^T application and loglik call (HIP events). */
int gpmi_band_last_timing(gpmi_band* b, double* reduce_ms, double* rhs_ms,
                          double* loglik_ms);

#ifdef __cplusplus
}
#endif

#endif /* GPMI_H_ */
