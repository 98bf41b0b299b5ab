// C-ABI (include/gpmi.h): the thread's last error, the Matérn entry points, and the
// dense operator's life and plain calls (create / destroy, loading K, the resident RHS,
// matvec, trace, the GPMI_* knobs). The factorization and the calls that consume a
// factor are gpmi_dense_factor.hip, the prediction gpmi_dense_predict.hip; the handle
// itself is gpmi_op.h.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "gpmi_op.h"
#include "gpmi_band.h"

using namespace gpmi;

namespace {

thread_local char g_err[512] = "";

int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

}  // namespace

namespace gpmi {
int set_error(int code, const char* msg) { return set_err(code, "%s", msg); }
int set_errorf(int code, const char* fmt, ...) {
  char b[sizeof(g_err)];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof(b), fmt, ap);
  va_end(ap);
  return set_err(code, "%s", b);
}
int upload_rhs(gpmi_op* op, double* dst, const double* rhs, int64_t ld, int nrhs, int col0) {
  std::vector<double> h((size_t)op->n_pad * RLD, 0.0);
  for (int64_t i = 0; i < op->n; ++i)
    for (int c = 0; c < nrhs; ++c) h[(size_t)i * RLD + c] = rhs[i * ld + col0 + c];
  HIP_TRY(hipMemcpyAsync(dst, h.data(), sizeof(double) * h.size(),
                         hipMemcpyHostToDevice, op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  return 0;
}
int op_view(const gpmi_op* op, OpView* v) {
  if (!op) return set_err(-1006, "null handle");
  v->device = op->device;
  v->n = op->n;
  v->n_pad = op->n_pad;
  v->K = op->K;
  v->has_K = op->has_K;
  return 0;
}
}  // namespace gpmi

namespace {
// K[i][i] = 1 for the pad rows n <= i < n_pad (at most 127 of them).
__global__ void pad_identity_kernel(double* K, int64_t ldk, int64_t n) {
  const int64_t i = n + threadIdx.x;
  if (i < ldk) K[i * ldk + i] = 1.0;
}
}  // namespace

extern "C" {

int gpmi_version(void) { return 100; }

int gpmi_last_error(char* buf, size_t len) {
  if (!buf || !len) return 0;
  strncpy(buf, g_err, len - 1);
  buf[len - 1] = 0;
  return 0;
}

int gpmi_device_count(int* count) {
  HIP_TRY(hipGetDeviceCount(count));
  return 0;
}

thread_local double g_assembly_ms = 0.0;   // last matern_dense_kernel launch (HIP events)

static int matern_params(double nu, MaternParams* P) {
  if (!(nu > 0.0)) return set_err(-1002, "nu must be positive (got %g)", nu);
  P->nu = nu;
  P->sqrt2nu = std::sqrt(2.0 * nu);
  P->mu = nu < 2.0 ? nu : nu - std::floor(nu) + 1.0;
  P->lp0 = (1.0 - P->mu) * std::log(2.0) - std::lgamma(P->mu);
  P->lp1 = -P->mu * std::log(2.0) - std::lgamma(P->mu + 1.0);
  if (nu == 0.5) P->mode = MATERN_HALF;
  else if (nu == 1.5) P->mode = MATERN_3HALF;
  else if (nu == 2.5) P->mode = MATERN_5HALF;
  else if (nu < 100) P->mode = MATERN_GENERAL;
  else P->mode = MATERN_GAUSS;
  return 0;
}

int gpmi_last_assembly_ms(double* ms) {
  if (!ms) return set_err(-1004, "null output");
  *ms = g_assembly_ms;
  return 0;
}

int gpmi_matern_values(int device, const double* x, int64_t m, double nu, double* out) {
  if (m <= 0) return 0;
  MaternParams P;
  int rc = matern_params(nu, &P);
  if (rc) return rc;
  DeviceGuard g(device);
  DevBuf<double> dx, dv;
  HIP_TRY(dx.reserve(m));
  HIP_TRY(dv.reserve(m));
  HIP_TRY(hipMemcpy(dx, x, sizeof(double) * m, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(matern_eval_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, dx,
                     m, P, dv);
  LAUNCH_CHECK("matern_eval_kernel");
  HIP_TRY(hipMemcpy(out, dv, sizeof(double) * m, hipMemcpyDeviceToHost));
  return 0;
}

static int assemble(int device, hipStream_t s, const double* points, int64_t n, int d,
                    const double* scale, double nu, double* Kdev, int64_t ldk,
                    int64_t n_pad) {
  if (d < 1 || d > GPMI_MAX_DIM)
    return set_err(-1003, "dimension %d outside [1, %d]", d, GPMI_MAX_DIM);
  MaternParams P;
  int rc = matern_params(nu, &P);
  if (rc) return rc;
  DeviceGuard g(device);
  DevBuf<double> dp, ds;
  HIP_TRY(dp.reserve((size_t)std::max<int64_t>(1, n * d)));
  HIP_TRY(ds.reserve(d));
  HIP_TRY(hipMemcpyAsync(dp, points, sizeof(double) * n * d, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ds, scale, sizeof(double) * d, hipMemcpyHostToDevice, s));
  // lower-triangular 64 x 64 tiles, each mirrored (gpmi_matern.hip)
  const int64_t T = (n_pad + 63) / 64;
  Event e0, e1;
  HIP_TRY(hipEventCreate(&e0.h));
  HIP_TRY(hipEventCreate(&e1.h));
  HIP_TRY(hipEventRecord(e0, s));
  launch_matern_dense(dim3((unsigned)(T * (T + 1) / 2)), s, dp, n, d, ds, P, Kdev, ldk, n_pad);
  LAUNCH_CHECK("matern_dense_kernel");
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  g_assembly_ms = ms;
  return 0;
}

int gpmi_matern_dense(int device, const double* points, int64_t n, int d,
                      const double* scale, double nu, double* K_out, int64_t ldk) {
  if (n <= 0) return 0;
  DeviceGuard g(device);
  DevBuf<double> dK;
  HIP_TRY(dK.reserve((size_t)n * n));
  int rc = assemble(device, nullptr, points, n, d, scale, nu, dK, n, n);
  if (rc) return rc;
  HIP_TRY(hipMemcpy2D(K_out, sizeof(double) * ldk, dK, sizeof(double) * n, sizeof(double) * n,
                      n, hipMemcpyDeviceToHost));
  return 0;
}

int gpmi_op_create(int device, int64_t n, int max_batch, gpmi_op** out) {
  if (!out) return set_err(-1004, "null output handle");
  if (n <= 0) return set_err(-1005, "matrix size must be positive");
  if (max_batch < 1) max_batch = 1;
  DeviceGuard g(device);
  std::unique_ptr<gpmi_op> owner(new gpmi_op());   // (a failed create just deletes it)
  gpmi_op* op = owner.get();
  DenseFactor& f = op->fac;
  op->device = device;
  op->n = n;
  op->n_pad = (n + TS - 1) / TS * TS;
  op->nt = (int)(op->n_pad / TS);
  op->max_batch = max_batch;
  if (const char* g = std::getenv("GPMI_GROUPS")) op->groups = std::atoi(g);
  if (const char* m = std::getenv("GPMI_PANEL")) {
    // rec (the default: it measures faster): the recursive panel
    // factorization (band SYRKs + panel_kernel); col: left-looking, one colpanel_kernel
    // launch per panel column
    if (!std::strcmp(m, "col")) op->panel_mode = DENSE_COL;
    else if (std::strcmp(m, "rec") && *m)
      return set_err(-1011, "GPMI_PANEL must be rec or col (got %s)", m);
  }
  if (const char* m = std::getenv("GPMI_KLOOP")) {
    // early (the default): syrk_kernel's k-loop with the LDS hand-off off the MFMA path;
    // late: the form before it (the bitwise tests and the in-process A/B). Same results.
    if (!std::strcmp(m, "late")) op->kloop = KLOOP_LATE;
    else if (std::strcmp(m, "early") && *m)
      return set_err(-1009, "GPMI_KLOOP must be early or late (got %s)", m);
  }
  op->tim.trace = std::getenv("GPMI_SYRK_TRACE") != nullptr;
  // (one stream; f.stream3 only for the two-halves batch form: HIP streams beyond
  // the process's hardware queues (GPU_MAX_HW_QUEUES = 4) share queues and slow other
  // objects' multi-stream work, a band reduction beside a dense operator holding three
  // streams: 161 -> 181 ms)
  HIP_TRY(hipStreamCreateWithFlags(&op->stream.h, hipStreamNonBlocking));
  for (Event* ev : {&f.ev_fork, &f.ev_g})
    HIP_TRY(hipEventCreateWithFlags(&ev->h, sync_event_flags()));
  const size_t np = (size_t)op->n_pad, nt = (size_t)op->nt, mb = (size_t)max_batch;
  const struct {
    const char* name;
    Sized buf;
  } bufs[] = {{"K", sized(op->K, np * np)},
              {"A", sized(f.A, mb * np * np)},
              {"R", sized(f.R, mb * np * RLD)},
              {"X", sized(f.X, mb * np * RLD)},
              {"U", sized(f.U, mb * TS * RLD)},
              {"Linv", sized(f.Linv, mb * nt * TS * TS)},
              {"logdiag", sized(f.logdiag, mb * nt)},
              {"gram", sized(f.gram, mb * nt * 256)},
              {"out", sized(f.out, mb * OUT_LD)},
              {"etas", sized(f.etas, mb)},
              {"rhs_src", sized(op->rhs_src, np * RLD)},
              {"scratch", sized(op->scratch, np * RLD)},
              {"scratch2", sized(op->scratch2, np * RLD)},
              {"tracebuf", sized(op->tracebuf, np * 2)},
              {"info", sized(f.info, mb)}};
  for (const auto& b : bufs) {
    const hipError_t e = b.buf.buf->reserve_bytes(b.buf.bytes);
    if (e != hipSuccess)
      return set_err(-(int)e, "allocation of %s failed: %s", b.name, hipGetErrorString(e));
  }
  HIP_TRY(hipMemsetAsync(op->rhs_src, 0, sizeof(double) * np * RLD, op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  *out = owner.release();
  return 0;
}

int gpmi_op_destroy(gpmi_op* op) {
  if (!op) return 0;
  DeviceGuard g(op->device);
  if (op->stream) (void)hipStreamSynchronize(op->stream);
  if (op->fac.stream3) (void)hipStreamSynchronize(op->fac.stream3);
  delete op;
  return 0;
}

int gpmi_op_size(const gpmi_op* op, int64_t* n, int64_t* n_pad) {
  if (!op) return set_err(-1006, "null handle");
  if (n) *n = op->n;
  if (n_pad) *n_pad = op->n_pad;
  return 0;
}

int gpmi_op_load_matrix(gpmi_op* op, const double* K_host, int64_t ldk) {
  if (!op) return set_err(-1006, "null handle");
  DeviceGuard g(op->device);
  const int64_t np = op->n_pad, n = op->n;
  // identity pad, then the n x n block
  HIP_TRY(hipMemsetAsync(op->K, 0, sizeof(double) * np * np, op->stream));
  HIP_TRY(hipMemcpy2DAsync(op->K, sizeof(double) * np, K_host, sizeof(double) * ldk,
                           sizeof(double) * n, n, hipMemcpyHostToDevice, op->stream));
  if (np > n) {
    std::vector<double> one(1, 1.0);
    for (int64_t i = n; i < np; ++i)
      HIP_TRY(hipMemcpyAsync(op->K + i * np + i, one.data(), sizeof(double),
                             hipMemcpyHostToDevice, op->stream));
  }
  HIP_TRY(hipStreamSynchronize(op->stream));
  op->has_K = true;
  op->fac.drop();
  return 0;
}

int gpmi_op_load_sparse(gpmi_op* op, const gpmi_sp* sp) {
  if (!op || !sp) return set_err(-1006, "null handle");
  int64_t n_sp = 0;
  if (int rc = gpmi_sp_info(sp, &n_sp, nullptr)) return rc;
  if (n_sp != op->n) return set_err(-1005, "sparse operator has n = %lld, dense has %lld",
                                    (long long)n_sp, (long long)op->n);
  DeviceGuard g(op->device);
  const int64_t np = op->n_pad;
  HIP_TRY(hipMemsetAsync(op->K, 0, sizeof(double) * np * np, op->stream));
  if (int rc = gpmi::sp_scatter_dense(sp, op->device, op->K, np, op->stream)) return rc;
  if (np > op->n) {
    hipLaunchKernelGGL(pad_identity_kernel, dim3(1), dim3(128), 0, op->stream, op->K, np, op->n);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(op->stream));
  op->has_K = true;
  op->fac.drop();
  return 0;
}

int gpmi_op_assemble_matern(gpmi_op* op, const double* points, int d, const double* scale,
                            double nu) {
  if (!op) return set_err(-1006, "null handle");
  int rc = assemble(op->device, op->stream, points, op->n, d, scale, nu, op->K, op->n_pad,
                    op->n_pad);
  if (rc) return rc;
  op->has_K = true;
  op->fac.drop();
  return 0;
}

int gpmi_op_get_matrix(gpmi_op* op, double* K_out, int64_t ldk) {
  if (!op) return set_err(-1006, "null handle");
  DeviceGuard g(op->device);
  HIP_TRY(hipMemcpy2DAsync(K_out, sizeof(double) * ldk, op->K, sizeof(double) * op->n_pad,
                           sizeof(double) * op->n, op->n, hipMemcpyDeviceToHost, op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  return 0;
}

int gpmi_op_set_rhs(gpmi_op* op, const double* rhs, int64_t ld, int nrhs) {
  if (!op) return set_err(-1006, "null handle");
  if (nrhs < 0 || nrhs > RLD) return set_err(-1007, "nrhs %d outside [0, %d]", nrhs, RLD);
  DeviceGuard g(op->device);
  int rc = upload_rhs(op, op->rhs_src, rhs, ld, nrhs, 0);
  if (rc) return rc;
  op->nrhs = nrhs;
  ++op->rhs_gen;
  return 0;
}

int gpmi_op_matvec(gpmi_op* op, const double* x, int64_t ld, int ncol, double* y,
                   int64_t ldy) {
  if (!op) return set_err(-1006, "null handle");
  if (!op->has_K) return set_err(-1000, "operator has no matrix");
  DeviceGuard g(op->device);
  std::vector<double> h((size_t)op->n_pad * RLD, 0.0);
  for (int c0 = 0; c0 < ncol; c0 += RLD) {
    const int nc = std::min(RLD, ncol - c0);
    std::fill(h.begin(), h.end(), 0.0);
    for (int64_t i = 0; i < op->n; ++i)
      for (int c = 0; c < nc; ++c) h[(size_t)i * RLD + c] = x[i * ld + c0 + c];
    HIP_TRY(hipMemcpyAsync(op->scratch, h.data(), sizeof(double) * h.size(),
                           hipMemcpyHostToDevice, op->stream));
    hipLaunchKernelGGL(gemv_sym_kernel, dim3((unsigned)((op->n + 3) / 4)), dim3(256), 0,
                       op->stream, op->K, op->n_pad, op->n, op->scratch, (int64_t)RLD, nc,
                       op->scratch2, 0.0, 1);
    LAUNCH_CHECK("gemv_sym_kernel");
    HIP_TRY(hipMemcpyAsync(h.data(), op->scratch2, sizeof(double) * h.size(),
                           hipMemcpyDeviceToHost, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    for (int64_t i = 0; i < op->n; ++i)
      for (int c = 0; c < nc; ++c) y[i * ldy + c0 + c] = h[(size_t)i * RLD + c];
  }
  return 0;
}

int gpmi_op_trace(gpmi_op* op, double* trace_k, double* trace_k2) {
  if (!op) return set_err(-1006, "null handle");
  if (!op->has_K) return set_err(-1000, "operator has no matrix");
  DeviceGuard g(op->device);
  hipLaunchKernelGGL(trace_kernel, dim3((unsigned)op->n), dim3(256), 0, op->stream, op->K,
                     op->n_pad, op->n, op->tracebuf);
  LAUNCH_CHECK("trace_kernel");
  std::vector<double> h((size_t)op->n * 2);
  HIP_TRY(hipMemcpyAsync(h.data(), op->tracebuf, sizeof(double) * h.size(),
                         hipMemcpyDeviceToHost, op->stream));
  HIP_TRY(hipStreamSynchronize(op->stream));
  double a = 0.0, f = 0.0;
  for (int64_t i = 0; i < op->n; ++i) {
    a += h[2 * i];
    f += h[2 * i + 1];
  }
  if (trace_k) *trace_k = a;
  if (trace_k2) *trace_k2 = f;
  return 0;
}

int gpmi_matern_cross(int device, const double* points, int64_t n, const double* test_points,
                      int64_t nstar, int d, const double* scale, double nu, double* C_out,
                      int64_t ldc) {
  if (!points || !test_points || !scale || !C_out) return set_err(-1004, "null argument");
  if (n < 1 || nstar < 1) return set_err(-1005, "point counts must be positive");
  if (d < 1 || d > GPMI_MAX_DIM)
    return set_err(-1003, "dimension %d outside [1, %d]", d, GPMI_MAX_DIM);
  MaternParams P;
  int rc = matern_params(nu, &P);
  if (rc) return rc;
  DeviceGuard g(device);
  DevBuf<double> dp, dt, ds, dC;
  HIP_TRY(dp.reserve((size_t)n * d));
  HIP_TRY(dt.reserve((size_t)nstar * d));
  HIP_TRY(ds.reserve(d));
  HIP_TRY(dC.reserve((size_t)nstar * n));
  HIP_TRY(hipMemcpy(dp, points, sizeof(double) * n * d, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dt, test_points, sizeof(double) * nstar * d, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ds, scale, sizeof(double) * d, hipMemcpyHostToDevice));
  launch_matern_cross(nullptr, dp, n, dt, nstar, d, ds, P, dC, n, nstar, n);
  LAUNCH_CHECK("matern_cross_kernel");
  HIP_TRY(hipMemcpy2D(C_out, sizeof(double) * ldc, dC, sizeof(double) * n, sizeof(double) * n,
                      nstar, hipMemcpyDeviceToHost));
  return 0;
}

int gpmi_op_set_timing(gpmi_op* op, int enable) {
  if (!op) return set_err(-1006, "null handle");
  op->tim.on = enable != 0;
  return 0;
}

int gpmi_op_set_outer(gpmi_op* op, int s) {
  if (!op) return set_err(-1006, "null handle");
  if (s < 1 || s > 32) return set_err(-1008, "outer panel width %d outside [1, 32]", s);
  op->outer = s;
  return 0;
}

}  // extern "C"

namespace gpmi {
int matern_params_host(double nu, MaternParams* P) { return matern_params(nu, P); }
}  // namespace gpmi
