// Host-side helpers of the C-ABI translation units (gpmi_api.hip, gpmi_dense_*.hip,
// gpmi_sparse_api.hip, gpmi_sparse_assemble.hip, gpmi_sparse_spmm.hip,
// gpmi_sparse_lanczos.hip, gpmi_sparse_cg.hip, gpmi_band_*.hip): the HIP error checks, the
// device guard and the owners of device allocations, pinned host memory, streams and events.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <initializer_list>
#include <utility>
#include <vector>

namespace gpmi {

int set_error(int code, const char* msg);   // gpmi_api.hip: the thread's last error

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      char b_[400];                                                                    \
      snprintf(b_, sizeof(b_), "%s failed: %s", #expr, hipGetErrorString(e_));        \
      return ::gpmi::set_error(-(int)e_, b_);                                          \
    }                                                                                  \
  } while (0)

#define LAUNCH_CHECK(name)                                                             \
  do {                                                                                 \
    hipError_t e_ = hipGetLastError();                                                 \
    if (e_ != hipSuccess) {                                                            \
      char b_[400];                                                                    \
      snprintf(b_, sizeof(b_), "launch of %s failed: %s", name, hipGetErrorString(e_)); \
      return ::gpmi::set_error(-(int)e_, b_);                                          \
    }                                                                                  \
  } while (0)

// (internal to the library: none of this is an exported symbol)
#pragma GCC visibility push(hidden)

// set_error with a printf-style message (gpmi_api.hip).
int set_errorf(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Makes `dev` the current device for a scope.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Owner of one device allocation (move-only).
struct DevMem {
  void* p = nullptr;
  size_t bytes = 0;

  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevMem& operator=(DevMem&& o) noexcept {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~DevMem() { (void)release(); }

  hipError_t release() {
    hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr;
    bytes = 0;
    return e;
  }
  // Grow-only. The old block is freed before the new one is allocated, so the peak is
  // the larger of the two and not their sum; a failed allocation leaves the buffer empty.
  hipError_t reserve_bytes(size_t n) {
    if (n <= bytes) return hipSuccess;
    hipError_t e = release();
    if (e != hipSuccess) return e;
    if ((e = hipMalloc(&p, n)) != hipSuccess) {
      p = nullptr;
      return e;
    }
    bytes = n;
    return hipSuccess;
  }
};

// ... of T: used as the T* it holds, sized in elements.
template <class T>
struct DevBuf : DevMem {
  operator T*() const { return static_cast<T*>(p); }
  hipError_t reserve(size_t count) { return reserve_bytes(sizeof(T) * count); }
};

// Owner of one pinned host allocation (hipHostMalloc with `flags`).
struct PinnedMem {
  void* p = nullptr;
  PinnedMem() = default;
  PinnedMem(const PinnedMem&) = delete;
  PinnedMem& operator=(const PinnedMem&) = delete;
  ~PinnedMem() { (void)release(); }
  hipError_t release() {
    hipError_t e = p ? hipHostFree(p) : hipSuccess;
    p = nullptr;
    return e;
  }
  hipError_t alloc(size_t bytes, unsigned flags) {
    hipError_t e = release();
    if (e != hipSuccess) return e;
    if ((e = hipHostMalloc(&p, bytes, flags)) != hipSuccess) p = nullptr;
    return e;
  }
};

// Owner of a stream or an event (created into h by the HIP call that fits).
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
  H h = nullptr;
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { (void)release(); }
  // Destroys the handle now (none afterwards, until it is created again).
  hipError_t release() {
    hipError_t e = h ? Destroy(h) : hipSuccess;
    h = nullptr;
    return e;
  }
  operator H() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// Events created on demand and kept: reserve(n, flags) makes [0, n) exist.
struct EventPool {
  std::vector<hipEvent_t> ev;
  EventPool() = default;
  EventPool(const EventPool&) = delete;
  EventPool& operator=(const EventPool&) = delete;
  ~EventPool() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  hipError_t reserve(size_t n, unsigned flags) {
    while (ev.size() < n) {
      hipEvent_t e;
      hipError_t rc = hipEventCreateWithFlags(&e, flags);
      if (rc != hipSuccess) return rc;
      ev.push_back(e);
    }
    return hipSuccess;
  }
  hipEvent_t operator[](size_t i) const { return ev[i]; }
};

// Buffers that share one capacity (in whatever unit the sizes were worked out for):
// grown together to hold `want`. All of them are freed before the first is allocated
// again, in the order given, so the group's peak is its new size alone; after a failure
// the capacity is 0 and the next call starts over.
struct Sized {
  DevMem* buf;
  size_t bytes;
};
template <class T>
Sized sized(DevBuf<T>& b, size_t count) {
  return {&b, sizeof(T) * count};
}
inline hipError_t regrow(int* cap, int want, std::initializer_list<Sized> bufs) {
  if (*cap >= want) return hipSuccess;
  *cap = 0;
  hipError_t e;
  for (const Sized& b : bufs)
    if ((e = b.buf->release()) != hipSuccess) return e;
  for (const Sized& b : bufs)
    if ((e = b.buf->reserve_bytes(b.bytes)) != hipSuccess) return e;
  *cap = want;
  return hipSuccess;
}

#pragma GCC visibility pop

}  // namespace gpmi
