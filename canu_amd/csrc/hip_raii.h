// hip_raii.h -- device memory and events that are released on every way out.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
  hipError_t alloc(size_t n) {
    release();
    bytes = std::max<size_t>(n, 1) * sizeof(T);
    return hipMalloc((void **)&p, bytes);
  }
  // grow-only: an allocation that already holds n elements is kept, with its contents
  hipError_t reserve(size_t n) {
    if (p && n * sizeof(T) <= bytes) return hipSuccess;
    return alloc(n);
  }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipError_t create() { return hipEventCreate(&e); }
  operator hipEvent_t() const { return e; }
};
