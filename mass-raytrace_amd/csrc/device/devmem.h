// devmem.h — DevBuf<T>, the one owner of a device allocation (hipMalloc /
// hipFree appear nowhere else). Move-only; it frees on the device that is
// current when it is destroyed or freed. alloc and reserve return the
// hipError_t for the caller's own check macro (HIP_CHECK, HIPF, BUILD_CHECK);
// after a failure the buffer is empty, never a pointer with a stale count.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;  // elements

  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      (void)free();
      p = o.p, n = o.n;
      o.p = nullptr, o.n = 0;
    }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)free(); }

  // Frees what it holds, then allocates exactly `count` elements (none for 0).
  hipError_t alloc(size_t count) {
    hipError_t e = free();
    if (e != hipSuccess || count == 0) return e;
    e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess)
      n = count;
    else
      p = nullptr;
    return e;
  }
  // At least `count` elements; growing does not keep the old contents.
  hipError_t reserve(size_t count) { return count <= n ? hipSuccess : alloc(count); }
  hipError_t free() {
    T* old = p;
    p = nullptr, n = 0;
    return old ? hipFree(old) : hipSuccess;
  }
};
