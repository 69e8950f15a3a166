// DevBuf: one owned device allocation -- a pointer and its capacity in bytes. The only place device
// memory of the context is freed: always after a device sync, and a buffer whose grow failed is
// empty (ptr == nullptr, cap == 0), safe to grow again or to destroy. No minimum size, no rounding.
// A: the allocator policy (alloc / free / sync / free_bytes); HipAlloc for the library, a fake for
// the host tests.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <utility>

namespace smaml {

struct HipAlloc {
  static hipError_t alloc(void** p, int64_t bytes) {
    const hipError_t e = hipMalloc(p, (size_t)bytes);
    if (e != hipSuccess) (void)hipGetLastError();  // reported through the status, not left sticky
    return e;
  }
  static hipError_t free(void* p) { return hipFree(p); }
  static hipError_t sync() { return hipDeviceSynchronize(); }
  static int64_t free_bytes() {
    size_t freeb = 0, totb = 0;
    if (hipMemGetInfo(&freeb, &totb) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    return (int64_t)freeb;
  }
};

template <class A>
struct DevBuf {
  void* ptr = nullptr;
  int64_t cap = 0;  // bytes

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), cap(o.cap) {
    o.ptr = nullptr;
    o.cap = 0;
  }
  ~DevBuf() { (void)release(); }

  template <class T>
  T* as() const {
    return static_cast<T*>(ptr);
  }

  hipError_t release() {
    if (!ptr) return hipSuccess;
    const hipError_t es = A::sync(), ef = A::free(ptr);
    ptr = nullptr;
    cap = 0;
    return es != hipSuccess ? es : ef;
  }

  // Room for `bytes`: the buffer as it is when it suffices (contents kept), else a fresh one (contents lost).
  hipError_t grow(int64_t bytes) {
    if (bytes <= cap) return hipSuccess;
    hipError_t e = release();
    if (e != hipSuccess) return e;
    e = A::alloc(&ptr, bytes);
    if (e == hipSuccess)
      cap = bytes;
    else
      ptr = nullptr;
    return e;
  }

  // Best effort: grows only while more than `margin` bytes would stay free. Whether the buffer has the room.
  bool grow_if_room(int64_t bytes, int64_t margin) {
    if (bytes <= cap) return true;
    (void)release();  // (its bytes count as free for the new one)
    return A::free_bytes() > bytes + margin && grow(bytes) == hipSuccess;
  }
};

// Buffers that are only usable together: all grown, or all empty.
template <class A>
hipError_t grow_all(std::initializer_list<std::pair<DevBuf<A>*, int64_t>> group) {
  for (auto& b : group) {
    const hipError_t e = b.first->grow(b.second);
    if (e == hipSuccess) continue;
    for (auto& x : group) (void)x.first->release();
    return e;
  }
  return hipSuccess;
}

}  // namespace smaml
