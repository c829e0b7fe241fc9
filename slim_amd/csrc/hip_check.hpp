// hip_check.hpp -- the HIP error type and the owning device buffer of the host code.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>

#include "../../include/slim.h"

namespace slimamd {

struct HipFail {
  hipError_t code;
  std::string where;
};

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) throw ::slimamd::HipFail{_e, std::string(#expr)};        \
  } while (0)

inline int32_t status_of(const HipFail& e) {
  return e.code == hipErrorOutOfMemory ? SLIM_ERROR_MEMORY : SLIM_ERROR;
}

// n elements of T in device memory (at least one), freed by the destructor.  Move-only.
template <class T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  explicit DeviceBuffer(size_t n) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * (n ? n : 1)));
    bytes_ = sizeof(T) * (n ? n : 1);
  }
  ~DeviceBuffer() { reset(); }
  DeviceBuffer(DeviceBuffer&& o) noexcept
      : p(std::exchange(o.p, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;

  T* get() const { return p; }
  size_t bytes() const { return bytes_; }
  T* release() {
    bytes_ = 0;
    return std::exchange(p, nullptr);
  }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes_ = 0;
  }

  // Grow-only workspace: keeps the buffer when it holds n elements already, else replaces it (the
  // contents are lost).  On out-of-memory, `evict()` may free something else and return true; the
  // allocation is then tried once more.
  T* reserve(size_t n) {
    return reserve(n, [] { return false; });
  }
  template <class Evict>
  T* reserve(size_t n, Evict&& evict) {
    const size_t need = sizeof(T) * (n ? n : 1);
    if (bytes_ >= need) return p;
    if (p) HIP_TRY(hipFree(p));
    p = nullptr;
    bytes_ = 0;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), need);
    if (e == hipErrorOutOfMemory && evict()) {
      (void)hipGetLastError();
      e = hipMalloc(reinterpret_cast<void**>(&p), need);
    }
    if (e != hipSuccess) {
      p = nullptr;
      throw HipFail{e, "hipMalloc(workspace)"};
    }
    bytes_ = need;
    return p;
  }

 private:
  T* p = nullptr;
  size_t bytes_ = 0;
};

}  // namespace slimamd
