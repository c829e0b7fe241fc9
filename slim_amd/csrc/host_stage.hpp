// host_stage.hpp -- what the scorers' host code (topn.hip, resident_eval.hip, eval.hip) shares: the rows of a host CSR staged
// in device memory, the report of a HIP failure, the CU count of the current device.  What an entry point is
// framed by (the error boundary, the event pair, the staged users and the staged host pair) is call_frame.hpp's.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>

#include "hip_check.hpp"
#include "host_csr.hpp"

namespace slimamd {

// The first rows of a host CSR in device memory.  Owns its buffers.
struct StagedCsr {
  DeviceBuffer<int64_t> ptr;
  DeviceBuffer<int32_t> ind;
  DeviceBuffer<float> val;  // empty (get() == nullptr) when values were not wanted or the matrix has none
  int64_t nnz = 0, max_row = 0;  // max_row: entries of the longest row
};

// Rows [0, nrows) of m.  stream == nullptr: blocking copies; else the copies are queued on it (from
// pageable memory: they have left the caller's arrays when the call returns).
inline StagedCsr stage_csr(const slim_csr_t* m, int32_t nrows, bool values, hipStream_t stream) {
  static_assert(sizeof(ssize_t) == sizeof(int64_t), "LP64 expected");
  auto put = [&](void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return;
    if (stream)
      HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    else
      HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  };
  StagedCsr s;
  s.nnz = m->rowptr[nrows];
  for (int32_t r = 0; r < nrows; ++r) s.max_row = std::max<int64_t>(s.max_row, m->rowptr[r + 1] - m->rowptr[r]);
  s.ptr = DeviceBuffer<int64_t>((size_t)nrows + 1);
  s.ind = DeviceBuffer<int32_t>((size_t)s.nnz);
  put(s.ptr.get(), m->rowptr, sizeof(int64_t) * ((size_t)nrows + 1));
  put(s.ind.get(), m->rowind, sizeof(int32_t) * (size_t)s.nnz);
  if (values && m->rowval) {
    s.val = DeviceBuffer<float>((size_t)s.nnz);
    put(s.val.get(), m->rowval, sizeof(float) * (size_t)s.nnz);
  }
  return s;
}

// a refusal of the caller's input: the message for last_error(), the status to return
inline int32_t refuse(const std::string& why) {
  set_error(why);
  return SLIM_ERROR_INPUT;
}

inline int32_t hip_failure(const char* who, const HipFail& e) {
  set_error(std::string(who) + ": HIP error '" + hipGetErrorString(e.code) + "' in " + e.where);
  return status_of(e);
}

inline int cu_count() {
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
  return prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
}

}  // namespace slimamd
