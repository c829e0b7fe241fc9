// filter.hip -- the candidate filter of the top-N lists (slim_gpu_filter.h): the object behind
// slimgpu_filter_t.  It validates its input once and keeps the host description -- a bitmap of one bit per
// item (set = may be recommended) and the exclusion CSR over user ids -- which the host scorer reads
// (host_csr.cpp: top_n_filtered).  The device scorers read a copy that filter_on_device makes on the first call
// that scores on a device and that stays until the filter is freed; nothing here needs a device before that.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "host_csr.hpp"
#include "host_stage.hpp"
#include "scorer.hpp"

struct slimgpu_filter {
  int32_t ncols = 0, xusers = 0;
  bool has_bits = false, has_rows = false;
  std::vector<uint32_t> bits;  // (ncols + 31) / 32 words, at least one
  std::vector<int64_t> xptr;   // xusers + 1
  std::vector<int32_t> xind;
  // the copy on `device` (-1: none yet)
  int device = -1;
  slimamd::DeviceBuffer<uint32_t> d_bits;
  slimamd::DeviceBuffer<int64_t> d_xptr;
  slimamd::DeviceBuffer<int32_t> d_xind;
};

namespace slimamd {
slimgpu_filter* filter_create(int32_t ncols, int32_t nitems, const int32_t* items, int32_t blocked, int32_t xusers,
                              const int64_t* xptr, const int32_t* xind, int32_t* status) {
  auto bad = [&](const std::string& why) {
    *status = refuse("SLIMGPU_FilterCreate: " + why);
    return static_cast<slimgpu_filter*>(nullptr);
  };
  if (ncols < 0 || nitems < 0 || (nitems > 0 && !items)) return bad("bad arguments (ncols >= 0, nitems ids)");
  if (xptr && xusers < 0) return bad("bad arguments (xusers >= 0)");
  for (int32_t j = 0; j < nitems; ++j)
    if (items[j] < 0 || items[j] >= ncols)
      return bad("item id " + std::to_string(items[j]) + " is outside [0, " + std::to_string(ncols) + ")");
  if (xptr) {
    if (xptr[0] != 0) return bad("xptr[0] is not 0");
    for (int32_t u = 0; u < xusers; ++u)
      if (xptr[u + 1] < xptr[u]) return bad("xptr does not ascend at user " + std::to_string(u));
    if (xptr[xusers] > 0 && !xind) return bad("exclusion rows without xind");
    for (int64_t x = 0; x < xptr[xusers]; ++x)
      if (xind[x] < 0 || xind[x] >= ncols)
        return bad("excluded id " + std::to_string(xind[x]) + " is outside [0, " + std::to_string(ncols) + ")");
  }
  try {
    slimgpu_filter* f = new slimgpu_filter;
    f->ncols = ncols;
    f->has_bits = blocked ? nitems > 0 : items != nullptr;
    if (f->has_bits) {
      const size_t words = ((size_t)ncols + 31) / 32;
      f->bits.assign(words ? words : 1, blocked ? ~0u : 0u);
      for (int32_t j = 0; j < nitems; ++j) {
        const uint32_t bit = 1u << (items[j] & 31);
        if (blocked) f->bits[items[j] >> 5] &= ~bit; else f->bits[items[j] >> 5] |= bit;
      }
    }
    f->has_rows = xptr != nullptr;
    if (f->has_rows) {
      f->xusers = xusers;
      f->xptr.assign(xptr, xptr + xusers + 1);
      f->xind.assign(xind, xind + xptr[xusers]);
    }
    *status = SLIM_OK;
    return f;
  } catch (const std::bad_alloc&) {
    set_error("SLIMGPU_FilterCreate: out of host memory");
    *status = SLIM_ERROR_MEMORY;
    return nullptr;
  }
}

void filter_free(slimgpu_filter* f) { delete f; }

HostFilter filter_host(const slimgpu_filter* f) {
  HostFilter h;
  if (!f) return h;
  h.ncols = f->ncols;
  if (f->has_bits) h.bits = f->bits.data();
  if (f->has_rows) {
    h.xusers = f->xusers;
    h.xptr = f->xptr.data();
    h.xind = f->xind.data();
  }
  return h;
}

int32_t filter_check(const char* who, const slimgpu_filter* f, int32_t model_ncols) {
  if (!f || f->ncols == model_ncols) return SLIM_OK;
  return refuse(std::string(who) + ": the filter was made for " + std::to_string(f->ncols) + " items, the model has " +
                std::to_string(model_ncols));
}

CandidateFilter filter_on_device(slimgpu_filter* f, int device, hipStream_t stream, int* allocs, int64_t* h2d) {
  CandidateFilter F;
  if (!f || (!f->has_bits && !f->has_rows)) return F;
  if (f->device != device) {  // first use here: the copy of another device goes
    f->d_bits.reset(); f->d_xptr.reset(); f->d_xind.reset();
    f->device = -1;
    auto put = [&](auto& buf, const auto& host) {
      using T = std::remove_reference_t<decltype(host[0])>;
      buf.reserve(host.size());
      if (allocs) ++*allocs;
      if (!host.empty()) {
        HIP_TRY(hipMemcpyAsync(buf.get(), host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice, stream));
        if (h2d) *h2d += (int64_t)(sizeof(T) * host.size());
      }
    };
    if (f->has_bits) put(f->d_bits, f->bits);
    if (f->has_rows) {
      put(f->d_xptr, f->xptr);
      put(f->d_xind, f->xind);
    }
    HIP_TRY(hipStreamSynchronize(stream));
    f->device = device;
  }
  if (f->has_bits) F.bits = f->d_bits.get();
  if (f->has_rows) {
    F.xptr = f->d_xptr.get(); F.xind = f->d_xind.get(); F.xusers = f->xusers;
  }
  return F;
}
}  // namespace slimamd
