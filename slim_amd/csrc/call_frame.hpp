// call_frame.hpp -- the frame that every device entry point of the scorers' host code stands in (resident_eval.hip,
// candidates.hip, explain.hip, topn.hip, eval.hip, cand_sample.hip, exposure.hip).  An entry point writes its own
// argument checks and its own middle; from here it gets the error boundary (guarded), the device of the call
// (open_device / open_current_device), a pair of events (EventPair), the users of a staged matrix as histories
// (stage_users) and a host model with a host history as views (stage_pair and its parts).
#pragma once

#include <new>
#include <string>

#include "host_stage.hpp"
#include "scorer.hpp"

namespace slimamd {

// The one error boundary: runs body() and returns its status; a HIP failure inside it becomes hip_failure(who, e),
// an allocation that the host refuses "<who>: out of host memory" with SLIM_ERROR_MEMORY.
template <class Body>
int32_t guarded(const char* who, Body&& body) {
  try {
    return body();
  } catch (const HipFail& e) {
    return hip_failure(who, e);
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return SLIM_ERROR_MEMORY;
  }
}

// The device of a call on a staged matrix: an earlier call's failure is not this one's, the handle's device is
// current, the handle's stream is the call's.
inline hipStream_t open_device(const DeviceCsrView& R) {
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(R.device));
  return static_cast<hipStream_t>(R.stream);
}
// The device of a call on host handles: the current one (the null stream is the call's).
inline int open_current_device() {
  (void)hipGetLastError();
  int ndev = 0, device = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0) throw HipFail{hipErrorNoDevice, "hipGetDeviceCount"};
  HIP_TRY(hipGetDevice(&device));
  return device;
}

// Two events around a piece of a stream's work, destroyed on every way out.
struct EventPair {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  EventPair() {
    HIP_TRY(hipEventCreate(&ev0));
    if (const hipError_t e = hipEventCreate(&ev1); e != hipSuccess) {
      (void)hipEventDestroy(ev0);
      throw HipFail{e, "hipEventCreate(&ev1)"};
    }
  }
  ~EventPair() {
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
  }
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  void begin(hipStream_t stream) { HIP_TRY(hipEventRecord(ev0, stream)); }
  void end(hipStream_t stream) { HIP_TRY(hipEventRecord(ev1, stream)); }
  float ms() const {  // (the stream has run)
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    return ms;
  }
};

// The users of a call on a staged matrix: `nu` (at least one) positions, `users` their rows (host, ascending; nullptr:
// the first rows).  The list's device copy, queued on `stream`, and the histories with the longest one measured (4
// bytes down, the stream drained).  *allocs grows by one for that length and by one for the list, *h2d (optional) by
// the list's bytes.
struct StagedUsers {
  DeviceBuffer<int32_t> d_users;
  HistoryView H;
};
inline StagedUsers stage_users(const DeviceCsrView& R, int32_t nu, const int32_t* users, hipStream_t stream,
                               int* allocs, int64_t* h2d = nullptr) {
  StagedUsers S;
  ++*allocs;
  if (users) {  // (pageable source: the copy has left the caller's array before the scorer is queued)
    S.d_users = DeviceBuffer<int32_t>((size_t)nu);
    ++*allocs;
    HIP_TRY(hipMemcpyAsync(S.d_users.get(), users, sizeof(int32_t) * (size_t)nu, hipMemcpyHostToDevice, stream));
    if (h2d) *h2d += (int64_t)(sizeof(int32_t) * (size_t)nu);
  }
  S.H = resident_history(R, nu, S.d_users.get(),
                         longest_history(stream, R.num_cus, nu, S.d_users.get(), R.d_ptr, nullptr));
  return S;
}

// A staged host model as the scorer's row view (rows_sorted: not known yet) and the staged rows of a host history
// as histories.
inline DeviceRowView staged_row_view(const slim_csr_t* W, const StagedCsr& w) {
  DeviceRowView V;
  V.nrows = W->nrows; V.ncols = W->ncols; V.nnz = w.nnz; V.max_row = w.max_row;
  V.d_ptr = w.ptr.get(); V.d_ind = w.ind.get(); V.d_val = w.val.get();
  return V;
}
inline HistoryView staged_history(const StagedCsr& h, int32_t nusers) {
  HistoryView H;
  H.nusers = nusers; H.max_hist = h.max_row;
  H.ptr = h.ptr.get(); H.ind = h.ind.get(); H.val = h.val.get();
  return H;
}
// the row order of a view decided once: a model without entries has none to check and stays unsorted
inline void decide_row_order(DeviceRowView& V, int num_cus) {
  if (!V.rows_sorted && V.nnz > 0) V.rows_sorted = rows_ascend_strictly(num_cus, V.nrows, V.d_ptr, V.d_ind);
}
// A host model and every row of a host history on the current device (blocking copies), as views.
struct StagedPair {
  StagedCsr w, h;
  DeviceRowView W;
  HistoryView H;
};
inline StagedPair stage_pair(const slim_csr_t* W, const slim_csr_t* hist, int num_cus) {
  StagedPair P;
  P.w = stage_csr(W, W->nrows, /*values=*/true, /*stream=*/nullptr);
  P.h = stage_csr(hist, hist->nrows, /*values=*/true, /*stream=*/nullptr);
  P.W = staged_row_view(W, P.w);
  decide_row_order(P.W, num_cus);
  P.H = staged_history(P.h, hist->nrows);
  return P;
}

}  // namespace slimamd
