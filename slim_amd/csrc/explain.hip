// explain.hip -- slim_gpu_explain.h on a device: which history items carry the score of a candidate.  The two calls
// mirror candidates.hip's: host handles (model and histories staged for the call) and a resident model with the
// rows of a staged matrix.  Both end in explain_rows, which makes the set's device copy on first use, launches
// k_explain (explain_kernels.hpp) and brings the outputs down into host images; from them only the first
// min(nwhy, support) places of every slot of a selected user are copied out, so that everything else stays as the
// caller filled it.  The device outputs and their images belong to the candidate set and only grow.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "call_frame.hpp"
#include "explain_kernels.hpp"
#include "host_csr.hpp"

namespace slimamd {
namespace {
constexpr int kStageDefault = 1024, kStageMax = 2048;  // 16 bytes each: 16 KB by default, 32 KB at most

// SLIM_EXPLAIN_STAGE=<entries>: history entries staged in LDS per user (tests put the boundary inside a history)
int stage_entries() {
  const char* s = std::getenv("SLIM_EXPLAIN_STAGE");
  if (!s || !*s) return kStageDefault;
  char* end = nullptr;
  const long v = std::strtol(s, &end, 10);
  if (*end || v < 1) return kStageDefault;
  return (int)std::min<long>(v, kStageMax);
}
// SLIM_EXPLAIN_FORM=16: the kernel with 16 places per lane at every nwhy
bool form16_forced() {
  const char* s = std::getenv("SLIM_EXPLAIN_FORM");
  return s && std::string(s) == "16";
}

// The part the two calls share once the model and the histories are views on `device`.  H.users is ignored:
// h_users (host, ascending; nullptr: users [0, H.nusers)) is uploaded into the set's workspace.
int32_t explain_rows(const char* who, const DeviceRowView& W, HistoryView H, const int32_t* h_users,
                     slimgpu_candset* cs, int device, int num_cus, hipStream_t stream, int32_t nwhy,
                     int32_t* why_items, float* why_terms, int32_t* support, slimgpu_eval_stats_t& st) {
  const std::string w(who);
  if (W.nnz > 0 && !W.rows_sorted)
    return refuse(w + ": the ids of some model row do not ascend strictly: the explanation kernel looks ids up by "
                      "binary search (SLIM_PREDICT=cpu explains any model)");
  if (W.nnz >= (int64_t)1 << 31) return refuse(w + ": the model has 2^31 entries or more");
  if (H.max_hist >= INT32_MAX) return refuse(w + ": a history has 2^31 - 1 entries or more");
  const int32_t nsel = H.nusers;
  const int64_t* cptr = candset_row_pointer(cs);
  int64_t entries = 0;  // of the selected rows
  for (int32_t q = 0; q < nsel; ++q) {
    const int32_t u = h_users ? h_users[q] : q;
    entries += cptr[u + 1] - cptr[u];
  }
  const bool places = why_items != nullptr;
  int set_allocs = 0;
  const CandidateRows rows = candset_on_device(cs, device, num_cus, stream, &set_allocs, &st.h2d_bytes);
  ExplainWorkspace& E = candset_explain_workspace(cs);
  E.allocs = 0;
  // no slicing: the outputs of all selected rows stand in device memory at once
  const size_t want = (size_t)entries * (places ? 8 * (size_t)nwhy + 4 : 4);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (want > (free_b + E.held()) / 2) {
    set_error(w + ": the outputs of " + std::to_string(entries) + " candidate entries at nwhy = " +
              std::to_string(nwhy) + " need " + std::to_string(want) + " bytes of device memory, more than half of "
              "the " + std::to_string(free_b + E.held()) + " that are free: pass user sub-lists");
    return SLIM_ERROR_MEMORY;
  }
  ExplainArgs A = {};
  A.wrows = W.nrows; A.wptr = W.d_ptr; A.wind = W.d_ind; A.wval = W.d_val;
  A.npos = nsel; A.hptr = H.ptr; A.hind = H.ind; A.hval = H.val;
  A.cptr = rows.cptr; A.lptr = rows.lptr; A.pairs = rows.pairs;
  A.nwhy = nwhy;
  A.stage = stage_entries();
  if (h_users) {
    int32_t* d_users = E.need(E.users, (size_t)nsel);
    HIP_TRY(hipMemcpyAsync(d_users, h_users, sizeof(int32_t) * (size_t)nsel, hipMemcpyHostToDevice, stream));
    st.h2d_bytes += (int64_t)(sizeof(int32_t) * (size_t)nsel);
    int64_t* d_obase = E.need(E.obase, (size_t)nsel + 1);
    hipLaunchKernelGGL(k_explain_base, dim3(1), dim3(256), 0, stream, nsel, d_users, rows.cptr, d_obase);
    HIP_TRY(hipGetLastError());
    A.users = d_users;
    A.obase = d_obase;
  }
  A.support = E.need(E.support, (size_t)entries);
  if (places) {
    A.items = E.need(E.items, (size_t)entries * nwhy);
    A.terms = E.need(E.terms, (size_t)entries * nwhy);
  }
  HIP_TRY(hipMemsetAsync(A.support, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(entries, 1), stream));
  EventPair ev;
  ev.begin(stream);
  if (nsel > 0 && entries > 0) {
    const dim3 grid((unsigned)std::min<int64_t>(nsel, (int64_t)num_cus * 8)), block(64 * kExplainWaves);
    const size_t lds = sizeof(int4) * (size_t)A.stage;
    if (std::getenv("SLIM_GPU_TRACE"))
      std::fprintf(stderr, "[trace] k_explain<%d>: %d positions, %d workgroups, %d staged entries, nwhy %d, %s\n",
                   nwhy > 4 || form16_forced() ? 16 : 4, nsel, (int)grid.x, A.stage, nwhy,
                   h_users ? "a user list" : "all users");
    if (nwhy > 4 || form16_forced())
      hipLaunchKernelGGL(k_explain<16>, grid, block, lds, stream, A);
    else
      hipLaunchKernelGGL(k_explain<4>, grid, block, lds, stream, A);
    HIP_TRY(hipGetLastError());
  }
  ev.end(stream);
  size_t down = 0;
  auto fetch = [&](auto& image, const auto* d, size_t n) {
    if (image.size() < n) image.resize(n);
    if (n == 0) return;
    HIP_TRY(hipMemcpyAsync(image.data(), d, sizeof(*d) * n, hipMemcpyDeviceToHost, stream));
    down += sizeof(*d) * n;
  };
  fetch(E.h_support, A.support, (size_t)entries);
  if (places) {
    fetch(E.h_items, A.items, (size_t)entries * nwhy);
    fetch(E.h_terms, A.terms, (size_t)entries * nwhy);
  }
  HIP_TRY(hipStreamSynchronize(stream));
  st.kernel_ms = ev.ms();
  st.d2h_bytes += (int64_t)down;
  st.path = kExplain;
  st.device_allocs = set_allocs + E.allocs;
  // out of the images: the rows of the positions stand side by side there, in the caller's arrays at cptr[user]
  int64_t ob = 0;
  for (int32_t q = 0; q < nsel; ++q) {
    const int32_t u = h_users ? h_users[q] : q;
    const int64_t e0 = cptr[u], len = cptr[u + 1] - e0;
    for (int64_t j = 0; j < len; ++j) {
      const int32_t n = E.h_support[ob + j];
      if (support) support[e0 + j] = n;
      if (!places) continue;
      const int64_t m = std::min<int64_t>(n, nwhy);
      std::copy_n(E.h_items.data() + (ob + j) * nwhy, m, why_items + (e0 + j) * nwhy);
      std::copy_n(E.h_terms.data() + (ob + j) * nwhy, m, why_terms + (e0 + j) * nwhy);
    }
    ob += len;
  }
  return SLIM_OK;
}
}  // namespace

int32_t explain_check(const char* who, int32_t nwhy, const int32_t* why_items, const float* why_terms) {
  const std::string w(who);
  if (nwhy < 1 || nwhy > SLIMGPU_MAX_WHY)
    return refuse(w + ": nwhy must be between 1 and " + std::to_string(SLIMGPU_MAX_WHY) + ", not " +
                  std::to_string(nwhy));
  if ((why_items == nullptr) != (why_terms == nullptr))
    return refuse(w + ": bad arguments (why_items and why_terms go together: both or neither)");
  return SLIM_OK;
}

int32_t explain_candidates(const slim_csr_t* W, const slim_csr_t* trn, slimgpu_candset* cs, int32_t nwhy,
                           int32_t* why_items, float* why_terms, int32_t* support) {
  const char* who = "SLIMGPU_ExplainCandidates";
  if (!W || !trn || !W->rowptr || !trn->rowptr || (!W->rowval && W->rowptr[W->nrows] > 0))
    return refuse(std::string(who) + ": bad arguments (a model with a row view, a history)");
  const int32_t nusers = trn->nrows;
  if (const int32_t rc = explain_check(who, nwhy, why_items, why_terms); rc != SLIM_OK) return rc;
  if (const int32_t rc = candset_check(who, cs, W->ncols, nusers, nullptr, 0, nullptr, nullptr); rc != SLIM_OK)
    return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  return guarded(who, [&]() -> int32_t {
    const int device = open_current_device();
    const int num_cus = cu_count();
    if (nusers > 0) {
      const StagedPair P = stage_pair(W, trn, num_cus);
      const int32_t rc = explain_rows(who, P.W, P.H, nullptr, cs, device, num_cus, /*stream=*/nullptr, nwhy, why_items,
                                      why_terms, support, st);
      if (rc != SLIM_OK) return rc;
      st.w_rows_read = P.h.nnz;
    }
    st.total_ms = ms_since(t_begin);
    last_eval_stats() = st;
    return SLIM_OK;
  });
}

int32_t matrix_explain_candidates(const slimgpu_model* model, slimgpu_matrix_t* mat, slimgpu_candset* cs,
                                  int32_t nusers, const int32_t* users, int32_t nwhy, int32_t* why_items,
                                  float* why_terms, int32_t* support) {
  const char* who = "SLIMGPU_MatrixExplainCandidates";
  DeviceRowView W;
  DeviceCsrView R;
  if (!model || !mat || model_row_view(model, &W) != SLIM_OK || matrix_csr_view(mat, &R) != SLIM_OK)
    return refuse(std::string(who) + ": bad arguments (a resident model with a row view, a staged matrix)");
  if (const int32_t rc = explain_check(who, nwhy, why_items, why_terms); rc != SLIM_OK) return rc;
  if (const int32_t rc = check_user_list(who, nusers, users, R.nrows); rc != SLIM_OK) return rc;
  if (const int32_t rc = check_pair(who, R, W); rc != SLIM_OK) return rc;
  const int32_t nu = users ? nusers : R.nrows;
  if (const int32_t rc = candset_check(who, cs, W.ncols, nu, users, 0, nullptr, nullptr); rc != SLIM_OK) return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  return guarded(who, [&]() -> int32_t {
    hipStream_t stream = open_device(R);
    if (nu > 0) {
      // (a history of any length below 2^31 - 1 is served: only a matrix that could hold a longer one is measured)
      const int64_t max_hist = R.nnz < INT32_MAX ? 0 : longest_history(stream, R.num_cus, R.nrows, nullptr, R.d_ptr, nullptr);
      const HistoryView H = resident_history(R, nu, nullptr, max_hist);
      const int32_t rc = explain_rows(who, W, H, users, cs, R.device, R.num_cus, stream, nwhy, why_items, why_terms,
                                      support, st);
      if (rc != SLIM_OK) return rc;
      st.w_rows_read = R.nnz;
    }
    st.total_ms = ms_since(t_begin);
    last_eval_stats() = st;
    return SLIM_OK;
  });
}
}  // namespace slimamd
