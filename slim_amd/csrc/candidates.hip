// candidates.hip -- per-user candidate sets (slim_gpu_cand.h): the object behind slimgpu_candset_t and the calls
// that score its rows on a device.  The object validates its input once and keeps the host description, a CSR over
// user ids taken as it is given, which the host scorer reads (host_csr.cpp: score_candidates_host).  The device
// scorer (topn_kernels.hpp: CandMode) reads a copy that candset_on_device makes on the first call that scores on a
// device: the rows as given and, per row, the live entries sorted by id with their slot.  Nothing here needs a
// device before that.  A set born on the device (cand_sample.hip) arrives with its rows in place: candset_adopt
// runs the same index step on them and the host keeps the row pointer only, the ids until somebody asks.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <chrono>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "call_frame.hpp"
#include "host_csr.hpp"

struct slimgpu_candset {
  int32_t ncols = 0, nusers = 0;
  std::vector<int64_t> cptr;  // nusers + 1
  std::vector<int32_t> cind;
  bool host_ids = true;  // cind holds the ids (a set born on the device fetches them on first need)
  // the copy on `device` (-1: none yet)
  int device = -1;
  slimamd::DeviceBuffer<int64_t> d_cptr, d_lptr;
  slimamd::DeviceBuffer<int32_t> d_cind;
  slimamd::DeviceBuffer<int2> d_pairs;
  slimamd::ExplainWorkspace why;  // explain.hip: the outputs of the explanations of this set's rows, on `device`
};

namespace slimamd {
namespace {
// key = row << 32 | id, payload = slot; an id outside [0, ncols) gets the key of a row behind the last, so that it
// never enters a row of the device form.  One wavefront per row, its lanes over the entries.
__global__ void k_cand_keys(int32_t nrows, int32_t ncols, const int64_t* __restrict__ cptr,
                            const int32_t* __restrict__ cind, unsigned long long* __restrict__ keys,
                            uint32_t* __restrict__ slots) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < nrows; r += nwaves) {
    const int64_t c0 = cptr[r], c1 = cptr[r + 1];
    for (int64_t e = c0 + lane; e < c1; e += 64) {
      const int32_t id = cind[e];
      const bool in = id >= 0 && id < ncols;
      keys[e] = in ? ((unsigned long long)r << 32) | (uint32_t)id : (unsigned long long)nrows << 32;
      slots[e] = (uint32_t)(e - c0);
    }
  }
}

// after the stable sort a run of equal (row, id) keeps the order of its slots: the last of it is live
__global__ void k_cand_flags(int64_t n, int32_t nrows, const unsigned long long* __restrict__ keys,
                             uint8_t* __restrict__ flags) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long k = keys[p];
    flags[p] = (k >> 32) < (unsigned long long)nrows && (p + 1 == n || keys[p + 1] != k);
  }
}

__global__ void k_cand_pairs(int64_t nlive, const unsigned long long* __restrict__ keys,
                             const uint32_t* __restrict__ slots, int2* __restrict__ pairs) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nlive; p += (int64_t)gridDim.x * blockDim.x)
    pairs[p] = make_int2((int)(uint32_t)keys[p], (int)slots[p]);
}

// lptr[r] = live entries of the rows before r (the live keys ascend: a binary search per row)
__global__ void k_cand_rowptr(int32_t nrows, int64_t nlive, const unsigned long long* __restrict__ keys,
                              int64_t* __restrict__ lptr) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= nrows; r += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long bound = (unsigned long long)r << 32;
    int64_t lo = 0, hi = nlive;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < bound) lo = mid + 1; else hi = mid;
    }
    lptr[r] = lo;
  }
}

unsigned grid_of(int64_t n, int num_cus) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)num_cus * 16));
}
}  // namespace

slimgpu_candset* candset_create(int32_t ncols, int32_t nusers, const int64_t* cptr, const int32_t* cind,
                                int32_t* status) {
  auto bad = [&](const std::string& why) {
    *status = refuse("SLIMGPU_CandSetCreate: " + why);
    return static_cast<slimgpu_candset*>(nullptr);
  };
  if (ncols < 1) return bad("ncols must be at least 1, not " + std::to_string(ncols));
  if (nusers < 0 || !cptr) return bad("bad arguments (nusers >= 0, a row pointer)");
  if (cptr[0] != 0) return bad("cptr[0] is not 0");
  for (int32_t u = 0; u < nusers; ++u) {
    if (cptr[u + 1] < cptr[u]) return bad("cptr does not ascend at user " + std::to_string(u));
    if (cptr[u + 1] - cptr[u] > INT32_MAX) return bad("the row of user " + std::to_string(u) + " has 2^31 entries or more");
  }
  if (cptr[nusers] > 0 && !cind) return bad("candidate rows without cind");
  std::unique_ptr<slimgpu_candset> cs;
  *status = guarded("SLIMGPU_CandSetCreate", [&]() -> int32_t {
    cs.reset(new slimgpu_candset);
    cs->ncols = ncols;
    cs->nusers = nusers;
    cs->cptr.assign(cptr, cptr + nusers + 1);
    cs->cind.assign(cind, cind + cptr[nusers]);
    return SLIM_OK;
  });
  return *status == SLIM_OK ? cs.release() : nullptr;
}

void candset_free(slimgpu_candset* cs) { delete cs; }

HostCandSet candset_host(const slimgpu_candset* cs) {
  HostCandSet h;
  if (!cs) return h;
  h.ncols = cs->ncols; h.nusers = cs->nusers;
  h.cptr = cs->cptr.data(); h.cind = cs->cind.data();
  return h;
}

int32_t candset_check(const char* who, const slimgpu_candset* cs, int32_t model_ncols, int32_t nsel,
                      const int32_t* users, int32_t nrcmds, const int32_t* output, const float* scores) {
  const std::string w(who);
  if (!cs) return refuse(w + ": bad arguments (a candidate set)");
  if (nrcmds < 0 || (nrcmds > 0 && (!output || !scores)))
    return refuse(w + ": bad arguments (nrcmds >= 0, output arrays for the lists)");
  if (cs->ncols != model_ncols)
    return refuse(w + ": the candidate set was made for " + std::to_string(cs->ncols) + " items, the model has " +
                  std::to_string(model_ncols));
  const int32_t last = nsel <= 0 ? -1 : (users ? users[nsel - 1] : nsel - 1);  // (a user list ascends)
  if (last >= cs->nusers)
    return refuse(w + ": the candidate set has " + std::to_string(cs->nusers) + " rows, user " + std::to_string(last) +
                  " is selected");
  if (nrcmds > 0)
    for (int32_t q = 0; q < nsel; ++q) {
      const int32_t u = users ? users[q] : q;
      if (cs->cptr[u + 1] - cs->cptr[u] > SLIMGPU_MAX_LIST)
        return refuse(w + ": the candidate row of user " + std::to_string(u) + " has " +
                      std::to_string(cs->cptr[u + 1] - cs->cptr[u]) + " entries: lists need rows of at most " +
                      std::to_string(SLIMGPU_MAX_LIST) + " (scores alone take rows of any length)");
    }
  return SLIM_OK;
}

namespace {
// The index half of a set's device copy, which an uploaded set and a device-born one (cand_sample.hip) share:
// d_cptr and d_cind hold the rows on the current device; d_lptr and d_pairs are made from them -- per row the live
// entries sorted by id with their slot (k_cand_keys, the stable radix sort, the live pairs).  Drains `stream`.
void candset_index(slimgpu_candset* cs, int num_cus, hipStream_t stream, int* allocs) {
  const int64_t n = cs->cptr[cs->nusers];
  const int32_t nrows = cs->nusers;
  cs->d_lptr.reserve((size_t)nrows + 1);
  if (allocs) ++*allocs;
  HIP_TRY(hipMemsetAsync(cs->d_lptr.get(), 0, sizeof(int64_t) * ((size_t)nrows + 1), stream));
  int64_t nlive = 0;
  if (n > 0) {
    // the sort's buffers live for this block only
    DeviceBuffer<unsigned long long> k_in((size_t)n), k_out((size_t)n), count(1);
    DeviceBuffer<uint32_t> s_in((size_t)n), s_out((size_t)n);
    DeviceBuffer<uint8_t> flags((size_t)n);
    if (allocs) *allocs += 7;
    hipLaunchKernelGGL(k_cand_keys, dim3(grid_of((int64_t)nrows * 64, num_cus)), dim3(256), 0, stream, nrows,
                       cs->ncols, cs->d_cptr.get(), cs->d_cind.get(), k_in.get(), s_in.get());
    HIP_TRY(hipGetLastError());
    unsigned bits = 33;  // the ids, and the rows up to nrows itself
    while (bits < 64 && (1ull << (bits - 32)) <= (unsigned long long)nrows) ++bits;
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, k_in.get(), k_out.get(), s_in.get(), s_out.get(),
                                      (size_t)n, 0u, bits, stream));
    size_t sel_bytes = 0, sel2_bytes = 0;
    HIP_TRY(rocprim::select(nullptr, sel_bytes, k_out.get(), flags.get(), k_in.get(), count.get(), (size_t)n,
                            stream));
    HIP_TRY(rocprim::select(nullptr, sel2_bytes, s_out.get(), flags.get(), s_in.get(), count.get(), (size_t)n,
                            stream));
    DeviceBuffer<char> tmp(std::max(tmp_bytes, std::max(sel_bytes, sel2_bytes)));
    if (allocs) ++*allocs;
    HIP_TRY(rocprim::radix_sort_pairs(tmp.get(), tmp_bytes, k_in.get(), k_out.get(), s_in.get(), s_out.get(),
                                      (size_t)n, 0u, bits, stream));
    hipLaunchKernelGGL(k_cand_flags, dim3(grid_of(n, num_cus)), dim3(256), 0, stream, n, nrows, k_out.get(),
                       flags.get());
    HIP_TRY(hipGetLastError());
    // the live entries, in order, back into the input buffers
    HIP_TRY(rocprim::select(tmp.get(), sel_bytes, k_out.get(), flags.get(), k_in.get(), count.get(), (size_t)n,
                            stream));
    HIP_TRY(rocprim::select(tmp.get(), sel2_bytes, s_out.get(), flags.get(), s_in.get(), count.get(), (size_t)n,
                            stream));
    unsigned long long h_count = 0;
    HIP_TRY(hipMemcpyAsync(&h_count, count.get(), sizeof(h_count), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    nlive = (int64_t)h_count;
    cs->d_pairs.reserve((size_t)nlive);
    if (allocs) ++*allocs;
    if (nlive > 0) {
      hipLaunchKernelGGL(k_cand_pairs, dim3(grid_of(nlive, num_cus)), dim3(256), 0, stream, nlive, k_in.get(),
                         s_in.get(), cs->d_pairs.get());
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_cand_rowptr, dim3(grid_of((int64_t)nrows + 1, num_cus)), dim3(256), 0, stream, nrows,
                         nlive, k_in.get(), cs->d_lptr.get());
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(stream));  // the sort's buffers go; later calls may use another stream
  } else {
    cs->d_pairs.reserve(1);
    if (allocs) ++*allocs;
    HIP_TRY(hipStreamSynchronize(stream));
  }
}

// The upload half: the host rows into d_cptr / d_cind on the current device, queued on `stream`.
void candset_upload(slimgpu_candset* cs, hipStream_t stream, int* allocs, int64_t* h2d) {
  const int64_t n = cs->cptr[cs->nusers];
  const int32_t nrows = cs->nusers;
  cs->d_cptr.reserve((size_t)nrows + 1);
  cs->d_cind.reserve((size_t)n);
  if (allocs) *allocs += 2;
  HIP_TRY(hipMemcpyAsync(cs->d_cptr.get(), cs->cptr.data(), sizeof(int64_t) * ((size_t)nrows + 1),
                         hipMemcpyHostToDevice, stream));
  if (n > 0)
    HIP_TRY(hipMemcpyAsync(cs->d_cind.get(), cs->cind.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice,
                           stream));
  if (h2d) *h2d += (int64_t)(sizeof(int64_t) * ((size_t)nrows + 1) + sizeof(int32_t) * (size_t)n);
}
}  // namespace

CandidateRows candset_on_device(slimgpu_candset* cs, int device, int num_cus, hipStream_t stream, int* allocs,
                                int64_t* h2d) {
  const int64_t n = cs->cptr[cs->nusers];
  if (cs->device != device) {  // first use here: the copy of another device goes
    candset_need_ids(cs);      // (a set born on that device: its ids come down before they go)
    cs->d_cptr.reset(); cs->d_lptr.reset(); cs->d_cind.reset(); cs->d_pairs.reset();
    cs->why = ExplainWorkspace();
    cs->device = -1;
    candset_upload(cs, stream, allocs, h2d);
    candset_index(cs, num_cus, stream, allocs);
    cs->device = device;
  }
  CandidateRows R;
  R.cptr = cs->d_cptr.get(); R.cind = cs->d_cind.get(); R.lptr = cs->d_lptr.get(); R.pairs = cs->d_pairs.get();
  R.nrows = cs->nusers;
  R.entries = n;
  return R;
}

slimgpu_candset* candset_adopt(int32_t ncols, std::vector<int64_t>&& h_cptr, DeviceBuffer<int64_t>&& d_cptr,
                               DeviceBuffer<int32_t>&& d_cind, int device, int num_cus, hipStream_t stream) {
  std::unique_ptr<slimgpu_candset> cs(new slimgpu_candset);  // (a failure passes through and frees it)
  cs->ncols = ncols;
  cs->nusers = (int32_t)h_cptr.size() - 1;
  cs->cptr = std::move(h_cptr);
  cs->host_ids = cs->cptr[cs->nusers] == 0;
  cs->d_cptr = std::move(d_cptr);
  cs->d_cind = std::move(d_cind);
  candset_index(cs.get(), num_cus, stream, nullptr);
  cs->device = device;
  return cs.release();
}

void candset_need_ids(slimgpu_candset* cs) {
  if (!cs || cs->host_ids) return;
  int now = 0;
  HIP_TRY(hipGetDevice(&now));
  HIP_TRY(hipSetDevice(cs->device));
  cs->cind.resize((size_t)cs->cptr[cs->nusers]);
  const hipError_t e = hipMemcpy(cs->cind.data(), cs->d_cind.get(), sizeof(int32_t) * cs->cind.size(),
                                 hipMemcpyDeviceToHost);
  (void)hipSetDevice(now);
  HIP_TRY(e);
  cs->host_ids = true;
}

int32_t candset_fetch_ids(const char* who, slimgpu_candset* cs) {
  return guarded(who, [&]() -> int32_t {
    candset_need_ids(cs);
    return SLIM_OK;
  });
}

ExplainWorkspace& candset_explain_workspace(slimgpu_candset* cs) { return cs->why; }
const int64_t* candset_row_pointer(const slimgpu_candset* cs) { return cs->cptr.data(); }

int32_t candset_rows(slimgpu_candset* cs, int64_t* cptr, int32_t* cind) {
  if (!cs) return refuse("SLIMGPU_CandSetRows: bad arguments (a candidate set)");
  if (cind)
    if (const int32_t rc = candset_fetch_ids("SLIMGPU_CandSetRows", cs); rc != SLIM_OK) return rc;
  if (cptr) std::copy(cs->cptr.begin(), cs->cptr.end(), cptr);
  if (cind) std::copy(cs->cind.begin(), cs->cind.end(), cind);
  return SLIM_OK;
}

int32_t candset_info(const slimgpu_candset* cs, int32_t* nrows, int32_t* ncols, int64_t* entries) {
  if (!cs) return refuse("SLIMGPU_CandSetInfo: bad arguments (a candidate set)");
  if (nrows) *nrows = cs->nusers;
  if (ncols) *ncols = cs->ncols;
  if (entries) *entries = cs->cptr[cs->nusers];
  return SLIM_OK;
}

size_t fetch_slot_scores(const ScorerWorkspace& ws, const slimgpu_candset* cs, int32_t nsel, const int32_t* users,
                         hipStream_t stream, float* slot_scores) {
  size_t bytes = 0;
  auto copy = [&](int64_t e0, int64_t e1) {
    if (e1 <= e0) return;
    HIP_TRY(hipMemcpyAsync(slot_scores + e0, ws.cand.get() + e0, sizeof(float) * (size_t)(e1 - e0),
                           hipMemcpyDeviceToHost, stream));
    bytes += sizeof(float) * (size_t)(e1 - e0);
  };
  if (!users) {
    copy(0, cs->cptr[nsel]);
  } else {
    for (int32_t q = 0; q < nsel;) {  // consecutive users lie side by side: one copy per run
      int32_t e = q + 1;
      while (e < nsel && users[e] == users[e - 1] + 1) ++e;
      copy(cs->cptr[users[q]], cs->cptr[users[e - 1] + 1]);
      q = e;
    }
  }
  HIP_TRY(hipStreamSynchronize(stream));
  return bytes;
}

namespace {
// The part the two scoring calls share once the model and the histories are views on `device`: the set's device
// copy, the scorer, the lists, what comes down.  h_users: the host copy of H.users (nullptr: the first rows).
int32_t score_rows(const char* who, const DeviceRowView& W, const HistoryView& H, const int32_t* h_users,
                   slimgpu_candset* cs, int device, int num_cus, hipStream_t stream, ScorerWorkspace& ws,
                   int32_t nrcmds, float* slot_scores, int32_t* output, float* scores, int32_t* counts,
                   slimgpu_eval_stats_t& st) {
  const CandidateRows rows = candset_on_device(cs, device, num_cus, stream, &ws.allocs, &st.h2d_bytes);
  EventPair ev;
  ev.begin(stream);
  st.path = queue_candidates(W, H, rows, nrcmds, num_cus, stream, ws);
  if (st.path == kRefused) return refuse(std::string(who) + ": " + std::string(last_error()));
  ev.end(stream);
  size_t down = 0;
  if (slot_scores) down += fetch_slot_scores(ws, cs, H.nusers, h_users, stream, slot_scores);
  if (nrcmds > 0) down += fetch_lists(ws, H.nusers, nrcmds, stream, output, scores, counts);
  HIP_TRY(hipStreamSynchronize(stream));
  st.kernel_ms = ev.ms();
  st.d2h_bytes += (int64_t)down;
  return SLIM_OK;
}
}  // namespace

int32_t score_candidates(const slim_csr_t* W, const slim_csr_t* trn, slimgpu_candset* cs, int32_t nrcmds,
                         float* slot_scores, int32_t* output, float* scores, int32_t* counts) {
  const char* who = "SLIMGPU_ScoreCandidates";
  if (!W || !trn || !W->rowptr || !trn->rowptr || (!W->rowval && W->rowptr[W->nrows] > 0))
    return refuse(std::string(who) + ": bad arguments (a model with a row view, a history)");
  const int32_t nusers = trn->nrows;
  if (const int32_t rc = candset_check(who, cs, W->ncols, nusers, nullptr, nrcmds, output, scores); rc != SLIM_OK)
    return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  return guarded(who, [&]() -> int32_t {
    const int device = open_current_device();
    const int num_cus = cu_count();
    if (nusers > 0) {
      const StagedPair P = stage_pair(W, trn, num_cus);
      ScorerWorkspace ws;
      const int32_t rc = score_rows(who, P.W, P.H, nullptr, cs, device, num_cus, /*stream=*/nullptr, ws, nrcmds,
                                    slot_scores, output, scores, counts, st);
      if (rc != SLIM_OK) return rc;
      st.device_allocs = ws.allocs;
      st.w_rows_read = P.h.nnz;
    }
    st.total_ms = ms_since(t_begin);
    last_eval_stats() = st;
    return SLIM_OK;
  });
}

int32_t matrix_score_candidates(const slimgpu_model* model, slimgpu_matrix_t* mat, slimgpu_candset* cs, int32_t nusers,
                                const int32_t* users, int32_t nrcmds, float* slot_scores, int32_t* output,
                                float* scores, int32_t* counts) {
  const char* who = "SLIMGPU_MatrixScoreCandidates";
  DeviceRowView W;
  DeviceCsrView R;
  if (!model || !mat || model_row_view(model, &W) != SLIM_OK || matrix_csr_view(mat, &R) != SLIM_OK)
    return refuse(std::string(who) + ": bad arguments (a resident model with a row view, a staged matrix)");
  if (const int32_t rc = check_user_list(who, nusers, users, R.nrows); rc != SLIM_OK) return rc;
  if (const int32_t rc = check_pair(who, R, W); rc != SLIM_OK) return rc;
  const int32_t nu = users ? nusers : R.nrows;
  if (const int32_t rc = candset_check(who, cs, W.ncols, nu, users, nrcmds, output, scores); rc != SLIM_OK) return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  return guarded(who, [&]() -> int32_t {
    hipStream_t stream = open_device(R);
    if (nu > 0) {
      ScorerWorkspace ws;
      const StagedUsers U = stage_users(R, nu, users, stream, &ws.allocs, &st.h2d_bytes);
      const int32_t rc = score_rows(who, W, U.H, users, cs, R.device, R.num_cus, stream, ws, nrcmds, slot_scores,
                                    output, scores, counts, st);
      if (rc != SLIM_OK) return rc;
      st.d2h_bytes += (int64_t)sizeof(int32_t);
      st.device_allocs = ws.allocs;
      st.w_rows_read = R.nnz;
    }
    st.total_ms = ms_since(t_begin);
    last_eval_stats() = st;
    return SLIM_OK;
  });
}
}  // namespace slimamd
