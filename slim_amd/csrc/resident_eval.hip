// resident_eval.hip -- a resident model against the resident matrix (slim_gpu_eval.h, slim_gpu_rank.h,
// slim_gpu_lists.h): the eval set, model_evaluate, model_ranks / model_evaluate_ranked, matrix_predict(_lists).
// The evaluate half of a model-selection cell without the host: the history is the staged matrix's CSR
// where it lies, the model is a resident model's row view, the test rows and the head / tail marker
// were staged once (slimgpu_evalset).  One fused kernel scores, selects and forms every user's terms;
// k_sum_in_user_order adds them; 8 + 32 bytes per cutoff come down.  The evaluated users are the matrix's
// first rows or a sorted list of them (positions, eval_terms.hpp); several list lengths are served by the
// one scoring pass of the longest.  Everything is queued through the scorer's one launch path (scorer.hpp).
// Every entry point is its checks and its own middle inside the shared frame (call_frame.hpp); the calls on an
// eval set stand in EvalCall below, where what holds for every evaluation is written once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <new>
#include <optional>
#include <string>
#include <vector>

#include "call_frame.hpp"

namespace slimamd {
struct EvalOut {  // what one evaluation brings down: the first 8 + 32 * ncutoffs bytes
  unsigned long long streamed;  // entries of the model rows streamed
  EvalSums sums[SLIMGPU_MAX_RANK_CUTOFFS];
};
}  // namespace slimamd

// What an evaluation needs besides the model (slim_gpu_eval.h: SLIMGPU_EvalSetCreate).  Owns its buffers;
// borrows the matrix.
struct slimgpu_evalset {
  slimgpu_matrix_t* mat = nullptr;
  int device = 0;
  int32_t nsel = 0, fm_ncols = 0;  // positions evaluated: the listed users, or every user
  int32_t nall = 0;                // rows of the staged test matrix: min(rows of the matrix, rows of tst)
  bool listed = false;             // d_users holds the user of every position (else position q is user q)
  slimamd::Cutoffs cut = {};       // list lengths; the lists scored have the last one's
  int64_t hist_entries = 0;  // history entries of the evaluated users: the model rows one evaluation streams
  int64_t max_hist = 0;      // the longest of those histories
  slimamd::StagedCsr tst;  // the test rows of the matrix's users (ids only)
  slimamd::DeviceBuffer<int32_t> d_fm, d_users;
  std::vector<int32_t> h_users;  // the listed users on the host: a candidate set's rows are checked against them
  slimamd::DeviceBuffer<slimamd::UserTerms> d_terms;  // [cut.n][nsel]
  slimamd::DeviceBuffer<slimamd::EvalOut> d_out;
  slimamd::ScorerWorkspace ws;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // ranks of the held-out items (slim_gpu_rank.h): the test entries of the evaluated users and the longest of
  // their test rows; where a position's entries start (listed users only: else the staged row pointer serves);
  // the terms of SLIMGPU_ModelEvaluateRanked, made on first use; the pre-pass's own events
  int64_t entries = 0, max_test = 0;
  slimamd::DeviceBuffer<int64_t> d_tbase;
  slimamd::DeviceBuffer<slimamd::UserTerms> d_rterms;  // [SLIMGPU_MAX_CUTOFFS][nsel]: one slice of cutoffs
  hipEvent_t evk0 = nullptr, evk1 = nullptr;
  // exposure (slim_gpu_exposure.h): the marker's host copy, the matrix's column counts (fetched by the first
  // exposure call) and the host image of the counters: the summaries are formed on the host
  std::vector<int32_t> h_fm;
  std::vector<uint32_t> h_pop, h_expo;
  // groups (slim_gpu_groups.h; ngroups == 0: none): the positions of every group (GroupPartition's order and offsets,
  // on the device), the evaluated members, the group sums [cutoff][group] of the last evaluation with their host
  // image, and that evaluation's cutoffs (0: none since the groups were set) and own rows
  int32_t ngroups = 0, group_ncut = 0;
  std::vector<int32_t> group_members;  // [ngroups + 1]; the last: every position
  slimamd::DeviceBuffer<int32_t> d_gorder;
  slimamd::DeviceBuffer<int64_t> d_goffsets;
  slimamd::DeviceBuffer<slimamd::EvalSums> d_gsums;  // [SLIMGPU_MAX_RANK_CUTOFFS][ngroups]
  std::vector<slimamd::EvalSums> h_gsums;
  slimamd::EvalResult group_every[SLIMGPU_MAX_RANK_CUTOFFS];
  const int64_t* tbase() const { return d_tbase.get() ? d_tbase.get() : tst.ptr.get(); }
  ~slimgpu_evalset() {
    (void)hipSetDevice(device);
    for (hipEvent_t e : {ev0, ev1, evk0, evk1})
      if (e) (void)hipEventDestroy(e);
  }
};

namespace slimamd {
namespace {
thread_local slimgpu_eval_stats_t g_eval_stats;
thread_local double g_rank_prepass_ms = 0;
}  // namespace

// the matrix and the model of one call: one device, one width, rows that are the caller's
int32_t check_pair(const char* who, const DeviceCsrView& R, const DeviceRowView& W) {
  if (R.merged)
    return refuse(std::string(who) + ": the matrix was staged with SLIM_GPU_DUPLICATES=sum and repeated pairs were "
              "merged: its rows are not the caller's, score through the host handle");
  if (W.device != R.device) return refuse(std::string(who) + ": the model and the matrix live on different devices");
  if (W.nrows != R.ncols)
    return refuse(std::string(who) + ": the model has " + std::to_string(W.nrows) + " items, the matrix " +
              std::to_string(R.ncols));
  return SLIM_OK;
}

// a list of users: at least one, without a list nusers is 0 (nrows < 0: no more); rows of [0, nrows), ascending
int32_t check_user_list(const char* who, int32_t nusers, const int32_t* users, int32_t nrows) {
  std::string what;
  if (users ? nusers < 1 : nusers != 0)
    what = users ? "a user list needs at least one user" : "nusers must be 0 without a user list";
  for (int32_t q = 0; q < nusers && nrows >= 0 && what.empty(); ++q) {
    if (users[q] < 0 || users[q] >= nrows)
      what = "user " + std::to_string(users[q]) + " is outside [0, " + std::to_string(nrows) + ")";
    else if (q > 0 && users[q] <= users[q - 1])
      what = "the user ids must ascend strictly";
  }
  if (what.empty()) return SLIM_OK;
  set_error(std::string(who) + ": " + what);
  return SLIM_ERROR_INPUT;
}

namespace {
HistoryView history_of(const DeviceCsrView& R, const slimgpu_evalset* es) {
  return resident_history(R, es->nsel, es->listed ? es->d_users.get() : nullptr, es->max_hist);
}

// ranked: an eval set with no list length (SLIMGPU_EvalSetCreateRanked; ncutoffs == 0, cutoffs unused)
slimgpu_evalset_t* evalset_create_impl(slimgpu_matrix_t* mat, const slim_csr_t* tst, const int32_t* fmarker,
                                       int32_t fm_ncols, int32_t ncutoffs, const int32_t* cutoffs, int32_t nusers,
                                       const int32_t* users, int32_t* status, bool ranked) {
  auto fail = [&](int32_t st) {
    if (status) *status = st;
    return static_cast<slimgpu_evalset_t*>(nullptr);
  };
  auto refuse = [&](const std::string& what) {
    set_error("SLIMGPU_EvalSetCreate: " + what);
    return fail(SLIM_ERROR_INPUT);
  };
  DeviceCsrView R;
  if (!mat || !tst || !tst->rowptr || !fmarker || fm_ncols < 0 || (!cutoffs && !ranked))
    return refuse("bad arguments (a staged matrix, a test handle, a marker, the list lengths)");
  if (!ranked && (ncutoffs < 1 || ncutoffs > SLIMGPU_MAX_CUTOFFS))
    return refuse("between 1 and " + std::to_string(SLIMGPU_MAX_CUTOFFS) + " list lengths, not " + std::to_string(ncutoffs));
  Cutoffs cut = {};
  cut.n = ncutoffs;
  for (int32_t k = 0; k < ncutoffs; ++k) {
    if (cutoffs[k] < 1 || cutoffs[k] > 128)
      return refuse("bad arguments (1 <= nrcmds <= 128, not " + std::to_string(cutoffs[k]) + ")");
    if (k > 0 && cutoffs[k] <= cutoffs[k - 1]) return refuse("the list lengths must ascend strictly");
    cut.c[k] = cutoffs[k];
  }
  if (check_user_list("SLIMGPU_EvalSetCreate", nusers, users, -1) != SLIM_OK) return fail(SLIM_ERROR_INPUT);
  if (matrix_csr_view(mat, &R) != SLIM_OK) return refuse("bad arguments (a staged matrix)");
  if (R.merged)
    return refuse("the matrix was staged with SLIM_GPU_DUPLICATES=sum and repeated pairs were "
                  "merged: its rows are not the caller's, evaluate through the host handle");
  const int32_t nall = std::min(R.nrows, tst->nrows);  // pyapi.c:309
  if (check_user_list("SLIMGPU_EvalSetCreate", nusers, users, nall) != SLIM_OK) return fail(SLIM_ERROR_INPUT);
  const int32_t nrcmds = ranked ? 1 : cut.c[cut.n - 1];
  std::unique_ptr<slimgpu_evalset> es;  // (a failure frees what was made)
  const int32_t st = guarded("SLIMGPU_EvalSetCreate", [&]() -> int32_t {
    hipStream_t stream = open_device(R);
    es.reset(new slimgpu_evalset());
    es->mat = mat; es->device = R.device; es->cut = cut; es->fm_ncols = fm_ncols;
    es->listed = users != nullptr;
    es->nsel = users ? nusers : nall;
    es->nall = nall;
    const int32_t nsel = es->nsel;
    es->tst = stage_csr(tst, nall, /*values=*/false, stream);
    es->d_fm = DeviceBuffer<int32_t>((size_t)fm_ncols);
    es->h_fm.assign(fmarker, fmarker + fm_ncols);
    es->d_terms = DeviceBuffer<UserTerms>((size_t)cut.n * (size_t)nsel);
    es->d_out = DeviceBuffer<EvalOut>(1);
    if (fm_ncols > 0)
      HIP_TRY(hipMemcpyAsync(es->d_fm.get(), fmarker, sizeof(int32_t) * (size_t)fm_ncols, hipMemcpyHostToDevice, stream));
    if (users) {  // (pageable source: the copy has left the caller's array when the call returns)
      es->d_users = DeviceBuffer<int32_t>((size_t)nsel);
      es->h_users.assign(users, users + nsel);
      HIP_TRY(hipMemcpyAsync(es->d_users.get(), users, sizeof(int32_t) * (size_t)nsel, hipMemcpyHostToDevice, stream));
    }
    // the test entries of the evaluated users, the longest of their test rows and, for listed users, where
    // every position's entries start in the rank arrays (every user: the staged row pointer is that)
    std::vector<int64_t> h_tbase;
    if (users || tst->rowptr[0] != 0) {
      h_tbase.resize((size_t)nsel + 1);
      h_tbase[0] = 0;
      for (int32_t q = 0; q < nsel; ++q) {
        const int32_t u = users ? users[q] : q;
        const int64_t len = tst->rowptr[u + 1] - tst->rowptr[u];
        es->max_test = std::max(es->max_test, len);
        h_tbase[(size_t)q + 1] = h_tbase[(size_t)q] + len;
      }
      es->entries = h_tbase[(size_t)nsel];
      es->d_tbase = DeviceBuffer<int64_t>((size_t)nsel + 1);
      HIP_TRY(hipMemcpyAsync(es->d_tbase.get(), h_tbase.data(), sizeof(int64_t) * ((size_t)nsel + 1),
                             hipMemcpyHostToDevice, stream));  // (h_tbase outlives the synchronize below)
    } else {
      es->entries = es->tst.nnz;
      es->max_test = es->tst.max_row;
    }
    // the longest history of the evaluated users and the number of their history entries, once (the
    // scorer's key width needs the first)
    HIP_TRY(hipMemsetAsync(es->d_out.get(), 0, sizeof(EvalOut), stream));
    es->max_hist = longest_history(stream, R.num_cus, nsel, es->d_users.get(), R.d_ptr, &es->hist_entries);
    // workspaces for the worst model: 64-bit keys, hence the smallest chunks and the largest split table
    DeviceRowView worst;
    worst.nrows = worst.ncols = R.ncols;
    worst.rows_sorted = true;
    reserve_scorer(es->ws, choose_scorer(worst, history_of(R, es.get()), ListsRequest{nrcmds}, /*force_key64=*/true),
                   R.ncols, std::max(R.ncols, 1), nsel, R.num_cus, /*lists=*/false);
    // (the eval set's four events live as long as it does: an evaluation creates none)
    for (hipEvent_t* e : {&es->ev0, &es->ev1, &es->evk0, &es->evk1}) HIP_TRY(hipEventCreate(e));
    return SLIM_OK;
  });
  if (st != SLIM_OK) return fail(st);
  if (status) *status = SLIM_OK;
  return es.release();
}

// The checks that every evaluation shares, in their order: the caller's own arguments (args_ok) and the handles,
// the eval set's list lengths (ncutoffs given: the count the call asks for), one device, one width.
int32_t check_evaluation(const char* who, bool args_ok, slimgpu_evalset_t* es, const slimgpu_model* model,
                         const int32_t* ncutoffs, DeviceRowView& W, DeviceCsrView& R) {
  if (!args_ok || !es || !model || model_row_view(model, &W) != SLIM_OK || matrix_csr_view(es->mat, &R) != SLIM_OK)
    return refuse(std::string(who) + ": needs an eval set and a resident model with a row view");
  if (ncutoffs && (*ncutoffs != es->cut.n || es->cut.n < 1))
    return refuse(std::string(who) + ": the eval set holds " + std::to_string(es->cut.n) +
              " list lengths, the call asks for " + std::to_string(*ncutoffs));
  if (const int32_t rc = check_pair(who, R, W); rc != SLIM_OK) return rc;
  if (es->device != R.device)
    return refuse(std::string(who) + ": the eval set and the matrix live on different devices");
  return SLIM_OK;
}

// The frame of a call on an eval set once its checks have passed (constructed inside guarded): the clock and the
// stats record, the device and the stream, the workspace's allocation count restarted, the histories.  A call that
// forms figures hands in its outputs (out[0 .. ncut)): they are zeroed, and the group rows on hand (slim_gpu_groups.h)
// stop being readable until finish() has put this call's in their place -- what holds for every evaluation is
// written here, once.  A call without figures (model_ranks: out == nullptr) leaves the group rows alone.
struct EvalCall {
  slimgpu_evalset_t* const es;
  const DeviceCsrView& R;
  const DeviceRowView& W;
  const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  hipStream_t stream = nullptr;
  HistoryView H;

  EvalCall(slimgpu_evalset_t* es_, const DeviceCsrView& R_, const DeviceRowView& W_, int32_t ncut, EvalResult* out)
      : es(es_), R(R_), W(W_) {
    for (int32_t k = 0; out && k < ncut; ++k) out[k] = EvalResult();
    stream = open_device(R);
    es->ws.allocs = 0;
    if (out) es->group_ncut = 0;
    H = history_of(R, es);
  }
  EvalSums* sums() const { return es->d_out.get()->sums; }  // where the call's sums are queued (queue_sums)

  // What every call of an eval set leaves in last_eval_stats() once its stream has run, with the time of the
  // scorer and what followed it (ev0 .. ev1) and, for a ranked call, of the pre-pass.
  void close(bool ranked) {
    float ms = 0;
    if (es->nsel > 0) {
      HIP_TRY(hipEventElapsedTime(&ms, es->ev0, es->ev1));
      st.kernel_ms = ms;
      if (ranked && es->entries > 0) {
        HIP_TRY(hipEventElapsedTime(&ms, es->evk0, es->evk1));
        g_rank_prepass_ms = ms;
      }
    }
    st.device_allocs = es->ws.allocs;
    st.w_rows_read = es->hist_entries;
    st.total_ms = ms_since(t_begin);
    g_eval_stats = st;
  }

  // The end of an evaluation whose sums of `ncut` cutoffs are queued into sums() (ev0 was recorded before its
  // scorer): ev1, the scorer's byte model, 8 + 32 * ncut bytes down, the sums as results, the stats.
  void finish(int32_t ncut, EvalResult* out, bool ranked) {
    EvalOut h = {};
    if (es->nsel > 0) {
      EvalOut* d_out = es->d_out.get();
      HIP_TRY(hipEventRecord(es->ev1, stream));
      HIP_TRY(hipMemsetAsync(&d_out->streamed, 0, sizeof(unsigned long long), stream));
      if (es->hist_entries > 0 && W.nnz > 0) queue_streamed_entries(stream, R.num_cus, H, W, &d_out->streamed);
      size_t down = sizeof(unsigned long long) + sizeof(EvalSums) * (size_t)ncut;
      HIP_TRY(hipMemcpyAsync(&h, d_out, down, hipMemcpyDeviceToHost, stream));
      if (es->ngroups > 0) {  // (the group rows come down with the same synchronisation)
        const size_t rows = sizeof(EvalSums) * (size_t)ncut * (size_t)es->ngroups;
        HIP_TRY(hipMemcpyAsync(es->h_gsums.data(), es->d_gsums.get(), rows, hipMemcpyDeviceToHost, stream));
        down += rows;
      }
      HIP_TRY(hipStreamSynchronize(stream));
      st.d2h_bytes = (int64_t)down;
    } else if (es->ngroups > 0) {
      std::fill(es->h_gsums.begin(), es->h_gsums.end(), EvalSums{});
    }
    for (int32_t k = 0; k < ncut; ++k) out[k] = result_of(h.sums[k]);
    if (es->ngroups > 0) {
      std::copy(out, out + ncut, es->group_every);
      es->group_ncut = ncut;
    }
    st.w_bytes = 8.0 * (double)h.streamed;
    close(ranked);
  }
};

// The sums of `ncut` cutoffs over `terms` ([ncut][nsel]) into out[0 .. ncut), positions added in position order: what
// every evaluation ends in.  While groups are set (slim_gpu_groups.h) one launch forms them and, from the same
// records, the group rows of these cutoffs -- k0: the place of the first among the call's.
void queue_sums(slimgpu_evalset_t* es, hipStream_t stream, int32_t ncut, const UserTerms* terms, EvalSums* out,
                int32_t k0 = 0) {
  if (es->ngroups == 0) return launch_sum_in_user_order(stream, es->nsel, ncut, terms, out);
  launch_sum_groups_in_user_order(stream, es->nsel, ncut, es->ngroups, terms, es->d_gorder.get(), es->d_goffsets.get(),
                                  es->d_gsums.get() + (size_t)k0 * (size_t)es->ngroups, out);
}
}  // namespace

slimgpu_eval_stats_t& last_eval_stats() { return g_eval_stats; }
double last_rank_prepass_ms() { return g_rank_prepass_ms; }

slimgpu_evalset_t* evalset_create(slimgpu_matrix_t* mat, const slim_csr_t* tst, const int32_t* fmarker,
                                  int32_t fm_ncols, int32_t ncutoffs, const int32_t* cutoffs, int32_t nusers,
                                  const int32_t* users, int32_t* status) {
  return evalset_create_impl(mat, tst, fmarker, fm_ncols, ncutoffs, cutoffs, nusers, users, status, /*ranked=*/false);
}

slimgpu_evalset_t* evalset_create_ranked(slimgpu_matrix_t* mat, const slim_csr_t* tst, const int32_t* fmarker,
                                         int32_t fm_ncols, int32_t nusers, const int32_t* users, int32_t* status) {
  return evalset_create_impl(mat, tst, fmarker, fm_ncols, 0, nullptr, nusers, users, status, /*ranked=*/true);
}

int64_t evalset_entries(const slimgpu_evalset_t* es) { return es ? es->entries : -1; }

int32_t evalset_rows(const slimgpu_evalset_t* es, EvalSetRows* out) {
  DeviceCsrView R;
  if (!es || !out || matrix_csr_view(es->mat, &R) != SLIM_OK) return SLIM_ERROR_INPUT;
  EvalSetRows V;
  V.device = es->device; V.num_cus = R.num_cus; V.stream = static_cast<hipStream_t>(R.stream);
  V.merged = R.merged;
  V.ncols = R.ncols; V.nall = es->nall; V.nsel = es->nsel;
  V.d_users = es->listed ? es->d_users.get() : nullptr;
  V.h_users = es->listed ? es->h_users.data() : nullptr;
  V.hptr = R.d_ptr; V.hind = R.d_ind;
  V.tptr = es->tst.ptr.get(); V.tind = es->tst.ind.get();
  V.max_hist = es->max_hist; V.max_test = es->max_test; V.test_entries = es->entries;
  V.mat = es->mat;
  *out = V;
  return SLIM_OK;
}
void evalset_free(slimgpu_evalset_t* es) { delete es; }
int32_t evalset_cutoffs(const slimgpu_evalset_t* es) { return es ? es->cut.n : 0; }

// ---- groups (slim_gpu_groups.h) -------------------------------------------------------------------
namespace {
// The groups of an eval set from a group per user (users: the eval set's list) or per position (users == nullptr):
// partitioned by the one host routine, sent to the device, and only then put in the place of the earlier ones.
int32_t install_groups(const char* who, slimgpu_evalset_t* es, const DeviceCsrView& R, const int32_t* users,
                       int32_t nall, int32_t ngroups, const int32_t* group_of) {
  const int32_t nsel = es->nsel;
  // (sized for a number of groups in range: the partition refuses any other before it writes)
  const size_t rows = (size_t)std::min(std::max(ngroups, 0), SLIMGPU_MAX_GROUPS) + 1;
  std::vector<int32_t> order((size_t)std::max(nsel, 1)), members(rows);
  std::vector<int64_t> offsets(rows);
  if (const int32_t rc = group_partition(who, nsel, users, nall, ngroups, group_of, order.data(), offsets.data());
      rc != SLIM_OK)
    return rc;
  for (int32_t g = 0; g < ngroups; ++g) members[(size_t)g] = (int32_t)(offsets[(size_t)g + 1] - offsets[(size_t)g]);
  members[(size_t)ngroups] = nsel;
  hipStream_t stream = static_cast<hipStream_t>(R.stream);
  DeviceBuffer<int32_t> d_order((size_t)std::max(nsel, 1));
  DeviceBuffer<int64_t> d_offsets((size_t)ngroups + 1);
  DeviceBuffer<EvalSums> d_sums((size_t)ngroups * SLIMGPU_MAX_RANK_CUTOFFS);
  if (nsel > 0)
    HIP_TRY(hipMemcpyAsync(d_order.get(), order.data(), sizeof(int32_t) * (size_t)nsel, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_offsets.get(), offsets.data(), sizeof(int64_t) * ((size_t)ngroups + 1),
                         hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));  // (the sources are this call's; an evaluation may still read the old ones)
  es->d_gorder = std::move(d_order);
  es->d_goffsets = std::move(d_offsets);
  es->d_gsums = std::move(d_sums);
  es->h_gsums.assign((size_t)ngroups * SLIMGPU_MAX_RANK_CUTOFFS, EvalSums{});
  es->group_members = std::move(members);
  es->ngroups = ngroups;
  es->group_ncut = 0;
  return SLIM_OK;
}
}  // namespace

int32_t evalset_set_groups(slimgpu_evalset_t* es, int32_t ngroups, const int32_t* group_of_user) {
  const char* who = "SLIMGPU_EvalSetSetGroups";
  DeviceCsrView R;
  if (!es || !group_of_user || matrix_csr_view(es->mat, &R) != SLIM_OK)
    return refuse(std::string(who) + ": bad arguments (an eval set and the array)");
  return guarded(who, [&]() -> int32_t {
    open_device(R);
    return install_groups(who, es, R, es->listed ? es->h_users.data() : nullptr, es->nall, ngroups, group_of_user);
  });
}

// the lengths are the staged matrix's, classified where they lie: 4 * nsel bytes come down once, and the positions'
// groups go through the host partition like a caller's
int32_t evalset_set_history_bands(slimgpu_evalset_t* es, int32_t nbounds, const int32_t* bounds) {
  const char* who = "SLIMGPU_EvalSetSetHistoryBands";
  DeviceCsrView R;
  if (!es || !bounds || matrix_csr_view(es->mat, &R) != SLIM_OK)
    return refuse(std::string(who) + ": bad arguments (an eval set and the array)");
  if (nbounds < 1 || nbounds > SLIMGPU_MAX_GROUPS - 1)
    return refuse(std::string(who) + ": between 1 and " + std::to_string(SLIMGPU_MAX_GROUPS - 1) + " bounds, not " +
                  std::to_string(nbounds));
  for (int32_t j = 0; j < nbounds; ++j) {
    if (bounds[j] < 1)
      return refuse(std::string(who) + ": a bound must be at least 1, not " + std::to_string(bounds[j]));
    if (j > 0 && bounds[j] <= bounds[j - 1]) return refuse(std::string(who) + ": the bounds must ascend strictly");
  }
  return guarded(who, [&]() -> int32_t {
    hipStream_t stream = open_device(R);
    const int32_t nsel = es->nsel;
    std::vector<int32_t> band((size_t)std::max(nsel, 1), 0);
    if (nsel > 0) {
      DeviceBuffer<int32_t> d_bounds((size_t)nbounds), d_band((size_t)nsel);
      HIP_TRY(hipMemcpyAsync(d_bounds.get(), bounds, sizeof(int32_t) * (size_t)nbounds, hipMemcpyHostToDevice, stream));
      launch_history_bands(stream, R.num_cus, nsel, es->listed ? es->d_users.get() : nullptr, R.d_ptr, nbounds,
                           d_bounds.get(), d_band.get());
      HIP_TRY(hipMemcpyAsync(band.data(), d_band.get(), sizeof(int32_t) * (size_t)nsel, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
    }
    return install_groups(who, es, R, nullptr, nsel, nbounds + 1, band.data());
  });
}

void evalset_clear_groups(slimgpu_evalset_t* es) {
  if (!es || es->ngroups == 0) return;
  DeviceCsrView R;
  if (matrix_csr_view(es->mat, &R) == SLIM_OK) {  // (an evaluation in flight may still read them)
    (void)hipSetDevice(R.device);
    (void)hipStreamSynchronize(static_cast<hipStream_t>(R.stream));
  }
  es->ngroups = es->group_ncut = 0;
  es->d_gorder = DeviceBuffer<int32_t>();
  es->d_goffsets = DeviceBuffer<int64_t>();
  es->d_gsums = DeviceBuffer<EvalSums>();
  es->h_gsums.clear();
  es->group_members.clear();
}

int32_t evalset_group_info(const slimgpu_evalset_t* es, int32_t* ngroups, int32_t* members) {
  if (!es || !ngroups) return refuse("SLIMGPU_EvalSetGroupInfo: bad arguments (an eval set, ngroups)");
  if (es->ngroups == 0) return refuse("SLIMGPU_EvalSetGroupInfo: no groups are set on this eval set");
  *ngroups = es->ngroups;
  if (members) std::copy(es->group_members.begin(), es->group_members.end(), members);
  return SLIM_OK;
}

int32_t evalset_groups(const slimgpu_evalset_t* es) { return es ? es->ngroups : 0; }

int32_t evalset_group_figures(const slimgpu_evalset_t* es, int32_t ncutoffs, EvalResult* out) {
  const char* who = "SLIMGPU_EvalSetLastGroupFigures";
  if (!es || !out) return refuse(std::string(who) + ": bad arguments (an eval set, the outputs)");
  if (es->ngroups == 0) return refuse(std::string(who) + ": no groups are set on this eval set");
  if (es->group_ncut == 0) return refuse(std::string(who) + ": no evaluation has run since the groups were set");
  if (ncutoffs != es->group_ncut)
    return refuse(std::string(who) + ": the last evaluation had " + std::to_string(es->group_ncut) +
                  " cutoffs, the call asks for " + std::to_string(ncutoffs));
  for (int32_t g = 0; g < es->ngroups; ++g)
    for (int32_t k = 0; k < ncutoffs; ++k)
      out[(size_t)g * ncutoffs + k] = result_of(es->h_gsums[(size_t)k * (size_t)es->ngroups + (size_t)g]);
  std::copy(es->group_every, es->group_every + ncutoffs, out + (size_t)es->ngroups * ncutoffs);
  return SLIM_OK;
}

int32_t model_evaluate(slimgpu_evalset_t* es, const slimgpu_model* model, int32_t ncutoffs, EvalResult* out,
                       slimgpu_filter* filter) {
  const char* who = filter ? "SLIMGPU_ModelEvaluateAtFiltered" : "SLIMGPU_ModelEvaluate";
  DeviceRowView W;
  DeviceCsrView R;
  if (const int32_t rc = check_evaluation(who, out != nullptr, es, model, &ncutoffs, W, R); rc != SLIM_OK) return rc;
  if (const int32_t rc = filter_check(who, filter, W.ncols); rc != SLIM_OK) return rc;
  const int32_t ncut = es->cut.n;
  return guarded(who, [&]() -> int32_t {
    EvalCall c(es, R, W, ncut, out);
    if (es->nsel > 0) {
      const ScorerRequest rq =
          EvalTargets{es->tst.ptr.get(), es->tst.ind.get(), es->d_fm.get(), es->fm_ncols, es->d_terms.get(), es->cut};
      // (the filter's device copy is made by its first call on this device; later ones allocate and send nothing)
      const CandidateFilter F = filter_on_device(filter, R.device, c.stream, &es->ws.allocs, &c.st.h2d_bytes);
      HIP_TRY(hipEventRecord(es->ev0, c.stream));
      c.st.path = queue_scorer(W, c.H, choose_scorer(W, c.H, rq), rq, R.num_cus, c.stream, es->ws, F).path;
      queue_sums(es, c.stream, ncut, es->d_terms.get(), c.sums());
    }
    c.finish(ncut, out, /*ranked=*/false);
    return SLIM_OK;
  });
}

namespace {
// the column counts of a staged matrix (the popularity of slimgpu_exposure_t::avg_pop)
void column_counts(const slimgpu_matrix_t* mat, int32_t ncols, std::vector<uint32_t>& pop) {
  std::vector<int64_t> cp((size_t)ncols + 1);
  if (matrix_get_column_view(mat, cp.data(), nullptr, nullptr, nullptr) != SLIM_OK)
    throw HipFail{hipErrorUnknown, "the column pointer of the staged matrix"};
  pop.resize((size_t)ncols);
  for (int32_t i = 0; i < ncols; ++i) pop[(size_t)i] = (uint32_t)(cp[(size_t)i + 1] - cp[(size_t)i]);
}
int32_t check_exposure_width(const char* who, const DeviceCsrView& R, const DeviceRowView& W) {
  if (W.ncols == R.ncols) return SLIM_OK;
  return refuse(std::string(who) + ": the model has " + std::to_string(W.ncols) + " columns, the matrix " +
                std::to_string(R.ncols) + ": the exposure is counted over the matrix's items");
}
}  // namespace

// model_evaluate with the lists kept (EvalTargets::keep_lists: the fused kernel writes them beside its terms, the
// wave path writes them anyway) and counted where they lie (exposure.hip).  The figures are model_evaluate's: the
// same kernels form the same records.  The list buffers and the counters are the workspace's and only grow.
int32_t model_evaluate_exposure(slimgpu_evalset_t* es, const slimgpu_model* model, slimgpu_filter* filter,
                                int32_t ncutoffs, EvalResult* out, uint32_t* exposure, slimgpu_exposure_t* summary) {
  const char* who = "SLIMGPU_ModelEvaluateExposure";
  DeviceRowView W;
  DeviceCsrView R;
  if (es && es->cut.n < 1)
    return refuse(std::string(who) + ": the eval set was made by SLIMGPU_EvalSetCreateRanked and has no list length");
  if (const int32_t rc = check_evaluation(who, out != nullptr, es, model, &ncutoffs, W, R); rc != SLIM_OK) return rc;
  if (const int32_t rc = filter_check(who, filter, W.ncols); rc != SLIM_OK) return rc;
  if (const int32_t rc = check_exposure_width(who, R, W); rc != SLIM_OK) return rc;
  const int32_t ncut = es->cut.n, nrcmds = es->cut.c[ncut - 1], ncols = R.ncols;
  return guarded(who, [&]() -> int32_t {
    EvalCall c(es, R, W, ncut, out);
    hipStream_t stream = c.stream;
    int64_t first_down = 0;
    if (es->h_pop.size() != (size_t)ncols) {  // (the first call on this eval set)
      column_counts(es->mat, ncols, es->h_pop);
      first_down = (int64_t)sizeof(int64_t) * ((int64_t)ncols + 1);
    }
    if (es->nsel > 0) {
      const ScorerRequest rq = EvalTargets{es->tst.ptr.get(), es->tst.ind.get(), es->d_fm.get(), es->fm_ncols,
                                           es->d_terms.get(), es->cut, /*keep_lists=*/true};
      const CandidateFilter F = filter_on_device(filter, R.device, stream, &es->ws.allocs, &c.st.h2d_bytes);
      HIP_TRY(hipEventRecord(es->ev0, stream));
      queue_exposure_clear(stream, ncols, es->cut, es->ws);
      c.st.path = queue_scorer(W, c.H, choose_scorer(W, c.H, rq), rq, R.num_cus, stream, es->ws, F).path;
      queue_sums(es, stream, ncut, es->d_terms.get(), c.sums());
      queue_exposure_count(stream, R.num_cus, es->ws.oid.get(), es->ws.ocnt.get(), es->nsel, nrcmds, ncols, es->cut,
                           es->ws);
      queue_exposure_cumulate(stream, R.num_cus, ncols, es->cut, es->ws);
    }
    c.finish(ncut, out, /*ranked=*/false);
    const size_t down = fetch_exposure(stream, ncols, es->cut, es->ws, es->h_expo, es->h_pop.data(), es->h_fm.data(),
                                       es->fm_ncols, es->nsel, /*engine_lists=*/true, exposure, summary);
    g_eval_stats.d2h_bytes += (int64_t)down + first_down;
    g_eval_stats.total_ms = ms_since(c.t_begin);
    return SLIM_OK;
  });
}

// The evaluation of candidate lists (slim_gpu_cand.h): the scorer writes the slot scores of the users' candidate
// rows, k_cand_lists orders every row and keeps the first cut.c[cut.n - 1], and the wave path's epilogue -- k_user_terms
// on lists and counts, then k_sum_in_user_order -- forms the figures.  A row shorter than a cutoff gives a list
// of its own length.
int32_t model_evaluate_candidates(slimgpu_evalset_t* es, const slimgpu_model* model, slimgpu_candset* cs,
                                  int32_t ncutoffs, EvalResult* out) {
  const char* who = "SLIMGPU_ModelEvaluateCandidates";
  DeviceRowView W;
  DeviceCsrView R;
  if (const int32_t rc = check_evaluation(who, out != nullptr, es, model, &ncutoffs, W, R); rc != SLIM_OK) return rc;
  const int32_t ncut = es->cut.n, nrcmds = es->cut.c[ncut - 1];
  const int32_t* h_users = es->listed ? es->h_users.data() : nullptr;
  static const int32_t lists_wanted = 0;  // (the lists stay on the device: any non-null address serves the check)
  static const float scores_wanted = 0;
  if (const int32_t rc = candset_check(who, cs, W.ncols, es->nsel, h_users, nrcmds, &lists_wanted, &scores_wanted);
      rc != SLIM_OK)
    return rc;
  return guarded(who, [&]() -> int32_t {
    EvalCall c(es, R, W, ncut, out);
    hipStream_t stream = c.stream;
    if (es->nsel > 0) {
      const CandidateRows rows = candset_on_device(cs, R.device, R.num_cus, stream, &es->ws.allocs, &c.st.h2d_bytes);
      HIP_TRY(hipEventRecord(es->ev0, stream));
      if (queue_candidates(W, c.H, rows, nrcmds, R.num_cus, stream, es->ws) == kRefused)
        return refuse(std::string(who) + ": " + last_error());
      launch_user_terms(stream, R.num_cus, es->nsel, c.H.users, nrcmds, es->cut, es->ws.oid.get(), es->ws.ocnt.get(),
                        es->tst.ptr.get(), es->tst.ind.get(), es->d_fm.get(), es->fm_ncols, es->d_terms.get());
      queue_sums(es, stream, ncut, es->d_terms.get(), c.sums());
    }
    c.st.path = kCand;
    c.finish(ncut, out, /*ranked=*/false);
    return SLIM_OK;
  });
}

// ---- the rank of every held-out item (slim_gpu_rank.h) ------------------------------------------
namespace {
// the checks both ranked calls share
int32_t check_ranked(const char* who, slimgpu_evalset_t* es, const slimgpu_model* model, slimgpu_filter* filter,
                     DeviceRowView& W, DeviceCsrView& R) {
  if (const int32_t rc = check_evaluation(who, true, es, model, nullptr, W, R); rc != SLIM_OK) return rc;
  return filter_check(who, filter, W.ncols);
}
// the scorer in rank mode on the call's stream: ranks and scores of the eval set's test entries are in es->ws.rank /
// rscore when the stream has run.  SLIM_OK or a refusal.
int32_t queue_ranks(const char* who, EvalCall& c, slimgpu_filter* filter) {
  slimgpu_evalset_t* es = c.es;
  g_rank_prepass_ms = 0;
  c.st.path = kRank;
  if (es->nsel <= 0) return SLIM_OK;
  const ScorerRequest rq = RankTargets{es->tst.ptr.get(), es->tst.ind.get(), es->tbase(),
                                       es->entries,       es->max_test,      es->evk0,    es->evk1};
  const CandidateFilter F = filter_on_device(filter, c.R.device, c.stream, &es->ws.allocs, &c.st.h2d_bytes);
  HIP_TRY(hipEventRecord(es->ev0, c.stream));
  if (queue_scorer(c.W, c.H, choose_scorer(c.W, c.H, rq), rq, c.R.num_cus, c.stream, es->ws, F).path != kRank)
    return refuse(std::string(who) + ": " + last_error());
  return SLIM_OK;
}
}  // namespace

int32_t model_ranks(slimgpu_evalset_t* es, const slimgpu_model* model, int32_t* ranks, float* scores,
                    slimgpu_filter* filter) {
  const char* who = filter ? "SLIMGPU_ModelRanksFiltered" : "SLIMGPU_ModelRanks";
  DeviceRowView W;
  DeviceCsrView R;
  if (const int32_t rc = check_ranked(who, es, model, filter, W, R); rc != SLIM_OK) return rc;
  return guarded(who, [&]() -> int32_t {
    EvalCall c(es, R, W, 0, nullptr);  // (no figures: the group rows stay the last evaluation's)
    if (const int32_t rc = queue_ranks(who, c, filter); rc != SLIM_OK) return rc;
    if (es->nsel > 0) {
      HIP_TRY(hipEventRecord(es->ev1, c.stream));
      const size_t n = (size_t)es->entries;
      if (ranks && n) {
        HIP_TRY(hipMemcpyAsync(ranks, es->ws.rank.get(), sizeof(int32_t) * n, hipMemcpyDeviceToHost, c.stream));
        c.st.d2h_bytes += (int64_t)(sizeof(int32_t) * n);
      }
      if (scores && n) {
        HIP_TRY(hipMemcpyAsync(scores, es->ws.rscore.get(), sizeof(float) * n, hipMemcpyDeviceToHost, c.stream));
        c.st.d2h_bytes += (int64_t)(sizeof(float) * n);
      }
      HIP_TRY(hipStreamSynchronize(c.stream));
    }
    c.close(/*ranked=*/true);
    return SLIM_OK;
  });
}

int32_t model_evaluate_ranked(slimgpu_evalset_t* es, const slimgpu_model* model, int32_t ncutoffs,
                              const int32_t* cutoffs, EvalResult* out, slimgpu_filter* filter) {
  if (!cutoffs || !out || ncutoffs < 1 || ncutoffs > SLIMGPU_MAX_RANK_CUTOFFS)
    return refuse("SLIMGPU_ModelEvaluateRanked: between 1 and " + std::to_string(SLIMGPU_MAX_RANK_CUTOFFS) +
              " cutoffs, not " + std::to_string(ncutoffs));
  for (int32_t k = 0; k < ncutoffs; ++k) {
    if (cutoffs[k] < 1)
      return refuse("SLIMGPU_ModelEvaluateRanked: a cutoff must be at least 1, not " + std::to_string(cutoffs[k]));
    if (k > 0 && cutoffs[k] <= cutoffs[k - 1])
      return refuse("SLIMGPU_ModelEvaluateRanked: the cutoffs must ascend strictly");
    out[k] = EvalResult();
  }
  const char* who = filter ? "SLIMGPU_ModelEvaluateRankedFiltered" : "SLIMGPU_ModelEvaluateRanked";
  DeviceRowView W;
  DeviceCsrView R;
  if (const int32_t rc = check_ranked(who, es, model, filter, W, R); rc != SLIM_OK) return rc;
  return guarded(who, [&]() -> int32_t {
    EvalCall c(es, R, W, ncutoffs, out);
    if (const int32_t rc = queue_ranks(who, c, filter); rc != SLIM_OK) return rc;
    if (es->nsel > 0) {
      const size_t nterms = (size_t)SLIMGPU_MAX_CUTOFFS * (size_t)es->nsel;
      if (es->d_rterms.bytes() < sizeof(UserTerms) * nterms) ++es->ws.allocs;
      UserTerms* d_terms = es->d_rterms.reserve(nterms);
      // the terms workspace holds 8 records per position: the cutoffs in slices of SLIMGPU_MAX_CUTOFFS
      for (int32_t k0 = 0; k0 < ncutoffs; k0 += SLIMGPU_MAX_CUTOFFS) {
        Cutoffs cut = {};
        cut.n = std::min<int32_t>(SLIMGPU_MAX_CUTOFFS, ncutoffs - k0);
        for (int32_t k = 0; k < cut.n; ++k) cut.c[k] = cutoffs[k0 + k];
        launch_rank_terms(c.stream, R.num_cus, es->nsel, c.H.users, cut, es->ws.rank.get(), es->tbase(),
                          es->tst.ptr.get(), es->tst.ind.get(), es->d_fm.get(), es->fm_ncols, d_terms);
        queue_sums(es, c.stream, cut.n, d_terms, c.sums() + k0, k0);
      }
    }
    c.finish(ncutoffs, out, /*ranked=*/true);
    return SLIM_OK;
  });
}

namespace {
// SLIMGPU_MatrixPredict (every row, lists of up to 128) and SLIMGPU_MatrixPredictLists (who names the caller)
int32_t matrix_predict_impl(const char* who, int32_t max_n, int32_t nrcmds, const slimgpu_model* model,
                            slimgpu_matrix_t* mat, int32_t nusers, const int32_t* users, int32_t* output,
                            float* scores, int32_t* counts, slimgpu_filter* filter = nullptr) {
  DeviceRowView W;
  DeviceCsrView R;
  const bool long_ok = max_n > 128;
  if (!model || !mat || !output || !scores || nrcmds < 1 || nrcmds > max_n || model_row_view(model, &W) != SLIM_OK ||
      matrix_csr_view(mat, &R) != SLIM_OK)
    return refuse(std::string(who) + ": bad arguments (a resident model, a staged matrix, 1 <= nrcmds <= " +
              std::to_string(max_n) + ")");
  if (const int32_t rc = check_user_list(who, nusers, users, R.nrows); rc != SLIM_OK) return rc;
  if (const int32_t rc = check_pair(who, R, W); rc != SLIM_OK) return rc;
  if (const int32_t rc = filter_check(who, filter, W.ncols); rc != SLIM_OK) return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  return guarded(who, [&]() -> int32_t {
    hipStream_t stream = open_device(R);
    const int32_t nu = users ? nusers : R.nrows;
    if (nu > 0) {
      ScorerWorkspace ws;
      const StagedUsers U = stage_users(R, nu, users, stream, &ws.allocs);
      const ScorerRequest rq = long_ok ? ScorerRequest(LongListsRequest{nrcmds}) : ScorerRequest(ListsRequest{nrcmds});
      const ScorerChoice C = choose_scorer(W, U.H, rq);
      const CandidateFilter F = filter_on_device(filter, R.device, stream, &ws.allocs);
      EventPair ev;
      ev.begin(stream);
      size_t down = 0;  // only the lists come down (and the longest history's length before them)
      if (long_ok) {    // (kernel_ms then spans the slices and their copies)
        st.path = score_lists(W, U.H, C, R.num_cus, stream, ws, output, scores, counts, &down, F);
        if (st.path == kRefused) return refuse(std::string(who) + ": " + std::string(last_error()));
        ev.end(stream);
        HIP_TRY(hipStreamSynchronize(stream));
      } else {
        st.path = queue_scorer(W, U.H, C, rq, R.num_cus, stream, ws).path;
        ev.end(stream);
        down = fetch_lists(ws, nu, nrcmds, stream, output, scores, nullptr);
      }
      st.d2h_bytes = (int64_t)(down + sizeof(int32_t));
      st.kernel_ms = ev.ms();
      st.device_allocs = ws.allocs;
      st.w_rows_read = R.nnz;
    }
    st.total_ms = ms_since(t_begin);
    g_eval_stats = st;
    if (long_ok && nu <= 0) last_list_stats() = slimgpu_list_stats_t{};
    return SLIM_OK;
  });
}
}  // namespace

int32_t matrix_predict(int32_t nrcmds, const slimgpu_model* model, slimgpu_matrix_t* mat, int32_t* output,
                       float* scores) {
  return matrix_predict_impl("SLIMGPU_MatrixPredict", 128, nrcmds, model, mat, 0, nullptr, output, scores, nullptr);
}

int32_t matrix_predict_lists(int32_t nrcmds, const slimgpu_model* model, slimgpu_matrix_t* mat, int32_t nusers,
                             const int32_t* users, int32_t* output, float* scores, int32_t* counts,
                             slimgpu_filter* filter) {
  return matrix_predict_impl("SLIMGPU_MatrixPredictLists", SLIMGPU_MAX_LIST, nrcmds, model, mat, nusers, users, output,
                             scores, counts, filter);
}

// matrix_predict_lists with the lists counted where they are made (score_exposure): only the counters come down.
// The two stand in the same frame and share no more than that: this one has checks of its own and no lists to fetch.
int32_t matrix_predict_exposure(slimgpu_matrix_t* mat, const slimgpu_model* model, int32_t nrcmds, int32_t nusers,
                                const int32_t* users, slimgpu_filter* filter, const int32_t* fmarker, int32_t fm_ncols,
                                int32_t ncutoffs, const int32_t* cutoffs, uint32_t* exposure,
                                slimgpu_exposure_t* summary) {
  const char* who = "SLIMGPU_MatrixPredictExposure";
  DeviceRowView W;
  DeviceCsrView R;
  if (!model || !mat || nrcmds < 1 || nrcmds > SLIMGPU_MAX_LIST || (fmarker && fm_ncols < 0) ||
      model_row_view(model, &W) != SLIM_OK || matrix_csr_view(mat, &R) != SLIM_OK)
    return refuse(std::string(who) + ": bad arguments (a resident model, a staged matrix, 1 <= nrcmds <= " +
                  std::to_string(SLIMGPU_MAX_LIST) + ")");
  if (const int32_t rc = exposure_cutoffs_check(who, nrcmds, ncutoffs, cutoffs); rc != SLIM_OK) return rc;
  if (const int32_t rc = check_user_list(who, nusers, users, R.nrows); rc != SLIM_OK) return rc;
  if (const int32_t rc = check_pair(who, R, W); rc != SLIM_OK) return rc;
  if (const int32_t rc = filter_check(who, filter, W.ncols); rc != SLIM_OK) return rc;
  if (const int32_t rc = check_exposure_width(who, R, W); rc != SLIM_OK) return rc;
  Cutoffs cut = {};
  cut.n = ncutoffs;
  for (int32_t k = 0; k < ncutoffs; ++k) cut.c[k] = cutoffs[k];
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  return guarded(who, [&]() -> int32_t {
    hipStream_t stream = open_device(R);
    const int32_t nu = users ? nusers : R.nrows;
    std::vector<uint32_t> pop, h_E;
    column_counts(mat, R.ncols, pop);
    ScorerWorkspace ws;
    StagedUsers U;
    std::optional<EventPair> ev;  // (without a user nothing is queued and nothing timed)
    if (nu > 0) {
      U = stage_users(R, nu, users, stream, &ws.allocs);
      const ScorerChoice C = choose_scorer(W, U.H, ScorerRequest(LongListsRequest{nrcmds}));
      const CandidateFilter F = filter_on_device(filter, R.device, stream, &ws.allocs);
      ev.emplace().begin(stream);
      st.path = score_exposure(W, U.H, C, R.num_cus, stream, ws, cut, F);
      if (st.path == kRefused) return refuse(std::string(who) + ": " + std::string(last_error()));
      ev->end(stream);
    }
    st.d2h_bytes = (int64_t)fetch_exposure(stream, R.ncols, cut, ws, h_E, pop.data(), fmarker, fm_ncols, nu,
                                           /*engine_lists=*/true, exposure, summary) +
                   (int64_t)sizeof(int64_t) * ((int64_t)R.ncols + 1) + (nu > 0 ? (int64_t)sizeof(int32_t) : 0);
    if (nu > 0) {
      st.kernel_ms = ev->ms();
      st.w_rows_read = R.nnz;
    } else {
      last_list_stats() = slimgpu_list_stats_t{};
    }
    st.device_allocs = ws.allocs;
    st.total_ms = ms_since(t_begin);
    g_eval_stats = st;
    return SLIM_OK;
  });
}
}  // namespace slimamd
