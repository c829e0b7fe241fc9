// scorer.hpp -- the top-N scorer as its host code sees it (internal; topn.hip implements it).  A caller describes
// the model (DeviceRowView) and the histories (HistoryView), says what it wants (ScorerRequest), lets
// choose_scorer decide once per call and queues through queue_scorer.
#pragma once

#include <chrono>
#include <string>
#include <variant>
#include <vector>

#include "engine.hpp"
#include "eval_terms.hpp"
#include "hip_check.hpp"

namespace slimamd {
// Device buffers of the scorers, grow-only: a second run of the same shape allocates nothing.
struct ScorerWorkspace {
  DeviceBuffer<uint32_t> split;            // chunk kernel: where every chunk starts in every model row
  DeviceBuffer<int32_t> queue, oid, ocnt;  // work queue; lists and their lengths (when they are wanted)
  DeviceBuffer<float> osc, score;          // list scores; wave kernel: score vectors
  DeviceBuffer<unsigned long long> disc;   // wave kernel: discovery vectors
  // rank mode: (key, score) of every test entry from the pre-pass, (rank, score) out
  DeviceBuffer<unsigned long long> tkey;
  DeviceBuffer<float> tscore, rscore;
  DeviceBuffer<int32_t> rank;
  // long lists: one slab of ncols (image, key, id) records per workgroup; the counters of slimgpu_list_stats_t
  DeviceBuffer<uint4> slab;
  DeviceBuffer<unsigned long long> lstats;
  DeviceBuffer<float> cand;                // candidate rows: the slot scores, laid out like the set
  // exposure (slim_gpu_exposure.h, exposure.hip): the counters [K][ncols], the places outside [0, ncols) [K]
  DeviceBuffer<uint32_t> expo;
  DeviceBuffer<unsigned long long> expo_out;
  int allocs = 0;                         // device allocations since the caller last cleared it
  template <class T>
  T* need(DeviceBuffer<T>& b, size_t n) {
    if (b.bytes() < sizeof(T) * (n ? n : 1)) ++allocs;
    return b.reserve(n);
  }
};

struct HistoryView {
  int32_t nusers = 0;               // positions
  const int32_t* users = nullptr;   // the user of every position; nullptr: position q is user q
  const int64_t* ptr = nullptr; const int32_t* ind = nullptr; const float* val = nullptr;
  int64_t max_hist = 0;
  int32_t user0 = 0;                // long lists without a user list: position q is user user0 + q (a slice)
};
// the rows of a staged matrix as histories: `nsel` positions, d_users their users (nullptr: the first rows)
inline HistoryView resident_history(const DeviceCsrView& R, int32_t nsel, const int32_t* d_users, int64_t max_hist) {
  HistoryView H;
  H.nusers = nsel; H.users = d_users; H.max_hist = max_hist;
  H.ptr = R.d_ptr; H.ind = R.d_ind; H.val = R.d_val;
  return H;
}

// A candidate filter (slim_gpu_filter.h) where the scorer runs; inert when its pointers are null.  bits: one bit
// per item, set = may be recommended; xptr / xind: the exclusion rows, a CSR over user ids with xusers rows.
struct CandidateFilter {
  const uint32_t* bits = nullptr;
  const int64_t* xptr = nullptr; const int32_t* xind = nullptr;
  int32_t xusers = 0;
};
// The device copy of `f` (nullptr: no filter) on the current device, `device`: uploaded on `stream` on the
// first use there (the stream is drained once, so that later calls may use another) and kept until the
// filter is freed.  *allocs grows by the device allocations this made, *h2d (optional) by the bytes it sent.
CandidateFilter filter_on_device(slimgpu_filter* f, int device, hipStream_t stream, int* allocs,
                                 int64_t* h2d = nullptr);

// What a caller wants, one of five.  Lists of up to 128 into ws.oid / osc / ocnt; the same of up to
// SLIMGPU_MAX_LIST (ws.lstats is the caller's to provide and to clear: it adds up over the slices of one call);
struct ListsRequest { int32_t nrcmds; };
struct LongListsRequest { int32_t nrcmds; };
struct EvalTargets {  // the users' terms of lists of cut.c[cut.n - 1]: the fused epilogue's inputs and output
  const int64_t* tptr; const int32_t* tind; const int32_t* fmarker;
  int32_t fm_ncols;
  UserTerms* terms;  // [cut.n][positions]
  Cutoffs cut;
  bool keep_lists = false;  // the lists behind the terms into ws.oid / osc / ocnt as well (the exposure call)
};
struct RankTargets {  // ranks and scores of the positions' test entries into ws.rank / ws.rscore
  const int64_t* tptr; const int32_t* tind;
  const int64_t* tbase;    // [positions + 1]: where a position's test entries start
  int64_t entries;         // test entries of all positions
  int64_t max_test;        // the longest test row among them
  hipEvent_t pre0, pre1;   // around the pre-pass (k_test_keys)
};
// A candidate set (slim_gpu_cand.h) where the scorer runs.  cptr / cind: the rows as given, a CSR over user ids with
// nrows rows and `entries` entries; lptr / pairs: per row the live entries -- inside [0, ncols), of a repeated id
// the last -- ascending by id, as (id, slot in the row).
struct CandidateRows {
  const int64_t* cptr = nullptr; const int32_t* cind = nullptr;
  const int64_t* lptr = nullptr; const int2* pairs = nullptr;
  int32_t nrows = 0;
  int64_t entries = 0;
};
// The device copy of `cs` on the current device, `device`: made on `stream` on the first use there (the rows
// uploaded, the device form made by the stable radix sort; the stream is drained once) and kept until the set is
// freed.  *allocs grows by the device allocations this made, *h2d (optional) by the bytes it sent.
CandidateRows candset_on_device(slimgpu_candset* cs, int device, int num_cus, hipStream_t stream, int* allocs,
                                int64_t* h2d = nullptr);
// A set whose rows were made on the current device, `device` (cand_sample.hip): takes the rows over (d_cptr: nrows + 1,
// d_cind: the entries; h_cptr: the row pointer's host copy), indexes them on `stream` as candset_on_device indexes
// uploaded rows and drains the stream.  The host copy of the ids is fetched on first need (engine.hpp:
// candset_need_ids).  Throws HipFail / std::bad_alloc.
slimgpu_candset* candset_adopt(int32_t ncols, std::vector<int64_t>&& h_cptr, DeviceBuffer<int64_t>&& d_cptr,
                               DeviceBuffer<int32_t>&& d_cind, int device, int num_cus, hipStream_t stream);
// What the sampler (cand_sample.hip) reads of an eval set (resident_eval.hip): its users, the resident history
// rows, the staged test rows.  nall: rows of the staged test matrix, the rows a sampled set has.
struct EvalSetRows {
  int device = 0, num_cus = 256;
  hipStream_t stream = nullptr;
  bool merged = false;
  int32_t ncols = 0, nall = 0, nsel = 0;
  const int32_t* d_users = nullptr;  // nullptr: position q is user q
  const int32_t* h_users = nullptr;
  const int64_t* hptr = nullptr; const int32_t* hind = nullptr;
  const int64_t* tptr = nullptr; const int32_t* tind = nullptr;
  int64_t max_hist = 0, max_test = 0, test_entries = 0;
  const slimgpu_matrix_t* mat = nullptr;  // the resident matrix (its column pointer gives the popularity weights)
};
int32_t evalset_rows(const slimgpu_evalset_t* es, EvalSetRows* out);
// Explanations (slim_gpu_explain.h): the device outputs of explain.hip and their host images, grow-only like
// ScorerWorkspace.  They belong to the candidate set (candidates.hip), live on the device of its copy and go with it.
struct ExplainWorkspace {
  DeviceBuffer<int32_t> items, support, users;
  DeviceBuffer<float> terms;
  DeviceBuffer<int64_t> obase;  // a user list: where every position's row starts in the outputs
  std::vector<int32_t> h_items, h_support;
  std::vector<float> h_terms;
  int allocs = 0;  // device allocations since the caller last cleared it
  template <class T>
  T* need(DeviceBuffer<T>& b, size_t n) {
    if (b.bytes() < sizeof(T) * (n ? n : 1)) ++allocs;
    return b.reserve(n);
  }
  size_t held() const { return items.bytes() + support.bytes() + users.bytes() + terms.bytes() + obase.bytes(); }
};
ExplainWorkspace& candset_explain_workspace(slimgpu_candset* cs);
const int64_t* candset_row_pointer(const slimgpu_candset* cs);  // the host copy, nusers + 1
struct CandTargets {  // the slot scores of the positions' candidate rows into ws.cand (cleared first, whole)
  CandidateRows rows;
};
using ScorerRequest = std::variant<ListsRequest, LongListsRequest, EvalTargets, RankTargets, CandTargets>;

// Which kernel serves.  The values are those of slimgpu_eval_stats_t::path and slimgpu_list_stats_t::path.
enum ScorerPath : int {
  kRefused = 0,  // nothing on the device serves
  kChunk = 1,    // the chunk kernel: lists of up to 64, with or without the fused evaluation
  kWave = 2,     // the wave kernel (k_user_terms behind it for an evaluation)
  kRank = 3,     // the chunk kernel in rank mode
  kLong = 4,     // the chunk kernel's long-list form
  kCand = 5,     // the chunk kernel scoring candidate rows (slim_gpu_cand.h)
  kExplain = 6,  // the explanation kernel (slim_gpu_explain.h, explain.hip)
};
struct ChunkPlan {  // geometry of the chunk kernel for a model / history pair: key width, chunk width, LDS
  bool key32 = false;
  int pos_bits = 32, item_bytes = 12, t2w = 8, cw = 64, nchunks = 1;
  size_t lds = 0;
};
struct ScorerChoice {
  ScorerPath path = kRefused;
  ChunkPlan plan;
  int32_t nrcmds = 1;      // the list length scored (1 for ranks)
  std::string refusal;     // kRefused: why
  bool chunk_pin_missed = false;  // SLIM_TOPN_KERNEL=chunk is set and the path is another
};
// Decides once per call; reads the SLIM_TOPN_* switches.  Of H only max_hist counts.  force_key64: the worst
// case of a model not seen yet (the smallest chunks, hence the largest split table).
ScorerChoice choose_scorer(const DeviceRowView& W, const HistoryView& H, const ScorerRequest& rq,
                           bool force_key64 = false);
struct ScorerLaunch {  // how queue_scorer served a call
  ScorerPath path = kRefused;  // the choice's; kRefused: set_error says why
  int groups = 0;  // workgroups of the chunk kernel, wavefronts of the wave kernel
  ChunkPlan plan;  // the chunk kernel's geometry
  std::chrono::steady_clock::time_point launched;  // host time at which the scorer kernel itself was first queued
};
// Queues on `stream` what `rq` asks for, on the path of `choice` (choose_scorer's for this W, H and rq).
// F narrows the candidates in every mode: those of the lists, of the lists behind an evaluation (both paths) and,
// in the rank mode, of the pre-pass and the rank kernel alike.  Candidate rows (CandTargets) take no filter.
ScorerLaunch queue_scorer(const DeviceRowView& W, const HistoryView& H, const ScorerChoice& choice,
                          const ScorerRequest& rq, int num_cus, hipStream_t stream, ScorerWorkspace& ws,
                          const CandidateFilter& F = {});
// the buffers of a choice's path ahead of time (lists: ws.oid / osc / ocnt too)
void reserve_scorer(ScorerWorkspace& ws, const ScorerChoice& choice, int32_t wrows, int32_t ncols, int32_t nusers,
                    int num_cus, bool lists);
// Brings the lists of a scorer queued on `stream` down and copies the counts[u] entries of every user's list; the
// slots beyond a list stay as the caller filled them.  counts is optional.  Returns the bytes that came down.
size_t fetch_lists(const ScorerWorkspace& ws, int32_t nusers, int32_t nrcmds, hipStream_t stream, int32_t* output,
                   float* scores, int32_t* counts);
// The lists of every position of H, of any length up to SLIMGPU_MAX_LIST (choice: choose_scorer's for a
// LongListsRequest), brought down like fetch_lists does.  Up to 128 this is one launch.  On the long-list path the
// users go through in slices, each brought down before the next is queued, and the slab counters of all slices are
// added into last_list_stats().  Returns the path (kRefused: set_error says why); *down: the bytes that came down.
ScorerPath score_lists(const DeviceRowView& W, const HistoryView& H, const ScorerChoice& choice, int num_cus,
                       hipStream_t stream, ScorerWorkspace& ws, int32_t* output, float* scores, int32_t* counts,
                       size_t* down, const CandidateFilter& F = {});
// Exposure (slim_gpu_exposure.h, exposure.hip).  Three steps on `stream`, all queued: the counters ws.expo
// [cut.n][ncols] and ws.expo_out [cut.n] reserved and cleared; every place p < min(cnt[q], cut.c[cut.n - 1]) of the
// device lists ids[npos][N] (cnt == nullptr: N places each; ids 16-byte aligned) added once, to the counter of its
// band -- any number of such calls add into the same counters; the bands turned into cumulative counts.
void queue_exposure_clear(hipStream_t stream, int32_t ncols, const Cutoffs& cut, ScorerWorkspace& ws);
void queue_exposure_count(hipStream_t stream, int num_cus, const int32_t* ids, const int32_t* cnt, int64_t npos,
                          int32_t N, int32_t ncols, const Cutoffs& cut, ScorerWorkspace& ws);
void queue_exposure_cumulate(hipStream_t stream, int num_cus, int32_t ncols, const Cutoffs& cut, ScorerWorkspace& ws);
// Brings the counters down (drains `stream`), copies them to `exposure` ([cut.n][ncols], may be null) and forms the
// summaries ([cut.n], may be null) on the host.  h_E: the host image, grown as needed.  engine_lists: the lists
// were a scorer's, which writes no id outside [0, ncols): that tally stays where it is.  Returns the bytes.
// Without a position (nlists == 0) nothing was queued and nothing comes down: the counters are all zero.
size_t fetch_exposure(hipStream_t stream, int32_t ncols, const Cutoffs& cut, const ScorerWorkspace& ws,
                      std::vector<uint32_t>& h_E, const uint32_t* pop, const int32_t* fmarker, int32_t fm_ncols,
                      int64_t nlists, bool engine_lists, uint32_t* exposure, slimgpu_exposure_t* summary);
// The lists of every position of H counted where they are made (score_lists without the fetch): up to 128 one
// launch, on the long-list path slice after slice into the same counters; the counters are cumulative when the
// stream has run.  Returns the path (kRefused: set_error says why, nothing is queued).
ScorerPath score_exposure(const DeviceRowView& W, const HistoryView& H, const ScorerChoice& choice, int num_cus,
                          hipStream_t stream, ScorerWorkspace& ws, const Cutoffs& cut, const CandidateFilter& F = {});
// resident_eval.hip: what the calls on a staged matrix check of their arguments. The matrix and the model of one
// call: one device, one width, rows that are the caller's.  A list of users: at least one, without a list nusers
// is 0 (nrows < 0: no more); rows of [0, nrows), ascending.  SLIM_OK, or SLIM_ERROR_INPUT with "<who>: ...".
int32_t check_pair(const char* who, const DeviceCsrView& R, const DeviceRowView& W);
int32_t check_user_list(const char* who, int32_t nusers, const int32_t* users, int32_t nrows);
// Brings down the slot scores (ws.cand) of the rows of the users at `nsel` positions (users: host, ascending;
// nullptr: users [0, nsel)) into slot_scores, which is laid out like the set; drains `stream`.  Returns the bytes.
size_t fetch_slot_scores(const ScorerWorkspace& ws, const slimgpu_candset* cs, int32_t nsel, const int32_t* users,
                         hipStream_t stream, float* slot_scores);
// Candidate rows (slim_gpu_cand.h): queues on `stream` the slot scores of the rows of H's users into ws.cand and,
// for nrcmds > 0, their lists (score descending, then slot ascending) into ws.oid / osc / ocnt -- every selected
// row is then at most SLIMGPU_MAX_LIST long, the caller has checked.  Returns kCand, or kRefused (set_error says
// why) with nothing queued.
ScorerPath queue_candidates(const DeviceRowView& W, const HistoryView& H, const CandidateRows& rows, int32_t nrcmds,
                            int num_cus, hipStream_t stream, ScorerWorkspace& ws);
// The entries of the longest row among the rows at `nsel` positions of a CSR (d_users == nullptr: rows [0, nsel))
// and, when `entries` is given, of all of them: one kernel on `stream`, 4 (16) bytes down, the stream drained.
int64_t longest_history(hipStream_t stream, int num_cus, int32_t nsel, const int32_t* d_users, const int64_t* d_ptr,
                        int64_t* entries);
// queued on `stream`: the entries of the model rows that the histories of H stream (the scorer's byte model)
// into *d_out, which is preset to 0
void queue_streamed_entries(hipStream_t stream, int num_cus, const HistoryView& H, const DeviceRowView& W,
                            unsigned long long* d_out);

inline double ms_since(const std::chrono::steady_clock::time_point& t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}
}  // namespace slimamd
