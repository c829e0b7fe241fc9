// topn.hip -- the top-N scorers' host side (the kernels: topn_kernels.hpp): the chunk kernel's plan, the choice
// of the kernel, the launch path, and the entry points that score a host history -- predict_device /
// predict_device_view and their forms for lists of up to SLIMGPU_MAX_LIST (predict_lists / predict_lists_view).
// Every entry point, here and in resident_eval.hip, stands in the shared frame (call_frame.hpp: the error boundary,
// the staged host pair), stages what it lacks on the device (host_stage.hpp),
// describes the model and the histories as views, lets choose_scorer decide once and goes through queue_scorer
// (scorer.hpp), the one place that builds the split table, fills the kernel arguments and launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "call_frame.hpp"
#include "topn_kernels.hpp"

namespace slimamd {
bool rows_ascend_strictly(int num_cus, int32_t nrows, const int64_t* d_ptr, const int32_t* d_ind) {
  DeviceBuffer<int32_t> d_unsorted(1);
  HIP_TRY(hipMemset(d_unsorted.get(), 0, sizeof(int32_t)));
  hipLaunchKernelGGL(k_rows_sorted, dim3(std::max(1, std::min(nrows / 4 + 1, num_cus * 8))), dim3(256), 0, 0, nrows,
                     d_ptr, d_ind, d_unsorted.get());
  HIP_TRY(hipGetLastError());
  int32_t unsorted = 0;
  HIP_TRY(hipMemcpy(&unsorted, d_unsorted.get(), sizeof(int32_t), hipMemcpyDeviceToHost));
  return unsorted == 0;
}

void queue_row_facts(void* stream, int num_cus, int32_t nrows, const int64_t* d_ptr, const int32_t* d_ind,
                     int32_t* d_facts) {
  hipLaunchKernelGGL(k_row_facts, dim3(std::max(1, std::min((nrows + 255) / 256, num_cus * 8))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), nrows, d_ptr, d_ind, d_facts);
  HIP_TRY(hipGetLastError());
}

int64_t longest_history(hipStream_t stream, int num_cus, int32_t nsel, const int32_t* d_users, const int64_t* d_ptr,
                        int64_t* entries) {
  DeviceBuffer<unsigned long long> d(2);  // [0]: the longest row (its low 32 bits), [1]: the entries
  HIP_TRY(hipMemsetAsync(d.get(), 0, 2 * sizeof(unsigned long long), stream));
  if (nsel > 0) {
    hipLaunchKernelGGL(k_longest_row, dim3(std::max(1, std::min((nsel + 255) / 256, num_cus * 8))), dim3(256), 0,
                       stream, nsel, d_users, d_ptr, reinterpret_cast<int32_t*>(d.get()),
                       entries ? d.get() + 1 : nullptr);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long h[2] = {};
  HIP_TRY(hipMemcpyAsync(h, d.get(), entries ? sizeof(h) : sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (entries) *entries = (int64_t)h[1];
  return (int64_t)(uint32_t)h[0];
}

void queue_streamed_entries(hipStream_t stream, int num_cus, const HistoryView& H, const DeviceRowView& W,
                            unsigned long long* d_out) {
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)H.nusers + 3) / 4, num_cus * 8));
  hipLaunchKernelGGL(k_streamed_entries, dim3(blocks), dim3(256), 0, stream, H.nusers, H.users, H.ptr, H.ind, W.nrows,
                     W.d_ptr, d_out);
  HIP_TRY(hipGetLastError());
}

namespace {
ChunkPlan plan_chunks(int32_t ncols, int64_t max_row, int64_t max_hist, bool force_key64) {
  ChunkPlan P;
  P.t2w = kT2Waves;
  if (const char* e = std::getenv("SLIM_TOPN_WAVES")) P.t2w = std::atoi(e) == 16 ? 16 : 8;
  const int t2w = P.t2w;
  // discovery keys: 32 bits when (longest history, longest model row) fit, else 64
  auto bits_for = [](int64_t v) { int b = 0; while ((int64_t(1) << b) <= v) ++b; return b; };
  P.key32 = !force_key64 && bits_for(max_row) + bits_for(max_hist) <= 31;
  if (const char* e = std::getenv("SLIM_TOPN_KEY")) P.key32 = P.key32 && std::atoi(e) != 64;
  P.pos_bits = P.key32 ? bits_for(max_row) : 32;
  P.item_bytes = P.key32 ? 8 : 12;
  // chunk width: round 1's footprint (1536 ids x 12 bytes x 8 wavefronts), less whatever the
  // merge area of this geometry needs beyond it, so that chunks + lists always fit the 160 KB
  const size_t merge_bytes = (size_t)t2w * kT2MaxN * 16 + (size_t)t2w * sizeof(int) + 256;
  const size_t chunk_bytes = std::min<size_t>((size_t)kT2MaxCW * 12 * kT2Waves,
                                              (size_t)160 * 1024 - merge_bytes);
  const int max_cw = (int)(chunk_bytes / ((size_t)P.item_bytes * t2w)) / 64 * 64;
  P.cw = std::max(64, std::min(max_cw, ((ncols + t2w - 1) / t2w + 63) / 64 * 64));
  if (const char* e = std::getenv("SLIM_TOPN_CW")) {
    const int v = std::atoi(e);
    if (v >= 64 && v <= max_cw && v % 64 == 0) P.cw = v;
  }
  P.nchunks = (ncols + P.cw - 1) / P.cw;
  P.lds = (size_t)t2w * P.cw * P.item_bytes + (size_t)t2w * kT2MaxN * 16 + t2w * sizeof(int);
  return P;
}
constexpr size_t kSplitLimit = size_t(2) << 30;  // bytes of split table beyond which the wave kernel serves

struct ListLength {  // the list length a request is scored with
  int32_t operator()(const ListsRequest& r) const { return r.nrcmds; }
  int32_t operator()(const LongListsRequest& r) const { return r.nrcmds; }
  int32_t operator()(const EvalTargets& e) const { return e.cut.c[e.cut.n - 1]; }
  int32_t operator()(const RankTargets&) const { return 1; }
  int32_t operator()(const CandTargets&) const { return 1; }
};
}  // namespace

// The chunk kernel serves lists of up to 64 from a model whose rows ascend, with fewer than 2^31 entries and a
// split table of at most 2 GB; its long-list form (only for a call that may have lists of any length) serves
// above 128, and at any length under SLIM_TOPN_KERNEL=long; only the chunk kernel has a rank form and a form for
// candidate rows.  The wave kernel serves the rest up to 128 (and everything under SLIM_TOPN_KERNEL=wave).
ScorerChoice choose_scorer(const DeviceRowView& W, const HistoryView& H, const ScorerRequest& rq, bool force_key64) {
  ScorerChoice C;
  C.plan = plan_chunks(std::max(W.ncols, 1), W.max_row, H.max_hist, force_key64);
  C.nrcmds = std::visit(ListLength{}, rq);
  const char* kenv = std::getenv("SLIM_TOPN_KERNEL");
  auto pinned = [&](const char* v) { return kenv && std::strcmp(kenv, v) == 0; };
  const bool ranks = std::holds_alternative<RankTargets>(rq), any_length = std::holds_alternative<LongListsRequest>(rq);
  const bool sorted = W.rows_sorted || W.nnz == 0;
  const bool chunk_ok = W.nnz < (int64_t(1) << 31) && sorted &&
                        (size_t)std::max(W.nrows, 1) * ((size_t)C.plan.nchunks + 1) * sizeof(uint32_t) <= kSplitLimit;
  if (std::holds_alternative<CandTargets>(rq)) {  // only the chunk kernel scores candidate rows
    if (chunk_ok)
      C.path = kCand;
    else
      C.refusal = !sorted ? "candidate rows need the chunk scorer: the model's rows do not ascend by id (row order)"
                          : "candidate rows need the chunk scorer: fewer than 2^31 model entries, a split table of at "
                            "most 2 GB";
  } else if (any_length && chunk_ok && (C.nrcmds > 128 || pinned("long"))) {
    C.path = kLong;
  } else if (C.nrcmds > 128) {
    C.refusal = !sorted
                    ? "lists of more than 128 need the chunk scorer: the model's rows do not ascend by id (row order)"
                    : "lists of more than 128 need the chunk scorer: fewer than 2^31 model entries, a split table of at "
                      "most 2 GB";
  } else if (C.nrcmds <= kT2MaxN && chunk_ok && !pinned("wave")) {
    C.path = ranks ? kRank : kChunk;
  } else if (ranks) {
    C.refusal = "ranks of the held-out items need the chunk scorer: model rows ascending by id, fewer than 2^31 model "
                "entries, a split table of at most 2 GB" +
                std::string(kenv ? " (SLIM_TOPN_KERNEL is set)" : "");
  } else {
    C.path = kWave;
  }
  C.chunk_pin_missed = pinned("chunk") && C.path != kChunk;
  return C;
}

namespace {
int wave_kernel_waves(int32_t nusers, int32_t nrcmds, int num_cus, size_t* lds_out) {
  const size_t lds = (size_t)nrcmds * 64 * (sizeof(float) + sizeof(unsigned long long) + sizeof(int));
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (128 * 1024) / lds));
  if (lds_out) *lds_out = lds;
  return std::max(1, std::min<int>(nusers, num_cus * per_cu));
}

// workgroups of a chunk kernel: as many per CU as its wavefronts and its LDS allow
int chunk_groups(size_t lds, int t2w, int32_t nusers, int num_cus) {
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(32 / t2w, (160 * 1024) / (lds + 64)));
  return std::max(1, std::min<int>(nusers, num_cus * per_cu));
}

// LDS of the long-list form: the chunks, or the winners and the sort area that take their place after the
// chunks, whichever is larger; then the histogram and the control words
int long_sort_cap() {
  int cap = kLongSortCap;
  if (const char* e = std::getenv("SLIM_TOPN_LONG_SORT")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= kLongMaxN) cap = v;
  }
  return cap;
}
size_t long_area_bytes(const ChunkPlan& P, int32_t nrcmds, int sort_cap) {
  auto p2 = [](size_t v) { size_t p = 1; while (p < v) p <<= 1; return p; };
  const size_t chunks = (size_t)P.t2w * P.cw * P.item_bytes;
  const size_t select = (p2((size_t)nrcmds) + p2((size_t)sort_cap)) * sizeof(uint4);
  return (std::max(chunks, select) + 15) / 16 * 16;
}
size_t long_lds_bytes(size_t area) { return area + kLongBins * sizeof(uint32_t) + kLcWords * sizeof(int); }
bool uses_split_table(ScorerPath path) { return path == kChunk || path == kRank || path == kLong || path == kCand; }

// the chunk kernel that takes Args, for the plan's workgroup and key width
template <class Args, int NW, typename KeyT>
constexpr auto chunk_kernel() {
  if constexpr (std::is_same_v<Args, TopN2Args>) return &topn_chunk_kernel<NW, KeyT>;
  else if constexpr (std::is_same_v<Args, TopNEvalArgs>) return &topn_chunk_eval_kernel<NW, KeyT>;
  else if constexpr (std::is_same_v<Args, TopNRankArgs>) return &topn_chunk_rank_kernel<NW, KeyT>;
  else if constexpr (std::is_same_v<Args, TopNCandArgs>) return &topn_chunk_cand_kernel<NW, KeyT>;
  else return &topn_chunk_long_kernel<NW, KeyT>;
}
template <class Args>
void (*pick_kernel(const ChunkPlan& P))(Args) {
  return P.key32 ? (P.t2w == 16 ? chunk_kernel<Args, 16, uint32_t>() : chunk_kernel<Args, 8, uint32_t>())
                 : (P.t2w == 16 ? chunk_kernel<Args, 16, unsigned long long>()
                                : chunk_kernel<Args, 8, unsigned long long>());
}

// the mode a kernel's arguments stand for, as SLIM_GPU_TRACE names it
template <class Args>
constexpr const char* scorer_mode() {
  if constexpr (std::is_same_v<Args, TopN2Args>) return "chunk";
  else if constexpr (std::is_same_v<Args, TopNEvalArgs>) return "eval";
  else if constexpr (std::is_same_v<Args, TopNRankArgs>) return "rank";
  else if constexpr (std::is_same_v<Args, TopNCandArgs>) return "cand";
  else if constexpr (std::is_same_v<Args, TopNLongArgs>) return "long";
  else return "wave";
}

// L.groups workgroups of `fn`; more than 64 KB of dynamic LDS are asked for first; a call's first launch is stamped
template <class Args>
void launch_scorer(void (*fn)(Args), ScorerLaunch& L, int threads, size_t lds, hipStream_t stream, const Args& A) {
  if (std::getenv("SLIM_GPU_TRACE"))  // how many positions a workgroup serves one after the other
    std::fprintf(stderr, "[trace] top-N scorer (%s): %d positions, %d workgroups of %d threads, %zu bytes of LDS\n",
                 scorer_mode<Args>(), (int)A.nusers, L.groups, threads, lds);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
  if (L.launched == std::chrono::steady_clock::time_point()) L.launched = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(fn, dim3(L.groups), dim3(threads), lds, stream, A);
  HIP_TRY(hipGetLastError());
}

// the model, the histories and the queue, which the wave kernel's and the chunk kernels' arguments name alike
template <class Args>
void fill_views(Args& T, const DeviceRowView& W, const HistoryView& H, const ScorerChoice& C,
                const ScorerWorkspace& ws) {
  T.nusers = H.nusers; T.users = H.users; T.nitems_rows = W.nrows; T.ncols = std::max(W.ncols, 1);
  T.nrcmds = C.nrcmds; T.queue = ws.queue.get();
  T.wptr = W.d_ptr; T.wind = W.d_ind; T.wval = W.d_val;
  T.hptr = H.ptr; T.hind = H.ind; T.hval = H.val;
}
void fill_common(ChunkArgs& T, const DeviceRowView& W, const HistoryView& H, const ScorerChoice& C,
                 const ScorerWorkspace& ws) {
  fill_views(T, W, H, C, ws);
  T.cw = C.plan.cw; T.nchunks = C.plan.nchunks; T.pos_bits = C.plan.pos_bits; T.wsplit = ws.split.get();
  T.wlast = W.nnz > 0 ? (uint32_t)(W.nnz - 1) : 0u;
}
// the filter of a call into the wave kernel's, a chunk kernel's or the pre-pass's arguments
void fill_filter(FilterArgs& A, const CandidateFilter& F) {
  A.bits = F.bits; A.xptr = F.xptr; A.xind = F.xind; A.xusers = F.xusers;
}
void fill_lists(TopN2Args& T, const ScorerWorkspace& ws) {
  T.out_ids = ws.oid.get(); T.out_scores = ws.osc.get(); T.out_cnt = ws.ocnt.get();
}
}  // namespace

void reserve_scorer(ScorerWorkspace& ws, const ScorerChoice& C, int32_t wrows, int32_t ncols, int32_t nusers,
                    int num_cus, bool lists) {
  ws.need(ws.queue, 2);
  if (uses_split_table(C.path)) {
    ws.need(ws.split, (size_t)std::max(wrows, 1) * ((size_t)C.plan.nchunks + 1));
  } else {
    const int nwaves = wave_kernel_waves(nusers, C.nrcmds, num_cus, nullptr);
    ws.need(ws.score, (size_t)nwaves * ncols); ws.need(ws.disc, (size_t)nwaves * ncols);
  }
  if (lists || C.path == kWave) {
    ws.need(ws.oid, (size_t)nusers * C.nrcmds); ws.need(ws.osc, (size_t)nusers * C.nrcmds);
    ws.need(ws.ocnt, (size_t)nusers);
  }
}

ScorerLaunch queue_scorer(const DeviceRowView& W, const HistoryView& H, const ScorerChoice& C, const ScorerRequest& rq,
                          int num_cus, hipStream_t stream, ScorerWorkspace& ws, const CandidateFilter& F) {
  ScorerLaunch L;
  L.path = C.path;
  L.plan = C.plan;
  if (C.path == kRefused) {
    set_error(C.refusal);
    return L;
  }
  const ChunkPlan& P = C.plan;
  const int32_t ncols = std::max(W.ncols, 1), nrcmds = C.nrcmds;
  const EvalTargets* ev = std::get_if<EvalTargets>(&rq);
  const bool lists = std::holds_alternative<ListsRequest>(rq) || std::holds_alternative<LongListsRequest>(rq) ||
                     (ev && ev->keep_lists);
  reserve_scorer(ws, C, W.nrows, ncols, H.nusers, num_cus, lists);
  HIP_TRY(hipMemsetAsync(ws.queue.get(), 0, 2 * sizeof(int32_t), stream));
  if (lists || C.path == kWave) HIP_TRY(hipMemsetAsync(ws.ocnt.get(), 0, sizeof(int32_t) * (size_t)H.nusers, stream));
  if (uses_split_table(C.path) && W.nrows > 0) {
    const int64_t total = (int64_t)W.nrows * (P.nchunks + 1);
    hipLaunchKernelGGL(k_row_split, dim3((unsigned)std::min<int64_t>((total + 255) / 256, num_cus * 16)), dim3(256), 0,
                       stream, W.nrows, P.nchunks, P.cw, W.d_ptr, W.d_ind, ws.split.get());
    HIP_TRY(hipGetLastError());
  }
  switch (C.path) {
    case kChunk:
      L.groups = chunk_groups(P.lds, P.t2w, H.nusers, num_cus);
      if (ev) {  // (no lists: the output pointers stay null)
        TopNEvalArgs A{};
        fill_common(A, W, H, C, ws);
        A.tptr = ev->tptr; A.tind = ev->tind; A.fmarker = ev->fmarker; A.fm_ncols = ev->fm_ncols; A.terms = ev->terms;
        A.cut = ev->cut;
        if (ev->keep_lists) fill_lists(A, ws);
        fill_filter(A.flt, F);
        launch_scorer(pick_kernel<TopNEvalArgs>(P), L, 64 * P.t2w, P.lds, stream, A);
      } else {
        TopN2Args A{};
        fill_common(A, W, H, C, ws);
        fill_lists(A, ws);
        fill_filter(A.flt, F);
        launch_scorer(pick_kernel<TopN2Args>(P), L, 64 * P.t2w, P.lds, stream, A);
      }
      break;
    case kLong: {
      TopNLongArgs A{};
      fill_common(A, W, H, C, ws);
      fill_lists(A, ws);
      fill_filter(A.flt, F);
      A.sort_cap = long_sort_cap();
      A.area = (int32_t)long_area_bytes(P, nrcmds, A.sort_cap);
      const size_t lds = long_lds_bytes((size_t)A.area);
      L.groups = chunk_groups(lds, P.t2w, H.nusers, num_cus);
      A.slab = ws.need(ws.slab, (size_t)L.groups * (size_t)ncols);
      A.stats = ws.lstats.get();
      A.user0 = H.user0;
      launch_scorer(pick_kernel<TopNLongArgs>(P), L, 64 * P.t2w, lds, stream, A);
      break;
    }
    case kRank: {
      const RankTargets& rk = std::get<RankTargets>(rq);
      L.groups = chunk_groups(P.lds, P.t2w, H.nusers, num_cus);
      ws.need(ws.tkey, (size_t)rk.entries); ws.need(ws.tscore, (size_t)rk.entries);
      ws.need(ws.rank, (size_t)rk.entries); ws.need(ws.rscore, (size_t)rk.entries);
      if (rk.entries <= 0) break;  // (no test entry: nothing to rank)
      HIP_TRY(hipEventRecord(rk.pre0, stream));
      const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)H.nusers + 3) / 4, (int64_t)num_cus * 16));
      FilterArgs FA;  // the pre-pass and the chunks decide candidacy by the same filter
      fill_filter(FA, F);
      hipLaunchKernelGGL(k_test_keys, dim3(blocks), dim3(256), 0, stream, H.nusers, H.users, W.nrows, ncols, P.pos_bits,
                         W.d_ptr, W.d_ind, W.d_val, H.ptr, H.ind, H.val, rk.tptr, rk.tind, rk.tbase, ws.tkey.get(),
                         ws.tscore.get(), FA);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(rk.pre1, stream));
      TopNRankArgs A{};
      fill_common(A, W, H, C, ws);
      A.tptr = rk.tptr; A.tbase = rk.tbase;
      A.tkey = ws.tkey.get(); A.tscore = ws.tscore.get(); A.rank = ws.rank.get(); A.rscore = ws.rscore.get();
      A.flt = FA;
      // a test row longer than the merge area holds keys for: one scoring pass per group of entries
      A.gsize = P.t2w * kT2MaxN;
      if (const char* e = std::getenv("SLIM_TOPN_RANK_GROUP")) {
        const int v = std::atoi(e);
        if (v >= 1 && v < A.gsize) A.gsize = v;
      }
      for (int64_t g0 = 0; g0 < rk.max_test; g0 += A.gsize) {
        if (g0 > 0) HIP_TRY(hipMemsetAsync(ws.queue.get(), 0, 2 * sizeof(int32_t), stream));
        A.g0 = (int32_t)g0;
        launch_scorer(pick_kernel<TopNRankArgs>(P), L, 64 * P.t2w, P.lds, stream, A);
      }
      break;
    }
    case kCand: {
      const CandidateRows& cr = std::get<CandTargets>(rq).rows;
      L.groups = chunk_groups(P.lds, P.t2w, H.nusers, num_cus);
      ws.need(ws.cand, (size_t)cr.entries);
      // what dead entries, empty histories and out-of-range ids keep
      HIP_TRY(hipMemsetAsync(ws.cand.get(), 0, sizeof(float) * (size_t)std::max<int64_t>(cr.entries, 1), stream));
      if (cr.entries <= 0) break;
      TopNCandArgs A{};
      fill_common(A, W, H, C, ws);
      A.cptr = cr.cptr; A.lptr = cr.lptr; A.pairs = cr.pairs; A.out = ws.cand.get();
      // a row's chunk bounds go to the merge area (plan_chunks: the bytes behind the chunks) where they fit;
      // SLIM_CAND_BOUNDS=search takes the search per chunk that serves when they do not
      const char* benv = std::getenv("SLIM_CAND_BOUNDS");
      A.bounds_table = ((size_t)P.nchunks + 1) * sizeof(int) <= (size_t)P.t2w * kT2MaxN * 16 + P.t2w * sizeof(int) &&
                       !(benv && std::strcmp(benv, "search") == 0);
      launch_scorer(pick_kernel<TopNCandArgs>(P), L, 64 * P.t2w, P.lds, stream, A);
      break;
    }
    default: {  // kWave
      size_t lds = 0;
      L.groups = wave_kernel_waves(H.nusers, nrcmds, num_cus, &lds);
      TopNArgs T;
      fill_views(T, W, H, C, ws);
      T.score = ws.score.get(); T.disc = ws.disc.get();
      T.out_ids = ws.oid.get(); T.out_scores = ws.osc.get(); T.out_cnt = ws.ocnt.get();
      fill_filter(T.flt, F);
      launch_scorer(&topn_kernel, L, 64, lds, stream, T);
      if (ev)
        launch_user_terms(stream, num_cus, H.nusers, H.users, nrcmds, ev->cut, ws.oid.get(), ws.ocnt.get(), ev->tptr,
                          ev->tind, ev->fmarker, ev->fm_ncols, ev->terms);
    }
  }
  return L;
}

ScorerPath queue_candidates(const DeviceRowView& W, const HistoryView& H, const CandidateRows& rows, int32_t nrcmds,
                            int num_cus, hipStream_t stream, ScorerWorkspace& ws) {
  const ScorerRequest rq = CandTargets{rows};
  if (queue_scorer(W, H, choose_scorer(W, H, rq), rq, num_cus, stream, ws).path != kCand) return kRefused;
  if (nrcmds > 0 && H.nusers > 0) {
    ws.need(ws.oid, (size_t)H.nusers * nrcmds); ws.need(ws.osc, (size_t)H.nusers * nrcmds);
    ws.need(ws.ocnt, (size_t)H.nusers);
    const size_t lds = (size_t)kLongMaxN * sizeof(uint4);  // the longest row a list is made of
    hipLaunchKernelGGL(k_cand_lists, dim3(std::max(1, std::min<int>(H.nusers, num_cus * 8))),
                       dim3(64 * kCandListWaves), lds, stream, H.nusers, H.users, nrcmds, rows.cptr, rows.cind,
                       ws.cand.get(), ws.oid.get(), ws.osc.get(), ws.ocnt.get());
    HIP_TRY(hipGetLastError());
  }
  return kCand;
}

size_t fetch_lists(const ScorerWorkspace& ws, int32_t nusers, int32_t nrcmds, hipStream_t stream, int32_t* output,
                   float* scores, int32_t* counts) {
  if (nusers <= 0) return 0;
  std::vector<int32_t> h_id((size_t)nusers * nrcmds), h_cnt((size_t)nusers);
  std::vector<float> h_sc((size_t)nusers * nrcmds);
  HIP_TRY(hipMemcpyAsync(h_id.data(), ws.oid.get(), sizeof(int32_t) * h_id.size(), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(h_sc.data(), ws.osc.get(), sizeof(float) * h_sc.size(), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(h_cnt.data(), ws.ocnt.get(), sizeof(int32_t) * h_cnt.size(), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int32_t u = 0; u < nusers; ++u) {
    for (int32_t r = 0; r < h_cnt[u]; ++r) {
      output[(int64_t)u * nrcmds + r] = h_id[(size_t)u * nrcmds + r];
      scores[(int64_t)u * nrcmds + r] = h_sc[(size_t)u * nrcmds + r];
    }
    if (counts) counts[u] = h_cnt[u];
  }
  return sizeof(int32_t) * (h_id.size() + h_cnt.size()) + sizeof(float) * h_sc.size();
}

namespace {
thread_local slimgpu_list_stats_t g_list_stats;

// Users of one slice of a long-list call: the device lists of a slice (8 bytes per slot) stay under a quarter
// of the HBM that is free when the call begins.  SLIM_TOPN_LONG_SLICE=<users> forces a length.
int32_t long_slice_users(int32_t nusers, int32_t nrcmds) {
  if (const char* e = std::getenv("SLIM_TOPN_LONG_SLICE")) {
    const long v = std::atol(e);
    if (v >= 1) return (int32_t)std::min<long>(v, std::max(nusers, 1));
  }
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t per_user = (size_t)nrcmds * (sizeof(int32_t) + sizeof(float)) + sizeof(int32_t);
  return (int32_t)std::max<size_t>(1, std::min<size_t>((size_t)std::max(nusers, 1), free_b / 4 / per_user));
}
}  // namespace

slimgpu_list_stats_t& last_list_stats() { return g_list_stats; }

namespace {
// The lists of every position of H, on the path of C (choose_scorer's for a LongListsRequest), into ws.oid / osc /
// ocnt; each(S, s0) follows every launch and consumes them: S the positions just scored, s0 the place of the first
// among H's.  Up to 128 this is one launch over H.  On the long-list path the users go through in slices on the one
// stream -- a slice is consumed before the next overwrites it -- and the slab counters of all slices add up in
// ws.lstats (fetch_long_stats).  ls.slices: the launches.  false: nothing serves (set_error says why, nothing queued).
template <class Each>
bool score_slices(const DeviceRowView& W, const HistoryView& H, const ScorerChoice& C, int num_cus, hipStream_t stream,
                  ScorerWorkspace& ws, const CandidateFilter& F, slimgpu_list_stats_t& ls, Each&& each) {
  const ScorerRequest rq = LongListsRequest{C.nrcmds};
  if (C.path != kLong) {
    if (queue_scorer(W, H, C, rq, num_cus, stream, ws, F).path == kRefused) return false;
    each(H, 0);
    ls.slices = 1;
    return true;
  }
  ws.need(ws.lstats, 8);
  HIP_TRY(hipMemsetAsync(ws.lstats.get(), 0, 8 * sizeof(unsigned long long), stream));
  const int32_t step = long_slice_users(H.nusers, C.nrcmds);
  for (int32_t s0 = 0; s0 < H.nusers; s0 += step) {
    HistoryView S = H;
    S.nusers = std::min(step, H.nusers - s0);
    if (H.users) S.users = H.users + s0; else S.user0 = H.user0 + s0;
    queue_scorer(W, S, C, rq, num_cus, stream, ws, F);  // (the exclusion rows go by user id: S names the users)
    each(S, s0);
    ++ls.slices;
  }
  return true;
}
// the slab counters of a long-list call brought down (the stream drained) and decoded; returns the bytes
size_t fetch_long_stats(const ScorerWorkspace& ws, hipStream_t stream, slimgpu_list_stats_t& ls) {
  unsigned long long h[5] = {};
  HIP_TRY(hipMemcpyAsync(h, ws.lstats.get(), sizeof(h), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  ls.candidates = (int64_t)h[0]; ls.contenders = (int64_t)h[1]; ls.refine_passes = (int64_t)h[2];
  ls.lds_sorts = (int64_t)h[3]; ls.key_refines = (int64_t)h[4];
  return sizeof(h);
}
}  // namespace

ScorerPath score_lists(const DeviceRowView& W, const HistoryView& H, const ScorerChoice& C, int num_cus,
                       hipStream_t stream, ScorerWorkspace& ws, int32_t* output, float* scores, int32_t* counts,
                       size_t* down, const CandidateFilter& F) {
  slimgpu_list_stats_t ls = {};
  const int64_t nrcmds = C.nrcmds;
  size_t bytes = 0;
  const bool served = score_slices(W, H, C, num_cus, stream, ws, F, ls, [&](const HistoryView& S, int32_t s0) {
    bytes += fetch_lists(ws, S.nusers, C.nrcmds, stream, output + s0 * nrcmds, scores + s0 * nrcmds,
                         counts ? counts + s0 : nullptr);
  });
  if (!served) return kRefused;
  if (C.path == kLong) bytes += fetch_long_stats(ws, stream, ls);
  ls.path = C.path;
  if (down) *down = bytes;
  g_list_stats = ls;
  return C.path;
}

ScorerPath score_exposure(const DeviceRowView& W, const HistoryView& H, const ScorerChoice& C, int num_cus,
                          hipStream_t stream, ScorerWorkspace& ws, const Cutoffs& cut, const CandidateFilter& F) {
  if (C.path == kRefused) {
    set_error(C.refusal);
    return kRefused;
  }
  slimgpu_list_stats_t ls = {};
  const int32_t ncols = std::max(W.ncols, 1);
  queue_exposure_clear(stream, ncols, cut, ws);
  // (score_slices cannot refuse here: queue_scorer refuses a refused choice only, and that was judged above)
  (void)score_slices(W, H, C, num_cus, stream, ws, F, ls, [&](const HistoryView& S, int32_t) {
    queue_exposure_count(stream, num_cus, ws.oid.get(), ws.ocnt.get(), S.nusers, C.nrcmds, ncols, cut, ws);
  });
  if (C.path == kLong) fetch_long_stats(ws, stream, ls);
  queue_exposure_cumulate(stream, num_cus, ncols, cut, ws);
  ls.path = C.path;
  g_list_stats = ls;
  return C.path;
}

// Top-N lists of every history row.  output/scores are [nusers][nrcmds], slots beyond a user's list length are left
// as the caller filled them; counts (optional) = list lengths.  W: its row view on the device -- uploaded by
// predict_device (host model), or where a resident model already holds it (nothing of W crosses PCIe).  The history
// is staged, the scorer queued on the null stream through queue_scorer, the lists brought down.  Only here,
// SLIM_TOPN_KERNEL=chunk is an error when the chunk kernel cannot serve (the resident entry points fall back).
namespace {
const char* predict_name(bool long_ok) { return long_ok ? "SLIMGPU_PredictLists" : "SLIMGPU_Predict"; }

// the argument check of a family's front doors (long_ok false: lists of up to 128; true: up to
// SLIMGPU_MAX_LIST, and the output arrays are needed); model_ok: the model's arrays are there
int32_t check_predict_args(bool long_ok, bool model_ok, const slim_csr_t* hist, int32_t nrcmds, const int32_t* output,
                           const float* scores) {
  const bool hist_ok = model_ok && hist && hist->rowptr && nrcmds >= 1;
  if (!long_ok && !(hist_ok && nrcmds <= 128)) return refuse("SLIMGPU_Predict: bad arguments (1 <= nrcmds <= 128)");
  if (long_ok && !(hist_ok && output && scores && nrcmds <= SLIMGPU_MAX_LIST))
    return refuse("SLIMGPU_PredictLists: bad arguments (a model, a history, output arrays, 1 <= nrcmds <= " +
              std::to_string(SLIMGPU_MAX_LIST) + ")");
  return SLIM_OK;
}
bool host_model_ok(const slim_csr_t* W) { return W && W->rowptr && (W->rowval || W->rowptr[W->nrows] <= 0); }

// predict_device_view (long_ok false) and predict_lists_view
int32_t predict_view_impl(const DeviceRowView& W, const slim_csr_t* hist, int32_t nrcmds, int32_t* output,
                          float* scores, int32_t* counts, bool long_ok, slimgpu_filter* filter = nullptr) {
  const int32_t nusers = hist->nrows;
  if (const int32_t rc = filter_check("SLIMGPU_PredictLists", filter, W.ncols); rc != SLIM_OK) return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  return guarded(predict_name(long_ok), [&]() -> int32_t {
    open_current_device();
    if (W.device >= 0) HIP_TRY(hipSetDevice(W.device));
    const int num_cus = cu_count();
    const StagedCsr h = stage_csr(hist, nusers, /*values=*/true, /*stream=*/nullptr);
    const HistoryView H = staged_history(h, nusers);
    DeviceRowView V = W;
    decide_row_order(V, num_cus);
    const ScorerRequest rq = long_ok ? ScorerRequest(LongListsRequest{nrcmds}) : ScorerRequest(ListsRequest{nrcmds});
    const ScorerChoice C = choose_scorer(V, H, rq);
    if (C.chunk_pin_missed)
      return refuse("SLIMGPU_Predict: SLIM_TOPN_KERNEL=chunk needs nrcmds <= 64 and model rows sorted by id");
    ScorerWorkspace ws;
    if (long_ok) {
      int device = 0;
      HIP_TRY(hipGetDevice(&device));
      const CandidateFilter F = filter_on_device(filter, device, /*stream=*/nullptr, &ws.allocs);
      if (score_lists(V, H, C, num_cus, /*stream=*/nullptr, ws, output, scores, counts, nullptr, F) == kRefused)
        return refuse("SLIMGPU_PredictLists: " + std::string(last_error()));
      return SLIM_OK;
    }
    const ScorerLaunch L = queue_scorer(V, H, C, rq, num_cus, /*stream=*/nullptr, ws);
    HIP_TRY(hipDeviceSynchronize());
    if (L.path == kChunk && std::getenv("SLIM_GPU_TRACE"))
      std::fprintf(stderr, "[trace] top-N chunk kernel: %d users, %d workgroups of %d wavefronts, chunks of %d ids, "
                           "%d-bit keys: %.1f ms (upload + split table before it: %.1f ms)\n",
                   nusers, L.groups, L.plan.t2w, L.plan.cw, L.plan.key32 ? 32 : 64, ms_since(L.launched),
                   std::chrono::duration<double, std::milli>(L.launched - t_begin).count());
    fetch_lists(ws, nusers, nrcmds, nullptr, output, scores, counts);
    return SLIM_OK;
  });
}

// predict_device (long_ok false) and predict_lists: the model staged, then as above
int32_t predict_impl(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds, int32_t* output, float* scores,
                     int32_t* counts, bool long_ok, slimgpu_filter* filter = nullptr) {
  if (const int32_t rc = filter_check("SLIMGPU_PredictLists", filter, W->ncols); rc != SLIM_OK) return rc;
  return guarded(predict_name(long_ok), [&]() -> int32_t {
    open_current_device();
    const StagedCsr w = stage_csr(W, W->nrows, /*values=*/true, /*stream=*/nullptr);
    return predict_view_impl(staged_row_view(W, w), hist, nrcmds, output, scores, counts, long_ok, filter);
  });
}
}  // namespace

int32_t predict_device_view(const DeviceRowView& W, const slim_csr_t* hist, int32_t nrcmds,
                            int32_t* output, float* scores, int32_t* counts) {
  const int32_t rc = check_predict_args(false, W.d_ptr != nullptr, hist, nrcmds, output, scores);
  return rc != SLIM_OK ? rc : predict_view_impl(W, hist, nrcmds, output, scores, counts, /*long_ok=*/false);
}
int32_t predict_lists_view(const DeviceRowView& W, const slim_csr_t* hist, int32_t nrcmds,
                           int32_t* output, float* scores, int32_t* counts, slimgpu_filter* filter) {
  const int32_t rc = check_predict_args(true, W.d_ptr != nullptr, hist, nrcmds, output, scores);
  return rc != SLIM_OK ? rc : predict_view_impl(W, hist, nrcmds, output, scores, counts, /*long_ok=*/true, filter);
}
int32_t predict_device(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds,
                       int32_t* output, float* scores, int32_t* counts) {
  const int32_t rc = check_predict_args(false, host_model_ok(W), hist, nrcmds, output, scores);
  return rc != SLIM_OK ? rc : predict_impl(W, hist, nrcmds, output, scores, counts, /*long_ok=*/false);
}
int32_t predict_lists(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds,
                      int32_t* output, float* scores, int32_t* counts, slimgpu_filter* filter) {
  const int32_t rc = check_predict_args(true, host_model_ok(W), hist, nrcmds, output, scores);
  return rc != SLIM_OK ? rc : predict_impl(W, hist, nrcmds, output, scores, counts, /*long_ok=*/true, filter);
}
}  // namespace slimamd
