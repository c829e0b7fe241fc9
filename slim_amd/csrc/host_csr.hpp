// host_csr.hpp -- host-side slim_csr_t utilities of libslim.so (C++17).
//
// Everything here is O(nnz) bookkeeping around the solver: building and
// releasing the handle objects, the row<->column index of a learned model, the
// top-N scorer and the HR/ARHR evaluation that consume W, and the model file
// formats.  None of it is on the training hot path (that is cd_wave.hpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/slim_gpu.h"

namespace slimamd {

constexpr double kEpsilon = 1e-7;  // reference src/libslim/def.h:14

// Thread-local error text behind SLIMGPU_LastError().
void set_error(const std::string& msg);
const char* last_error();

// Allocate an all-NULL handle / release a handle and every array it owns.
slim_csr_t* csr_new();
void csr_free(slim_csr_t* m);

// max id + 1 (reference src/libslim/setup.c:117).
int32_t max_index_plus_one(int64_t nnz, const int32_t* ind);

// Deep copy of a caller's CSR into a new handle (row view only); val may be NULL.
slim_csr_t* csr_from_rows(int32_t nrows, const ssize_t* ptr, const int32_t* ind,
                          const float* val);

// Build the missing view of `m` from the other one by a counting-sort transpose
// (ascending ids inside each output row/column).  what: 0 = build columns from
// rows, 1 = build rows from columns.  Replaces the GKlib call sites
// src/libslim/setup.c:128 and src/libslim/estimate.c:591.
void csr_build_index(slim_csr_t* m, int what);

// Assemble a trained model from its column view (takes ownership of the three
// malloc'd arrays) and add the row view (reference estimate.c:570-593).
// row_view = false: the piece of a sharded solve, columns only (multi_gpu.cpp merges them).
slim_csr_t* model_from_columns(int32_t n, ssize_t* colptr, int32_t* colind,
                               float* colval, bool row_view = true);

// ---- consumers of W (host; reference predict.c, api.c:215-245) -------------

// Scratch reused across users: marker (preset -1) and candidate list.
struct TopNScratch {
  std::vector<int32_t> marker;
  std::vector<float> key;
  std::vector<int32_t> val;
  explicit TopNScratch(int32_t ncols) : marker(ncols, -1), key(ncols), val(ncols) {}
};

// predict.c:15-71.  Returns the list length.
int32_t top_n(const slim_csr_t* W, int32_t nratings, const int32_t* itemids,
              const float* ratings, int32_t nrcmds, int32_t* rids, float* rscores,
              TopNScratch& ws);
// A candidate filter (slim_gpu_filter.h) as the host scorer reads it.  bits: one bit per item, set = may be
// recommended (nullptr: every item may); xptr / xind: exclusion rows over user ids (nullptr: none).
struct HostFilter {
  int32_t ncols = 0, xusers = 0;
  const uint32_t* bits = nullptr;
  const int64_t* xptr = nullptr;
  const int32_t* xind = nullptr;
};
// top_n for user `user` under a filter: the candidates are those of top_n that F allows and the user's
// exclusion row does not name; their scores and their order among themselves are top_n's.
int32_t top_n_filtered(const slim_csr_t* W, int32_t nratings, const int32_t* itemids,
                       const float* ratings, int32_t nrcmds, int32_t* rids, float* rscores,
                       TopNScratch& ws, const HostFilter& F, int32_t user);
// predict.c:77-133: rank a fixed negative-candidate list.
int32_t top_n_1vsk(const slim_csr_t* W, int32_t nratings, const int32_t* itemids,
                   const float* ratings, int32_t nrcmds, int32_t* rids,
                   float* rscores, int32_t nnegs, const int32_t* negitems);

// A candidate set (slim_gpu_cand.h) as the host scorer reads it: a CSR over user ids, ids as given.
struct HostCandSet {
  int32_t ncols = 0, nusers = 0;
  const int64_t* cptr = nullptr;
  const int32_t* cind = nullptr;
};
// top_n_1vsk's loop over the candidate rows of the users [0, trn->nrows): slot_scores (optional) laid out like
// the set, lists (nrcmds > 0) of min(nrcmds, row length) into output / scores [user][nrcmds], counts optional.
// The ncols-long slot table is made once per call and restored after each user.
void score_candidates_host(const slim_csr_t* W, const slim_csr_t* trn, const HostCandSet& S, int32_t nrcmds,
                           float* slot_scores, int32_t* output, float* scores, int32_t* counts);

// slim_gpu_explain.h on the host, the plain loop: per user the slot table of score_candidates_host, per history
// position a walk of the model row and, per live slot it touches, a count and a bounded insertion into the slot's
// places (term descending, then position ascending; -0.0f ties with 0.0f).  Users [0, trn->nrows).  why_items and
// why_terms ([entries][nwhy], both or neither) and support ([entries]) are optional; only the first
// min(nwhy, support) places of a slot are written, and support = 0 for a slot that carries nothing.
void explain_candidates_host(const slim_csr_t* W, const slim_csr_t* trn, const HostCandSet& S, int32_t nwhy,
                             int32_t* why_items, float* why_terms, int32_t* support);

// The sampler of slim_gpu_sample.h, which states it; the device kernels (cand_sample.hip) use the same helpers.
constexpr uint64_t kSampleG = 0x9E3779B97F4A7C15ull;
#if defined(__HIP__) || defined(__HIPCC__)
#define SLIMAMD_HD __host__ __device__
#else
#define SLIMAMD_HD
#endif
SLIMAMD_HD inline uint64_t sample_mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
SLIMAMD_HD inline uint64_t sample_base(uint64_t seed, uint64_t user) { return sample_mix64(seed + kSampleG * (user + 1)); }
SLIMAMD_HD inline uint64_t sample_key(uint64_t base, uint64_t d) { return sample_mix64(base + kSampleG * (d + 1)); }
SLIMAMD_HD inline uint32_t sample_item(uint64_t key, uint32_t ncols) { return (uint32_t)(((key >> 32) * ncols) >> 32); }
inline int64_t sample_guard(int32_t nnegs) { return 16 * (int64_t)nnegs + 1024; }
// The weighted rule's two: the upper 64 bits of a * b, and the item i with C[i] <= r < C[i + 1] in the prefix table
// C[0 .. n] (C[0] = 0, ascending, r < C[n]; an item of weight 0 has an empty interval and is never found).
SLIMAMD_HD inline uint64_t sample_mulhi64(uint64_t a, uint64_t b) {
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
}
SLIMAMD_HD inline int32_t sample_search(const uint64_t* C, int32_t n, uint64_t r) {
  int32_t lo = 0, hi = n;  // C[lo] <= r < C[hi]
  while (hi - lo > 1) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (C[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}
// The rows of SLIMGPU_CandSetSample: min(trn rows, tst rows) of them, those of the users listed (ascending;
// nullptr: all) filled.  wC (nullptr: the uniform rules): the weighted rule over the prefix table C[0 .. ncols] of the
// weights, C[ncols] > 0.  The arguments are checked by the caller.
void sample_candidates_host(int32_t ncols, const slim_csr_t* trn, const slim_csr_t* tst, int32_t nusers,
                            const int32_t* users, int32_t nnegs, uint64_t seed, std::vector<int64_t>& cptr,
                            std::vector<int32_t>& cind, const uint64_t* wC = nullptr);

// api.c:215-245.  malloc'd marker array (0 head / 1 tail).
int32_t* head_tail_split(int32_t nrows, int32_t ncols, const ssize_t* rowptr,
                         const int32_t* rowind);
// its second half: the marker from the entry count of every item (pop[ncols]) and the count of all entries, which is
// all that head_tail_split reads of the rows (a staged matrix has both in its column pointer)
int32_t* head_tail_from_counts(int32_t ncols, const std::vector<int64_t>& pop, int64_t nnz);

struct EvalResult {
  float hr = 0, hr_head = 0, hr_tail = 0, arhr = 0;
  int32_t nvalid = 0, nvalid_head = 0, nvalid_tail = 0;
};
// the four figures and the three counts as the C ABI hands them out: metrics[4], nvalid[3]
inline void figures_out(const EvalResult& e, double* metrics, int32_t* nvalid) {
  metrics[0] = e.hr; metrics[1] = e.hr_head; metrics[2] = e.hr_tail; metrics[3] = e.arhr;
  nvalid[0] = e.nvalid; nvalid[1] = e.nvalid_head; nvalid[2] = e.nvalid_tail;
}
// pyapi.c:309-366: HR/ARHR of `model` for users with a non-empty test row.
// lists/counts (optional): top-N ids [nusers][nrcmds] and list lengths computed elsewhere
// (the GPU scorer); when null the host scorer is used.
EvalResult evaluate(const slim_csr_t* model, const slim_csr_t* trn,
                    const slim_csr_t* tst, int32_t nrcmds, const int32_t* fmarker,
                    int32_t fm_ncols, const int32_t* lists = nullptr,
                    const int32_t* counts = nullptr);

// slim_gpu_exposure.h on the host.  exposure_cutoffs_check: 1 <= K <= SLIMGPU_MAX_CUTOFFS cutoffs, each at least
// 1, strictly ascending, the last at most nrcmds.  exposure_lists_check: that and the lists of a caller (ncols >= 1,
// nlists >= 0, ids unless nlists == 0, every counts[q] in [0, nrcmds]).  Both: SLIM_OK, or SLIM_ERROR_INPUT with
// "<who>: ..." as the error text.
int32_t exposure_cutoffs_check(const char* who, int32_t nrcmds, int32_t ncutoffs, const int32_t* cutoffs);
int32_t exposure_lists_check(const char* who, int32_t ncols, int64_t nlists, int32_t nrcmds, const int32_t* ids,
                             const int32_t* counts, int32_t ncutoffs, const int32_t* cutoffs);
// the definition in code: E[K][ncols] and outside[K] are cleared, then every place p < min(len_q, c_{K-1}) adds one
// to the counter of its band and a last pass turns bands into cumulative counts (the device kernel's two steps)
void list_exposure_host(int32_t ncols, int64_t nlists, int32_t nrcmds, const int32_t* ids, const int32_t* counts,
                        int32_t ncutoffs, const int32_t* cutoffs, uint32_t* E, int64_t* outside);
// the summary of one cutoff's counters E[ncols]: exact integers, 128-bit numerators, one division per double
void exposure_summary(int32_t ncols, const uint32_t* pop, const int32_t* fmarker, int32_t fm_ncols, int64_t nlists,
                      const uint32_t* E, int64_t outside, slimgpu_exposure_t* out);

// slim_gpu_groups.h on the host, the definition in code: a stable counting sort of the positions by the group of
// their user (users == nullptr: position q is user q).  order[offsets[g] .. offsets[g + 1]) are the positions of group
// g, ascending; positions of group -1 are not listed.  SLIM_OK, or SLIM_ERROR_INPUT with "<who>: ..." as the error
// text and nothing written: ngroups outside [1, SLIMGPU_MAX_GROUPS], a group outside [-1, ngroups) for any user of
// [0, nall), a user outside [0, nall).
int32_t group_partition(const char* who, int32_t nsel, const int32_t* users, int32_t nall, int32_t ngroups,
                        const int32_t* group_of_user, int32_t* order, int64_t* offsets);

// slim_gpu_split.h on the host.  split_check: the parameters alone (SLIM_OK, or SLIM_ERROR_INPUT with "<who>: ..." as
// the error text).  split_host: the definition in code, one thread; *trn and *tst are matrices as csr_from_rows makes
// them and are written only on SLIM_OK.  The device kernels (split.hip) hash with the same helpers.
int32_t split_check(const char* who, const slimgpu_split_t* s);
int32_t split_host(const slim_csr_t* data, const slimgpu_split_t& s, slim_csr_t** trn, slim_csr_t** tst);

// ---- files ------------------------------------------------------------------
bool write_binrow(const slim_csr_t* m, const char* path);   // api.c:174-177
slim_csr_t* read_binrow(const char* path);                  // api.c:187-194
bool write_text_csr(const slim_csr_t* m, const char* path); // pyapi.c:47-51
slim_csr_t* read_text_csr(const char* path);                // pyapi.c:59-64

}  // namespace slimamd
