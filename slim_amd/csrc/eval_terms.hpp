// eval_terms.hpp -- what eval.hip's HR / ARHR kernels share with the fused scorer of topn_kernels.hpp: the
// per-user record, the list of cutoffs and the two launches (per-user terms from lists in HBM, the sum
// in position order).
//
// Positions and users: an evaluation runs over `nsel` positions q; the user at position q is users[q],
// or q itself when there is no user list.  History and test row are the user's; everything the scorer
// writes (lists, terms) is indexed by the position.
//
// Cutoffs: the scorer's order is total (score descending, then discovery key), so the list of length c
// is the first c ranks of any longer list.  One walk over a user's hitting ranks, in rank order, therefore
// serves every cutoff: the record of cutoff k is formed from the running sums when the walk passes rank
// cutoffs[k].  The float additions behind cutoff k are a prefix of those behind cutoff k + 1, in the same
// order, so each record equals the one a separate evaluation with lists of cutoffs[k] forms, bit for bit.
// Records are laid out terms[k * nsel + q].
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/slim_gpu_eval.h"
#include "host_csr.hpp"

namespace slimamd {

struct UserTerms {      // what one user adds to the accumulators of pyapi.c:309-366
  double hr_all, hr_head, hr_tail;
  float arhr;
  int32_t flags;        // 1 valid, 2 has a head test item, 4 has a tail test item
};

struct Cutoffs {        // list lengths, strictly ascending; c[n - 1] is the length of the lists scored
  int32_t n;
  int32_t c[SLIMGPU_MAX_CUTOFFS];
  // The kernels read c[] through constant indices only (a kernel argument indexed by a variable is copied
  // to scratch): the lengths packed one per byte.  That holds the lengths of an eval set (at most 128); the
  // last length of a list that comes from the host (SLIMGPU_Evaluate: any nrcmds) may not fit, and no kernel
  // reads it from the word -- k_user_terms ends its last record at the lists' row length.
  __host__ __device__ __forceinline__ unsigned long long packed() const {
    unsigned long long p = 0;
#pragma unroll
    for (int j = 0; j < SLIMGPU_MAX_CUTOFFS; ++j) p |= (unsigned long long)(uint32_t)(c[j] & 0xff) << (8 * j);
    return p;
  }
  // ... and length k of such a word
  __host__ __device__ static __forceinline__ int32_t at(unsigned long long packed, int k) {
    return (int32_t)((packed >> (8 * k)) & 0xff);
  }
};
inline Cutoffs one_cutoff(int32_t nrcmds) {
  Cutoffs C = {};
  C.n = 1;
  C.c[0] = nrcmds;
  return C;
}

struct EvalSums {       // the accumulators of one cutoff
  float f[4];           // hr_all, hr_head, hr_tail, arhr
  int32_t n[3];         // nvalid, nvalid_head, nvalid_tail
  int32_t pad;
};
// the figures of one cutoff's accumulators
inline EvalResult result_of(const EvalSums& s) {
  EvalResult r;
  r.nvalid = s.n[0]; r.nvalid_head = s.n[1]; r.nvalid_tail = s.n[2];
  r.hr = s.n[0] > 0 ? s.f[0] / s.n[0] : 0; r.arhr = s.n[0] > 0 ? s.f[3] / s.n[0] : 0;
  r.hr_head = s.n[1] > 0 ? s.f[1] / s.n[1] : 0; r.hr_tail = s.n[2] > 0 ? s.f[2] / s.n[2] : 0;
  return r;
}

// the hits of one user, walked in rank order (both scorers' epilogues)
struct HitWalk {
  int nh0 = 0, nh1 = 0, nh2 = 0;
  float gain = 0.0f;
  __device__ __forceinline__ void hit(int rank, int cls) {
    if (cls) ++nh1; else ++nh0;
    ++nh2;
    gain = (float)((double)gain + 1.0 / (1.0 + rank));
  }
  // the record of the ranks walked so far; flags == 0: a user without test items
  __device__ __forceinline__ UserTerms terms(int ntrue0, int ntrue1, int64_t tlen, float ideal, int flags) const {
    UserTerms t = {0.0, 0.0, 0.0, 0.0f, 0};
    if (flags) {
      t.hr_head = nh0 > 0 ? 1.0 * nh0 / ntrue0 : 0.0;
      t.hr_tail = nh1 > 0 ? 1.0 * nh1 / ntrue1 : 0.0;
      t.hr_all = 1.0 * nh2 / double(tlen);
      t.arhr = gain / ideal;
      t.flags = flags;
    }
    return t;
  }
};

// eval.hip.  Both queue one kernel on `stream` and throw HipFail when the launch fails.
// terms[k*nsel + q] of lists[q*nrcmds .. +min(counts[q], cut.c[k])) against the test row of the user at
// position q (device arrays; users == nullptr: user q), nrcmds = the row length of `lists`
void launch_user_terms(hipStream_t stream, int num_cus, int32_t nsel, const int32_t* users, int32_t nrcmds,
                       const Cutoffs& cut, const int32_t* lists, const int32_t* counts, const int64_t* tptr,
                       const int32_t* tind, const int32_t* fmarker, int32_t fm_ncols, UserTerms* terms);
// terms[k*nsel + q] from the RANKS of the test entries of the user at position q (slim_gpu_rank.h; ranks[tbase[q]
// + z] belongs to entry z of the user's test row): the distinct non-zero ranks <= cut.c[k], walked ascending.
// Any cutoff >= 1 (cut.c is read as it is, not through the packed word).
void launch_rank_terms(hipStream_t stream, int num_cus, int32_t nsel, const int32_t* users, const Cutoffs& cut,
                       const int32_t* ranks, const int64_t* tbase, const int64_t* tptr, const int32_t* tind,
                       const int32_t* fmarker, int32_t fm_ncols, UserTerms* terms);
// out[k] = the accumulators of cutoff k, positions added in position order (one wavefront per cutoff)
void launch_sum_in_user_order(hipStream_t stream, int32_t nsel, int32_t ncut, const UserTerms* terms,
                              EvalSums* out);
// slim_gpu_groups.h: out[k * ngroups + g] = the accumulators of cutoff k over the positions order[offsets[g] ..
// offsets[g + 1]) (device arrays; ascending inside a group, each in [0, nsel)), added in that order with the
// arithmetic of launch_sum_in_user_order (one wavefront per cutoff and group); ngroups >= 1.  The same launch forms
// every[k], launch_sum_in_user_order's output bit for bit, in one more wavefront per cutoff: it stands in for that
// launch, it does not follow it.
void launch_sum_groups_in_user_order(hipStream_t stream, int32_t nsel, int32_t ncut, int32_t ngroups,
                                     const UserTerms* terms, const int32_t* order, const int64_t* offsets,
                                     EvalSums* out, EvalSums* every);
// group_of_position[q] = #{j : the history length of the user at position q >= bounds[j]} (bounds[nbounds]: a device
// array, ascending, nbounds <= SLIMGPU_MAX_GROUPS; hptr: the staged matrix's row pointer)
void launch_history_bands(hipStream_t stream, int num_cus, int32_t nsel, const int32_t* users, const int64_t* hptr,
                          int32_t nbounds, const int32_t* bounds, int32_t* group_of_position);

}  // namespace slimamd
