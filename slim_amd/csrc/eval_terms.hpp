// eval_terms.hpp -- what eval.hip's HR / ARHR kernels share with the fused scorer of topn.hip: the
// per-user record and the two launches (per-user terms from lists in HBM, the sum in user order).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace slimamd {

struct UserTerms {      // what one user adds to the accumulators of pyapi.c:309-366
  double hr_all, hr_head, hr_tail;
  float arhr;
  int32_t flags;        // 1 valid, 2 has a head test item, 4 has a tail test item
};

// eval.hip.  Both queue one kernel on `stream` and throw HipFail when the launch fails.
// terms[u] of lists[u*nrcmds .. +counts[u]) against test row u (device arrays)
void launch_user_terms(hipStream_t stream, int num_cus, int32_t nusers, int32_t nrcmds, const int32_t* lists,
                       const int32_t* counts, const int64_t* tptr, const int32_t* tind, const int32_t* fmarker,
                       int32_t fm_ncols, UserTerms* terms);
// out_f[4] = the four float accumulators, out_n[3] = the three counts, users added in user order
void launch_sum_in_user_order(hipStream_t stream, int32_t nusers, const UserTerms* terms, float* out_f,
                              int32_t* out_n);

}  // namespace slimamd
