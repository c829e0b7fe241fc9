/*
 * slim_gpu_wsample.h -- engine extensions of libslim.so: popularity-weighted negatives for the 1-vs-k protocol.  The
 * two samplers of slim_gpu_sample.h under THE WEIGHTED RULE, which that header states and which is the contract: the
 * host call, the device call and any restatement of it give the same rows bit for bit.  Included by
 * slim_gpu_sample.h; plain C types only.  A header of its own so that slim_gpu_sample.h goes on declaring exactly the
 * four calls it declared (the uniform sampler's ABI is unchanged, and its checks read that header's declarations);
 * including either header gives both.
 *
 * weights: ncols of them (the items of the resident matrix / the ncols argument), read during the call only; NULL:
 * popularity.  Everything else -- rows, empty rows, users, the tie rule, the refusals, the set that comes out -- is as
 * the uniform calls have it; weights that sum to 0 are SLIM_ERROR_INPUT with a SLIMGPU_LastError text, *out untouched.
 */
#ifndef SLIM_AMD_SLIM_GPU_WSAMPLE_H_
#define SLIM_AMD_SLIM_GPU_WSAMPLE_H_

#include "slim_gpu_sample.h"

#ifdef __cplusplus
extern "C" {
#endif

int32_t SLIMGPU_EvalSetSampleCandidatesWeighted(slimgpu_evalset_t *es, int32_t nnegs, uint64_t seed,
                                                const uint32_t *weights /* ncols of them; NULL: popularity */,
                                                slimgpu_candset_t **out);
int32_t SLIMGPU_CandSetSampleWeighted(int32_t ncols, slim_t *trn, slim_t *tst, int32_t nusers, const int32_t *users,
                                      int32_t nnegs, uint64_t seed, const uint32_t *weights, slimgpu_candset_t **out);
/* milliseconds of the sampling kernel of this thread's most recent SLIMGPU_EvalSetSampleCandidatesWeighted that
   launched it (a refused call leaves the figure alone); 0 before the first and when that call could not be timed,
   never an earlier call's figure for it.  A measurement aid like SLIMGPU_LastRankPrepassMs */
double SLIMGPU_LastSampleKernelMs(void);

#ifdef __cplusplus
}
#endif

#endif /* SLIM_AMD_SLIM_GPU_WSAMPLE_H_ */
