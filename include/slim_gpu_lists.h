/*
 * slim_gpu_lists.h -- engine extensions of libslim.so: top-N lists of up to SLIMGPU_MAX_LIST items per user
 * on the device (candidate generation for a downstream ranker).  Included by slim_gpu.h; plain C types only.
 *
 * The list of a user is the first min(nrcmds, #candidates) of the user's candidates in the scorer's total
 * order: score descending, then discovery order.  Candidates (items touched by the history and not in it),
 * scores (float additions in history order, products and sums rounded separately) and discovery keys are
 * exactly those of the other top-N scorers, so ids and scores equal the host scorer's (Py_SLIM_Predict with
 * SLIM_PREDICT=cpu) bit for bit at every length.  output / scores are [users][nrcmds]; the slots beyond a
 * list stay as the caller filled them; counts (may be NULL) receives the list lengths.
 *
 * Up to 128 the three calls take the paths of SLIMGPU_Predict / SLIMGPU_ModelPredict / SLIMGPU_MatrixPredict
 * (the chunk kernel up to 64, the wave kernel up to 128) and give their results.  Above 128 the chunk
 * kernel's long-list form serves: it scores in LDS chunks like the chunk kernel, appends every candidate to a
 * per-workgroup slab in HBM, finds the N-th candidate with a histogram over the leading bits of the order and
 * puts the winners in order in LDS.  It needs what the rank mode needs (slim_gpu_rank.h): model rows ascending
 * by id, fewer than 2^31 model entries, a split table of at most 2 GB; anything else is SLIM_ERROR_INPUT with
 * a SLIMGPU_LastError text and nothing is written.  The device lists are 8 bytes per slot, so the users go
 * through in slices that keep them under a quarter of the free HBM, each brought down before the next is
 * queued.  Environment, for tests: SLIM_TOPN_KERNEL=long takes the long-list form at every length,
 * SLIM_TOPN_LONG_SORT=<entries> caps the contenders that are sorted in LDS, SLIM_TOPN_LONG_SLICE=<users>
 * forces the slice length.
 */
#ifndef SLIM_AMD_SLIM_GPU_LISTS_H_
#define SLIM_AMD_SLIM_GPU_LISTS_H_

#include "slim_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLIMGPU_MAX_LIST 4096
/* host model, host histories (SLIMGPU_Predict's arguments + counts, which may be NULL) */
int32_t SLIMGPU_PredictLists(int32_t nrcmds, slim_t *model, slim_t *trn,
                             int32_t *output, float *scores, int32_t *counts);
/* resident model, host histories */
int32_t SLIMGPU_ModelPredictLists(int32_t nrcmds, const slimgpu_model_t *model, slim_t *trn,
                                  int32_t *output, float *scores, int32_t *counts);
/* resident model, rows of the staged matrix; users == NULL (nusers == 0): every row, else a strictly
   ascending list as SLIMGPU_EvalSetCreateAt takes it; output[q * nrcmds + r] for position q.
   slimgpu_eval_stats_t is filled as by SLIMGPU_MatrixPredict, with path 4 on the long-list form */
int32_t SLIMGPU_MatrixPredictLists(int32_t nrcmds, const slimgpu_model_t *model, slimgpu_matrix_t *mat,
                                   int32_t nusers, const int32_t *users,
                                   int32_t *output, float *scores, int32_t *counts);
/* Counters of the most recent of the three calls on this thread. */
typedef struct slimgpu_list_stats_t {
  int32_t path;            /* 1 chunk, 2 wave, 4 long lists */
  int32_t slices;          /* user slices the call went through in */
  int64_t candidates;      /* appended to the slabs, all users */
  int64_t contenders;      /* entries of the boundary bins, all users */
  int64_t refine_passes;   /* passes beyond the first histogram, all users */
  int64_t lds_sorts, key_refines; /* users whose contenders were sorted in LDS / refined on the key */
} slimgpu_list_stats_t;
int32_t SLIMGPU_LastListStats(slimgpu_list_stats_t *out);

#ifdef __cplusplus
}
#endif

#include "slim_gpu_exposure.h"

#endif /* SLIM_AMD_SLIM_GPU_LISTS_H_ */
