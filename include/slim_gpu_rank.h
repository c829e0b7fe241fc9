/*
 * slim_gpu_rank.h -- engine extensions of libslim.so: the rank of every held-out item among a user's
 * candidates, and from it the evaluation of a resident model at ANY list length.  Included by
 * slim_gpu.h; plain C types only.
 *
 * The scorer's order is total (score descending, then discovery order), so a test item t of a user has
 * one well-defined place among the user's candidates:
 *     rank = 1 + #{candidates c : c stands before t},
 * with candidates (items touched by the history and not in it), scores (float additions in history
 * order, products and sums rounded separately) and discovery keys exactly those of the top-N scorers.
 * rank = 0 and score = 0 when t is not a candidate: never touched, in the user's history, an id < 0 or
 * >= the model's width, or an empty history -- such an item is in no list of any length.
 * Contract: for every N, t stands at position r of the length-N list of the host scorer and of
 * SLIMGPU_MatrixPredict iff rank == r + 1 <= N, with that list's score bit for bit.  No list is formed:
 * a pre-pass finds (score, key) of every test entry, the scorer counts the candidates ahead of each.
 *
 * Needs a model whose rows ascend by id (every resident model does), fewer than 2^31 model entries and
 * a split table of at most 2 GB; anything else is SLIM_ERROR_INPUT with a SLIMGPU_LastError text.
 * slimgpu_eval_stats_t::path is 3.  From the second call on an eval set: no device allocation, nothing
 * host to device.
 */
#ifndef SLIM_AMD_SLIM_GPU_RANK_H_
#define SLIM_AMD_SLIM_GPU_RANK_H_

#include "slim_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLIMGPU_MAX_RANK_CUTOFFS 32
typedef struct slimgpu_evalset slimgpu_evalset_t; /* (slim_gpu_eval.h) */

/* an eval set with no list length (users as in SLIMGPU_EvalSetCreateAt) */
slimgpu_evalset_t *SLIMGPU_EvalSetCreateRanked(slimgpu_matrix_t *mat, slim_t *tsthandle, const int32_t *fmarker,
                                               int32_t fm_ncols, int32_t nusers, const int32_t *users, int32_t *r_status);
int64_t SLIMGPU_EvalSetEntries(const slimgpu_evalset_t *es);   /* test entries of the selected users; -1: null */
/* ranks / scores: host arrays of SLIMGPU_EvalSetEntries, positions in order, each test row in its order; either may be NULL.
   Only the ranks and scores come down: slimgpu_eval_stats_t::w_bytes stays 0 (SLIMGPU_ModelEvaluateRanked reports it) */
int32_t SLIMGPU_ModelRanks(slimgpu_evalset_t *es, const slimgpu_model_t *model, int32_t *ranks, float *scores);
/* cutoffs strictly ascending, >= 1, no upper bound; metrics[k*4..), nvalid[k*3..) as SLIMGPU_ModelEvaluateAt */
int32_t SLIMGPU_ModelEvaluateRanked(slimgpu_evalset_t *es, const slimgpu_model_t *model, int32_t ncutoffs,
                                    const int32_t *cutoffs, double *metrics, int32_t *nvalid);
/* a host model made resident on mat's device: row view uploaded, column view formed by transpose_on_device,
   k_row_facts; rows must ascend strictly (SLIM_ERROR_INPUT); n = max(nrows, ncols), missing rows empty */
slimgpu_model_t *SLIMGPU_ModelFromHost(slimgpu_matrix_t *mat, slim_t *model, int32_t *r_status);
/* milliseconds of the pre-pass (the test entries' scores and keys) of the most recent SLIMGPU_ModelRanks /
   SLIMGPU_ModelEvaluateRanked on this thread, from HIP events of its own; it is part of kernel_ms */
double SLIMGPU_LastRankPrepassMs(void);

#ifdef __cplusplus
}
#endif
#endif /* SLIM_AMD_SLIM_GPU_RANK_H_ */
