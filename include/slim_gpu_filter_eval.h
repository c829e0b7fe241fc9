/*
 * slim_gpu_filter_eval.h -- engine extensions of libslim.so: the evaluation and the ranks of slim_gpu_eval.h /
 * slim_gpu_rank.h, and the model-selection grid, under a candidate filter of slim_gpu_filter.h.  Included by
 * slim_gpu_filter.h; plain C types only.
 *
 * The candidates of a user are those of slim_gpu_filter.h: touched by the history, not in it, allowed by the item
 * set and not in the exclusion row of the USER ID -- users[q] on an eval set made for a user list, never the
 * position.  (The declarations have a header of their own: slim_gpu_filter.h is the list calls'.)  A test entry the filter
 * removes stays in its test row: it counts in nvalid, nvalid_head, nvalid_tail and in every denominator, with its
 * head / tail class; it is a miss at every cutoff; its rank is 0 and its score 0, like any non-candidate of
 * slim_gpu_rank.h.  That is what SLIMGPU_Evaluate gives on the filtered lists -- a caller who wants such entries
 * out of the denominators removes them from the test matrix.  Bit for bit:
 *   - for every cutoff c <= 128 the figures of SLIMGPU_ModelEvaluateAtFiltered are those of SLIMGPU_Evaluate on the
 *     filtered lists of length c (the first c survivors of the unfiltered full ranking);
 *   - for every N, test item t stands at position r of the filtered list of length N iff rank == r + 1 <= N, with
 *     that list's score;
 *   - SLIMGPU_ModelEvaluateRankedFiltered at cutoff c equals SLIMGPU_Evaluate on the filtered lists of length c, any c;
 *   - a filter that allows everything and excludes nothing, and filter == NULL, give the unfiltered call's output.
 * Once the filter's device copy exists the eval set's guarantee holds with it: no device allocation, nothing host
 * to device.
 */
#ifndef SLIM_AMD_SLIM_GPU_FILTER_EVAL_H_
#define SLIM_AMD_SLIM_GPU_FILTER_EVAL_H_

#include "slim_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SLIMGPU_ModelEvaluateAt / SLIMGPU_ModelRanks / SLIMGPU_ModelEvaluateRanked under a filter: outputs, limits
   and refusals are those of the unfiltered calls; a filter made for another ncols than the model's is
   SLIM_ERROR_INPUT with a SLIMGPU_LastError text, before anything is queued or written */
int32_t SLIMGPU_ModelEvaluateAtFiltered(slimgpu_evalset_t *es, const slimgpu_model_t *model,
                                        slimgpu_filter_t *filter, int32_t ncutoffs, double *metrics,
                                        int32_t *nvalid);
int32_t SLIMGPU_ModelRanksFiltered(slimgpu_evalset_t *es, const slimgpu_model_t *model, slimgpu_filter_t *filter,
                                   int32_t *ranks, float *scores);
int32_t SLIMGPU_ModelEvaluateRankedFiltered(slimgpu_evalset_t *es, const slimgpu_model_t *model,
                                            slimgpu_filter_t *filter, int32_t ncutoffs, const int32_t *cutoffs,
                                            double *metrics, int32_t *nvalid);
/* Py_SLIM_Mselect with every pair evaluated under a filter (NULL: Py_SLIM_Mselect itself).  At nrcmds <= 128 the
   eval set serves, above it the ranked eval set; SLIM_OPTION_GPU_EVALSTRIDE combines (exclusion rows by user
   id).  The header prints one more line: the items allowed out of ncols and the number of exclusion entries.
   A filtered grid needs the evaluation in HBM and a filter as wide as the resident models (slim_gpu_grid.h lists
   what that takes): anything else is SLIM_ERROR_INPUT before the first solve, with a SLIMGPU_LastError text that
   says which -- never an evaluation on the raw catalogue. */
int32_t Py_SLIM_MselectFiltered(slim_t *trnhandle, slim_t *tsthandle, int32_t *ioptions, double *doptions,
                                double *arrayl1, double *arrayl2, int32_t nl1, int32_t nl2, double *bestl1HR,
                                double *bestl2HR, double *bestHRHR, double *bestARHR, double *bestl1AR,
                                double *bestl2AR, double *bestHRAR, double *bestARAR, slimgpu_filter_t *filter);

#ifdef __cplusplus
}
#endif
#endif /* SLIM_AMD_SLIM_GPU_FILTER_EVAL_H_ */
