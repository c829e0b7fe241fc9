/*
 * slim_gpu_eval.h -- engine extensions of libslim.so for the evaluate half of a model-selection
 * grid: a resident model (slim_gpu.h: SLIMGPU_LearnResident) scored and evaluated against the
 * training matrix staged in HBM.  Included by slim_gpu.h; plain C types only.
 */
#ifndef SLIM_AMD_SLIM_GPU_EVAL_H_
#define SLIM_AMD_SLIM_GPU_EVAL_H_

#include "slim_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLIMGPU_MAX_CUTOFFS 8 /* list lengths one eval set serves (SLIMGPU_EvalSetCreateAt) */

/* Evaluation without leaving HBM.  Every cell of a model-selection grid is learn + evaluate
 * (src/programs/slim_mselect.c:99-196, src/libslim/pyapi.c:283-375); with the model resident and R
 * staged, the evaluation needs nothing from the host but the test set, which is staged once per
 * grid.  SLIMGPU_EvalSetCreate holds the test rows (tsthandle's row view), fmarker[fm_ncols]
 * (SLIM_DetermineHeadAndTail's output) and every workspace the scorer needs for lists of nrcmds
 * (1..128); the history is mat's CSR where it lies, users = min(mat rows, test rows) as pyapi.c
 * does.  It borrows mat, which must outlive it.  A matrix whose repeated pairs were merged at
 * staging (SLIM_GPU_DUPLICATES=sum) no longer holds the caller's rows -- a score would round
 * differently from the reference's per-entry additions -- and is refused with SLIM_ERROR_INPUT, by
 * SLIMGPU_MatrixPredict too.  Matrix, model and eval set must live on one device (SLIM_ERROR_INPUT
 * otherwise); the work runs on the matrix's stream. */
typedef struct slimgpu_evalset slimgpu_evalset_t;
slimgpu_evalset_t *SLIMGPU_EvalSetCreate(slimgpu_matrix_t *mat, slim_t *tsthandle,
                                         const int32_t *fmarker, int32_t fm_ncols,
                                         int32_t nrcmds, int32_t *r_status);
void SLIMGPU_EvalSetFree(slimgpu_evalset_t **es);
/* metrics = {HR, HR_head, HR_tail, ARHR}, nvalid[3]: exactly the outputs SLIMGPU_Evaluate gives for
 * the lists of SLIMGPU_ModelPredict, bit for bit.  40 bytes cross PCIe.  The last row of
 * SLIMGPU_ModelEvaluateAt: on an eval set made by SLIMGPU_EvalSetCreateAt, the figures of its largest
 * cutoff over its users. */
int32_t SLIMGPU_ModelEvaluate(slimgpu_evalset_t *es, const slimgpu_model_t *model,
                              double *metrics, int32_t *nvalid);

/* Several list lengths and a subset of the users from ONE scoring pass.  The scorer's order is total
 * (score descending, then discovery order), so the list of length c is the first c ranks of a longer
 * list, and a user's hits are walked once in rank order: the float additions behind cutoff k are a
 * prefix of those behind cutoff k + 1.  Users are scored independently of each other.  Hence the
 * contract: row k of SLIMGPU_ModelEvaluateAt equals, bit for bit, SLIMGPU_ModelEvaluate on an eval set
 * created with nrcmds = cutoffs[k] over a matrix and a test set that hold exactly the selected users'
 * rows, in list order.  SLIMGPU_EvalSetCreate(.., nrcmds, ..) is SLIMGPU_EvalSetCreateAt(.., 1, &nrcmds,
 * 0, NULL, ..).  A malformed list -- unsorted, repeated, out of range, more than SLIMGPU_MAX_CUTOFFS
 * cutoffs, a cutoff of 0 or 129 -- is SLIM_ERROR_INPUT with a SLIMGPU_LastError text.  From the second
 * evaluation on: no device allocation, nothing host to device, at most 8 + 32 * ncutoffs bytes device to
 * host.  In slimgpu_eval_stats_t, w_rows_read and w_bytes count the selected users only; path follows
 * the largest cutoff (1 up to 64, 2 above). */
/* Like SLIMGPU_EvalSetCreate, for `ncutoffs` list lengths (strictly ascending, 1 <= c <= 128,
 * 1 <= ncutoffs <= SLIMGPU_MAX_CUTOFFS) and, when users != NULL, for the `nusers` listed users only
 * (strictly ascending ids in [0, min(mat rows, test rows)), nusers >= 1; users == NULL needs
 * nusers == 0 and means every user).  Lists are copied; staged once, like the test rows. */
slimgpu_evalset_t *SLIMGPU_EvalSetCreateAt(slimgpu_matrix_t *mat, slim_t *tsthandle,
                                           const int32_t *fmarker, int32_t fm_ncols,
                                           int32_t ncutoffs, const int32_t *cutoffs,
                                           int32_t nusers, const int32_t *users, int32_t *r_status);
/* metrics[k*4 .. +4) = {HR, HR_head, HR_tail, ARHR}, nvalid[k*3 .. +3) for cutoff k, from ONE scoring
 * pass.  ncutoffs must equal the eval set's (SLIM_ERROR_INPUT otherwise). */
int32_t SLIMGPU_ModelEvaluateAt(slimgpu_evalset_t *es, const slimgpu_model_t *model,
                                int32_t ncutoffs, double *metrics, int32_t *nvalid);
/* Option slot of Py_SLIM_Mselect (and slim_mselect -evalstride=K): with K > 1 the grid evaluates users
 * 0, K, 2K, ... only; -1 or 1: every user.  Needs the evaluation in HBM (slim_gpu_grid.h lists what that
 * takes): without it the call fails with SLIM_ERROR_INPUT before the first solve.  (nrcmds above 128 is served
 * from the ranks of the held-out items, slim_gpu_rank.h.) */
enum { SLIM_OPTION_GPU_EVALSTRIDE = 22 };
/* Top-N of every row of the resident matrix through a resident model: only the lists come down.
 * Bit-identical to SLIMGPU_ModelPredict on the host handle of the same rows. */
int32_t SLIMGPU_MatrixPredict(int32_t nrcmds, const slimgpu_model_t *model,
                              slimgpu_matrix_t *mat, int32_t *output, float *scores);
/* Counters of the most recent SLIMGPU_ModelEvaluate / SLIMGPU_MatrixPredict on this thread. */
typedef struct slimgpu_eval_stats_t {
  int32_t path;          /* 1 fused chunk kernel, 2 wave kernel + k_user_terms, 3 ranks (slim_gpu_rank.h),
                            4 long lists (slim_gpu_lists.h), 5 candidate rows (slim_gpu_cand.h),
                            6 explanations (slim_gpu_explain.h), 7 a split (slim_gpu_split.h) */
  int32_t device_allocs; /* device allocations made by this call               */
  int64_t h2d_bytes, d2h_bytes;
  double kernel_ms, total_ms;
  int64_t w_rows_read;   /* model rows streamed: sum of history lengths        */
  double w_bytes;        /* their bytes (8 per entry): the scorer's byte model */
} slimgpu_eval_stats_t;
int32_t SLIMGPU_LastEvalStats(slimgpu_eval_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* SLIM_AMD_SLIM_GPU_EVAL_H_ */
