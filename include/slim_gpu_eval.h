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
 * the lists of SLIMGPU_ModelPredict, bit for bit.  28 bytes cross PCIe. */
int32_t SLIMGPU_ModelEvaluate(slimgpu_evalset_t *es, const slimgpu_model_t *model,
                              double *metrics, int32_t *nvalid);
/* Top-N of every row of the resident matrix through a resident model: only the lists come down.
 * Bit-identical to SLIMGPU_ModelPredict on the host handle of the same rows. */
int32_t SLIMGPU_MatrixPredict(int32_t nrcmds, const slimgpu_model_t *model,
                              slimgpu_matrix_t *mat, int32_t *output, float *scores);
/* Counters of the most recent SLIMGPU_ModelEvaluate / SLIMGPU_MatrixPredict on this thread. */
typedef struct slimgpu_eval_stats_t {
  int32_t path;          /* 1 fused chunk kernel, 2 wave kernel + k_user_terms */
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
