/*
 * slim_gpu_grid.h -- engine extensions of libslim.so: the evaluator of a model-selection grid.  What
 * Py_SLIM_Mselect* and slim_mselect loop over; plain C types only.
 *
 * A grid holds, between its pairs: the training matrix staged in HBM (none for ADMM), the head / tail marker, the
 * eval set (listed cutoffs up to 128, ranked above) and the sampled candidate set, the previous pair's model
 * (resident in HBM, or on the host for several GPUs, SLIM_GPU_RESIDENT=0 and ADMM) and the caller's filter, which
 * it borrows.  SLIMGPU_GridFree releases all of it but the filter and the two matrix handles, which stay the
 * caller's and must outlive the grid.
 *
 * What each evaluation mode needs -- the one list; the other headers point here.  All of it is judged by
 * SLIMGPU_GridOpen, before the first solve, and a refusal is SLIM_ERROR_INPUT with a SLIMGPU_LastError text that
 * names the first obstacle in the order below:
 *
 *   the evaluation in HBM   cd (ADMM leaves no model in HBM), one GPU, SLIM_GPU_RESIDENT not 0,
 *                           SLIM_GPU_EVAL_RESIDENT not 0, nrcmds >= 1, an eval set that could be made (a matrix
 *                           staged without merged pairs, SLIM_GPU_DUPLICATES)
 *   SLIM_OPTION_GPU_EVALSTRIDE (22)    at least 1; above 1 the evaluation in HBM
 *   SLIM_OPTION_GPU_EVALNEGS (23)      at least 0; above 0: no filter, the evaluation in HBM, nrcmds <= 128, a
 *                                      sampler that serves (slim_gpu_sample.h)
 *   SLIM_OPTION_GPU_EVALNEGPOP (25)    0 or 1; 1 needs slot 23
 *   SLIM_OPTION_GPU_EVALEXPOSURE (26)  0 or 1; 1: the evaluation in HBM, nrcmds <= 128, slot 23 off
 *   a filter                           the evaluation in HBM, a filter as wide as the staged matrix
 *   user groups (slim_gpu_groups.h)    group ids in [-1, ngroups), 1 to 1024 groups, select_group in [-1, ngroups);
 *                                      the evaluation in HBM.  Judged by SLIMGPU_GridSetGroups, after the open and
 *                                      before the first solve; they combine with every mode above
 *
 * A grid with none of these (a plain grid) never fails for want of the evaluation in HBM: it falls back to top-N
 * lists on the device and hit counting on the device, then to the host loop.  A strided, filtered, sampled, exposure
 * or grouped grid never falls back to the unrestricted figures: a pair that cannot be evaluated as asked is SLIM_ERROR.
 *
 * SLIM_GPU_NGPUS in the environment serves where ioptions leaves SLIM_OPTION_GPU_NGPUS at -1, as for SLIM_Learn.
 */
#ifndef SLIM_AMD_SLIM_GPU_GRID_H_
#define SLIM_AMD_SLIM_GPU_GRID_H_

#include "slim_gpu_exposure.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slimgpu_grid slimgpu_grid_t;

typedef struct slimgpu_grid_cell_t {
  double l1r, l2r;
  int64_t nnz;                 /* entries of the pair's model                                       */
  double metrics[4];           /* HR, HR of the head, HR of the tail, ARHR                          */
  int32_t nvalid[3];           /* evaluated users: all, with a head item held out, with a tail item */
  int32_t has_exposure;        /* 1 when slot 26 is on: exposure is the summary of the pair's lists */
  slimgpu_exposure_t exposure;
  double solve_seconds;        /* the solve alone (SLIMGPU_LastStats: total_ms)                     */
} slimgpu_grid_cell_t;

/* ncols: the width of the head / tail marker; 0: the larger of the two matrices' largest id + 1, as
   Py_SLIM_Mselect takes it.  nsolves: the pairs to come (SLIMGPU_MatrixExpectSolves).  filter may be NULL.  On a
   refusal *grid is left as it was */
int32_t SLIMGPU_GridOpen(slim_t *trnhandle, slim_t *tsthandle, int32_t *ioptions, double *doptions, int32_t ncols,
                         int32_t nsolves, slimgpu_filter_t *filter, slimgpu_grid_t **grid);
/* (SLIMGPU_GridOpenOn, the same grid over a training matrix that is staged already: slim_gpu_split.h) */
/* the header lines of the modes in use, to stdout: "  evaluating every K-th user ...", "  item filter ...",
   "  sampled negatives ..." */
void SLIMGPU_GridDescribe(const slimgpu_grid_t *grid);
/* the next pair: learnt from the previous pair's model, evaluated as the grid was opened.  On a failure the
   status of what failed; the previous model is gone either way, and the next pair starts from scratch */
int32_t SLIMGPU_GridSolve(slimgpu_grid_t *grid, double l1r, double l2r, slimgpu_grid_cell_t *cell);
/* the host model of the last solved pair (fetched on the first request when it is resident); the grid's until the
   next SLIMGPU_GridSolve or SLIMGPU_GridFree.  NULL with *status set when there is none */
slim_t *SLIMGPU_GridModel(slimgpu_grid_t *grid, int32_t *status);
/* grid or *grid NULL: nothing happens */
void SLIMGPU_GridFree(slimgpu_grid_t **grid);

#ifdef __cplusplus
}
#endif

#endif /* SLIM_AMD_SLIM_GPU_GRID_H_ */
