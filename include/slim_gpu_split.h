/*
 * slim_gpu_split.h -- engine extensions of libslim.so: one interactions matrix split into a train and a test matrix,
 * reproducibly from a seed, on the host (SLIMGPU_SplitHost) or where the staged matrix lies (SLIMGPU_MatrixSplit).
 * Included by slim_gpu.h; plain C types only.
 *
 * THE RULE.  This text is the contract: the host call, the device call and any restatement of it give the same rows
 * bit for bit.  mix64, G, base(seed, u), key(seed, u, i) and mulhi64 are those of slim_gpu_sample.h, exactly; all
 * arithmetic is unsigned 64-bit and wraps.  u is the USER ID (the row), i the ITEM ID of a stored entry.
 *
 *   SLIMGPU_SPLIT_LEAVE_OUT (F = nfolds >= 1, f = fold in [0, F), h = nheld >= 1, m = minkeep >= 1, F * h <= 128).
 *   Order the L stored entries of row u by (key(seed, u, item), item, position in the row), ascending.  The user
 *   takes part when L >= F * h + m; its held-out entries in fold f are those at ranks [f * h, (f + 1) * h) of that
 *   order.  The test rows of the F folds are therefore disjoint, and every user that takes part holds out exactly h
 *   entries in every fold.  (F * h <= 128: per row this is a "128 smallest keys" selection, never a sort.)
 *
 *   SLIMGPU_SPLIT_FOLDS (F >= 2, f in [0, F), m >= 1; nheld is not read).  The usual (F - 1) / F : 1 / F split:
 *   entry (u, i) belongs to fold mulhi64(key(seed, u, i), F).  The user takes part in fold f when at least m of its
 *   entries lie outside fold f and at least one lies inside; its held-out entries are those inside.
 *
 *   In both modes a user that does not take part keeps its whole row in train and has an empty test row.  The train
 *   row is the source row minus the held-out entries, the test row the held-out entries; both keep the source row's
 *   order and carry the source values (rowval; none for a binary matrix), so a history walk adds in the order it
 *   always did.  Both outputs have the source's number of rows.
 *
 * SLIM_ERROR_INPUT with a SLIMGPU_LastError text and the outputs untouched: a mode other than the two; nfolds < 1
 * (< 2 for folds); fold outside [0, nfolds); minkeep < 1; in leave-out mode nheld < 1 or nfolds * nheld > 128; a
 * staged matrix whose repeated pairs were merged (SLIM_GPU_DUPLICATES=sum: its rows are not the caller's, the reason
 * the eval set refuses it); in the host call an item id below 0.
 *
 * SLIMGPU_SplitHost is plain C++ on one thread.  Both of its outputs, and the test matrix of SLIMGPU_MatrixSplit, are
 * matrices as Py_csr_wrapper makes them (ncols = largest id + 1) and are released by Py_csr_free.
 *
 * SLIMGPU_MatrixSplit reads a matrix staged on one device.  The train half is written into fresh device arrays and
 * staged as SLIMGPU_MatrixFromDevice stages them (ncols = its largest id + 1, what SLIMGPU_MatrixFromHost of the host
 * call's train rows has); the new handle owns its arrays, lives on the source's device and is released by
 * SLIMGPU_MatrixFree.  Only the test half comes down: 8 bytes per row for the row pointer and 8 bytes per held-out
 * entry (4 for a binary matrix), plus 12 bytes of the staging's own (the train half's entries and largest id).
 * Nothing goes up.  SLIMGPU_LastEvalStats reports the call: path 7, h2d_bytes, d2h_bytes, device_allocs, kernel_ms
 * (the mark pass with the scan, plus the scatter pass; not the row pointer's way down and the allocations between
 * them) and total_ms.
 *
 * THE CROSS-VALIDATED GRID.  Py_SLIM_MselectCV is Py_SLIM_Mselect for a caller with ONE interactions matrix: the
 * l1 x l2 grid is run once per fold f = 0 .. F - 1 of `split` (its `fold` is not read) and a pair is judged by the
 * mean of its fold figures.  The data is staged once for all folds; per fold SLIMGPU_MatrixSplit cuts it where it
 * lies, SLIMGPU_GridOpenOn (below) opens the grid on the train half with nsolves = nl1 * nl2, every pair is
 * solved and printed as Py_SLIM_Mselect prints it under a "fold f of F" header, and the grid is freed.  Option slots
 * 22 - 26 (stride, sampled negatives and their seed, popularity, exposure) and the filter pass to every fold's grid
 * unchanged.  Where the device split cannot serve -- several GPUs, ADMM, SLIM_GPU_RESIDENT=0, and
 * SLIM_GPU_EVAL_RESIDENT=0, where a grid needs host rows to score -- every fold is split by SLIMGPU_SplitHost and its
 * grid opened from the host handles (SLIMGPU_GridOpen): the folds are the same, and so are the figures.
 *
 *   A pair's CV figure is the mean of its fold figures, summed as doubles in fold order and divided by F.  The best
 *   pairs are chosen on the mean HR and on the mean ARHR with Py_SLIM_Mselect's strict `>` in grid order (l1 outer,
 *   l2 inner); the eight outputs are those of Py_SLIM_Mselect with means for figures.  A fold in which a pair has
 *   nvalid < 1 ends the call as it ends Py_SLIM_Mselect (SLIM_ERROR, the pair in bestl1HR / bestl2HR).  One summary
 *   line per pair closes the output: mean, minimum and maximum of HR and ARHR over the folds.
 *
 *   cells (optional): [F][nl1 * nl2][SLIMGPU_CV_CELL] doubles, row (f, a * nl2 + b) = fold, l1, l2, HR, HR_head,
 *   HR_tail, ARHR, nvalid, nvalid_head, nvalid_tail, the model's entries -- the figures of SLIMGPU_GridSolve, as
 *   doubles.
 *
 * Not built: temporal splits (the hash sees no time stamp), user-level (cold-start) folds, user groups inside a
 * cross-validated grid, a split on several GPUs (a handle with replicas is split on its first device; the result
 * has no replicas).
 */
#ifndef SLIM_AMD_SLIM_GPU_SPLIT_H_
#define SLIM_AMD_SLIM_GPU_SPLIT_H_

#ifdef __cplusplus
extern "C" {
#endif

#define SLIMGPU_SPLIT_LEAVE_OUT 0
#define SLIMGPU_SPLIT_FOLDS 1
#define SLIMGPU_SPLIT_MAX_HELD 128 /* nfolds * nheld, leave-out mode */
#define SLIMGPU_EVAL_PATH_SPLIT 7  /* slimgpu_eval_stats_t::path of SLIMGPU_MatrixSplit */

typedef struct slimgpu_split_t {
  int32_t mode;    /* SLIMGPU_SPLIT_LEAVE_OUT or SLIMGPU_SPLIT_FOLDS */
  int32_t nfolds;  /* F                                              */
  int32_t fold;    /* f in [0, F)                                    */
  int32_t nheld;   /* h; leave-out mode only                         */
  int32_t minkeep; /* m: entries a user's train row must keep        */
  uint64_t seed;   /* seed of the hash                               */
} slimgpu_split_t;

int32_t SLIMGPU_SplitHost(slim_t *data, const slimgpu_split_t *split, slim_t **trn, slim_t **tst);
int32_t SLIMGPU_MatrixSplit(slimgpu_matrix_t *src, const slimgpu_split_t *split, slimgpu_matrix_t **trn,
                            slim_t **tst);

typedef struct slimgpu_grid slimgpu_grid_t;       /* (slim_gpu_grid.h) */
typedef struct slimgpu_filter slimgpu_filter_t;   /* (slim_gpu_filter.h) */
/* SLIMGPU_GridOpen (slim_gpu_grid.h) over a training matrix that is staged already, on one device (the train half of
   SLIMGPU_MatrixSplit): nothing of the training rows is on the host.  The grid OWNS the matrix once
   this returns SLIM_OK and SLIMGPU_GridFree releases it; on a refusal the matrix stays the caller's.  The head / tail
   marker is formed from the matrix's column pointer (8 bytes per item come down) and equals
   SLIM_DetermineHeadAndTail on the same rows exactly; ncols 0: the larger of the matrix's width and the test rows'
   largest id + 1.  Such a grid keeps its models in HBM and evaluates them there, so beside what the modes of
   slim_gpu_grid.h need it is refused (SLIM_ERROR_INPUT) for ADMM, several GPUs, SLIM_GPU_RESIDENT=0, SLIM_GPU_EVAL_RESIDENT=0, nrcmds < 1
   and an eval set that cannot be made; SLIMGPU_GridOpen on host handles serves there */
int32_t SLIMGPU_GridOpenOn(slimgpu_matrix_t *trn, slim_t *tsthandle, int32_t *ioptions, double *doptions,
                           int32_t ncols, int32_t nsolves, slimgpu_filter_t *filter, slimgpu_grid_t **grid);

#define SLIMGPU_CV_CELL 11
int32_t Py_SLIM_MselectCV(slim_t *datahandle, int32_t *ioptions, double *doptions, double *arrayl1, double *arrayl2,
                          int32_t nl1, int32_t nl2, const slimgpu_split_t *split, slimgpu_filter_t *filter,
                          double *bestl1HR, double *bestl2HR, double *bestHRHR, double *bestARHR, double *bestl1AR,
                          double *bestl2AR, double *bestHRAR, double *bestARAR, double *cells);
/* the same over a list of pairs, solved in the order given (an l12 file: slim_mselect -cvfolds); best[8]: the eight
   outputs in Py_SLIM_MselectCV's order; cells: [F][npairs][SLIMGPU_CV_CELL] or NULL */
int32_t SLIMGPU_MselectCVPairs(slim_t *datahandle, int32_t *ioptions, double *doptions, int32_t npairs,
                               const double *l1, const double *l2, const slimgpu_split_t *split,
                               slimgpu_filter_t *filter, double *best, double *cells);

#ifdef __cplusplus
}
#endif

#endif /* SLIM_AMD_SLIM_GPU_SPLIT_H_ */
