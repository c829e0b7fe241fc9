/*
 * slim_gpu_exposure.h -- engine extensions of libslim.so: what the top-N lists show.  Per-item exposure counts,
 * catalogue coverage, tail share, concentration.  Included by slim_gpu_lists.h; plain C types only.
 *
 * The quantity.  Positions q = 0 .. npos - 1, each with a list L_q of len_q ids, and cutoffs c_0 < .. < c_{K-1},
 * 1 <= K <= SLIMGPU_MAX_CUTOFFS:
 *
 *     E_k[i] = #{ (q, p) : p < min(len_q, c_k), L_q[p] == i }        i in [0, ncols)
 *
 * E counts places: the engine's lists never repeat an id, a caller's may, and each place counts.  A counted place
 * whose id lies outside [0, ncols) is skipped and tallied in `outside` (the engine's own lists hold none).  A slot
 * at or beyond len_q is never read for its meaning: callers leave anything there.  The counters are uint32 and wrap;
 * only a caller's lists with repeated ids can reach that (engine lists: E_k[i] <= npos).
 *
 * Every double of slimgpu_exposure_t is the quotient of two exact integers: numerator and denominator are formed
 * in 128-bit integer arithmetic, each is converted to double once (round to nearest) and they are divided once;
 * slots == 0 gives 0.0.  float(num) / float(den) on Python ints gives the same bits.
 *
 * Worked example: ncols 6, lists [0,1,2] [0,2] [0,0,5] (lengths 3, 2, 3), cutoffs (1, 3),
 * fmarker = [0,0,1,1,1,1], pop = [10,5,3,1,1,2].
 *   cutoff 1: E = [3,0,0,0,0,0], slots 3, distinct 1, tail_slots 0, gini 15/18, avg_pop 10
 *   cutoff 3: E = [4,1,2,0,0,1], slots 8, distinct 4, tail_slots 3, coverage 4/6, tail_share 3/8, gini 26/48,
 *             avg_pop 53/8
 *
 * The device calls count where the lists are: one kernel (exposure.hip) adds every place once, into the counter
 * of its band b(p) = min{k : p < c_k}, in LDS counters over a window of item ids; a second pass turns the bands
 * into E_k = B_0 + .. + B_k.  Only the counters come down (4 * K * ncols bytes); the summary is formed from them on
 * the host.  Results are integers, hence the same whatever the window and the grid are.  Environment, for tests:
 * SLIM_EXPOSURE_WINDOW=<ids> caps the ids of one LDS window.
 *
 * SLIM_ERROR_INPUT with a SLIMGPU_LastError text, before anything is queued or written: cutoffs unsorted, repeated,
 * < 1, more than SLIMGPU_MAX_CUTOFFS, cutoffs[K-1] > nrcmds; ncutoffs different from the eval set's; an eval set
 * without a list length (SLIMGPU_EvalSetCreateRanked); ncols < 1; nlists < 0; a counts[q] outside [0, nrcmds]; null
 * lists with nlists > 0; a filter of another width; model and matrix on different devices; a matrix whose
 * duplicates were merged.  Without a device, or with SLIM_PREDICT=cpu, only SLIMGPU_ListExposure works.
 *
 * Not built: exposure of candidate-set and sampled lists, several GPUs, position-discounted exposure, per-user-group
 * exposure, choosing the best pair by exposure, slim_predict.
 */
#ifndef SLIM_AMD_SLIM_GPU_EXPOSURE_H_
#define SLIM_AMD_SLIM_GPU_EXPOSURE_H_

#include "slim_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slimgpu_evalset slimgpu_evalset_t; /* (slim_gpu_eval.h) */
typedef struct slimgpu_filter slimgpu_filter_t;   /* (slim_gpu_filter.h) */

typedef struct slimgpu_exposure_t {
  int64_t lists;        /* positions counted, empty lists included                         */
  int64_t slots;        /* sum_i E[i]                                                      */
  int64_t tail_slots;   /* sum of E[i] over items with fmarker[i] != 0 or i >= fm_ncols
                           (the class rule of the evaluation); 0 when fmarker == NULL      */
  int64_t outside;      /* counted places skipped for an id outside [0, ncols)             */
  int32_t distinct;     /* #{i : E[i] > 0}                                                 */
  int32_t ncols;
  double coverage;      /* distinct / ncols                                                */
  double tail_share;    /* tail_slots / slots                                              */
  double gini;          /* sum_{j=1..n} (2j - n - 1) x_(j) / (n * slots): x_(1) <= .. <= x_(n)
                           are the E[i] ascending, n = ncols                               */
  double avg_pop;       /* sum_i E[i] * pop[i] / slots; pop NULL: 0                        */
} slimgpu_exposure_t;

/* host only, no device: the definition in code (host_csr.cpp).  ids: [nlists][nrcmds]; counts NULL: every list
   has nrcmds places.  exposure: [ncutoffs][ncols] uint32 or NULL; summary: [ncutoffs] or NULL */
int32_t SLIMGPU_ListExposure(int32_t ncols, const uint32_t *pop, const int32_t *fmarker, int32_t fm_ncols,
                             int64_t nlists, int32_t nrcmds, const int32_t *ids, const int32_t *counts,
                             int32_t ncutoffs, const int32_t *cutoffs, uint32_t *exposure,
                             slimgpu_exposure_t *summary);
/* the same lists counted on mat's device (uploaded, counted by the kernel): ncols and pop (column counts) are
   mat's; outputs bit-equal to SLIMGPU_ListExposure */
int32_t SLIMGPU_MatrixListExposure(slimgpu_matrix_t *mat, const int32_t *fmarker, int32_t fm_ncols, int64_t nlists,
                                   int32_t nrcmds, const int32_t *ids, const int32_t *counts, int32_t ncutoffs,
                                   const int32_t *cutoffs, uint32_t *exposure, slimgpu_exposure_t *summary);
/* the lists of SLIMGPU_MatrixPredictListsFiltered (same users / filter arguments, 1 <= nrcmds <= SLIMGPU_MAX_LIST,
   cutoffs[ncutoffs-1] <= nrcmds) counted where they are made: no list comes down.  Above 128 the long-list path
   serves; its user slices are counted one after the other into the same counters */
int32_t SLIMGPU_MatrixPredictExposure(slimgpu_matrix_t *mat, const slimgpu_model_t *model, int32_t nrcmds,
                                      int32_t nusers, const int32_t *users, slimgpu_filter_t *filter,
                                      const int32_t *fmarker, int32_t fm_ncols, int32_t ncutoffs,
                                      const int32_t *cutoffs, uint32_t *exposure, slimgpu_exposure_t *summary);
/* SLIMGPU_ModelEvaluateAtFiltered (filter NULL: SLIMGPU_ModelEvaluateAt) and, from the same scoring pass, the
   exposure of the lists behind it at the eval set's cutoffs, users and fmarker: every selected user's list
   counts, with or without a test row.  From the second call on an eval set: no device allocation, nothing host to
   device, device to host the evaluation's 8 + 32 * K bytes and the 4 * K * ncols of the counters (they always
   come down: the summary is formed from them); slimgpu_eval_stats_t as for the evaluation, path 1 or 2 */
int32_t SLIMGPU_ModelEvaluateExposure(slimgpu_evalset_t *es, const slimgpu_model_t *model, slimgpu_filter_t *filter,
                                      int32_t ncutoffs, double *metrics, int32_t *nvalid, uint32_t *exposure,
                                      slimgpu_exposure_t *summary);

enum { SLIM_OPTION_GPU_EVALEXPOSURE = 26 };   /* Py_SLIM_Mselect*: 1 = one exposure line per pair; -1 / 0: off */
#define SLIMGPU_EXPOSURE_CELL 8               /* l1, l2, HR, ARHR, coverage, tail_share, gini, avg_pop */
/* Py_SLIM_MselectFiltered (filter NULL: Py_SLIM_Mselect) with slot 26 forced on; cells:
   [nl1*nl2][SLIMGPU_EXPOSURE_CELL] in the order the pairs are solved, or NULL.  With slot 26 every pair line is
   followed by one line of the lists of the grid's nrcmds: coverage, tail_share, gini, avg_pop, distinct, slots.
   The slot needs the evaluation in HBM (slim_gpu_grid.h lists what that takes) and lists of at most 128: without
   it, with nrcmds > 128 or with sampled negatives (slot 23) the call is SLIM_ERROR_INPUT before the first solve,
   with a text that says which.  SLIM_OPTION_GPU_EVALSTRIDE and a filter combine.  The choice of the best pairs is
   unchanged */
int32_t Py_SLIM_MselectExposure(slim_t *trnhandle, slim_t *tsthandle, int32_t *ioptions, double *doptions,
                                double *arrayl1, double *arrayl2, int32_t nl1, int32_t nl2, double *bestl1HR,
                                double *bestl2HR, double *bestHRHR, double *bestARHR, double *bestl1AR,
                                double *bestl2AR, double *bestHRAR, double *bestARAR, slimgpu_filter_t *filter,
                                double *cells);

#ifdef __cplusplus
}
#endif

#endif /* SLIM_AMD_SLIM_GPU_EXPOSURE_H_ */
