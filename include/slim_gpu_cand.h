/*
 * slim_gpu_cand.h -- engine extensions of libslim.so: per-user candidate sets, the 1-vs-k protocol at any k.
 * Included by slim_gpu.h; plain C types only.
 *
 * The caller brings the candidates of every user -- sampled negatives plus the held-out item, the union of
 * several generators -- and the model scores and orders exactly those.  For a user, every entry of its
 * candidate row gets the 1-vs-k score of Py_SLIM_GetTopN_1vsk (the reference's GetRec_1vsk, predict.c:77-133):
 *   - the float sum over the history in history order, products and sums rounded separately, from 0.0f;
 *   - history items are scored like any other item: this protocol does not exclude them;
 *   - an id never touched scores 0; an id outside [0, ncols) scores 0 and still takes part in the order;
 *   - of a repeated id the last occurrence carries the score, earlier ones score 0;
 *   - the order of a row is score descending, then slot ascending.
 * No candidate filter applies.
 *
 * The object validates once, on the host, and keeps a host copy (the host fallback reads it).  Its device copy is
 * made on the first call that scores on a device -- the rows as given and, per row, the live entries sorted by
 * id with their slot -- and kept until SLIMGPU_CandSetFree: later calls allocate and upload nothing for it.  A
 * set is tied to a number of items, not to a model.
 *
 * The device scorer is the chunk kernel (slimgpu_eval_stats_t::path 5): it needs model rows ascending by id,
 * fewer than 2^31 model entries and a split table of at most 2 GB; anything else is SLIM_ERROR_INPUT with a
 * SLIMGPU_LastError text and nothing is written.  One history walk per user serves a row of any length.
 *
 * Sampled negatives (slim_gpu_sample.h, included below): SLIMGPU_EvalSetSampleCandidates makes the set of the
 * 1-vs-k protocol on the device -- per evaluated user nnegs sampled non-interacted items, then its held-out items --
 * SLIMGPU_CandSetSample makes the same rows on the host, SLIMGPU_CandSetRows copies the rows of any set out.  The
 * held-out items stand behind the negatives, so under "score descending, then slot ascending" a score tie goes to
 * the negative: the pessimistic choice.  The option slots below put Py_SLIM_Mselect on that protocol.
 *
 * Explanations (slim_gpu_explain.h, included below): the terms behind a slot score, the largest of them per slot.
 *
 * Popularity-weighted negatives: SLIMGPU_EvalSetSampleCandidatesWeighted / SLIMGPU_CandSetSampleWeighted
 * (slim_gpu_sample.h states the rule) and option slot 25 below.
 *
 * Not built: the neg-file protocol of slim_predict (random tie order).
 * SLIMGPU_Predict1vsK is unchanged (rows of one width, up to 1024).
 */
#ifndef SLIM_AMD_SLIM_GPU_CAND_H_
#define SLIM_AMD_SLIM_GPU_CAND_H_

#include "slim_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slimgpu_candset slimgpu_candset_t;
/* rows: a CSR over user ids, ids as given (no order, repeats, out-of-range ids allowed).  cptr[0] != 0, a cptr
   that descends, a row of 2^31 entries or more, ncols < 1 are SLIM_ERROR_INPUT with a SLIMGPU_LastError text. */
int32_t SLIMGPU_CandSetCreate(int32_t ncols, int32_t nusers, const int64_t *cptr, const int32_t *cind,
                              slimgpu_candset_t **out);
void SLIMGPU_CandSetFree(slimgpu_candset_t *cs);

/* slot_scores (may be NULL): laid out like the set, slot_scores[cptr[u] + j]; rows of users not selected stay as
   the caller filled them.  nrcmds == 0: no lists; else output / scores are [positions][nrcmds], the first
   min(nrcmds, row length) of position q hold the row in order, the slots beyond stay as the caller filled them;
   counts (may be NULL) = list lengths.  Lists need rows of at most SLIMGPU_MAX_LIST entries: with a longer row
   among the selected users a call that asks for lists is SLIM_ERROR_INPUT before anything is written.  Also
   SLIM_ERROR_INPUT, outputs untouched: a set made for another ncols than the model's, a set with fewer rows than
   a selected user id needs, matrix and model on different devices, a matrix whose duplicates were merged. */
/* host model, host histories (every row of trn is selected) */
int32_t SLIMGPU_ScoreCandidates(slim_t *model, slim_t *trn, slimgpu_candset_t *cs, int32_t nrcmds,
                                float *slot_scores, int32_t *output, float *scores, int32_t *counts);
/* resident model, rows of the staged matrix; users as SLIMGPU_MatrixPredictLists takes them.  The candidate row
   of a position is that of its USER ID, never of the position. */
int32_t SLIMGPU_MatrixScoreCandidates(const slimgpu_model_t *model, slimgpu_matrix_t *mat, slimgpu_candset_t *cs,
                                      int32_t nusers, const int32_t *users, int32_t nrcmds,
                                      float *slot_scores, int32_t *output, float *scores, int32_t *counts);
/* HR / HR_head / HR_tail / ARHR of the candidate lists at the eval set's cutoffs and users, in HBM; metrics and
   nvalid as SLIMGPU_ModelEvaluateAt.  From the second call on: no device allocation, nothing host to device, at
   most 8 + 32 * ncutoffs bytes device to host. */
int32_t SLIMGPU_ModelEvaluateCandidates(slimgpu_evalset_t *es, const slimgpu_model_t *model, slimgpu_candset_t *cs,
                                        int32_t ncutoffs, double *metrics, int32_t *nvalid);
/* policy-routed (SLIM_PREDICT=gpu|cpu|auto) with a host fallback, like Py_SLIM_Predict */
int32_t Py_SLIM_ScoreCandidates(slim_t *model, slim_t *trn, slimgpu_candset_t *cs, int32_t nrcmds,
                                float *slot_scores, int32_t *output, float *scores, int32_t *counts);

/* Py_SLIM_Mselect / Py_SLIM_MselectFiltered on sampled negatives (slots beside SLIM_OPTION_GPU_EVALSTRIDE = 22):
   with EVALNEGS > 0 the candidate set is sampled once, on the device, after the eval set exists, and every pair is
   evaluated by SLIMGPU_ModelEvaluateCandidates' path -- HR / ARHR of the lists of nrcmds among nnegs negatives and
   the held-out items.  The header prints nnegs, the seed and the set's entries; the selection of the best pairs is
   unchanged; EVALSTRIDE combines.  SLIM_ERROR_INPUT before the first solve, with a text that says which: a filter,
   nrcmds > 128 (the candidate lists use the eval set's cutoffs), and whatever keeps the evaluation out of HBM
   (slim_gpu_grid.h has the list).  Never a fall-back to the full-catalogue figures. */
enum {
  SLIM_OPTION_GPU_EVALNEGS = 23, /* sampled negatives per user; -1 or 0: off */
  SLIM_OPTION_GPU_EVALSEED = 24, /* the sampler's seed; -1: 1 */
  /* 1: the negatives are drawn in proportion to item popularity (the weighted rule of slim_gpu_sample.h, NULL
     weights) and the header line says "popularity"; -1 or 0: uniformly.  1 with EVALNEGS off is SLIM_ERROR_INPUT
     before the first solve: there is nothing to weight */
  SLIM_OPTION_GPU_EVALNEGPOP = 25
};

#ifdef __cplusplus
}
#endif

#include "slim_gpu_sample.h"
#include "slim_gpu_explain.h"

#endif /* SLIM_AMD_SLIM_GPU_CAND_H_ */
