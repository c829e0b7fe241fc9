/*
 * slim_gpu_explain.h -- engine extensions of libslim.so: which history items carry a candidate's score.
 * Included by slim_gpu_cand.h; plain C types only.
 *
 * A SLIM score is a sum over the user's history, score(u, i) = sum_p r[u, h_p] * w[h_p, i].  The calls here keep
 * the terms apart: for every selected user u and every slot j of its candidate row (slot id i) they return how
 * many history positions contribute and the largest contributions ("because you bought X").
 *
 * Terms of a slot: one per history position p (history order, the order the scorers walk) whose model row h_p
 * stores an entry for i.  t_p = r[u, h_p] * w[h_p, i], a float product rounded on its own as the 1-vs-k scorer
 * forms it; r = 1 for a binary history.  A stored coefficient of 0.0f or -0.0f is still a term.  A history id
 * without a model row contributes nothing.  A history that holds an item twice gives one term per position.
 * Slots that carry nothing, as slim_gpu_cand.h puts the score: an id outside [0, ncols), every occurrence of a
 * repeated id but the last, an id that no history row touches.  For them support = 0 and nothing else is written.
 *
 * support[cptr[u] + j]: the number of terms, all of them and not min(.., nwhy).
 * The explanation: the first min(nwhy, support) terms ordered by term value descending, then position ascending;
 * -0.0f and 0.0f compare equal in that order; the term returned is the product as computed, sign of zero included.
 *   why_items[(cptr[u] + j) * nwhy + r] = h_p (engine item id), why_terms[(cptr[u] + j) * nwhy + r] = t_p.
 * Places beyond min(nwhy, support) stay as the caller filled them, and so do the rows of users not selected,
 * support included.
 *
 * What ties this to the scorers: a slot with support <= nwhy, its terms put back into position order and added
 * from 0.0f one float addition each, gives the slot score of SLIMGPU_ScoreCandidates / Py_SLIM_GetTopN_1vsk bit
 * for bit.  No candidate filter applies; history items are explained like any other candidate.
 *
 * why_items / why_terms may both be NULL (support only); one of the two alone is SLIM_ERROR_INPUT.  support may be
 * NULL.  SLIM_ERROR_INPUT with a SLIMGPU_LastError text that names the call and every output untouched: a set made
 * for another ncols, too few rows for a selected user, matrix and model on different devices, a matrix whose
 * duplicates were merged, nwhy outside [1, SLIMGPU_MAX_WHY], and on the device model rows that do not ascend
 * strictly by id or 2^31 model entries or more.
 *
 * The device calls (slimgpu_eval_stats_t::path 6) do not slice the users: a call whose device outputs -- the
 * entries of the selected rows times (8 * nwhy + 4) bytes -- exceed half of the free device memory is
 * SLIM_ERROR_MEMORY before anything is written; pass user sub-lists then.  The outputs' device buffers belong to the
 * candidate set and only grow: from the second call of the same shapes on a resident pair there is no device
 * allocation and nothing goes host to device but the user list.  Environment, for tests:
 * SLIM_EXPLAIN_STAGE=<entries> history entries staged in LDS per user (default 1024), SLIM_EXPLAIN_FORM=16 takes
 * the kernel with 16 places per lane at every nwhy.
 */
#ifndef SLIM_AMD_SLIM_GPU_EXPLAIN_H_
#define SLIM_AMD_SLIM_GPU_EXPLAIN_H_

#include "slim_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLIMGPU_MAX_WHY 16
/* host model, host histories: every row of trn is selected */
int32_t SLIMGPU_ExplainCandidates(slim_t *model, slim_t *trn, slimgpu_candset_t *cs, int32_t nwhy,
                                  int32_t *why_items, float *why_terms, int32_t *support);
/* resident model, rows of the staged matrix; users as SLIMGPU_MatrixScoreCandidates takes them */
int32_t SLIMGPU_MatrixExplainCandidates(const slimgpu_model_t *model, slimgpu_matrix_t *mat,
                                        slimgpu_candset_t *cs, int32_t nusers, const int32_t *users,
                                        int32_t nwhy, int32_t *why_items, float *why_terms, int32_t *support);
/* policy-routed (SLIM_PREDICT=gpu|cpu|auto) with the host fallback, like Py_SLIM_ScoreCandidates */
int32_t Py_SLIM_ExplainCandidates(slim_t *model, slim_t *trn, slimgpu_candset_t *cs, int32_t nwhy,
                                  int32_t *why_items, float *why_terms, int32_t *support);

#ifdef __cplusplus
}
#endif

#endif /* SLIM_AMD_SLIM_GPU_EXPLAIN_H_ */
