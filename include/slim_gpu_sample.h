/*
 * slim_gpu_sample.h -- engine extensions of libslim.so: sampled negatives for the 1-vs-k protocol.  Candidate sets
 * (slim_gpu_cand.h) whose rows are "nnegs sampled non-interacted items, then the held-out items", made where the
 * matrix and the test rows lie (SLIMGPU_EvalSetSampleCandidates) or on the host (SLIMGPU_CandSetSample), and
 * SLIMGPU_CandSetRows, which copies the rows of any set out.  Included by slim_gpu_cand.h; plain C types only.
 *
 * THE SAMPLER.  This text is the contract: the host call, the device call and any restatement of it give the same
 * rows bit for bit.  All arithmetic is unsigned 64-bit and wraps.  G = 0x9E3779B97F4A7C15.
 *
 *   mix64(z):       z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   base(seed, u)   = mix64(seed + G * (u + 1))               u is the USER ID, never the position in a user list
 *   key(seed, u, d) = mix64(base(seed, u) + G * (d + 1))
 *   item(seed, u, d) = ((key(seed, u, d) >> 32) * ncols) >> 32        in [0, ncols)
 *
 * For user u let X_u be the distinct ids in [0, ncols) of its history row united with its test row, E = |X_u| and
 * free = ncols - E.  Its negatives follow one of two rules.
 *
 *   Sparse rule, when 2 * (E + nnegs) <= ncols: the first nnegs distinct ids of item(seed, u, 0), item(seed, u, 1),
 *   ... that are not in X_u, in draw order.  A draw counts only at its first occurrence (of two equal draws the
 *   lower draw index is that occurrence).  The sequence stops at d = 16 * nnegs + 1024: every draw is accepted
 *   with probability >= 1/2, so a row that is short for that reason will not be seen; if it is, it is short on
 *   host and device alike.
 *
 *   Dense rule, otherwise (free <= nnegs included): the min(nnegs, free) ids i not in X_u with the smallest
 *   (key(seed, u, i), i), in that order -- uniform without replacement, at ncols hashes.
 *
 * The candidate row of a selected user with a non-empty test row is its negatives followed by its test row exactly
 * as staged (ids beyond ncols, repeats and history items included).  A user with an empty test row, or one the
 * user list does not select, has an empty row.  THE TIE RULE: the order of a row is score descending, then slot
 * ascending, and the held-out items stand BEHIND the negatives, so a score tie goes to the negative.  SLIM gives
 * many items the score 0; this is the pessimistic choice.  The sampler is uniform only: popularity-weighted
 * negatives are not built.
 *
 * A sampled set has min(rows of trn, rows of tst) rows and is an ordinary candidate set in every call of
 * slim_gpu_cand.h.  The device call writes the rows straight into the set's device copy and indexes them as an
 * uploaded set's are; of such a set the host keeps the row pointer only (8 bytes per user come down once) and
 * fetches the ids when SLIMGPU_CandSetRows or the host scorer (Py_SLIM_ScoreCandidates under SLIM_PREDICT=cpu)
 * first needs them.  The device sampler keeps X_u and the accepted ids as one bit per item in LDS, which bounds the
 * catalogue: at most SLIMGPU_SAMPLE_MAX_NCOLS items (a 64 KB bitmap); beyond that the device call is refused and
 * the host call serves.  A sampled evaluation costs about what the full-catalogue one costs -- the history walk
 * dominates this scorer -- so this is a protocol, not a speed-up.
 *
 * SLIM_ERROR_INPUT with a SLIMGPU_LastError text, *out untouched: nnegs < 1; nnegs + the longest selected test row
 * above SLIMGPU_MAX_LIST (the evaluation needs lists); a matrix whose duplicates were merged; the device call above
 * SLIMGPU_SAMPLE_MAX_NCOLS items; ncols < 1, a user list that does not ascend strictly inside the rows.
 */
#ifndef SLIM_AMD_SLIM_GPU_SAMPLE_H_
#define SLIM_AMD_SLIM_GPU_SAMPLE_H_

#include "slim_gpu_cand.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLIMGPU_SAMPLE_MAX_NCOLS 524288

/* the eval set's users, resident history rows and staged test rows (a list eval set or a ranked one alike) */
int32_t SLIMGPU_EvalSetSampleCandidates(slimgpu_evalset_t *es, int32_t nnegs, uint64_t seed,
                                        slimgpu_candset_t **out);
/* the same rows made on the host: users as SLIMGPU_MatrixPredictLists takes them (NULL and 0: every user) */
int32_t SLIMGPU_CandSetSample(int32_t ncols, slim_t *trn, slim_t *tst, int32_t nusers, const int32_t *users,
                              int32_t nnegs, uint64_t seed, slimgpu_candset_t **out);
/* copies a set's rows out: cptr[nrows + 1] and / or cind[entries] (either may be NULL), for any set; the sizes
   come from SLIMGPU_CandSetInfo (each of its outputs may be NULL) */
int32_t SLIMGPU_CandSetRows(slimgpu_candset_t *cs, int64_t *cptr, int32_t *cind);
int32_t SLIMGPU_CandSetInfo(slimgpu_candset_t *cs, int32_t *nrows, int32_t *ncols, int64_t *entries);

#ifdef __cplusplus
}
#endif

#endif /* SLIM_AMD_SLIM_GPU_SAMPLE_H_ */
