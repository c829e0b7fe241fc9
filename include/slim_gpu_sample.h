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
 * many items the score 0; this is the pessimistic choice.
 *
 * THE WEIGHTED RULE (SLIMGPU_EvalSetSampleCandidatesWeighted, SLIMGPU_CandSetSampleWeighted; declared in
 * slim_gpu_wsample.h, included below): negatives drawn in proportion to a weight per item -- item popularity, the
 * other published kind of 1-vs-k.  mix64, G, base and key are those above; mulhi64(a, b) is the upper 64 bits of the
 * 128-bit product; all arithmetic is unsigned and exact.
 *
 *   Weights.  The caller gives w[0 .. ncols) as uint32_t, or NULL for "popularity": on the device the number of
 *   stored entries of column i in all rows of the resident matrix, on the host the number of entries of all rows of
 *   trn with id i in [0, ncols).  C[i] = w[0] + ... + w[i-1] in 64 bits and T = C[ncols].  T = 0 is refused.  An
 *   item of weight 0 is never a negative.
 *
 *   One draw.  pick(d) = the item i with C[i] <= mulhi64(key(seed, u, d), T) < C[i+1].
 *
 *   Phase 1, rejection.  The negatives are the first nnegs distinct ids of pick(0), pick(1), ... outside X_u, in draw
 *   order; a draw counts at its first occurrence; the sequence stops at D = 16 * nnegs + 1024 draws.  Drawing from
 *   the full weights and rejecting what is taken is exactly successive weighted sampling without replacement.
 *
 *   Phase 2, only when phase 1 ended short.  F = the items of positive weight neither in X_u nor accepted.  For
 *   j = 0 ... min(nnegs - got, |F|) - 1: R = the sum of the weights still in F, r = mulhi64(key(seed, u, D + j), R),
 *   the negative is the item of F, in id order, at which the running sum of F's weights first exceeds r, and that
 *   item leaves F.  Phase 2 continues the same distribution over what is left, so a row is short only when fewer
 *   than nnegs eligible items of positive weight exist.
 *
 * One rule, no sparse / dense switch: with real popularity the head carries half the mass and "every draw is
 * accepted with probability >= 1/2" cannot be promised.  Rows, empty rows, the tie rule, the refusals and the
 * SLIMGPU_SAMPLE_MAX_NCOLS bound of the device call are those of the uniform calls; T = 0 is refused as well.  The
 * uniform calls are unchanged: same symbols, same rows.
 *
 * The weighted device sampler keeps, beside the bitmap and the accepted ids, the prefix table C in HBM (8 bytes per
 * item: 0.8 MB at 100 K items, L2-resident; a device scan of the uploaded weights -- 4 bytes per item host to device
 * per call; for NULL weights the resident matrix's column pointer comes to the host first, 8 bytes per item, and its
 * differences are the weights) and, for phase 2, the remaining mass per block of 1024 items in LDS (4 KB at the
 * item bound): a user that enters phase 2 reads all of C once to form them, and a pick then scans the block sums and
 * one block, not the catalogue again.  Bitmap + ids + block sums
 * are 84 KB at SLIMGPU_SAMPLE_MAX_NCOLS items and nnegs = SLIMGPU_MAX_LIST.  Per draw: one hash, one 64 x 64 multiply
 * and about log2(ncols) dependent reads of C.  Not built: weights for several GPUs, C cached on the handle between
 * calls, the neg-file protocol of slim_predict.
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
 * SLIMGPU_SAMPLE_MAX_NCOLS items; ncols < 1, a user list that does not ascend strictly inside the rows; under the
 * weighted rule weights that sum to 0.
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

#include "slim_gpu_wsample.h"

#endif /* SLIM_AMD_SLIM_GPU_SAMPLE_H_ */
