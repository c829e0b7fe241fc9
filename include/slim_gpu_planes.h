/*
 * slim_gpu_planes.h -- a look at the byte planes of G = R^T R (pulled in by slim_gpu.h; a header
 * of its own like slim_gpu_eval.h, so that slim_gpu.h keeps the set of entry points it had).
 *
 * Item-space CD streams G as byte planes in popularity order whenever G is integer-valued below
 * 2^24 (slimgpu_kernel_et, SLIMGPU_KERNEL_GRAM; SLIMGPU_MatrixGramCommit forms them).  Entry
 * (row i, rank r), r != rank_of[i], decodes as
 *     lo[i * ldb + r] + 16 * base[i * 8192 + (c % 512) * 16 + c / 512]
 *       + 256 * hi[hi_off[i] + r]                          where r < hi_k[i] * 8192
 *       + 65536 * hi[hi_off[i] + hi_k[i] * 8192 + r]       where r < hi2_k[i] * 8192
 * with c = r / 16; rank 0 is the item with the most ratings, ties by id.  The planes hold a filler
 * at the row's own rank: G_ii is diag[i].  Tests hold the planes against R^T R with this.
 */
#ifndef SLIM_AMD_SLIM_GPU_PLANES_H_
#define SLIM_AMD_SLIM_GPU_PLANES_H_

#include "slim.h"

#ifdef __cplusplus
extern "C" {
#endif

struct slimgpu_matrix;

/* Device pointers (the handle's own buffers: valid until the next build or commit of G, or the
 * handle's end) and sizes. */
typedef struct slimgpu_gram_planes_t {
  int32_t ncols;
  int32_t nchunks;        /* 16-rank chunks of a row: ceil(ncols / 16)                           */
  int64_t ldb;            /* bytes per row of lo: 16 nchunks                                     */
  int64_t hi_bytes;       /* length of the pool, the group of slack behind the last row included */
  const uint8_t *lo;      /* [ncols][ldb]                                                        */
  const uint8_t *base;    /* [ncols][8192]                                                       */
  const uint8_t *hi;      /* [hi_bytes]: row i's hi groups, then its hi2 groups, at hi_off[i]    */
  const int64_t *hi_off;  /* [ncols]                                                             */
  const int32_t *hi_k;    /* [ncols] groups of 8192 ranks in the row's hi plane                  */
  const int32_t *hi2_k;   /* [ncols] ... in its hi2 plane                                        */
  const float *diag;      /* [ncols]                                                             */
  const uint32_t *meta;   /* [ncols][4]: {rank | hi_k << 17 | hi2_k << 21, hi_off / 8192, nnz of
                             the column, bits of G_ii}                                           */
  const int32_t *rank_of; /* [ncols]                                                             */
  const int32_t *item_of; /* [16 nchunks], -1 behind ncols                                       */
} slimgpu_gram_planes_t;

/* SLIM_OK, or SLIM_ERROR_INPUT when the handle holds no planes (no G yet, a G that is not
 * integer-valued in [0, 2^24), more items than the planes' layout holds). */
int32_t SLIMGPU_MatrixGramPlanes(struct slimgpu_matrix *mat, slimgpu_gram_planes_t *out);

#ifdef __cplusplus
}
#endif

#endif /* SLIM_AMD_SLIM_GPU_PLANES_H_ */
