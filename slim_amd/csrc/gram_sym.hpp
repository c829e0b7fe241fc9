// gram_sym.hpp -- the mirror half of G = R^T R in one streaming pass.
//
// The G builder (cd_tile.hpp, S.gram_mode 3) forms every sum once: the tile at position t of the work
// list writes the entries of its P rows whose column belongs to a tile at or behind t.  The other half
// used to leave the tile kernel with them, one 4-byte store per entry into a row of its own: 5e9
// scattered stores on 100K items.  Here it is filled after the build's last launch instead.
//
// A workgroup takes the pair of 64 x 64 blocks (I, J) and (J, I), I <= J, of G in id order, loads
// both into LDS -- 64 row segments of 256 bytes each (G_ld is a multiple of 64 floats, so a segment
// is aligned and inside its row) -- and writes both back.  Entry (a, b) keeps its own value when the
// tile of row a is not behind the tile of row b, pos[a] / P <= pos[b] / P, and takes G[b][a] from the
// other block otherwise.  The rule is by position, not by value: sums of negative ratings may be
// negative or cancel, and what the losing side held before (zeros of the memset, the entries of a
// launch that was abandoned) is never looked at.  Entries inside one tile, the diagonal among them,
// were written from both sides and keep their values; so do the pad columns [ncols, G_ld).
// The transposed read walks a column of a tile whose rows are 65 floats apart: no bank conflicts.
#pragma once
#include <cstdint>

namespace slimamd {

constexpr int kSymB = 64;    // block edge
constexpr int kSymNT = 256;  // threads: a wavefront moves 16 row segments of each block

// (G, G_ld, ncols, pos = position of every column in the build's work list, log2 of the tile width P);
// grid (nb, nb) with nb = ceil(ncols / 64): the workgroups below the diagonal return at once
using GramSymFn = void (*)(float*, int64_t, int, const int32_t*, int);
GramSymFn gram_sym_fn();

}  // namespace slimamd

#ifdef SLIM_GRAM_SYM_KERNEL
#include <hip/hip_runtime.h>

namespace slimamd {

__global__ __launch_bounds__(kSymNT) void gram_sym_kernel(float* __restrict__ G, const int64_t ld, const int ncols,
                                                          const int32_t* __restrict__ pos, const int logp) {
  const int I = blockIdx.y, J = blockIdx.x;
  if (J < I) return;
  constexpr int B = kSymB, NWV = kSymNT / 64;
  __shared__ float sa[B][B + 1], sb[B][B + 1];
  __shared__ int ta[B], tb[B];  // tile of every row of block (I, J) / of block (J, I); rows behind ncols: none
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i0 = I * B, j0 = J * B;
  const bool diag = I == J;
  if (tid < B) ta[tid] = i0 + tid < ncols ? pos[i0 + tid] >> logp : 0x7fffffff;
  else if (tid < 2 * B) tb[tid - B] = j0 + tid - B < ncols ? pos[j0 + tid - B] >> logp : 0x7fffffff;
#pragma unroll
  for (int r = w; r < B; r += NWV) {
    sa[r][lane] = i0 + r < ncols ? G[(int64_t)(i0 + r) * ld + j0 + lane] : 0.0f;
    if (!diag) sb[r][lane] = j0 + r < ncols ? G[(int64_t)(j0 + r) * ld + i0 + lane] : 0.0f;
  }
  __syncthreads();
  // block (I, J): row a = i0 + r, column b = j0 + lane.  (A column behind ncols has no row to take a
  // value from: its tile is "none", behind every tile.)
  const int tcol = tb[lane];
#pragma unroll
  for (int r = w; r < B; r += NWV) {
    const float own = sa[r][lane], other = diag ? sa[lane][r] : sb[lane][r];
    if (i0 + r < ncols) G[(int64_t)(i0 + r) * ld + j0 + lane] = ta[r] <= tcol ? own : other;
  }
  if (diag) return;
  // block (J, I): row b = j0 + r, column a = i0 + lane
  const int tcol2 = ta[lane];
#pragma unroll
  for (int r = w; r < B; r += NWV) {
    const float own = sb[r][lane], other = sa[lane][r];
    if (j0 + r < ncols) G[(int64_t)(j0 + r) * ld + i0 + lane] = tb[r] <= tcol2 ? own : other;
  }
}

}  // namespace slimamd
#endif
