// gram_pack.hpp -- G = R^T R as byte planes (the form the item-space kernel of cd_gramr.hpp streams).
//
// An update of item-space CD reads one row of G (cd_gram.hpp): 4 ncols bytes as floats.  For a
// binary or small-integer rating matrix every entry of G is a non-negative integer below 2^24
// (a co-rating count, or a sum of products of small integers) and most of them are small:
// G_ij ~ nnz_i nnz_j / nrows, so in a row only the columns of the most popular items reach 256
// (C4: ~10 % of an average row; nothing reaches 65 536 outside the 160 x 160 block of the top
// items).  The packed form stores a row as
//
//     lo [ncols]      bits 0..7 of every entry, columns in POPULARITY order (rank 0 = the item
//                     with the most ratings, ties by id)
//     hi [hi_k 8192]  bits 8..15 of the first hi_k groups of 8192 ranks -- behind the last rank of
//                     the row that needs them the plane simply ends
//     hi2[hi2_k 8192] bits 16..23, likewise
//
// Behind that prefix a 16-rank chunk is stored RELATIVE to a per-chunk base: adjacent ranks are
// about equally popular, so the 16 entries of a chunk spread by a few standard deviations of a
// count around a common level (C4: ~270 +- 50) -- `lo` holds entry - 16 b, `base` the byte b
// (floor(min / 16), at most 255); a chunk whose entries do not fit that (spread above 255, level
// above 4080) extends the prefix.  Decoded as (float)(lo + 16 b + 256 hi + 65536 hi2), exactly.
//
// The DIAGONAL entry G_ii = |a_i|^2 is not a co-rating count of two different items: it sits at
// the row's own rank and is as large as the row's largest entries (the first version kept it in the
// planes, and the hi plane of an item of rank r then reached to r: 54-63 % of a row on C4 instead of
// its popular head).  The planes hold a filler there (the chunk's base level) and the kernel puts
// `diag[i]` in its place when it decodes that chunk.
//
// i.e. ~1.1-1.2 bytes per entry instead of 4, decoded exactly: (float)(lo + 256 hi + 65536 hi2)
// is the float the unpacked G holds, so a kernel that reads the planes performs the very fmaf
// sequence a kernel that reads the floats performs.  A matrix whose G holds anything else
// (fractional or negative ratings) is not packed and stays with the float kernels.
//
// Ranks (not ids) index the planes' columns and the kernel's g vector; rank_of / item_of
// translate.  Groups of 8192 ranks = 512 threads x 16 bytes: the unit in which cd_gramr.hpp's
// workgroup walks a row.
#pragma once
#include <cstdint>

#include "cd_wave.hpp"

namespace slimamd {

constexpr int kGramrNT = 512;     // threads of cd_gramr.hpp's workgroup
constexpr int kPackGroup = 8192;  // ranks per group: 512 threads x one 16-byte load
constexpr int kGramrMaxGroups = 13;  // groups of the largest instantiation, cd_gramr_kernel<10, 3>: 106 496 items
constexpr int kPackJT = 64;  // the streamed pack (gram_pack_scan_t / gram_pack_write_t): items per workgroup,
constexpr int kPackTS = 8;   // and chunk slots per workgroup
constexpr int kGramrCarryMaxGroups = 6;  // instantiations that can carry g from solve to solve (cd_gramr.hpp, g_save / g_load)

struct GramPacked {
  const uint8_t* lo;       // [ncols][ldb]
  int64_t ldb;             // bytes per row of lo: ncols rounded up to 16
  const uint8_t* hi;       // pool of hi planes, row i at hi_off[i], hi_k[i] * 8192 bytes
  const int64_t* hi_off;
  const int32_t* hi_k;
  const int64_t* hi2_off;  // bits 16-23 of the first hi2_k[i] groups: in the same pool, right behind the row's hi
  const int32_t* hi2_k;    // groups (hi2_off[i] = hi_off[i] + hi_k[i] * 8192: the solver needs no second offset)
  const uint8_t* base;     // [ncols][8192]: byte [t * 16 + k] = b of chunk t + 512 k (0 inside the hi prefix)
  const float* diag;       // [ncols]: G_ii, kept out of the planes (see below)
  const uint4* meta;       // [ncols]: what the solver needs of a row in ONE 16-byte record, so that a lane
                           // can load it with its batch header: {rank | hi_k << 17 | hi2_k << 21,
                           // hi_off / 8192, nnz of the column, bits of |a_i|^2 = G_ii}
  const int32_t* rank_of;  // [ncols]
  const int32_t* item_of;  // [nchunks * 16]; -1 behind ncols
  int32_t nchunks;         // 16-rank chunks of a row: ceil(ncols / 16)
};

#ifdef SLIM_GRAM_PACK_KERNELS  // (defined by the one translation unit that owns the two kernels)
// Pass 1, one workgroup per row: how many groups need the hi / hi2 plane (use_base: chunks behind
// the prefix may be stored relative to a base byte), and whether the row can be packed at all
// (flags[0] |= 1 otherwise).
__global__ __launch_bounds__(256) void gram_pack_scan(const float* __restrict__ G, int64_t ld, int ncols,
                                                      const int32_t* __restrict__ item_of, int nchunks,
                                                      int use_base, int32_t* __restrict__ hi_k,
                                                      int32_t* __restrict__ hi2_k, int32_t* __restrict__ flags) {
  const int row = blockIdx.x;
  const float* __restrict__ g = G + (int64_t)row * ld;
  int last1 = -1, last2 = -1;  // last chunk that needs the hi plane, last chunk with an entry >= 65536
  bool bad = false;
  for (int c = threadIdx.x; c < nchunks; c += 256) {
    int mn = 0x7fffffff, mx = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int it = item_of[c * 16 + e];
      if (it >= 0) {
        const float v = g[it];
        const int iv = (int)v;
        if (!(v >= 0.0f && v < 16777216.0f) || (float)iv != v) bad = true;
        if (it != row) {  // (the diagonal is kept apart)
          mn = iv < mn ? iv : mn;
          mx = iv > mx ? iv : mx;
        }
      }
    }
    int b = (use_base && mn != 0x7fffffff) ? (mn >> 4) : 0;
    b = b > 255 ? 255 : b;
    if (mx - 16 * b > 255) last1 = c;
    if (mx >= 65536) last2 = c;
  }
  __shared__ int s1, s2, sb;
  if (threadIdx.x == 0) {
    s1 = -1;
    s2 = -1;
    sb = 0;
  }
  __syncthreads();
  atomicMax(&s1, last1);
  atomicMax(&s2, last2);
  if (bad) atomicOr(&sb, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    constexpr int CG = kPackGroup / 16;  // chunks per group
    hi_k[row] = (s1 + CG) / CG;          // ceil((s1 + 1) / 512); 0 when s1 == -1
    hi2_k[row] = (s2 + CG) / CG;
    if (sb) atomicOr(flags, 1);
  }
}

// Pass 2, one workgroup per row: write the planes (16 ranks per thread and step).
__global__ __launch_bounds__(256) void gram_pack_write(const float* __restrict__ G, int64_t ld, int ncols,
                                                       const int32_t* __restrict__ item_of, int nchunks,
                                                       uint8_t* __restrict__ lo, int64_t ldb,
                                                       uint8_t* __restrict__ hi, const int64_t* __restrict__ hi_off,
                                                       const int32_t* __restrict__ hi_k,
                                                       uint8_t* __restrict__ hi2, const int64_t* __restrict__ hi2_off,
                                                       const int32_t* __restrict__ hi2_k,
                                                       uint8_t* __restrict__ base, float* __restrict__ diag) {
  const int row = blockIdx.x;
  const float* __restrict__ g = G + (int64_t)row * ld;
  const int n1 = hi_k[row] * (kPackGroup / 16), n2 = hi2_k[row] * (kPackGroup / 16);
  uint8_t* __restrict__ plo = lo + (int64_t)row * ldb;
  uint8_t* __restrict__ phi = hi + hi_off[row];
  uint8_t* __restrict__ ph2 = hi2 + hi2_off[row];
  uint8_t* __restrict__ pb = base + (int64_t)row * kPackGroup;
  const int nmax = max(nchunks, max(n1, n2));
  for (int c = threadIdx.x; c < nmax; c += 256) {
    uint32_t w0[4] = {0, 0, 0, 0}, w1[4] = {0, 0, 0, 0}, w2[4] = {0, 0, 0, 0};
    if (c < nchunks) {
      uint32_t iv[16];
      uint32_t mn = 0xffffffffu;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int it = item_of[c * 16 + e];
        iv[e] = it >= 0 ? (uint32_t)(int)g[it] : 0u;
        if (it == row) diag[row] = g[it];
        if (it >= 0 && it != row) mn = iv[e] < mn ? iv[e] : mn;
      }
      uint32_t b = 0;
      if (c >= n1) {  // behind the prefix: relative to the chunk's base (pass 1 made sure it fits)
        b = mn == 0xffffffffu ? 0u : (mn >> 4);
        b = b > 255u ? 255u : b;
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int it = item_of[c * 16 + e];
        const uint32_t v = (it >= 0 && it != row) ? iv[e] - 16u * b : 0u;  // (diagonal: a filler)
        w0[e >> 2] |= (v & 255u) << (8 * (e & 3));
        w1[e >> 2] |= ((v >> 8) & 255u) << (8 * (e & 3));
        w2[e >> 2] |= ((v >> 16) & 255u) << (8 * (e & 3));
      }
      *reinterpret_cast<uint4*>(plo + 16 * (int64_t)c) = make_uint4(w0[0], w0[1], w0[2], w0[3]);
      pb[(c & (kGramrNT - 1)) * 16 + (c / kGramrNT)] = (uint8_t)b;
    }
    if (c < n1) *reinterpret_cast<uint4*>(phi + 16 * (int64_t)c) = make_uint4(w1[0], w1[1], w1[2], w1[3]);
    if (c < n2) *reinterpret_cast<uint4*>(ph2 + 16 * (int64_t)c) = make_uint4(w2[0], w2[1], w2[2], w2[3]);
  }
}

// ---- the same two passes by streaming transposed tiles (the default; the two kernels above stay
// reachable with SLIM_GPU_PACK_GATHER=1) ------------------------------------------------------------
// The planes exist only for an integer-valued G below 2^24, whose sums are exact in any order: such a
// G is exactly symmetric, and entry (row j, rank r) of the planes, G[j][item_of[r]], is
// G[item_of[r]][j].  Read along that form a 16-rank chunk is 16 ROWS of G, each read contiguously
// along j, instead of 16 four-byte gathers per row: the permutation becomes a choice of rows.
//
// A workgroup of 256 threads owns 8 consecutive chunk slots t0 .. t0 + 7 (a slot t of 0..511 holds the
// chunks t + 512 k of every group k) and kPackJT = 64 consecutive items j.  Per group it loads the
// tile of the 128 rows item_of[16 (t + 512 k) + e] by the 64 floats [j0, j0 + 64) into LDS -- one
// wavefront load per 256-byte row segment; G_ld is a multiple of 64 floats, so a segment is aligned
// and inside its row for every j0 --, and thread (j, t) reads its 16 values down the rank dimension.
// Lanes are laid out t fastest, so that the eight 16-byte stores of one row j are one 128-byte run.
// A thread serves two items, j and j + 32.
constexpr int kPackTileRows = 16 * kPackTS;          // 128 rows of G per tile
// row r of the tile at r * 64 + (r / 16) * 4: the 4 floats between chunks put the 32 lanes of an
// LDS read (8 slots x 4 items) on 32 different banks; a row's 64 floats are conflict-free as they are
constexpr int kPackTileFloats = kPackTileRows * kPackJT + 4 * kPackTS;
static_assert(kGramrNT % kPackTS == 0 && kGramrMaxGroups <= 16, "slots per workgroup; base bytes of a 16-byte record");

__device__ __forceinline__ int pack_tile_at(int slot, int e, int jl) { return (slot * 16 + e) * kPackJT + slot * 4 + jl; }

// rows item_of[16 c + e], c = c0 .. c0 + 7, columns [j0, j0 + 64) of G -> tile; zeros behind nchunks / ncols
__device__ __forceinline__ void pack_tile_load(const float* __restrict__ G, int64_t ld,
                                               const int32_t* __restrict__ item_of, int nchunks, int c0, int j0,
                                               float* __restrict__ tile) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#pragma unroll
  for (int h = 0; h < 2; ++h) {  // a wavefront loads 2 slots: 16 row segments in flight each
    const int slot = 2 * w + h;
    const int c = c0 + slot;
    int it[16];
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) it[e] = item_of[(c < nchunks ? c : 0) * 16 + e];  // (one 64-byte scalar load)
#pragma unroll
    for (int e = 0; e < 16; ++e) it[e] = c < nchunks ? it[e] : -1;
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = G[(int64_t)(it[e] >= 0 ? it[e] : 0) * ld + j0 + lane];  // (no branch: row 0 is there)
#pragma unroll
    for (int e = 0; e < 16; ++e) tile[pack_tile_at(slot, e, lane)] = it[e] >= 0 ? v[e] : 0.0f;
  }
}

// Pass 1: last1[j] / last2[j] (both -1 before the launch) = the last chunk of row j that needs the hi
// plane / holds an entry >= 65536, by the very tests of gram_pack_scan; flags[0] |= 1 unless every
// entry of G is an integer in [0, 2^24).  grid (512 / 8, ceil(ncols / 64)).
__global__ __launch_bounds__(256) void gram_pack_scan_t(const float* __restrict__ G, int64_t ld, int ncols,
                                                        const int32_t* __restrict__ item_of,
                                                        const int32_t* __restrict__ rank_of, int nchunks,
                                                        int use_base, int32_t* __restrict__ last1,
                                                        int32_t* __restrict__ last2, int32_t* __restrict__ flags) {
  __shared__ float tile[kPackTileFloats];
  const int t0 = blockIdx.x * kPackTS, j0 = blockIdx.y * kPackJT;
  const int tl = threadIdx.x & (kPackTS - 1), jl = (int)threadIdx.x >> 3;
  const int ngroups = (nchunks + kGramrNT - 1) / kGramrNT;
  int rj[2], l1[2] = {-1, -1}, l2[2] = {-1, -1};
#pragma unroll
  for (int p = 0; p < 2; ++p) rj[p] = j0 + jl + 32 * p < ncols ? rank_of[j0 + jl + 32 * p] : -1;
  bool bad = false;
  for (int k = 0; k < ngroups; ++k) {
    pack_tile_load(G, ld, item_of, nchunks, t0 + kGramrNT * k, j0, tile);
    __syncthreads();
    const int c = t0 + tl + kGramrNT * k;
    if (c < nchunks) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        if (rj[p] < 0) continue;  // (an item behind ncols)
        int mn = 0x7fffffff, mx = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          if (c * 16 + e < ncols) {
            const float v = tile[pack_tile_at(tl, e, jl + 32 * p)];
            const int iv = (int)v;
            if (!(v >= 0.0f && v < 16777216.0f) || (float)iv != v) bad = true;
            if (c * 16 + e != rj[p]) {  // (the diagonal is kept apart)
              mn = iv < mn ? iv : mn;
              mx = iv > mx ? iv : mx;
            }
          }
        }
        int b = (use_base && mn != 0x7fffffff) ? (mn >> 4) : 0;
        b = b > 255 ? 255 : b;
        if (mx - 16 * b > 255) l1[p] = c;
        if (mx >= 65536) l2[p] = c;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    if (l1[p] >= 0) atomicMax(&last1[j0 + jl + 32 * p], l1[p]);  // (l >= 0 only for an item inside ncols)
    if (l2[p] >= 0) atomicMax(&last2[j0 + jl + 32 * p], l2[p]);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, 1);
}

// last chunk -> groups of the plane, in place: ceil((last + 1) / 512), 0 for -1 (gram_pack_scan's rounding)
__global__ void gram_pack_groups(int ncols, int32_t* __restrict__ hi_k, int32_t* __restrict__ hi2_k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int CG = kPackGroup / 16;
  if (i < ncols) {
    hi_k[i] = (hi_k[i] + CG) / CG;
    hi2_k[i] = (hi2_k[i] + CG) / CG;
  }
}

// Pass 2, the same walk: byte for byte the planes of gram_pack_write.  A thread keeps the 16 base
// bytes of its (item, slot) in registers and stores the record once; every store is 16 bytes.  Every
// record of base is written (zeros inside the prefix and behind nchunks): no memset before.
__global__ __launch_bounds__(256) void gram_pack_write_t(const float* __restrict__ G, int64_t ld, int ncols,
                                                         const int32_t* __restrict__ item_of,
                                                         const int32_t* __restrict__ rank_of, int nchunks,
                                                         uint8_t* __restrict__ lo, int64_t ldb,
                                                         uint8_t* __restrict__ hi, const int64_t* __restrict__ hi_off,
                                                         const int32_t* __restrict__ hi_k,
                                                         uint8_t* __restrict__ hi2, const int64_t* __restrict__ hi2_off,
                                                         const int32_t* __restrict__ hi2_k,
                                                         uint8_t* __restrict__ base, float* __restrict__ diag) {
  __shared__ float tile[kPackTileFloats];
  const int t0 = blockIdx.x * kPackTS, j0 = blockIdx.y * kPackJT;
  const int tl = threadIdx.x & (kPackTS - 1), jl = (int)threadIdx.x >> 3;
  const int ngroups = (nchunks + kGramrNT - 1) / kGramrNT;
  int rj[2], n1[2], n2[2];
  uint8_t *plo[2], *phi[2], *ph2[2];
  uint64_t rec[2][2] = {{0, 0}, {0, 0}};  // the base bytes of groups 0..7 and 8..15
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int j = j0 + jl + 32 * p;
    const bool in = j < ncols;
    rj[p] = in ? rank_of[j] : -1;
    n1[p] = in ? hi_k[j] * (kPackGroup / 16) : 0;
    n2[p] = in ? hi2_k[j] * (kPackGroup / 16) : 0;
    plo[p] = lo + (int64_t)j * ldb;
    phi[p] = hi + (in ? hi_off[j] : 0);
    ph2[p] = hi2 + (in ? hi2_off[j] : 0);
  }
  for (int k = 0; k < ngroups; ++k) {
    pack_tile_load(G, ld, item_of, nchunks, t0 + kGramrNT * k, j0, tile);
    __syncthreads();
    const int c = t0 + tl + kGramrNT * k;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (rj[p] < 0) continue;  // (an item behind ncols)
      uint32_t w0[4] = {0, 0, 0, 0}, w1[4] = {0, 0, 0, 0}, w2[4] = {0, 0, 0, 0};
      if (c < nchunks) {
        uint32_t iv[16];
        uint32_t mn = 0xffffffffu;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float v = tile[pack_tile_at(tl, e, jl + 32 * p)];
          const bool in = c * 16 + e < ncols;
          iv[e] = in ? (uint32_t)(int)v : 0u;
          if (in && c * 16 + e != rj[p]) mn = iv[e] < mn ? iv[e] : mn;
        }
        if (c == (rj[p] >> 4)) diag[j0 + jl + 32 * p] = tile[pack_tile_at(tl, rj[p] & 15, jl + 32 * p)];
        uint32_t b = 0;
        if (c >= n1[p]) {  // behind the prefix: relative to the chunk's base (pass 1 made sure it fits)
          b = mn == 0xffffffffu ? 0u : (mn >> 4);
          b = b > 255u ? 255u : b;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const uint32_t v = (c * 16 + e < ncols && c * 16 + e != rj[p]) ? iv[e] - 16u * b : 0u;  // (diagonal: a filler)
          w0[e >> 2] |= (v & 255u) << (8 * (e & 3));
          w1[e >> 2] |= ((v >> 8) & 255u) << (8 * (e & 3));
          w2[e >> 2] |= ((v >> 16) & 255u) << (8 * (e & 3));
        }
        *reinterpret_cast<uint4*>(plo[p] + 16 * (int64_t)c) = make_uint4(w0[0], w0[1], w0[2], w0[3]);
        if (k < 8) rec[p][0] |= (uint64_t)b << (8 * k);
        else rec[p][1] |= (uint64_t)b << (8 * (k - 8));
      }
      if (c < n1[p]) *reinterpret_cast<uint4*>(phi[p] + 16 * (int64_t)c) = make_uint4(w1[0], w1[1], w1[2], w1[3]);
      if (c < n2[p]) *reinterpret_cast<uint4*>(ph2[p] + 16 * (int64_t)c) = make_uint4(w2[0], w2[1], w2[2], w2[3]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 2; ++p)
    if (rj[p] >= 0)  // byte [t * 16 + k] = b of chunk t + 512 k
      *reinterpret_cast<uint4*>(base + (int64_t)(j0 + jl + 32 * p) * kPackGroup + 16 * (t0 + tl)) =
          make_uint4((uint32_t)rec[p][0], (uint32_t)(rec[p][0] >> 32), (uint32_t)rec[p][1], (uint32_t)(rec[p][1] >> 32));
}

// the row records (after pass 2).  The solver takes |a_i|^2 and its root from the record instead
// of csq / cnorm: flags[0] |= 2 (and the planes are not used) unless G_ii == csq[i] and
// sqrtf(csq[i]) == cnorm[i] bit for bit -- true for the integer-valued matrices that can be packed.
__global__ void gram_pack_meta(int ncols, const int32_t* __restrict__ rank_of, const int32_t* __restrict__ hi_k,
                               const int32_t* __restrict__ hi2_k, const int64_t* __restrict__ hi_off,
                               const float* __restrict__ diag, const int64_t* __restrict__ colptr,
                               const float* __restrict__ csq, const float* __restrict__ cnorm,
                               uint4* __restrict__ meta, int32_t* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncols) {
    if (diag[i] != csq[i] || sqrtf(csq[i]) != cnorm[i]) atomicOr(flags, 2);
    meta[i] = make_uint4((uint32_t)rank_of[i] | ((uint32_t)hi_k[i] << 17) | ((uint32_t)hi2_k[i] << 21),
                         (uint32_t)(hi_off[i] / kPackGroup), (uint32_t)(colptr[i + 1] - colptr[i]),
                         __float_as_uint(csq[i]));
  }
}

#endif  // SLIM_GRAM_PACK_KERNELS

// the 16 floats of one chunk: lo + 256 hi + 65536 hi2, exact (integers below 2^24)
__device__ __forceinline__ void unpack16(const uint4 l, float (&f)[16]) {
  const uint32_t w[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[4 * j + 0] = (float)(w[j] & 255u);
    f[4 * j + 1] = (float)((w[j] >> 8) & 255u);
    f[4 * j + 2] = (float)((w[j] >> 16) & 255u);
    f[4 * j + 3] = (float)(w[j] >> 24);
  }
}
__device__ __forceinline__ void unpack16_add(const uint4 h, const float scale, float (&f)[16]) {
  const uint32_t w[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[4 * j + 0] = fmaf(scale, (float)(w[j] & 255u), f[4 * j + 0]);
    f[4 * j + 1] = fmaf(scale, (float)((w[j] >> 8) & 255u), f[4 * j + 1]);
    f[4 * j + 2] = fmaf(scale, (float)((w[j] >> 16) & 255u), f[4 * j + 2]);
    f[4 * j + 3] = fmaf(scale, (float)(w[j] >> 24), f[4 * j + 3]);
  }
}

}  // namespace slimamd
