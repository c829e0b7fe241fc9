// topn_kernels.hpp -- the device code of the top-N scorers; topn.hip instantiates and
// launches it, scorer.hpp is the host side's interface.  Everything here has internal linkage (an unnamed
// namespace): the header is for topn.hip alone, a second includer would compile every kernel again.
//
// What it computes is GetRecommendations of the reference (src/libslim/predict.c:15-71) applied to
// every row of a history matrix (Py_SLIM_Predict, src/libslim/pyapi.c:530-563): the score of candidate k is the sum
// over the user's history items i of rating_i * W[i,k] (row i of the model), items of the history are excluded, the N
// best candidates are returned in descending score order.
//
// One wavefront per user, results BIT-IDENTICAL to the library's host path (host_csr.cpp::top_n):
//   * history rows are walked in order and the nnz of a row go to different lanes (ids in a row are distinct), so
//     every candidate receives its float additions in exactly the host's order; products and sums are rounded
//     separately (no FMA contraction);
//   * ties are broken by discovery order like the host (the reference's gk_fkvsortd leaves tie order undefined): the
//     first touch of a candidate records (history index, position in the W row), which sorts like the host's
//     discovery counter;
//   * selection: one pass over the score vector with a per-lane sorted list of the N best (LDS), then N rounds of a
//     wave-wide arg-max over the 64 list heads.
// The score/discovery vectors (12 bytes per item) live in a per-wavefront HBM slab.  A second kernel
// (topn_chunk_kernel, below) keeps them in LDS and serves lists of up to 64 from models with sorted rows; its
// long-list form (topn_chunk_long_kernel) selects by threshold and serves lists of up to SLIMGPU_MAX_LIST.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "engine.hpp"
#include "eval_terms.hpp"

namespace slimamd {
namespace {
constexpr unsigned long long kUntouched = ~0ull;
constexpr unsigned long long kExcluded = ~0ull - 1ull;

// A candidate filter (slim_gpu_filter.h) as the kernels read it; inert when its pointers are null.  bits: one bit per
// item, set = may be recommended (nullptr: every item may).  xptr / xind: the exclusion rows, a CSR over USER ids
// with xusers rows (nullptr: none; a user >= xusers has none).
struct FilterArgs {
  const uint32_t* bits = nullptr;
  const int64_t* xptr = nullptr; const int32_t* xind = nullptr;
  int32_t xusers = 0;
};
__device__ __forceinline__ bool filter_allows(const uint32_t* __restrict__ bits, const int id) {
  return (bits[id >> 5] >> (id & 31)) & 1u;
}

struct TopNArgs {
  int32_t nusers, nitems_rows, ncols, nrcmds;  // nusers: positions
  const int32_t* users = nullptr;  // the user of every position; nullptr: position q is user q
  FilterArgs flt;
  const int64_t* wptr; const int32_t* wind; const float* wval;
  const int64_t* hptr; const int32_t* hind;
  const float* hval;  // nullptr: implicit ratings of 1
  float* score;                // [nwaves][ncols]
  unsigned long long* disc;    // [nwaves][ncols]
  int32_t* out_ids; float* out_scores; int32_t* out_cnt;
  int32_t* queue;
};

// a candidate is "better" when its score is higher, or equal with an earlier discovery (KeyT: the discovery key)
template <typename KeyT>
__device__ __forceinline__ bool better(float sa, KeyT da, float sb, KeyT db) {
  return sa > sb || (sa == sb && da < db);
}

__device__ __forceinline__ int64_t uni64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
// the exclusion row of user u (wave-uniform): [x0, x1) in xind, empty without a filter
__device__ __forceinline__ void exclusion_row(const FilterArgs& F, const int u, int64_t& x0, int64_t& x1) {
  x0 = x1 = 0;
  if (F.xptr != nullptr && u < F.xusers) x0 = uni64(F.xptr[u]), x1 = uni64(F.xptr[u + 1]);
}

// Control flow is wave-uniform wherever the data allows it: positions are strided statically
// over the wavefronts (outputs are indexed by the position, history by its user), loop bounds over history rows and output ranks are scalars, and the
// only divergent loops are the lane-strided walks and the per-lane list insertion.
__global__ __launch_bounds__(64) void topn_kernel(const TopNArgs T) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x;
  const int N = T.nrcmds;
  // per-lane sorted lists, lane-major so a lane's slots sit in different banks
  float* l_score = reinterpret_cast<float*>(smem);                                       // [N][64]
  unsigned long long* l_disc = reinterpret_cast<unsigned long long*>(l_score + N * 64);  // [N][64]
  int* l_id = reinterpret_cast<int*>(l_disc + N * 64);                                   // [N][64]

  float* score = T.score + (int64_t)blockIdx.x * T.ncols;
  unsigned long long* disc = T.disc + (int64_t)blockIdx.x * T.ncols;

  for (int q = (int)blockIdx.x; q < T.nusers; q += (int)gridDim.x) {
    const int u = T.users ? __builtin_amdgcn_readfirstlane(T.users[q]) : q;
    const int64_t h0 = uni64(T.hptr[u]), h1 = uni64(T.hptr[u + 1]);
    int64_t x0, x1;
    exclusion_row(T.flt, u, x0, x1);

    // an item the filter does not allow is excluded before anything touches it
    if (T.flt.bits == nullptr)
      for (int k = lane; k < T.ncols; k += 64) disc[k] = kUntouched;
    else
      for (int k = lane; k < T.ncols; k += 64) disc[k] = filter_allows(T.flt.bits, k) ? kUntouched : kExcluded;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    // history items are never recommended (predict.c:35-38), nor is the user's exclusion row
    for (int64_t h = h0 + lane; h < h1; h += 64) {
      const int i = T.hind[h];
      if (i >= 0 && i < T.ncols) disc[i] = kExcluded;
    }
    for (int64_t x = x0 + lane; x < x1; x += 64) {
      const int i = T.flt.xind[x];
      if (i >= 0 && i < T.ncols) disc[i] = kExcluded;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");

    // accumulate, history order outside, W-row entries across lanes (predict.c:40-58)
    for (int64_t h = h0; h < h1; ++h) {
      const int i = __builtin_amdgcn_readfirstlane(T.hind[h]);
      if (i >= 0 && i < T.nitems_rows) {
        const float rating = T.hval ? T.hval[h] : 1.0f;
        const int64_t w0 = uni64(T.wptr[i]), w1 = uni64(T.wptr[i + 1]);
        for (int64_t j = w0 + lane; j < w1; j += 64) {
          const int k = T.wind[j];
          const unsigned long long d = disc[k];
          if (d != kExcluded) {
            // the host scorer rounds the product and the sum separately: no FMA here
#pragma clang fp contract(off)
            float acc = 0.0f;
            if (d == kUntouched)
              disc[k] = ((unsigned long long)(h - h0) << 32) | (unsigned long long)(j - w0);
            else
              acc = score[k];
            const float prod = rating * T.wval[j];
            score[k] = acc + prod;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      }
    }

    // per-lane N best of the lane's stride of the score vector
    int cnt = 0;  // entries in this lane's list
    for (int k = lane; k < T.ncols; k += 64) {
      const unsigned long long d = disc[k];
      const float sc = score[k];
      bool want = d < kExcluded;
      if (want && cnt == N)
        want = better(sc, d, l_score[(N - 1) * 64 + lane], l_disc[(N - 1) * 64 + lane]);
      if (want) {
        int pos = cnt < N ? cnt : N - 1;  // insertion from the tail
        while (pos > 0 &&
               better(sc, d, l_score[(pos - 1) * 64 + lane], l_disc[(pos - 1) * 64 + lane])) {
          l_score[pos * 64 + lane] = l_score[(pos - 1) * 64 + lane];
          l_disc[pos * 64 + lane] = l_disc[(pos - 1) * 64 + lane];
          l_id[pos * 64 + lane] = l_id[(pos - 1) * 64 + lane];
          --pos;
        }
        l_score[pos * 64 + lane] = sc;
        l_disc[pos * 64 + lane] = d;
        l_id[pos * 64 + lane] = k;
        if (cnt < N) ++cnt;
      }
    }

    // N rounds: the best of the 64 list heads wins and is popped
    int head = 0, nout = 0;
    for (int r = 0; r < N; ++r) {
      const bool has = head < cnt;
      float bs = has ? l_score[head * 64 + lane] : 0.0f;
      unsigned long long bd = has ? l_disc[head * 64 + lane] : kUntouched;  // empty sorts last
      const int my_id = has ? l_id[head * 64 + lane] : 0;
      int bl = lane;
      int bh = has ? 1 : 0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float os = __shfl_xor(bs, off);
        const unsigned int od_lo = __shfl_xor((unsigned int)bd, off);
        const unsigned int od_hi = __shfl_xor((unsigned int)(bd >> 32), off);
        const unsigned long long od = ((unsigned long long)od_hi << 32) | od_lo;
        const int ol = __shfl_xor(bl, off);
        const int oh = __shfl_xor(bh, off);
        const bool take = oh != 0 && (bh == 0 || better(os, od, bs, bd));
        bs = take ? os : bs;
        bd = take ? od : bd;
        bl = take ? ol : bl;
        bh = take ? oh : bh;
      }
      const int winner = __builtin_amdgcn_readfirstlane(bl);
      const int any = __builtin_amdgcn_readfirstlane(bh);
      const int id = __shfl(my_id, winner);
      if (any) {
        if (lane == 0) {
          T.out_ids[(int64_t)q * N + r] = id;
          T.out_scores[(int64_t)q * N + r] = bs;
        }
        if (lane == winner) ++head;
        ++nout;
      }
    }
    if (lane == 0) T.out_cnt[q] = nout;
  }
}

// ---- second kernel: score chunks in LDS -------------------------------------------------
//
// topn_kernel keeps the 12-byte-per-item score/discovery vectors of a user in HBM, so every multiply-add costs ~4
// random sector requests: measured on a C4-shaped model (100K items, 2700 entries per row, histories of ~890 items)
// it is bound by the request rate at 14e9 adds/s = 5.8K users/s -- slower than the host scorer on a 128-core box.
//
// Here a workgroup of 8 wavefronts serves one user and the ITEMS are cut into chunks of CW ids whose score/discovery
// arrays live in LDS (12 bytes x CW per wavefront). Wavefront w owns chunks w, w+8, ...; for each of its chunks it
// walks the user's history in order and, for history item i, only the entries of row i of W whose ids fall into the
// chunk -- rows are sorted, and wsplit[i][c] (built once per call) is where chunk c starts in row i. Every candidate
// still receives its additions in history order, products and sums rounded separately, and the first touch still
// records (history index, position in the row), so the result is bit-identical to topn_kernel and to the host. HBM
// sees each W entry once per user, in coalesced segments; everything else is LDS.
//   * the (start, length, rating) of up to 64 history items are fetched lane-parallel, then consumed one item at a
//     time through v_readlane; the segment loads run kT2Depth items ahead of the LDS updates;
//   * selection: a wavefront keeps its N best in REGISTERS (lane t = rank t); a candidate that beats the current N-th
//     is inserted with one ballot + one lane shift; the 8 lists are merged through LDS by wavefront 0.
constexpr int kT2Waves = 8;       // default workgroup: 8 wavefronts x 1536-id chunks
constexpr int kT2Depth = 16;
constexpr int kT2MaxN = 64;       // lists live one rank per lane: up to a wavefront's width
constexpr int kT2MaxCW = 1536;

// What every chunk kernel reads: the model and its split table, the histories, the work queue.  Each form of
// the kernel takes this plus its own fields.
struct ChunkArgs {
  int32_t nusers, nitems_rows, ncols, nrcmds;  // nusers: positions pulled from the queue
  const int32_t* users = nullptr;  // the user of every position; nullptr: position q is user q
  int32_t cw, nchunks;
  uint32_t wlast;    // nnz(W) - 1 (0 for an empty model): clamp for the unconditional loads
  int32_t pos_bits;  // discovery key = history index << pos_bits | position in the row
  const int64_t* wptr; const int32_t* wind; const float* wval;
  const uint32_t* wsplit;  // [nitems_rows][nchunks + 1]: offset in row i of the first id >= c * cw
  const int64_t* hptr; const int32_t* hind; const float* hval;
  int32_t* queue;
  FilterArgs flt;  // every mode takes one: lists, the fused evaluation, ranks (with k_test_keys), long lists
};
struct TopN2Args : ChunkArgs {  // lists of up to 64 (topn_chunk_kernel)
  int32_t* out_ids = nullptr; float* out_scores = nullptr; int32_t* out_cnt = nullptr;
};
// lists + the fused evaluation (topn_chunk_eval_kernel): the test rows, the head / tail marker, one record per
// cutoff and position (terms[k * nusers + q]); cut.c[cut.n - 1] == nrcmds.  Lists are written only when an
// output pointer is given.
struct TopNEvalArgs : TopN2Args {
  const int64_t* tptr = nullptr; const int32_t* tind = nullptr; const int32_t* fmarker = nullptr;
  int32_t fm_ncols = 0;
  UserTerms* terms = nullptr;
  Cutoffs cut = {};
};
// rank mode (slim_gpu_rank.h, topn_chunk_rank_kernel): the scorer counts, for every test entry of the user, the
// candidates that stand before it.  (score, key) of the test entries come from k_test_keys, which ran before
// the scorer.
constexpr unsigned long long kNoCandidate = ~0ull;  // key of a test entry that is no candidate (every KeyT's kUnt)
struct TopNRankArgs : ChunkArgs {
  const int64_t* tptr = nullptr;   // the test rows' pointer: how many entries a user has
  const int64_t* tbase = nullptr;  // [nusers + 1]: where a position's test entries start in the arrays below
  const unsigned long long* tkey = nullptr;  // discovery key of every test entry, kNoCandidate: not a candidate
  const float* tscore = nullptr;
  int32_t* rank = nullptr;    // out: 1 + candidates ahead, 0: not a candidate
  float* rscore = nullptr;    // out: the entry's score, 0 when it is no candidate
  int32_t g0 = 0, gsize = 0;  // this pass serves entries [g0, g0 + gsize) of every test row
};
// long lists (slim_gpu_lists.h, topn_chunk_long_kernel): the candidates of a user go to the workgroup's slab, a
// histogram over the leading bits of their order finds the N-th, the winners are put in order in LDS.
constexpr int kLongMaxN = SLIMGPU_MAX_LIST;
constexpr int kLongBins = 2048;      // 11 bits per selection pass
constexpr int kLongSortCap = 2048;   // contenders that are sorted in LDS rather than refined further
struct TopNLongArgs : TopN2Args {
  uint4* slab = nullptr;               // [workgroups][ncols]: (image, key high, key low, id)
  unsigned long long* stats = nullptr; // candidates, contenders, refine passes, LDS sorts, key refinements
  int32_t user0 = 0;                   // without a user list: position q is user user0 + q
  int32_t sort_cap = kLongSortCap;
  int32_t area = 0;                    // bytes of the chunk / selection area; the histogram lies behind it
};

// candidate rows (slim_gpu_cand.h, topn_chunk_cand_kernel): no selection; after a chunk the scores of the ids the
// user's candidate row names inside it go to the row's slots.  The rows go by USER id, like the exclusion rows.
struct TopNCandArgs : ChunkArgs {
  const int64_t* cptr = nullptr;  // the set as given: where a user's slots start in `out`
  const int64_t* lptr = nullptr;  // the live entries of every row, ascending by id ...
  const int2* pairs = nullptr;    // ... as (id, slot in the row); ids inside [0, ncols)
  float* out = nullptr;           // slot scores, laid out like the set; cleared before the launch
  int32_t bounds_table = 0;       // the nchunks + 1 chunk bounds of a row fit the merge area
};

__device__ __forceinline__ unsigned long long readlane_key(unsigned long long v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_up_key(unsigned long long v) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t readlane_key(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ uint32_t shfl_up_key(uint32_t v) { return (uint32_t)__shfl_up((int)v, 1); }

// rows of W sorted by id?  (one wavefront per row; flag set when an inversion is found)
__global__ void k_rows_sorted(int32_t nrows, const int64_t* __restrict__ ptr,
                              const int32_t* __restrict__ ind, int32_t* __restrict__ unsorted) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < nrows; r += nwaves) {
    const int64_t s = ptr[r], e = ptr[r + 1];
    bool bad = false;
    for (int64_t j = s + 1 + lane; j < e; j += 64) bad |= ind[j - 1] >= ind[j];
    if (bad) atomicExch(unsorted, 1);
  }
}

// wsplit[r][c] = number of ids of row r below c * cw (binary search; rows are sorted)
__global__ void k_row_split(int32_t nrows, int32_t nchunks, int32_t cw,
                            const int64_t* __restrict__ ptr, const int32_t* __restrict__ ind,
                            uint32_t* __restrict__ split) {
  const int64_t total = (int64_t)nrows * (nchunks + 1);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t r = (int32_t)(t / (nchunks + 1)), c = (int32_t)(t % (nchunks + 1));
    const int64_t s = ptr[r], e = ptr[r + 1];
    const int64_t bound = (int64_t)c * cw;
    int64_t lo = s, hi = e;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)ind[mid] < bound) lo = mid + 1; else hi = mid;
    }
    split[t] = (uint32_t)(lo - s);
  }
}

// The pre-pass of the rank mode: (score, discovery key) of every test entry of the evaluated users, as the
// scorer forms them for that item -- a chunk can only be counted against keys known before it is scanned.
// One wavefront per position, its test entries one after the other.  For an entry t the LANES stand over the
// history items: each finds t in its item's model row by binary search (rows ascend), so the dependent
// searches of 64 history items run side by side; the found products are then added in lane order = history
// order, starting from 0.0f + the first, products and sums rounded separately -- the additions of `update`
// in the same order.  The first history index that has t, and t's position in that row, form the key.  An
// entry equal to a history item, outside [0, ncols) or never touched is no candidate (kNoCandidate, score 0).
// Under a filter (F; inert when its pointers are null) so is an entry whose bit is clear in the bitmap or whose
// id stands in the exclusion row of user u.  The row is taken as it is given -- no order, repeats -- so it is
// walked lane-strided, one ballot per 64 entries; an id outside [0, ncols) never reaches the walk, and a user
// >= xusers has no row (exclusion_row).  The filter is asked BEFORE the searches: a removed entry costs none,
// and a surviving one receives exactly the additions it receives without a filter.  Both filter branches are
// on kernel arguments.
__global__ __launch_bounds__(256) void k_test_keys(int32_t nsel, const int32_t* __restrict__ users, int32_t wrows,
                                                   int32_t ncols, int32_t pos_bits, const int64_t* __restrict__ wptr,
                                                   const int32_t* __restrict__ wind, const float* __restrict__ wval,
                                                   const int64_t* __restrict__ hptr, const int32_t* __restrict__ hind,
                                                   const float* __restrict__ hval, const int64_t* __restrict__ tptr,
                                                   const int32_t* __restrict__ tind, const int64_t* __restrict__ tbase,
                                                   unsigned long long* __restrict__ tkey,
                                                   float* __restrict__ tscore, const FilterArgs F) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t q = wave; q < nsel; q += nwaves) {
    const int32_t u = users ? users[q] : (int32_t)q;
    const int64_t h0 = hptr[u], h1 = hptr[u + 1];
    const int64_t t0 = tptr[u], t1 = tptr[u + 1];
    const int64_t out = tbase[q];
    int64_t x0, x1;
    exclusion_row(F, u, x0, x1);
    for (int64_t z = t0; z < t1; ++z) {
      const int32_t t = tind[z];
      unsigned long long key = kNoCandidate;
      float acc = 0.0f;
      bool in_hist = false, touched = false;  // in_hist: in the history, or removed by the filter
      if (t >= 0 && t < ncols) {
        if (F.bits != nullptr) in_hist = !filter_allows(F.bits, t);
        if (F.xptr != nullptr)
          for (int64_t xb = x0; xb < x1 && !in_hist; xb += 64) {
            const int64_t x = xb + lane;
            in_hist = __ballot(x < x1 && F.xind[x] == t) != 0;
          }
        for (int64_t hb = h0; hb < h1 && !in_hist; hb += 64) {
          const int64_t h = hb + lane;
          bool found = false, same = false;
          float prod = 0.0f;
          uint32_t pos = 0;
          if (h < h1) {
            const int32_t i = hind[h];
            same = i == t;
            if (i >= 0 && i < wrows) {
              const int64_t s = wptr[i], e = wptr[i + 1];
              int64_t lo = s, hi = e;
              while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (wind[mid] < t) lo = mid + 1; else hi = mid;
              }
              if (lo < e && wind[lo] == t) {
#pragma clang fp contract(off)
                found = true;
                prod = (hval ? hval[h] : 1.0f) * wval[lo];
                pos = (uint32_t)(lo - s);
              }
            }
          }
          in_hist = __ballot(same) != 0;
          unsigned long long mask = __ballot(found);
          if (mask && !touched) {
            const int l = __builtin_ctzll(mask);
            key = ((unsigned long long)(uint32_t)(hb - h0 + l) << pos_bits) |
                  (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)pos, l);
            touched = true;
          }
          while (mask) {  // the in-order float sum over the lanes
#pragma clang fp contract(off)
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            acc = acc + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(prod), l));
          }
        }
      }
      if (in_hist || !touched) {
        key = kNoCandidate;
        acc = 0.0f;
      }
      if (lane == 0) {
        tkey[out + (z - t0)] = key;
        tscore[out + (z - t0)] = acc;
      }
    }
  }
}

// ---- long lists: selection by threshold ------------------------------------------------------------
// A candidate's place in the scorer's order is the 96-bit number (image : key), ascending: `image` is the
// complement of the usual order-preserving integer image of a float, so that a higher score is a smaller
// number, and the discovery key breaks ties as better() does.
// The image is taken from the raw bits, which would tell -0.0 from +0.0 where better() does not.  A score is
// never -0.0: its first addition is 0.0f + prod, which is +0.0 for prod == -0.0, and a sum of finite terms
// rounds to -0.0 only when every term is -0.0.  Scores are finite, so no image is that of a NaN either.
__device__ __forceinline__ uint32_t score_image(const float s) {
  const uint32_t b = __float_as_uint(s);
  return ~(b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u));
}
__device__ __forceinline__ float image_score(const uint32_t image) {
  const uint32_t v = ~image;
  return __uint_as_float((v >> 31) ? v ^ 0x80000000u : ~v);
}
// 11 bits of (image : key) from bit `shift` up (shift <= 85)
__device__ __forceinline__ uint32_t long_digit(const uint4 r, const int shift) {
  const unsigned long long key = ((unsigned long long)r.y << 32) | r.z;
  unsigned long long v;
  if (shift >= 64) v = r.x >> (shift - 64);
  else if (shift == 0) v = key;
  else v = (key >> shift) | ((unsigned long long)r.x << (64 - shift));
  return (uint32_t)v & (kLongBins - 1);
}
__device__ __forceinline__ bool long_before(const uint4 a, const uint4 b) {
  return a.x < b.x || (a.x == b.x && (a.y < b.y || (a.y == b.y && a.z < b.z)));
}
// bitonic sort of n = 2^k records in LDS, ascending, by the whole workgroup (ends on a barrier)
template <int NW>
__device__ __forceinline__ void long_sort(uint4* rec, const int n) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n >> 1); t += 64 * NW) {
        const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
        const bool up = (lo & k) == 0;
        const uint4 a = rec[lo], b = rec[hi];
        if (long_before(b, a) == up) {
          rec[lo] = b;
          rec[hi] = a;
        }
      }
      __syncthreads();
    }
}
// control words of the selection, behind the histogram
enum { kLcAppended = 0, kLcWinners, kLcContenders, kLcBin, kLcAbove, kLcInBin, kLcAnd, kLcOr = kLcAnd + 3, kLcWords = 16 };

// The first `N` of the `ncand` records in `slab`, in order, to position q of the outputs.  On entry hist holds
// the counts of the records' leading 11 bits and ctl[kLcWinners] is 0; every thread of the workgroup calls.
// A pass finds the bin that holds the last missing place (wavefront 0, a prefix over the bins), then sweeps
// the contenders once: records of earlier bins go to the winners in LDS, records of that bin are compacted to
// the front of the slab -- in place: a sweep step reads 4 * 64 * NW records, and only behind a barrier writes
// at most as many to places that were read already.  Few enough contenders are sorted in LDS; otherwise the
// next pass takes the 11 bits from the highest bit in which the contenders still differ (known from the AND
// and the OR of their records, gathered in the sweep): below bit 64 they share one score and only the key is
// left to split them.  Nothing depends on the order of the slab.
template <int NW>
__device__ __forceinline__ void long_select(uint4* __restrict__ slab, char* area, uint32_t* hist, int* ctl, const int N,
                            const int sort_cap, const int ncand, int32_t* __restrict__ out_ids,
                            float* __restrict__ out_scores, int32_t* __restrict__ out_cnt, const int64_t q,
                            unsigned long long* __restrict__ stats) {
  constexpr int T = 64 * NW;
  constexpr int kSweep = 4;  // records a thread reads per sweep step: the loads of a step are in flight together
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int winp2 = 1;
  while (winp2 < N) winp2 <<= 1;
  uint4* win = reinterpret_cast<uint4*>(area);
  uint4* srt = win + winp2;
  const uint4 last = make_uint4(~0u, ~0u, ~0u, ~0u);  // sorts behind every record
  const unsigned long long below = (1ull << lane) - 1;
  int nwin = 0, passes = 0, first_bin = 0, sorted = 0, key_pass = 0;
  if (ncand <= N) {
    for (int i = tid; i < ncand; i += T) win[i] = slab[i];
    nwin = ncand;
  } else {
    int ncont = ncand, missing = N, shift = 85;
    for (;;) {
      if (wave == 0) {  // lane l: bins [32 l, 32 l + 32)
        int s = 0;
        for (int j = 0; j < kLongBins / 64; ++j) s += (int)hist[lane * (kLongBins / 64) + j];
        int incl = s;
        for (int off = 1; off < 64; off <<= 1) {
          const int t = __shfl_up(incl, off);
          if (lane >= off) incl += t;
        }
        int c = incl - s;
        if (c < missing && missing <= incl)
          for (int j = 0; j < kLongBins / 64; ++j) {
            const int h = (int)hist[lane * (kLongBins / 64) + j];
            if (c + h >= missing) {
              ctl[kLcBin] = lane * (kLongBins / 64) + j;
              ctl[kLcAbove] = c;
              ctl[kLcInBin] = h;
              break;
            }
            c += h;
          }
        if (lane == 0) {
          ctl[kLcContenders] = 0;
          for (int j = 0; j < 3; ++j) {
            ctl[kLcAnd + j] = -1;
            ctl[kLcOr + j] = 0;
          }
        }
      }
      __syncthreads();
      const int bin = ctl[kLcBin], above = ctl[kLcAbove], in_bin = ctl[kLcInBin];
      const bool take_bin = in_bin == missing - above;  // the bin ends exactly at the N-th: all of it wins
      if (passes == 0) first_bin = in_bin;
      uint32_t a0 = ~0u, a1 = ~0u, a2 = ~0u, o0 = 0, o1 = 0, o2 = 0;
      for (int b0 = 0; b0 < ncont; b0 += kSweep * T) {
        uint4 r[kSweep];
        int cls[kSweep];  // 0 wins, 1 contends, 2 is out
#pragma unroll
        for (int j = 0; j < kSweep; ++j) {
          const int i = b0 + j * T + tid;
          r[j] = last;
          if (i < ncont) r[j] = slab[i];
        }
#pragma unroll
        for (int j = 0; j < kSweep; ++j) {
          const int dg = (int)long_digit(r[j], shift);
          cls[j] = b0 + j * T + tid >= ncont ? 2 : ((dg < bin || (take_bin && dg == bin)) ? 0 : (dg == bin ? 1 : 2));
        }
        __syncthreads();  // the records of this step are read: places before them may be written
#pragma unroll
        for (int j = 0; j < kSweep; ++j) {
          const unsigned long long wm = __ballot(cls[j] == 0);
          if (wm) {
            int at = 0;
            if (lane == 0) at = atomicAdd(&ctl[kLcWinners], __popcll(wm));
            at = __builtin_amdgcn_readfirstlane(at) + __popcll(wm & below);
            if (cls[j] == 0) win[at] = r[j];
          }
          const unsigned long long cm = __ballot(cls[j] == 1);
          if (cm) {
            int at = 0;
            if (lane == 0) at = atomicAdd(&ctl[kLcContenders], __popcll(cm));
            at = __builtin_amdgcn_readfirstlane(at) + __popcll(cm & below);
            if (cls[j] == 1) {
              slab[at] = r[j];
              a0 &= r[j].x; a1 &= r[j].y; a2 &= r[j].z;
              o0 |= r[j].x; o1 |= r[j].y; o2 |= r[j].z;
            }
          }
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        a0 &= (uint32_t)__shfl_xor((int)a0, off); a1 &= (uint32_t)__shfl_xor((int)a1, off);
        a2 &= (uint32_t)__shfl_xor((int)a2, off);
        o0 |= (uint32_t)__shfl_xor((int)o0, off); o1 |= (uint32_t)__shfl_xor((int)o1, off);
        o2 |= (uint32_t)__shfl_xor((int)o2, off);
      }
      if (lane == 0) {
        atomicAnd(&ctl[kLcAnd], (int)a0); atomicAnd(&ctl[kLcAnd + 1], (int)a1); atomicAnd(&ctl[kLcAnd + 2], (int)a2);
        atomicOr(&ctl[kLcOr], (int)o0); atomicOr(&ctl[kLcOr + 1], (int)o1); atomicOr(&ctl[kLcOr + 2], (int)o2);
      }
      __syncthreads();
      nwin = ctl[kLcWinners];
      ncont = ctl[kLcContenders];
      missing = N - nwin;
      if (missing <= 0 || ncont <= 0) break;
      if (ncont <= sort_cap) {
        int p2 = 1;
        while (p2 < ncont) p2 <<= 1;
        for (int i = tid; i < p2; i += T) {
          uint4 v = last;
          if (i < ncont) v = slab[i];
          srt[i] = v;
        }
        __syncthreads();
        long_sort<NW>(srt, p2);
        for (int i = tid; i < missing; i += T) win[nwin + i] = srt[i];
        nwin += missing;
        sorted = 1;
        break;
      }
      // the contenders differ (keys are distinct): the next 11 bits start at the highest differing bit
      const uint32_t d0 = (uint32_t)(ctl[kLcAnd] ^ ctl[kLcOr]), d1 = (uint32_t)(ctl[kLcAnd + 1] ^ ctl[kLcOr + 1]),
                     d2 = (uint32_t)(ctl[kLcAnd + 2] ^ ctl[kLcOr + 2]);
      const int top = d0 ? 95 - __clz((int)d0) : (d1 ? 63 - __clz((int)d1) : 31 - __clz((int)(d2 | 1u)));
      shift = top > 10 ? top - 10 : 0;
      ++passes;
      if (top < 64) key_pass = 1;
      for (int z = tid; z < kLongBins; z += T) hist[z] = 0;
      __syncthreads();
      for (int i = tid; i < ncont; i += T) atomicAdd(&hist[long_digit(slab[i], shift)], 1u);
      __syncthreads();
    }
  }
  // the winners in order, then out
  int p2 = 1;
  while (p2 < nwin) p2 <<= 1;
  __syncthreads();
  for (int i = nwin + tid; i < p2; i += T) win[i] = last;
  __syncthreads();
  long_sort<NW>(win, p2);
  for (int r = tid; r < nwin; r += T) {
    const uint4 w = win[r];
    out_ids[q * N + r] = (int32_t)w.w;
    out_scores[q * N + r] = image_score(w.x);
  }
  if (tid == 0) {
    out_cnt[q] = nwin;
    atomicAdd(stats, (unsigned long long)ncand);
    if (first_bin) atomicAdd(stats + 1, (unsigned long long)first_bin);
    if (passes) atomicAdd(stats + 2, (unsigned long long)passes);
    if (sorted) atomicAdd(stats + 3, 1ull);
    if (key_pass) atomicAdd(stats + 4, 1ull);
  }
}

// ---- the chunk scorer: shared phases and a mode ------------------------------------------------------
// KeyT: discovery key (history index << pos_bits | position in the model row).  32 bits when the longest history and
// the longest model row allow it (8 bytes of LDS per item: chunks of 2304 ids), else 64.
// Drawing a position, preparing a chunk, walking the history into it and scanning it are the same whatever is wanted
// of the candidates.  What is wanted is a Mode: it owns its argument struct and its state (one object per user) and
// says what happens when a user begins (begin: it reads where the history lies, at its own point; false: skip this
// user), with a finished chunk of this wavefront (chunk) and after the last chunk (finish; every thread calls).
// `pos` is the position in LDS: it stays until the barrier that ends the user and is re-read after the chunks, so
// that it does not occupy a scalar register through them.
// a thread's place in the workgroup and its wavefront's part of the dynamic LDS
template <int NW, typename KeyT>
struct ChunkLds {
  static constexpr KeyT kUnt = ~KeyT(0), kExc = ~KeyT(0) - 1;
  char* smem;
  int tid, lane, wave, cw;
  KeyT* disc;    // [cw]: this wavefront's chunk
  float* score;  // [cw]
  char* marea;   // behind the chunks: the merge area of the lists, the test keys and counts of the ranks
  __device__ __forceinline__ ChunkLds(char* s, const int CW) : smem(s), tid(threadIdx.x), lane(tid & 63), cw(CW) {
    wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    disc = reinterpret_cast<KeyT*>(smem) + (size_t)wave * CW;
    score = reinterpret_cast<float*>(smem + (size_t)NW * CW * sizeof(KeyT)) + (size_t)wave * CW;
    marea = smem + (size_t)NW * CW * (sizeof(KeyT) + 4);
  }
};

// a position from the queue into `pos`, and its user (looked up once; outputs are indexed by the position).
// -1: the queue is empty.
template <class Args>
__device__ __forceinline__ int draw_user(const Args& T, int& pos, const int tid) {
  if (tid == 0) pos = atomicAdd(T.queue, 1);
  __syncthreads();
  int u = __builtin_amdgcn_readfirstlane(pos);
  if (u >= T.nusers) return -1;
  if (T.users) u = __builtin_amdgcn_readfirstlane(T.users[u]);
  return u;
}

// Candidacy is decided here and nowhere else: a slot that leaves as kExc is no candidate whatever the history
// walk adds to it, and nothing behind the walk looks at such a slot.  Without a filter the history's items are
// excluded; with one (FilterArgs) so are the ids its bitmap does not allow -- the 64 lanes of a step read the two
// words of their 64 ids, any `base`, and the short last chunk never reads past word (ncols - 1) / 32 -- and the
// ids of the exclusion row of user `u` (the body's, after Mode::begin has settled which user the position is),
// under the history's range guard.  The row's bounds are two scalar loads per chunk: held across the walk they
// would take four scalar registers it has not got.  The branches are on kernel arguments: wave-uniform.
// MARK false (a mode that scores given candidates, CandMode): nobody is excluded, not the history either -- every
// slot leaves as kUnt and none is ever kExc.
template <bool MARK = true, class Args, class Lds>
__device__ __forceinline__ void prepare_chunk(const Args& T, const Lds& L, const int base, const int width,
                                              const int64_t h0, const int64_t h1, const int u) {
  if constexpr (!MARK) {
    for (int k = L.lane; k < width; k += 64) L.disc[k] = Lds::kUnt;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    return;
  }
  if (T.flt.bits == nullptr)
    for (int k = L.lane; k < width; k += 64) L.disc[k] = Lds::kUnt;
  else
    for (int k = L.lane; k < width; k += 64) L.disc[k] = filter_allows(T.flt.bits, base + k) ? Lds::kUnt : Lds::kExc;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  for (int64_t h = h0 + L.lane; h < h1; h += 64) {  // history items are never recommended
    const int i = T.hind[h];
    if (i >= base && i < base + width) L.disc[i - base] = Lds::kExc;
  }
  if (T.flt.xptr != nullptr) {  // nor are the user's exclusions
    int64_t x0, x1;
    exclusion_row(T.flt, u, x0, x1);
    for (int64_t x = x0 + L.lane; x < x1; x += 64) {
      const int i = T.flt.xind[x];
      if (i >= base && i < base + width) L.disc[i - base] = Lds::kExc;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
}

// the user's history, in order, into chunk c (ids from `base`) of this wavefront
template <typename KeyT, class Args, class Lds>
__device__ __forceinline__ void walk_history(const Args& T, const Lds& L, const int c, const int base, const int64_t h0,
                                             const int64_t h1) {
  constexpr int D = kT2Depth;
  constexpr KeyT kUnt = Lds::kUnt;
  const int lane = L.lane;
  KeyT* disc = L.disc;
  float* score = L.score;
  // branch-free: both reads issue together; an untouched slot reads garbage as its score and
  // selects 0; an excluded slot keeps its key and accumulates a score nobody reads
  auto update = [&](const int idx, const KeyT key, const float prod) {
#pragma clang fp contract(off)
    const KeyT d = disc[idx];
    const float old = score[idx];
    const bool first = d == kUnt;
    disc[idx] = first ? key : d;
    score[idx] = (first ? 0.0f : old) + prod;
  };

  for (int64_t hb = h0; hb < h1; hb += 64) {
    const int nb = (h1 - hb) < 64 ? (int)(h1 - hb) : 64;
    // lane l: where history item hb + l meets this chunk
    uint32_t my_s = 0;  // element offset of the segment in wind / wval (nnz(W) < 2^31)
    int my_len = 0;
    uint32_t my_p0 = 0;
    float my_r = 1.0f;
    if (lane < nb) {
      const int i = T.hind[hb + lane];
      if (T.hval) my_r = T.hval[hb + lane];
      if (i >= 0 && i < T.nitems_rows) {
        const uint32_t* sp = T.wsplit + (int64_t)i * (T.nchunks + 1) + c;
        my_p0 = sp[0];
        my_len = (int)(sp[1] - my_p0);
        my_s = (uint32_t)T.wptr[i] + my_p0;
      }
    }
    // The segment loads are UNCONDITIONAL instructions (clamped address, predicate applied
    // when the entry is consumed) and every step issues exactly one fetch: the number of
    // loads in flight is then the same on every path, so the compiler can wait for the oldest
    // fetch only (s_waitcnt vmcnt(2*(D-1))).  With loads under `if (lane < len)` it had to
    // drain the queue at every step, and the kernel ran at one L2 round trip per step
    // whatever the depth.  Items past the batch have length 0: their steps do nothing.
    int qk[D], qlen[D];
    float qv[D];
    auto fetch = [&](const int l, int& k, float& v, int& len) {
      const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)my_s, l);
      len = __builtin_amdgcn_readlane(my_len, l);
      uint32_t j = s + (uint32_t)lane;
      j = j < T.wlast ? j : T.wlast;
      k = T.wind[j];
      v = T.wval[j];
    };
#pragma unroll
    for (int d = 0; d < D; ++d) fetch(d, qk[d], qv[d], qlen[d]);
    const int nbp = (nb + D - 1) / D * D;  // <= 64: lanes past nb hold length 0
    for (int lb = 0; lb < nbp; lb += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int l = lb + d;
        const int kraw = qk[d];
        const float v = qv[d];
        const int len = qlen[d];
        fetch((l + D) & 63, qk[d], qv[d], qlen[d]);
        const float rating = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_r), l));
        const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)my_p0, l);
        const KeyT hkey = (KeyT)(uint32_t)(hb - h0 + l) << T.pos_bits;
        if (lane < len) {
#pragma clang fp contract(off)
          const float prod = rating * v;
          update(kraw - base, hkey | (KeyT)(p0 + (uint32_t)lane), prod);
        }
        if (len > 64) {  // a segment longer than one wavefront step (dense rows)
          const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)my_s, l);
          for (uint32_t t = 64 + (uint32_t)lane; t < (uint32_t)len; t += 64) {
#pragma clang fp contract(off)
            const float prod = rating * T.wval[s + t];
            update(T.wind[s + t] - base, hkey | (KeyT)(p0 + t), prod);
          }
        }
      }
    }
  }
}

// the slots of a finished chunk, 64 at a time: f(k, d, sc, cand) with lane l at slot k = 64 * step + l, its
// key and score (kUnt and 0 past the chunk's width) and whether it is a candidate (touched and not excluded)
template <class Lds, class F>
__device__ __forceinline__ void scan_chunk(const Lds& L, const int width, F&& f) {
  for (int kb = 0; kb < width; kb += 64) {
    const int k = kb + L.lane;
    auto d = Lds::kUnt;
    float sc = 0.0f;
    if (k < width) {
      d = L.disc[k];
      sc = L.score[k];
    }
    f(k, d, sc, d < Lds::kExc);
  }
}

// Lists of up to 64. A wavefront keeps its N best in registers (lane t = rank t); wavefront 0 merges the lists
// through LDS and writes the user's row. EVAL: the fused epilogue of the resident evaluation. Once wavefront 0 has
// merged the lists, lane t holds rank t; the user's test row sits in LDS (loaded by the whole workgroup into
// wavefront 0's score chunk, which is free by then; what does not fit is walked from HBM), every lane tests its id
// against it, one ballot gives the hit mask, and the user's UserTerms records are formed exactly as k_user_terms
// (eval.hip) forms them -- gain added in rank order, ideal in test-row order, float accumulators fed with double
// terms; the set bits are walked once and the record of cutoff k leaves when the walk passes rank cut.c[k]
// (eval_terms.hpp: the additions behind a cutoff are a prefix of those behind the next one, so every record is the
// one a separate evaluation with lists of that length forms). Lists are written only when an output pointer is given.
template <int NW, typename KeyT, bool EVAL>
struct ListsMode {
  using Args = std::conditional_t<EVAL, TopNEvalArgs, TopN2Args>;
  using Lds = ChunkLds<NW, KeyT>;
  static constexpr bool kMarkHistory = true;
  // this wavefront's N best so far: lane t holds rank t
  float ls = 0.0f;
  KeyT ld = Lds::kUnt;
  int lid = -1;
  int count = 0;
  float worst_s = 0.0f;
  KeyT worst_d = 0;

  __device__ __forceinline__ void insert(const int lane, const int N, const float cs, const KeyT cd, const int cid) {
    const bool ahead = lane < count && better(ls, ld, cs, cd);
    const int p = __popcll(__ballot(ahead));  // sorted list: the entries ahead are ranks 0..p-1
    const float us = __shfl_up(ls, 1);
    const KeyT ud = shfl_up_key(ld);
    const int uid = __shfl_up(lid, 1);
    if (lane > p && lane < N) { ls = us; ld = ud; lid = uid; }
    if (lane == p) { ls = cs; ld = cd; lid = cid; }
    if (count < N) ++count;
    if (count == N) {
      worst_s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ls), N - 1));
      worst_d = readlane_key(ld, N - 1);
    }
  }
  __device__ __forceinline__ void offer(const int lane, const int N, const float cs, const KeyT cd, const int cid) {
    if (count < N || better(cs, cd, worst_s, worst_d)) insert(lane, N, cs, cd, cid);
  }

  __device__ __forceinline__ bool begin(const Args& T, const Lds&, int& u, const int&, int64_t& h0, int64_t& h1) {
    h0 = uni64(T.hptr[u]), h1 = uni64(T.hptr[u + 1]);
    return true;
  }

  // candidates of this chunk against the wavefront's N best
  __device__ __forceinline__ void chunk(const Args& T, const Lds& L, const int base, const int width) {
    const int lane = L.lane, N = T.nrcmds;
    scan_chunk(L, width, [&](const int k, const KeyT d, const float sc, const bool cand) {
      bool want = cand;
      if (want && count == N) want = better(sc, d, worst_s, worst_d);
      unsigned long long mask = __ballot(want);
      while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float cs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sc), l));
        const KeyT cd = readlane_key(d, l);
        offer(lane, N, cs, cd, base + (k - lane) + l);
      }
    });
  }

  // merge the wavefronts' lists (wavefront 0), write the user's row
  __device__ __forceinline__ void finish(const Args& T, const Lds& L, const int u, const int& pos) {
    const int lane = L.lane, wave = L.wave, CW = L.cw, N = T.nrcmds;
    float* m_s = reinterpret_cast<float*>(L.marea);
    KeyT* m_d = reinterpret_cast<KeyT*>(L.marea + NW * kT2MaxN * 4);
    int* m_id = reinterpret_cast<int*>(L.marea + NW * kT2MaxN * 12);
    int* m_cnt = reinterpret_cast<int*>(L.marea + NW * kT2MaxN * 16);
    if (lane < kT2MaxN) {
      m_s[wave * kT2MaxN + lane] = ls;
      m_d[wave * kT2MaxN + lane] = ld;
      m_id[wave * kT2MaxN + lane] = lid;
    }
    if (lane == 0) m_cnt[wave] = count;
    __syncthreads();
    int64_t t0 = 0, t1 = 0;
    int tl = 0;
    // (every wavefront is past its chunks: wavefront 0's score chunk is free until the next user)
    int* s_test = reinterpret_cast<int*>(L.smem + (size_t)NW * CW * sizeof(KeyT));
    if constexpr (EVAL) {
      t0 = uni64(T.tptr[u]);
      t1 = uni64(T.tptr[u + 1]);
      tl = (t1 - t0) < (int64_t)CW ? (int)(t1 - t0) : CW;
      for (int z = L.tid; z < tl; z += 64 * NW) s_test[z] = T.tind[t0 + z];
    }
    const int q = __builtin_amdgcn_readfirstlane(pos);  // (unchanged until the barrier that ends this user)
    if (wave == 0) {
      for (int w = 1; w < NW; ++w) {
        const int cw_ = __builtin_amdgcn_readfirstlane(m_cnt[w]);
        for (int t = 0; t < cw_; ++t) {
          const float cs = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m_s[w * kT2MaxN + t])));
          const KeyT cd = readlane_key(m_d[w * kT2MaxN + t], 0);
          const int cid = __builtin_amdgcn_readfirstlane(m_id[w * kT2MaxN + t]);
          offer(lane, N, cs, cd, cid);
        }
      }
      if (!EVAL || T.out_ids != nullptr) {
        if (lane < count) {
          T.out_ids[(int64_t)q * N + lane] = lid;
          T.out_scores[(int64_t)q * N + lane] = ls;
        }
        if (lane == 0) T.out_cnt[q] = count;
      }
    }
    if constexpr (EVAL) {
      __syncthreads();  // the test row is in LDS
      if (wave == 0) {
        // what does not depend on the cutoff, once: the test row's classes, ideal, the hit mask
        const int64_t tlen = t1 - t0;
        int ntrue0 = 0, ntrue1 = 0, flags = 0;
        float ideal = 0.0f;
        unsigned long long mask = 0;
        if (tlen >= 1) {
          flags = 1;
          bool hit = false;
          for (int64_t z = 0; z < tlen; ++z) {
            const int it = z < tl ? s_test[z] : T.tind[t0 + z];
            const int cls = (it >= 0 && it < T.fm_ncols) ? T.fmarker[it] : 1;
            if (cls) ++ntrue1; else ++ntrue0;
            flags |= cls ? 4 : 2;
            ideal = (float)((double)ideal + 1.0 / (1.0 + double(z)));
            hit = hit || it == lid;
          }
          mask = __ballot(hit && lane < count);  // set bits = ranks that hit
        }
        // one walk in rank order; cutoff k's record is the sums of the ranks below cut.c[k]
        HitWalk w;
        const unsigned long long cuts = T.cut.packed();
        for (int k = 0; k < T.cut.n; ++k) {
          const int c = Cutoffs::at(cuts, k);
          while (mask && __builtin_ctzll(mask) < c) {
            const int r = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int id = __builtin_amdgcn_readlane(lid, r);
            w.hit(r, (id >= 0 && id < T.fm_ncols) ? T.fmarker[id] : 1);
          }
          const UserTerms t = w.terms(ntrue0, ntrue1, tlen, ideal, flags);
          if (lane == 0) T.terms[(int64_t)k * T.nusers + q] = t;
        }
      }
    }
  }
};

// Ranks: no lists.  The merge area holds the user's test keys and one integer count per key; the candidate
// scan of a chunk adds to each count the chunk's slots that stand before the key (a ballot and a popcount per
// 64 slots, gathered in registers -- lane j owns key j -- and added to LDS once per chunk); after the chunks
// wavefront 0 writes rank = 1 + count.
template <int NW, typename KeyT>
struct RankMode {
  using Args = TopNRankArgs;
  using Lds = ChunkLds<NW, KeyT>;
  static constexpr bool kMarkHistory = true;
  float* r_s = nullptr;  // the user's test keys of this pass in the merge area, and their counts
  KeyT* r_d = nullptr;
  int* r_c = nullptr;
  int ng = 0;         // test entries of this user served by this pass
  int64_t rbase = 0;  // ... and where they start in the rank arrays

  __device__ __forceinline__ bool begin(const Args& T, const Lds& L, int& u, const int& pos, int64_t& h0, int64_t& h1) {
    h0 = uni64(T.hptr[u]), h1 = uni64(T.hptr[u + 1]);
    r_s = reinterpret_cast<float*>(L.marea);
    r_d = reinterpret_cast<KeyT*>(L.marea + NW * kT2MaxN * 4);
    r_c = reinterpret_cast<int*>(L.marea + NW * kT2MaxN * 12);
    const int64_t tlen = uni64(T.tptr[u + 1]) - uni64(T.tptr[u]);
    const int64_t left = tlen - (int64_t)T.g0;
    ng = left < 0 ? 0 : (left < (int64_t)T.gsize ? (int)left : T.gsize);
    rbase = uni64(T.tbase[__builtin_amdgcn_readfirstlane(pos)]) + T.g0;
    if (ng == 0 || h0 == h1) {  // nothing to count (an empty history: k_test_keys said "no candidate")
      for (int z = L.tid; z < ng; z += 64 * NW) {
        T.rank[rbase + z] = 0;
        T.rscore[rbase + z] = 0.0f;
      }
      return false;
    }
    for (int z = L.tid; z < ng; z += 64 * NW) {
      r_s[z] = T.tscore[rbase + z];
      r_d[z] = (KeyT)T.tkey[rbase + z];
      r_c[z] = 0;
    }
    __syncthreads();
    return true;
  }

  // candidates of this chunk against the user's test keys: integer adds, so any order
  __device__ __forceinline__ void chunk(const Args&, const Lds& L, const int, const int width) {
    const int lane = L.lane;
    for (int jb = 0; jb < ng; jb += 64) {
      const int nj = (ng - jb) < 64 ? (ng - jb) : 64;
      float my_ts = 0.0f;
      KeyT my_td = Lds::kUnt;
      if (lane < nj) {
        my_ts = r_s[jb + lane];
        my_td = r_d[jb + lane];
      }
      int my_cnt = 0;
      scan_chunk(L, width, [&](const int, const KeyT d, const float sc, const bool cand) {
        if (__ballot(cand) == 0) return;
        for (int j = 0; j < nj; ++j) {
          const float ts = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_ts), j));
          const KeyT td = readlane_key(my_td, j);
          const int ahead = __popcll(__ballot(cand && better(sc, d, ts, td)));
          if (lane == j) my_cnt += ahead;
        }
      });
      if (lane < nj && my_cnt) atomicAdd(&r_c[jb + lane], my_cnt);
    }
  }

  __device__ __forceinline__ void finish(const Args& T, const Lds& L, int, const int&) {
    __syncthreads();  // every wavefront's counts are in
    if (L.wave == 0)
      for (int z = L.lane; z < ng; z += 64) {
        const bool cand = r_d[z] != Lds::kUnt;
        T.rank[rbase + z] = cand ? 1 + r_c[z] : 0;
        T.rscore[rbase + z] = cand ? r_s[z] : 0.0f;
      }
  }
};

// Long lists: lists of up to SLIMGPU_MAX_LIST.  No lists in registers and no merge: the candidate scan of a
// chunk appends the chunk's candidates to the workgroup's slab (a ballot and a popcount per 64 slots, one LDS
// atomic per wavefront step for the place) and counts the leading bits of their order in a histogram that lies
// where the merge area would; long_select picks and orders the list after the chunks, in the LDS of the
// chunks, which are free by then.
template <int NW, typename KeyT>
struct LongMode {
  using Args = TopNLongArgs;
  using Lds = ChunkLds<NW, KeyT>;
  static constexpr bool kMarkHistory = true;
  uint32_t* l_hist = nullptr;  // the histogram and the control words, behind the chunk / selection area
  int* l_ctl = nullptr;

  __device__ __forceinline__ bool begin(const Args& T, const Lds& L, int& u, const int&, int64_t& h0, int64_t& h1) {
    if (!T.users) u += T.user0;
    l_hist = reinterpret_cast<uint32_t*>(L.smem + T.area);
    l_ctl = reinterpret_cast<int*>(l_hist + kLongBins);
    for (int z = L.tid; z < kLongBins; z += 64 * NW) l_hist[z] = 0;
    if (L.tid == 0) l_ctl[kLcAppended] = l_ctl[kLcWinners] = 0;
    __syncthreads();
    h0 = uni64(T.hptr[u]), h1 = uni64(T.hptr[u + 1]);
    return true;
  }

  // candidates of this chunk to the slab, their leading bits to the histogram
  __device__ __forceinline__ void chunk(const Args& T, const Lds& L, const int base, const int width) {
    const int lane = L.lane;
    uint4* slab = T.slab + (size_t)blockIdx.x * (size_t)T.ncols;
    scan_chunk(L, width, [&](const int k, const KeyT d, const float sc, const bool cand) {
      const unsigned long long mask = __ballot(cand);
      if (mask == 0) return;
      int at = 0;
      if (lane == 0) at = atomicAdd(&l_ctl[kLcAppended], __popcll(mask));
      at = __builtin_amdgcn_readfirstlane(at) + __popcll(mask & ((1ull << lane) - 1));
      if (cand) {  // (a user has at most ncols candidates: every slot of every chunk once)
        const uint32_t image = score_image(sc);
        const unsigned long long key = (unsigned long long)d;
        slab[at] = make_uint4(image, (uint32_t)(key >> 32), (uint32_t)key, (uint32_t)(base + k));
        atomicAdd(&l_hist[image >> 21], 1u);
      }
    });
  }

  __device__ __forceinline__ void finish(const Args& T, const Lds& L, int, const int& pos) {
    __syncthreads();  // every wavefront's candidates are in the slab and in the histogram
    const int ncand = l_ctl[kLcAppended];
    long_select<NW>(T.slab + (size_t)blockIdx.x * (size_t)T.ncols, L.smem, l_hist, l_ctl, T.nrcmds, T.sort_cap, ncand,
                    T.out_ids, T.out_scores, T.out_cnt, (int64_t)__builtin_amdgcn_readfirstlane(pos), T.stats);
  }
};

// Candidate rows: the scores of the ids a caller names per user (slim_gpu_cand.h), history items included, so
// prepare_chunk marks nothing (kMarkHistory false).  The device form of the set holds a row's live entries
// ascending by id, so the entries of chunk c are one stretch of the row.  begin finds the nchunks + 1 stretch
// bounds ONCE per user -- thread c searches bound c * cw, the offsets (from the row's start) go to the merge
// area, which this mode has no other use for; a table that does not fit there is replaced by a wave-uniform
// search per chunk.  chunk: lanes stride over the stretch, read (key, score) of slot id - base and write the
// score -- 0 for a slot nothing touched -- to the entry's slot of the output.  Entries that are not live (an
// earlier occurrence of a repeated id, an id outside [0, ncols)) and the rows of users without a history are
// never written: the output was cleared before the launch.  The row's pointers are scalar loads per chunk, like
// the exclusion row's, so that they hold no scalar registers across the walk.
template <int NW, typename KeyT>
struct CandMode {
  using Args = TopNCandArgs;
  using Lds = ChunkLds<NW, KeyT>;
  static constexpr bool kMarkHistory = false;
  int user = 0;

  // first entry of [r0, r1) whose id is >= bound
  static __device__ __forceinline__ int64_t lower(const int2* __restrict__ pairs, int64_t lo, int64_t hi,
                                                  const int64_t bound) {
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)pairs[mid].x < bound) lo = mid + 1; else hi = mid;
    }
    return lo;
  }

  __device__ __forceinline__ bool begin(const Args& T, const Lds& L, int& u, const int&, int64_t& h0, int64_t& h1) {
    h0 = uni64(T.hptr[u]), h1 = uni64(T.hptr[u + 1]);
    user = u;
    const int64_t r0 = uni64(T.lptr[u]), r1 = uni64(T.lptr[u + 1]);
    if (h0 == h1 || r0 == r1) return false;  // every slot of the row keeps its 0
    if (T.bounds_table) {
      int* bounds = reinterpret_cast<int*>(L.marea);
      for (int c = L.tid; c <= T.nchunks; c += 64 * NW)
        bounds[c] = (int)(lower(T.pairs, r0, r1, (int64_t)c * T.cw) - r0);
      __syncthreads();
    }
    return true;
  }

  __device__ __forceinline__ void chunk(const Args& T, const Lds& L, const int base, const int width) {
    const int64_t r0 = uni64(T.lptr[user]), c0 = uni64(T.cptr[user]);
    int64_t lo, hi;
    if (T.bounds_table) {
      const int* bounds = reinterpret_cast<const int*>(L.marea);
      const int c = base / T.cw;
      lo = r0 + __builtin_amdgcn_readfirstlane(bounds[c]);
      hi = r0 + __builtin_amdgcn_readfirstlane(bounds[c + 1]);
    } else {
      const int64_t r1 = uni64(T.lptr[user + 1]);
      lo = uni64(lower(T.pairs, r0, r1, (int64_t)base));
      hi = uni64(lower(T.pairs, lo, r1, (int64_t)base + width));
    }
    for (int64_t e = lo + L.lane; e < hi; e += 64) {
      const int2 p = T.pairs[e];
      const int k = p.x - base;  // in [0, width): the stretch holds the ids of this chunk only
      const KeyT d = L.disc[k];
      const float sc = L.score[k];
      T.out[c0 + p.y] = d == Lds::kUnt ? 0.0f : sc;
    }
  }

  __device__ __forceinline__ void finish(const Args&, const Lds&, int, const int&) {}
};

template <int NW, typename KeyT, class Mode>
__device__ __forceinline__ void topn_chunk_body(const typename Mode::Args& T) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_user;
  const ChunkLds<NW, KeyT> L(smem, T.cw);
  for (;;) {
    int u = draw_user(T, s_user, L.tid);
    if (u < 0) break;
    int64_t h0, h1;
    Mode M;
    if (M.begin(T, L, u, s_user, h0, h1)) {
      for (int c = L.wave; c < T.nchunks; c += NW) {
        const int base = c * T.cw;
        const int width = (T.ncols - base) < T.cw ? (T.ncols - base) : T.cw;
        prepare_chunk<Mode::kMarkHistory>(T, L, base, width, h0, h1, u);
        walk_history<KeyT>(T, L, c, base, h0, h1);
        M.chunk(T, L, base, width);
      }
      M.finish(T, L, u, s_user);
    }
    __syncthreads();  // s_user and the user's LDS are read: the next position may be drawn
  }
}

template <int NW, typename KeyT>
__global__ __launch_bounds__(64 * NW) void topn_chunk_kernel(const TopN2Args T) {
  topn_chunk_body<NW, KeyT, ListsMode<NW, KeyT, false>>(T);
}
template <int NW, typename KeyT>
__global__ __launch_bounds__(64 * NW) void topn_chunk_eval_kernel(const TopNEvalArgs T) {
  topn_chunk_body<NW, KeyT, ListsMode<NW, KeyT, true>>(T);
}
template <int NW, typename KeyT>
__global__ __launch_bounds__(64 * NW) void topn_chunk_rank_kernel(const TopNRankArgs T) {
  topn_chunk_body<NW, KeyT, RankMode<NW, KeyT>>(T);
}
template <int NW, typename KeyT>
__global__ __launch_bounds__(64 * NW) void topn_chunk_long_kernel(const TopNLongArgs T) {
  topn_chunk_body<NW, KeyT, LongMode<NW, KeyT>>(T);
}
template <int NW, typename KeyT>
__global__ __launch_bounds__(64 * NW) void topn_chunk_cand_kernel(const TopNCandArgs T) {
  topn_chunk_body<NW, KeyT, CandMode<NW, KeyT>>(T);
}

// The lists of candidate rows, after the scorer on the same stream: one workgroup per position.  A row's records
// (image of the slot's score, slot, id) -- every entry of the row as given, dead ones with their 0 -- are sorted
// in LDS (long_sort: image ascending = score descending, then slot ascending: emit_best's order) and the first
// min(nrcmds, row length) leave.  Rows are at most SLIMGPU_MAX_LIST long (the host refuses longer ones).
constexpr int kCandListWaves = 4;
__global__ __launch_bounds__(64 * kCandListWaves) void k_cand_lists(
    int32_t npos, const int32_t* __restrict__ users, int32_t nrcmds, const int64_t* __restrict__ cptr,
    const int32_t* __restrict__ cind, const float* __restrict__ slot_scores, int32_t* __restrict__ out_ids,
    float* __restrict__ out_scores, int32_t* __restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* rec = reinterpret_cast<uint4*>(smem);
  const int tid = threadIdx.x;
  for (int q = (int)blockIdx.x; q < npos; q += (int)gridDim.x) {
    const int u = users ? users[q] : q;
    const int64_t c0 = cptr[u];
    const int len = min((int)(cptr[u + 1] - c0), kLongMaxN);
    int p2 = 1;
    while (p2 < len) p2 <<= 1;
    for (int j = tid; j < p2; j += 64 * kCandListWaves)
      rec[j] = j < len ? make_uint4(score_image(slot_scores[c0 + j]), 0u, (uint32_t)j, (uint32_t)cind[c0 + j])
                       : make_uint4(~0u, ~0u, ~0u, ~0u);
    __syncthreads();
    long_sort<kCandListWaves>(rec, p2);
    const int n = len < nrcmds ? len : nrcmds;
    for (int r = tid; r < n; r += 64 * kCandListWaves) {
      const uint4 w = rec[r];
      out_ids[(int64_t)q * nrcmds + r] = (int32_t)w.w;
      out_scores[(int64_t)q * nrcmds + r] = image_score(w.x);
    }
    if (tid == 0) out_cnt[q] = n;
    __syncthreads();  // the records are read: the next position may overwrite them
  }
}

// facts[0] = entries of the longest row, facts[1] = 1 when some row's ids are not strictly ascending
// (both preset to 0)
__global__ void k_row_facts(int32_t nrows, const int64_t* __restrict__ ptr, const int32_t* __restrict__ ind,
                            int32_t* __restrict__ facts) {
  int32_t mx = 0;
  bool bad = false;
  for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    const int64_t s = ptr[r], e = ptr[r + 1];
    mx = max(mx, (int32_t)(e - s));
    for (int64_t j = s + 1; j < e; ++j) bad |= ind[j - 1] >= ind[j];
  }
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
  if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(facts, mx);
  if (bad) atomicExch(facts + 1, 1);
}

// entries of the longest row among the rows at `nsel` positions of a CSR (users == nullptr: rows
// [0, nsel)), and, when `total` is given, the entries of all of them (both preset to 0)
__global__ void k_longest_row(int32_t nsel, const int32_t* __restrict__ users, const int64_t* __restrict__ ptr,
                              int32_t* __restrict__ out, unsigned long long* __restrict__ total) {
  int32_t mx = 0;
  unsigned long long sum = 0;
  for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nsel; q += gridDim.x * blockDim.x) {
    const int32_t r = users ? users[q] : q;
    const int64_t len = ptr[r + 1] - ptr[r];
    mx = max(mx, (int32_t)len);
    sum += (unsigned long long)len;
  }
  for (int off = 32; off > 0; off >>= 1) {
    mx = max(mx, __shfl_xor(mx, off));
    const uint32_t lo = __shfl_xor((uint32_t)sum, off), hi = __shfl_xor((uint32_t)(sum >> 32), off);
    sum += ((unsigned long long)hi << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(out, mx);
  if (total && (threadIdx.x & 63) == 0 && sum) atomicAdd(total, sum);
}

// the scorer's byte model: entries of the model rows that the histories of the users at `nsel` positions
// stream (out preset to 0).  One wavefront per position, its lanes over the history.
__global__ void k_streamed_entries(int32_t nsel, const int32_t* __restrict__ users, const int64_t* __restrict__ hptr,
                                   const int32_t* __restrict__ hind, int32_t wrows,
                                   const int64_t* __restrict__ wptr, unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long sum = 0;
  for (int64_t q = wave; q < nsel; q += nwaves) {
    const int32_t u = users ? users[q] : (int32_t)q;
    const int64_t h1 = hptr[u + 1];
    for (int64_t h = hptr[u] + lane; h < h1; h += 64) {
      const int32_t i = hind[h];
      if (i >= 0 && i < wrows) sum += (unsigned long long)(wptr[i + 1] - wptr[i]);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)sum, off), hi = __shfl_xor((uint32_t)(sum >> 32), off);
    sum += ((unsigned long long)hi << 32) | lo;
  }
  if (lane == 0 && sum) atomicAdd(out, sum);
}
}  // namespace
}  // namespace slimamd
