// topn.hip -- top-N recommendation for every user on the GPU.
//
// What it computes is GetRecommendations of the reference
// (/root/reference/src/libslim/predict.c:15-71) applied to every row of a history matrix
// (Py_SLIM_Predict, src/libslim/pyapi.c:530-563): the score of candidate k is the sum over
// the user's history items i of rating_i * W[i,k] (row i of the model), items of the
// history are excluded, the N best candidates are returned in descending score order.
//
// One wavefront per user, results BIT-IDENTICAL to the library's host path
// (host_csr.cpp::top_n):
//   * history rows are walked in order and the nnz of a row go to different lanes (ids in a
//     row are distinct), so every candidate receives its float additions in exactly the
//     host's order; products and sums are rounded separately (no FMA contraction);
//   * ties are broken by discovery order like the host (the reference's gk_fkvsortd leaves
//     tie order undefined): the first touch of a candidate records (history index, position
//     in the W row), which sorts like the host's discovery counter;
//   * selection: one pass over the score vector with a per-lane sorted list of the N best
//     (LDS), then N rounds of a wave-wide arg-max over the 64 list heads.
// The score/discovery vectors (12 bytes per item) live in a per-wavefront HBM slab.  A second kernel
// (topn_chunk_kernel, below) keeps them in LDS and serves lists of up to 64 from models with sorted rows; its
// long-list form (topn_chunk_long_kernel) selects by threshold and serves lists of up to SLIMGPU_MAX_LIST.
//
// Host side: every entry point -- predict_device / predict_device_view (a host history), matrix_predict, their
// forms for lists of up to SLIMGPU_MAX_LIST (predict_lists / predict_lists_view / matrix_predict_lists),
// model_evaluate and the ranked calls model_ranks / model_evaluate_ranked (the resident matrix) -- stages what it lacks on the device (host_stage.hpp),
// describes the model and the histories as views and goes through queue_scorer, the one place that
// chooses the kernel, builds the split table, fills the kernel arguments and launches.
#include <hip/hip_runtime.h>

#include <new>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "eval_terms.hpp"
#include "hip_check.hpp"
#include "host_csr.hpp"
#include "host_stage.hpp"

namespace slimamd {

// Device buffers of the scorers, grow-only: a second run of the same shape allocates nothing.
struct ScorerWorkspace {
  DeviceBuffer<uint32_t> split;            // chunk kernel: where every chunk starts in every model row
  DeviceBuffer<int32_t> queue, oid, ocnt;  // work queue; lists and their lengths (when they are wanted)
  DeviceBuffer<float> osc, score;          // list scores; wave kernel: score vectors
  DeviceBuffer<unsigned long long> disc;   // wave kernel: discovery vectors
  // rank mode: (key, score) of every test entry from the pre-pass, (rank, score) out
  DeviceBuffer<unsigned long long> tkey;
  DeviceBuffer<float> tscore, rscore;
  DeviceBuffer<int32_t> rank;
  // long lists: one slab of ncols (image, key, id) records per workgroup; the counters of slimgpu_list_stats_t
  DeviceBuffer<uint4> slab;
  DeviceBuffer<unsigned long long> lstats;
  int allocs = 0;                          // device allocations since the caller last cleared it
  template <class T>
  T* need(DeviceBuffer<T>& b, size_t n) {
    if (b.bytes() < sizeof(T) * (n ? n : 1)) ++allocs;
    return b.reserve(n);
  }
};

}  // namespace slimamd

// What an evaluation needs besides the model (slim_gpu_eval.h: SLIMGPU_EvalSetCreate).  Owns its buffers;
// borrows the matrix.
struct slimgpu_evalset {
  slimgpu_matrix_t* mat = nullptr;
  int device = 0;
  int32_t nsel = 0, fm_ncols = 0;  // positions evaluated: the listed users, or every user
  bool listed = false;             // d_users holds the user of every position (else position q is user q)
  slimamd::Cutoffs cut = {};       // list lengths; the lists scored have the last one's
  int64_t hist_entries = 0;  // history entries of the evaluated users: the model rows one evaluation streams
  int64_t max_hist = 0;      // the longest of those histories
  slimamd::StagedCsr tst;  // the test rows of the matrix's users (ids only)
  slimamd::DeviceBuffer<int32_t> d_fm, d_users;
  slimamd::DeviceBuffer<slimamd::UserTerms> d_terms;  // [cut.n][nsel]
  slimamd::DeviceBuffer<unsigned long long> d_out;    // EvalOut
  slimamd::ScorerWorkspace ws;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // ranks of the held-out items (slim_gpu_rank.h): the test entries of the evaluated users and the longest of
  // their test rows; where a position's entries start (listed users only: else the staged row pointer serves);
  // the workspaces of SLIMGPU_ModelEvaluateRanked, made on first use; the pre-pass's own events
  int64_t entries = 0, max_test = 0;
  slimamd::DeviceBuffer<int64_t> d_tbase;
  slimamd::DeviceBuffer<slimamd::UserTerms> d_rterms;  // [SLIMGPU_MAX_CUTOFFS][nsel]: one slice of cutoffs
  slimamd::DeviceBuffer<unsigned long long> d_rout;    // RankOut
  hipEvent_t evk0 = nullptr, evk1 = nullptr;
  ~slimgpu_evalset() {
    (void)hipSetDevice(device);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (evk0) (void)hipEventDestroy(evk0);
    if (evk1) (void)hipEventDestroy(evk1);
  }
};

namespace slimamd {

namespace {

constexpr unsigned long long kUntouched = ~0ull;
constexpr unsigned long long kExcluded = ~0ull - 1ull;

struct TopNArgs {
  int32_t nusers, nitems_rows, ncols, nrcmds;  // nusers: positions
  const int32_t* users = nullptr;  // the user of every position; nullptr: position q is user q
  const int64_t* wptr;
  const int32_t* wind;
  const float* wval;
  const int64_t* hptr;
  const int32_t* hind;
  const float* hval;  // nullptr: implicit ratings of 1
  float* score;                // [nwaves][ncols]
  unsigned long long* disc;    // [nwaves][ncols]
  int32_t* out_ids;
  float* out_scores;
  int32_t* out_cnt;
  int32_t* queue;
};

// a candidate is "better" when its score is higher, or equal with an earlier discovery
__device__ __forceinline__ bool better(float sa, unsigned long long da, float sb,
                                       unsigned long long db) {
  return sa > sb || (sa == sb && da < db);
}

__device__ __forceinline__ int64_t uni64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
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

    for (int k = lane; k < T.ncols; k += 64) disc[k] = kUntouched;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    // history items are never recommended (predict.c:35-38)
    for (int64_t h = h0 + lane; h < h1; h += 64) {
      const int i = T.hind[h];
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
// topn_kernel keeps the 12-byte-per-item score/discovery vectors of a user in HBM, so every
// multiply-add costs ~4 random sector requests: measured on a C4-shaped model (100K items,
// 2700 entries per row, histories of ~890 items) it is bound by the request rate at
// 14e9 adds/s = 5.8K users/s -- slower than the host scorer on a 128-core box.
//
// Here a workgroup of 8 wavefronts serves one user and the ITEMS are cut into chunks of CW ids
// whose score/discovery arrays live in LDS (12 bytes x CW per wavefront).  Wavefront w owns
// chunks w, w+8, ...; for each of its chunks it walks the user's history in order and, for
// history item i, only the entries of row i of W whose ids fall into the chunk -- rows are
// sorted, and wsplit[i][c] (built once per call) is where chunk c starts in row i.  Every
// candidate still receives its additions in history order, products and sums rounded
// separately, and the first touch still records (history index, position in the row), so the
// result is bit-identical to topn_kernel and to the host.  HBM sees each W entry once per
// user, in coalesced segments; everything else is LDS.
//   * the (start, length, rating) of up to 64 history items are fetched lane-parallel, then
//     consumed one item at a time through v_readlane; the segment loads run kT2Depth items
//     ahead of the LDS updates;
//   * selection: a wavefront keeps its N best in REGISTERS (lane t = rank t); a candidate that
//     beats the current N-th is inserted with one ballot + one lane shift; the 8 lists are
//     merged through LDS by wavefront 0.
constexpr int kT2Waves = 8;       // default workgroup: 8 wavefronts x 1536-id chunks
constexpr int kT2Depth = 16;
constexpr int kT2MaxN = 64;       // lists live one rank per lane: up to a wavefront's width
constexpr int kT2MaxCW = 1536;

struct TopN2Args {
  int32_t nusers, nitems_rows, ncols, nrcmds;  // nusers: positions pulled from the queue
  const int32_t* users = nullptr;  // the user of every position; nullptr: position q is user q
  int32_t cw, nchunks;
  uint32_t wlast;    // nnz(W) - 1 (0 for an empty model): clamp for the unconditional loads
  int32_t pos_bits;  // discovery key = history index << pos_bits | position in the row
  const int64_t* wptr;
  const int32_t* wind;
  const float* wval;
  const uint32_t* wsplit;  // [nitems_rows][nchunks + 1]: offset in row i of the first id >= c * cw
  const int64_t* hptr;
  const int32_t* hind;
  const float* hval;
  int32_t* out_ids;
  float* out_scores;
  int32_t* out_cnt;
  int32_t* queue;
  // fused evaluation (EVAL instantiations only): the test rows, the head / tail marker, one record per
  // cutoff and position (terms[k * nusers + q]); cut.c[cut.n - 1] == nrcmds
  const int64_t* tptr = nullptr;
  const int32_t* tind = nullptr;
  const int32_t* fmarker = nullptr;
  int32_t fm_ncols = 0;
  UserTerms* terms = nullptr;
  Cutoffs cut = {};
};

// rank mode (slim_gpu_rank.h): the scorer counts, for every test entry of the user, the candidates that stand
// before it.  (score, key) of the test entries come from k_test_keys, which ran before the scorer.
constexpr unsigned long long kNoCandidate = ~0ull;  // key of a test entry that is no candidate (every KeyT's kUnt)
struct TopNRankArgs : TopN2Args {
  const int64_t* tbase = nullptr;  // [nusers + 1]: where a position's test entries start in the arrays below
  const unsigned long long* tkey = nullptr;  // discovery key of every test entry, kNoCandidate: not a candidate
  const float* tscore = nullptr;
  int32_t* rank = nullptr;    // out: 1 + candidates ahead, 0: not a candidate
  float* rscore = nullptr;    // out: the entry's score, 0 when it is no candidate
  int32_t g0 = 0, gsize = 0;  // this pass serves entries [g0, g0 + gsize) of every test row
};

// long lists (slim_gpu_lists.h): the candidates of a user go to the workgroup's slab, a histogram over the
// leading bits of their order finds the N-th, the winners are put in order in LDS.
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

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long readlane_key(unsigned long long v, int l) { return readlane64(v, l); }
__device__ __forceinline__ uint32_t readlane_key(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ unsigned long long shfl_up_key(unsigned long long v) { return shfl_up64(v); }
__device__ __forceinline__ uint32_t shfl_up_key(uint32_t v) { return (uint32_t)__shfl_up((int)v, 1); }
template <typename KeyT>
__device__ __forceinline__ bool better(float sa, KeyT da, float sb, KeyT db) {
  return sa > sb || (sa == sb && da < db);
}

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

}  // namespace

bool rows_ascend_strictly(int num_cus, int32_t nrows, const int64_t* d_ptr, const int32_t* d_ind) {
  DeviceBuffer<int32_t> d_unsorted(1);
  HIP_TRY(hipMemset(d_unsorted.get(), 0, sizeof(int32_t)));
  hipLaunchKernelGGL(k_rows_sorted, dim3(std::max(1, std::min(nrows / 4 + 1, num_cus * 8))), dim3(256), 0, 0, nrows,
                     d_ptr, d_ind, d_unsorted.get());
  HIP_TRY(hipGetLastError());
  int32_t unsorted = 0;
  HIP_TRY(hipMemcpy(&unsorted, d_unsorted.get(), sizeof(int32_t), hipMemcpyDeviceToHost));
  return unsorted == 0;
}

namespace {

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
__global__ __launch_bounds__(256) void k_test_keys(int32_t nsel, const int32_t* __restrict__ users, int32_t wrows,
                                                   int32_t ncols, int32_t pos_bits, const int64_t* __restrict__ wptr,
                                                   const int32_t* __restrict__ wind, const float* __restrict__ wval,
                                                   const int64_t* __restrict__ hptr, const int32_t* __restrict__ hind,
                                                   const float* __restrict__ hval, const int64_t* __restrict__ tptr,
                                                   const int32_t* __restrict__ tind, const int64_t* __restrict__ tbase,
                                                   unsigned long long* __restrict__ tkey,
                                                   float* __restrict__ tscore) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t q = wave; q < nsel; q += nwaves) {
    const int32_t u = users ? users[q] : (int32_t)q;
    const int64_t h0 = hptr[u], h1 = hptr[u + 1];
    const int64_t t0 = tptr[u], t1 = tptr[u + 1];
    const int64_t out = tbase[q];
    for (int64_t z = t0; z < t1; ++z) {
      const int32_t t = tind[z];
      unsigned long long key = kNoCandidate;
      float acc = 0.0f;
      bool in_hist = false, touched = false;
      if (t >= 0 && t < ncols) {
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

// KeyT: discovery key (history index << pos_bits | position in the model row).  32 bits when
// the longest history and the longest model row allow it (8 bytes of LDS per item: chunks of
// 2304 ids), else 64.
// EVAL: the fused epilogue of the resident evaluation.  Once wavefront 0 has merged the lists, lane t
// holds rank t; the user's test row sits in LDS (loaded by the whole workgroup into wavefront 0's score
// chunk, which is free by then; what does not fit is walked from HBM), every lane tests its id against
// it, one ballot gives the hit mask, and the user's UserTerms records are formed exactly as k_user_terms
// (eval.hip) forms them -- gain added in rank order, ideal in test-row order, float accumulators fed with
// double terms; the set bits are walked once and the record of cutoff k leaves when the walk passes rank
// cut.c[k] (eval_terms.hpp: the additions behind a cutoff are a prefix of those behind the next one, so
// every record is the one a separate evaluation with lists of that length forms).  Lists are written only
// when an output pointer is given.
// RANK (Args = TopNRankArgs): no lists.  The merge area holds the user's test keys and one integer count per
// key; the candidate scan of a chunk adds to each count the chunk's slots that stand before the key (a ballot
// and a popcount per 64 slots, gathered in registers -- lane j owns key j -- and added to LDS once per chunk);
// after the chunks wavefront 0 writes rank = 1 + count.  Everything up to and including `update` is shared.
// LONG (Args = TopNLongArgs): lists of up to SLIMGPU_MAX_LIST.  No lists in registers and no merge: the
// candidate scan of a chunk appends the chunk's candidates to the workgroup's slab (a ballot and a popcount
// per 64 slots, one LDS atomic per wavefront step for the place) and counts the leading bits of their order in
// a histogram that lies where the merge area would; long_select picks and orders the list after the chunks,
// in the LDS of the chunks, which are free by then.
template <int NW, typename KeyT, bool EVAL, bool RANK = false, class Args = TopN2Args, bool LONG = false>
__device__ __forceinline__ void topn_chunk_body(const Args& T) {
  constexpr KeyT kUnt = ~KeyT(0), kExc = ~KeyT(0) - 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int D = kT2Depth;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = T.nrcmds, CW = T.cw;
  KeyT* disc = reinterpret_cast<KeyT*>(smem) + (size_t)wave * CW;
  float* score = reinterpret_cast<float*>(smem + (size_t)NW * CW * sizeof(KeyT)) + (size_t)wave * CW;
  char* marea = smem + (size_t)NW * CW * (sizeof(KeyT) + 4);
  float* m_s = reinterpret_cast<float*>(marea);
  KeyT* m_d = reinterpret_cast<KeyT*>(marea + NW * kT2MaxN * 4);
  int* m_id = reinterpret_cast<int*>(marea + NW * kT2MaxN * 12);
  int* m_cnt = reinterpret_cast<int*>(marea + NW * kT2MaxN * 16);
  __shared__ int s_user;

  for (;;) {
    if (tid == 0) s_user = atomicAdd(T.queue, 1);
    __syncthreads();
    // a position; the user is looked up once, outputs are indexed by the position (re-read from LDS after
    // the chunks, so that it does not occupy a scalar register through them)
    int u = __builtin_amdgcn_readfirstlane(s_user);
    if (u >= T.nusers) break;
    if (T.users) u = __builtin_amdgcn_readfirstlane(T.users[u]);
    uint32_t* l_hist = nullptr;
    int* l_ctl = nullptr;
    if constexpr (LONG) {
      if (!T.users) u += T.user0;
      l_hist = reinterpret_cast<uint32_t*>(smem + T.area);
      l_ctl = reinterpret_cast<int*>(l_hist + kLongBins);
      for (int z = tid; z < kLongBins; z += 64 * NW) l_hist[z] = 0;
      if (tid == 0) l_ctl[kLcAppended] = l_ctl[kLcWinners] = 0;
      __syncthreads();
    }
    const int64_t h0 = uni64(T.hptr[u]), h1 = uni64(T.hptr[u + 1]);

    // rank mode: the user's test keys of this pass into the merge area, counts zeroed
    float* r_s = reinterpret_cast<float*>(marea);
    KeyT* r_d = reinterpret_cast<KeyT*>(marea + NW * kT2MaxN * 4);
    int* r_c = reinterpret_cast<int*>(marea + NW * kT2MaxN * 12);
    int ng = 0;          // test entries of this user served by this pass
    int64_t rbase = 0;   // ... and where they start in the rank arrays
    if constexpr (RANK) {
      const int64_t tlen = uni64(T.tptr[u + 1]) - uni64(T.tptr[u]);
      const int64_t left = tlen - (int64_t)T.g0;
      ng = left < 0 ? 0 : (left < (int64_t)T.gsize ? (int)left : T.gsize);
      if (ng == 0 || h0 == h1) {  // nothing to count (an empty history: k_test_keys said "no candidate")
        rbase = uni64(T.tbase[__builtin_amdgcn_readfirstlane(s_user)]) + T.g0;
        for (int z = tid; z < ng; z += 64 * NW) {
          T.rank[rbase + z] = 0;
          T.rscore[rbase + z] = 0.0f;
        }
        __syncthreads();  // s_user is read: the next position may be drawn
        continue;
      }
      rbase = uni64(T.tbase[__builtin_amdgcn_readfirstlane(s_user)]) + T.g0;
      for (int z = tid; z < ng; z += 64 * NW) {
        r_s[z] = T.tscore[rbase + z];
        r_d[z] = (KeyT)T.tkey[rbase + z];
        r_c[z] = 0;
      }
      __syncthreads();
    }

    // this wavefront's N best so far: lane t holds rank t
    float ls = 0.0f;
    KeyT ld = kUnt;
    int lid = -1;
    int count = 0;
    float worst_s = 0.0f;
    KeyT worst_d = 0;
    auto insert = [&](const float cs, const KeyT cd, const int cid) {
      const bool ahead = lane < count && better(ls, ld, cs, cd);
      const int p = __popcll(__ballot(ahead));  // sorted list: the entries ahead are ranks 0..p-1
      const float us = __shfl_up(ls, 1);
      const KeyT ud = shfl_up_key(ld);
      const int uid = __shfl_up(lid, 1);
      if (lane > p && lane < N) {
        ls = us;
        ld = ud;
        lid = uid;
      }
      if (lane == p) {
        ls = cs;
        ld = cd;
        lid = cid;
      }
      if (count < N) ++count;
      if (count == N) {
        worst_s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ls), N - 1));
        worst_d = readlane_key(ld, N - 1);
      }
    };
    auto offer = [&](const float cs, const KeyT cd, const int cid) {
      if (count < N || better(cs, cd, worst_s, worst_d)) insert(cs, cd, cid);
    };

    for (int c = wave; c < T.nchunks; c += NW) {
      const int base = c * CW;
      const int width = (T.ncols - base) < CW ? (T.ncols - base) : CW;
      for (int k = lane; k < width; k += 64) disc[k] = kUnt;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      for (int64_t h = h0 + lane; h < h1; h += 64) {  // history items are never recommended
        const int i = T.hind[h];
        if (i >= base && i < base + width) disc[i - base] = kExc;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");

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

      if constexpr (RANK) {
        // candidates of this chunk against the user's test keys: integer adds, so any order
        for (int jb = 0; jb < ng; jb += 64) {
          const int nj = (ng - jb) < 64 ? (ng - jb) : 64;
          float my_ts = 0.0f;
          KeyT my_td = kUnt;
          if (lane < nj) {
            my_ts = r_s[jb + lane];
            my_td = r_d[jb + lane];
          }
          int my_cnt = 0;
          for (int kb = 0; kb < width; kb += 64) {
            const int k = kb + lane;
            KeyT d = kUnt;
            float sc = 0.0f;
            if (k < width) {
              d = disc[k];
              sc = score[k];
            }
            const bool cand = d < kExc;
            if (__ballot(cand) == 0) continue;
            for (int j = 0; j < nj; ++j) {
              const float ts = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_ts), j));
              const KeyT td = readlane_key(my_td, j);
              const int ahead = __popcll(__ballot(cand && better(sc, d, ts, td)));
              if (lane == j) my_cnt += ahead;
            }
          }
          if (lane < nj && my_cnt) atomicAdd(&r_c[jb + lane], my_cnt);
        }
      } else if constexpr (LONG) {
        // candidates of this chunk to the slab, their leading bits to the histogram
        uint4* slab = T.slab + (size_t)blockIdx.x * (size_t)T.ncols;
        for (int kb = 0; kb < width; kb += 64) {
          const int k = kb + lane;
          KeyT d = kUnt;
          float sc = 0.0f;
          if (k < width) {
            d = disc[k];
            sc = score[k];
          }
          const bool cand = d < kExc;
          const unsigned long long mask = __ballot(cand);
          if (mask == 0) continue;
          int at = 0;
          if (lane == 0) at = atomicAdd(&l_ctl[kLcAppended], __popcll(mask));
          at = __builtin_amdgcn_readfirstlane(at) + __popcll(mask & ((1ull << lane) - 1));
          if (cand) {  // (a user has at most ncols candidates: every slot of every chunk once)
            const uint32_t image = score_image(sc);
            const unsigned long long key = (unsigned long long)d;
            slab[at] = make_uint4(image, (uint32_t)(key >> 32), (uint32_t)key, (uint32_t)(base + k));
            atomicAdd(&l_hist[image >> 21], 1u);
          }
        }
      } else
      // candidates of this chunk against the wavefront's N best
      for (int kb = 0; kb < width; kb += 64) {
        const int k = kb + lane;
        KeyT d = kUnt;
        float sc = 0.0f;
        if (k < width) {
          d = disc[k];
          sc = score[k];
        }
        bool want = d < kExc;
        if (want && count == N) want = better(sc, d, worst_s, worst_d);
        unsigned long long mask = __ballot(want);
        while (mask) {
          const int l = __builtin_ctzll(mask);
          mask &= mask - 1;
          const float cs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sc), l));
          const KeyT cd = readlane_key(d, l);
          offer(cs, cd, base + kb + l);
        }
      }
    }

    if constexpr (RANK) {
      __syncthreads();  // every wavefront's counts are in
      if (wave == 0)
        for (int z = lane; z < ng; z += 64) {
          const bool cand = r_d[z] != kUnt;
          T.rank[rbase + z] = cand ? 1 + r_c[z] : 0;
          T.rscore[rbase + z] = cand ? r_s[z] : 0.0f;
        }
      __syncthreads();
      continue;
    }
    if constexpr (LONG) {
      __syncthreads();  // every wavefront's candidates are in the slab and in the histogram
      const int ncand = l_ctl[kLcAppended];
      long_select<NW>(T.slab + (size_t)blockIdx.x * (size_t)T.ncols, smem, l_hist, l_ctl, N, T.sort_cap, ncand,
                      T.out_ids, T.out_scores, T.out_cnt, (int64_t)__builtin_amdgcn_readfirstlane(s_user), T.stats);
      __syncthreads();
      continue;
    }
    // merge the wavefronts' lists (wavefront 0), write the user's row
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
    int* s_test = reinterpret_cast<int*>(smem + (size_t)NW * CW * sizeof(KeyT));
    if constexpr (EVAL) {
      t0 = uni64(T.tptr[u]);
      t1 = uni64(T.tptr[u + 1]);
      tl = (t1 - t0) < (int64_t)CW ? (int)(t1 - t0) : CW;
      for (int z = tid; z < tl; z += 64 * NW) s_test[z] = T.tind[t0 + z];
    }
    const int q = __builtin_amdgcn_readfirstlane(s_user);  // (unchanged until the barrier that ends this user)
    if (wave == 0) {
      for (int w = 1; w < NW; ++w) {
        const int cw_ = __builtin_amdgcn_readfirstlane(m_cnt[w]);
        for (int t = 0; t < cw_; ++t) {
          const float cs = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m_s[w * kT2MaxN + t])));
          const KeyT cd = readlane_key(m_d[w * kT2MaxN + t], 0);
          const int cid = __builtin_amdgcn_readfirstlane(m_id[w * kT2MaxN + t]);
          offer(cs, cd, cid);
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
    __syncthreads();
  }
}

template <int NW, typename KeyT>
__global__ __launch_bounds__(64 * NW) void topn_chunk_kernel(const TopN2Args T) {
  topn_chunk_body<NW, KeyT, false>(T);
}
template <int NW, typename KeyT>
__global__ __launch_bounds__(64 * NW) void topn_chunk_eval_kernel(const TopN2Args T) {
  topn_chunk_body<NW, KeyT, true>(T);
}
template <int NW, typename KeyT>
__global__ __launch_bounds__(64 * NW) void topn_chunk_rank_kernel(const TopNRankArgs T) {
  topn_chunk_body<NW, KeyT, false, true, TopNRankArgs>(T);
}
template <int NW, typename KeyT>
__global__ __launch_bounds__(64 * NW) void topn_chunk_long_kernel(const TopNLongArgs T) {
  topn_chunk_body<NW, KeyT, false, false, TopNLongArgs, true>(T);
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

// Geometry of the chunk kernel for a model / history pair: key width, chunk width, LDS.
struct ChunkPlan {
  bool key32 = false;
  int pos_bits = 32, item_bytes = 12, t2w = kT2Waves, cw = 64, nchunks = 1;
  size_t lds = 0;
};
// force_key64: the worst case of a model not seen yet (the smallest chunks, hence the largest split table)
ChunkPlan plan_chunks(int32_t ncols, int64_t max_row, int64_t max_hist, bool force_key64) {
  ChunkPlan P;
  if (const char* e = std::getenv("SLIM_TOPN_WAVES")) P.t2w = std::atoi(e) == 16 ? 16 : 8;
  const int t2w = P.t2w;
  // discovery keys: 32 bits when (longest history, longest model row) fit, else 64
  auto bits_for = [](int64_t v) { int b = 0; while ((int64_t(1) << b) <= v) ++b; return b; };
  P.key32 = !force_key64 && bits_for(max_row) + bits_for(max_hist) <= 31;
  if (const char* e = std::getenv("SLIM_TOPN_KEY")) P.key32 = P.key32 && std::atoi(e) != 64;
  P.pos_bits = P.key32 ? bits_for(max_row) : 32;
  P.item_bytes = P.key32 ? 8 : 12;
  // chunk width: round 1's footprint (1536 ids x 12 bytes x 8 wavefronts), less whatever the
  // merge area of this geometry needs beyond it, so that chunks + lists always fit the 160 KB
  const size_t merge_bytes = (size_t)t2w * kT2MaxN * 16 + (size_t)t2w * sizeof(int) + 256;
  const size_t chunk_bytes = std::min<size_t>((size_t)kT2MaxCW * 12 * kT2Waves,
                                              (size_t)160 * 1024 - merge_bytes);
  const int max_cw = (int)(chunk_bytes / ((size_t)P.item_bytes * t2w)) / 64 * 64;
  P.cw = std::max(64, std::min(max_cw, ((ncols + t2w - 1) / t2w + 63) / 64 * 64));
  if (const char* e = std::getenv("SLIM_TOPN_CW")) {
    const int v = std::atoi(e);
    if (v >= 64 && v <= max_cw && v % 64 == 0) P.cw = v;
  }
  P.nchunks = (ncols + P.cw - 1) / P.cw;
  P.lds = (size_t)t2w * P.cw * P.item_bytes + (size_t)t2w * kT2MaxN * 16 + t2w * sizeof(int);
  return P;
}
constexpr size_t kSplitLimit = size_t(2) << 30;  // bytes of split table beyond which the wave kernel serves

// ---- the launch path -----------------------------------------------------------------------------
//
// Every entry point describes its model (DeviceRowView) and its histories (HistoryView) and queues the
// scorer through queue_scorer: the kernel choice, the split table, the kernel arguments, LDS and grid
// exist here only.
struct HistoryView {
  int32_t nusers = 0;               // positions
  const int32_t* users = nullptr;   // the user of every position; nullptr: position q is user q
  const int64_t* ptr = nullptr;
  const int32_t* ind = nullptr;
  const float* val = nullptr;
  int64_t max_hist = 0;
  int32_t user0 = 0;                // long lists without a user list: position q is user user0 + q (a slice)
};
struct EvalTargets {  // the fused epilogue's inputs and output
  const int64_t* tptr;
  const int32_t* tind;
  const int32_t* fmarker;
  int32_t fm_ncols;
  UserTerms* terms;  // [cut.n][positions]
  Cutoffs cut;       // cut.c[cut.n - 1] == the nrcmds the scorer is queued with
};

struct RankTargets {  // the rank mode's inputs; the outputs are ws.rank / ws.rscore
  const int64_t* tptr;
  const int32_t* tind;
  const int64_t* tbase;    // [positions + 1]: where a position's test entries start
  int64_t entries;         // test entries of all positions
  int64_t max_test;        // the longest test row among them
  hipEvent_t pre0, pre1;   // around the pre-pass (k_test_keys)
};

int wave_kernel_waves(int32_t nusers, int32_t nrcmds, int num_cus, size_t* lds_out) {
  const size_t lds = (size_t)nrcmds * 64 * (sizeof(float) + sizeof(unsigned long long) + sizeof(int));
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (128 * 1024) / lds));
  if (lds_out) *lds_out = lds;
  return std::max(1, std::min<int>(nusers, num_cus * per_cu));
}

// which kernel serves: 1 the chunk kernel, 2 the wave kernel (lists of more than 64, a split table
// beyond 2 GB, model rows not sorted, SLIM_TOPN_KERNEL=wave).  With long_ok (a call that wants lists and may
// have them of any length up to SLIMGPU_MAX_LIST): 4, the chunk kernel's long-list form, above 128 and at
// any length under SLIM_TOPN_KERNEL=long -- where the chunk scorer can serve; 0 above 128 where it cannot.
int scorer_path(const DeviceRowView& W, int32_t nrcmds, const ChunkPlan& P, bool long_ok = false) {
  const char* kenv = std::getenv("SLIM_TOPN_KERNEL");
  const bool chunk_ok = W.nnz < (int64_t(1) << 31) && (W.rows_sorted || W.nnz == 0) &&
                        (size_t)std::max(W.nrows, 1) * ((size_t)P.nchunks + 1) * sizeof(uint32_t) <= kSplitLimit;
  if (long_ok && chunk_ok && (nrcmds > 128 || (kenv && std::strcmp(kenv, "long") == 0))) return 4;
  if (nrcmds > 128) return 0;
  const bool chunked = nrcmds <= kT2MaxN && chunk_ok && !(kenv && std::strcmp(kenv, "wave") == 0);
  return chunked ? 1 : 2;
}

// LDS of the long-list form: the chunks, or the winners and the sort area that take their place after the
// chunks, whichever is larger; then the histogram and the control words
int long_sort_cap() {
  int cap = kLongSortCap;
  if (const char* e = std::getenv("SLIM_TOPN_LONG_SORT")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= kLongMaxN) cap = v;
  }
  return cap;
}
size_t long_area_bytes(const ChunkPlan& P, int32_t nrcmds, int sort_cap) {
  auto p2 = [](size_t v) { size_t p = 1; while (p < v) p <<= 1; return p; };
  const size_t chunks = (size_t)P.t2w * P.cw * P.item_bytes;
  const size_t select = (p2((size_t)nrcmds) + p2((size_t)sort_cap)) * sizeof(uint4);
  return (std::max(chunks, select) + 15) / 16 * 16;
}
size_t long_lds_bytes(size_t area) { return area + kLongBins * sizeof(uint32_t) + kLcWords * sizeof(int); }
int long_groups(size_t lds, int t2w, int32_t nusers, int num_cus) {
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(32 / t2w, (160 * 1024) / (lds + 64)));
  return std::max(1, std::min<int>(nusers, num_cus * per_cu));
}

void reserve_scorer(ScorerWorkspace& ws, int path, int32_t wrows, int32_t ncols, const ChunkPlan& P, int32_t nusers,
                    int32_t nrcmds, int num_cus, bool lists) {
  ws.need(ws.queue, 2);
  if (path == 1 || path == 4) {
    ws.need(ws.split, (size_t)std::max(wrows, 1) * ((size_t)P.nchunks + 1));
  } else {
    const int nwaves = wave_kernel_waves(nusers, nrcmds, num_cus, nullptr);
    ws.need(ws.score, (size_t)nwaves * ncols);
    ws.need(ws.disc, (size_t)nwaves * ncols);
  }
  if (lists || path == 2) {
    ws.need(ws.oid, (size_t)nusers * nrcmds);
    ws.need(ws.osc, (size_t)nusers * nrcmds);
    ws.need(ws.ocnt, (size_t)nusers);
  }
}

// How queue_scorer served a call.
struct ScorerLaunch {
  int path = 0;    // scorer_path; 3: the chunk kernel in rank mode; 0: rank mode refused (set_error says why)
  int groups = 0;  // workgroups of the chunk kernel, wavefronts of the wave kernel
  ChunkPlan plan;  // the chunk kernel's geometry
  std::chrono::steady_clock::time_point launched;  // host time at which the scorer kernel itself was queued
};

// Queues the scorer on `stream`: lists into ws.oid / osc / ocnt when `lists` (always on path 2), the
// users' terms into ev->terms when ev is given.
// Rank mode (rk given; nrcmds, ev and lists are not used): the ranks and scores of the positions' test entries
// into ws.rank / ws.rscore.  Only the chunk kernel has a rank form.
// long_ok: lists of up to SLIMGPU_MAX_LIST may be asked for (scorer_path's 4; ws.lstats is the caller's to
// provide and to clear, it adds up over the slices of one call); path 0 with set_error where nothing serves.
ScorerLaunch queue_scorer(const DeviceRowView& W, const HistoryView& H, int32_t nrcmds, int num_cus,
                          hipStream_t stream, ScorerWorkspace& ws, const EvalTargets* ev, bool lists,
                          const RankTargets* rk = nullptr, bool long_ok = false) {
  const int32_t ncols = std::max(W.ncols, 1);
  const ChunkPlan P = plan_chunks(ncols, W.max_row, H.max_hist, false);
  if (rk) {
    nrcmds = 1;
    ev = nullptr;
    lists = false;
  }
  const int path = scorer_path(W, nrcmds, P, long_ok && lists && !ev && !rk);
  ScorerLaunch L;
  L.path = path;
  L.plan = P;
  if (path == 0) {
    set_error(!(W.rows_sorted || W.nnz == 0)
                  ? "lists of more than 128 need the chunk scorer: the model's rows do not ascend by id (row order)"
                  : "lists of more than 128 need the chunk scorer: fewer than 2^31 model entries, a split table of at "
                    "most 2 GB");
    return L;
  }
  if (rk && path != 1) {
    set_error("ranks of the held-out items need the chunk scorer: model rows ascending by id, fewer than 2^31 model "
              "entries, a split table of at most 2 GB" +
              std::string(std::getenv("SLIM_TOPN_KERNEL") ? " (SLIM_TOPN_KERNEL is set)" : ""));
    L.path = 0;
    return L;
  }
  reserve_scorer(ws, path, W.nrows, ncols, P, H.nusers, nrcmds, num_cus, lists);
  if (rk) {
    ws.need(ws.tkey, (size_t)rk->entries);
    ws.need(ws.tscore, (size_t)rk->entries);
    ws.need(ws.rank, (size_t)rk->entries);
    ws.need(ws.rscore, (size_t)rk->entries);
  }
  HIP_TRY(hipMemsetAsync(ws.queue.get(), 0, 2 * sizeof(int32_t), stream));
  if (lists || path == 2) HIP_TRY(hipMemsetAsync(ws.ocnt.get(), 0, sizeof(int32_t) * (size_t)H.nusers, stream));
  if (path == 1 || path == 4) {
    if (W.nrows > 0) {
      const int64_t total = (int64_t)W.nrows * (P.nchunks + 1);
      hipLaunchKernelGGL(k_row_split, dim3((unsigned)std::min<int64_t>((total + 255) / 256, num_cus * 16)), dim3(256),
                         0, stream, W.nrows, P.nchunks, P.cw, W.d_ptr, W.d_ind, ws.split.get());
      HIP_TRY(hipGetLastError());
    }
    TopNRankArgs T{};
    T.nusers = H.nusers;
    T.users = H.users;
    T.nitems_rows = W.nrows;
    T.ncols = ncols;
    T.nrcmds = nrcmds;
    T.cw = P.cw;
    T.nchunks = P.nchunks;
    T.pos_bits = P.pos_bits;
    T.wlast = W.nnz > 0 ? (uint32_t)(W.nnz - 1) : 0u;
    T.wptr = W.d_ptr; T.wind = W.d_ind; T.wval = W.d_val; T.wsplit = ws.split.get();
    T.hptr = H.ptr; T.hind = H.ind; T.hval = H.val;
    T.out_ids = lists ? ws.oid.get() : nullptr;
    T.out_scores = lists ? ws.osc.get() : nullptr;
    T.out_cnt = lists ? ws.ocnt.get() : nullptr;
    T.queue = ws.queue.get();
    if (ev) {
      T.tptr = ev->tptr; T.tind = ev->tind; T.fmarker = ev->fmarker; T.fm_ncols = ev->fm_ncols; T.terms = ev->terms;
      T.cut = ev->cut;
    }
    const bool w16 = P.t2w == 16;
    if (path == 4) {
      TopNLongArgs A{};
      static_cast<TopN2Args&>(A) = static_cast<const TopN2Args&>(T);
      A.sort_cap = long_sort_cap();
      A.area = (int32_t)long_area_bytes(P, nrcmds, A.sort_cap);
      const size_t lds = long_lds_bytes((size_t)A.area);
      const int nwg = long_groups(lds, P.t2w, H.nusers, num_cus);
      L.groups = nwg;
      A.slab = ws.need(ws.slab, (size_t)nwg * (size_t)ncols);
      A.stats = ws.lstats.get();
      A.user0 = H.user0;
      auto lfn = P.key32 ? (w16 ? topn_chunk_long_kernel<16, uint32_t> : topn_chunk_long_kernel<8, uint32_t>)
                         : (w16 ? topn_chunk_long_kernel<16, unsigned long long>
                                : topn_chunk_long_kernel<8, unsigned long long>);
      if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(lfn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
      L.launched = std::chrono::steady_clock::now();
      hipLaunchKernelGGL(lfn, dim3(nwg), dim3(64 * P.t2w), lds, stream, A);
      HIP_TRY(hipGetLastError());
      return L;
    }
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(32 / P.t2w, (160 * 1024) / (P.lds + 64)));
    const int nwg = std::max(1, std::min<int>(H.nusers, num_cus * per_cu));
    L.groups = nwg;
    if (rk) {
      L.path = 3;
      if (rk->entries <= 0) return L;  // (no test entry: nothing to rank)
      HIP_TRY(hipEventRecord(rk->pre0, stream));
      const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)H.nusers + 3) / 4, (int64_t)num_cus * 16));
      hipLaunchKernelGGL(k_test_keys, dim3(blocks), dim3(256), 0, stream, H.nusers, H.users, W.nrows, ncols, P.pos_bits,
                         W.d_ptr, W.d_ind, W.d_val, H.ptr, H.ind, H.val, rk->tptr, rk->tind, rk->tbase, ws.tkey.get(),
                         ws.tscore.get());
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(rk->pre1, stream));
      T.tptr = rk->tptr; T.tind = rk->tind; T.tbase = rk->tbase;
      T.tkey = ws.tkey.get(); T.tscore = ws.tscore.get(); T.rank = ws.rank.get(); T.rscore = ws.rscore.get();
      // a test row longer than the merge area holds keys for: one scoring pass per group of entries
      int group = P.t2w * kT2MaxN;
      if (const char* e = std::getenv("SLIM_TOPN_RANK_GROUP")) {
        const int v = std::atoi(e);
        if (v >= 1 && v < group) group = v;
      }
      T.gsize = group;
      auto rfn = P.key32 ? (w16 ? topn_chunk_rank_kernel<16, uint32_t> : topn_chunk_rank_kernel<8, uint32_t>)
                         : (w16 ? topn_chunk_rank_kernel<16, unsigned long long>
                                : topn_chunk_rank_kernel<8, unsigned long long>);
      if (P.lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(rfn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)P.lds));
      L.launched = std::chrono::steady_clock::now();
      for (int64_t g0 = 0; g0 < rk->max_test; g0 += group) {
        if (g0 > 0) HIP_TRY(hipMemsetAsync(ws.queue.get(), 0, 2 * sizeof(int32_t), stream));
        T.g0 = (int32_t)g0;
        hipLaunchKernelGGL(rfn, dim3(nwg), dim3(64 * P.t2w), P.lds, stream, T);
        HIP_TRY(hipGetLastError());
      }
      return L;
    }
    auto kfn = ev ? (P.key32 ? (w16 ? topn_chunk_eval_kernel<16, uint32_t> : topn_chunk_eval_kernel<8, uint32_t>)
                             : (w16 ? topn_chunk_eval_kernel<16, unsigned long long>
                                    : topn_chunk_eval_kernel<8, unsigned long long>))
                  : (P.key32 ? (w16 ? topn_chunk_kernel<16, uint32_t> : topn_chunk_kernel<8, uint32_t>)
                             : (w16 ? topn_chunk_kernel<16, unsigned long long>
                                    : topn_chunk_kernel<8, unsigned long long>));
    if (P.lds > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)P.lds));
    L.launched = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(kfn, dim3(nwg), dim3(64 * P.t2w), P.lds, stream, static_cast<const TopN2Args&>(T));
    HIP_TRY(hipGetLastError());
  } else {
    size_t lds = 0;
    const int nwaves = wave_kernel_waves(H.nusers, nrcmds, num_cus, &lds);
    TopNArgs T;
    T.nusers = H.nusers;
    T.users = H.users;
    T.nitems_rows = W.nrows;
    T.ncols = ncols;
    T.nrcmds = nrcmds;
    T.wptr = W.d_ptr; T.wind = W.d_ind; T.wval = W.d_val;
    T.hptr = H.ptr; T.hind = H.ind; T.hval = H.val;
    T.score = ws.score.get(); T.disc = ws.disc.get();
    T.out_ids = ws.oid.get(); T.out_scores = ws.osc.get(); T.out_cnt = ws.ocnt.get(); T.queue = ws.queue.get();
    if (lds > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(topn_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    L.groups = nwaves;
    L.launched = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(topn_kernel, dim3(nwaves), dim3(64), lds, stream, T);
    HIP_TRY(hipGetLastError());
    if (ev)
      launch_user_terms(stream, num_cus, H.nusers, H.users, nrcmds, ev->cut, ws.oid.get(), ws.ocnt.get(), ev->tptr,
                        ev->tind, ev->fmarker, ev->fm_ncols, ev->terms);
  }
  return L;
}

// Brings the lists of a scorer queued on `stream` down and copies the counts[u] entries of every user's
// list; the slots beyond a list stay as the caller filled them.  counts is optional.  Returns the bytes
// that came down.
size_t fetch_lists(const ScorerWorkspace& ws, int32_t nusers, int32_t nrcmds, hipStream_t stream, int32_t* output,
                   float* scores, int32_t* counts) {
  if (nusers <= 0) return 0;
  std::vector<int32_t> h_id((size_t)nusers * nrcmds), h_cnt((size_t)nusers);
  std::vector<float> h_sc((size_t)nusers * nrcmds);
  HIP_TRY(hipMemcpyAsync(h_id.data(), ws.oid.get(), sizeof(int32_t) * h_id.size(), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(h_sc.data(), ws.osc.get(), sizeof(float) * h_sc.size(), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(h_cnt.data(), ws.ocnt.get(), sizeof(int32_t) * h_cnt.size(), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int32_t u = 0; u < nusers; ++u) {
    for (int32_t r = 0; r < h_cnt[u]; ++r) {
      output[(int64_t)u * nrcmds + r] = h_id[(size_t)u * nrcmds + r];
      scores[(int64_t)u * nrcmds + r] = h_sc[(size_t)u * nrcmds + r];
    }
    if (counts) counts[u] = h_cnt[u];
  }
  return sizeof(int32_t) * (h_id.size() + h_cnt.size()) + sizeof(float) * h_sc.size();
}

double ms_since(const std::chrono::steady_clock::time_point& t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

thread_local slimgpu_list_stats_t g_list_stats;

// Users of one slice of a long-list call: the device lists of a slice (8 bytes per slot) stay under a quarter
// of the HBM that is free when the call begins.  SLIM_TOPN_LONG_SLICE=<users> forces a length.
int32_t long_slice_users(int32_t nusers, int32_t nrcmds) {
  if (const char* e = std::getenv("SLIM_TOPN_LONG_SLICE")) {
    const long v = std::atol(e);
    if (v >= 1) return (int32_t)std::min<long>(v, std::max(nusers, 1));
  }
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t per_user = (size_t)nrcmds * (sizeof(int32_t) + sizeof(float)) + sizeof(int32_t);
  return (int32_t)std::max<size_t>(1, std::min<size_t>((size_t)std::max(nusers, 1), free_b / 4 / per_user));
}

// The lists of every position of H through queue_scorer, brought down into output / scores / counts (counts
// may be null).  Up to 128 this is one launch on the chunk or the wave kernel, as ever.  On the long-list
// path the users go through in slices, each brought down before the next is queued, and the slab counters
// of all slices are added into g_list_stats.  Returns the path (0: refused, set_error says why); *down gets
// the bytes that came down.
int score_lists(const DeviceRowView& W, const HistoryView& H, int32_t nrcmds, int num_cus, hipStream_t stream,
                ScorerWorkspace& ws, int32_t* output, float* scores, int32_t* counts, ScorerLaunch* launch,
                size_t* down) {
  slimgpu_list_stats_t ls = {};
  const ChunkPlan P = plan_chunks(std::max(W.ncols, 1), W.max_row, H.max_hist, false);
  const int path = scorer_path(W, nrcmds, P, /*long_ok=*/true);
  size_t bytes = 0;
  if (path != 4) {
    const ScorerLaunch L = queue_scorer(W, H, nrcmds, num_cus, stream, ws, nullptr, /*lists=*/true, nullptr, true);
    if (launch) *launch = L;
    if (L.path == 0) return 0;
    bytes = fetch_lists(ws, H.nusers, nrcmds, stream, output, scores, counts);
    ls.path = L.path;
    ls.slices = 1;
  } else {
    ws.need(ws.lstats, 8);
    HIP_TRY(hipMemsetAsync(ws.lstats.get(), 0, 8 * sizeof(unsigned long long), stream));
    const int32_t step = long_slice_users(H.nusers, nrcmds);
    for (int32_t s0 = 0; s0 < H.nusers; s0 += step) {
      HistoryView S = H;
      S.nusers = std::min(step, H.nusers - s0);
      if (H.users) S.users = H.users + s0; else S.user0 = H.user0 + s0;
      const ScorerLaunch L = queue_scorer(W, S, nrcmds, num_cus, stream, ws, nullptr, /*lists=*/true, nullptr, true);
      if (launch && s0 == 0) *launch = L;
      if (L.path != 4) return 0;
      bytes += fetch_lists(ws, S.nusers, nrcmds, stream, output + (int64_t)s0 * nrcmds, scores + (int64_t)s0 * nrcmds,
                           counts ? counts + s0 : nullptr);
      ++ls.slices;
    }
    unsigned long long h[5] = {};
    HIP_TRY(hipMemcpyAsync(h, ws.lstats.get(), sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    bytes += sizeof(h);
    ls.path = 4;
    ls.candidates = (int64_t)h[0];
    ls.contenders = (int64_t)h[1];
    ls.refine_passes = (int64_t)h[2];
    ls.lds_sorts = (int64_t)h[3];
    ls.key_refines = (int64_t)h[4];
  }
  if (down) *down = bytes;
  g_list_stats = ls;
  return ls.path;
}

}  // namespace

slimgpu_list_stats_t& last_list_stats() { return g_list_stats; }

// Top-N lists of every history row.  output/scores are [nusers][nrcmds], slots beyond a
// user's list length are left as the caller filled them; counts (optional) = list lengths.
// W: its row view on the device -- uploaded by predict_device (host model), or where a resident model
// already holds it (nothing of W crosses PCIe).  The history is staged, the scorer queued on the null
// stream through queue_scorer, the lists brought down.  Only here, SLIM_TOPN_KERNEL=chunk is an error
// when the chunk kernel cannot serve (the resident entry points fall back to the wave kernel).
namespace {

// predict_device_view (long_ok false: lists of up to 128) and predict_lists_view (up to SLIMGPU_MAX_LIST)
int32_t predict_view_impl(const DeviceRowView& W, const slim_csr_t* hist, int32_t nrcmds, int32_t* output,
                          float* scores, int32_t* counts, bool long_ok) {
  const int32_t nusers = hist->nrows;
  const auto t_begin = std::chrono::steady_clock::now();
  try {
    (void)hipGetLastError();  // a failure of an earlier call must not be reported by this one
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw HipFail{hipErrorNoDevice, "hipGetDeviceCount"};
    if (W.device >= 0) HIP_TRY(hipSetDevice(W.device));
    const int num_cus = cu_count();
    const StagedCsr h = stage_csr(hist, nusers, /*values=*/true, /*stream=*/nullptr);
    HistoryView H;
    H.nusers = nusers;
    H.ptr = h.ptr.get(); H.ind = h.ind.get(); H.val = h.val.get();
    H.max_hist = h.max_row;
    DeviceRowView V = W;
    if (!V.rows_sorted && V.nnz > 0) V.rows_sorted = rows_ascend_strictly(num_cus, V.nrows, V.d_ptr, V.d_ind);
    const char* kenv = std::getenv("SLIM_TOPN_KERNEL");
    if (kenv && std::strcmp(kenv, "chunk") == 0 &&
        scorer_path(V, nrcmds, plan_chunks(std::max(V.ncols, 1), V.max_row, H.max_hist, false)) != 1) {
      set_error("SLIMGPU_Predict: SLIM_TOPN_KERNEL=chunk needs nrcmds <= 64 and model rows sorted by id");
      return SLIM_ERROR_INPUT;
    }
    ScorerWorkspace ws;
    if (long_ok) {
      if (score_lists(V, H, nrcmds, num_cus, /*stream=*/nullptr, ws, output, scores, counts, nullptr, nullptr) == 0) {
        set_error("SLIMGPU_PredictLists: " + std::string(last_error()));
        return SLIM_ERROR_INPUT;
      }
      return SLIM_OK;
    }
    const ScorerLaunch L =
        queue_scorer(V, H, nrcmds, num_cus, /*stream=*/nullptr, ws, /*ev=*/nullptr, /*lists=*/true);
    HIP_TRY(hipDeviceSynchronize());
    if (L.path == 1 && std::getenv("SLIM_GPU_TRACE"))
      std::fprintf(stderr, "[trace] top-N chunk kernel: %d users, %d workgroups of %d wavefronts, chunks of %d ids, "
                           "%d-bit keys: %.1f ms (upload + split table before it: %.1f ms)\n",
                   nusers, L.groups, L.plan.t2w, L.plan.cw, L.plan.key32 ? 32 : 64, ms_since(L.launched),
                   std::chrono::duration<double, std::milli>(L.launched - t_begin).count());
    fetch_lists(ws, nusers, nrcmds, nullptr, output, scores, counts);
    return SLIM_OK;
  } catch (const HipFail& e) {
    return hip_failure(long_ok ? "SLIMGPU_PredictLists" : "SLIMGPU_Predict", e);
  } catch (const std::bad_alloc&) {
    set_error(std::string(long_ok ? "SLIMGPU_PredictLists" : "SLIMGPU_Predict") + ": out of host memory");
    return SLIM_ERROR_MEMORY;
  }
}

int32_t predict_impl(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds, int32_t* output, float* scores,
                     int32_t* counts, bool long_ok);

}  // namespace

int32_t predict_device_view(const DeviceRowView& W, const slim_csr_t* hist, int32_t nrcmds,
                            int32_t* output, float* scores, int32_t* counts) {
  if (!hist || !hist->rowptr || !W.d_ptr || nrcmds < 1 || nrcmds > 128) {
    set_error("SLIMGPU_Predict: bad arguments (1 <= nrcmds <= 128)");
    return SLIM_ERROR_INPUT;
  }
  return predict_view_impl(W, hist, nrcmds, output, scores, counts, /*long_ok=*/false);
}

int32_t predict_lists_view(const DeviceRowView& W, const slim_csr_t* hist, int32_t nrcmds,
                           int32_t* output, float* scores, int32_t* counts) {
  if (!hist || !hist->rowptr || !W.d_ptr || !output || !scores || nrcmds < 1 || nrcmds > SLIMGPU_MAX_LIST) {
    set_error("SLIMGPU_PredictLists: bad arguments (a model, a history, output arrays, 1 <= nrcmds <= " +
              std::to_string(SLIMGPU_MAX_LIST) + ")");
    return SLIM_ERROR_INPUT;
  }
  return predict_view_impl(W, hist, nrcmds, output, scores, counts, /*long_ok=*/true);
}

int32_t predict_device(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds,
                       int32_t* output, float* scores, int32_t* counts) {
  if (!W || !hist || !W->rowptr || !hist->rowptr || (!W->rowval && W->rowptr[W->nrows] > 0) || nrcmds < 1 ||
      nrcmds > 128) {
    set_error("SLIMGPU_Predict: bad arguments (1 <= nrcmds <= 128)");
    return SLIM_ERROR_INPUT;
  }
  return predict_impl(W, hist, nrcmds, output, scores, counts, /*long_ok=*/false);
}

int32_t predict_lists(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds,
                      int32_t* output, float* scores, int32_t* counts) {
  if (!W || !hist || !W->rowptr || !hist->rowptr || (!W->rowval && W->rowptr[W->nrows] > 0) || !output || !scores ||
      nrcmds < 1 || nrcmds > SLIMGPU_MAX_LIST) {
    set_error("SLIMGPU_PredictLists: bad arguments (a model, a history, output arrays, 1 <= nrcmds <= " +
              std::to_string(SLIMGPU_MAX_LIST) + ")");
    return SLIM_ERROR_INPUT;
  }
  return predict_impl(W, hist, nrcmds, output, scores, counts, /*long_ok=*/true);
}

namespace {

int32_t predict_impl(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds, int32_t* output, float* scores,
                     int32_t* counts, bool long_ok) {
  try {
    (void)hipGetLastError();
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw HipFail{hipErrorNoDevice, "hipGetDeviceCount"};
    const StagedCsr w = stage_csr(W, W->nrows, /*values=*/true, /*stream=*/nullptr);
    DeviceRowView v;
    v.nrows = W->nrows;
    v.ncols = W->ncols;
    v.nnz = w.nnz;
    v.max_row = w.max_row;
    v.d_ptr = w.ptr.get();
    v.d_ind = w.ind.get();
    v.d_val = w.val.get();
    return predict_view_impl(v, hist, nrcmds, output, scores, counts, long_ok);
  } catch (const HipFail& e) {
    return hip_failure(long_ok ? "SLIMGPU_PredictLists" : "SLIMGPU_Predict", e);
  }
}

}  // namespace

// ---- a resident model against the resident matrix ----------------------------------------------
//
// The evaluate half of a model-selection cell without the host: the history is the staged matrix's CSR
// where it lies, the model is a resident model's row view, the test rows and the head / tail marker
// were staged once (slimgpu_evalset).  One fused kernel scores, selects and forms every user's terms;
// k_sum_in_user_order adds them; 8 + 32 bytes per cutoff come down.  The evaluated users are the matrix's
// first rows or a sorted list of them (positions, eval_terms.hpp); several list lengths are served by the
// one scoring pass of the longest.
namespace {

thread_local slimgpu_eval_stats_t g_eval_stats;

struct EvalOut {  // what one evaluation brings down: the first 8 + 32 * ncutoffs bytes
  unsigned long long streamed;  // entries of the model rows streamed
  EvalSums sums[SLIMGPU_MAX_CUTOFFS];
};

// the matrix and the model of one call: one device, one width, rows that are the caller's
int32_t check_pair(const char* who, const DeviceCsrView& R, const DeviceRowView& W) {
  if (R.merged) {
    set_error(std::string(who) + ": the matrix was staged with SLIM_GPU_DUPLICATES=sum and repeated pairs were "
              "merged: its rows are not the caller's, score through the host handle");
    return SLIM_ERROR_INPUT;
  }
  if (W.device != R.device) {
    set_error(std::string(who) + ": the model and the matrix live on different devices");
    return SLIM_ERROR_INPUT;
  }
  if (W.nrows != R.ncols) {
    set_error(std::string(who) + ": the model has " + std::to_string(W.nrows) + " items, the matrix " +
              std::to_string(R.ncols));
    return SLIM_ERROR_INPUT;
  }
  return SLIM_OK;
}

}  // namespace

slimgpu_eval_stats_t& last_eval_stats() { return g_eval_stats; }

void queue_row_facts(void* stream, int num_cus, int32_t nrows, const int64_t* d_ptr, const int32_t* d_ind,
                     int32_t* d_facts) {
  hipLaunchKernelGGL(k_row_facts, dim3(std::max(1, std::min((nrows + 255) / 256, num_cus * 8))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), nrows, d_ptr, d_ind, d_facts);
  HIP_TRY(hipGetLastError());
}

namespace {

// ranked: an eval set with no list length (SLIMGPU_EvalSetCreateRanked; ncutoffs == 0, cutoffs unused)
slimgpu_evalset_t* evalset_create_impl(slimgpu_matrix_t* mat, const slim_csr_t* tst, const int32_t* fmarker,
                                       int32_t fm_ncols, int32_t ncutoffs, const int32_t* cutoffs, int32_t nusers,
                                       const int32_t* users, int32_t* status, bool ranked) {
  auto fail = [&](int32_t st) {
    if (status) *status = st;
    return static_cast<slimgpu_evalset_t*>(nullptr);
  };
  auto refuse = [&](const std::string& what) {
    set_error("SLIMGPU_EvalSetCreate: " + what);
    return fail(SLIM_ERROR_INPUT);
  };
  DeviceCsrView R;
  if (!mat || !tst || !tst->rowptr || !fmarker || fm_ncols < 0 || (!cutoffs && !ranked))
    return refuse("bad arguments (a staged matrix, a test handle, a marker, the list lengths)");
  if (!ranked && (ncutoffs < 1 || ncutoffs > SLIMGPU_MAX_CUTOFFS))
    return refuse("between 1 and " + std::to_string(SLIMGPU_MAX_CUTOFFS) + " list lengths, not " + std::to_string(ncutoffs));
  Cutoffs cut = {};
  cut.n = ncutoffs;
  for (int32_t k = 0; k < ncutoffs; ++k) {
    if (cutoffs[k] < 1 || cutoffs[k] > 128)
      return refuse("bad arguments (1 <= nrcmds <= 128, not " + std::to_string(cutoffs[k]) + ")");
    if (k > 0 && cutoffs[k] <= cutoffs[k - 1]) return refuse("the list lengths must ascend strictly");
    cut.c[k] = cutoffs[k];
  }
  if (users ? nusers < 1 : nusers != 0)
    return refuse(users ? "a user list needs at least one user" : "nusers must be 0 without a user list");
  if (matrix_csr_view(mat, &R) != SLIM_OK) return refuse("bad arguments (a staged matrix)");
  if (R.merged)
    return refuse("the matrix was staged with SLIM_GPU_DUPLICATES=sum and repeated pairs were "
                  "merged: its rows are not the caller's, evaluate through the host handle");
  const int32_t nall = std::min(R.nrows, tst->nrows);  // pyapi.c:309
  for (int32_t q = 0; q < nusers; ++q) {
    if (users[q] < 0 || users[q] >= nall)
      return refuse("user " + std::to_string(users[q]) + " is outside [0, " + std::to_string(nall) + ")");
    if (q > 0 && users[q] <= users[q - 1]) return refuse("the user ids must ascend strictly");
  }
  const int32_t nrcmds = ranked ? 1 : cut.c[cut.n - 1];
  slimgpu_evalset* es = nullptr;
  try {
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(R.device));
    hipStream_t stream = static_cast<hipStream_t>(R.stream);
    es = new slimgpu_evalset();
    es->mat = mat;
    es->device = R.device;
    es->listed = users != nullptr;
    es->nsel = users ? nusers : nall;
    es->cut = cut;
    es->fm_ncols = fm_ncols;
    const int32_t nsel = es->nsel;
    es->tst = stage_csr(tst, nall, /*values=*/false, stream);
    es->d_fm = DeviceBuffer<int32_t>((size_t)fm_ncols);
    es->d_terms = DeviceBuffer<UserTerms>((size_t)cut.n * (size_t)nsel);
    es->d_out = DeviceBuffer<unsigned long long>(sizeof(EvalOut) / sizeof(unsigned long long));
    if (fm_ncols > 0)
      HIP_TRY(hipMemcpyAsync(es->d_fm.get(), fmarker, sizeof(int32_t) * (size_t)fm_ncols, hipMemcpyHostToDevice, stream));
    if (users) {  // (pageable source: the copy has left the caller's array when the call returns)
      es->d_users = DeviceBuffer<int32_t>((size_t)nsel);
      HIP_TRY(hipMemcpyAsync(es->d_users.get(), users, sizeof(int32_t) * (size_t)nsel, hipMemcpyHostToDevice, stream));
    }
    // the test entries of the evaluated users, the longest of their test rows and, for listed users, where
    // every position's entries start in the rank arrays (every user: the staged row pointer is that)
    std::vector<int64_t> h_tbase;
    if (users || tst->rowptr[0] != 0) {
      h_tbase.resize((size_t)nsel + 1);
      h_tbase[0] = 0;
      for (int32_t q = 0; q < nsel; ++q) {
        const int32_t u = users ? users[q] : q;
        const int64_t len = tst->rowptr[u + 1] - tst->rowptr[u];
        es->max_test = std::max(es->max_test, len);
        h_tbase[(size_t)q + 1] = h_tbase[(size_t)q] + len;
      }
      es->entries = h_tbase[(size_t)nsel];
      es->d_tbase = DeviceBuffer<int64_t>((size_t)nsel + 1);
      HIP_TRY(hipMemcpyAsync(es->d_tbase.get(), h_tbase.data(), sizeof(int64_t) * ((size_t)nsel + 1),
                             hipMemcpyHostToDevice, stream));  // (h_tbase outlives the synchronize below)
    } else {
      es->entries = es->tst.nnz;
      es->max_test = es->tst.max_row;
    }
    // the longest history of the evaluated users and the number of their history entries, once (the
    // scorer's key width needs the first)
    EvalOut* d_out = reinterpret_cast<EvalOut*>(es->d_out.get());
    int32_t* d_max = &d_out->sums[0].n[0];
    HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(EvalOut), stream));
    if (nsel > 0) {
      hipLaunchKernelGGL(k_longest_row, dim3(std::max(1, std::min((nsel + 255) / 256, R.num_cus * 8))), dim3(256), 0,
                         stream, nsel, static_cast<const int32_t*>(users ? es->d_users.get() : nullptr), R.d_ptr, d_max,
                         &d_out->streamed);
      HIP_TRY(hipGetLastError());
    }
    int32_t h_max = 0;
    unsigned long long h_total = 0;
    HIP_TRY(hipMemcpyAsync(&h_max, d_max, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&h_total, &d_out->streamed, sizeof(h_total), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    es->max_hist = h_max;
    es->hist_entries = (int64_t)h_total;
    // workspaces for the worst model: 64-bit keys, hence the smallest chunks and the largest split table
    DeviceRowView worst;
    worst.nrows = worst.ncols = R.ncols;
    worst.rows_sorted = true;
    const ChunkPlan P = plan_chunks(std::max(R.ncols, 1), 0, es->max_hist, /*force_key64=*/true);
    reserve_scorer(es->ws, scorer_path(worst, nrcmds, P), R.ncols, std::max(R.ncols, 1), P, nsel, nrcmds, R.num_cus,
                   /*lists=*/false);
    HIP_TRY(hipEventCreate(&es->ev0));
    HIP_TRY(hipEventCreate(&es->ev1));
    HIP_TRY(hipEventCreate(&es->evk0));
    HIP_TRY(hipEventCreate(&es->evk1));
    if (status) *status = SLIM_OK;
    return es;
  } catch (const HipFail& e) {
    delete es;
    return fail(hip_failure("SLIMGPU_EvalSetCreate", e));
  } catch (const std::bad_alloc&) {
    delete es;
    set_error("SLIMGPU_EvalSetCreate: out of host memory");
    return fail(SLIM_ERROR_MEMORY);
  }
}

}  // namespace

slimgpu_evalset_t* evalset_create(slimgpu_matrix_t* mat, const slim_csr_t* tst, const int32_t* fmarker,
                                  int32_t fm_ncols, int32_t ncutoffs, const int32_t* cutoffs, int32_t nusers,
                                  const int32_t* users, int32_t* status) {
  return evalset_create_impl(mat, tst, fmarker, fm_ncols, ncutoffs, cutoffs, nusers, users, status, /*ranked=*/false);
}

slimgpu_evalset_t* evalset_create_ranked(slimgpu_matrix_t* mat, const slim_csr_t* tst, const int32_t* fmarker,
                                         int32_t fm_ncols, int32_t nusers, const int32_t* users, int32_t* status) {
  return evalset_create_impl(mat, tst, fmarker, fm_ncols, 0, nullptr, nusers, users, status, /*ranked=*/true);
}

int64_t evalset_entries(const slimgpu_evalset_t* es) { return es ? es->entries : -1; }

void evalset_free(slimgpu_evalset_t* es) { delete es; }

int32_t evalset_cutoffs(const slimgpu_evalset_t* es) { return es ? es->cut.n : 0; }

int32_t model_evaluate(slimgpu_evalset_t* es, const slimgpu_model* model, int32_t ncutoffs, EvalResult* out) {
  DeviceRowView W;
  DeviceCsrView R;
  if (!es || !model || !out || model_row_view(model, &W) != SLIM_OK || matrix_csr_view(es->mat, &R) != SLIM_OK) {
    set_error("SLIMGPU_ModelEvaluate: needs an eval set and a resident model with a row view");
    return SLIM_ERROR_INPUT;
  }
  if (ncutoffs != es->cut.n || es->cut.n < 1) {
    set_error("SLIMGPU_ModelEvaluate: the eval set holds " + std::to_string(es->cut.n) + " list lengths, the call asks for " +
              std::to_string(ncutoffs));
    return SLIM_ERROR_INPUT;
  }
  if (const int32_t rc = check_pair("SLIMGPU_ModelEvaluate", R, W); rc != SLIM_OK) return rc;
  if (es->device != R.device) {
    set_error("SLIMGPU_ModelEvaluate: the eval set and the matrix live on different devices");
    return SLIM_ERROR_INPUT;
  }
  const int32_t ncut = es->cut.n;
  for (int32_t k = 0; k < ncut; ++k) out[k] = EvalResult();
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  try {
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(R.device));
    hipStream_t stream = static_cast<hipStream_t>(R.stream);
    es->ws.allocs = 0;
    EvalOut h = {};
    if (es->nsel > 0) {
      HistoryView H;
      H.nusers = es->nsel;
      H.users = es->listed ? es->d_users.get() : nullptr;
      H.ptr = R.d_ptr; H.ind = R.d_ind; H.val = R.d_val;
      H.max_hist = es->max_hist;
      const EvalTargets ev = {es->tst.ptr.get(), es->tst.ind.get(), es->d_fm.get(), es->fm_ncols, es->d_terms.get(), es->cut};
      EvalOut* d_out = reinterpret_cast<EvalOut*>(es->d_out.get());
      HIP_TRY(hipEventRecord(es->ev0, stream));
      st.path = queue_scorer(W, H, es->cut.c[ncut - 1], R.num_cus, stream, es->ws, &ev, /*lists=*/false).path;
      launch_sum_in_user_order(stream, es->nsel, ncut, es->d_terms.get(), d_out->sums);
      HIP_TRY(hipEventRecord(es->ev1, stream));
      HIP_TRY(hipMemsetAsync(&d_out->streamed, 0, sizeof(unsigned long long), stream));
      if (es->hist_entries > 0 && W.nnz > 0) {
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)es->nsel + 3) / 4, R.num_cus * 8));
        hipLaunchKernelGGL(k_streamed_entries, dim3(blocks), dim3(256), 0, stream, es->nsel, H.users, R.d_ptr, R.d_ind,
                           W.nrows, W.d_ptr, &d_out->streamed);
        HIP_TRY(hipGetLastError());
      }
      const size_t down = sizeof(unsigned long long) + sizeof(EvalSums) * (size_t)ncut;
      HIP_TRY(hipMemcpyAsync(&h, d_out, down, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      st.d2h_bytes = (int64_t)down;
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, es->ev0, es->ev1));
      st.kernel_ms = ms;
    }
    for (int32_t k = 0; k < ncut; ++k) {
      const EvalSums& s = h.sums[k];
      out[k].nvalid = s.n[0];
      out[k].nvalid_head = s.n[1];
      out[k].nvalid_tail = s.n[2];
      out[k].hr = s.n[0] > 0 ? s.f[0] / s.n[0] : 0;
      out[k].hr_head = s.n[1] > 0 ? s.f[1] / s.n[1] : 0;
      out[k].hr_tail = s.n[2] > 0 ? s.f[2] / s.n[2] : 0;
      out[k].arhr = s.n[0] > 0 ? s.f[3] / s.n[0] : 0;
    }
    st.device_allocs = es->ws.allocs;
    st.w_rows_read = es->hist_entries;
    st.w_bytes = 8.0 * (double)h.streamed;
    st.total_ms = ms_since(t_begin);
    g_eval_stats = st;
    return SLIM_OK;
  } catch (const HipFail& e) {
    return hip_failure("SLIMGPU_ModelEvaluate", e);
  }
}

// ---- the rank of every held-out item (slim_gpu_rank.h) ------------------------------------------
namespace {

thread_local double g_rank_prepass_ms = 0;

struct RankOut {  // what SLIMGPU_ModelEvaluateRanked brings down: the first 8 + 32 * ncutoffs bytes
  unsigned long long streamed;
  EvalSums sums[SLIMGPU_MAX_RANK_CUTOFFS];
};

// the checks both ranked calls share, then the scorer in rank mode on the matrix's stream: ranks and scores of
// the eval set's test entries are in es->ws.rank / rscore when the stream has run.  SLIM_OK or a refusal.
int32_t queue_ranks(const char* who, slimgpu_evalset_t* es, const slimgpu_model* model, DeviceRowView& W,
                    DeviceCsrView& R, HistoryView& H, slimgpu_eval_stats_t& st) {
  if (!es || !model || model_row_view(model, &W) != SLIM_OK || matrix_csr_view(es->mat, &R) != SLIM_OK) {
    set_error(std::string(who) + ": needs an eval set and a resident model with a row view");
    return SLIM_ERROR_INPUT;
  }
  if (const int32_t rc = check_pair(who, R, W); rc != SLIM_OK) return rc;
  if (es->device != R.device) {
    set_error(std::string(who) + ": the eval set and the matrix live on different devices");
    return SLIM_ERROR_INPUT;
  }
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(R.device));
  hipStream_t stream = static_cast<hipStream_t>(R.stream);
  es->ws.allocs = 0;
  g_rank_prepass_ms = 0;
  if (es->nsel <= 0) {
    st.path = 3;
    return SLIM_OK;
  }
  H.nusers = es->nsel;
  H.users = es->listed ? es->d_users.get() : nullptr;
  H.ptr = R.d_ptr; H.ind = R.d_ind; H.val = R.d_val;
  H.max_hist = es->max_hist;
  const RankTargets rk = {es->tst.ptr.get(), es->tst.ind.get(),
                          es->d_tbase.get() ? es->d_tbase.get() : es->tst.ptr.get(),
                          es->entries, es->max_test, es->evk0, es->evk1};
  HIP_TRY(hipEventRecord(es->ev0, stream));
  const ScorerLaunch L = queue_scorer(W, H, 1, R.num_cus, stream, es->ws, nullptr, false, &rk);
  if (L.path != 3) {
    set_error(std::string(who) + ": " + last_error());
    return SLIM_ERROR_INPUT;
  }
  st.path = 3;
  return SLIM_OK;
}

// after the stream has run: the times of the scorer (ev0 .. ev1) and of its pre-pass
void read_rank_times(slimgpu_evalset_t* es, slimgpu_eval_stats_t& st) {
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, es->ev0, es->ev1));
  st.kernel_ms = ms;
  if (es->entries > 0) {
    HIP_TRY(hipEventElapsedTime(&ms, es->evk0, es->evk1));
    g_rank_prepass_ms = ms;
  }
}

}  // namespace

double last_rank_prepass_ms() { return g_rank_prepass_ms; }

int32_t model_ranks(slimgpu_evalset_t* es, const slimgpu_model* model, int32_t* ranks, float* scores) {
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  try {
    DeviceRowView W;
    DeviceCsrView R;
    HistoryView H;
    if (const int32_t rc = queue_ranks("SLIMGPU_ModelRanks", es, model, W, R, H, st); rc != SLIM_OK) return rc;
    if (es->nsel > 0) {
      hipStream_t stream = static_cast<hipStream_t>(R.stream);
      HIP_TRY(hipEventRecord(es->ev1, stream));
      const size_t n = (size_t)es->entries;
      if (ranks && n) {
        HIP_TRY(hipMemcpyAsync(ranks, es->ws.rank.get(), sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
        st.d2h_bytes += (int64_t)(sizeof(int32_t) * n);
      }
      if (scores && n) {
        HIP_TRY(hipMemcpyAsync(scores, es->ws.rscore.get(), sizeof(float) * n, hipMemcpyDeviceToHost, stream));
        st.d2h_bytes += (int64_t)(sizeof(float) * n);
      }
      HIP_TRY(hipStreamSynchronize(stream));
      read_rank_times(es, st);
    }
    st.device_allocs = es->ws.allocs;
    st.w_rows_read = es->hist_entries;
    st.total_ms = ms_since(t_begin);
    g_eval_stats = st;
    return SLIM_OK;
  } catch (const HipFail& e) {
    return hip_failure("SLIMGPU_ModelRanks", e);
  }
}

int32_t model_evaluate_ranked(slimgpu_evalset_t* es, const slimgpu_model* model, int32_t ncutoffs,
                              const int32_t* cutoffs, EvalResult* out) {
  if (!cutoffs || !out || ncutoffs < 1 || ncutoffs > SLIMGPU_MAX_RANK_CUTOFFS) {
    set_error("SLIMGPU_ModelEvaluateRanked: between 1 and " + std::to_string(SLIMGPU_MAX_RANK_CUTOFFS) +
              " cutoffs, not " + std::to_string(ncutoffs));
    return SLIM_ERROR_INPUT;
  }
  for (int32_t k = 0; k < ncutoffs; ++k) {
    if (cutoffs[k] < 1) {
      set_error("SLIMGPU_ModelEvaluateRanked: a cutoff must be at least 1, not " + std::to_string(cutoffs[k]));
      return SLIM_ERROR_INPUT;
    }
    if (k > 0 && cutoffs[k] <= cutoffs[k - 1]) {
      set_error("SLIMGPU_ModelEvaluateRanked: the cutoffs must ascend strictly");
      return SLIM_ERROR_INPUT;
    }
    out[k] = EvalResult();
  }
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  try {
    DeviceRowView W;
    DeviceCsrView R;
    HistoryView H;
    if (const int32_t rc = queue_ranks("SLIMGPU_ModelEvaluateRanked", es, model, W, R, H, st); rc != SLIM_OK) return rc;
    RankOut h = {};
    if (es->nsel > 0) {
      hipStream_t stream = static_cast<hipStream_t>(R.stream);
      const size_t nterms = (size_t)SLIMGPU_MAX_CUTOFFS * (size_t)es->nsel;
      if (es->d_rterms.bytes() < sizeof(UserTerms) * nterms) ++es->ws.allocs;
      UserTerms* d_terms = es->d_rterms.reserve(nterms);
      if (!es->d_rout.get()) ++es->ws.allocs;
      RankOut* d_out = reinterpret_cast<RankOut*>(es->d_rout.reserve(sizeof(RankOut) / sizeof(unsigned long long)));
      // the terms workspace holds 8 records per position: the cutoffs in slices of SLIMGPU_MAX_CUTOFFS
      for (int32_t k0 = 0; k0 < ncutoffs; k0 += SLIMGPU_MAX_CUTOFFS) {
        Cutoffs cut = {};
        cut.n = std::min<int32_t>(SLIMGPU_MAX_CUTOFFS, ncutoffs - k0);
        for (int32_t k = 0; k < cut.n; ++k) cut.c[k] = cutoffs[k0 + k];
        launch_rank_terms(stream, R.num_cus, es->nsel, H.users, cut, es->ws.rank.get(),
                          es->d_tbase.get() ? es->d_tbase.get() : es->tst.ptr.get(), es->tst.ptr.get(),
                          es->tst.ind.get(), es->d_fm.get(), es->fm_ncols, d_terms);
        launch_sum_in_user_order(stream, es->nsel, cut.n, d_terms, d_out->sums + k0);
      }
      HIP_TRY(hipEventRecord(es->ev1, stream));
      HIP_TRY(hipMemsetAsync(&d_out->streamed, 0, sizeof(unsigned long long), stream));
      if (es->hist_entries > 0 && W.nnz > 0) {
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)es->nsel + 3) / 4, R.num_cus * 8));
        hipLaunchKernelGGL(k_streamed_entries, dim3(blocks), dim3(256), 0, stream, es->nsel, H.users, R.d_ptr, R.d_ind,
                           W.nrows, W.d_ptr, &d_out->streamed);
        HIP_TRY(hipGetLastError());
      }
      const size_t down = sizeof(unsigned long long) + sizeof(EvalSums) * (size_t)ncutoffs;
      HIP_TRY(hipMemcpyAsync(&h, d_out, down, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      st.d2h_bytes = (int64_t)down;
      read_rank_times(es, st);
    }
    for (int32_t k = 0; k < ncutoffs; ++k) {
      const EvalSums& s = h.sums[k];
      out[k].nvalid = s.n[0];
      out[k].nvalid_head = s.n[1];
      out[k].nvalid_tail = s.n[2];
      out[k].hr = s.n[0] > 0 ? s.f[0] / s.n[0] : 0;
      out[k].hr_head = s.n[1] > 0 ? s.f[1] / s.n[1] : 0;
      out[k].hr_tail = s.n[2] > 0 ? s.f[2] / s.n[2] : 0;
      out[k].arhr = s.n[0] > 0 ? s.f[3] / s.n[0] : 0;
    }
    st.device_allocs = es->ws.allocs;
    st.w_rows_read = es->hist_entries;
    st.w_bytes = 8.0 * (double)h.streamed;
    st.total_ms = ms_since(t_begin);
    g_eval_stats = st;
    return SLIM_OK;
  } catch (const HipFail& e) {
    return hip_failure("SLIMGPU_ModelEvaluateRanked", e);
  }
}

namespace {

// SLIMGPU_MatrixPredict (every row, lists of up to 128) and SLIMGPU_MatrixPredictLists (who names the caller)
int32_t matrix_predict_impl(const char* who, int32_t max_n, int32_t nrcmds, const slimgpu_model* model,
                            slimgpu_matrix_t* mat, int32_t nusers, const int32_t* users, int32_t* output,
                            float* scores, int32_t* counts) {
  DeviceRowView W;
  DeviceCsrView R;
  const bool long_ok = max_n > 128;
  if (!model || !mat || !output || !scores || nrcmds < 1 || nrcmds > max_n || model_row_view(model, &W) != SLIM_OK ||
      matrix_csr_view(mat, &R) != SLIM_OK) {
    set_error(std::string(who) + ": bad arguments (a resident model, a staged matrix, 1 <= nrcmds <= " +
              std::to_string(max_n) + ")");
    return SLIM_ERROR_INPUT;
  }
  if (users ? nusers < 1 : nusers != 0) {
    set_error(std::string(who) + (users ? ": a user list needs at least one user" : ": nusers must be 0 without a user list"));
    return SLIM_ERROR_INPUT;
  }
  for (int32_t q = 0; q < nusers; ++q) {
    if (users[q] < 0 || users[q] >= R.nrows) {
      set_error(std::string(who) + ": user " + std::to_string(users[q]) + " is outside [0, " + std::to_string(R.nrows) + ")");
      return SLIM_ERROR_INPUT;
    }
    if (q > 0 && users[q] <= users[q - 1]) {
      set_error(std::string(who) + ": the user ids must ascend strictly");
      return SLIM_ERROR_INPUT;
    }
  }
  if (const int32_t rc = check_pair(who, R, W); rc != SLIM_OK) return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int32_t rc = SLIM_OK;
  try {
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(R.device));
    hipStream_t stream = static_cast<hipStream_t>(R.stream);
    const int32_t nu = users ? nusers : R.nrows;
    if (nu > 0) {
      ScorerWorkspace ws;
      DeviceBuffer<int32_t> d_max(1), d_users;
      ++ws.allocs;
      if (users) {  // (pageable source: the copy has left the caller's array before the scorer is queued)
        d_users = DeviceBuffer<int32_t>((size_t)nu);
        ++ws.allocs;
        HIP_TRY(hipMemcpyAsync(d_users.get(), users, sizeof(int32_t) * (size_t)nu, hipMemcpyHostToDevice, stream));
      }
      HIP_TRY(hipMemsetAsync(d_max.get(), 0, sizeof(int32_t), stream));
      hipLaunchKernelGGL(k_longest_row, dim3(std::max(1, std::min((nu + 255) / 256, R.num_cus * 8))), dim3(256), 0,
                         stream, nu, static_cast<const int32_t*>(d_users.get()), R.d_ptr, d_max.get(),
                         static_cast<unsigned long long*>(nullptr));
      HIP_TRY(hipGetLastError());
      int32_t h_max = 0;
      HIP_TRY(hipMemcpyAsync(&h_max, d_max.get(), sizeof(int32_t), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      HistoryView H;
      H.nusers = nu;
      H.users = d_users.get();
      H.ptr = R.d_ptr; H.ind = R.d_ind; H.val = R.d_val;
      H.max_hist = h_max;
      HIP_TRY(hipEventCreate(&ev0));
      HIP_TRY(hipEventCreate(&ev1));
      HIP_TRY(hipEventRecord(ev0, stream));
      if (long_ok) {  // (kernel_ms then spans the slices and their copies)
        size_t down = 0;
        st.path = score_lists(W, H, nrcmds, R.num_cus, stream, ws, output, scores, counts, nullptr, &down);
        if (st.path == 0) {
          set_error(std::string(who) + ": " + std::string(last_error()));
          rc = SLIM_ERROR_INPUT;
        }
        HIP_TRY(hipEventRecord(ev1, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        st.d2h_bytes = (int64_t)(down + sizeof(int32_t));
      } else {
      st.path = queue_scorer(W, H, nrcmds, R.num_cus, stream, ws, nullptr, /*lists=*/true).path;
      HIP_TRY(hipEventRecord(ev1, stream));
      // only the lists come down (and the longest history's length before them)
      st.d2h_bytes = (int64_t)(fetch_lists(ws, nu, nrcmds, stream, output, scores, nullptr) + sizeof(int32_t));
      }
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
      st.kernel_ms = ms;
      st.device_allocs = ws.allocs;
      st.w_rows_read = R.nnz;
    }
    st.total_ms = ms_since(t_begin);
    if (rc == SLIM_OK) g_eval_stats = st;
    if (rc == SLIM_OK && long_ok && nu <= 0) {
      g_list_stats = slimgpu_list_stats_t{};
    }
  } catch (const HipFail& e) {
    rc = hip_failure(who, e);
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    rc = SLIM_ERROR_MEMORY;
  }
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  return rc;
}

}  // namespace

int32_t matrix_predict(int32_t nrcmds, const slimgpu_model* model, slimgpu_matrix_t* mat, int32_t* output,
                       float* scores) {
  return matrix_predict_impl("SLIMGPU_MatrixPredict", 128, nrcmds, model, mat, 0, nullptr, output, scores, nullptr);
}

int32_t matrix_predict_lists(int32_t nrcmds, const slimgpu_model* model, slimgpu_matrix_t* mat, int32_t nusers,
                             const int32_t* users, int32_t* output, float* scores, int32_t* counts) {
  return matrix_predict_impl("SLIMGPU_MatrixPredictLists", SLIMGPU_MAX_LIST, nrcmds, model, mat, nusers, users, output,
                             scores, counts);
}

}  // namespace slimamd
