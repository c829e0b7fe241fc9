// cand_sample.hip -- the device sampler of slim_gpu_sample.h: the candidate set of the 1-vs-k protocol made where the
// matrix and the test rows lie.  k_sample_negatives draws every selected user's negatives (one wavefront per user),
// k_sample_rowlen and a scan give the row pointer, k_sample_rows writes "negatives, then the test row" into the
// set's device copy, and candset_adopt (candidates.hip) indexes those rows as it indexes uploaded ones.  The host
// learns the row pointer only.  The draws are those of host_csr.cpp: sample_candidates_host, bit for bit; both read
// sample_mix64 & co. from host_csr.hpp, and include/slim_gpu_sample.h states the rule.
// k_sample_weighted draws under the weighted rule of the same header (negatives in proportion to a weight per item)
// and shares every other pass.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <optional>
#include <string>
#include <vector>

#include "call_frame.hpp"
#include "host_csr.hpp"

namespace slimamd {
namespace {
struct SampleArgs {
  int32_t nsel, ncols, nnegs;
  uint64_t seed;
  const int32_t* users;  // the user of every position; nullptr: position q is user q
  const int64_t* hptr; const int32_t* hind;
  const int64_t* tptr; const int32_t* tind;
  int32_t* negs;         // [nsel][nnegs]: the negatives of a position, in order
  int32_t* nneg;         // [nsel]: how many
  int32_t rec_offset;    // LDS: where the dense rule's sort records start
  int32_t rec_cap;       // how many of them there are (a power of two >= nnegs; 0: no user can be dense)
};

__device__ __forceinline__ bool bit_of(const uint32_t* bm, const int id) { return (bm[id >> 5] >> (id & 31)) & 1u; }
// sets the bit of an id inside [0, ncols); 1 when it was clear
__device__ __forceinline__ int mark_id(uint32_t* bm, const int id, const int ncols) {
  if ((uint32_t)id >= (uint32_t)ncols) return 0;
  const uint32_t bit = 1u << (id & 31);
  return (atomicOr(&bm[id >> 5], bit) & bit) ? 0 : 1;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Bitonic sort of n = 2^k records (key high, key low, id) in LDS, ascending, by one wavefront; ends on a barrier.
// (long_sort of topn_kernels.hpp for a workgroup of one wavefront: that header is topn.hip's alone.)
__device__ __forceinline__ bool rec_before(const uint4 a, const uint4 b) {
  return a.x < b.x || (a.x == b.x && (a.y < b.y || (a.y == b.y && a.z < b.z)));
}
__device__ __forceinline__ void sample_sort(uint4* rec, const int n) {
  const int lane = threadIdx.x;
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (n >> 1); t += 64) {
        const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
        const bool up = (lo & k) == 0;
        const uint4 a = rec[lo], b = rec[hi];
        if (rec_before(b, a) == up) {
          rec[lo] = b;
          rec[hi] = a;
        }
      }
      __syncthreads();
    }
}

// One wavefront (a workgroup of 64) per position.  LDS: one bit per item -- X_u and the accepted ids, which serves
// exclusion and de-duplication at once and is cleared by un-marking what was marked --, the accepted ids in order,
// and, when some user may fall under the dense rule, the records its sort needs.
__global__ __launch_bounds__(64) void k_sample_negatives(const SampleArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* bm = reinterpret_cast<uint32_t*>(smem);
  const int ncols = A.ncols, nnegs = A.nnegs;
  const int nwords = (ncols + 31) >> 5;
  int32_t* acc = reinterpret_cast<int32_t*>(bm + nwords);
  uint4* rec = reinterpret_cast<uint4*>(smem + A.rec_offset);
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;  // the lanes before this one
  for (int w = lane; w < nwords; w += 64) bm[w] = 0u;
  __syncthreads();
  for (int q = (int)blockIdx.x; q < A.nsel; q += (int)gridDim.x) {
    const int u = A.users ? A.users[q] : q;
    const int64_t t0 = A.tptr[u], t1 = A.tptr[u + 1];
    if (t1 <= t0) {  // (no held-out item: an empty row)
      if (lane == 0) A.nneg[q] = 0;
      continue;
    }
    const int64_t h0 = A.hptr[u], h1 = A.hptr[u + 1];
    int fresh = 0;
    for (int64_t e = h0 + lane; e < h1; e += 64) fresh += mark_id(bm, A.hind[e], ncols);
    for (int64_t e = t0 + lane; e < t1; e += 64) fresh += mark_id(bm, A.tind[e], ncols);
    const int E = wave_sum(fresh);
    __syncthreads();
    const uint64_t base = sample_base(A.seed, (uint64_t)u);
    int got = 0;
    const bool sparse = 2 * ((int64_t)E + nnegs) <= (int64_t)ncols;
    if (sparse) {
      const int stop = 16 * nnegs + 1024;  // the guard: the loop is bounded
      for (int d0 = 0; d0 < stop && got < nnegs; d0 += 64) {
        const int d = d0 + lane;
        const int id = (int)sample_item(sample_key(base, (uint64_t)d), (uint32_t)ncols);
        const bool cand = d < stop && !bit_of(bm, id);
        // of equal draws in this batch the lowest lane is the first occurrence
        bool dup = false;
        unsigned long long rem = __ballot(cand);
        while (rem) {
          const int first = __ffsll((long long)rem) - 1;
          const int v = __shfl(id, first);
          const bool mine = cand && id == v;
          if (mine && lane != first) dup = true;
          rem &= ~__ballot(mine);
        }
        const bool ok = cand && !dup;
        const unsigned long long okmask = __ballot(ok);
        const int pos = got + __popcll(okmask & below);
        if (ok && pos < nnegs) {  // (the last batch is cut at nnegs)
          acc[pos] = id;
          atomicOr(&bm[id >> 5], 1u << (id & 31));
        }
        got = min(nnegs, got + __popcll(okmask));
        __syncthreads();
      }
    } else if (A.rec_cap > 0) {
      // the m eligible ids with the smallest (key, id): the m-th smallest key bit by bit, then one collecting pass
      const int m = min(nnegs, ncols - E);
      uint64_t T = 0;
      int k = m;  // ends as: how many of the ids whose key is T belong to the m
      for (int b = 63; b >= 0 && m > 0; --b) {
        int c = 0;
        for (int i = lane; i < ncols; i += 64)
          if (!bit_of(bm, i) && (sample_key(base, (uint64_t)i) >> b) == (T >> b)) ++c;
        c = wave_sum(c);
        if (k > c) {
          k -= c;
          T |= 1ull << b;
        }
      }
      int n = 0, eqseen = 0;
      for (int i0 = 0; i0 < ncols && m > 0; i0 += 64) {
        const int i = i0 + lane;
        const bool elig = i < ncols && !bit_of(bm, i);
        const uint64_t key = elig ? sample_key(base, (uint64_t)i) : 0;
        const bool eq = elig && key == T;
        const unsigned long long eqmask = __ballot(eq);
        const bool take = (elig && key < T) || (eq && eqseen + __popcll(eqmask & below) < k);
        const unsigned long long tmask = __ballot(take);
        const int pos = n + __popcll(tmask & below);
        if (take && pos < A.rec_cap) rec[pos] = make_uint4((uint32_t)(key >> 32), (uint32_t)key, (uint32_t)i, 0u);
        n += __popcll(tmask);
        eqseen += __popcll(eqmask);
      }
      n = min(n, A.rec_cap);
      int p2 = 1;
      while (p2 < n) p2 <<= 1;
      for (int j = n + lane; j < p2; j += 64) rec[j] = make_uint4(~0u, ~0u, ~0u, ~0u);
      __syncthreads();
      if (n > 0) sample_sort(rec, p2);  // (key, id) ascending
      for (int j = lane; j < n; j += 64) acc[j] = (int32_t)rec[j].z;
      got = n;
      __syncthreads();
    }
    for (int j = lane; j < got; j += 64) A.negs[(int64_t)q * nnegs + j] = acc[j];
    if (lane == 0) A.nneg[q] = got;
    // un-mark: whole words go to 0, which is what every one of them was
    for (int64_t e = h0 + lane; e < h1; e += 64) {
      const int id = A.hind[e];
      if ((uint32_t)id < (uint32_t)ncols) bm[id >> 5] = 0u;
    }
    for (int64_t e = t0 + lane; e < t1; e += 64) {
      const int id = A.tind[e];
      if ((uint32_t)id < (uint32_t)ncols) bm[id >> 5] = 0u;
    }
    if (sparse)
      for (int j = lane; j < got; j += 64) bm[acc[j] >> 5] = 0u;
    __syncthreads();
  }
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
  for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off);
  return v;
}
// inclusive sums over the lanes of a wavefront, lane order
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, const int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, off);
    if (lane >= off) v += t;
  }
  return v;
}

// The weighted rule (slim_gpu_sample.h), one wavefront per position.  C[0 .. ncols] is the prefix table of the weights
// in HBM (T = C[ncols] > 0).  LDS: the bitmap and the accepted ids of k_sample_negatives and, from rec_offset on, the
// remaining mass of every block of 1024 items (64-bit sums), which phase 2 forms once per user that reaches it.
// Phase 1 is the sparse loop with another draw: 64 draws a batch, every lane hashes, multiplies and searches C.
// Entering phase 2 reads all of C once for the user, to form the block sums; after that a pick scans the block sums,
// then the 1024 items of one block -- not the catalogue again.  Every loop is
// bounded by the draw guard, by nnegs or by the block counts.
__global__ __launch_bounds__(64) void k_sample_weighted(const SampleArgs A, const uint64_t* __restrict__ C,
                                                        const uint64_t T) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* bm = reinterpret_cast<uint32_t*>(smem);
  const int ncols = A.ncols, nnegs = A.nnegs;
  const int nwords = (ncols + 31) >> 5;
  int32_t* acc = reinterpret_cast<int32_t*>(bm + nwords);
  uint64_t* bs = reinterpret_cast<uint64_t*>(smem + A.rec_offset);
  const int nblk = (ncols + 1023) >> 10;
  const int per = (nblk + 63) >> 6;  // blocks per lane when a pick scans the block sums
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int stop = 16 * nnegs + 1024;  // D, the draw guard
  for (int w = lane; w < nwords; w += 64) bm[w] = 0u;
  __syncthreads();
  for (int q = (int)blockIdx.x; q < A.nsel; q += (int)gridDim.x) {
    const int u = A.users ? A.users[q] : q;
    const int64_t t0 = A.tptr[u], t1 = A.tptr[u + 1];
    if (t1 <= t0) {  // (no held-out item: an empty row)
      if (lane == 0) A.nneg[q] = 0;
      continue;
    }
    const int64_t h0 = A.hptr[u], h1 = A.hptr[u + 1];
    for (int64_t e = h0 + lane; e < h1; e += 64) mark_id(bm, A.hind[e], ncols);
    for (int64_t e = t0 + lane; e < t1; e += 64) mark_id(bm, A.tind[e], ncols);
    __syncthreads();
    const uint64_t base = sample_base(A.seed, (uint64_t)u);
    int got = 0;
    // phase 1: draws from the full weights; what is taken is rejected
    for (int d0 = 0; d0 < stop && got < nnegs; d0 += 64) {
      const int d = d0 + lane;
      const int id = d < stop ? sample_search(C, ncols, sample_mulhi64(sample_key(base, (uint64_t)d), T)) : 0;
      const bool cand = d < stop && !bit_of(bm, id);
      // of equal draws in this batch the lowest lane is the first occurrence
      bool dup = false;
      unsigned long long rem = __ballot(cand);
      while (rem) {
        const int first = __ffsll((long long)rem) - 1;
        const int v = __shfl(id, first);
        const bool mine = cand && id == v;
        if (mine && lane != first) dup = true;
        rem &= ~__ballot(mine);
      }
      const bool ok = cand && !dup;
      const unsigned long long okmask = __ballot(ok);
      const int pos = got + __popcll(okmask & below);
      if (ok && pos < nnegs) {  // (the last batch is cut at nnegs)
        acc[pos] = id;
        atomicOr(&bm[id >> 5], 1u << (id & 31));
      }
      got = min(nnegs, got + __popcll(okmask));
      __syncthreads();
    }
    if (got < nnegs) {
      // phase 2: the same distribution over what is left.  left = the mass of F; an item's mass is its weight while
      // its bit is clear.  The loop ends at nnegs or when F is empty (every item of F has a positive weight).
      uint64_t left = 0;
      for (int b = 0; b < nblk; ++b) {
        uint64_t m = 0;
        for (int k = 0; k < 16; ++k) {
          const int i = (b << 10) + (k << 6) + lane;
          if (i < ncols && !bit_of(bm, i)) m += C[i + 1] - C[i];
        }
        m = wave_sum64(m);
        if (lane == 0) bs[b] = m;
        left += m;
      }
      __syncthreads();
      for (int j = 0; got < nnegs && left > 0; ++j) {
        const uint64_t r = sample_mulhi64(sample_key(base, (uint64_t)stop + (uint64_t)j), left);  // r < left
        // the block at which the running sum first exceeds r: lane l holds blocks [l * per, (l + 1) * per)
        uint64_t mine = 0;
        for (int k = 0; k < per; ++k) {
          const int b = lane * per + k;
          if (b < nblk) mine += bs[b];
        }
        const uint64_t incl = wave_scan64(mine, lane);
        const unsigned long long over = __ballot(incl > r);
        if (over == 0) break;  // (the sums are left's: not reached)
        const int fl = __ffsll((long long)over) - 1;
        uint64_t before = (uint64_t)__shfl((unsigned long long)(incl - mine), fl);
        int b = fl * per;
        for (int k = 1; k < per && b + 1 < nblk; ++k) {  // (the last of the lane's blocks is the one if no earlier is)
          const uint64_t s = bs[b];
          if (before + s > r) break;
          before += s;
          ++b;
        }
        // the item inside the block, in id order: lane l holds the 16 items from (b << 10) + 16 * l
        const uint64_t r2 = r - before;
        const int i0 = (b << 10) + (lane << 4);
        uint32_t wt[16];
        uint64_t msum = 0;
        uint64_t prev = C[min(i0, ncols)];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int i = i0 + k;
          const uint64_t next = C[min(i + 1, ncols)];
          wt[k] = (i < ncols && !bit_of(bm, i)) ? (uint32_t)(next - prev) : 0u;
          msum += wt[k];
          prev = next;
        }
        const uint64_t incl2 = wave_scan64(msum, lane);
        const unsigned long long over2 = __ballot(incl2 > r2);
        if (over2 == 0) break;  // (bs[b] is the block's mass: not reached)
        const int fl2 = __ffsll((long long)over2) - 1;
        uint64_t run = incl2 - msum;
        int found = -1;
        uint32_t wf = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          run += wt[k];
          if (found < 0 && run > r2) {
            found = k;
            wf = wt[k];
          }
        }
        const int id = __shfl(i0 + found, fl2);
        const uint32_t wid = (uint32_t)__shfl((int)wf, fl2);
        if (lane == 0) {
          acc[got] = id;
          bm[id >> 5] |= 1u << (id & 31);
          bs[b] -= wid;
        }
        left -= wid;
        ++got;
        __syncthreads();
      }
    }
    for (int j = lane; j < got; j += 64) A.negs[(int64_t)q * nnegs + j] = acc[j];
    if (lane == 0) A.nneg[q] = got;
    // un-mark: whole words go to 0, which is what every one of them was
    for (int64_t e = h0 + lane; e < h1; e += 64) {
      const int id = A.hind[e];
      if ((uint32_t)id < (uint32_t)ncols) bm[id >> 5] = 0u;
    }
    for (int64_t e = t0 + lane; e < t1; e += 64) {
      const int id = A.tind[e];
      if ((uint32_t)id < (uint32_t)ncols) bm[id >> 5] = 0u;
    }
    for (int j = lane; j < got; j += 64) bm[acc[j] >> 5] = 0u;
    __syncthreads();
  }
}

// len[u + 1] = entries of user u's row (len is preset to 0: the rows of users not selected are empty)
__global__ void k_sample_rowlen(int32_t nsel, const int32_t* __restrict__ users, const int64_t* __restrict__ tptr,
                                const int32_t* __restrict__ nneg, int64_t* __restrict__ len) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nsel; q += (int64_t)gridDim.x * blockDim.x) {
    const int32_t u = users ? users[q] : (int32_t)q;
    const int64_t tl = tptr[u + 1] - tptr[u];
    len[(int64_t)u + 1] = tl > 0 ? nneg[q] + tl : 0;
  }
}

// the rows: the negatives, then the test row as staged.  One wavefront per position.
__global__ void k_sample_rows(int32_t nsel, const int32_t* __restrict__ users, int32_t nnegs,
                              const int32_t* __restrict__ negs, const int32_t* __restrict__ nneg,
                              const int64_t* __restrict__ tptr, const int32_t* __restrict__ tind,
                              const int64_t* __restrict__ cptr, int32_t* __restrict__ cind) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t q = wave; q < nsel; q += nwaves) {
    const int32_t u = users ? users[q] : (int32_t)q;
    const int64_t t0 = tptr[u], tl = tptr[u + 1] - t0;
    if (tl <= 0) continue;
    const int64_t c0 = cptr[u];
    const int n = nneg[q];
    for (int j = lane; j < n; j += 64) cind[c0 + j] = negs[q * nnegs + j];
    for (int64_t j = lane; j < tl; j += 64) cind[c0 + n + j] = tind[t0 + j];
  }
}
}  // namespace

namespace {
thread_local double g_weighted_kernel_ms = 0.0;  // k_sample_weighted of this thread's most recent weighted call
struct Widen {  // the scan of the uploaded weights adds in 64 bits
  __host__ __device__ uint64_t operator()(const uint32_t v) const { return (uint64_t)v; }
};

// Both device calls.  weighted: the weighted rule, over `weights` (ncols of them, on the host) or, when nullptr, over
// the popularity of the resident matrix's columns, read off its column view's pointer.
slimgpu_candset* sample_on_device(const char* name, slimgpu_evalset_t* es, int32_t nnegs, uint64_t seed, bool weighted,
                                  const uint32_t* weights, int32_t* status) {
  const std::string who = std::string(name) + ": ";
  auto bad = [&](const std::string& why) {
    *status = refuse(who + why);
    return static_cast<slimgpu_candset*>(nullptr);
  };
  EvalSetRows V;
  if (evalset_rows(es, &V) != SLIM_OK) return bad("bad arguments (an eval set)");
  if (nnegs < 1) return bad("nnegs must be at least 1, not " + std::to_string(nnegs));
  if (V.merged)
    return bad("the matrix was staged with SLIM_GPU_DUPLICATES=sum and repeated pairs were merged: its rows are not "
               "the caller's");
  if ((int64_t)nnegs + V.max_test > SLIMGPU_MAX_LIST)
    return bad("nnegs " + std::to_string(nnegs) + " and the longest selected test row, " + std::to_string(V.max_test) +
               " entries, give a candidate row above " + std::to_string(SLIMGPU_MAX_LIST) +
               ": the evaluation needs lists");
  if (V.ncols < 1 || V.ncols > SLIMGPU_SAMPLE_MAX_NCOLS)
    return bad("the matrix has " + std::to_string(V.ncols) + " items: the device sampler keeps one bit per item in LDS "
               "and takes at most " + std::to_string(SLIMGPU_SAMPLE_MAX_NCOLS) + " (SLIMGPU_CandSetSample" + (weighted ? "Weighted" : "") + " serves)");
  uint64_t T = 0;  // the weights' sum
  std::vector<uint32_t> popularity;
  slimgpu_candset* cs = nullptr;
  *status = guarded(name, [&]() -> int32_t {
    if (weighted && !weights) {  // the column counts of the resident matrix, from its column view's pointer
      std::vector<int64_t> cp((size_t)V.ncols + 1, 0);
      if (matrix_get_column_view(V.mat, cp.data(), nullptr, nullptr, nullptr) != SLIM_OK)
        return refuse(who + "the resident matrix has no column view");
      popularity.resize((size_t)V.ncols);
      for (int32_t i = 0; i < V.ncols; ++i) popularity[i] = (uint32_t)(cp[(size_t)i + 1] - cp[i]);
      weights = popularity.data();
    }
    if (weighted)
      for (int32_t i = 0; i < V.ncols; ++i) T += weights[i];
    if (weighted && T == 0) return refuse(who + "the weights sum to 0 (T = 0): nothing can be drawn");
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(V.device));
    hipStream_t stream = V.stream;
    const int32_t nsel = V.nsel, nall = V.nall;
    std::vector<int64_t> h_cptr((size_t)nall + 1, 0);
    DeviceBuffer<int64_t> d_cptr((size_t)nall + 1);
    DeviceBuffer<int32_t> d_cind;
    if (nsel > 0) {
      DeviceBuffer<int32_t> negs((size_t)nsel * (size_t)nnegs), nneg((size_t)nsel);
      DeviceBuffer<int64_t> len((size_t)nall + 1);
      SampleArgs A = {};
      A.nsel = nsel; A.ncols = V.ncols; A.nnegs = nnegs; A.seed = seed;
      A.users = V.d_users; A.hptr = V.hptr; A.hind = V.hind; A.tptr = V.tptr; A.tind = V.tind;
      A.negs = negs.get(); A.nneg = nneg.get();
      // a user is dense only when 2 * (E + nnegs) > ncols, and E is at most its history plus its test row
      const bool dense = 2 * (V.max_hist + V.max_test + (int64_t)nnegs) > (int64_t)V.ncols;
      size_t lds = sizeof(uint32_t) * (size_t)((V.ncols + 31) >> 5) + sizeof(int32_t) * (size_t)nnegs;
      lds = (lds + 15) / 16 * 16;
      A.rec_offset = (int32_t)lds;
      if (dense) {
        A.rec_cap = 1;
        while (A.rec_cap < nnegs) A.rec_cap <<= 1;
        lds += sizeof(uint4) * (size_t)A.rec_cap;
      }
      DeviceBuffer<uint32_t> d_w;
      DeviceBuffer<uint64_t> d_C;
      DeviceBuffer<char> wtmp;
      const uint64_t* C = nullptr;
      if (weighted) {
        // C[0 .. ncols]: an exclusive scan, in 64 bits, of the uploaded weights and a closing 0
        const size_t n1 = (size_t)V.ncols + 1;
        {
          d_w = DeviceBuffer<uint32_t>(n1);
          d_C = DeviceBuffer<uint64_t>(n1);
          HIP_TRY(hipMemsetAsync(d_w.get() + V.ncols, 0, sizeof(uint32_t), stream));
          HIP_TRY(hipMemcpyAsync(d_w.get(), weights, sizeof(uint32_t) * (size_t)V.ncols, hipMemcpyHostToDevice, stream));
          auto in = rocprim::make_transform_iterator(d_w.get(), Widen());
          size_t wbytes = 0;
          HIP_TRY(rocprim::exclusive_scan(nullptr, wbytes, in, d_C.get(), (uint64_t)0, n1, rocprim::plus<uint64_t>(),
                                          stream));
          wtmp = DeviceBuffer<char>(wbytes);
          HIP_TRY(rocprim::exclusive_scan(wtmp.get(), wbytes, in, d_C.get(), (uint64_t)0, n1, rocprim::plus<uint64_t>(),
                                          stream));
          C = d_C.get();
        }
        // bitmap + ids + the block sums of phase 2: 84 KB at the item bound and nnegs = SLIMGPU_MAX_LIST
        lds = sizeof(uint32_t) * (size_t)((V.ncols + 31) >> 5) + sizeof(int32_t) * (size_t)nnegs;
        lds = (lds + 15) / 16 * 16;
        A.rec_offset = (int32_t)lds;
        A.rec_cap = 0;
        lds += sizeof(uint64_t) * (size_t)((V.ncols + 1023) >> 10);
        if (lds > 64 * 1024)
          HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sample_weighted),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      } else if (lds > 64 * 1024) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sample_negatives),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      }
      const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, (160 * 1024) / (lds + 64)));
      const int groups = std::max(1, std::min<int>(nsel, V.num_cus * per_cu));
      if (std::getenv("SLIM_GPU_TRACE")) {  // how many positions a workgroup serves one after the other
        if (weighted)
          std::fprintf(stderr, "[trace] k_sample_weighted: %d positions, %d workgroups, %zu bytes of LDS, %d items, "
                               "nnegs %d, per %d\n",
                       nsel, groups, lds, V.ncols, nnegs, (((V.ncols + 1023) >> 10) + 63) >> 6);
        else
          std::fprintf(stderr, "[trace] k_sample_negatives: %d positions, %d workgroups, %zu bytes of LDS, %d items, "
                               "nnegs %d, %s\n",
                       nsel, groups, lds, V.ncols, nnegs, dense ? "sort records" : "no sort records");
      }
      bool timed = false;
      // the weighted kernel's own time, for SLIMGPU_LastSampleKernelMs: a record that fails leaves the call untimed
      std::optional<EventPair> ev;
      if (weighted) {
        ev.emplace();
        g_weighted_kernel_ms = 0.0;  // (never the figure of an earlier call: 0 when this one cannot be timed)
        timed = hipEventRecord(ev->ev0, stream) == hipSuccess;
        hipLaunchKernelGGL(k_sample_weighted, dim3(groups), dim3(64), lds, stream, A, C, T);
        timed = hipEventRecord(ev->ev1, stream) == hipSuccess && timed;
      } else {
        hipLaunchKernelGGL(k_sample_negatives, dim3(groups), dim3(64), lds, stream, A);
      }
      HIP_TRY(hipGetLastError());
      const unsigned flat = (unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)nsel + 255) / 256, (int64_t)V.num_cus * 16));
      HIP_TRY(hipMemsetAsync(len.get(), 0, sizeof(int64_t) * ((size_t)nall + 1), stream));
      hipLaunchKernelGGL(k_sample_rowlen, dim3(flat), dim3(256), 0, stream, nsel, V.d_users, V.tptr, nneg.get(),
                         len.get());
      HIP_TRY(hipGetLastError());
      size_t scan_bytes = 0;
      HIP_TRY(rocprim::inclusive_scan(nullptr, scan_bytes, len.get(), d_cptr.get(), (size_t)nall + 1,
                                      rocprim::plus<int64_t>(), stream));
      DeviceBuffer<char> tmp(scan_bytes);
      HIP_TRY(rocprim::inclusive_scan(tmp.get(), scan_bytes, len.get(), d_cptr.get(), (size_t)nall + 1,
                                      rocprim::plus<int64_t>(), stream));
      // the row pointer is all the host learns of the set: 8 bytes per user, once
      HIP_TRY(hipMemcpyAsync(h_cptr.data(), d_cptr.get(), sizeof(int64_t) * ((size_t)nall + 1), hipMemcpyDeviceToHost,
                             stream));
      HIP_TRY(hipStreamSynchronize(stream));
      const int64_t n = h_cptr[(size_t)nall];
      if (n < 0 || n > (int64_t)nsel * nnegs + V.test_entries) throw HipFail{hipErrorUnknown, "the sampled row pointer"};
      d_cind = DeviceBuffer<int32_t>((size_t)n);
      const unsigned waves = (unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)nsel + 3) / 4, (int64_t)V.num_cus * 16));
      hipLaunchKernelGGL(k_sample_rows, dim3(waves), dim3(256), 0, stream, nsel, V.d_users, nnegs, negs.get(),
                         nneg.get(), V.tptr, V.tind, d_cptr.get(), d_cind.get());
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(stream));  // (negs and nneg go with this block)
      if (weighted && timed) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev->ev0, ev->ev1) == hipSuccess) g_weighted_kernel_ms = ms;
      }
    } else {
      d_cind = DeviceBuffer<int32_t>(0);
      HIP_TRY(hipMemsetAsync(d_cptr.get(), 0, sizeof(int64_t) * ((size_t)nall + 1), stream));
    }
    cs = candset_adopt(V.ncols, std::move(h_cptr), std::move(d_cptr), std::move(d_cind), V.device, V.num_cus, stream);
    return SLIM_OK;
  });
  return cs;
}
}  // namespace

slimgpu_candset* evalset_sample_candidates(slimgpu_evalset_t* es, int32_t nnegs, uint64_t seed, int32_t* status) {
  return sample_on_device("SLIMGPU_EvalSetSampleCandidates", es, nnegs, seed, false, nullptr, status);
}
double last_weighted_sample_kernel_ms() { return g_weighted_kernel_ms; }
slimgpu_candset* evalset_sample_candidates_weighted(slimgpu_evalset_t* es, int32_t nnegs, uint64_t seed,
                                                    const uint32_t* weights, int32_t* status) {
  return sample_on_device("SLIMGPU_EvalSetSampleCandidatesWeighted", es, nnegs, seed, true, weights, status);
}
}  // namespace slimamd
