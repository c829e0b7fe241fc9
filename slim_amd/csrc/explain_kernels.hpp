// explain_kernels.hpp -- the kernels of slim_gpu_explain.h (explain.hip launches them): the terms behind the slot
// scores of candidate rows, kept apart instead of added.
//
// k_explain: one workgroup of 4 wavefronts per position (user), grid-stride.  The workgroup stages the first
// `stage` history entries of the user in LDS as 16-byte records (h, r, W.ptr[h], W.ptr[h + 1]); positions behind
// them are read from HBM by the same code (history_record).  Each wavefront takes the live slots wave, wave + 4, .. of
// the user's candidate row.  Per slot the lanes stride over the history positions; a lane looks the slot's id up in
// the model row (rows ascend: a binary search), forms t = r * w and puts a 64-bit key into its own sorted list of
// K places, which lives in registers (the insertion is unrolled: no dynamic register index, nothing in scratch).
// Then at most nwhy rounds take the wave-wide maximum of the lanes' heads; positions are unique, so one lane owns
// it, pops it and writes the item and the term.  The slot loop is the outer loop: a lane's state lives for one slot.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace slimamd {

constexpr int kExplainWaves = 4;

struct ExplainArgs {
  // the model's rows (ids ascend inside a row; fewer than 2^31 entries) and the histories
  int32_t wrows;
  const int64_t* wptr; const int32_t* wind; const float* wval;
  int32_t npos;
  const int32_t* users;  // the user of every position; nullptr: position q is user q
  const int64_t* hptr; const int32_t* hind; const float* hval;  // hval == nullptr: binary
  // the candidate rows: cptr as given, lptr / pairs the live entries as (id, slot)
  const int64_t* cptr; const int64_t* lptr; const int2* pairs;
  // the outputs, rows of the positions side by side: position q starts at obase[q] (nullptr: at cptr[q], the
  // layout of the set); items / terms are [entries][nwhy] and may both be null; support is preset to 0
  const int64_t* obase;
  int32_t nwhy;
  int32_t stage;  // history entries staged in LDS (the launch's dynamic LDS holds 16 bytes for each)
  int32_t* items; float* terms; int32_t* support;
};

// The order of the terms as an unsigned order: the image of t grows with t, and -0.0f shares the image of 0.0f.
__device__ __forceinline__ uint32_t term_image(float t) {
  const uint32_t b = t == 0.0f ? 0u : __float_as_uint(t);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
// key = image << 32 | (2^31 - 1 - p) << 1 | (t is -0.0f): larger is better (term descending, then position
// ascending); the lowest bit never decides, positions are unique.  0 is no key: p stays below 2^31 - 1.
__device__ __forceinline__ unsigned long long term_key(float t, uint32_t p) {
  const uint32_t neg0 = __float_as_uint(t) == 0x80000000u;
  return ((unsigned long long)term_image(t) << 32) | ((0x7FFFFFFFu - p) << 1) | neg0;
}
__device__ __forceinline__ uint32_t key_position(unsigned long long k) { return 0x7FFFFFFFu - ((uint32_t)k >> 1); }
__device__ __forceinline__ float key_term(unsigned long long k) {  // the product as computed, sign of zero included
  if ((uint32_t)k & 1u) return -0.0f;
  const uint32_t img = (uint32_t)(k >> 32);
  return __uint_as_float(img ^ ((img >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// position p of the history that starts at h0: (h, bits of r, begin and end of model row h); a history id without
// a model row gets an empty row
__device__ __forceinline__ int4 history_record(const ExplainArgs& A, int64_t h0, uint32_t p) {
  const int32_t h = A.hind[h0 + p];
  const float r = A.hval ? A.hval[h0 + p] : 1.0f;
  const bool in = h >= 0 && h < A.wrows;
  return make_int4(h, (int)__float_as_uint(r), in ? (int)A.wptr[h] : 0, in ? (int)A.wptr[h + 1] : 0);
}

template <int K>
__global__ __launch_bounds__(64 * kExplainWaves) void k_explain(const ExplainArgs A) {
  extern __shared__ int4 staged[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int q = blockIdx.x; q < A.npos; q += gridDim.x) {
    const int u = A.users ? __builtin_amdgcn_readfirstlane(A.users[q]) : q;
    const int64_t h0 = A.hptr[u];
    const uint32_t n = (uint32_t)(A.hptr[u + 1] - h0);
    const uint32_t nst = n < (uint32_t)A.stage ? n : (uint32_t)A.stage;
    const int64_t l0 = A.lptr[u], l1 = A.lptr[u + 1];
    const int64_t ob = A.obase ? A.obase[q] : A.cptr[u];
    if (l1 > l0)
      for (uint32_t p = tid; p < nst; p += 64 * kExplainWaves) staged[p] = history_record(A, h0, p);
    __syncthreads();
    for (int64_t s = l0 + wave; s < l1; s += kExplainWaves) {
      const int2 cand = A.pairs[s];  // (id, slot)
      unsigned long long best[K];
#pragma unroll
      for (int k = 0; k < K; ++k) best[k] = 0;
      int hits = 0;
      for (uint32_t p = lane; p < n; p += 64) {
        const int4 rec = p < nst ? staged[p] : history_record(A, h0, p);
        int lo = rec.z, hi = rec.w;
        while (lo < hi) {
          const int mid = (int)(((uint32_t)lo + (uint32_t)hi) >> 1);
          if (A.wind[mid] < cand.x) lo = mid + 1; else hi = mid;
        }
        if (lo < rec.w && A.wind[lo] == cand.x) {
          ++hits;
          unsigned long long key = term_key(__fmul_rn(__uint_as_float((uint32_t)rec.y), A.wval[lo]), p);
          if (key > best[K - 1]) {
#pragma unroll
            for (int k = 0; k < K; ++k) {  // the list stays descending; the smaller of each pair moves on
              const unsigned long long a = best[k];
              best[k] = a > key ? a : key;
              key = a > key ? key : a;
            }
          }
        }
      }
      hits = wave_sum(hits);
      if (lane == 0) A.support[ob + cand.y] = hits;
      if (A.items) {
        const int rounds = hits < A.nwhy ? hits : A.nwhy;
        for (int r = 0; r < rounds; ++r) {
          const unsigned long long top = wave_max_key(best[0]);
          if (top == 0) break;   // the empty key: no lane holds another term
          if (best[0] == top) {  // exactly one lane: the positions are unique
            const int64_t at = (ob + cand.y) * A.nwhy + r;
            A.items[at] = A.hind[h0 + key_position(top)];
            A.terms[at] = key_term(top);
#pragma unroll
            for (int k = 0; k + 1 < K; ++k) best[k] = best[k + 1];
            best[K - 1] = 0;
          }
        }
      }
    }
    __syncthreads();  // the next user's records replace these
  }
}

// obase[q] = entries of the candidate rows of the users at the positions before q, obase[npos] = all of them: one
// workgroup of 256, a running sum over blocks of 256 positions
__global__ __launch_bounds__(256) void k_explain_base(int32_t npos, const int32_t* __restrict__ users,
                                                      const int64_t* __restrict__ cptr, int64_t* __restrict__ obase) {
  __shared__ int64_t part[256];
  const int tid = threadIdx.x;
  int64_t carry = 0;
  for (int32_t q0 = 0; q0 <= npos; q0 += 256) {
    const int32_t q = q0 + tid;
    int64_t len = 0;
    if (q < npos) {
      const int32_t u = users[q];
      len = cptr[u + 1] - cptr[u];
    }
    part[tid] = len;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int64_t add = tid >= off ? part[tid - off] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    if (q <= npos) obase[q] = carry + part[tid] - len;  // exclusive
    carry += part[255];
    __syncthreads();
  }
}

}  // namespace slimamd
