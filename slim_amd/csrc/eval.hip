// eval.hip -- the consumers of a learned model that the reference runs per user on the host,
// as HIP kernels:
//   * hit counting, HR / ARHR and the head / tail split of the leave-k-out protocol
//     (/root/reference/src/programs/slim_predict.c:181-236, slim_mselect.c:122-187,
//     src/libslim/pyapi.c:309-366), one user per lane (every list length of an evaluation from one
//     walk over the list, eval_terms.hpp), then ONE wavefront per list length adding the users'
//     terms in user order with the reference's own arithmetic (float accumulators fed with
//     double terms, pyapi.c:223-230) -- so the four figures are the host loop's, bit for bit;
//   * the 1-vs-k protocol (src/libslim/predict.c:77-133, pyapi.c:483-528): every user ranks
//     a given list of candidate items; one wavefront per user, one candidate per lane, the
//     candidate's entry of each history item's model row found by binary search (model rows
//     ascending by id) and added in history order -- the float additions of the host loop in
//     the same order, hence the same scores; ties keep candidate order like the host's
//     stable sort.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "call_frame.hpp"
#include "engine.hpp"
#include "eval_terms.hpp"
#include "hip_check.hpp"
#include "host_csr.hpp"

namespace slimamd {

namespace {

// ---- HR / ARHR -------------------------------------------------------------------------

// One lane per position: the test row once (what does not depend on the cutoff), then ONE walk over the
// list in rank order; the record of a cutoff is formed when the walk reaches its rank (or the end of the
// list), from the sums so far -- the prefix argument of eval_terms.hpp.
__global__ void k_user_terms(int32_t nsel, const int32_t* __restrict__ users, int32_t nrcmds, const Cutoffs cut,
                             const int32_t* __restrict__ lists, const int32_t* __restrict__ counts,
                             const int64_t* __restrict__ tptr, const int32_t* __restrict__ tind,
                             const int32_t* __restrict__ fmarker, int32_t fm_ncols,
                             UserTerms* __restrict__ out) {
  for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nsel; q += gridDim.x * blockDim.x) {
    const int32_t u = users ? users[q] : q;
    const int64_t t0 = tptr[u], t1 = tptr[u + 1];
    int ntrue0 = 0, ntrue1 = 0, flags = 0;
    float ideal = 0.0f;
    if (t1 - t0 >= 1) {
      flags = 1;
      for (int64_t z = t0; z < t1; ++z) {
        const int32_t it = tind[z];
        const int cls = (it >= 0 && it < fm_ncols) ? fmarker[it] : 1;
        if (cls) ++ntrue1; else ++ntrue0;
        flags |= cls ? 4 : 2;
        ideal = (float)((double)ideal + 1.0 / (1.0 + double(z - t0)));
      }
    }
    HitWalk w;
    const int n = flags ? counts[q] : 0;
    int r = 0;
    const unsigned long long cuts = cut.packed();
    for (int k = 0; k < cut.n; ++k) {
      // the last record takes the whole list, whatever its row length nrcmds (SLIMGPU_Evaluate sets no upper
      // bound on it); the lengths before it come from an eval set and are at most 128
      const int end = min(n, k == cut.n - 1 ? nrcmds : Cutoffs::at(cuts, k));
      for (; r < end; ++r) {
        const int32_t id = lists[(int64_t)q * nrcmds + r];
        bool hit = false;
        for (int64_t z = t0; z < t1 && !hit; ++z) hit = tind[z] == id;
        if (hit) w.hit(r, (id >= 0 && id < fm_ncols) ? fmarker[id] : 1);
      }
      out[(int64_t)k * nsel + q] = w.terms(ntrue0, ntrue1, t1 - t0, ideal, flags);
    }
  }
}

// The same records from the ranks of the test entries (slim_gpu_rank.h) instead of lists: a test item is in
// the list of length c exactly when 0 < rank <= c, and it stands at position rank - 1 there.  One lane per
// position.  The hits are the DISTINCT non-zero ranks (distinct candidates have distinct ranks, so one id
// listed twice in the test row gives one rank twice and, like one list slot, one hit), walked ascending: the
// additions of k_user_terms in the same order.  Everything about the test row is formed as there.
__global__ void k_rank_terms(int32_t nsel, const int32_t* __restrict__ users, const Cutoffs cut,
                             const int32_t* __restrict__ ranks, const int64_t* __restrict__ tbase,
                             const int64_t* __restrict__ tptr, const int32_t* __restrict__ tind,
                             const int32_t* __restrict__ fmarker, int32_t fm_ncols, UserTerms* __restrict__ out) {
  for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nsel; q += gridDim.x * blockDim.x) {
    const int32_t u = users ? users[q] : q;
    const int64_t t0 = tptr[u], t1 = tptr[u + 1];
    const int32_t* rk = ranks + tbase[q];
    int ntrue0 = 0, ntrue1 = 0, flags = 0;
    float ideal = 0.0f;
    if (t1 - t0 >= 1) {
      flags = 1;
      for (int64_t z = t0; z < t1; ++z) {
        const int32_t it = tind[z];
        const int cls = (it >= 0 && it < fm_ncols) ? fmarker[it] : 1;
        if (cls) ++ntrue1; else ++ntrue0;
        flags |= cls ? 4 : 2;
        ideal = (float)((double)ideal + 1.0 / (1.0 + double(z - t0)));
      }
    }
    HitWalk w;
    // the smallest rank above `prev`, and its item
    int32_t prev = 0, nxt = 0, nxt_id = 0;
    auto advance = [&] {
      nxt = 0;
      for (int64_t z = t0; z < t1; ++z) {
        const int32_t r = rk[z - t0];
        if (r > prev && (nxt == 0 || r < nxt)) {
          nxt = r;
          nxt_id = tind[z];
        }
      }
    };
    advance();
#pragma unroll
    for (int k = 0; k < SLIMGPU_MAX_CUTOFFS; ++k) {  // (constant indices into the kernel argument)
      if (k < cut.n) {
        const int32_t c = cut.c[k];
        while (nxt != 0 && nxt <= c) {
          w.hit(nxt - 1, (nxt_id >= 0 && nxt_id < fm_ncols) ? fmarker[nxt_id] : 1);
          prev = nxt;
          advance();
        }
        out[(int64_t)k * nsel + q] = w.terms(ntrue0, ntrue1, t1 - t0, ideal, flags);
      }
    }
  }
}

// The accumulators of one cutoff in one wavefront: every lane holds a record, add() walks the first `cnt` lanes in
// lane order and every lane keeps the same running sums.
struct SumsInLaneOrder {
  float hr_all = 0, hr_head = 0, hr_tail = 0, arhr = 0;
  int nvalid = 0, nhead = 0, ntail = 0;
  __device__ __forceinline__ void add(const UserTerms& t, int cnt) {
    for (int k = 0; k < cnt; ++k) {
      const int fl = __shfl(t.flags, k);
      if (!(fl & 1)) continue;
      const double a = __shfl(t.hr_all, k), h = __shfl(t.hr_head, k), tl = __shfl(t.hr_tail, k);
      const float ar = __shfl(t.arhr, k);
      ++nvalid;
      nhead += (fl & 2) ? 1 : 0;
      ntail += (fl & 4) ? 1 : 0;
      hr_head = (float)((double)hr_head + h);   // float += double, as the host loop
      hr_tail = (float)((double)hr_tail + tl);
      hr_all = (float)((double)hr_all + a);
      arhr += ar;
    }
  }
  __device__ __forceinline__ void store(EvalSums& o) const {
    o.f[0] = hr_all; o.f[1] = hr_head; o.f[2] = hr_tail; o.f[3] = arhr;
    o.n[0] = nvalid; o.n[1] = nhead; o.n[2] = ntail;
    o.pad = 0;
  }
};

// every position of one cutoff: 64 positions' terms per coalesced load, added by lane order = position order
__device__ __forceinline__ SumsInLaneOrder sum_every_position(int32_t nsel, const UserTerms* __restrict__ terms,
                                                              int lane) {
  SumsInLaneOrder sums;
  for (int32_t b = 0; b < nsel; b += 64) {
    const int32_t u = b + lane;
    UserTerms t = {0.0, 0.0, 0.0, 0.0f, 0};
    if (u < nsel) t = terms[u];
    sums.add(t, nsel - b < 64 ? nsel - b : 64);
  }
  return sums;
}

// one wavefront per cutoff
__global__ __launch_bounds__(64) void k_sum_in_user_order(int32_t nsel, const UserTerms* __restrict__ terms,
                                                          EvalSums* __restrict__ out) {
  const int lane = threadIdx.x;
  const SumsInLaneOrder sums = sum_every_position(nsel, terms + (int64_t)blockIdx.x * nsel, lane);
  if (lane == 0) sums.store(out[blockIdx.x]);
}

// one wavefront per (cutoff, group) = (blockIdx.x, blockIdx.y), ngroups = gridDim.y - 1: the positions
// order[offsets[g] .. offsets[g + 1]) of the group (slim_gpu_groups.h; ascending, every one in [0, nsel)), 64 gathered
// records at a time, added by lane order = position order with the arithmetic above.  out[k * ngroups + g]; a group
// without positions gives zeros.  The last row of blocks is k_sum_in_user_order's work, every[k], in the same launch:
// the longest chain of the launch is the one over everybody, which ran anyway.
__global__ __launch_bounds__(64) void k_sum_groups_in_user_order(int32_t nsel, const UserTerms* __restrict__ terms,
                                                                 const int32_t* __restrict__ order,
                                                                 const int64_t* __restrict__ offsets,
                                                                 EvalSums* __restrict__ out,
                                                                 EvalSums* __restrict__ every) {
  const int lane = threadIdx.x;
  const int ngroups = gridDim.y - 1;
  terms += (int64_t)blockIdx.x * nsel;
  if ((int)blockIdx.y == ngroups) {
    const SumsInLaneOrder all = sum_every_position(nsel, terms, lane);
    if (lane == 0) all.store(every[blockIdx.x]);
    return;
  }
  const int64_t i0 = offsets[blockIdx.y], i1 = offsets[blockIdx.y + 1];
  SumsInLaneOrder sums;
  for (int64_t b = i0; b < i1; b += 64) {
    const int64_t i = b + lane;
    UserTerms t = {0.0, 0.0, 0.0, 0.0f, 0};
    if (i < i1) t = terms[order[i]];
    sums.add(t, i1 - b < 64 ? (int)(i1 - b) : 64);
  }
  if (lane == 0) sums.store(out[(int64_t)blockIdx.x * ngroups + blockIdx.y]);
}

// the group of every position by the length of its user's history: #{j : length >= bounds[j]} (bounds ascend; they
// are read from LDS)
__global__ __launch_bounds__(256) void k_history_bands(int32_t nsel, const int32_t* __restrict__ users,
                                                       const int64_t* __restrict__ hptr, int32_t nbounds,
                                                       const int32_t* __restrict__ bounds,
                                                       int32_t* __restrict__ group_of_position) {
  __shared__ int32_t s_bounds[SLIMGPU_MAX_GROUPS];
  for (int j = threadIdx.x; j < nbounds; j += blockDim.x) s_bounds[j] = bounds[j];
  __syncthreads();
  for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nsel; q += gridDim.x * blockDim.x) {
    const int32_t u = users ? users[q] : q;
    const int64_t len = hptr[u + 1] - hptr[u];
    int lo = 0, hi = nbounds;  // the first bound above len
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_bounds[mid] <= len) lo = mid + 1; else hi = mid;
    }
    group_of_position[q] = lo;
  }
}

// ---- 1-vs-k ----------------------------------------------------------------------------

constexpr int kMaxCandPerLane = 16;  // up to 1024 candidates per user

__global__ __launch_bounds__(64) void k_topn_1vsk(int32_t nusers, int32_t wrows, int32_t ncols,
                                                  int32_t nrcmds, int32_t nnegs,
                                                  const int64_t* __restrict__ wptr,
                                                  const int32_t* __restrict__ wind,
                                                  const float* __restrict__ wval,
                                                  const int64_t* __restrict__ hptr,
                                                  const int32_t* __restrict__ hind,
                                                  const float* __restrict__ hval,
                                                  const int32_t* __restrict__ negitems,
                                                  int32_t* __restrict__ out_ids,
                                                  float* __restrict__ out_scores) {
  const int lane = threadIdx.x;
  const int per = (nnegs + 63) / 64;
  for (int32_t u = blockIdx.x; u < nusers; u += gridDim.x) {
    const int32_t* neg = negitems + (int64_t)u * nnegs;
    int cid[kMaxCandPerLane];
    float key[kMaxCandPerLane];
    bool live[kMaxCandPerLane];  // receives scores: a valid id not repeated later in the list
#pragma unroll
    for (int k = 0; k < kMaxCandPerLane; ++k) {
      const int c = lane + 64 * k;
      cid[k] = (k < per && c < nnegs) ? neg[c] : -1;
      key[k] = 0.0f;
      live[k] = k < per && c < nnegs && cid[k] >= 0 && cid[k] < ncols;
      // predict.c:92-99: the position table keeps the LAST occurrence of a repeated id
      if (live[k])
        for (int c2 = c + 1; c2 < nnegs; ++c2)
          if (neg[c2] == cid[k]) {
            live[k] = false;
            break;
          }
    }
    const int64_t h0 = hptr[u], h1 = hptr[u + 1];
    for (int64_t e = h0; e < h1; ++e) {  // history order, as the host loop
      const int32_t i = hind[e];
      if (i < 0 || i >= wrows) continue;
      const float rating = hval ? hval[e] : 1.0f;
      const int64_t s = wptr[i], t = wptr[i + 1];
#pragma unroll
      for (int k = 0; k < kMaxCandPerLane; ++k) {
        if (!live[k]) continue;
        int64_t lo = s, hi = t;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (wind[mid] < cid[k]) lo = mid + 1; else hi = mid;
        }
        if (lo < t && wind[lo] == cid[k]) {
          // product and sum rounded separately, like the host's `key += rating * w` (__fmul_rn and
          // __fadd_rn are plain operators to the compiler: it fused them into one FMA, and rated
          // histories scored an ulp off the host)
#pragma clang fp contract(off)
          const float prod = rating * wval[lo];
          key[k] = key[k] + prod;
        }
      }
    }
    // emit_best: descending score, ties in candidate order; nrcmds rounds of a wave arg-max
    const int n = nnegs < nrcmds ? nnegs : nrcmds;
    bool used[kMaxCandPerLane];
#pragma unroll
    for (int k = 0; k < kMaxCandPerLane; ++k) used[k] = !(k < per && lane + 64 * k < nnegs);
    for (int r = 0; r < n; ++r) {
      float bs = -__builtin_huge_valf();
      int bc = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < kMaxCandPerLane; ++k) {
        const int c = lane + 64 * k;
        if (!used[k] && (key[k] > bs || (key[k] == bs && c < bc))) {
          bs = key[k];
          bc = c;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float os = __shfl_xor(bs, off);
        const int oc = __shfl_xor(bc, off);
        if (os > bs || (os == bs && oc < bc)) {
          bs = os;
          bc = oc;
        }
      }
      if ((bc & 63) == lane) {
        const int k = bc >> 6;
#pragma unroll
        for (int kk = 0; kk < kMaxCandPerLane; ++kk)
          if (kk == k) {
            used[kk] = true;
            out_ids[(int64_t)u * nrcmds + r] = neg[bc];
            out_scores[(int64_t)u * nrcmds + r] = key[kk];
          }
      }
    }
  }
}

template <class T>
void upload(DeviceBuffer<T>& b, const T* src, size_t n) {
  if (n) HIP_TRY(hipMemcpy(b.get(), src, sizeof(T) * n, hipMemcpyHostToDevice));
}

}  // namespace

void launch_user_terms(hipStream_t stream, int num_cus, int32_t nsel, const int32_t* users, int32_t nrcmds,
                       const Cutoffs& cut, const int32_t* lists, const int32_t* counts, const int64_t* tptr,
                       const int32_t* tind, const int32_t* fmarker, int32_t fm_ncols, UserTerms* terms) {
  const int blocks = std::max(1, std::min((nsel + 255) / 256, num_cus * 8));
  hipLaunchKernelGGL(k_user_terms, dim3(blocks), dim3(256), 0, stream, nsel, users, nrcmds, cut, lists, counts,
                     tptr, tind, fmarker, fm_ncols, terms);
  HIP_TRY(hipGetLastError());
}

void launch_rank_terms(hipStream_t stream, int num_cus, int32_t nsel, const int32_t* users, const Cutoffs& cut,
                       const int32_t* ranks, const int64_t* tbase, const int64_t* tptr, const int32_t* tind,
                       const int32_t* fmarker, int32_t fm_ncols, UserTerms* terms) {
  const int blocks = std::max(1, std::min((nsel + 255) / 256, num_cus * 8));
  hipLaunchKernelGGL(k_rank_terms, dim3(blocks), dim3(256), 0, stream, nsel, users, cut, ranks, tbase, tptr, tind,
                     fmarker, fm_ncols, terms);
  HIP_TRY(hipGetLastError());
}

void launch_sum_in_user_order(hipStream_t stream, int32_t nsel, int32_t ncut, const UserTerms* terms,
                              EvalSums* out) {
  hipLaunchKernelGGL(k_sum_in_user_order, dim3(ncut), dim3(64), 0, stream, nsel, terms, out);
  HIP_TRY(hipGetLastError());
}

void launch_sum_groups_in_user_order(hipStream_t stream, int32_t nsel, int32_t ncut, int32_t ngroups,
                                     const UserTerms* terms, const int32_t* order, const int64_t* offsets,
                                     EvalSums* out, EvalSums* every) {
  hipLaunchKernelGGL(k_sum_groups_in_user_order, dim3(ncut, ngroups + 1), dim3(64), 0, stream, nsel, terms, order,
                     offsets, out, every);
  HIP_TRY(hipGetLastError());
}

void launch_history_bands(hipStream_t stream, int num_cus, int32_t nsel, const int32_t* users, const int64_t* hptr,
                          int32_t nbounds, const int32_t* bounds, int32_t* group_of_position) {
  const int blocks = std::max(1, std::min((nsel + 255) / 256, num_cus * 8));
  hipLaunchKernelGGL(k_history_bands, dim3(blocks), dim3(256), 0, stream, nsel, users, hptr, nbounds, bounds,
                     group_of_position);
  HIP_TRY(hipGetLastError());
}

int32_t evaluate_device(int32_t nusers, int32_t nrcmds, const int32_t* lists, const int32_t* counts,
                        const slim_csr_t* tst, const int32_t* fmarker, int32_t fm_ncols,
                        EvalResult* out) {
  if (!lists || !counts || !tst || !tst->rowptr || !fmarker || !out || nrcmds < 1) {
    set_error("SLIMGPU_Evaluate: bad arguments");
    return SLIM_ERROR_INPUT;
  }
  nusers = std::min(nusers, tst->nrows);
  *out = EvalResult();
  if (nusers <= 0) return SLIM_OK;
  return guarded("SLIMGPU_Evaluate", [&]() -> int32_t {
    (void)hipGetLastError();
    DeviceBuffer<int32_t> d_lists((size_t)nusers * nrcmds), d_counts((size_t)nusers),
        d_fm((size_t)std::max(fm_ncols, 1));
    const StagedCsr t = stage_csr(tst, nusers, /*values=*/false, /*stream=*/nullptr);
    DeviceBuffer<UserTerms> d_terms((size_t)nusers);
    DeviceBuffer<EvalSums> d_sums(1);
    upload(d_lists, lists, (size_t)nusers * nrcmds);
    upload(d_counts, counts, (size_t)nusers);
    upload(d_fm, fmarker, (size_t)fm_ncols);
    // every user, one cutoff: the lists are as long as the caller made them
    launch_user_terms(nullptr, cu_count(), nusers, nullptr, nrcmds, one_cutoff(nrcmds), d_lists.get(),
                      d_counts.get(), t.ptr.get(), t.ind.get(), d_fm.get(), fm_ncols, d_terms.get());
    launch_sum_in_user_order(nullptr, nusers, 1, d_terms.get(), d_sums.get());
    EvalSums h;
    HIP_TRY(hipMemcpy(&h, d_sums.get(), sizeof(h), hipMemcpyDeviceToHost));
    *out = result_of(h);
    return SLIM_OK;
  });
}

int32_t predict_1vsk_device(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds,
                            int32_t nnegs, const int32_t* negitems, int32_t* output,
                            float* scores) {
  if (!W || !hist || !W->rowptr || !hist->rowptr || (!W->rowval && W->rowptr[W->nrows] > 0) || nrcmds < 1 ||
      nnegs < 1 || !negitems || nnegs > 64 * kMaxCandPerLane) {
    set_error("SLIMGPU_Predict1vsK: bad arguments (1 <= nnegs <= 1024)");
    return SLIM_ERROR_INPUT;
  }
  const int32_t nusers = hist->nrows;
  if (nusers <= 0) return SLIM_ERROR;
  return guarded("SLIMGPU_Predict1vsK", [&]() -> int32_t {
    (void)hipGetLastError();
    const int cus = cu_count();
    const StagedPair P = stage_pair(W, hist, cus);  // (a model without entries has no row out of order)
    if (P.W.nnz > 0 && !P.W.rows_sorted) return refuse("SLIMGPU_Predict1vsK: model rows are not ascending by item id");
    DeviceBuffer<int32_t> d_neg((size_t)nusers * nnegs), d_oid((size_t)nusers * nrcmds);
    DeviceBuffer<float> d_osc((size_t)nusers * nrcmds);
    upload(d_neg, negitems, (size_t)nusers * nnegs);
    hipLaunchKernelGGL(k_topn_1vsk, dim3(std::max(1, std::min(nusers, cus * 16))), dim3(64), 0, 0,
                       nusers, W->nrows, W->ncols, nrcmds, nnegs, P.W.d_ptr, P.W.d_ind, P.W.d_val, P.H.ptr,
                       P.H.ind, P.H.val, d_neg.get(), d_oid.get(), d_osc.get());
    HIP_TRY(hipGetLastError());
    const int32_t n = std::min(nnegs, nrcmds);
    std::vector<int32_t> h_id((size_t)nusers * nrcmds);
    std::vector<float> h_sc((size_t)nusers * nrcmds);
    HIP_TRY(hipMemcpy(h_id.data(), d_oid.get(), sizeof(int32_t) * h_id.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_sc.data(), d_osc.get(), sizeof(float) * h_sc.size(), hipMemcpyDeviceToHost));
    for (int32_t u = 0; u < nusers; ++u)
      for (int32_t r = 0; r < n; ++r) {
        output[(int64_t)u * nrcmds + r] = h_id[(size_t)u * nrcmds + r];
        scores[(int64_t)u * nrcmds + r] = h_sc[(size_t)u * nrcmds + r];
      }
    return SLIM_OK;
  });
}

}  // namespace slimamd
