// split.hip -- the device split of slim_gpu_split.h: a staged matrix cut into a train matrix, staged where it is made,
// and a test matrix, the only part that comes down.  include/slim_gpu_split.h states the rule and host_csr.cpp:
// split_host is its definition in code; the kernels here hash with the same helpers (host_csr.hpp: sample_base & co.)
// and give the same rows bit for bit.
//
// Two passes and a scan between them.  The mark pass decides per entry, held or kept (one byte per entry, cleared
// first, so that rows which cannot take part are never read), and counts the held entries of every row; rocPRIM scans
// the counts into the test row pointer, and the train row pointer is the source's minus it; the scatter pass copies
// every row into its two halves in source order.  No global atomics: a row belongs to one team of lanes from its
// first entry to its last.  Rows run from empty to 10^5 entries and more, so each pass has three forms, launched one
// after the other over all rows, each taking the rows of its length class:
//   short  up to kSplitShortRow entries: 16 lanes per row, four rows per wavefront, ranks and prefixes by shuffles
//   wave   up to kSplitWaveRow entries: a wavefront (a workgroup of 64) per row
//   long   beyond: a workgroup of 256 per row, kSplitLongPiece entries at once
// In leave-out mode a row needs its (f + 1) * h <= 128 smallest (key, item, position) and never a sort of the row: a
// team keeps candidate records in LDS, and once it has sorted them for the first time the K-th smallest is a bound
// that turns all but about K * ln(L / K) of the remaining entries away with one comparison.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "call_frame.hpp"
#include "host_csr.hpp"

namespace slimamd {
namespace {
constexpr int kSplitShortRow = 16;     // rows up to this: 16 lanes each
constexpr int kSplitWaveRow = 2048;    // rows up to this: a wavefront each
constexpr int kSplitLongPiece = 1024;  // longer rows: a workgroup each, this many entries at once
constexpr int kSplitShortRowsPerBlock = 256 / 16;

struct MarkArgs {
  int32_t nrows, leave;  // leave: 1 leave-out, 0 folds
  uint64_t seed, F, f;
  int64_t h, m;
  const int64_t* ptr;
  const int32_t* ind;
  uint8_t* held;  // [nnz], cleared: 1 = held out
  int64_t* tcnt;  // [nrows + 1], cleared: tcnt[u + 1] = held entries of row u
};
struct ScatterArgs {
  int32_t nrows;
  const int64_t* sptr; const int32_t* sind; const float* sval;  // the source (sval nullptr: binary)
  const uint8_t* held;
  const int64_t* tptr;  // the test row pointer; the train row pointer is sptr - tptr
  int32_t* nind; float* nval;
  int32_t* tind; float* tval;
};

// a row of L entries can take part at all (the folds rule needs one entry inside and m outside)
__device__ __forceinline__ bool may_take_part(const MarkArgs& A, const int64_t L) {
  return A.leave ? L >= (int64_t)A.F * A.h + A.m : L >= A.m + 1;
}
__device__ __forceinline__ bool rec_before(const uint4 a, const uint4 b) {  // (key high, key low, item, position)
  return a.x != b.x ? a.x < b.x : a.y != b.y ? a.y < b.y : a.z != b.z ? a.z < b.z : a.w < b.w;
}

// ---- the mark pass -------------------------------------------------------------------------------------------------
// Short rows: lane `sub` of a group of 16 holds entry `sub`; the rank of an entry is the number of the row's entries
// before it in the order, counted over 16 shuffle rounds; the folds count is a 16-lane sum.
__global__ __launch_bounds__(256) void k_split_mark_short(const MarkArgs A) {
  const int sub = threadIdx.x & 15;
  const int64_t stride = (int64_t)gridDim.x * kSplitShortRowsPerBlock;
  // (every lane of a wavefront makes the same number of rounds: the shuffles below need them all)
  for (int64_t first = (int64_t)blockIdx.x * kSplitShortRowsPerBlock; first < A.nrows; first += stride) {
    const int64_t row = first + (threadIdx.x >> 4);
    int64_t r0 = 0, L = 0;
    if (row < A.nrows) {
      r0 = A.ptr[row];
      L = A.ptr[row + 1] - r0;
      if (L > kSplitShortRow || !may_take_part(A, L)) L = 0;
    }
    const bool active = sub < L;
    uint32_t item = 0xFFFFFFFFu;
    uint64_t key = ~0ull;
    if (active) {
      item = (uint32_t)A.ind[r0 + sub];
      key = sample_key(sample_base(A.seed, (uint64_t)row), (uint64_t)item);
    }
    bool held = false;
    int64_t out = 0;
    if (A.leave) {
      int rank = 0;
      for (int j = 0; j < 16; ++j) {
        const uint32_t ohi = __shfl((uint32_t)(key >> 32), j, 16), olo = __shfl((uint32_t)key, j, 16);
        const uint32_t oitem = __shfl(item, j, 16);
        const uint64_t okey = ((uint64_t)ohi << 32) | olo;
        const bool before = okey != key ? okey < key : oitem != item ? oitem < item : j < sub;
        rank += (j < L && before) ? 1 : 0;
      }
      held = active && rank >= (int64_t)A.f * A.h && rank < (int64_t)(A.f + 1) * A.h;
      out = L > 0 ? A.h : 0;
    } else {
      const int inside = active && sample_mulhi64(key, A.F) == A.f ? 1 : 0;
      int cnt = inside;
      for (int off = 8; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 16);
      const bool part = cnt >= 1 && L - cnt >= A.m;
      held = inside && part;
      out = part ? cnt : 0;
    }
    if (held) A.held[r0 + sub] = 1;
    if (sub == 0 && out > 0) A.tcnt[row + 1] = out;
  }
}

// the rows of a batch of NT that belong to the class (lo, hi] (and, in the mark pass, can take part), listed in LDS
template <int NT, class Keep>
__device__ __forceinline__ int list_rows(const int64_t first, const int32_t nrows, const int64_t* ptr, const int64_t lo,
                                         const int64_t hi, int32_t* list, int* nlist, Keep&& keep) {
  if (threadIdx.x == 0) *nlist = 0;
  __syncthreads();
  const int64_t row = first + threadIdx.x;
  if (row < nrows) {
    const int64_t L = ptr[row + 1] - ptr[row];
    if (L > lo && L <= hi && keep(L)) list[atomicAdd(nlist, 1)] = (int32_t)row;
  }
  __syncthreads();
  return *nlist;
}

// ascending bitonic sort of rec[0 .. n), n a power of two, by the whole workgroup; ends on a barrier
template <int NT>
__device__ __forceinline__ void split_sort(uint4* rec, const int n) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n >> 1); t += NT) {
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

// Wave and long rows: a workgroup of NT lanes per row, NT * EPT entries at once, CAP candidate records in LDS.
// Invariant of the leave-out selection: before a piece is read there is room for all of it (n + NT * EPT <= CAP);
// when there is not, the records are sorted, the K smallest kept, and the K-th becomes the bound.  A row that takes
// part has L >= K entries, and the K smallest of what was read so far are always among the records.
template <int NT, int EPT, int CAP>
__global__ __launch_bounds__(NT) void k_split_mark_team(const MarkArgs A, const int64_t lo, const int64_t hi) {
  static_assert(CAP >= NT * EPT + SLIMGPU_SPLIT_MAX_HELD && (CAP & (CAP - 1)) == 0, "room for a piece beside K records");
  __shared__ uint4 rec[CAP];
  __shared__ int32_t list[NT];
  __shared__ int nlist, nrec;
  __shared__ int wsum[NT / 64];
  const int t = threadIdx.x;
  for (int64_t first = (int64_t)blockIdx.x * NT; first < A.nrows; first += (int64_t)gridDim.x * NT) {
    const int nl = list_rows<NT>(first, A.nrows, A.ptr, lo, hi, list, &nlist,
                                 [&](const int64_t L) { return may_take_part(A, L); });
    for (int q = 0; q < nl; ++q) {
      const int32_t row = list[q];
      const int64_t r0 = A.ptr[row], L = A.ptr[row + 1] - r0;
      const uint64_t base = sample_base(A.seed, (uint64_t)row);
      if (A.leave) {
        const int K = (int)((A.f + 1) * A.h);
        // sorts the n records (padded to a power of two), keeps the K smallest; returns how many are kept
        auto compact = [&](const int n) {
          int P = 2;
          while (P < n) P <<= 1;
          for (int k = n + t; k < P; k += NT) rec[k] = make_uint4(~0u, ~0u, ~0u, ~0u);
          __syncthreads();
          split_sort<NT>(rec, P);
          return n < K ? n : K;
        };
        if (t == 0) nrec = 0;
        __syncthreads();
        int n = 0;
        bool bounded = false;
        uint4 bound = make_uint4(~0u, ~0u, ~0u, ~0u);
        for (int64_t p0 = 0; p0 < L; p0 += NT * EPT) {
          if (n + NT * EPT > CAP) {  // (n > K here, so the bound exists from now on)
            n = compact(n);
            bound = rec[K - 1];
            bounded = true;
            __syncthreads();  // (every lane has read the bound before a record may land on it)
            if (t == 0) nrec = n;
            __syncthreads();
          }
          for (int j = 0; j < EPT; ++j) {
            const int64_t p = p0 + (int64_t)j * NT + t;
            if (p < L) {
              const uint32_t item = (uint32_t)A.ind[r0 + p];
              const uint64_t key = sample_key(base, (uint64_t)item);
              const uint4 r = make_uint4((uint32_t)(key >> 32), (uint32_t)key, item, (uint32_t)p);
              if (!bounded || rec_before(r, bound)) rec[atomicAdd(&nrec, 1)] = r;
            }
          }
          __syncthreads();
          n = nrec;
          // (every wavefront has read the count before one of them appends to it again: n is the same in all of them,
          // and the barriers inside the branch above are reached by all or by none)
          __syncthreads();
        }
        n = compact(n);  // n >= K: the row has at least K entries
        for (int r = (int)(A.f * A.h) + t; r < K; r += NT) A.held[r0 + rec[r].w] = 1;
        if (t == 0) A.tcnt[row + 1] = A.h;
        __syncthreads();  // (the records are read before the next row clears them)
      } else {
        int cnt = 0;
        for (int64_t p = t; p < L; p += NT)
          if (sample_mulhi64(sample_key(base, (uint64_t)(uint32_t)A.ind[r0 + p]), A.F) == A.f) {
            A.held[r0 + p] = 1;
            ++cnt;
          }
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
        if ((t & 63) == 0) wsum[t >> 6] = cnt;
        __syncthreads();
        int64_t inside = 0;
        for (int w = 0; w < NT / 64; ++w) inside += wsum[w];
        const bool part = inside >= 1 && L - inside >= A.m;
        if (!part && inside > 0)  // the marks are taken back, each by the lane that made it
          for (int64_t p = t; p < L; p += NT)
            if (sample_mulhi64(sample_key(base, (uint64_t)(uint32_t)A.ind[r0 + p]), A.F) == A.f) A.held[r0 + p] = 0;
        if (t == 0 && part) A.tcnt[row + 1] = inside;
        __syncthreads();  // (wsum is read before the next row writes it)
      }
    }
    __syncthreads();  // (every lane has the batch's count before the next batch clears it)
  }
}

// ---- the scatter pass ----------------------------------------------------------------------------------------------
__global__ void k_split_train_ptr(const int32_t nrows, const int64_t* sptr, const int64_t* tptr, int64_t* nptr) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u <= nrows; u += (int64_t)gridDim.x * blockDim.x)
    nptr[u] = sptr[u] - tptr[u];
}

__device__ __forceinline__ void put_entry(const ScatterArgs& A, const int64_t src, const bool held, const int64_t ndst,
                                          const int64_t tdst) {
  const int32_t id = A.sind[src];
  if (held) A.tind[tdst] = id; else A.nind[ndst] = id;
  if (A.sval) {
    const float v = A.sval[src];
    if (held) A.tval[tdst] = v; else A.nval[ndst] = v;
  }
}

__global__ __launch_bounds__(256) void k_split_scatter_short(const ScatterArgs A) {
  const int sub = threadIdx.x & 15, lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * kSplitShortRowsPerBlock;
  for (int64_t first = (int64_t)blockIdx.x * kSplitShortRowsPerBlock; first < A.nrows; first += stride) {
    const int64_t row = first + (threadIdx.x >> 4);
    int64_t r0 = 0, L = 0, t0 = 0, tc = 0;
    if (row < A.nrows) {
      r0 = A.sptr[row];
      L = A.sptr[row + 1] - r0;
      if (L > kSplitShortRow) L = 0;
      t0 = A.tptr[row];
      tc = A.tptr[row + 1] - t0;
    }
    const bool active = sub < L;
    const bool held = active && tc > 0 && A.held[r0 + sub] != 0;
    const unsigned long long all = __ballot(held);  // (every lane of the wavefront is here)
    const uint32_t mine = (uint32_t)(all >> (lane & 48)) & 0xFFFFu;
    const int hp = __popc(mine & ((1u << sub) - 1u));
    if (active) put_entry(A, r0 + sub, held, (r0 - t0) + (sub - hp), t0 + hp);
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_split_scatter_team(const ScatterArgs A, const int64_t lo, const int64_t hi) {
  __shared__ int32_t list[NT];
  __shared__ int nlist;
  __shared__ int wsum[2][NT / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int flip = 0;
  for (int64_t first = (int64_t)blockIdx.x * NT; first < A.nrows; first += (int64_t)gridDim.x * NT) {
    const int nl = list_rows<NT>(first, A.nrows, A.sptr, lo, hi, list, &nlist, [](const int64_t) { return true; });
    for (int q = 0; q < nl; ++q) {
      const int32_t row = list[q];
      const int64_t r0 = A.sptr[row], L = A.sptr[row + 1] - r0;
      const int64_t t0 = A.tptr[row], tc = A.tptr[row + 1] - t0, n0 = r0 - t0;
      if (tc == 0) {  // nothing held: the row is copied
        for (int64_t p = t; p < L; p += NT) put_entry(A, r0 + p, false, n0 + p, 0);
        continue;
      }
      int64_t before = 0;  // held entries of the pieces behind
      for (int64_t p0 = 0; p0 < L; p0 += NT) {
        const int64_t p = p0 + t;
        const bool held = p < L && A.held[r0 + p] != 0;
        const unsigned long long mask = __ballot(held);
        int hp = __popcll(mask & below);
        int total = __popcll(mask);
        if (NT > 64) {
          if (lane == 0) wsum[flip][wave] = total;
          __syncthreads();
          total = 0;
          for (int w = 0; w < NT / 64; ++w) {
            if (w < wave) hp += wsum[flip][w];
            total += wsum[flip][w];
          }
          flip ^= 1;  // (the next piece writes the other half: one barrier per piece)
        }
        if (p < L) put_entry(A, r0 + p, held, n0 + (p - before - hp), t0 + before + hp);
        before += total;
      }
    }
    __syncthreads();  // (every lane has the batch's count before the next batch clears it)
  }
}

template <class T>
T* host_array(size_t n) {
  T* p = static_cast<T*>(std::malloc(sizeof(T) * (n ? n : 1)));
  if (!p) throw std::bad_alloc();
  return p;
}
}  // namespace

int32_t matrix_split(slimgpu_matrix_t* src, const slimgpu_split_t* split, slimgpu_matrix_t** trn_out,
                     slim_csr_t** tst_out) {
  const char* who = "SLIMGPU_MatrixSplit";
  DeviceCsrView R;
  if (!src || !trn_out || !tst_out || matrix_csr_view(src, &R) != SLIM_OK)
    return refuse(std::string(who) + ": bad arguments (a staged matrix, the two outputs)");
  if (const int32_t rc = split_check(who, split); rc != SLIM_OK) return rc;
  if (R.merged)
    return refuse(std::string(who) + ": the matrix was staged with SLIM_GPU_DUPLICATES=sum and repeated pairs were "
                  "merged: its rows are not the caller's");
  const auto wall0 = std::chrono::steady_clock::now();
  slimgpu_eval_stats_t st = {};
  st.path = SLIMGPU_EVAL_PATH_SPLIT;
  slimgpu_matrix_t* trn = nullptr;
  slim_csr_t* tst = nullptr;
  const int32_t rc = guarded(who, [&]() -> int32_t {
    hipStream_t stream = open_device(R);
    const int32_t nrows = R.nrows;
    const int64_t nnz = R.nnz;
    const size_t np = (size_t)nrows + 1;
    MarkArgs M = {};
    M.nrows = nrows; M.leave = split->mode == SLIMGPU_SPLIT_LEAVE_OUT;
    M.seed = split->seed; M.F = (uint64_t)split->nfolds; M.f = (uint64_t)split->fold;
    M.h = split->nheld; M.m = split->minkeep;
    M.ptr = R.d_ptr; M.ind = R.d_ind;
    DeviceBuffer<uint8_t> held((size_t)nnz);
    DeviceBuffer<int64_t> tcnt(np), tptr(np), nptr(np);
    st.device_allocs += 4;
    M.held = held.get(); M.tcnt = tcnt.get();
    HIP_TRY(hipMemsetAsync(held.get(), 0, (size_t)std::max<int64_t>(nnz, 1), stream));
    HIP_TRY(hipMemsetAsync(tcnt.get(), 0, sizeof(int64_t) * np, stream));
    // grids: what the rows need, capped; the rest is the grid-stride loop's
    auto blocks = [&](int rows_per_block, int per_cu) {
      return (unsigned)std::max<int64_t>(
          1, std::min<int64_t>(((int64_t)nrows + rows_per_block - 1) / rows_per_block, (int64_t)R.num_cus * per_cu));
    };
    const unsigned g_short = blocks(kSplitShortRowsPerBlock, 8), g_wave = blocks(64, 32), g_long = blocks(256, 8);
    EventPair ev, ev2;  // the mark pass with the scan, and the scatter pass: not the copy and the allocations between
    ev.begin(stream);
    if (nnz > 0) {
      hipLaunchKernelGGL(k_split_mark_short, dim3(g_short), dim3(256), 0, stream, M);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL((k_split_mark_team<64, 1, 256>), dim3(g_wave), dim3(64), 0, stream, M,
                         (int64_t)kSplitShortRow, (int64_t)kSplitWaveRow);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL((k_split_mark_team<256, kSplitLongPiece / 256, 2048>), dim3(g_long), dim3(256), 0, stream, M,
                         (int64_t)kSplitWaveRow, INT64_MAX);
      HIP_TRY(hipGetLastError());
    }
    size_t scan_bytes = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, scan_bytes, tcnt.get(), tptr.get(), np, rocprim::plus<int64_t>(), stream));
    DeviceBuffer<char> tmp(scan_bytes);
    ++st.device_allocs;
    HIP_TRY(rocprim::inclusive_scan(tmp.get(), scan_bytes, tcnt.get(), tptr.get(), np, rocprim::plus<int64_t>(),
                                    stream));
    hipLaunchKernelGGL(k_split_train_ptr, dim3(blocks(256, 8)), dim3(256), 0, stream, nrows, R.d_ptr, tptr.get(),
                       nptr.get());
    HIP_TRY(hipGetLastError());
    ev.end(stream);
    // the test row pointer comes down: its last entry sizes the four output arrays
    struct HostHalf {  // (the arrays of the test matrix until the handle takes them)
      ssize_t* ptr = nullptr; int32_t* ind = nullptr; float* val = nullptr;
      ~HostHalf() { std::free(ptr); std::free(ind); std::free(val); }
    } H;
    static_assert(sizeof(ssize_t) == sizeof(int64_t), "LP64 expected");
    H.ptr = host_array<ssize_t>(np);
    HIP_TRY(hipMemcpyAsync(H.ptr, tptr.get(), sizeof(int64_t) * np, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    st.d2h_bytes += (int64_t)(sizeof(int64_t) * np);
    const int64_t nt = H.ptr[nrows];
    if (nt < 0 || nt > nnz) throw HipFail{hipErrorUnknown, "the test row pointer"};
    const int64_t nk = nnz - nt;
    const bool binary = R.d_val == nullptr;
    DeviceBuffer<int32_t> nind((size_t)nk), tind((size_t)nt);
    DeviceBuffer<float> nval, tval;
    st.device_allocs += 2;
    if (!binary) {
      nval = DeviceBuffer<float>((size_t)nk);
      tval = DeviceBuffer<float>((size_t)nt);
      st.device_allocs += 2;
    }
    ev2.begin(stream);
    if (nnz > 0) {
      ScatterArgs S = {};
      S.nrows = nrows; S.sptr = R.d_ptr; S.sind = R.d_ind; S.sval = R.d_val; S.held = held.get(); S.tptr = tptr.get();
      S.nind = nind.get(); S.nval = nval.get(); S.tind = tind.get(); S.tval = tval.get();
      hipLaunchKernelGGL(k_split_scatter_short, dim3(g_short), dim3(256), 0, stream, S);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_split_scatter_team<64>, dim3(g_wave), dim3(64), 0, stream, S, (int64_t)kSplitShortRow,
                         (int64_t)kSplitWaveRow);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_split_scatter_team<256>, dim3(g_long), dim3(256), 0, stream, S, (int64_t)kSplitWaveRow,
                         INT64_MAX);
      HIP_TRY(hipGetLastError());
    }
    ev2.end(stream);
    // the test half: 4 (binary) or 8 bytes per held-out entry
    H.ind = host_array<int32_t>((size_t)nt);
    if (!binary) H.val = host_array<float>((size_t)nt);
    if (nt > 0) {
      HIP_TRY(hipMemcpyAsync(H.ind, tind.get(), sizeof(int32_t) * (size_t)nt, hipMemcpyDeviceToHost, stream));
      st.d2h_bytes += (int64_t)(sizeof(int32_t) * (size_t)nt);
      if (!binary) {
        HIP_TRY(hipMemcpyAsync(H.val, tval.get(), sizeof(float) * (size_t)nt, hipMemcpyDeviceToHost, stream));
        st.d2h_bytes += (int64_t)(sizeof(float) * (size_t)nt);
      }
    }
    HIP_TRY(hipStreamSynchronize(stream));  // (the train arrays are complete before another stream stages them)
    st.kernel_ms = ev.ms() + ev2.ms();
    tst = csr_new();
    if (!tst) throw std::bad_alloc();
    tst->nrows = nrows;
    tst->ncols = max_index_plus_one(nt, H.ind);
    tst->rowptr = H.ptr; tst->rowind = H.ind; tst->rowval = H.val;
    H.ptr = nullptr; H.ind = nullptr; H.val = nullptr;
    // the train half is staged where it lies, as SLIMGPU_MatrixFromDevice stages borrowed arrays; the handle then
    // takes them over.  (The staging reads the entry count and the largest id for itself: 12 bytes down.)
    // The source's staging options: of LearnOptions, matrix_from_device reads the device alone (pick_device), and a
    // handle keeps no other option of its staging; the day staging reads another one, it has to travel here too.
    LearnOptions o;
    o.device = R.device;
    int32_t status = SLIM_ERROR;
    trn = matrix_from_device(nrows, 0, nptr.get(), nind.get(), binary ? nullptr : nval.get(), o, &status);
    if (!trn) return status;
    matrix_adopt_csr(trn);
    nptr.release(); nind.release(); nval.release();
    st.d2h_bytes += 12;
    return SLIM_OK;
  });
  if (rc != SLIM_OK) {
    csr_free(tst);
    return rc;
  }
  st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  last_eval_stats() = st;
  *trn_out = trn;
  *tst_out = tst;
  return SLIM_OK;
}

}  // namespace slimamd

extern "C" int32_t SLIMGPU_MatrixSplit(slimgpu_matrix_t* src, const slimgpu_split_t* split, slimgpu_matrix_t** trn,
                                       slim_t** tst) {
  slimamd::set_error("");
  slim_csr_t* t = nullptr;
  const int32_t rc = slimamd::matrix_split(src, split, trn, &t);
  if (rc == SLIM_OK) *tst = t;
  return rc;
}
