// exposure.hip -- slim_gpu_exposure.h on a device: how often every item stands in the top-N lists.  The lists are
// where a scorer left them (ScorerWorkspace::oid / ocnt) or were uploaded for the call; only the counters come down.
//
// One add per place, whatever the number of cutoffs: place p adds to the counter of its band
// b(p) = min{k : p < c_k}; k_exposure_cumulate then turns bands into E_k = B_0 + .. + B_k.
//
// No global atomic per place.  A recommender's lists are the worst shape for them: the ids of one wave-instruction
// lie in 64 different rows, and a handful of head items sit in a large share of all lists.  MI355X_MICROARCH
// (Global float atomics) prices those two at about 0.08 TB/s of added bytes and another 14x slower; that is
// measured for float adds, integer adds are unmeasured and taken to be no better.  So the counters live in LDS: the
// grid is (window of item ids) x (share of the positions), a workgroup walks its share of the id rows with 16-byte
// loads, counts the places whose id falls into its window with ds_add_u32 and, at its end, adds every non-zero
// counter to global memory once.  The lists are read once per window, out of L2 / Infinity Cache: 4 bytes a place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "call_frame.hpp"
#include "host_csr.hpp"

namespace slimamd {
namespace {
constexpr int kExpoThreads = 1024;
constexpr size_t kExpoLdsBudget = 128 * 1024;  // of the CU's 160 KB; above 64 KB it is asked for (launch below)

struct ExposureArgs {
  const int32_t* ids; const int32_t* cnt;  // [npos][N], [npos] (nullptr: N places each)
  int64_t npos;
  int32_t N, ncols, K;
  int32_t window;   // item ids per window; LDS: K * window band counters, then K for the ids outside [0, ncols)
  int32_t rows;     // positions per share, a multiple of 4 (16-byte loads) with rows * N < 2^31
  int32_t last;     // c[K - 1]: places at or beyond it add nothing
  int32_t t[SLIMGPU_MAX_CUTOFFS - 1];  // c[0 .. K - 2], INT_MAX beyond: band = #{k : p >= t[k]} (constant indices only)
  uint32_t* bands;              // [K][ncols]
  unsigned long long* outside;  // [K]
};

__global__ __launch_bounds__(kExpoThreads) void k_exposure_bands(const ExposureArgs A) {
  extern __shared__ uint32_t s_cnt[];
  const int tid = threadIdx.x;
  const int w0 = (int)blockIdx.x * A.window;
  const uint32_t wn = (uint32_t)min(A.window, A.ncols - w0);
  const int nctr = A.K * A.window + A.K;
  for (int i = tid; i < nctr; i += kExpoThreads) s_cnt[i] = 0u;
  __syncthreads();
  const int64_t q0 = (int64_t)blockIdx.y * A.rows;
  const int64_t q1 = min(A.npos, q0 + (int64_t)A.rows);
  if (q0 < q1) {
    const int32_t* __restrict__ base = A.ids + q0 * (int64_t)A.N;
    const int32_t* __restrict__ cnt = A.cnt ? A.cnt + q0 : nullptr;
    const uint32_t N = (uint32_t)A.N;
    const uint32_t total = (uint32_t)((q1 - q0) * (int64_t)A.N);
    const bool tally_outside = blockIdx.x == 0;
    // place p of row r (of this share) holds id
    auto place = [&](const uint32_t r, const int p, const int id) {
      if (p >= A.last) return;
      if (cnt && p >= cnt[r]) return;
      int b = 0;
#pragma unroll
      for (int k = 0; k < SLIMGPU_MAX_CUTOFFS - 1; ++k) b += p >= A.t[k] ? 1 : 0;
      const uint32_t j = (uint32_t)id - (uint32_t)w0;
      if (j < wn) atomicAdd(&s_cnt[b * A.window + (int)j], 1u);
      else if (tally_outside && (uint32_t)id >= (uint32_t)A.ncols) atomicAdd(&s_cnt[A.K * A.window + b], 1u);
    };
    const uint32_t nvec = total >> 2;
    const int4* __restrict__ vbase = reinterpret_cast<const int4*>(base);
    for (uint32_t v = tid; v < nvec; v += kExpoThreads) {
      const int4 x = vbase[v];
      uint32_t r = (4u * v) / N;
      uint32_t p = 4u * v - r * N;
      const int id[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        place(r, (int)p, id[e]);
        if (++p == N) { p = 0; ++r; }
      }
    }
    for (uint32_t e = 4u * nvec + tid; e < total; e += kExpoThreads) {  // (the last share's last places)
      const uint32_t r = e / N;
      place(r, (int)(e - r * N), base[e]);
    }
  }
  __syncthreads();
  const bool alone = gridDim.y == 1;  // the window is this workgroup's: no atomic needed
  for (int i = tid; i < A.K * A.window; i += kExpoThreads) {
    const uint32_t v = s_cnt[i];
    if (v == 0u) continue;
    const int b = i / A.window;
    uint32_t* dst = A.bands + (size_t)b * (size_t)A.ncols + (size_t)(w0 + (i - b * A.window));
    if (alone) *dst += v; else atomicAdd(dst, v);
  }
  if (blockIdx.x == 0 && tid < A.K) {
    const uint32_t v = s_cnt[A.K * A.window + tid];
    if (v) atomicAdd(A.outside + tid, (unsigned long long)v);
  }
}

__global__ __launch_bounds__(256) void k_exposure_cumulate(const int32_t ncols, const int32_t K,
                                                           uint32_t* __restrict__ E,
                                                           unsigned long long* __restrict__ outside) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ncols; i += (int64_t)gridDim.x * 256) {
    uint32_t run = E[i];
    for (int k = 1; k < K; ++k) {
      run += E[(size_t)k * (size_t)ncols + (size_t)i];
      E[(size_t)k * (size_t)ncols + (size_t)i] = run;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int k = 1; k < K; ++k) outside[k] += outside[k - 1];
}

// SLIM_EXPOSURE_WINDOW=<ids>: at most so many item ids per LDS window (tests put window edges inside small catalogues)
int32_t window_cap() {
  const char* s = std::getenv("SLIM_EXPOSURE_WINDOW");
  if (!s || !*s) return INT_MAX;
  char* end = nullptr;
  const long v = std::strtol(s, &end, 10);
  return (*end || v < 1) ? INT_MAX : (int32_t)std::min<long>(v, INT_MAX);
}
}  // namespace

void queue_exposure_clear(hipStream_t stream, int32_t ncols, const Cutoffs& cut, ScorerWorkspace& ws) {
  const size_t n = (size_t)cut.n * (size_t)ncols;
  ws.need(ws.expo, n);
  ws.need(ws.expo_out, SLIMGPU_MAX_CUTOFFS);
  HIP_TRY(hipMemsetAsync(ws.expo.get(), 0, sizeof(uint32_t) * n, stream));
  HIP_TRY(hipMemsetAsync(ws.expo_out.get(), 0, sizeof(unsigned long long) * SLIMGPU_MAX_CUTOFFS, stream));
}

void queue_exposure_count(hipStream_t stream, int num_cus, const int32_t* ids, const int32_t* cnt, int64_t npos,
                          int32_t N, int32_t ncols, const Cutoffs& cut, ScorerWorkspace& ws) {
  if (npos <= 0) return;
  const int K = cut.n;
  ExposureArgs A{};
  A.ids = ids; A.cnt = cnt; A.npos = npos; A.N = N; A.ncols = ncols; A.K = K;
  A.last = cut.c[K - 1];
  for (int k = 0; k < SLIMGPU_MAX_CUTOFFS - 1; ++k) A.t[k] = k < K - 1 ? cut.c[k] : INT_MAX;
  A.bands = ws.expo.get(); A.outside = ws.expo_out.get();
  // the window: what the LDS budget holds of K counters per id, the whole catalogue when that fits
  const size_t fit = (kExpoLdsBudget - sizeof(uint32_t) * (size_t)K) / (sizeof(uint32_t) * (size_t)K);
  A.window = (int32_t)std::min<size_t>({fit, (size_t)ncols, (size_t)window_cap()});
  const size_t lds = sizeof(uint32_t) * ((size_t)K * (size_t)A.window + (size_t)K);
  const int64_t nwin = ((int64_t)ncols + A.window - 1) / A.window;
  // the shares: enough workgroups to fill the CUs (two of 16 wavefronts where the LDS allows), at least 16K places
  // each, rows in multiples of 4 and less than 2^31 places
  const int per_cu = lds * 2 + 128 <= 160 * 1024 ? 2 : 1;
  const int64_t want = std::max<int64_t>(1, ((int64_t)num_cus * per_cu + nwin - 1) / nwin);
  auto up4 = [](int64_t v) { return (v + 3) / 4 * 4; };
  int64_t rows = std::max(up4((npos + want - 1) / want), up4((16384 + N - 1) / N));
  rows = std::max<int64_t>(4, std::min<int64_t>(rows, ((int64_t)INT_MAX / N) / 4 * 4));
  const int64_t nshare = (npos + rows - 1) / rows;
  if (nwin > INT_MAX || nshare > 65535) throw HipFail{hipErrorInvalidValue, "exposure: the grid does not fit a launch"};
  A.rows = (int32_t)rows;
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_exposure_bands),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_exposure_bands, dim3((unsigned)nwin, (unsigned)nshare), dim3(kExpoThreads), lds, stream, A);
  HIP_TRY(hipGetLastError());
}

void queue_exposure_cumulate(hipStream_t stream, int num_cus, int32_t ncols, const Cutoffs& cut, ScorerWorkspace& ws) {
  if (cut.n < 2) return;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)ncols + 255) / 256, (int64_t)num_cus * 8));
  hipLaunchKernelGGL(k_exposure_cumulate, dim3(blocks), dim3(256), 0, stream, ncols, cut.n, ws.expo.get(),
                     ws.expo_out.get());
  HIP_TRY(hipGetLastError());
}

size_t fetch_exposure(hipStream_t stream, int32_t ncols, const Cutoffs& cut, const ScorerWorkspace& ws,
                      std::vector<uint32_t>& h_E, const uint32_t* pop, const int32_t* fmarker, int32_t fm_ncols,
                      int64_t nlists, bool engine_lists, uint32_t* exposure, slimgpu_exposure_t* summary) {
  const size_t n = (size_t)cut.n * (size_t)ncols;
  if (h_E.size() < n) h_E.resize(n);
  unsigned long long outside[SLIMGPU_MAX_CUTOFFS] = {};
  size_t down = 0;
  if (nlists > 0) {
    HIP_TRY(hipMemcpyAsync(h_E.data(), ws.expo.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost, stream));
    down = sizeof(uint32_t) * n;
    if (!engine_lists) {
      HIP_TRY(hipMemcpyAsync(outside, ws.expo_out.get(), sizeof(unsigned long long) * (size_t)cut.n,
                             hipMemcpyDeviceToHost, stream));
      down += sizeof(unsigned long long) * (size_t)cut.n;
    }
    HIP_TRY(hipStreamSynchronize(stream));
  } else {
    std::fill(h_E.begin(), h_E.begin() + (ptrdiff_t)n, 0u);
  }
  if (exposure) std::copy(h_E.begin(), h_E.begin() + (ptrdiff_t)n, exposure);
  for (int32_t k = 0; summary && k < cut.n; ++k)
    exposure_summary(ncols, pop, fmarker, fm_ncols, nlists, h_E.data() + (size_t)k * (size_t)ncols,
                     (int64_t)outside[k], &summary[k]);
  return down;
}

// SLIMGPU_MatrixListExposure: a caller's lists uploaded in slices of at most 256 MB and counted on mat's device
int32_t matrix_list_exposure(slimgpu_matrix_t* mat, const int32_t* fmarker, int32_t fm_ncols, int64_t nlists,
                             int32_t nrcmds, const int32_t* ids, const int32_t* counts, int32_t ncutoffs,
                             const int32_t* cutoffs, uint32_t* exposure, slimgpu_exposure_t* summary) {
  const char* who = "SLIMGPU_MatrixListExposure";
  DeviceCsrView R;
  if (!mat || matrix_csr_view(mat, &R) != SLIM_OK) return refuse(std::string(who) + ": needs a staged matrix");
  if (const int32_t rc = exposure_lists_check(who, R.ncols, nlists, nrcmds, ids, counts, ncutoffs, cutoffs);
      rc != SLIM_OK)
    return rc;
  if (R.merged)
    return refuse(std::string(who) + ": the matrix was staged with SLIM_GPU_DUPLICATES=sum and repeated pairs were "
                  "merged: its column counts are not the caller's");
  if (fmarker && fm_ncols < 0) return refuse(std::string(who) + ": fm_ncols must be at least 0");
  if (nrcmds > (1 << 24))  // (a share of the kernel is at least 4 rows and fewer than 2^31 places)
    return refuse(std::string(who) + ": rows of more than 2^24 places are counted on the host only (SLIMGPU_ListExposure)");
  Cutoffs cut = {};
  cut.n = ncutoffs;
  for (int32_t k = 0; k < ncutoffs; ++k) cut.c[k] = cutoffs[k];
  return guarded(who, [&]() -> int32_t {
    hipStream_t stream = open_device(R);
    std::vector<int64_t> cp((size_t)R.ncols + 1);
    if (matrix_get_column_view(mat, cp.data(), nullptr, nullptr, nullptr) != SLIM_OK) return SLIM_ERROR;
    std::vector<uint32_t> pop((size_t)R.ncols);
    for (int32_t i = 0; i < R.ncols; ++i) pop[(size_t)i] = (uint32_t)(cp[(size_t)i + 1] - cp[(size_t)i]);
    ScorerWorkspace ws;
    if (nlists > 0) queue_exposure_clear(stream, R.ncols, cut, ws);
    const int64_t step = std::max<int64_t>(4, ((int64_t)64 << 20) / nrcmds / 4 * 4);  // 64 M ids a slice
    const int64_t held = std::min(step, nlists);
    DeviceBuffer<int32_t> d_ids((size_t)held * (size_t)nrcmds), d_cnt((size_t)held);
    for (int64_t s0 = 0; s0 < nlists; s0 += step) {
      const int64_t n = std::min(step, nlists - s0);
      HIP_TRY(hipMemcpyAsync(d_ids.get(), ids + s0 * (int64_t)nrcmds, sizeof(int32_t) * (size_t)n * (size_t)nrcmds,
                             hipMemcpyHostToDevice, stream));
      if (counts)
        HIP_TRY(hipMemcpyAsync(d_cnt.get(), counts + s0, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, stream));
      queue_exposure_count(stream, R.num_cus, d_ids.get(), counts ? d_cnt.get() : nullptr, n, nrcmds, R.ncols, cut, ws);
      if (s0 + step < nlists) HIP_TRY(hipStreamSynchronize(stream));  // (the next slice takes the same buffers)
    }
    if (nlists > 0) queue_exposure_cumulate(stream, R.num_cus, R.ncols, cut, ws);
    std::vector<uint32_t> h_E;
    fetch_exposure(stream, R.ncols, cut, ws, h_E, pop.data(), fmarker, fm_ncols, nlists, /*engine_lists=*/false, exposure,
                   summary);
    return SLIM_OK;
  });
}
}  // namespace slimamd
