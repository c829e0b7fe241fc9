// engine.hip -- HBM staging of the training matrix and the CD solve driver.
//
// Staging is the device form of CreateTrainingMatrix
// (/root/reference/src/libslim/setup.c:109-135): the caller's CSR is copied to
// HBM once (or adopted if it already lives there), the column view is built by
// a stable radix sort on the item id (keeps user ids ascending inside every
// column, which is what gk_csr_CreateIndex + slim_csr_SortIndices guarantee,
// setup.c:128,132), and the column norms are reduced one wavefront per column
// (gk_csr_ComputeNorms, setup.c:130).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <numeric>
#include <memory>
#include <string>
#include <thread>

#include <rocprim/device/device_radix_sort.hpp>

#include "tile_inst.hpp"
#include "gram_inst.hpp"
#include "gramr_inst.hpp"
#include "gram_sym.hpp"
#include "fslim_gram_inst.hpp"
#include "cd_wave.hpp"
#include "engine.hpp"
#include "hip_check.hpp"
#include "host_csr.hpp"

// ---- the opaque handle ---------------------------------------------------------
inline uint64_t slimgpu_next_uid() {
  static std::atomic<uint64_t> n{0};
  return ++n;
}

using slimamd::DeviceBuffer;

// user ranges of equal nnz and the slice boundaries of every column over them (ensure_split)
struct UserSplit {
  DeviceBuffer<int32_t> ubounds;  // [nranges + 1]
  DeviceBuffer<int64_t> csplit;   // [ncols][nranges + 1]
  int32_t nranges = 0, max_rows = 0;
};

struct slimgpu_matrix {
  const uint64_t uid = slimgpu_next_uid();  // (a handle's identity beyond its address)
  int device = 0;
  hipStream_t stream = nullptr;
  int32_t nrows = 0, ncols = 0;
  int64_t nnz = 0;
  bool binary = false;
  bool owns_csr = false;
  bool exact_gram = false;  // ratings are not small integers: aTy sums formed in a fixed order
  bool nonpositive = false;  // some rating is <= 0: a co-rating sum can cancel to exactly 0
  bool merged = false;  // SLIM_GPU_DUPLICATES=sum merged repeated pairs: the rows are no longer the caller's
  // CSR (the caller's of SLIMGPU_MatrixFromDevice unless owns_csr)
  int64_t* d_rowptr = nullptr;
  int32_t* d_rowind = nullptr;
  float* d_rowval = nullptr;
  // CSC + per-column scalars
  DeviceBuffer<int64_t> d_colptr;
  DeviceBuffer<int32_t> d_colind;
  DeviceBuffer<float> d_colval, d_cnorm, d_csq;
  std::vector<int64_t> h_cost;  // scheduling proxy per column (Gram work G)
  std::vector<int64_t> h_rowptr;  // host copy, fetched on first clustered solve
  // column slice boundaries for tile clusters of size K (index log2 K), built on demand
  UserSplit split[6];
  // the G builder's user passes (learn_cd, gram_passes): 32 * np user ranges of equal nnz
  UserSplit gsplit;
  double setup_ms = 0;
  int num_cus = 256;
  // copies of this matrix on other devices of the node (multi_gpu.cpp); owned by this handle
  std::vector<slimgpu_matrix*> replicas;
  // workspace reused by successive solves (grow-only, DeviceBuffer::reserve)
  // screen sums (a_i . y for every column i and every item of a tile) of the most recent tile
  // solve, reusable by the next solve of the same columns in the same geometry (model-selection
  // grids: slim_mselect.c:99-113 solves every (l1, l2) pair over the same R)
  DeviceBuffer<float> ws_gram;
  std::vector<int32_t> gram_order;  // work list the sums belong to (empty: none recorded)
  int gram_geom[6] = {0, 0, 0, 0, 0, 0};  // tileP, K, K_hi, nheavy, shard count, shard index
  // G = R^T R (item-space CD, cd_gram.hpp): [ncols][G_ld] floats, built on the first solve that
  // takes that path and kept with the handle
  DeviceBuffer<float> ws_G;
  DeviceBuffer<int32_t> ws_nunion;
  int64_t G_ld = 0;
  bool G_ready = false;
  double G_build_ms = 0, G_alloc_ms = 0, G_sums_ms = 0, G_sums_kernel_ms = 0, G_pack_ms = 0;
  // G as byte planes in popularity order (gram_pack.hpp), what cd_gramr.hpp streams: built from
  // the float G right after it, when every entry is a non-negative integer below 2^24
  DeviceBuffer<uint8_t> ws_Glo, ws_Ghi, ws_Gbase;
  DeviceBuffer<float> ws_Gdiag;
  DeviceBuffer<uint4> ws_Gmeta;
  DeviceBuffer<int64_t> ws_hioff, ws_hi2off;
  DeviceBuffer<int32_t> ws_hik, ws_hi2k, ws_rankof, ws_itemof;
  int64_t Gp_ldb = 0, Gp_pool_bytes = 0;
  int32_t Gp_nchunks = 0;
  bool Gp_ready = false, Gp_tried = false;
  bool Gf_dropped = false;          // the floats of G were freed once the planes stood (drop_float_gram)
  double Gp_bytes_per_row = 0;      // average bytes of a packed row (lo + hi + hi2)
  int expect_solves = 0;            // announced by the caller (model-selection grids)
  std::vector<int32_t> last_order;  // work list of the most recent solve
  DeviceBuffer<int32_t> ws_order, ws_cnt, ws_stat_i, ws_misc, ws_arena_i, ws_ulist;
  DeviceBuffer<int64_t> ws_off, ws_stat_l, ws_icolptr;
  DeviceBuffer<float> ws_stat_f, ws_arena_v, ws_slab, ws_xslab, ws_part, ws_icolval;
  // item-space FSLIM (cd_fslim_gram.hpp): the neighbour lists of a slice of the work list
  DeviceBuffer<int32_t> ws_fn, ws_fid, ws_fslot;
  DeviceBuffer<float> ws_faty;
  DeviceBuffer<uint64_t> ws_trace;
  // the G builder's view of the column ids (build_gview): lives for one build
  DeviceBuffer<uint4> ws_gview;
  DeviceBuffer<int64_t> ws_gvbase;
  DeviceBuffer<int32_t> ws_gvrows;
  DeviceBuffer<uint16_t> ws_gvcnt;
  DeviceBuffer<unsigned long long> ws_mailbox;
  DeviceBuffer<int32_t> ws_icolind;
  // the row view of a resident model (transpose_on_device)
  DeviceBuffer<uint32_t> ws_tkeys[2];
  DeviceBuffer<uint64_t> ws_tpay[2];
  DeviceBuffer<uint8_t> ws_ttmp;

  ~slimgpu_matrix() {
    (void)hipSetDevice(device);
    if (owns_csr) {
      (void)hipFree(d_rowptr);
      (void)hipFree(d_rowind);
      (void)hipFree(d_rowval);
    }
  }
};

// A learned model resident in HBM (SLIMGPU_LearnResident): the column view as SaveModel lays it out
// (estimate.c:570-593; ids ascending in every column) and the row view, formed on the device.
struct slimgpu_model {
  int device = 0;
  int32_t n = 0;      // nrows = ncols of W
  int64_t nnz = 0;
  // facts of the row view, found on the device when it is built (k_row_facts): the scorers size
  // their discovery keys by the longest row and need ids ascending inside every row
  int32_t max_row = 0;
  bool rows_sorted = true;
  DeviceBuffer<int64_t> d_colptr, d_rowptr;
  DeviceBuffer<int32_t> d_colind, d_rowind;
  DeviceBuffer<float> d_colval, d_rowval;
  // g of every problem as the solve that produced this model left it (cd_gramr.hpp, g_save): the
  // next solve of the same problems on the same handle starts from it when only l2 moved (the same
  // l1 = the same active sets) instead of re-folding this model into g row by row.  The buffer travels
  // down the chain of a grid's models (the next solve updates it in place and takes it over).
  mutable DeviceBuffer<float> d_gsave;
  mutable bool gsave_valid = false;
  int64_t gsave_stride = 0;
  double gsave_l1 = 0;
  uint64_t gsave_owner = 0;  // uid of the matrix handle
  // a fetch to the host running beside the next solve (model_fetch_begin)
  std::thread fetcher;
  bool fetch_begun = false;
  slim_csr_t* fetched = nullptr;
  int32_t fetch_status = 0;
  std::string fetch_error;
  double fetch_ms = 0;

  ~slimgpu_model() { (void)hipSetDevice(device); }
};

namespace slimamd {

namespace {

thread_local slimgpu_stats_t g_stats;
thread_local ColumnStats g_colstats;

struct InputError {  // malformed caller data: SLIM_ERROR_INPUT
  std::string msg;
};

double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

void report(const HipFail& e, const char* what) {
  set_error(std::string(what) + ": HIP error '" + hipGetErrorString(e.code) + "' in " + e.where +
            " -- the SLIM CD path needs a gfx950 GPU; there is no CPU fallback");
}

void drop_screen_cache(slimgpu_matrix* m) {
  m->ws_gram.reset();
  m->gram_order.clear();
}

// the eviction rule of the handle's workspaces (DeviceBuffer::reserve): when the device is out of
// memory the screen-sum cache is given up -- it only saves a pass, nothing depends on it
auto evict_cache(slimgpu_matrix* m) {
  return [m] {
    if (!m->ws_gram.get()) return false;
    drop_screen_cache(m);
    return true;
  };
}

// ---- the G builder's view of the column ids (SolveArgs::gview) ------------------
// One wavefront per (user range, group of 64 work-list positions), lane = position.

// 16-byte pieces (8 ids) the block of (range, group) takes: every slice of the group / 8, rounded up (cnt,
// per position), summed
__global__ void k_gview_rows(const int32_t* __restrict__ order, int32_t nwork, const int64_t* __restrict__ csplit,
                             int32_t stride, int32_t ngroups, int32_t nblocks, int32_t* __restrict__ rows,
                             uint16_t* __restrict__ cnt) {
  const int b = (int)blockIdx.x * ((int)blockDim.x >> 6) + ((int)threadIdx.x >> 6);
  if (b >= nblocks) return;
  const int r = b / ngroups, pl = (b % ngroups) * 64 + ((int)threadIdx.x & 63);
  int len = 0;
  if (pl < nwork) {
    const int64_t* const c = csplit + (int64_t)order[pl] * stride + r;
    len = (int)(c[1] - c[0]);
  }
  int n = (len + 7) >> 3;
  cnt[(int64_t)b * 64 + (threadIdx.x & 63)] = (uint16_t)n;  // (a range holds fewer than 2^16 users)
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
  if ((threadIdx.x & 63) == 0) rows[b] = n;
}

// the blocks themselves: every lane walks its slice and stores its ids, relative to the range's first
// user, eight to a piece; the last piece of a slice is filled up with the sentinel.  Row c of a block
// holds piece c of every lane that has one, in lane order, and the rows follow each other without a
// gap (a wavefront store is up to 1 KB contiguous) -- cd_tile.hpp finds a piece the same way
__global__ void k_gview_fill(const int32_t* __restrict__ order, int32_t nwork, const int64_t* __restrict__ csplit,
                             int32_t stride, const int32_t* __restrict__ ubounds, const int32_t* __restrict__ ci,
                             int32_t ngroups, int32_t nblocks, const int64_t* __restrict__ base, uint32_t sentinel,
                             uint4* __restrict__ view) {
  const int b = (int)blockIdx.x * ((int)blockDim.x >> 6) + ((int)threadIdx.x >> 6);
  if (b >= nblocks) return;
  const int lane = (int)threadIdx.x & 63;
  const int r = b / ngroups, pl = (b % ngroups) * 64 + lane;
  const int64_t end = base[b + 1];
  const int32_t u0 = ubounds[r];
  int64_t cs = 0;
  int len = 0;
  if (pl < nwork) {
    const int64_t* const c = csplit + (int64_t)order[pl] * stride + r;
    cs = c[0];
    len = (int)(c[1] - cs);
  }
  int64_t at = base[b];  // the row's first piece
  for (int c = 0;; ++c) {
    const bool mine = 8 * c < len;
    const uint64_t who = __ballot(mine);
    if (who == 0ull) break;
    if (mine) {
      const int64_t slot = at + __popcll(who & ((1ull << lane) - 1ull));
      uint32_t id[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) id[j] = 8 * c + j < len ? (uint32_t)(ci[cs + 8 * c + j] - u0) : sentinel;
      if (slot < end)  // (always: base was summed from the same lengths)
        view[slot] = make_uint4(id[0] | (id[1] << 16), id[2] | (id[3] << 16), id[4] | (id[5] << 16),
                                id[6] | (id[7] << 16));
    }
    at += __popcll(who);
  }
}

// ---- staging kernels -----------------------------------------------------------

__global__ void k_max_index(const int32_t* __restrict__ ind, int64_t n, int32_t* out) {
  int32_t m = -1;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x)
    m = max(m, ind[k]);
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

// Input checks done while staging (the reference trusts its caller; a GPU kernel fed a
// malformed CSR corrupts memory instead of crashing cleanly).  Bits of the flag word:
constexpr int kBadRowptr = 1;   // rowptr not non-decreasing / not ending at nnz
constexpr int kBadColumn = 2;   // item id outside [0, ncols)
constexpr int kDupEntry = 4;    // the same (user, item) pair twice

// key = item id, payload = (user id << 32 | value bits); one wavefront per row
__global__ void k_pack_rows(int32_t nrows, int32_t ncols, int64_t nnz,
                            const int64_t* __restrict__ rowptr,
                            const int32_t* __restrict__ rowind,
                            const float* __restrict__ rowval, uint32_t* __restrict__ keys,
                            uint64_t* __restrict__ payload, int32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t u = wave; u < nrows; u += nwaves) {
    int64_t s = rowptr[u], e = rowptr[u + 1];
    if (s < 0 || e < s || e > nnz || (u == 0 && s != 0)) {
      if (lane == 0) atomicOr(flags, kBadRowptr);
      continue;  // never index with a bad offset
    }
    for (int64_t k = s + lane; k < e; k += 64) {
      if ((uint32_t)rowind[k] >= (uint32_t)ncols) atomicOr(flags, kBadColumn);
      keys[k] = (uint32_t)rowind[k];
      const uint32_t bits = rowval ? __float_as_uint(rowval[k]) : 0x3F800000u;
      payload[k] = ((uint64_t)(uint32_t)u << 32) | bits;
    }
  }
}

__global__ void k_unpack_cols(int64_t nnz, const uint64_t* __restrict__ payload,
                              int32_t* __restrict__ colind, float* __restrict__ colval) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nnz;
       k += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t p = payload[k];
    colind[k] = (int32_t)(p >> 32);
    if (colval) colval[k] = __uint_as_float((uint32_t)p);
  }
}

// after the stable sort a repeated (user, item) pair is two adjacent equal entries of a column
__global__ void k_check_dups(int64_t nnz, const uint32_t* __restrict__ keys,
                             const uint64_t* __restrict__ payload, int32_t* __restrict__ flags) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; k < nnz;
       k += (int64_t)gridDim.x * blockDim.x)
    if (keys[k] == keys[k - 1] && (payload[k] >> 32) == (payload[k - 1] >> 32))
      atomicOr(flags, kDupEntry);
}

// colptr from the sorted keys: entry k opens every column in (key[k-1], key[k]]
__global__ void k_col_offsets(int64_t nnz, int32_t ncols, const uint32_t* __restrict__ keys,
                              int64_t* __restrict__ colptr) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nnz;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lo = k == 0 ? 0 : (int64_t)keys[k - 1] + 1;
    const int64_t hi = k == nnz ? (int64_t)ncols : (int64_t)keys[k];
    for (int64_t c = lo; c <= hi; ++c) colptr[c] = k;
  }
}

// one wavefront per column: fp32 sum of squares, norm, and the Gram work G
__global__ void k_col_scalars(int32_t ncols, const int64_t* __restrict__ colptr,
                              const int32_t* __restrict__ colind,
                              const float* __restrict__ colval,
                              const int64_t* __restrict__ rowptr, float* __restrict__ csq,
                              float* __restrict__ cnorm, int64_t* __restrict__ cost,
                              int32_t* __restrict__ inexact) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t c = wave; c < ncols; c += nwaves) {
    const int64_t s = colptr[c], e = colptr[c + 1];
    float ss = 0.0f;
    int64_t g = 0;
    for (int64_t k = s + lane; k < e; k += 64) {
      const float v = colval ? colval[k] : 1.0f;
      ss += v * v;
      // float sums of products of small integers are exact in any order; anything else
      // (fractional ratings, huge values) must not be accumulated with float atomics
      if (v != rintf(v) || fabsf(v) > 2048.0f) atomicOr(inexact, 1);
      // (bit 1: a rating <= 0 -- co-rating sums can then cancel to 0, which matters to FSLIM's
      // candidate rule, neighbors.c:46-60)
      if (!(v > 0.0f)) atomicOr(inexact, 2);
      const int32_t u = colind[k];
      g += rowptr[u + 1] - rowptr[u];
    }
    for (int off = 32; off > 0; off >>= 1) {
      ss += __shfl_xor(ss, off);
      g += __shfl_xor(g, off);
    }
    if (lane == 0) {
      if (!colval) ss = (float)(e - s);
      if (!(ss < 16777216.0f)) atomicOr(inexact, 1);  // a dot product can reach |a_i||a_j|
      csq[c] = ss;
      cnorm[c] = sqrtf(ss);
      cost[c] = g;
    }
  }
}

// csplit[c][j] = first position of column c whose user id is >= ubounds[j]
__global__ void k_col_split(int32_t ncols, int32_t K, const int32_t* __restrict__ ubounds,
                            const int64_t* __restrict__ colptr,
                            const int32_t* __restrict__ colind, int64_t* __restrict__ csplit) {
  const int64_t n = (int64_t)ncols * (K + 1);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = (int32_t)(t / (K + 1)), j = (int32_t)(t % (K + 1));
    int64_t lo = colptr[c], hi = colptr[c + 1];
    if (j == K) {
      lo = hi;
    } else if (j > 0) {
      const int32_t ub = ubounds[j];
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (colind[mid] < ub) lo = mid + 1; else hi = mid;
      }
    }
    csplit[t] = lo;
  }
}

// one wavefront per column: the entries a launch left in its arena, into column order
__global__ void k_gather_columns(int32_t ncols, const int64_t* __restrict__ colptr,
                                 const int64_t* __restrict__ src_off, const int32_t* __restrict__ src_ind,
                                 const float* __restrict__ src_val, int32_t* __restrict__ colind,
                                 float* __restrict__ colval) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t c = wave; c < ncols; c += nwaves) {
    const int64_t d = colptr[c], n = colptr[c + 1] - d, s = src_off[c];
    for (int64_t k = lane; k < n; k += 64) {
      colind[d + k] = src_ind[s + k];
      colval[d + k] = src_val[s + k];
    }
  }
}


int grid_for(int64_t n, int block, int cap_blocks) {
  int64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap_blocks) g = cap_blocks;
  return (int)g;
}

void pick_device(slimgpu_matrix* m, const LearnOptions& opt) {
  (void)hipGetLastError();  // a failure of an earlier call must not be reported by this one
  int count = 0;
  HIP_TRY(hipGetDeviceCount(&count));
  if (count <= 0) throw HipFail{hipErrorNoDevice, "hipGetDeviceCount"};
  if (opt.device >= 0) {
    HIP_TRY(hipSetDevice(opt.device));
    m->device = opt.device;
  } else {
    HIP_TRY(hipGetDevice(&m->device));
  }
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, m->device));
  m->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
}

// The other view of a sparse matrix of n rows held as (ptr, ind, val), over the caller's sort
// buffers: key = id, payload = (source row << 32 | value), stable radix sort by key -- entries of a
// destination row keep the order of their source rows (ascending ids) -- then ind / val and the
// offsets of the ncols destination rows.  pack_entries flags a bad offset or id; dups (optional)
// flags repeated pairs after the sort.
struct SortBufs {
  uint32_t *keys_in, *keys_out;
  uint64_t *pay_in, *pay_out;
};

void pack_entries(slimgpu_matrix* m, int32_t n, int32_t ncols, int64_t nnz, const int64_t* ptr,
                  const int32_t* ind, const float* val, const SortBufs& b, int32_t* flags) {
  hipLaunchKernelGGL(k_pack_rows, dim3(grid_for((int64_t)n * 64, 256, m->num_cus * 16)), dim3(256), 0,
                     m->stream, n, ncols, nnz, ptr, ind, val, b.keys_in, b.pay_in, flags);
  HIP_TRY(hipGetLastError());
}

// tmp_for(bytes): the sort's temporary storage
template <class TmpFor>
void sort_entries(slimgpu_matrix* m, int32_t ncols, int64_t nnz, const SortBufs& b, TmpFor&& tmp_for,
                  int32_t* dups, int64_t* o_ptr, int32_t* o_ind, float* o_val) {
  hipStream_t st = m->stream;
  const int cap = m->num_cus * 16;
  unsigned bits = 1;
  while ((1ull << bits) < (unsigned long long)ncols) ++bits;
  size_t tmp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, b.keys_in, b.keys_out, b.pay_in, b.pay_out,
                                    (size_t)nnz, 0u, bits, st));
  void* tmp = tmp_for(tmp_bytes ? tmp_bytes : 1);
  HIP_TRY(rocprim::radix_sort_pairs(tmp, tmp_bytes, b.keys_in, b.keys_out, b.pay_in, b.pay_out,
                                    (size_t)nnz, 0u, bits, st));
  if (dups) {
    hipLaunchKernelGGL(k_check_dups, dim3(grid_for(nnz, 256, cap)), dim3(256), 0, st, nnz,
                       b.keys_out, b.pay_out, dups);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_unpack_cols, dim3(grid_for(nnz, 256, cap)), dim3(256), 0, st, nnz,
                     b.pay_out, o_ind, o_val);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_col_offsets, dim3(grid_for(nnz + 1, 256, cap)), dim3(256), 0, st, nnz,
                     ncols, b.keys_out, o_ptr);
  HIP_TRY(hipGetLastError());
}

// Build CSC + scalars from the device CSR of m (nrows/nnz/ncols already set).
void build_column_view(slimgpu_matrix* m) {
  hipStream_t st = m->stream;
  const int64_t nnz = m->nnz;
  m->d_colptr = DeviceBuffer<int64_t>((size_t)m->ncols + 1);
  // (+ 64 entries of slack: the G builder reads whole 128-byte lines of a column slice, cd_tile.hpp)
  m->d_colind = DeviceBuffer<int32_t>((size_t)nnz + 64);
  if (!m->binary) m->d_colval = DeviceBuffer<float>((size_t)nnz);
  m->d_cnorm = DeviceBuffer<float>((size_t)m->ncols);
  m->d_csq = DeviceBuffer<float>((size_t)m->ncols);
  DeviceBuffer<int64_t> d_cost((size_t)m->ncols);

  if (nnz > 0) {
    if (nnz > 0xFFFFFFF0ll) throw HipFail{hipErrorInvalidValue, "nnz >= 2^32 not supported"};
    DeviceBuffer<uint32_t> keys_in((size_t)nnz), keys_out((size_t)nnz);
    DeviceBuffer<uint64_t> pay_in((size_t)nnz), pay_out((size_t)nnz);
    const SortBufs b{keys_in.get(), keys_out.get(), pay_in.get(), pay_out.get()};
    DeviceBuffer<int32_t> d_flags(1);
    HIP_TRY(hipMemsetAsync(d_flags.get(), 0, sizeof(int32_t), st));
    pack_entries(m, m->nrows, m->ncols, nnz, m->d_rowptr, m->d_rowind, m->d_rowval, b, d_flags.get());
    int32_t h_flags = 0;
    HIP_TRY(hipMemcpyAsync(&h_flags, d_flags.get(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_flags)  // checked before the sort: its bit count assumes ids < ncols
      throw InputError{h_flags & kBadRowptr
                           ? "rowptr is not a non-decreasing offset array ending at nnz"
                           : "item id outside [0, ncols)"};
    DeviceBuffer<uint8_t> tmp;
    sort_entries(m, m->ncols, nnz, b, [&](size_t bytes) { return (tmp = DeviceBuffer<uint8_t>(bytes)).get(); },
                 d_flags.get(), m->d_colptr.get(), m->d_colind.get(), m->d_colval.get());
    HIP_TRY(hipMemcpyAsync(&h_flags, d_flags.get(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_flags & kDupEntry)
      // the reference walks duplicates as separate entries (norm from v1^2 + v2^2, dots from
      // v1 + v2): not a well-defined problem, and two lanes updating one residual race here
      throw InputError{"duplicate (user, item) entries in the rating matrix (SLIM_GPU_DUPLICATES=sum "
                       "merges them while a host matrix is staged)"};
  } else {
    HIP_TRY(hipMemsetAsync(m->d_colptr.get(), 0, sizeof(int64_t) * ((size_t)m->ncols + 1), st));
  }
  DeviceBuffer<int32_t> d_inexact(1);
  HIP_TRY(hipMemsetAsync(d_inexact.get(), 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(k_col_scalars, dim3(grid_for((int64_t)m->ncols * 64, 256, m->num_cus * 16)),
                     dim3(256), 0, st, m->ncols, m->d_colptr.get(), m->d_colind.get(), m->d_colval.get(),
                     m->d_rowptr, m->d_csq.get(), m->d_cnorm.get(), d_cost.get(), d_inexact.get());
  HIP_TRY(hipGetLastError());
  int32_t h_inexact = 0;
  HIP_TRY(hipMemcpyAsync(&h_inexact, d_inexact.get(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
  m->h_cost.resize((size_t)m->ncols);
  HIP_TRY(hipMemcpyAsync(m->h_cost.data(), d_cost.get(), sizeof(int64_t) * (size_t)m->ncols,
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  m->exact_gram = (h_inexact & 1) != 0;
  m->nonpositive = (h_inexact & 2) != 0;
}

// The other view of a square sparse matrix held as (ptr, ind, val) with n rows, on the device (the
// staging pass's steps): entries of a destination row keep the order of their source rows, i.e.
// ascending ids, the arrays csr_build_index (host_csr.cpp) forms.  The outputs are allocated here;
// temporaries live with the handle.
void transpose_on_device(slimgpu_matrix* m, int32_t n, int64_t nnz, const int64_t* d_ptr,
                         const int32_t* d_ind, const float* d_val, DeviceBuffer<int64_t>& o_ptr,
                         DeviceBuffer<int32_t>& o_ind, DeviceBuffer<float>& o_val) {
  o_ptr = DeviceBuffer<int64_t>((size_t)n + 1);
  o_ind = DeviceBuffer<int32_t>((size_t)std::max<int64_t>(nnz, 1));
  o_val = DeviceBuffer<float>((size_t)std::max<int64_t>(nnz, 1));
  if (nnz <= 0) {
    HIP_TRY(hipMemsetAsync(o_ptr.get(), 0, sizeof(int64_t) * ((size_t)n + 1), m->stream));
    return;
  }
  if (nnz > 0xFFFFFFF0ll) throw HipFail{hipErrorInvalidValue, "model nnz >= 2^32 not supported"};
  const auto evict = evict_cache(m);
  const SortBufs b{m->ws_tkeys[0].reserve((size_t)nnz, evict), m->ws_tkeys[1].reserve((size_t)nnz, evict),
                   m->ws_tpay[0].reserve((size_t)nnz, evict), m->ws_tpay[1].reserve((size_t)nnz, evict)};
  int32_t* d_flags = m->ws_misc.reserve(16, evict);  // (the solver's scalars: read back already)
  pack_entries(m, n, n, nnz, d_ptr, d_ind, d_val, b, d_flags);
  sort_entries(m, n, nnz, b, [&](size_t bytes) { return m->ws_ttmp.reserve(bytes, evict); }, nullptr,
               o_ptr.get(), o_ind.get(), o_val.get());
}

// user ranges of equal nnz + per-column slice boundaries over them, into the cache slot s: nr
// ranges (a cluster of K = nr members, or the G builder's np passes of 32).  even_share: the
// cluster form's boundaries (nnz / nr * j, integer); else nnz * j / nr in floating point.
void ensure_split(slimgpu_matrix* m, UserSplit& s, int nr, bool even_share) {
  if (s.nranges == nr) return;
  s.ubounds.reset();
  s.csplit.reset();
  s.nranges = 0;
  std::vector<int32_t> ub((size_t)nr + 1, 0);
  ub[(size_t)nr] = m->nrows;
  if (nr > 1) {
    if (m->h_rowptr.empty()) {
      m->h_rowptr.resize((size_t)m->nrows + 1);
      HIP_TRY(hipMemcpy(m->h_rowptr.data(), m->d_rowptr, sizeof(int64_t) * ((size_t)m->nrows + 1),
                        hipMemcpyDeviceToHost));
    }
    for (int j = 1; j < nr; ++j) {
      const int64_t want = even_share ? m->nnz / nr * j : (int64_t)((double)m->nnz / nr * j);
      ub[(size_t)j] = (int32_t)(std::lower_bound(m->h_rowptr.begin(), m->h_rowptr.end(), want) -
                                m->h_rowptr.begin());
      ub[(size_t)j] = std::min(std::max(ub[(size_t)j], ub[(size_t)j - 1]), m->nrows);
    }
  }
  int32_t mx = 1;
  for (int j = 0; j < nr; ++j) mx = std::max(mx, ub[(size_t)j + 1] - ub[(size_t)j]);
  s.max_rows = mx;
  s.ubounds = DeviceBuffer<int32_t>((size_t)nr + 1);
  HIP_TRY(hipMemcpy(s.ubounds.get(), ub.data(), sizeof(int32_t) * ((size_t)nr + 1), hipMemcpyHostToDevice));
  s.csplit = DeviceBuffer<int64_t>((size_t)m->ncols * ((size_t)nr + 1));
  hipLaunchKernelGGL(k_col_split, dim3(grid_for((int64_t)m->ncols * (nr + 1), 256, m->num_cus * 8)), dim3(256), 0,
                     m->stream, m->ncols, nr, s.ubounds.get(), m->d_colptr.get(), m->d_colind.get(),
                     s.csplit.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(m->stream));
  s.nranges = nr;
}

void ensure_cluster_split(slimgpu_matrix* m, int lg) { ensure_split(m, m->split[lg], 1 << lg, true); }

void destroy(slimgpu_matrix* m) {
  if (!m) return;
  for (slimgpu_matrix* r : m->replicas) destroy(r);
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;  // (~slimgpu_matrix frees the device arrays)
}

}  // namespace

slimgpu_stats_t& last_stats() { return g_stats; }
ColumnStats& last_column_stats() { return g_colstats; }

LearnOptions decode_options(const int32_t* io, const double* dopt) {
  LearnOptions o;
  auto geti = [&](int idx, int32_t def) { return (!io || io[idx] == -1) ? def : io[idx]; };
  auto getd = [&](int idx, double def) { return (!dopt || dopt[idx] == -1) ? def : dopt[idx]; };
  o.nthreads = geti(SLIM_OPTION_NTHREADS, 1);
  o.nnbrs = geti(SLIM_OPTION_NNBRS, 0);
  o.simtype = geti(SLIM_OPTION_SIMTYPE, SLIM_SIMTYPE_COS);
  o.dbglvl = geti(SLIM_OPTION_DBGLVL, 0);
  o.algo = geti(SLIM_OPTION_ALGO, SLIM_ALGO_CD);
  o.ordered = geti(SLIM_OPTION_ORDERED, 0);
  o.maxniters = geti(SLIM_OPTION_MAXNITERS, 10000);
  o.l1r = getd(SLIM_OPTION_L1R, 1.0);
  o.l2r = getd(SLIM_OPTION_L2R, 1.0);
  o.optTol = getd(SLIM_OPTION_OPTTOL, 1e-7);
  o.col_begin = geti(SLIM_OPTION_GPU_COLBEGIN, 0);
  o.col_end = geti(SLIM_OPTION_GPU_COLEND, -1);
  o.seed = (uint32_t)geti(SLIM_OPTION_GPU_SEED, 1);
  o.device = geti(SLIM_OPTION_GPU_DEVICE, -1);
  o.kernel = geti(SLIM_OPTION_GPU_KERNEL, SLIMGPU_KERNEL_AUTO);
  o.cluster = geti(SLIM_OPTION_GPU_CLUSTER, 0);
  o.heavy_tiles = geti(SLIM_OPTION_GPU_HEAVYTILES, -1);
  o.heavy_cluster = geti(SLIM_OPTION_GPU_HEAVYCLUSTER, 0);
  o.ngpus = std::max(1, geti(SLIM_OPTION_GPU_NGPUS, 1));
  o.shard_count = std::max(1, geti(SLIM_OPTION_GPU_SHARDCOUNT, 1));
  o.shard_index = geti(SLIM_OPTION_GPU_SHARDINDEX, 0);
  return o;
}

int32_t device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

namespace {
// A new handle filled by fill(m); on failure: the message (prefixed by who), the status, and the
// handle destroyed.
template <class Fill>
slimgpu_matrix_t* make_matrix(const char* who, int32_t* status, Fill&& fill) {
  slimgpu_matrix* m = nullptr;
  try {
    m = new slimgpu_matrix();
    fill(m);
    if (status) *status = SLIM_OK;
    return m;
  } catch (const HipFail& e) {
    report(e, who);
    if (status) *status = status_of(e);
  } catch (const InputError& e) {
    set_error(std::string(who) + ": " + e.msg);
    if (status) *status = SLIM_ERROR_INPUT;
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    if (status) *status = SLIM_ERROR_MEMORY;
  }
  destroy(m);
  return nullptr;
}
}  // namespace

slimgpu_matrix_t* matrix_from_host(int32_t nrows, const ssize_t* rowptr, const int32_t* rowind,
                                   const float* rowval, const LearnOptions& opt,
                                   int32_t* status) {
  if (nrows < 0 || !rowptr || (rowptr[nrows] > 0 && !rowind)) {
    set_error("SLIMGPU_MatrixFromHost: bad CSR arguments");
    if (status) *status = SLIM_ERROR_INPUT;
    return nullptr;
  }
  const double t0 = now_ms();
  // Repeated (user, item) pairs.  The reference copies them verbatim (setup.c:119-126) and then
  // treats them inconsistently -- the LAST value of a pair is the target y[u] (estimate.c:406-408),
  // dot products take both entries, the norm is v1^2 + v2^2 -- and two lanes updating one
  // residual would race here, so the engine rejects them (default) or, with
  // SLIM_GPU_DUPLICATES=sum, merges them before staging: the values of a pair are added
  // (an implicit-feedback matrix, rowval == NULL, keeps one entry and stays binary).
  std::vector<int64_t> mptr;
  std::vector<int32_t> mind;
  std::vector<float> mval;
  try {  // (host vectors of nnz entries: a failed allocation is SLIM_ERROR_MEMORY, not a terminate)
  if (const char* e = std::getenv("SLIM_GPU_DUPLICATES"); e && std::strcmp(e, "sum") == 0 && nrows > 0) {
    bool any = false;
    std::vector<std::pair<int32_t, float>> row;
    mptr.assign((size_t)nrows + 1, 0);
    mind.reserve((size_t)rowptr[nrows]);
    if (rowval) mval.reserve((size_t)rowptr[nrows]);
    for (int32_t u = 0; u < nrows; ++u) {
      const int64_t s0 = rowptr[u], e0 = rowptr[u + 1];
      row.clear();
      for (int64_t k = s0; k < e0; ++k) row.emplace_back(rowind[k], rowval ? rowval[k] : 1.0f);
      bool sorted = true;
      for (size_t k = 1; k < row.size(); ++k) sorted = sorted && row[k - 1].first < row[k].first;
      if (!sorted) {  // (strictly ascending rows hold no repeated pair and are copied as they are)
        std::stable_sort(row.begin(), row.end(),
                         [](const auto& a, const auto& b) { return a.first < b.first; });
        size_t w = 0;
        for (size_t k = 0; k < row.size(); ++k) {
          if (w > 0 && row[w - 1].first == row[k].first) {
            if (rowval) row[w - 1].second += row[k].second;
            any = true;
          } else {
            row[w++] = row[k];
          }
        }
        row.resize(w);
      }
      for (const auto& pr : row) {
        mind.push_back(pr.first);
        if (rowval) mval.push_back(pr.second);
      }
      mptr[(size_t)u + 1] = (int64_t)mind.size();
    }
    if (any) {  // stage the merged copy (rows now ascending by item id)
      rowptr = reinterpret_cast<const ssize_t*>(mptr.data());
      rowind = mind.data();
      if (rowval) rowval = mval.data();
    }
  }
  } catch (const std::bad_alloc&) {
    set_error("SLIMGPU_MatrixFromHost: out of host memory while merging repeated pairs");
    if (status) *status = SLIM_ERROR_MEMORY;
    return nullptr;
  }
  return make_matrix("SLIMGPU_MatrixFromHost", status, [&](slimgpu_matrix* m) {
    pick_device(m, opt);
    m->nrows = nrows;
    m->nnz = rowptr[nrows];
    m->binary = rowval == nullptr;
    m->merged = !mptr.empty() && rowptr == reinterpret_cast<const ssize_t*>(mptr.data());
    m->ncols = max_index_plus_one(m->nnz, rowind);  // setup.c:117
    if (m->ncols <= 0) m->ncols = 1;
    m->owns_csr = true;
    m->d_rowptr = DeviceBuffer<int64_t>((size_t)nrows + 1).release();
    m->d_rowind = DeviceBuffer<int32_t>((size_t)m->nnz).release();
    m->d_rowval = m->binary ? nullptr : DeviceBuffer<float>((size_t)m->nnz).release();
    static_assert(sizeof(ssize_t) == sizeof(int64_t), "LP64 expected");
    HIP_TRY(hipMemcpyAsync(m->d_rowptr, rowptr, sizeof(int64_t) * ((size_t)nrows + 1),
                           hipMemcpyHostToDevice, m->stream));
    if (m->nnz > 0) {
      HIP_TRY(hipMemcpyAsync(m->d_rowind, rowind, sizeof(int32_t) * (size_t)m->nnz,
                             hipMemcpyHostToDevice, m->stream));
      if (!m->binary)
        HIP_TRY(hipMemcpyAsync(m->d_rowval, rowval, sizeof(float) * (size_t)m->nnz,
                               hipMemcpyHostToDevice, m->stream));
    }
    build_column_view(m);
    m->setup_ms = now_ms() - t0;
  });
}

slimgpu_matrix_t* matrix_from_device(int32_t nrows, int32_t ncols, const int64_t* d_rowptr,
                                     const int32_t* d_rowind, const float* d_rowval,
                                     const LearnOptions& opt, int32_t* status) {
  if (nrows < 0 || !d_rowptr) {
    set_error("SLIMGPU_MatrixFromDevice: bad CSR arguments");
    if (status) *status = SLIM_ERROR_INPUT;
    return nullptr;
  }
  const double t0 = now_ms();
  return make_matrix("SLIMGPU_MatrixFromDevice", status, [&](slimgpu_matrix* m) {
    pick_device(m, opt);
    m->nrows = nrows;
    m->owns_csr = false;
    m->d_rowptr = const_cast<int64_t*>(d_rowptr);
    m->d_rowind = const_cast<int32_t*>(d_rowind);
    m->d_rowval = const_cast<float*>(d_rowval);
    m->binary = d_rowval == nullptr;
    HIP_TRY(hipMemcpy(&m->nnz, d_rowptr + nrows, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (ncols <= 0) {
      DeviceBuffer<int32_t> d_max(1);
      int32_t init = -1;
      HIP_TRY(hipMemcpy(d_max.get(), &init, sizeof(int32_t), hipMemcpyHostToDevice));
      if (m->nnz > 0) {
        hipLaunchKernelGGL(k_max_index, dim3(grid_for(m->nnz, 256, m->num_cus * 8)), dim3(256), 0,
                           m->stream, m->d_rowind, m->nnz, d_max.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(m->stream));
      }
      HIP_TRY(hipMemcpy(&init, d_max.get(), sizeof(int32_t), hipMemcpyDeviceToHost));
      ncols = init + 1;
    }
    m->ncols = ncols > 0 ? ncols : 1;
    build_column_view(m);
    m->setup_ms = now_ms() - t0;
  });
}

void matrix_free(slimgpu_matrix_t* m) { destroy(m); }

// A copy of a staged matrix on another device: the FINISHED views (CSR, CSC, column scalars) go
// device to device (hipMemcpyPeerAsync: over xGMI where the devices are peers), so the target
// neither sorts nor needs the 24 bytes per nnz of sort temporaries.  From one root the N - 1
// copies of a node run on N - 1 different links at once.
slimgpu_matrix_t* matrix_clone_to_device(const slimgpu_matrix_t* src, int32_t device,
                                         int32_t* status) {
  const double t0 = now_ms();
  return make_matrix("SLIMGPU_MatrixFromHost (device-to-device copy of the staged matrix)", status,
                     [&](slimgpu_matrix* m) {
    (void)hipGetLastError();
    LearnOptions o;
    o.device = device;
    pick_device(m, o);
    m->nrows = src->nrows;
    m->ncols = src->ncols;
    m->nnz = src->nnz;
    m->binary = src->binary;
    m->exact_gram = src->exact_gram;
    m->nonpositive = src->nonpositive;
    m->merged = src->merged;
    m->owns_csr = true;
    m->h_cost = src->h_cost;
    const size_t nz = (size_t)std::max<int64_t>(m->nnz, 1);
    m->d_rowptr = DeviceBuffer<int64_t>((size_t)m->nrows + 1).release();
    m->d_rowind = DeviceBuffer<int32_t>(nz).release();
    m->d_rowval = m->binary ? nullptr : DeviceBuffer<float>(nz).release();
    m->d_colptr = DeviceBuffer<int64_t>((size_t)m->ncols + 1);
    m->d_colind = DeviceBuffer<int32_t>(nz + 64);
    if (!m->binary) m->d_colval = DeviceBuffer<float>(nz);
    m->d_cnorm = DeviceBuffer<float>((size_t)m->ncols);
    m->d_csq = DeviceBuffer<float>((size_t)m->ncols);
    // device to device over xGMI when the two devices can reach each other (asked, not
    // assumed: a partitioned node or an IOMMU setting can say no), else through a pinned host
    // buffer, 256 MB at a time -- slower, never wrong.  SLIM_GPU_PEER=0 forces the host route.
    int can_peer = m->device == src->device ? 1 : 0;
    if (!can_peer) {
      if (hipDeviceCanAccessPeer(&can_peer, m->device, src->device) != hipSuccess) can_peer = 0;
      (void)hipGetLastError();
    }
    if (const char* e = std::getenv("SLIM_GPU_PEER")) can_peer = can_peer && std::atoi(e) != 0;
    void* bounce = nullptr;
    const size_t bounce_bytes = size_t(256) << 20;
    struct BounceFree {
      void** p;
      ~BounceFree() {
        if (*p) (void)hipHostFree(*p);
      }
    } bounce_guard{&bounce};
    auto peer = [&](void* dst, const void* from, size_t bytes) {
      if (bytes == 0 || !dst || !from) return;
      if (can_peer) {
        HIP_TRY(hipMemcpyPeerAsync(dst, m->device, from, src->device, bytes, m->stream));
        return;
      }
      if (!bounce) HIP_TRY(hipHostMalloc(&bounce, bounce_bytes, hipHostMallocDefault));
      for (size_t off = 0; off < bytes; off += bounce_bytes) {
        const size_t n = std::min(bounce_bytes, bytes - off);
        HIP_TRY(hipSetDevice(src->device));
        HIP_TRY(hipMemcpy(bounce, static_cast<const char*>(from) + off, n, hipMemcpyDeviceToHost));
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(hipMemcpy(static_cast<char*>(dst) + off, bounce, n, hipMemcpyHostToDevice));
      }
    };
    peer(m->d_rowptr, src->d_rowptr, sizeof(int64_t) * ((size_t)m->nrows + 1));
    peer(m->d_colptr.get(), src->d_colptr.get(), sizeof(int64_t) * ((size_t)m->ncols + 1));
    peer(m->d_cnorm.get(), src->d_cnorm.get(), sizeof(float) * (size_t)m->ncols);
    peer(m->d_csq.get(), src->d_csq.get(), sizeof(float) * (size_t)m->ncols);
    if (m->nnz > 0) {
      peer(m->d_rowind, src->d_rowind, sizeof(int32_t) * (size_t)m->nnz);
      peer(m->d_colind.get(), src->d_colind.get(), sizeof(int32_t) * (size_t)m->nnz);
      peer(m->d_rowval, src->d_rowval, sizeof(float) * (size_t)m->nnz);
      peer(m->d_colval.get(), src->d_colval.get(), sizeof(float) * (size_t)m->nnz);
    }
    HIP_TRY(hipStreamSynchronize(m->stream));
    m->setup_ms = now_ms() - t0;
  });
}

void matrix_add_replica(slimgpu_matrix_t* m, slimgpu_matrix_t* replica) {
  m->replicas.push_back(replica);
}
const std::vector<slimgpu_matrix_t*>& matrix_replicas(const slimgpu_matrix_t* m) {
  return m->replicas;
}
void matrix_adopt_csr(slimgpu_matrix_t* m) { m->owns_csr = true; }
int32_t matrix_device(const slimgpu_matrix_t* m) { return m ? m->device : -1; }
void matrix_set_setup_ms(slimgpu_matrix_t* m, double ms) { m->setup_ms = ms; }

int32_t matrix_info(const slimgpu_matrix_t* m, int32_t* nrows, int32_t* ncols, int64_t* nnz) {
  if (!m) return SLIM_ERROR_INPUT;
  if (nrows) *nrows = m->nrows;
  if (ncols) *ncols = m->ncols;
  if (nnz) *nnz = m->nnz;
  return SLIM_OK;
}

double matrix_setup_ms(const slimgpu_matrix_t* m) { return m ? m->setup_ms : 0.0; }

void matrix_expect_solves(slimgpu_matrix_t* m, int32_t n) {
  if (!m) return;
  m->expect_solves = n;
  for (slimgpu_matrix* r : m->replicas) r->expect_solves = n;
}

int32_t matrix_column_cost(const slimgpu_matrix_t* m, int64_t* cost) {
  if (!m || !cost) return SLIM_ERROR_INPUT;
  std::memcpy(cost, m->h_cost.data(), sizeof(int64_t) * m->h_cost.size());
  return SLIM_OK;
}

int32_t matrix_get_column_view(const slimgpu_matrix_t* m, int64_t* colptr, int32_t* colind,
                               float* colval, float* cnorms) {
  if (!m) return SLIM_ERROR_INPUT;
  try {
    HIP_TRY(hipSetDevice(m->device));
    if (colptr)
      HIP_TRY(hipMemcpy(colptr, m->d_colptr.get(), sizeof(int64_t) * ((size_t)m->ncols + 1),
                        hipMemcpyDeviceToHost));
    if (colind && m->nnz)
      HIP_TRY(hipMemcpy(colind, m->d_colind.get(), sizeof(int32_t) * (size_t)m->nnz,
                        hipMemcpyDeviceToHost));
    if (colval && m->nnz && m->d_colval.get())
      HIP_TRY(hipMemcpy(colval, m->d_colval.get(), sizeof(float) * (size_t)m->nnz,
                        hipMemcpyDeviceToHost));
    if (cnorms)
      HIP_TRY(hipMemcpy(cnorms, m->d_cnorm.get(), sizeof(float) * (size_t)m->ncols,
                        hipMemcpyDeviceToHost));
    return SLIM_OK;
  } catch (const HipFail& e) {
    report(e, "SLIMGPU_MatrixGetColumnView");
    return status_of(e);
  }
}

// ---- the solve -----------------------------------------------------------------

namespace {

KernelFn pick_kernel(bool lds, bool has_val) {
  if (lds) return has_val ? cd_wave_kernel<true, true> : cd_wave_kernel<true, false>;
  return has_val ? cd_wave_kernel<false, true> : cd_wave_kernel<false, false>;
}

int round_up(int v, int q) { return (v + q - 1) / q * q; }

// test-only behaviour switches: honoured only when SLIM_GPU_TEST_HOOKS=1 is set as well
bool test_hook(const char* name) {
  const char* master = std::getenv("SLIM_GPU_TEST_HOOKS");
  return master && std::atoi(master) == 1 && std::getenv(name) != nullptr;
}

constexpr int kBitmapBytes = 64 * 1024;  // dynamic LDS of a tile workgroup (user bitmap): two
                                         // 8-wave workgroups per CU still fit (2 x (64 + 10) KB)

}  // namespace

namespace {

// G (floats, m->ws_G) -> byte planes in popularity order (gram_pack.hpp).  Returns false, and
// leaves the handle on the float kernels, when G holds anything but integers in [0, 2^24)
// (fractional or negative ratings) or the planes do not fit the free memory.
bool pack_gram(slimgpu_matrix* m) {
  if (std::getenv("SLIM_GPU_NO_GRAMR")) return false;  // (not an attempt: a later call may pack)
  m->Gp_tried = true;
  const int32_t ncols = m->ncols;
  hipStream_t st = m->stream;
  const double t0 = now_ms();
  // popularity order: ratings per item descending, ties by id
  std::vector<int64_t> cp((size_t)ncols + 1);
  HIP_TRY(hipMemcpy(cp.data(), m->d_colptr.get(), sizeof(int64_t) * cp.size(), hipMemcpyDeviceToHost));
  const int32_t nchunks = (ncols + 15) / 16;
  // Nothing reads the planes beyond the largest on-chip instantiation (gramr_kernel(): 13 groups of
  // 8192 ranks = 106 496 items), and their layout ends not far behind it: one base byte per group in
  // a 16-byte record per thread (16 groups), 17 bits of rank and 4 bits of hi_k / hi2_k in the row
  // record (131 072 ranks, 15 groups).  Larger matrices stay on the float kernels.
  static_assert(kGramrMaxGroups <= 15 && kGramrMaxGroups * kPackGroup <= (1 << 17),
                "row record: 17 bits of rank, 4 bits per plane length; base bytes: 16 groups per thread");
  if ((nchunks + kGramrNT - 1) / kGramrNT > kGramrMaxGroups) return false;
  std::vector<int32_t> item_of((size_t)nchunks * 16, -1), rank_of((size_t)ncols);
  std::iota(item_of.begin(), item_of.begin() + ncols, 0);
  std::stable_sort(item_of.begin(), item_of.begin() + ncols, [&](int32_t a, int32_t b) {
    return cp[(size_t)a + 1] - cp[(size_t)a] > cp[(size_t)b + 1] - cp[(size_t)b];
  });
  for (int32_t r = 0; r < ncols; ++r) rank_of[(size_t)item_of[(size_t)r]] = r;
  int32_t* d_item_of = m->ws_itemof.reserve(item_of.size());
  int32_t* d_rank_of = m->ws_rankof.reserve(rank_of.size());
  HIP_TRY(hipMemcpyAsync(d_item_of, item_of.data(), sizeof(int32_t) * item_of.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_rank_of, rank_of.data(), sizeof(int32_t) * rank_of.size(), hipMemcpyHostToDevice, st));
  int32_t* d_hik = m->ws_hik.reserve((size_t)ncols + 1);   // [ncols] + the flag word
  int32_t* d_hi2k = m->ws_hi2k.reserve((size_t)ncols);
  int32_t* d_flag = d_hik + ncols;
  HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), st));
  const float* dG = m->ws_G.get();
  // (SLIM_GPU_PACK_BASE=0: no per-chunk base bytes -- the first form of the planes, A/B runs)
  int use_base = 1;
  if (const char* e = std::getenv("SLIM_GPU_PACK_BASE")) use_base = std::atoi(e) != 0;
  // (SLIM_GPU_PACK_GATHER=1: the per-row kernels that gather g[item_of[.]] -- A/B runs and the tests
  // that hold the streamed form against them; the streamed form reads G[item_of[r]][j] for
  // G[j][item_of[r]], equal wherever planes are built at all: an integer-valued G is exactly symmetric)
  bool gather = false;
  if (const char* e = std::getenv("SLIM_GPU_PACK_GATHER")) gather = std::atoi(e) != 0;
  const dim3 tgrid(kGramrNT / kPackTS, (ncols + kPackJT - 1) / kPackJT);
  if (gather) {
    hipLaunchKernelGGL(gram_pack_scan_fn(), dim3(ncols), dim3(256), 0, st, dG, m->G_ld, ncols, d_item_of, nchunks,
                       use_base, d_hik, d_hi2k, d_flag);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemsetAsync(d_hik, 0xff, sizeof(int32_t) * (size_t)ncols, st));  // last chunk: -1
    HIP_TRY(hipMemsetAsync(d_hi2k, 0xff, sizeof(int32_t) * (size_t)ncols, st));
    hipLaunchKernelGGL(gram_pack_scan_t_fn(), tgrid, dim3(256), 0, st, dG, m->G_ld, ncols, d_item_of, d_rank_of,
                       nchunks, use_base, d_hik, d_hi2k, d_flag);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gram_pack_groups_fn(), dim3((ncols + 255) / 256), dim3(256), 0, st, ncols, d_hik, d_hi2k);
    HIP_TRY(hipGetLastError());
  }
  std::vector<int32_t> hk((size_t)ncols + 1), h2k((size_t)ncols);
  HIP_TRY(hipMemcpyAsync(hk.data(), d_hik, sizeof(int32_t) * hk.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h2k.data(), d_hi2k, sizeof(int32_t) * h2k.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (hk[(size_t)ncols] != 0) return false;  // not integers in [0, 2^24): stays on the float kernels
  // one pool: a row's hi groups, then its hi2 groups (the solver derives the second offset)
  std::vector<int64_t> off1((size_t)ncols), off2((size_t)ncols);
  int64_t n1 = 0, n2 = 0, npool = 0;
  for (int32_t i = 0; i < ncols; ++i) {
    off1[(size_t)i] = npool;
    npool += (int64_t)hk[(size_t)i] * kPackGroup;
    off2[(size_t)i] = npool;
    npool += (int64_t)h2k[(size_t)i] * kPackGroup;
    n1 += (int64_t)hk[(size_t)i] * kPackGroup;
    n2 += (int64_t)h2k[(size_t)i] * kPackGroup;
  }
  const int64_t ldb = (int64_t)nchunks * 16;
  // (a group of slack behind each pool: a lane outside a plane's prefix reads byte 0 of the plane)
  const size_t need = (size_t)ncols * ((size_t)ldb + kPackGroup) + (size_t)n1 + (size_t)n2 + 2 * (size_t)kPackGroup;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need + (size_t(4) << 30) > free_b + m->ws_Glo.bytes() + m->ws_Ghi.bytes() + m->ws_Gbase.bytes()) return false;
  uint8_t* d_lo = m->ws_Glo.reserve((size_t)ncols * (size_t)ldb);
  uint8_t* d_hi = m->ws_Ghi.reserve((size_t)npool + kPackGroup);
  uint8_t* d_hi2 = d_hi;
  uint8_t* d_base = m->ws_Gbase.reserve((size_t)ncols * kPackGroup);
  if (gather) {  // (streamed: every record is written)
    HIP_TRY(hipMemsetAsync(d_base, 0, (size_t)ncols * kPackGroup, st));
  }
  float* d_diag = m->ws_Gdiag.reserve((size_t)ncols);
  HIP_TRY(hipMemsetAsync(d_diag, 0, sizeof(float) * (size_t)ncols, st));
  int64_t* d_off1 = m->ws_hioff.reserve((size_t)ncols);
  int64_t* d_off2 = m->ws_hi2off.reserve((size_t)ncols);
  HIP_TRY(hipMemcpyAsync(d_off1, off1.data(), sizeof(int64_t) * off1.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_off2, off2.data(), sizeof(int64_t) * off2.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_hi + npool, 0, kPackGroup, st));
  if (gather) {
    hipLaunchKernelGGL(gram_pack_write_fn(), dim3(ncols), dim3(256), 0, st, dG, m->G_ld, ncols, d_item_of, nchunks,
                       d_lo, ldb, d_hi, d_off1, d_hik, d_hi2, d_off2, d_hi2k, d_base, d_diag);
  } else {
    hipLaunchKernelGGL(gram_pack_write_t_fn(), tgrid, dim3(256), 0, st, dG, m->G_ld, ncols, d_item_of, d_rank_of,
                       nchunks, d_lo, ldb, d_hi, d_off1, d_hik, d_hi2, d_off2, d_hi2k, d_base, d_diag);
  }
  HIP_TRY(hipGetLastError());
  uint4* d_meta = m->ws_Gmeta.reserve((size_t)ncols);
  hipLaunchKernelGGL(gram_pack_meta_fn(), dim3((ncols + 255) / 256), dim3(256), 0, st, ncols, d_rank_of, d_hik,
                     d_hi2k, d_off1, d_diag, m->d_colptr.get(), m->d_csq.get(), m->d_cnorm.get(), d_meta, d_flag);
  HIP_TRY(hipGetLastError());
  int32_t meta_flag = 0;
  HIP_TRY(hipMemcpyAsync(&meta_flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (off1 / off2 are locals)
  if (meta_flag & 2) return false;    // |a_i|^2 of the planes is not the column view's: float kernels
  m->Gp_ldb = ldb;
  m->Gp_pool_bytes = npool + kPackGroup;
  m->Gp_nchunks = nchunks;
  m->Gp_bytes_per_row = (double)ldb + 16.0 * std::min(nchunks, kGramrNT) + (double)(n1 + n2) / std::max(1, ncols);
  m->Gp_ready = true;
  if (const char* te = std::getenv("SLIM_GPU_TRACE"); te && std::atoi(te) >= 1)
    std::fprintf(stderr, "[trace] G packed (%s): lo %.2f GB + base %.2f GB + hi %.2f GB + hi2 %.3f GB = %.3f bytes per entry, %.1f ms\n",
                 gather ? "gathers" : "streamed tiles", (double)ncols * ldb * 1e-9, (double)ncols * kPackGroup * 1e-9, n1 * 1e-9, n2 * 1e-9,
                 m->Gp_bytes_per_row / std::max(1, ncols), now_ms() - t0);
  return true;
}

// Once the byte planes stand and a kernel can consume them, nothing reads the floats of G: the
// on-chip kernel takes aTy of a problem (x's active set, the loss term) from the planes of row iC
// (cd_gramr.hpp, SLIM_GRAMR_FROM_PLANES).  Large ones are freed -- C4: 40 GB per handle --; a later
// solve with SLIM_GPU_NO_GRAMR=1 forms them again (SLIMGPU_MatrixGramView does not: it refuses,
// SLIM_ERROR_INPUT, once they are gone).
// SLIM_GPU_KEEP_G=1 keeps them; SLIM_GPU_DROP_G_MIN_GB sets the size from which they go (default 8).
void drop_float_gram(slimgpu_matrix* m) {
  if (!m->Gp_ready || !m->ws_G.get() || std::getenv("SLIM_GPU_KEEP_G") || std::getenv("SLIM_GPU_NO_GRAMR")) return;
  if ((m->Gp_nchunks + kGramrNT - 1) / kGramrNT > kGramrMaxGroups) return;
  double min_gb = 8.0;
  if (const char* e = std::getenv("SLIM_GPU_DROP_G_MIN_GB")) min_gb = std::atof(e);
  if ((double)m->ws_G.bytes() < min_gb * 1073741824.0) return;
  (void)hipStreamSynchronize(m->stream);
  m->ws_G.reset();
  m->Gf_dropped = true;
}

// ---- the solve, step by step (learn_cd at the end drives them) ---------------------------

// An input the solve refuses: set_error(msg), the call returns status.
struct Refusal {
  int32_t status;
  std::string msg;
};

int64_t gram_ld(int32_t ncols) { return round_up(round_up(ncols, 64), 64); }

// The work list: the requested columns (a range or an explicit set), most expensive first
// (longest-processing-time order), this shard's granules of it, the G row block first.
struct WorkList {
  std::vector<int32_t> order;
  int32_t G_block = 0;  // (G in row blocks: entries of the block at the head of order)
};

WorkList work_list(const slimgpu_matrix* m, const LearnOptions& opt, const int32_t* columns,
                   int32_t ncolumns) {
  const int32_t ncols = m->ncols;
  WorkList w;
  if (columns) {  // an explicit set of item columns instead of a range
    std::vector<char> seen((size_t)ncols, 0);
    for (int32_t k = 0; k < ncolumns; ++k) {
      if (columns[k] < 0 || columns[k] >= ncols || seen[(size_t)columns[k]])
        throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_LearnColumns: column ids must be distinct and inside [0, ncols)"};
      seen[(size_t)columns[k]] = 1;
    }
    w.order.assign(columns, columns + ncolumns);
  } else {
    int32_t cb = std::max(0, opt.col_begin);
    const int32_t ce = opt.col_end < 0 ? ncols : std::min(opt.col_end, ncols);
    if (cb > ce) cb = ce;
    w.order.resize((size_t)(ce - cb));
    std::iota(w.order.begin(), w.order.end(), cb);
  }
  if (opt.shard_index < 0 || opt.shard_index >= opt.shard_count)
    throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_Learn: shard index outside [0, shard count)"};
  std::vector<int32_t>& order = w.order;
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t a, int32_t b) { return m->h_cost[a] > m->h_cost[b]; });
  if (opt.shard_count > 1) {  // granules of 32 work-list entries, dealt round-robin
    std::vector<int32_t> mine;
    for (int32_t t = 0; t < (int32_t)order.size(); ++t)
      if ((t / 32) % opt.shard_count == opt.shard_index) mine.push_back(order[(size_t)t]);
    order.swap(mine);
  }
  // (G = R^T R by row blocks: the block's items come first in the list and only their tiles run
  // -- a tile forms the sums with every column at or behind its own position, so the first tiles
  // of a list form whole rows)
  if (opt.build_G && opt.G_rows_end >= 0) {
    auto in_block = [&](int32_t c) { return c >= opt.G_rows_begin && c < opt.G_rows_end; };
    std::stable_partition(order.begin(), order.end(), in_block);
    w.G_block = (int32_t)std::count_if(order.begin(), order.end(), in_block);
  }
  return w;
}

// G = R^T R by the tile kernel's screen pass over every column (S.gram_mode 3): a nested solve of
// learn_cd (hence its recursive device lock) with the options `bo` inherits; rows
// [G_rows_begin, G_rows_end) only when G_rows_end >= 0.  zero_first: into a fresh, zeroed m->ws_G
// (alloc_ms: what that took).  Returns the nested solve's status.
int32_t build_gram(slimgpu_matrix* m, LearnOptions bo, bool zero_first, double* alloc_ms = nullptr) {
  if (zero_first) {
    const double t0 = now_ms();
    const int64_t G_ld = gram_ld(m->ncols);
    drop_screen_cache(m);  // (G holds the same sums for every column)
    float* dG = m->ws_G.reserve((size_t)m->ncols * (size_t)G_ld);
    if (alloc_ms) *alloc_ms = now_ms() - t0;
    HIP_TRY(hipMemsetAsync(dG, 0, sizeof(float) * (size_t)m->ncols * (size_t)G_ld, m->stream));
    m->G_ld = G_ld;
  }
  if (bo.G_rows_end >= 0 && bo.G_rows_begin == bo.G_rows_end) return SLIM_OK;
  bo.kernel = SLIMGPU_KERNEL_TILE;
  bo.build_G = true;
  bo.heavy_tiles = 0;
  int32_t st = SLIM_OK;
  if (slim_csr_t* none = learn_cd(m, bo, nullptr, &st, nullptr, 0, false)) csr_free(none);
  return st;
}

// The kernel and geometry of a solve.
struct Path {
  int kernel = 0;
  bool use_gram = false, use_gramr = false, use_tile = false, use_lds = false;
  int nrows_pad = 0, ncols_pad = 0;
  size_t vec_floats = 0, lds_need = 0;  // the wave kernels' work vectors
  int gram_nw = 0, gram_v = 0;          // item space (cd_gram.hpp)
  GramrFn fn_r = nullptr;               // item space on the byte planes (cd_gramr.hpp)
  int gramr_kr = 0, gramr_kl = 0;
  size_t gram_lds = 0;
  KernelFn fn = nullptr;
  int tileP = 32, tileNW = 16;
  int req_cluster = 0;
  size_t gram_bits_lds = 0;  // G builder: one word per user of a member's range in LDS
  // G builder: the staging tiles of the read-once sum (cd_tile.hpp, gram_store_lines), one per wavefront in
  // the launch's dynamic LDS; 0: that launch cannot hold them and reads the sums in four rounds
  size_t gram_stage_lds = 0;
  const char* gram_stage_why = "";
  int gram_passes = 1;       // G builder: user passes
  int wg_slots = 0;          // co-resident tile workgroups
  int nwaves = 1;            // workgroups launched (tiles: re-planned by plan_tiles)
  int trace_level = 0;
  bool has_imodel = false;
  bool exact_gram = false;   // the aTy sums in a fixed order, no float atomics (SolveArgs::exact_gram)
  // FSLIM in item space (cd_fslim_gram.hpp)
  bool use_fgram = false, f_block = false;
  int f_stride = 0, f_ustride = 0, f_tab_n = 0, f_waves = 1;
  size_t f_wave_lds = 0, f_union_lds = 0;
  FslimFn fn_f = nullptr;
};

// The kernel flavour, up to the item-space choice (which may need G built first).
Path choose_kernel(slimgpu_matrix* m, const LearnOptions& opt, int32_t nwork) {
  const int32_t ncols = m->ncols;
  Path p;
  p.nrows_pad = round_up(std::max(m->nrows, 1), 64);
  p.ncols_pad = round_up(ncols, 64);
  p.vec_floats = (size_t)p.nrows_pad + 2 * (size_t)p.ncols_pad;
  p.lds_need = p.vec_floats * sizeof(float);
  p.kernel = opt.kernel;
  // Item-space CD on G = R^T R (cd_gram.hpp): when asked for, or -- left to the engine -- when
  // this matrix is being solved repeatedly (G is there already; the caller announced a grid,
  // SLIMGPU_MatrixExpectSolves; the very work list of the previous call comes again), the
  // matrix is beyond the one-wavefront-per-item kernel, g fits the LDS of a CU and G the HBM.
  const bool gram_fits =
      gram_geometry(p.ncols_pad, &p.gram_nw, &p.gram_v) && opt.nnbrs == 0 && !opt.build_G && ncols > 0;
  const size_t G_bytes = sizeof(float) * (size_t)ncols * (size_t)gram_ld(ncols);
  if (p.kernel == SLIMGPU_KERNEL_GRAM_FSLIM) {
    // FSLIM in item space (cd_fslim_gram.hpp): only when asked for, and only where a row of the
    // float G says who the co-rated columns are and a problem's state fits a wavefront's LDS
    if (opt.nnbrs <= 0 || opt.build_G)
      throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_Learn: the item-space FSLIM kernel needs nnbrs > 0"};
    if (m->nonpositive)
      throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_Learn: the item-space FSLIM kernel needs ratings > 0: with a rating <= 0 "
                                      "a co-rating sum can cancel to 0 and G cannot mark the column as co-rated "
                                      "(the tile kernel solves such matrices)"};
    if (std::min(opt.nnbrs, ncols - 1) > kFslimMaxNbrs)
      throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_Learn: the item-space FSLIM kernel holds at most 4096 neighbours per "
                                      "problem in LDS (min(nnbrs, ncols - 1) is larger)"};
    if (m->G_ready && m->Gf_dropped) {  // (this path reads the floats: form them again; the planes stay)
      m->G_ready = false;
      m->Gf_dropped = false;
    }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (!m->G_ready && G_bytes + (size_t(4) << 30) > free_b + m->ws_gram.bytes())
      throw Refusal{SLIM_ERROR_MEMORY, "SLIMGPU_Learn: G = R^T R (4 ncols^2 bytes) does not fit the free HBM"};
    p.use_fgram = true;
    return p;
  }
  if (p.kernel == SLIMGPU_KERNEL_GRAM) {
    if (!gram_fits) throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_Learn: the item-space kernel has no FSLIM form"};
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (!m->G_ready && G_bytes + (size_t(4) << 30) > free_b + m->ws_gram.bytes())
      throw Refusal{SLIM_ERROR_MEMORY, "SLIMGPU_Learn: G = R^T R (4 ncols^2 bytes) does not fit the free HBM"};
    p.use_gram = true;
  } else if (p.kernel == SLIMGPU_KERNEL_AUTO && gram_fits && p.lds_need > 64 * 1024 &&
             !std::getenv("SLIM_GPU_NO_GRAMCD")) {
    // The engine's own choice between the residual (tile) kernel and item space, by their byte
    // models per problem and sweep: the tile kernel moves ~5.4 bytes per nnz of
    // R (ids + one residual line per nnz shared by 32 problems, write-backs), item space one
    // row of G per update -- f ncols rows of 4 ncols bytes with f ~ 3 % of the coordinates
    // carrying a coefficient (C4 2.6 %, C4 at 0.1 % 2.7 %, ml100k 2.4 %).  rho = item / tile
    // = (ncols^2 / nnz) / 45; measured 0.22 on C4 (1.3 against 5.8 ms per column), 2.6 on C4 at
    // 0.1 % density.  G itself costs what ~ncols / 32 columns cost the tile kernel (one screen
    // pass over every column; measured ncols / 64 on C4, ncols / 36 on C5), so a FIRST solve
    // takes item space when the columns it solves -- times the number of solves the caller
    // announced (SLIMGPU_MatrixExpectSolves: a model-selection grid) -- save more than that;
    // with G already there the per-column figure decides alone.  A shard of a multi-GPU solve
    // applies the rule to its own columns (every replica builds its own G).  Deterministic in
    // the call's arguments and the handle's state (G built or not): the same call on a fresh
    // handle always takes the same kernel.
    const double rho = (double)ncols * (double)ncols / std::max(1.0, (double)m->nnz) / 45.0;
    const double solves = (double)std::max(1, m->expect_solves);
    // (explicit cluster / heavy-phase options describe a residual-kernel launch: honoured)
    const bool tile_geometry_asked = opt.cluster != 0 || opt.heavy_tiles >= 0 || opt.heavy_cluster != 0;
    bool item_space = rho < 1.0 && !tile_geometry_asked &&
                      (m->G_ready || (double)nwork * solves * (1.0 - rho) > (double)ncols / 32.0);
    if (const char* e = std::getenv("SLIM_GPU_GRAMCD"); e && std::strcmp(e, "never-first") == 0)
      item_space = item_space && (m->G_ready || m->expect_solves >= 2);  // (round-4 policy, A/B runs)
    if (item_space) {
      size_t free_b = 0, total_b = 0;
      HIP_TRY(hipMemGetInfo(&free_b, &total_b));
      p.use_gram = m->G_ready || G_bytes + (size_t(8) << 30) <= free_b + m->ws_gram.bytes();
    }
  }
  if (p.use_gram) p.kernel = SLIMGPU_KERNEL_GRAM;
  if (p.use_gram && m->G_ready && m->Gf_dropped && std::getenv("SLIM_GPU_NO_GRAMR")) {
    m->G_ready = false;  // (the float kernels were asked for: form the floats again; the planes stay)
    m->Gf_dropped = false;
  }
  return p;
}

// G for an item-space solve, once per handle, timed into the handle (charged to this solve's stats).
// floats_only: neither packed into byte planes nor dropped (the FSLIM path reads the floats; a later
// plain item-space solve finds G_ready && !Gp_tried and packs then)
int32_t gram_for_solve(slimgpu_matrix* m, const LearnOptions& opt, int32_t trace_level, bool floats_only) {
  const double tb = now_ms();
  LearnOptions bo = opt;
  bo.col_begin = 0;
  bo.col_end = -1;
  bo.shard_count = 1;
  bo.shard_index = 0;
  bo.nnbrs = 0;
  bo.cluster = 0;
  bo.dbglvl = 0;
  double alloc_ms = 0;
  const int32_t st = build_gram(m, bo, true, &alloc_ms);
  if (st != SLIM_OK) return st;
  const double t_sums = now_ms();
  const double sums_kernel_ms = last_stats().kernel_ms;
  m->G_ready = true;
  m->Gf_dropped = false;
  if (!floats_only) {
    if (!m->Gp_ready) {  // (planes of an earlier build of the same G are still right)
      m->Gp_tried = false;
      if (!pack_gram(m)) m->Gp_ready = false;
    }
    drop_float_gram(m);
  }
  m->G_build_ms = now_ms() - tb;
  m->G_alloc_ms = alloc_ms;
  m->G_sums_ms = t_sums - tb - alloc_ms;
  m->G_sums_kernel_ms = sums_kernel_ms;
  m->G_pack_ms = now_ms() - t_sums;
  if (trace_level >= 1)
    std::fprintf(stderr, "[trace] G = R^T R (%d x %d, %.2f GB) built in %.1f ms: allocation %.1f, sums %.1f "
                 "(kernel %.1f), byte planes %.1f\n", m->ncols, m->ncols,
                 sizeof(float) * (double)m->ncols * (double)m->G_ld * 1e-9, m->G_build_ms, m->G_alloc_ms,
                 m->G_sums_ms, sums_kernel_ms, m->G_pack_ms);
  return SLIM_OK;
}

// The rest of the path: the tile / wave flavour, the kernel function, the G builder's word form,
// and how many workgroups fit.
void finish_path(slimgpu_matrix* m, const LearnOptions& opt, int32_t nwork, const slim_csr_t* imodel,
                 const slimgpu_model* warm_dev, Path& p) {
  // (FSLIM on ratings that can cancel: the fixed-order pass also counts co-ratings, so that
  // a candidate whose sum is 0 stays a candidate -- neighbors.c:46-60 marks every co-rated item)
  p.exact_gram = m->exact_gram || std::getenv("SLIM_GPU_EXACT_GRAM") || (opt.nnbrs > 0 && m->nonpositive);
  if (p.kernel == SLIMGPU_KERNEL_AUTO)
    p.kernel = p.lds_need <= 64 * 1024 ? SLIMGPU_KERNEL_WAVE_LDS : SLIMGPU_KERNEL_TILE;
  if (p.kernel == SLIMGPU_KERNEL_WAVE_LDS && p.lds_need > 160 * 1024)
    throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_Learn: work vectors do not fit the 160 KiB LDS of a CU"};
  if (p.kernel < SLIMGPU_KERNEL_WAVE_LDS || p.kernel > SLIMGPU_KERNEL_GRAM_FSLIM)
    throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_Learn: unknown kernel selection"};
  if (p.use_fgram) {
    // lists of min(nnbrs, ncols - 1) entries, rounded up to a wavefront; a tile's union holds at most
    // 32 of them.  The nn x nn block of G goes to LDS up to 128 neighbours (16 KB / 64 KB per
    // wavefront); beyond, or with SLIM_GPU_FSLIM_BLOCK=0, its entries are gathered per update.
    p.f_stride = std::max(64, round_up(std::min(opt.nnbrs, m->ncols - 1), 64));
    p.f_ustride = (int)std::min<int64_t>((int64_t)32 * p.f_stride, p.ncols_pad);
    p.f_block = p.f_stride <= kFslimBlockMaxStride;
    if (const char* e = std::getenv("SLIM_GPU_FSLIM_BLOCK")) p.f_block = p.f_block && std::atoi(e) != 0;
    p.f_tab_n = p.f_block ? round_up(p.f_ustride, 8) : 0;
    p.f_wave_lds = fslim_wave_lds(p.f_stride, p.f_block, p.f_tab_n);
    p.f_waves = (int)std::max<size_t>(1, std::min<size_t>(p.f_block ? kFslimMaxWaves : 4, (size_t(150) << 10) / p.f_wave_lds));
    p.fn_f = fslim_solve_fn(p.f_block);
    p.f_union_lds = fslim_union_lds(m->ncols);
    if (p.f_union_lds > (size_t(150) << 10))
      throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_Learn: the item-space FSLIM kernel's item bitmap does not fit the LDS of a CU"};
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fslim_union_fn()),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.f_union_lds));
    const size_t lds = p.f_wave_lds * (size_t)p.f_waves;
    int per_cu = 0;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(p.fn_f), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(p.fn_f), 64 * p.f_waves, lds));
    if (per_cu < 1)
      throw Refusal{SLIM_ERROR, "SLIMGPU_Learn: the item-space FSLIM kernel does not fit a compute unit of this device"};
    p.nwaves = std::max(1, std::min((nwork + p.f_waves - 1) / p.f_waves, m->num_cus * per_cu));
    if (warm_dev && warm_dev->device != m->device)
      throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_LearnResident: the warm-start model lives on another device"};
    p.has_imodel = false;  // (estimate.c:424-431: the FSLIM branch never warm-starts)
    if (p.trace_level >= 1)
      std::fprintf(stderr, "[trace] item-space FSLIM: form %s, lists of %d, %d wavefronts per workgroup (%zu KB of LDS "
                   "each), %d workgroups per CU\n", p.f_block ? "block in LDS" : "gathered", p.f_stride, p.f_waves,
                   p.f_wave_lds >> 10, per_cu);
    return;
  }
  p.use_lds = p.kernel == SLIMGPU_KERNEL_WAVE_LDS;
  if (p.use_gram && p.gram_v == 0)  // g in HBM: 8 or 16 wavefronts per workgroup
    if (const char* e = std::getenv("SLIM_GPU_GRAM_NW")) p.gram_nw = std::atoi(e) == 8 ? 8 : 16;
  // item space with g on chip and G as byte planes (cd_gramr.hpp) whenever G could be packed and
  // the items fit the largest instantiation (106 496); SLIM_GPU_NO_GRAMR=1: the float kernels
  if (p.use_gram && m->G_ready && !m->Gp_tried && !m->Gf_dropped) {
    (void)pack_gram(m);
    drop_float_gram(m);
  }
  size_t gramr_lds = 0;
  bool gramr_ring = false;
  int gramr_wps = 0;
  // rows through the LDS ring (global_load_lds) where a row is many groups long -- measured
  // (profiles/r05/gramr_dma_ab.txt): C4, 13 groups, kernel 6.62 -> 5.37 s; C5, 3 groups, where
  // one round of register loads already holds the whole row, 1.32 -> 1.41 s.
  // SLIM_GPU_GRAMR_DMA=0 / 1 forces either.
  bool gramr_dma = (m->Gp_nchunks + kGramrNT - 1) / kGramrNT > 6;
  if (const char* e = std::getenv("SLIM_GPU_GRAMR_DMA")) gramr_dma = std::atoi(e) != 0;
  if (p.use_gram && m->Gp_ready && !std::getenv("SLIM_GPU_NO_GRAMR"))
    p.fn_r = gramr_kernel(m->Gp_nchunks, gramr_dma, &p.gramr_kr, &p.gramr_kl, &gramr_lds, &gramr_ring, &gramr_wps);
  p.use_gramr = p.fn_r != nullptr;
  if (p.use_gram && !p.use_gramr && m->Gf_dropped)
    throw Refusal{SLIM_ERROR, "SLIMGPU_Learn: the floats of G were dropped and the byte-plane kernel cannot run this solve"};
  if (p.use_gramr) {
    p.gram_nw = kGramrNT / 64;
    p.gram_v = 1;  // (x only in the slab: g is on chip)
  }
  p.gram_lds = p.use_gramr ? gramr_lds : (p.gram_v > 0 ? sizeof(float) * (size_t)p.ncols_pad : 0);
  if (p.use_gram && p.trace_level >= 1) {  // which instantiation this solve runs (gram_inst.hpp, gramr_inst.hpp)
    if (p.use_gramr)
      std::fprintf(stderr, "[trace] item-space kernel: packed <%d,%d>, %s loads, WPS %d\n", p.gramr_kr, p.gramr_kl,
                   gramr_ring ? "ring" : "register", gramr_wps);
    else
      std::fprintf(stderr, "[trace] item-space kernel: float <%d,%d>\n", p.gram_nw, p.gram_v);
  }
  // tile width: 32 item columns per workgroup (128-byte residual lines) unless the row
  // offsets would overflow the kernel's 32-bit byte offsets
  p.tileP = p.kernel == SLIMGPU_KERNEL_TILE16 ? 16 : 32;
  if (p.kernel == SLIMGPU_KERNEL_TILE && ((int64_t)p.nrows_pad + 64) * 128 >= (int64_t(1) << 32)) p.tileP = 16;
  p.use_tile = p.kernel == SLIMGPU_KERNEL_TILE || p.kernel == SLIMGPU_KERNEL_TILE16;
  if (p.use_tile && ((int64_t)p.nrows_pad + 64) * 4 * p.tileP >= (int64_t(1) << 32)) {
    p.use_tile = false;  // > 67M users: fall back to one wavefront per item
    p.kernel = SLIMGPU_KERNEL_WAVE_HBM;
  }
  if (p.use_tile && p.tileP == 16 && opt.nnbrs > 0) {  // FSLIM exists for 32-wide tiles only
    p.use_tile = false;
    p.kernel = SLIMGPU_KERNEL_WAVE_HBM;
  }
  if (p.use_tile) p.kernel = p.tileP == 32 ? SLIMGPU_KERNEL_TILE : SLIMGPU_KERNEL_TILE16;
  if (opt.build_G && !p.use_tile)
    throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_Learn: G = R^T R is built by the tile kernel, which this matrix cannot use"};
  p.fn = p.use_gram ? gram_kernel(p.gram_nw, p.gram_v) : pick_kernel(p.use_lds, !m->binary);
  // tile workgroup geometry: 16 wavefronts (1 workgroup per CU) or 8 (2 per CU, phases of
  // the two overlap).  SLIM_GPU_TILE_NW overrides the default.
  // Measured on C4 (profiles/r01): with few tiles per cluster the launch is bound by the
  // slowest tile and one big workgroup per CU finishes it sooner (134 vs 109-116 col/s at
  // 256 tiles); with many tiles throughput matters and two small workgroups win (150 vs
  // ~141 col/s at 512 tiles).
  p.tileNW = (nwork + p.tileP - 1) / p.tileP >= 2 * m->num_cus ? 8 : 16;
  // G = R^T R of a binary matrix: clusters of 32 whose members keep the y of a tile's 32 items as
  // one word per user of their range in LDS (cd_tile.hpp, gbits) -- when that range fits
  p.req_cluster = opt.cluster;
  if (opt.build_G && p.use_tile && p.tileP == 32 && m->binary && !std::getenv("SLIM_GPU_NO_GBITS")) {
    ensure_cluster_split(m, 5);
    const size_t need = sizeof(uint32_t) * (size_t)(round_up(m->split[5].max_rows, 64) + 64);
    // (test hook: pretend a member holds only that many users, so that small matrices take the passes)
    size_t words_cap = 148 * 1024;
    if (test_hook("SLIM_GPU_TEST_GBITS_ROWS"))
      words_cap = sizeof(uint32_t) * (size_t)(round_up(std::max(64, std::atoi(std::getenv("SLIM_GPU_TEST_GBITS_ROWS"))), 64) + 64);
    if (need <= words_cap && m->num_cus >= 32) {
      p.gram_bits_lds = need;
      p.req_cluster = 32;
      p.tileNW = 16;
    } else if (m->num_cus >= 32 && !std::getenv("SLIM_GPU_NO_GPASSES")) {
      // More users than 32 members hold as words (C5: 10M users, 312K per member): the same
      // kernel in USER PASSES -- np launches over the whole work list, launch s with member k on
      // range 32 s + k of 32 np ranges of equal nnz, its sums added to G (exact: integer counts).
      // The id stream is the same 4 bytes per nnz and tile either way (a member reads its
      // ranges' slices of every column); what passes add is a bitmap build per tile and pass.
      const int64_t rows_cap = (int64_t)(words_cap / sizeof(uint32_t)) - 128;
      int np = (int)((m->split[5].max_rows + rows_cap - 1) / rows_cap);
      for (; np <= 64; ++np) {
        ensure_split(m, m->gsplit, 32 * np, false);
        const size_t need_p = sizeof(uint32_t) * (size_t)(round_up(m->gsplit.max_rows, 64) + 64);
        if (need_p <= words_cap) {
          p.gram_bits_lds = need_p;
          p.req_cluster = 32;
          p.tileNW = 16;
          p.gram_passes = np;
          if (p.trace_level >= 1)
            std::fprintf(stderr, "[trace] G builder: %d user passes (32 members x %d users at most, %zu KB of words)\n",
                         np, m->gsplit.max_rows, need_p >> 10);
          break;
        }
      }
    }
  }
  // (four 4-wavefront workgroups per CU were measured too: no gain, even on columns of ~900 nnz)
  if (const char* e = std::getenv("SLIM_GPU_TILE_NW")) p.tileNW = std::atoi(e) == 16 ? 16 : 8;
  // warm start (estimate.c:453-464) on the tile path: how the previous coefficients are folded
  // into the residual -- "row" (default for 32-wide tiles: one pass over the member's rows,
  // x lines from one copy per cluster) or "col" (one pass per column of the union list)
  if (warm_dev && warm_dev->device != m->device)
    throw Refusal{SLIM_ERROR_INPUT, "SLIMGPU_LearnResident: the warm-start model lives on another device"};
  p.has_imodel = warm_dev ? warm_dev->n > 0 : (imodel && imodel->colptr && imodel->ncols > 0);
  bool row_fold = true;
  if (const char* e = std::getenv("SLIM_GPU_FOLD")) row_fold = std::strcmp(e, "col") != 0;
  if (p.use_tile) {
    const bool prof = p.trace_level >= 2;
    const bool val = !m->binary;
    const bool nw16 = p.tileNW == 16;
    // (form / profiled: what the branch that assigns p.fn instantiates, for the trace line below)
    const char* form = "colfold";
    bool profiled = false;
    if (p.tileP == 32 && opt.nnbrs > 0) {
      p.fn = tile_kernel_p32_fslim(val, nw16);
      form = "fslim";
    } else if (p.tileP == 32 && !prof && !p.has_imodel) {
      p.fn = tile_kernel_p32_cold(val, nw16);
      form = "cold";
    } else if (p.tileP == 32 && !prof && row_fold) {
      p.fn = tile_kernel_p32_rowfold(val, nw16);
      form = "rowfold";
    } else if (p.tileP == 32) {
      p.fn = nw16 ? tile_kernel_p32_nw16(val, prof) : tile_kernel_p32_nw8(val, prof);
      profiled = prof;
    } else {
      p.fn = nw16 ? tile_kernel_p16_nw16(val, prof) : tile_kernel_p16_nw8(val, prof);
      profiled = prof;
    }
    if (p.trace_level >= 1)  // which instantiation of cd_tile_kernel this solve runs (tile_inst.hpp)
      std::fprintf(stderr, "[trace] tile kernel: P %d, %d wavefronts, form %s, %s%s\n", p.tileP, nw16 ? 16 : 8,
                   form, val ? "valued" : "binary", profiled ? ", profiled" : "");
  }
  int waves_per_cu;
  if (p.use_gram) {  // one workgroup per problem, as many per CU as g (LDS) and registers allow
    int per_cu = 0;
    const void* kfn = p.use_gramr ? reinterpret_cast<const void*>(p.fn_r) : reinterpret_cast<const void*>(p.fn);
    HIP_TRY(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.gram_lds));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, 64 * p.gram_nw, p.gram_lds));
    if (per_cu < 1)
      throw Refusal{SLIM_ERROR, "SLIMGPU_Learn: the item-space kernel does not fit a compute unit of this device"};
    waves_per_cu = per_cu;
  } else if (p.use_lds) {
    waves_per_cu = (int)std::min<size_t>(16, (160 * 1024) / std::max<size_t>(p.lds_need, 1));
    if (waves_per_cu < 1) waves_per_cu = 1;
    if (p.lds_need > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(p.fn),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_need));
  } else {
    waves_per_cu = 8;
  }
  // wave kernels: one block = one wavefront; tile kernel: one block = 16 wavefronts
  p.nwaves = std::max(1, std::min(nwork, m->num_cus * waves_per_cu));
  if (!p.use_gram && !p.use_tile && p.trace_level >= 1)  // which instantiation of cd_wave_kernel this solve runs
    std::fprintf(stderr, "[trace] wave kernel: %s, %s, sums %s, %d wavefronts, %zu bytes of LDS\n",
                 p.use_lds ? "lds" : "hbm", m->binary ? "binary" : "valued", p.exact_gram ? "ordered" : "atomic",
                 p.nwaves, p.use_lds ? p.lds_need : (size_t)0);
  // co-resident tile workgroups: what the occupancy calculator grants this instantiation
  // (1 x 16 or 2 x 8 wavefronts per CU by design; fewer if the register or LDS footprint
  // of a build ever grows), never more than the design assumes
  p.wg_slots = m->num_cus * (16 / p.tileNW);
  if (p.use_tile) {
    int per_cu = 0;
    const size_t worst_lds = std::max<size_t>(kBitmapBytes, p.gram_bits_lds);
    // (static + dynamic LDS beyond 64 KB needs the attribute)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(p.fn),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)worst_lds));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(p.fn),
                                                         64 * p.tileNW, worst_lds));
    // G builder: the launches of a build also hold a staging tile per wavefront (gram_store_lines reads
    // every partial sum once) -- where that fits the CU next to the kernel's static LDS and costs the
    // build's launches no workgroup per CU.  Only a build's launches are sized by it.
    // SLIM_GPU_GREAD=0: the four-round read (A/B runs, tests)
    if (opt.build_G && per_cu >= 1) {
      const size_t stage = (size_t)kGramStageBytes * (size_t)p.tileNW;
      const char* e = std::getenv("SLIM_GPU_GREAD");
      if (e && std::atoi(e) == 0) {
        p.gram_stage_why = "SLIM_GPU_GREAD=0";
      } else if (p.tileP != 32) {
        p.gram_stage_why = "16-item tiles";
      } else if (stage > worst_lds) {
        hipFuncAttributes fa{};
        HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(p.fn)));
        int per_cu_s = 0;
        if (fa.sharedSizeBytes + stage <= (size_t)160 * 1024) {
          HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(p.fn),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage));
          HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_s, reinterpret_cast<const void*>(p.fn),
                                                               64 * p.tileNW, stage));
        }
        if (per_cu_s >= std::min(per_cu, 16 / p.tileNW)) {
          p.gram_stage_lds = stage;
          per_cu = per_cu_s;
        } else {
          p.gram_stage_why = "no room in LDS";
        }
      } else {
        p.gram_stage_lds = stage;
      }
    }
    if (per_cu < 1)
      throw Refusal{SLIM_ERROR, "SLIMGPU_Learn: the tile kernel does not fit a compute unit of this device"};
    p.wg_slots = m->num_cus * std::min(per_cu, 16 / p.tileNW);
  }
}

// Tile geometry: clusters, the heavy phase and the per-workgroup slab sizes.  force_k1: no
// clusters, no heavy phase -- the geometry that needs no co-residency at all (fallback after a
// cluster timed out waiting for a member, e.g. under a CU mask).
struct TileGeom {
  bool force_k1 = false;
  int clusterK = 1, cluster_lg = 0, nclusters = 0;
  int clusterHi = 0, hi_lg = 0, nheavy = 0, nclusters_hi = 0;
  size_t tile_r = 0, tile_x = 0, tile_u = 0;
  int nwaves = 0;  // workgroups launched
};

TileGeom plan_tiles(slimgpu_matrix* m, const LearnOptions& opt, const Path& p,
                    const std::vector<int32_t>& order, bool force_k1) {
  const int32_t ncols = m->ncols, nwork = (int32_t)order.size();
  const int tileP = p.tileP;
  TileGeom t;
  t.force_k1 = force_k1;
  int auto_heavy = 0;
  const int ngroups_all = (nwork + tileP - 1) / tileP;
  // cluster size: share a tile among K workgroups when there are too few tiles to keep
  // every CU busy behind the slowest one (auto), or as requested
  const int req = p.req_cluster;
  if (force_k1) {
    t.clusterK = 1;
  } else if (req == 1 || req == 2 || req == 4 || req == 8 || req == 16 || req == 32) {
    t.clusterK = req;
  } else {
    // the heaviest tile runs ~7x the median (popular items need more sweeps): a
    // cluster should see >= ~8 tiles so the others fill in behind it; with fewer
    // tiles per cluster, larger clusters shorten that critical path instead
    // ... but a member's slice of a column should stay long enough (>= ~512 nnz on
    // average) for the gather to amortise the per-visit exchange
    int cap = 1;
    while (cap < 16 && (m->nnz / std::max(ncols, 1)) / (2 * cap) >= 512) cap *= 2;
    // heavy tiles (queue order = cost order): a few tiles of the most popular items run
    // 5-8x the median (measured on C4: 52 / 36 / 29 s against 6.4 s).  They go to big
    // clusters first (below), which lets everything else use small, efficient clusters:
    // clusters of 2-4 reach ~0.9 of the HBM roofline, clusters of 8 pay ~25 % for the
    // per-visit exchange.  Cost is only a proxy for time, so the test is generous (a
    // light tile solved by a big cluster wastes a few CU-seconds, a heavy one solved by
    // a small cluster is the critical path of the launch).
    if (opt.heavy_tiles < 0 && p.tileNW == 16 && ngroups_all >= 16) {
      auto tile_cost = [&](int gI) {
        int64_t c = 0;
        for (int k = gI * tileP; k < std::min((gI + 1) * tileP, nwork); ++k) c += m->h_cost[order[(size_t)k]];
        return c;
      };
      const int64_t med = tile_cost(ngroups_all / 2);
      while (auto_heavy < ngroups_all / 16 && tile_cost(auto_heavy) >= 12 * med) ++auto_heavy;
    }
    const int64_t fill = auto_heavy > 0 ? 4 : 8;  // tiles wanted per workgroup slot
    while (t.clusterK < cap && (int64_t)ngroups_all * t.clusterK < fill * (int64_t)p.wg_slots) t.clusterK *= 2;
  }
  while (t.clusterK > 1 && p.wg_slots / t.clusterK < 1) t.clusterK /= 2;
  for (t.cluster_lg = 0; (1 << t.cluster_lg) < t.clusterK; ++t.cluster_lg) {}
  ensure_cluster_split(m, t.cluster_lg);
  // (+ 64 rows: the spare residual line behind a member's user range, cd_tile.hpp)
  t.tile_r = (size_t)(round_up(m->split[t.cluster_lg].max_rows, 64) + 64) * tileP;
  // (the G builder's word-per-user form keeps no residual: C5 would reserve 10 GB of lines)
  if (opt.build_G && p.gram_bits_lds && t.clusterK == 32 && !force_k1) t.tile_r = (size_t)64 * tileP;
  t.tile_x = (size_t)p.ncols_pad * tileP;
  t.tile_u = (size_t)p.ncols_pad;
  t.nclusters = std::max(1, std::min(ngroups_all, p.wg_slots / t.clusterK));
  // heavy phase: the first nheavy tiles (most expensive) go to clusters of clusterHi
  t.nheavy = std::min(opt.heavy_tiles < 0 ? auto_heavy : opt.heavy_tiles, ngroups_all);
  t.clusterHi = opt.heavy_cluster;
  if (const char* e = std::getenv("SLIM_GPU_HEAVY")) {  // "tiles,cluster" (experiments)
    int a = 0, b = 0;
    if (std::sscanf(e, "%d,%d", &a, &b) == 2) {
      t.nheavy = std::min(std::max(a, 0), ngroups_all);
      t.clusterHi = b;
    }
  }
  if (t.clusterHi != 2 && t.clusterHi != 4 && t.clusterHi != 8 && t.clusterHi != 16 && t.clusterHi != 32)
    t.clusterHi = std::max(16, std::min(4 * t.clusterK, kTileKMax));
  if (t.clusterHi <= t.clusterK || t.nclusters * t.clusterK < t.clusterHi || force_k1) t.nheavy = 0;
  if (t.nheavy > 0) {
    for (t.hi_lg = 0; (1 << t.hi_lg) < t.clusterHi; ++t.hi_lg) {}
    ensure_cluster_split(m, t.hi_lg);
    t.nclusters_hi = t.nclusters * t.clusterK / t.clusterHi;
    t.tile_r = std::max(t.tile_r, (size_t)(round_up(m->split[t.hi_lg].max_rows, 64) + 64) * tileP);
  }
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t per_cl = ((t.tile_r + 2 * t.tile_x) * sizeof(float) + t.tile_u * sizeof(int32_t)) * t.clusterK;
  // (the screen-sum cache is given up when a workspace does not fit: reserve evicts it)
  const size_t have = free_b + m->ws_slab.bytes() + m->ws_xslab.bytes() + m->ws_ulist.bytes() +
                      m->ws_part.bytes() + m->ws_gram.bytes();
  const size_t budget = have > (size_t(6) << 30) ? have - (size_t(6) << 30) : have / 2;
  if ((size_t)t.nclusters * per_cl > budget) {
    t.nclusters = (int)std::max<size_t>(1, budget / per_cl);
    t.nclusters_hi = t.nclusters * t.clusterK / std::max(t.clusterHi, 1);
    if (t.nclusters_hi < 1) t.nheavy = 0;
  }
  t.nwaves = t.nclusters * t.clusterK;
  return t;
}

size_t mailbox_stride(int tileP) { return 2 * (size_t)kTileKMax * (size_t)tileP + 8; }

// The per-workgroup work space of the launches (handle workspaces) and the tile workgroup's
// dynamic LDS.
struct Slabs {
  float *slab = nullptr, *xslab = nullptr, *part = nullptr;
  int32_t *ulist = nullptr, *nunion = nullptr;
  unsigned long long* mailbox = nullptr;
  size_t mailbox_words = 0;
  int bm_shift = 0, bm_words = 1;
  // dynamic LDS of a tile workgroup: the user bitmap of the screen pass (FSLIM: the select
  // histograms)
  size_t tile_lds = 0;
  bool gram_words = false;  // tile_lds holds the G builder's word per user (Path::gram_bits_lds)
  // item-space FSLIM: the neighbour lists of one slice of the work list, f_slice_tiles tiles long
  int32_t *f_n = nullptr, *f_id = nullptr, *f_slot = nullptr;
  float* f_aty = nullptr;
  int f_slice_tiles = 0;
};

Slabs alloc_slabs(slimgpu_matrix* m, const LearnOptions& opt, const Path& p, const TileGeom& t, int32_t nwork,
                  int nwaves) {
  Slabs s;
  const auto evict = evict_cache(m);
  if (p.use_fgram) {
    // 12 bytes per list entry (id, aTy, union slot).  Lists beyond a quarter of the free memory:
    // the work list goes through in slices of whole tiles (SLIM_GPU_FSLIM_SLICE_TILES forces a length)
    const size_t ngroups0 = std::max<size_t>(1, ((size_t)nwork + 31) / 32);
    const size_t per_tile = (size_t)32 * (size_t)p.f_stride * 12;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t have = free_b + m->ws_fid.bytes() + m->ws_faty.bytes() + m->ws_fslot.bytes();
    size_t tiles = ngroups0;
    if (tiles * per_tile > have / 4) tiles = std::max<size_t>(1, have / 4 / per_tile);
    if (const char* e = std::getenv("SLIM_GPU_FSLIM_SLICE_TILES"); e && std::atoi(e) > 0)
      tiles = std::min<size_t>(tiles, (size_t)std::atoi(e));
    s.f_slice_tiles = (int)tiles;
    const size_t npos = std::min<size_t>((size_t)std::max(nwork, 1), tiles * 32);
    s.f_n = m->ws_fn.reserve(npos, evict);
    s.f_id = m->ws_fid.reserve(npos * (size_t)p.f_stride, evict);
    s.f_aty = m->ws_faty.reserve(npos * (size_t)p.f_stride, evict);
    s.f_slot = m->ws_fslot.reserve(npos * (size_t)p.f_stride, evict);
    s.ulist = m->ws_ulist.reserve((size_t)p.f_ustride * tiles, evict);
    s.nunion = m->ws_nunion.reserve(tiles, evict);
  } else if (p.use_gram) {
    const size_t ngroups0 = ((size_t)nwork + 31) / 32;
    s.xslab = m->ws_xslab.reserve((size_t)p.ncols_pad * (size_t)nwaves, evict);
    if (p.gram_v == 0) s.slab = m->ws_slab.reserve((size_t)p.ncols_pad * (size_t)nwaves, evict);
    s.ulist = m->ws_ulist.reserve((size_t)p.ncols_pad * ngroups0, evict);
    s.nunion = m->ws_nunion.reserve(ngroups0, evict);
  } else if (p.use_tile) {
    s.mailbox_words = (size_t)(std::max(t.nclusters, 1) + t.nclusters_hi) * mailbox_stride(p.tileP);
    s.slab = m->ws_slab.reserve(t.tile_r * (size_t)nwaves, evict);
    s.xslab = m->ws_xslab.reserve(t.tile_x * (size_t)nwaves, evict);
    s.ulist = m->ws_ulist.reserve(t.tile_u * (size_t)nwaves, evict);
    s.mailbox = m->ws_mailbox.reserve(s.mailbox_words, evict);
    s.part = m->ws_part.reserve(t.tile_x * (size_t)nwaves, evict);
    // LDS user bitmap of the screen pass: one bit per 2^shift users of a member's range,
    // at most kBitmapBytes
    const int64_t range = (int64_t)(t.tile_r / (size_t)p.tileP);
    auto words_at = [&](int sh) { return ((range >> sh) + 1 + 31) / 32; };
    while (words_at(s.bm_shift) * 4 > kBitmapBytes) ++s.bm_shift;
    s.bm_words = (int)words_at(s.bm_shift);
    if (opt.nnbrs > 0) s.bm_words = std::max(s.bm_words, p.tileP * 256);  // FSLIM's select histograms
    // (the bitmap follows the member's user range, which grows when the fallback re-plans
    // without clusters: the launch size must follow it)
    s.tile_lds = sizeof(uint32_t) * (size_t)s.bm_words;
    if (p.gram_bits_lds && t.clusterK == 32 && !t.force_k1) {  // one word per user of a member's range
      s.bm_shift = 0;
      s.bm_words = (int)(p.gram_bits_lds / sizeof(uint32_t));
      s.tile_lds = p.gram_bits_lds;
      s.gram_words = true;
    }
    // (a build's launches: the words or the bitmap, and over them the staging tiles of gram_store_lines)
    if (opt.build_G) s.tile_lds = std::max(s.tile_lds, p.gram_stage_lds);
  } else if (!p.use_lds) {
    s.slab = m->ws_slab.reserve(p.vec_floats * (size_t)nwaves);
  }
  return s;
}

// A piece of the output arena of a resident solve: the arena itself (owned by the handle) or,
// once a later launch overwrites it, a copy of its entries.
struct ArenaSeg {
  const int32_t* ind;
  const float* val;
  int64_t n;
  DeviceBuffer<int32_t> own_i;
  DeviceBuffer<float> own_v;
};

// Everything the launches of one solve share.
struct Launch {
  Path p;
  TileGeom t;
  Slabs s;
  int nwaves = 1;
  int32_t *order = nullptr, *cnt = nullptr, *sti = nullptr, *misc = nullptr;
  int64_t *off = nullptr, *stl = nullptr;
  float* stf = nullptr;
  // warm start: the column view of the previous model
  const int64_t* icolptr = nullptr;
  const int32_t* icolind = nullptr;
  const float* icolval = nullptr;
  int32_t incols = 0;
  // screen-sum cache: 1 record, 2 read (m->ws_gram)
  int gram_mode = 0;
  float* gram = nullptr;
  int gram_geom[6] = {0, 0, 0, 0, 0, 0};
  int gram_pass = 0;
  // g carried between the solves of a grid (slimgpu_model::d_gsave)
  DeviceBuffer<float> carry;
  int64_t carry_stride = 0;
  bool carry_from_warm = false;
  bool cluster_fallback = false;
  int64_t arena_cap = 0;
  int32_t G_block = 0;
  // the G builder's view of the column ids (build_gview), tried once per build
  bool gview_tried = false;
  const uint4* gview = nullptr;
  const int64_t* gview_base = nullptr;
  const uint16_t* gview_cnt = nullptr;
  int32_t gview_ngroups = 0, gview_sentinel = 0;
  size_t gview_bytes = 0;
  double gview_ms = 0;
  const char* gview_why = "";  // why the ids come from the column view instead
};

// The launches' buffers, the warm start, the screen-sum cache and the carried g.
void prepare_launch(slimgpu_matrix* m, const LearnOptions& opt, const std::vector<int32_t>& order,
                    const slim_csr_t* imodel, const slimgpu_model* warm_dev, bool resident, bool all_columns,
                    Launch& L) {
  const int32_t ncols = m->ncols, nwork = (int32_t)order.size();
  const Path& p = L.p;
  hipStream_t stream = m->stream;
  L.nwaves = p.nwaves;
  if (p.use_tile) {
    L.t = plan_tiles(m, opt, p, order, false);
    L.nwaves = L.t.nwaves;
  }
  L.order = m->ws_order.reserve((size_t)nwork);
  L.cnt = m->ws_cnt.reserve((size_t)ncols);
  L.off = m->ws_off.reserve((size_t)ncols);
  L.sti = m->ws_stat_i.reserve(3 * (size_t)ncols);
  L.stl = m->ws_stat_l.reserve(4 * (size_t)ncols);
  L.stf = m->ws_stat_f.reserve(2 * (size_t)ncols);
  // misc: [0] queue (int32) [1] overflow (int32) [2..3] cursor (u64) [4] queue of the heavy phase
  L.misc = m->ws_misc.reserve(16);
  L.s = alloc_slabs(m, opt, p, L.t, nwork, L.nwaves);

  // output arena: a column of W holds at most ncols - 1 entries and, on the large
  // configurations, ~2.7K (C4, both densities) to ~4K (C5); columns that do not fit are
  // solved again with a larger arena (run_launches), so the size is only a matter of cost
  L.arena_cap = std::max<int64_t>(1 << 20, (int64_t)nwork * std::min<int64_t>(ncols, 8192));
  if (const char* env_cap = std::getenv("SLIM_GPU_ARENA")) L.arena_cap = std::max<int64_t>(1, std::atoll(env_cap));

  if (p.has_imodel && warm_dev) {  // no upload: the solver reads the resident column view
    L.incols = warm_dev->n;
    L.icolptr = warm_dev->d_colptr.get();
    L.icolind = warm_dev->d_colind.get();
    L.icolval = warm_dev->d_colval.get();
  } else if (p.has_imodel) {
    L.incols = imodel->ncols;
    const int64_t innz = imodel->colptr[L.incols];
    int64_t* cp = m->ws_icolptr.reserve((size_t)L.incols + 1);
    int32_t* ci = m->ws_icolind.reserve((size_t)innz);
    float* cv = m->ws_icolval.reserve((size_t)innz);
    HIP_TRY(hipMemcpyAsync(cp, imodel->colptr, sizeof(int64_t) * ((size_t)L.incols + 1),
                           hipMemcpyHostToDevice, stream));
    if (innz > 0) {
      HIP_TRY(hipMemcpyAsync(ci, imodel->colind, sizeof(int32_t) * (size_t)innz, hipMemcpyHostToDevice, stream));
      HIP_TRY(hipMemcpyAsync(cv, imodel->colval, sizeof(float) * (size_t)innz, hipMemcpyHostToDevice, stream));
    }
    L.icolptr = cp;
    L.icolind = ci;
    L.icolval = cv;
  }
  HIP_TRY(hipMemsetAsync(L.cnt, 0, sizeof(int32_t) * (size_t)ncols, stream));
  HIP_TRY(hipMemsetAsync(L.off, 0, sizeof(int64_t) * (size_t)ncols, stream));
  HIP_TRY(hipMemsetAsync(L.sti, 0, sizeof(int32_t) * 3 * (size_t)ncols, stream));
  HIP_TRY(hipMemsetAsync(L.stl, 0, sizeof(int64_t) * 4 * (size_t)ncols, stream));
  HIP_TRY(hipMemsetAsync(L.stf, 0, sizeof(float) * 2 * (size_t)ncols, stream));

  // screen-sum cache: read when this very work list was solved last time in this geometry,
  // else record (if the [tiles][ncols][P] array fits comfortably next to everything else)
  const TileGeom& t = L.t;
  const int geom[6] = {p.tileP, t.clusterK, t.nheavy > 0 ? t.clusterHi : 0, t.nheavy, opt.shard_count,
                       opt.shard_index};
  std::copy(geom, geom + 6, L.gram_geom);
  if (p.use_tile && !opt.build_G && !std::getenv("SLIM_GPU_NO_GRAM")) {
    const size_t ngroups0 = ((size_t)nwork + p.tileP - 1) / p.tileP;
    const size_t need = ngroups0 * t.tile_x * sizeof(float);
    if (!m->gram_order.empty() && m->gram_order == order && m->ws_gram.bytes() >= need &&
        std::equal(geom, geom + 6, m->gram_geom)) {
      L.gram_mode = 2;
      L.gram = m->ws_gram.get();
    } else {
      size_t free_b = 0, total_b = 0;
      HIP_TRY(hipMemGetInfo(&free_b, &total_b));
      // (a quarter of what is free, 32 GB at most: a second handle or a replica on the same
      // device must still find room -- and the cache is dropped whenever a workspace needs it)
      if (need <= (size_t(32) << 30) && need <= (free_b + m->ws_gram.bytes()) / 4) {
        m->gram_order.clear();  // (invalid while it is being rewritten)
        L.gram = m->ws_gram.reserve(need / sizeof(float));
        L.gram_mode = 1;
      }
    }
  }

  // g carried between the solves of a grid (slimgpu_model::d_gsave): all columns of an unsharded
  // solve on the packed kernel, the model staying in HBM
  const int carry_groups = std::max(p.gramr_kr, 1) + p.gramr_kl;
  if (resident && p.use_gramr && carry_groups <= kGramrCarryMaxGroups && all_columns && nwork == ncols &&
      opt.shard_count == 1 && !std::getenv("SLIM_GPU_NO_CARRY")) {
    L.carry_stride = (int64_t)carry_groups * 8192;
    const size_t carry_bytes = sizeof(float) * (size_t)ncols * (size_t)L.carry_stride;
    if (warm_dev && warm_dev->d_gsave.get() && warm_dev->gsave_owner == m->uid &&
        warm_dev->gsave_stride == L.carry_stride && warm_dev->n == ncols) {
      // the previous model's buffer: read where l1 is the same, overwritten in place either way, and
      // no longer that model's from here on (a failure below leaves nothing half-valid behind)
      L.carry_from_warm = warm_dev->gsave_valid && warm_dev->gsave_l1 == opt.l1r;
      L.carry = std::move(warm_dev->d_gsave);
      warm_dev->gsave_valid = false;
    } else {
      size_t free_b = 0, total_b = 0;
      HIP_TRY(hipMemGetInfo(&free_b, &total_b));
      if (carry_bytes <= (size_t(8) << 30) && carry_bytes * 4 <= free_b)
        L.carry = DeviceBuffer<float>((size_t)ncols * (size_t)L.carry_stride);
    }
  }
}

// The kernel arguments of one launch over `pending` (attempt: 0 first, > 0 an arena retry).
SolveArgs solve_args(slimgpu_matrix* m, const LearnOptions& opt, Launch& L, const std::vector<int32_t>& pending,
                     int attempt, int32_t* d_ai, float* d_av) {
  const Path& p = L.p;
  const TileGeom& t = L.t;
  const int32_t ncols = m->ncols, npend = (int32_t)pending.size();
  hipStream_t stream = m->stream;
  SolveArgs S;
  S.l1 = (float)opt.l1r;
  S.l2 = (float)opt.l2r;
  S.opt_tol = (float)opt.optTol;
  S.maxniters = opt.maxniters;
  S.seed = opt.seed;
  S.nnbrs = opt.nnbrs;
  S.simtype = opt.simtype;
  S.order = L.order;
  S.nwork = npend;
  S.queue = L.misc;
  S.icolptr = L.icolptr;
  S.icolind = L.icolind;
  S.icolval = L.icolval;
  S.incols = L.incols;
  S.slab = L.s.slab;
  S.slab_stride = p.use_tile ? (int64_t)t.tile_r : (int64_t)p.vec_floats;
  S.nrows_pad = p.nrows_pad;
  S.ncols_pad = p.ncols_pad;
  S.xslab = L.s.xslab;
  S.x_stride = (int64_t)t.tile_x;
  S.ulist = L.s.ulist;
  S.u_stride = (int64_t)t.tile_u;
  S.ngroups = (npend + p.tileP - 1) / p.tileP;
  if (opt.build_G && opt.G_rows_end >= 0) S.ngroups = (L.G_block + p.tileP - 1) / p.tileP;
  S.cluster = t.clusterK;
  S.ubounds = p.use_tile ? m->split[t.cluster_lg].ubounds.get() : nullptr;
  S.csplit = p.use_tile ? m->split[t.cluster_lg].csplit.get() : nullptr;
  S.mailbox = L.s.mailbox;
  S.exact_gram = p.exact_gram ? 1 : 0;  // (decided in finish_path, where the trace names it)
  S.atypart = L.s.part;
  S.bm_shift = L.s.bm_shift;
  S.bm_words = L.s.bm_words;
  S.nheavy = p.use_tile ? t.nheavy : 0;
  S.cluster_hi = t.clusterHi;
  S.ubounds_hi = t.nheavy > 0 ? m->split[t.hi_lg].ubounds.get() : nullptr;
  S.csplit_hi = t.nheavy > 0 ? m->split[t.hi_lg].csplit.get() : nullptr;
  S.mailbox_hi = L.s.mailbox ? L.s.mailbox + (size_t)std::max(t.nclusters, 1) * mailbox_stride(p.tileP) : nullptr;
  S.queue_hi = L.misc + 4;
  S.hi_prefetch = 1;
  S.shard_count = opt.shard_count;
  S.shard_index = opt.shard_index;
  S.nnz_last = m->nnz > 0 ? m->nnz - 1 : 0;
  S.xcd_swizzle = 0;
  // (valid for the first launch over the whole work list only: a retry solves a subset,
  // the fallback another geometry)
  S.gram_mode = (attempt == 0 && !L.cluster_fallback) ? L.gram_mode : 0;
  S.gram = L.gram;
  S.G = m->ws_G.get();  // (nullptr once dropped: only the float kernels read it)
  S.G_ld = m->G_ld;
  S.tile_nunion = L.s.nunion;
  S.gram_pos = nullptr;
  // (2: lanes = columns, bit-sliced counters; SLIM_GPU_GBITS=1: the round-4 form, one column
  // per wavefront and 32 ballots per 64 nnz)
  S.gram_bits = (p.gram_bits_lds && t.clusterK == 32 && L.s.gram_words) ? 2 : 0;
  if (const char* e = std::getenv("SLIM_GPU_GBITS"); e && S.gram_bits) S.gram_bits = std::atoi(e) == 1 ? 1 : 2;
  S.gram_split_stride = t.clusterK + 1;
  S.gram_accum = 0;
  S.gram_store = 0;
  S.gram_read = 0;
  S.gview = nullptr;  // (run_launches: build_gview)
  S.gview_base = nullptr;
  S.gview_cnt = nullptr;
  S.gview_ngroups = 0;
  S.gview_range0 = 0;
  S.gview_sentinel = 0;
  // (SLIM_GPU_GPART16=0: float partial sums, as the other forms write them)
  S.gram_part16 = S.gram_bits == 2 ? 1 : 0;
  if (const char* e = std::getenv("SLIM_GPU_GPART16"); e && std::atoi(e) == 0) S.gram_part16 = 0;
  S.g_save = nullptr;
  S.g_load = nullptr;
  S.g_stride = 0;
  if (L.carry.get()) {  // (resident models on the packed kernel: g carried from pair to pair, see slimgpu_model)
    S.g_save = L.carry.get();
    S.g_stride = L.carry_stride;
    // (a retry re-solves a column whose slot already holds this solve's result: it folds again)
    S.g_load = (L.carry_from_warm && attempt == 0) ? L.carry.get() : nullptr;
  }
  if (L.p.gram_passes > 1) {
    if (S.gram_bits) {  // pass gram_pass of gram_passes: this launch's 32 user ranges
      S.ubounds = m->gsplit.ubounds.get() + 32 * L.gram_pass;
      S.csplit = m->gsplit.csplit.get() + 32 * L.gram_pass;
      S.gram_split_stride = 32 * L.p.gram_passes + 1;
      S.gram_accum = L.gram_pass > 0;
    } else {  // (re-planned without clusters: one launch forms all of G from the top)
      L.p.gram_passes = 1;
      L.gram_pass = 0;
    }
  }
  if (opt.build_G) {
    // (the symmetric fill needs every column in ONE launch; a re-plan after a cluster
    // timeout starts the fill again from the top with the whole list)
    if (npend != ncols)
      throw Refusal{SLIM_ERROR, "SLIMGPU_Learn: internal: G = R^T R must be built over all columns at once"};
    std::vector<int32_t> pos((size_t)ncols, 0);
    for (int32_t k = 0; k < npend; ++k) pos[(size_t)pending[(size_t)k]] = k;
    int32_t* d_pos = m->ws_nunion.reserve((size_t)ncols, evict_cache(m));
    HIP_TRY(hipMemcpyAsync(d_pos, pos.data(), sizeof(int32_t) * (size_t)ncols, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // (pos is a local)
    S.gram_pos = d_pos;
    S.gram_mode = 3;
    // How the sums leave the tiles (SolveArgs::gram_store): in whole lines, and on the path that forms
    // all of G the mirror half by gram_sym_kernel after the last launch (run_launches).  Row blocks keep
    // the mirror stores in the tile kernel: their lists run the block's tiles only.
    // SLIM_GPU_GLINES=1: whole lines with the mirror stores, no pass; =0: the form before both (A/B runs)
    S.gram_store = opt.G_rows_end >= 0 ? 1 : 2;
    if (const char* e = std::getenv("SLIM_GPU_GLINES"); e && std::atoi(e) >= 0 && std::atoi(e) < S.gram_store)
      S.gram_store = std::atoi(e);
    // (the launch's LDS holds a staging tile per wavefront: finish_path, alloc_slabs)
    S.gram_read = (S.gram_store != 0 && p.gram_stage_lds && L.s.tile_lds >= p.gram_stage_lds) ? 1 : 0;
  }
  if (p.use_gram) {
    S.slab_stride = (int64_t)p.ncols_pad;
    S.x_stride = (int64_t)p.ncols_pad;
    S.u_stride = (int64_t)p.ncols_pad;
    S.ngroups = (npend + 31) / 32;
  }
  if (p.use_fgram) {
    S.u_stride = (int64_t)p.f_ustride;
    S.ngroups = (npend + 31) / 32;
  }
  if (const char* e = std::getenv("SLIM_GPU_HI_PREFETCH")) S.hi_prefetch = std::atoi(e);
  if (p.use_tile)
    HIP_TRY(hipMemsetAsync(L.s.mailbox, 0, sizeof(unsigned long long) * L.s.mailbox_words, stream));
  S.trace = nullptr;
  if (p.use_tile && p.trace_level >= 1) {
    S.trace = m->ws_trace.reserve(16 * (size_t)S.ngroups);
    HIP_TRY(hipMemsetAsync(S.trace, 0, sizeof(uint64_t) * 16 * (size_t)S.ngroups, stream));
  }
  S.out_cnt = L.cnt;
  S.out_off = L.off;
  S.out_ind = d_ai;
  S.out_val = d_av;
  S.out_cursor = reinterpret_cast<unsigned long long*>(L.misc + 2);
  S.out_cap = L.arena_cap;
  S.overflow = L.misc + 1;
  S.st_na = L.sti;
  S.st_sweeps = L.sti + ncols;
  S.st_conv = L.sti + 2 * (size_t)ncols;
  S.st_G = L.stl;
  S.st_D = L.stl + ncols;
  S.st_U = L.stl + 2 * (size_t)ncols;
  S.st_B = L.stl + 3 * (size_t)ncols;
  S.st_err = L.stf;
  S.st_obj = L.stf + ncols;
  return S;
}

// The bit-sliced G builder's view of the column ids (SolveArgs::gview, cd_tile.hpp), over every user
// range of the split in use (all passes) and the work list of this build, which S holds as its first
// launch sees them.  Built before that launch, dropped when the build ends (run_launches).  Without it
// -- SLIM_GPU_GVIEW=0, a range too long for 16-bit ids, no room in HBM -- the builder reads the
// column view as it always did: the same G.
void build_gview(slimgpu_matrix* m, Launch& L, const SolveArgs& S, const int32_t* d_colind) {
  L.gview_tried = true;
  if (const char* e = std::getenv("SLIM_GPU_GVIEW"); e && std::atoi(e) == 0) {
    L.gview_why = " (SLIM_GPU_GVIEW=0)";
    return;
  }
  hipStream_t stream = m->stream;
  const double t0 = now_ms();
  const int nranges = 32 * L.p.gram_passes;
  const int ngroups = (S.nwork + 63) / 64;
  // the spare word: behind every range's users, inside the LDS words (round_up(max_rows, 64) + 64 of them)
  const int sentinel = S.bm_words - 64;
  if ((int64_t)nranges * ngroups >= (int64_t(1) << 31) || sentinel >= 65536 || sentinel < 0) {
    L.gview_why = " (ranges beyond 16-bit ids)";
    return;
  }
  const int nblocks = nranges * ngroups;
  try {
    int32_t* d_rows = m->ws_gvrows.reserve((size_t)nblocks);
    int64_t* d_base = m->ws_gvbase.reserve((size_t)nblocks + 1);
    uint16_t* d_cnt = m->ws_gvcnt.reserve((size_t)nblocks * 64);
    const dim3 grid((unsigned)((nblocks + 3) / 4)), block(256);
    hipLaunchKernelGGL(k_gview_rows, grid, block, 0, stream, S.order, S.nwork, S.csplit, S.gram_split_stride, ngroups,
                       nblocks, d_rows, d_cnt);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> rows((size_t)nblocks);
    HIP_TRY(hipMemcpyAsync(rows.data(), d_rows, sizeof(int32_t) * rows.size(), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::vector<int64_t> base((size_t)nblocks + 1, 0);
    for (int b = 0; b < nblocks; ++b) base[(size_t)b + 1] = base[(size_t)b] + rows[(size_t)b];
    const int64_t total = base[(size_t)nblocks];
    uint4* d_view = m->ws_gview.reserve((size_t)std::max<int64_t>(total, 1), evict_cache(m));
    HIP_TRY(hipMemcpyAsync(d_base, base.data(), sizeof(int64_t) * base.size(), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_gview_fill, grid, block, 0, stream, S.order, S.nwork, S.csplit, S.gram_split_stride, S.ubounds,
                       d_colind, ngroups, nblocks, d_base, (uint32_t)sentinel, d_view);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));  // (base is a local)
    L.gview = d_view;
    L.gview_base = d_base;
    L.gview_cnt = d_cnt;
    L.gview_ngroups = ngroups;
    L.gview_sentinel = sentinel;
    L.gview_bytes = (size_t)total * 16;
    L.gview_ms = now_ms() - t0;
  } catch (const HipFail& e) {
    if (e.code != hipErrorOutOfMemory) throw;
    (void)hipGetLastError();
    m->ws_gview.reset();
    L.gview_why = " (no room for the 16-bit view)";
  }
}

// SLIM_GPU_TRACE: the per-tile timeline of a launch -- where does it spend its time?
void print_tile_trace(const slimgpu_matrix* m, const Launch& L, const SolveArgs& S, const std::vector<int32_t>& pending,
                      int launch_waves, float ms) {
  const int clusterK = L.t.clusterK, tileP = L.p.tileP, npend = (int)pending.size();
  std::vector<uint64_t> tr(16 * (size_t)S.ngroups);
  HIP_TRY(hipMemcpy(tr.data(), S.trace, sizeof(uint64_t) * tr.size(), hipMemcpyDeviceToHost));
  uint64_t t0 = ~0ull, t1 = 0;
  double busy = 0, setup = 0, sweeps = 0, fold = 0;
  std::vector<double> dur;
  for (int gI = 0; gI < S.ngroups; ++gI) {
    const uint64_t* e = &tr[8 * (size_t)gI];
    t0 = std::min(t0, e[0]);
    t1 = std::max(t1, e[3]);
    const double wk = double(e[6]) / clusterK;  // heavy tiles occupy more workgroups
    busy += double(e[3] - e[0]) * wk;
    setup += double(e[1] - e[0]) * wk;
    sweeps += double(e[2] - e[1]) * wk;
    fold += double(e[7] - e[1]) * wk;  // warm-start fold (part of "sweeps")
    dur.push_back(double(e[3] - e[0]) * 1e-5);
  }
  std::sort(dur.begin(), dur.end());
  const double span = double(t1 - t0);
  std::fprintf(stderr,
               "[trace] tiles %d (%d heavy, clusters of %d) on %d workgroups (clusters of %d): span %.2f ms (event %.2f ms), busy/"
               "(span*wgs) %.2f, setup %.1f%% sweeps %.1f%% (fold %.1f%%) of busy; tile ms min %.2f med "
               "%.2f p90 %.2f max %.2f\n",
               S.ngroups, S.nheavy, S.nheavy > 0 ? L.t.clusterHi : 0, launch_waves, clusterK, span * 1e-5, ms,
               busy * clusterK / (span * launch_waves), 100 * setup / busy, 100 * sweeps / busy,
               100 * fold / busy,
               dur.front(), dur[dur.size() / 2], dur[dur.size() * 9 / 10], dur.back());
  if (S.ngroups >= 16) {  // queue order = cost order: (estimated cost, measured ms)
    std::fprintf(stderr, "[trace] tile cost -> ms, queue order:");
    for (int k = 0; k < 19; ++k) {
      const int gI = k < 12 ? k : (int)((int64_t)S.ngroups * (k - 11) / 8) - (k == 19 ? 1 : 0);
      if (gI >= S.ngroups) break;
      double c = 0;
      for (int j = gI * tileP; j < std::min((gI + 1) * tileP, npend); ++j)
        c += (double)m->h_cost[pending[(size_t)j]];
      std::fprintf(stderr, " [%d] %.3g -> %.0f", gI, c,
                   double(tr[8 * (size_t)gI + 3] - tr[8 * (size_t)gI]) * 1e-5);
    }
    std::fprintf(stderr, "\n");
  }
  if (L.p.trace_level >= 2) {
    double ph[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int gI = 0; gI < S.ngroups; ++gI)
      for (int k = 0; k < 7; ++k) ph[k] += double(tr[8 * (size_t)S.ngroups + 8 * (size_t)gI + k]);
    const double tot = ph[0] + ph[1] + ph[2] + ph[3] + ph[4];
    std::fprintf(stderr,
                 "[trace] visit phases (shader clocks/visit): loads %.0f reduce+barrier %.0f "
                 "math %.0f stores %.0f closing barrier %.0f | total %.0f; visits %.0f, "
                 "%.1f%% with update\n",
                 ph[0] / ph[5], ph[1] / ph[5], ph[2] / ph[5], ph[3] / ph[5], ph[4] / ph[5],
                 tot / ph[5], ph[5], 100 * ph[6] / ph[5]);
  }
}

// What the launches left: per-column counts and offsets into the entries, the entries themselves
// (host vectors, or the arena pieces of a resident solve, in launch order).
struct Entries {
  std::vector<int32_t> cnt;
  std::vector<int64_t> off;
  int64_t total = 0;
  std::vector<int32_t> ind;
  std::vector<float> val;
  std::vector<ArenaSeg> segs;
  double kernel_ms = 0, d2h_ms = 0;
};

// The launches: the whole work list, then again every column that overflowed the arena (with a
// larger one), the void launch of a cluster that timed out re-planned without clusters, and the G
// builder's user passes.
Entries run_launches(slimgpu_matrix* m, const LearnOptions& opt, const std::vector<int32_t>& order, bool resident,
                     Launch& L) {
  const int32_t ncols = m->ncols;
  hipStream_t stream = m->stream;
  const Path& p = L.p;
  struct EventPair {  // released on every exit path
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } events;
  HIP_TRY(hipEventCreate(&events.a));
  HIP_TRY(hipEventCreate(&events.b));
  const hipEvent_t ev0 = events.a, ev1 = events.b;
  DevMatrix A;
  A.nrows = m->nrows;
  A.ncols = ncols;
  A.nnz = m->nnz;
  A.rowptr = m->d_rowptr;
  A.rowind = m->d_rowind;
  A.rowval = m->d_rowval;
  A.colptr = m->d_colptr.get();
  A.colind = m->d_colind.get();
  A.colval = m->d_colval.get();
  A.cnorm = m->d_cnorm.get();
  A.csq = m->d_csq.get();
  GramPacked P{};
  if (p.use_gramr) {
    P.lo = m->ws_Glo.get();
    P.ldb = m->Gp_ldb;
    P.hi = m->ws_Ghi.get();
    P.hi_off = m->ws_hioff.get();
    P.hi_k = m->ws_hik.get();
    P.hi2_off = m->ws_hi2off.get();
    P.hi2_k = m->ws_hi2k.get();
    P.base = m->ws_Gbase.get();
    P.diag = m->ws_Gdiag.get();
    P.meta = m->ws_Gmeta.get();
    P.rank_of = m->ws_rankof.get();
    P.item_of = m->ws_itemof.get();
    P.nchunks = m->Gp_nchunks;
  }

  struct DropView {  // the id view of a G build ends with the build, on every exit path
    slimgpu_matrix* m;
    ~DropView() {
      m->ws_gview.reset();
      m->ws_gvbase.reset();
      m->ws_gvrows.reset();
      m->ws_gvcnt.reset();
    }
  } drop_view{m};

  Entries E;
  E.cnt.assign((size_t)ncols, 0);
  E.off.assign((size_t)ncols, 0);
  std::vector<int32_t> h_cnt((size_t)ncols, 0);
  std::vector<int64_t> h_off((size_t)ncols, 0);
  std::vector<int32_t> pending = order;  // columns still to solve
  for (int attempt = 0; attempt < 8 && !pending.empty(); ++attempt) {
    const int32_t npend = (int32_t)pending.size();
    int32_t* d_ai = m->ws_arena_i.reserve((size_t)L.arena_cap, evict_cache(m));
    float* d_av = m->ws_arena_v.reserve((size_t)L.arena_cap, evict_cache(m));
    if (L.gram_mode != 0 && m->ws_gram.get() != L.gram) {
      // the arena did not fit next to the screen-sum cache and reserve gave the cache up
      // (drop_screen_cache): this launch neither records nor reads it
      L.gram_mode = 0;
      L.gram = nullptr;
    }
    HIP_TRY(hipMemcpyAsync(L.order, pending.data(), sizeof(int32_t) * (size_t)npend, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(L.misc, 0, sizeof(int32_t) * 16, stream));
    if (attempt > 0) L.t.nheavy = 0;  // a retry regroups what is left: plain clusters
    SolveArgs S = solve_args(m, opt, L, pending, attempt, d_ai, d_av);
    const int clusterK = L.t.clusterK;
    if (opt.build_G && S.gram_bits == 2 && !L.gview_tried) build_gview(m, L, S, A.colind);
    if (opt.build_G && S.gram_bits == 2 && L.gview) {
      S.gview = L.gview;
      S.gview_base = L.gview_base;
      S.gview_cnt = L.gview_cnt;
      S.gview_ngroups = L.gview_ngroups;
      S.gview_range0 = 32 * L.gram_pass;
      S.gview_sentinel = L.gview_sentinel;
    }
    if (opt.build_G && p.trace_level >= 1) {  // which form of the G builder this launch is (cd_tile.hpp, gram_mode 3)
      const bool in_passes = S.gram_bits != 0 && p.gram_passes > 1;
      std::fprintf(stderr, "[trace] G builder: form %s, clusters of %d, pass %d of %d, %d users at most per member\n",
                   S.gram_bits == 2 ? "bits2" : (S.gram_bits == 1 ? "bits1" : "lines"), clusterK, L.gram_pass + 1,
                   p.gram_passes, in_passes ? m->gsplit.max_rows : m->split[L.t.cluster_lg].max_rows);
      if (S.gview)
        std::fprintf(stderr, "[trace] G builder: ids from view, %zu bytes = %.3f x 2 bytes per nnz, built in %.1f ms\n",
                     L.gview_bytes, (double)L.gview_bytes / (2.0 * (double)std::max<int64_t>(m->nnz, 1)), L.gview_ms);
      else
        std::fprintf(stderr, "[trace] G builder: ids from csc%s\n", S.gram_bits == 2 ? L.gview_why : "");
      if (S.gram_read)  // how gram_store_lines reads the members' partial sums
        std::fprintf(stderr, "[trace] G builder: sums read once, %zu of %zu bytes of LDS hold the staging tiles\n",
                     p.gram_stage_lds, L.s.tile_lds);
      else if (S.gram_store != 0)
        std::fprintf(stderr, "[trace] G builder: sums read in rounds (%s)\n", p.gram_stage_why);
    }

    // clustered tiles: always launch whole clusters (every member must be resident)
    const int launch_waves = p.use_tile ? std::max(1, std::min((npend + p.tileP - 1) / p.tileP, L.t.nclusters)) * clusterK
                                        : std::max(1, std::min(npend, L.nwaves));
    HIP_TRY(hipEventRecord(ev0, stream));
    // the union of the active sets of every tile, read off G (inside kernel_ms): off the byte
    // planes when the packed solver runs (the floats may be gone: drop_float_gram)
    if (p.use_gramr)
      hipLaunchKernelGGL(gramr_union_fn(), dim3(S.ngroups), dim3(gramr_union_threads()), 0, stream, A, S, P);
    else if (p.use_gram)
      hipLaunchKernelGGL(gram_union_fn(), dim3(S.ngroups), dim3(64), 0, stream, A, S);
    // the heavy phase needs at least one whole big cluster in the launch
    if (S.nheavy > 0 && launch_waves < L.t.clusterHi) S.nheavy = 0;
    // test hook: launch the last cluster one member short, which is what a CU mask or a
    // second tenant does to a cluster -- exercises the timeout + fallback path below
    int launch_now = launch_waves;
    // (acts only together with the master switch SLIM_GPU_TEST_HOOKS=1: an inherited
    // environment must not void production launches)
    if (p.use_tile && clusterK > 1 && !L.cluster_fallback && test_hook("SLIM_GPU_TEST_DROP_MEMBER")) {
      launch_now -= 1;
      S.nheavy = 0;
    }
    // members of a cluster on one XCD (one L2): matters for the row-wise fold, whose x lines
    // are shared by the cluster; placement only, never correctness
    // (8 XCDs of 32 CUs on this part; asked of the device as CUs / 32, so that a partition mode
    // or another part does not get a placement that straddles XCDs: clusters must tile an XCD's
    // share of the launch)
    const int nxcd = m->num_cus % 32 == 0 ? m->num_cus / 32 : 1;
    if (p.use_tile && clusterK > 1 && nxcd == 8 && launch_now % 8 == 0 &&
        (launch_now / 8) % clusterK == 0 && (S.nheavy == 0 || (launch_now / 8) % L.t.clusterHi == 0)) {
      S.xcd_swizzle = 1;
      if (const char* e = std::getenv("SLIM_GPU_XCD")) S.xcd_swizzle = std::atoi(e) != 0;
    }
    if (p.use_fgram) {
      // select -> union -> solve over every slice of the work list (whole tiles; one slice unless the
      // lists would not fit): all inside kernel_ms
      FslimArgs F{};
      F.stride = p.f_stride;
      F.nbr_n = L.s.f_n;
      F.nbr_id = L.s.f_id;
      F.nbr_aty = L.s.f_aty;
      F.nbr_slot = L.s.f_slot;
      F.wave_lds = (int32_t)p.f_wave_lds;
      F.tab_n = p.f_tab_n;
      const int slice = L.s.f_slice_tiles * 32;
      for (int pos0 = 0; pos0 < npend; pos0 += slice) {
        F.pos0 = pos0;
        F.npos = std::min(slice, npend - pos0);
        if (pos0 > 0) HIP_TRY(hipMemsetAsync(L.misc, 0, sizeof(int32_t), stream));  // (the queue head)
        hipLaunchKernelGGL(fslim_select_fn(), dim3(F.npos), dim3(kFslimSelectThreads), 0, stream, A, S, F);
        hipLaunchKernelGGL(fslim_union_fn(), dim3((F.npos + 31) / 32), dim3(kFslimUnionThreads), p.f_union_lds, stream,
                           A, S, F);
        hipLaunchKernelGGL(p.fn_f, dim3(std::max(1, std::min((F.npos + p.f_waves - 1) / p.f_waves, L.nwaves))),
                           dim3(64 * p.f_waves), p.f_wave_lds * (size_t)p.f_waves, stream, A, S, F);
        HIP_TRY(hipGetLastError());
      }
    } else if (p.use_gramr)
      hipLaunchKernelGGL(p.fn_r, dim3(launch_now), dim3(kGramrNT), p.gram_lds, stream, A, S, P);
    else
      hipLaunchKernelGGL(p.fn, dim3(launch_now), dim3(p.use_gram ? 64 * p.gram_nw : (p.use_tile ? 64 * p.tileNW : 64)),
                         p.use_gram ? p.gram_lds : (p.use_lds ? p.lds_need : (p.use_tile ? L.s.tile_lds : 0)),
                         stream, A, S);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, stream));

    int32_t h_misc[4];
    HIP_TRY(hipMemcpyAsync(h_misc, L.misc, sizeof(h_misc), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_cnt.data(), L.cnt, sizeof(int32_t) * (size_t)ncols, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_off.data(), L.off, sizeof(int64_t) * (size_t)ncols, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    E.kernel_ms += ms;
    if (S.trace) print_tile_trace(m, L, S, pending, launch_waves, ms);

    if (h_misc[1] == 2) {
      // A cluster waited ~10 s for a member that never published: not every workgroup of the
      // launch was resident (CU mask, another tenant on the device).  The launch is void;
      // solve everything that is pending again without clusters -- that geometry has no
      // inter-workgroup dependency, so it completes on any number of compute units.
      if (!L.cluster_fallback && (clusterK > 1 || L.t.nheavy > 0)) {
        L.cluster_fallback = true;
        std::fprintf(stderr, "[slim-gpu] tile cluster timed out (workgroups not co-resident); "
                             "re-solving %d columns without clusters\n", npend);
        L.t = plan_tiles(m, opt, p, order, true);
        L.nwaves = L.t.nwaves;
        L.s = alloc_slabs(m, opt, p, L.t, (int32_t)order.size(), L.nwaves);
        --attempt;  // the void launch does not count as an arena retry
        continue;
      }
      throw Refusal{SLIM_ERROR, "SLIMGPU_Learn: a tile cluster timed out waiting for a member workgroup "
                                "(were all workgroups resident?)"};
    }
    if (p.gram_passes > 1 && ++L.gram_pass < p.gram_passes) {
      --attempt;  // the same work list again, over the next user ranges
      continue;
    }
    if (opt.build_G && S.gram_store == 2) {
      // every tile of the build has written its own rows (with user passes: this was the last one):
      // the mirror half in one pass (gram_sym.hpp), counted with the build's kernels
      const unsigned nb = (unsigned)((ncols + kSymB - 1) / kSymB);
      int logp = 0;
      while ((1 << logp) < p.tileP) ++logp;
      HIP_TRY(hipEventRecord(ev0, stream));
      hipLaunchKernelGGL(gram_sym_fn(), dim3(nb, nb), dim3(kSymNT), 0, stream, S.G, S.G_ld, ncols, S.gram_pos, logp);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(ev1, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      float sym_ms = 0;
      HIP_TRY(hipEventElapsedTime(&sym_ms, ev0, ev1));
      E.kernel_ms += sym_ms;
      if (p.trace_level >= 1)
        std::fprintf(stderr, "[trace] G builder: mirror half filled in %.2f ms (%u x %u blocks of %d)\n", sym_ms, nb, nb,
                     kSymB);
    }
    if (S.gram_mode == 1) {  // the launch completed: its screen sums are reusable
      m->gram_order = order;
      std::copy(L.gram_geom, L.gram_geom + 6, m->gram_geom);
    }
    unsigned long long cursor;
    std::memcpy(&cursor, h_misc + 2, sizeof(cursor));
    const int64_t used = std::min<int64_t>((int64_t)cursor, L.arena_cap);
    const int64_t base = E.total;
    const double t_d2h = now_ms();
    if (resident) {  // the arena stays where it is; a retry (below) moves it aside first
      E.segs.push_back({d_ai, d_av, used, {}, {}});
    } else {
      E.ind.resize((size_t)(base + used));
      E.val.resize((size_t)(base + used));
      if (used > 0) {
        HIP_TRY(hipMemcpyAsync(E.ind.data() + base, d_ai, sizeof(int32_t) * (size_t)used, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(E.val.data() + base, d_av, sizeof(float) * (size_t)used, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
      }
    }
    E.d2h_ms += now_ms() - t_d2h;
    E.total += used;

    std::vector<int32_t> again;
    int64_t need = 0;
    for (int32_t c : pending) {
      if (h_cnt[c] >= 0) {
        E.cnt[c] = h_cnt[c];
        E.off[c] = base + h_off[c];
      } else {  // did not fit the arena: solve again with a larger one
        again.push_back(c);
        need += -(int64_t)h_cnt[c] - 1;
      }
    }
    pending.swap(again);
    if (!pending.empty()) L.arena_cap = std::max<int64_t>(L.arena_cap, need + 1024);
    if (resident && !pending.empty() && used > 0) {  // the next attempt overwrites the arena
      ArenaSeg& sg = E.segs.back();
      sg.own_i = DeviceBuffer<int32_t>((size_t)used);
      sg.own_v = DeviceBuffer<float>((size_t)used);
      HIP_TRY(hipMemcpyAsync(sg.own_i.get(), sg.ind, sizeof(int32_t) * (size_t)used, hipMemcpyDeviceToDevice, stream));
      HIP_TRY(hipMemcpyAsync(sg.own_v.get(), sg.val, sizeof(float) * (size_t)used, hipMemcpyDeviceToDevice, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      sg.ind = sg.own_i.get();
      sg.val = sg.own_v.get();
    }
  }
  if (!pending.empty()) throw Refusal{SLIM_ERROR_MEMORY, "SLIMGPU_Learn: output arena overflow persisted"};
  return E;
}

// The per-column counters of the solve (into cs), and the item-space kernel's byte model.
struct Counters {
  std::vector<float> err, obj;
  int64_t gram_rows = 0;  // item-space kernel: rows of G it read
  double gram_bytes = 0;
};

Counters read_counters(const slimgpu_matrix* m, const Launch& L, const std::vector<int32_t>& requested,
                       ColumnStats& cs) {
  const size_t ncols = (size_t)m->ncols;
  cs.nacols.assign(ncols, 0);
  cs.sweeps.assign(ncols, 0);
  cs.conv.assign(ncols, 0);
  cs.G.assign(ncols, 0);
  cs.D.assign(ncols, 0);
  cs.U.assign(ncols, 0);
  Counters k;
  k.err.resize(ncols);
  k.obj.resize(ncols);
  HIP_TRY(hipMemcpy(cs.nacols.data(), L.sti, sizeof(int32_t) * ncols, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cs.sweeps.data(), L.sti + ncols, sizeof(int32_t) * ncols, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cs.conv.data(), L.sti + 2 * ncols, sizeof(int32_t) * ncols, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cs.G.data(), L.stl, sizeof(int64_t) * ncols, hipMemcpyDeviceToHost));
  if (L.p.use_gram) {
    for (int32_t c : requested) k.gram_rows += cs.G[(size_t)c];
    if (L.p.use_gramr) {  // packed rows: the bytes each column's updates streamed, counted on the device
      std::vector<int64_t> hb(ncols);
      HIP_TRY(hipMemcpy(hb.data(), L.stl + 3 * ncols, sizeof(int64_t) * ncols, hipMemcpyDeviceToHost));
      for (int32_t c : requested) k.gram_bytes += (double)hb[(size_t)c];
    } else {
      k.gram_bytes = (double)k.gram_rows * 4.0 * (double)L.p.ncols_pad;
    }
  }
  if (L.p.use_tile || L.p.use_gram || L.p.use_fgram)  // the Gram work of a column is the staging pass's cost figure
    for (int32_t c : requested) cs.G[(size_t)c] = m->h_cost[(size_t)c];
  HIP_TRY(hipMemcpy(cs.D.data(), L.stl + ncols, sizeof(int64_t) * ncols, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cs.U.data(), L.stl + 2 * ncols, sizeof(int64_t) * ncols, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(k.err.data(), L.stf, sizeof(float) * ncols, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(k.obj.data(), L.stf + ncols, sizeof(float) * ncols, hipMemcpyDeviceToHost));
  return k;
}

// SaveModel (estimate.c:570-593): concatenate the columns, then the row view.
slim_csr_t* assemble_host_model(int32_t ncols, const Entries& E, int64_t tnnz, bool row_view) {
  ssize_t* colptr = static_cast<ssize_t*>(std::malloc(sizeof(ssize_t) * ((size_t)ncols + 1)));
  int32_t* colind = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (size_t)std::max<int64_t>(tnnz, 1)));
  float* colval = static_cast<float*>(std::malloc(sizeof(float) * (size_t)std::max<int64_t>(tnnz, 1)));
  if (!colptr || !colind || !colval) {
    std::free(colptr); std::free(colind); std::free(colval);
    throw Refusal{SLIM_ERROR_MEMORY, "SLIMGPU_Learn: out of host memory for the model"};
  }
  colptr[0] = 0;
  for (int32_t c = 0; c < ncols; ++c) {
    const int64_t n = E.cnt[c];
    if (n > 0) {
      std::memcpy(colind + colptr[c], E.ind.data() + E.off[c], sizeof(int32_t) * (size_t)n);
      std::memcpy(colval + colptr[c], E.val.data() + E.off[c], sizeof(float) * (size_t)n);
    }
    colptr[c + 1] = colptr[c] + n;
  }
  return model_from_columns(ncols, colptr, colind, colval, row_view);
}

// The same two steps on the device: the arena's columns gathered into column order, the row view
// by the staging pass's stable sort (transpose_on_device) -- nothing crosses PCIe unless the caller
// fetches the model (model_fetch).  carry: the g this solve left (the model takes it over).
std::unique_ptr<slimgpu_model> assemble_resident_model(slimgpu_matrix* m, const LearnOptions& opt, Entries& E,
                                                       int64_t tnnz, Launch& L, bool row_view,
                                                       double* t_columns_done) {
  const int32_t ncols = m->ncols;
  hipStream_t stream = m->stream;
  std::unique_ptr<slimgpu_model> dm(new slimgpu_model());
  dm->device = m->device;
  dm->n = ncols;
  dm->nnz = tnnz;
  std::vector<int64_t> h_colptr((size_t)ncols + 1, 0);
  for (int32_t c = 0; c < ncols; ++c) h_colptr[(size_t)c + 1] = h_colptr[(size_t)c] + E.cnt[(size_t)c];
  const int32_t* src_i = E.segs.empty() ? nullptr : E.segs[0].ind;
  const float* src_v = E.segs.empty() ? nullptr : E.segs[0].val;
  DeviceBuffer<int32_t> cat_i;
  DeviceBuffer<float> cat_v;
  if (E.segs.size() > 1) {  // (a column overflowed its arena: the launches' pieces, in order)
    cat_i = DeviceBuffer<int32_t>((size_t)std::max<int64_t>(E.total, 1));
    cat_v = DeviceBuffer<float>((size_t)std::max<int64_t>(E.total, 1));
    int64_t at = 0;
    for (const ArenaSeg& sg : E.segs) {
      if (sg.n > 0) {
        HIP_TRY(hipMemcpyAsync(cat_i.get() + at, sg.ind, sizeof(int32_t) * (size_t)sg.n, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(cat_v.get() + at, sg.val, sizeof(float) * (size_t)sg.n, hipMemcpyDeviceToDevice, stream));
      }
      at += sg.n;
    }
    src_i = cat_i.get();
    src_v = cat_v.get();
  }
  dm->d_colptr = DeviceBuffer<int64_t>((size_t)ncols + 1);
  dm->d_colind = DeviceBuffer<int32_t>((size_t)std::max<int64_t>(tnnz, 1));
  dm->d_colval = DeviceBuffer<float>((size_t)std::max<int64_t>(tnnz, 1));
  int64_t* d_src = m->ws_off.reserve((size_t)ncols, evict_cache(m));  // (the solver's own offsets: done with)
  HIP_TRY(hipMemcpyAsync(dm->d_colptr.get(), h_colptr.data(), sizeof(int64_t) * ((size_t)ncols + 1),
                         hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_src, E.off.data(), sizeof(int64_t) * (size_t)ncols, hipMemcpyHostToDevice, stream));
  if (tnnz > 0) {
    hipLaunchKernelGGL(k_gather_columns, dim3(grid_for((int64_t)ncols * 64, 256, m->num_cus * 16)), dim3(256),
                       0, stream, ncols, dm->d_colptr.get(), d_src, src_i, src_v, dm->d_colind.get(),
                       dm->d_colval.get());
    HIP_TRY(hipGetLastError());
  }
  *t_columns_done = now_ms();
  if (row_view) {
    transpose_on_device(m, ncols, tnnz, dm->d_colptr.get(), dm->d_colind.get(), dm->d_colval.get(), dm->d_rowptr,
                        dm->d_rowind, dm->d_rowval);
    // the longest row and the order inside the rows, for the scorers (8 bytes come down, once per model)
    int32_t* d_facts = m->ws_misc.reserve(2);
    int32_t facts[2] = {0, 0};
    HIP_TRY(hipMemsetAsync(d_facts, 0, sizeof(facts), stream));
    queue_row_facts(stream, m->num_cus, ncols, dm->d_rowptr.get(), dm->d_rowind.get(), d_facts);
    HIP_TRY(hipMemcpyAsync(facts, d_facts, sizeof(facts), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    dm->max_row = facts[0];
    dm->rows_sorted = facts[1] == 0;
  }
  HIP_TRY(hipStreamSynchronize(stream));
  if (L.carry.get()) {
    dm->d_gsave = std::move(L.carry);
    dm->gsave_valid = true;
    dm->gsave_stride = L.carry_stride;
    dm->gsave_l1 = opt.l1r;
    dm->gsave_owner = m->uid;
  }
  return dm;
}

// SLIM_DBG_PROGRESS, estimate.c:507-514: one line per solved column, in column order (the reference
// prints them as its threads finish).  Everything but "a0s" comes from the counters the kernels
// return; a0s (ComputeAvgZeroScore, estimate.c:627-662: the mean of the 10 largest predicted scores
// among the users that did NOT rate the item) is a diagnostic that costs one pass over R per column
// -- done here on the host, as the reference does, because this switch is for eyeballing small
// runs.  tmr: the reference prints a timer it never starts (estimate.c:377,514).
void print_progress(const slimgpu_matrix* m, const slim_csr_t* model, const std::vector<int32_t>& requested,
                    const ColumnStats& cs, const Counters& k) {
  const int32_t ncols = m->ncols;
  const ssize_t* colptr = model->colptr;
  const int32_t* colind = model->colind;
  const float* colval = model->colval;
  std::vector<int64_t> hp((size_t)m->nrows + 1);
  std::vector<int32_t> hi((size_t)std::max<int64_t>(m->nnz, 1));
  std::vector<float> hv(m->binary ? 0 : (size_t)std::max<int64_t>(m->nnz, 1));
  std::vector<int64_t> hcp((size_t)ncols + 1);
  HIP_TRY(hipMemcpy(hp.data(), m->d_rowptr, sizeof(int64_t) * hp.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hcp.data(), m->d_colptr.get(), sizeof(int64_t) * hcp.size(), hipMemcpyDeviceToHost));
  if (m->nnz > 0) {
    HIP_TRY(hipMemcpy(hi.data(), m->d_rowind, sizeof(int32_t) * (size_t)m->nnz, hipMemcpyDeviceToHost));
    if (!m->binary)
      HIP_TRY(hipMemcpy(hv.data(), m->d_rowval, sizeof(float) * (size_t)m->nnz, hipMemcpyDeviceToHost));
  }
  std::vector<int32_t> sorted = requested;
  std::sort(sorted.begin(), sorted.end());
  std::vector<double> xd((size_t)ncols, 0.0);
  std::vector<float> scores;
  for (int32_t c : sorted) {
    double nrm1 = 0.0;
    for (ssize_t e = colptr[c]; e < colptr[c + 1]; ++e) {
      xd[(size_t)colind[e]] = colval[e];
      nrm1 += colval[e];
    }
    scores.clear();
    for (int32_t u = 0; u < m->nrows; ++u) {
      bool has = false;
      double r = 0.0;
      for (int64_t e = hp[(size_t)u]; e < hp[(size_t)u + 1]; ++e) {
        if (hi[(size_t)e] == c) has = true;
        r += xd[(size_t)hi[(size_t)e]] * (m->binary ? 1.0 : (double)hv[(size_t)e]);
      }
      if (!has) scores.push_back((float)r);
    }
    const size_t ntop = std::min<size_t>(10, scores.size());
    std::partial_sort(scores.begin(), scores.begin() + (ptrdiff_t)ntop, scores.end(), std::greater<float>());
    float a0 = 0.0f;
    for (size_t j = 0; j < ntop; ++j) a0 += scores[j];
    for (ssize_t e = colptr[c]; e < colptr[c + 1]; ++e) xd[(size_t)colind[e]] = 0.0;
    const size_t i = (size_t)c;
    std::printf("Col: %5d %5zd rs: %3d nits: %4d nnz: %4d rsd: %.2le obj: %.2le ff: %.3lf nrm1: "
                "%.3lf a0s: %.3lf tmr: %.2le\n",
                c, (ssize_t)(hcp[i + 1] - hcp[i]), cs.conv[i], cs.sweeps[i], (int)(colptr[c + 1] - colptr[c]),
                (double)k.err[i], (double)k.obj[i], k.obj[i] != 0 ? (double)k.err[i] / (double)k.obj[i] : 0.0,
                nrm1, ntop ? (double)a0 / (double)ntop : 0.0, 0.0);
  }
  std::fflush(stdout);
}

// The solve's figures (last_stats()); the G build's times are charged to the solve that paid for it.
slimgpu_stats_t solve_stats(slimgpu_matrix* m, const Launch& L, const Entries& E, const Counters& k,
                            const ColumnStats& cs, const std::vector<int32_t>& requested, int64_t tnnz) {
  const Path& p = L.p;
  slimgpu_stats_t st;
  std::memset(&st, 0, sizeof(st));
  st.ncols_solved = (int32_t)requested.size();
  st.kernel = p.kernel;
  st.nwaves = L.nwaves;
  st.lds_bytes = p.use_lds ? (int32_t)p.lds_need : 0;
  st.setup_ms = m->setup_ms;
  st.kernel_ms = E.kernel_ms;
  for (int32_t c : requested) {
    st.G += cs.G[c];
    st.D += cs.D[c];
    st.U += cs.U[c];
    st.sweeps += cs.sweeps[c];
    st.error += k.err[c];
    st.objval += k.obj[c];
  }
  st.nnzW = tnnz;
  st.alg_bytes = m->binary ? 4.0 * st.G + 8.0 * st.D + 4.0 * st.U + 8.0 * st.nnzW
                           : 8.0 * st.G + 12.0 * st.D + 4.0 * st.U + 8.0 * st.nnzW;
  if (p.use_gram || p.use_fgram) {
    st.gram_build_ms = m->G_build_ms;
    st.gram_alloc_ms = m->G_alloc_ms;
    st.gram_sums_ms = m->G_sums_ms;
    st.gram_sums_kernel_ms = m->G_sums_kernel_ms;
    st.gram_pack_ms = m->G_pack_ms;
    m->G_build_ms = m->G_alloc_ms = m->G_sums_ms = m->G_sums_kernel_ms = m->G_pack_ms = 0.0;
  }
  st.gram_rows = k.gram_rows;
  st.gram_bytes = k.gram_bytes;
  return st;
}

}  // namespace

slim_csr_t* learn_cd(slimgpu_matrix_t* m, const LearnOptions& opt, const slim_csr_t* imodel,
                     int32_t* status, const int32_t* columns, int32_t ncolumns, bool row_view,
                     ResidentIO* rio) {
  const double t_begin = now_ms();
  auto fail = [&](int32_t code) -> slim_csr_t* {
    if (status) *status = code;
    return nullptr;
  };
  if (!m) {
    set_error("SLIMGPU_Learn: null matrix");
    return fail(SLIM_ERROR_INPUT);
  }
  try {
    const WorkList w = work_list(m, opt, columns, ncolumns);
    const std::vector<int32_t>& requested = w.order;
    const int32_t nwork = (int32_t)requested.size();
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(m->device));
    // One solve at a time per device and process: the tile kernel sizes its grid to the whole
    // chip and its clusters need every member workgroup resident, which two concurrent
    // launches (two host threads calling SLIM_Learn on one GPU) would not guarantee.
    // (recursive: the first item-space solve builds G through a nested call of this function)
    static std::recursive_mutex device_lock[64];
    std::lock_guard<std::recursive_mutex> solve_guard(device_lock[m->device & 63]);

    const slimgpu_model* warm_dev = rio ? rio->warm : nullptr;  // previous model already in HBM
    const bool resident = rio && rio->out;                      // the learned model stays in HBM
    const char* trace_env = std::getenv("SLIM_GPU_TRACE");
    Launch L;
    L.G_block = w.G_block;
    L.p = choose_kernel(m, opt, nwork);
    L.p.trace_level = trace_env ? std::atoi(trace_env) : 0;
    if ((L.p.use_gram || L.p.use_fgram) && !m->G_ready) {
      if (const int32_t st = gram_for_solve(m, opt, L.p.trace_level, L.p.use_fgram); st != SLIM_OK) return fail(st);
    }
    finish_path(m, opt, nwork, imodel, warm_dev, L.p);
    prepare_launch(m, opt, requested, imodel, warm_dev, resident, columns == nullptr, L);
    const double t_prep_done = now_ms();  // (host phases, SLIM_GPU_TRACE: prep | launches + D2H | counters | columns | row view)

    Entries E = run_launches(m, opt, requested, resident, L);
    const double t_kernel_done = now_ms();
    ColumnStats& cs = g_colstats;
    const Counters k = read_counters(m, L, requested, cs);
    const double t_counters_done = now_ms();
    int64_t tnnz = 0;
    for (int32_t c = 0; c < m->ncols; ++c) tnnz += E.cnt[c];
    slim_csr_t* model = nullptr;
    double t_columns_done = t_counters_done;
    if (resident) {
      *rio->out = assemble_resident_model(m, opt, E, tnnz, L, row_view, &t_columns_done).release();
    } else {
      model = assemble_host_model(m->ncols, E, tnnz, row_view);
      t_columns_done = now_ms();
    }
    if (L.p.trace_level >= 1)
      std::fprintf(stderr, "[slim_gpu trace] host phases: prep %.0f ms, launches + D2H %.0f ms (kernel %.0f, D2H of "
                   "%lld entries %.0f), counters %.0f ms, columns %.0f ms, row view %.0f ms\n",
                   t_prep_done - t_begin, t_kernel_done - t_prep_done, E.kernel_ms, (long long)E.total, E.d2h_ms,
                   t_counters_done - t_kernel_done, t_columns_done - t_counters_done, now_ms() - t_columns_done);
    if ((opt.dbglvl & SLIM_DBG_PROGRESS) && model) print_progress(m, model, requested, cs, k);

    slimgpu_stats_t st = solve_stats(m, L, E, k, cs, requested, tnnz);
    st.gather_ms = now_ms() - t_kernel_done;
    if (!opt.build_G) m->last_order = requested;
    st.total_ms = now_ms() - t_begin;
    g_stats = st;
    if (opt.dbglvl & SLIM_DBG_INFO)  // estimate.c:552-555
      std::printf("Done estimation: loss: %.5le, fit: %.5le, ffrac: %.3lf,  #nzs: %zd\n", st.objval,
                  st.error, st.objval != 0 ? st.error / st.objval : 0.0, (ssize_t)tnnz);
    if (status) *status = SLIM_OK;
    return model;
  } catch (const Refusal& r) {
    set_error(r.msg);
    return fail(r.status);
  } catch (const HipFail& e) {
    report(e, "SLIMGPU_Learn");
    return fail(status_of(e));
  } catch (const std::bad_alloc&) {
    set_error("SLIMGPU_Learn: out of host memory");
    return fail(SLIM_ERROR_MEMORY);
  }
}

// -- models resident in HBM (engine.hpp) -----------------------------------------------------
slimgpu_model* learn_resident(slimgpu_matrix_t* m, const LearnOptions& opt, const slimgpu_model* warm,
                              int32_t* status) {
  if (m && !m->replicas.empty()) {
    set_error("SLIMGPU_LearnResident: a model resident in HBM belongs to one device (ngpus = 1)");
    if (status) *status = SLIM_ERROR_INPUT;
    return nullptr;
  }
  slimgpu_model* out = nullptr;
  ResidentIO rio;
  rio.warm = warm;
  rio.out = &out;
  int32_t st = SLIM_ERROR;
  (void)learn_cd(m, opt, nullptr, &st, nullptr, 0, /*row_view=*/true, &rio);
  if (status) *status = st;
  if (st != SLIM_OK && out) {
    model_free(out);
    out = nullptr;
  }
  return out;
}

// A host model made resident (saved models, hand-made test models): its rows go up as they are, the
// column view is formed on the device like a learned model's row view (transpose_on_device: entries of a
// column in ascending row order, the layout SaveModel gives), k_row_facts finds the longest row and
// refuses rows whose ids do not ascend strictly.  W is square with n = max(nrows, ncols); rows the host
// model lacks are empty.  No carried g: as a warm start it is folded like any model without one.
slimgpu_model* model_from_host(slimgpu_matrix_t* m, const slim_csr_t* W, int32_t* status) {
  auto fail = [&](int32_t st, const std::string& why) {
    set_error("SLIMGPU_ModelFromHost: " + why);
    if (status) *status = st;
    return static_cast<slimgpu_model*>(nullptr);
  };
  if (!m || !W || !W->rowptr || W->nrows < 0 || W->ncols < 0)
    return fail(SLIM_ERROR_INPUT, "bad arguments (a staged matrix, a model handle with a row view)");
  if (!m->replicas.empty()) return fail(SLIM_ERROR_INPUT, "a model resident in HBM belongs to one device (ngpus = 1)");
  const int32_t n = std::max(W->nrows, W->ncols);
  const int64_t nnz = W->rowptr[W->nrows];
  if (W->rowptr[0] != 0) return fail(SLIM_ERROR_INPUT, "the row pointer does not start at 0");
  for (int32_t r = 0; r < W->nrows; ++r)
    if (W->rowptr[r + 1] < W->rowptr[r]) return fail(SLIM_ERROR_INPUT, "the row pointer descends");
  if (nnz > 0 && (!W->rowind || !W->rowval)) return fail(SLIM_ERROR_INPUT, "the model has no values");
  for (int64_t j = 0; j < nnz; ++j)
    if (W->rowind[j] < 0 || W->rowind[j] >= n) return fail(SLIM_ERROR_INPUT, "an item id outside the model");
  try {
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t stream = m->stream;
    std::unique_ptr<slimgpu_model> dm(new slimgpu_model());
    dm->device = m->device;
    dm->n = n;
    dm->nnz = nnz;
    std::vector<int64_t> h_ptr((size_t)n + 1, nnz);
    for (int32_t r = 0; r <= W->nrows; ++r) h_ptr[(size_t)r] = W->rowptr[r];
    dm->d_rowptr = DeviceBuffer<int64_t>((size_t)n + 1);
    dm->d_rowind = DeviceBuffer<int32_t>((size_t)std::max<int64_t>(nnz, 1));
    dm->d_rowval = DeviceBuffer<float>((size_t)std::max<int64_t>(nnz, 1));
    HIP_TRY(hipMemcpyAsync(dm->d_rowptr.get(), h_ptr.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice,
                           stream));
    if (nnz > 0) {
      HIP_TRY(hipMemcpyAsync(dm->d_rowind.get(), W->rowind, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, stream));
      HIP_TRY(hipMemcpyAsync(dm->d_rowval.get(), W->rowval, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, stream));
    }
    int32_t* d_facts = m->ws_misc.reserve(16);
    int32_t facts[2] = {0, 0};
    HIP_TRY(hipMemsetAsync(d_facts, 0, sizeof(facts), stream));
    queue_row_facts(stream, m->num_cus, n, dm->d_rowptr.get(), dm->d_rowind.get(), d_facts);
    HIP_TRY(hipMemcpyAsync(facts, d_facts, sizeof(facts), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (facts[1] != 0) return fail(SLIM_ERROR_INPUT, "the item ids of a model row do not ascend strictly");
    dm->max_row = facts[0];
    dm->rows_sorted = true;
    transpose_on_device(m, n, nnz, dm->d_rowptr.get(), dm->d_rowind.get(), dm->d_rowval.get(), dm->d_colptr,
                        dm->d_colind, dm->d_colval);
    HIP_TRY(hipStreamSynchronize(stream));
    if (status) *status = SLIM_OK;
    return dm.release();
  } catch (const HipFail& e) {
    report(e, "SLIMGPU_ModelFromHost");
    if (status) *status = status_of(e);
    return nullptr;
  } catch (const std::bad_alloc&) {
    return fail(SLIM_ERROR_MEMORY, "out of host memory");
  }
}

int32_t model_row_view(const slimgpu_model* w, DeviceRowView* out) {
  if (!w || !w->d_rowptr.get() || !out) {
    set_error("resident model: no row view");
    return SLIM_ERROR_INPUT;
  }
  out->nrows = out->ncols = w->n;
  out->nnz = w->nnz;
  out->max_row = w->max_row;  // recorded when the row view was built: nothing is copied here
  out->rows_sorted = w->rows_sorted;
  out->device = w->device;
  out->d_ptr = w->d_rowptr.get();
  out->d_ind = w->d_rowind.get();
  out->d_val = w->d_rowval.get();
  return SLIM_OK;
}

int32_t matrix_csr_view(const slimgpu_matrix_t* m, DeviceCsrView* out) {
  if (!m || !m->d_rowptr || !out) {
    set_error("staged matrix: no CSR on the device");
    return SLIM_ERROR_INPUT;
  }
  out->device = m->device;
  out->stream = m->stream;
  out->num_cus = m->num_cus;
  out->nrows = m->nrows;
  out->ncols = m->ncols;
  out->nnz = m->nnz;
  out->merged = m->merged;
  out->d_ptr = m->d_rowptr;
  out->d_ind = m->d_rowind;
  out->d_val = m->binary ? nullptr : m->d_rowval;
  return SLIM_OK;
}

int64_t model_nnz(const slimgpu_model* w) { return w ? w->nnz : -1; }
int32_t model_ncols(const slimgpu_model* w) { return w ? w->n : -1; }

namespace {
// D2H of both views into arrays the host model owns (csr_free releases them)
void fetch_now(slimgpu_model* w) {
  const double t0 = now_ms();
  ssize_t *cp = nullptr, *rp = nullptr;
  int32_t *ci = nullptr, *ri = nullptr;
  float *cv = nullptr, *rv = nullptr;
  hipStream_t cs = nullptr;
  try {
    HIP_TRY(hipSetDevice(w->device));
    static_assert(sizeof(ssize_t) == sizeof(int64_t), "offsets travel as they are");
    const size_t n1 = (size_t)w->n + 1, nz = (size_t)std::max<int64_t>(w->nnz, 1);
    cp = static_cast<ssize_t*>(std::malloc(sizeof(ssize_t) * n1));
    rp = static_cast<ssize_t*>(std::malloc(sizeof(ssize_t) * n1));
    ci = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * nz));
    ri = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * nz));
    cv = static_cast<float*>(std::malloc(sizeof(float) * nz));
    rv = static_cast<float*>(std::malloc(sizeof(float) * nz));
    if (!cp || !rp || !ci || !ri || !cv || !rv) throw std::bad_alloc();
    // its own stream: the copies run on the DMA engines beside whatever the solver's stream is doing
    HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    HIP_TRY(hipMemcpyAsync(cp, w->d_colptr.get(), sizeof(int64_t) * n1, hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipMemcpyAsync(rp, w->d_rowptr.get(), sizeof(int64_t) * n1, hipMemcpyDeviceToHost, cs));
    if (w->nnz > 0) {
      HIP_TRY(hipMemcpyAsync(ci, w->d_colind.get(), sizeof(int32_t) * (size_t)w->nnz, hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipMemcpyAsync(cv, w->d_colval.get(), sizeof(float) * (size_t)w->nnz, hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipMemcpyAsync(ri, w->d_rowind.get(), sizeof(int32_t) * (size_t)w->nnz, hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipMemcpyAsync(rv, w->d_rowval.get(), sizeof(float) * (size_t)w->nnz, hipMemcpyDeviceToHost, cs));
    }
    HIP_TRY(hipStreamSynchronize(cs));
    (void)hipStreamDestroy(cs);
    cs = nullptr;
    slim_csr_t* hm = model_from_columns(w->n, cp, ci, cv, /*row_view=*/false);
    if (!hm) throw std::bad_alloc();
    hm->rowptr = rp;
    hm->rowind = ri;
    hm->rowval = rv;
    w->fetched = hm;
    w->fetch_status = SLIM_OK;
  } catch (const HipFail& e) {
    w->fetch_error = "SLIMGPU_ModelFetch: " + e.where + ": " + hipGetErrorString(e.code);
    w->fetch_status = SLIM_ERROR;
  } catch (const std::bad_alloc&) {
    w->fetch_error = "SLIMGPU_ModelFetch: out of host memory";
    w->fetch_status = SLIM_ERROR_MEMORY;
  }
  if (w->fetch_status != SLIM_OK) {
    if (cs) (void)hipStreamDestroy(cs);
    std::free(cp); std::free(rp); std::free(ci); std::free(ri); std::free(cv); std::free(rv);
  }
  w->fetch_ms = now_ms() - t0;
}
}  // namespace

int32_t model_fetch_begin(slimgpu_model* w) {
  if (!w || !w->d_rowptr.get()) {
    set_error("SLIMGPU_ModelFetchBegin: null model");
    return SLIM_ERROR_INPUT;
  }
  if (w->fetch_begun) return SLIM_OK;
  w->fetch_begun = true;
  w->fetched = nullptr;
  w->fetch_status = SLIM_OK;
  try {
    w->fetcher = std::thread(fetch_now, w);
  } catch (const std::system_error&) {  // no thread: the fetch happens in model_fetch
    w->fetch_begun = false;
  }
  return SLIM_OK;
}

slim_csr_t* model_fetch(slimgpu_model* w, int32_t* status, double* ms) {
  if (!w || !w->d_rowptr.get()) {
    set_error("SLIMGPU_ModelFetch: null model");
    if (status) *status = SLIM_ERROR_INPUT;
    return nullptr;
  }
  if (w->fetch_begun) {
    if (w->fetcher.joinable()) w->fetcher.join();
    w->fetch_begun = false;
  } else {
    fetch_now(w);
  }
  slim_csr_t* hm = w->fetched;  // the caller's from here on (SLIM_FreeModel); a later fetch copies again
  w->fetched = nullptr;
  if (w->fetch_status != SLIM_OK) set_error(w->fetch_error);
  if (status) *status = w->fetch_status;
  if (ms) *ms = w->fetch_ms;
  return hm;
}

void model_free(slimgpu_model* w) {
  if (!w) return;
  if (w->fetcher.joinable()) w->fetcher.join();
  if (w->fetched) csr_free(w->fetched);
  delete w;  // (~slimgpu_model frees the device arrays)
}

// -- G = R^T R in row blocks (engine.hpp) ---------------------------------------------------
int32_t gram_build_rows(slimgpu_matrix_t* m, int32_t row_begin, int32_t row_end) {
  if (!m || row_begin < 0 || row_end > m->ncols || row_begin > row_end) {
    set_error("SLIMGPU_MatrixGramBuildRows: rows outside [0, ncols)");
    return SLIM_ERROR_INPUT;
  }
  try {
    HIP_TRY(hipSetDevice(m->device));
    const size_t G_bytes = sizeof(float) * (size_t)m->ncols * (size_t)gram_ld(m->ncols);
    const bool fresh = m->G_ready || m->ws_G.bytes() < G_bytes;  // a fresh G: nothing of an earlier one is kept
    if (fresh) {
      size_t free_b = 0, total_b = 0;
      HIP_TRY(hipMemGetInfo(&free_b, &total_b));
      if (G_bytes + (size_t(8) << 30) > free_b + m->ws_G.bytes() + m->ws_gram.bytes()) {
        set_error("SLIMGPU_MatrixGramBuildRows: G = R^T R (4 ncols^2 bytes) does not fit the free HBM");
        return SLIM_ERROR_MEMORY;
      }
      m->G_ready = false;
      m->Gp_ready = false;
      m->Gp_tried = false;
    }
    LearnOptions bo;
    bo.G_rows_begin = row_begin;
    bo.G_rows_end = row_end;
    return build_gram(m, bo, fresh);
  } catch (const HipFail& e) {
    report(e, "SLIMGPU_MatrixGramBuildRows");
    return status_of(e);
  }
}

int32_t gram_view(slimgpu_matrix_t* m, void** dptr, int64_t* ld, int32_t* nrows) {
  if (!m || !m->ws_G.get() || m->G_ld <= 0) {
    set_error("SLIMGPU_MatrixGramView: no G on this handle (SLIMGPU_MatrixGramBuildRows first)");
    return SLIM_ERROR_INPUT;
  }
  if (dptr) *dptr = m->ws_G.get();
  if (ld) *ld = m->G_ld;
  if (nrows) *nrows = m->ncols;
  return SLIM_OK;
}

int32_t gram_commit(slimgpu_matrix_t* m) {
  if (!m || !m->ws_G.get() || m->G_ld <= 0) {
    set_error("SLIMGPU_MatrixGramCommit: no G on this handle");
    return SLIM_ERROR_INPUT;
  }
  try {
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream));
    m->G_ready = true;
    m->Gp_ready = false;
    m->Gp_tried = false;
    m->Gf_dropped = false;
    (void)pack_gram(m);  // (false: G is not integer-valued or the planes do not fit -- float kernels)
    drop_float_gram(m);
    return SLIM_OK;
  } catch (const HipFail& e) {
    report(e, "SLIMGPU_MatrixGramCommit");
    return status_of(e);
  }
}

int32_t gram_planes(slimgpu_matrix_t* m, slimgpu_gram_planes_t* out) {
  if (!m || !out || !m->Gp_ready) {
    set_error("SLIMGPU_MatrixGramPlanes: no byte planes on this handle (no G committed, or a G that could not be packed)");
    return SLIM_ERROR_INPUT;
  }
  out->ncols = m->ncols;
  out->nchunks = m->Gp_nchunks;
  out->ldb = m->Gp_ldb;
  out->hi_bytes = m->Gp_pool_bytes;
  out->lo = m->ws_Glo.get();
  out->base = m->ws_Gbase.get();
  out->hi = m->ws_Ghi.get();
  out->hi_off = m->ws_hioff.get();
  out->hi_k = m->ws_hik.get();
  out->hi2_k = m->ws_hi2k.get();
  out->diag = m->ws_Gdiag.get();
  out->meta = reinterpret_cast<const uint32_t*>(m->ws_Gmeta.get());
  out->rank_of = m->ws_rankof.get();
  out->item_of = m->ws_itemof.get();
  return SLIM_OK;
}

}  // namespace slimamd
