// engine.hpp -- device side of libslim.so: the training matrix staged in HBM and
// the driver that runs the CD kernels over a set of item columns.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/slim_gpu.h"

namespace slimamd {

struct EvalResult;  // host_csr.hpp

// Decoded SLIM_Learn options (reference src/libslim/api.c:42-52 + slim_gpu.h).
struct LearnOptions {
  int32_t nthreads = 1, nnbrs = 0, simtype = 0, dbglvl = 0, algo = SLIM_ALGO_CD;
  int32_t ordered = 0, maxniters = 10000;
  double l1r = 1.0, l2r = 1.0, optTol = 1e-7;
  int32_t col_begin = 0, col_end = -1;  // -1: ncols
  uint32_t seed = 1;
  int32_t device = -1;  // -1: current
  int32_t kernel = SLIMGPU_KERNEL_AUTO;
  int32_t cluster = 0;  // tile-cluster size (0 = auto)
  int32_t heavy_tiles = -1;   // tiles solved by big clusters first (-1 = auto, 0 = none)
  int32_t heavy_cluster = 0;  // size of those clusters (0 = auto)
  int32_t ngpus = 1;          // SLIM_Learn & co: devices to shard over (multi_gpu.cpp)
  int32_t shard_count = 1, shard_index = 0;  // one shard of the cost-ordered work list
  bool build_G = false;  // internal: this call fills G = R^T R (engine.hip), it solves nothing
  int32_t G_rows_begin = 0, G_rows_end = -1;  // internal, with build_G: only rows [begin, end) of G (-1: all)
};
LearnOptions decode_options(const int32_t* ioptions, const double* doptions);

struct ColumnStats {
  std::vector<int32_t> nacols, sweeps, conv;
  std::vector<int64_t> G, D, U;
};

// Per-thread record of the most recent solve (SLIMGPU_LastStats & co).
slimgpu_stats_t& last_stats();
ColumnStats& last_column_stats();

// Implemented in engine.hip
slimgpu_matrix_t* matrix_from_host(int32_t nrows, const ssize_t* rowptr,
                                   const int32_t* rowind, const float* rowval,
                                   const LearnOptions& opt, int32_t* status);
slimgpu_matrix_t* matrix_from_device(int32_t nrows, int32_t ncols,
                                     const int64_t* d_rowptr, const int32_t* d_rowind,
                                     const float* d_rowval, const LearnOptions& opt,
                                     int32_t* status);
void matrix_free(slimgpu_matrix_t* m);
// copy of a staged matrix (all views, no re-sort) on another device, device to device
slimgpu_matrix_t* matrix_clone_to_device(const slimgpu_matrix_t* src, int32_t device,
                                         int32_t* status);
int32_t matrix_info(const slimgpu_matrix_t* m, int32_t* nrows, int32_t* ncols, int64_t* nnz);
int32_t matrix_get_column_view(const slimgpu_matrix_t* m, int64_t* colptr, int32_t* colind,
                               float* colval, float* cnorms);
double matrix_setup_ms(const slimgpu_matrix_t* m);
int32_t matrix_column_cost(const slimgpu_matrix_t* m, int64_t* cost);
// the caller is about to solve this matrix n times (a model-selection grid): lets the engine pay
// for G = R^T R up front (item-space CD, cd_gram.hpp)
void matrix_expect_solves(slimgpu_matrix_t* m, int32_t n);
// G = R^T R in pieces (multi-GPU: every rank forms the rows of a block of items, the blocks are
// exchanged by the caller, e.g. an RCCL broadcast per block into the view below, then committed):
// gram_build_rows fills rows [row_begin, row_end) of the handle's G (all of its ncols entries each),
// gram_view gives the device buffer (floats, ld per row), gram_commit declares every row present and
// forms the byte planes.  SLIM_OK or an error code (set_error).
int32_t gram_build_rows(slimgpu_matrix_t* m, int32_t row_begin, int32_t row_end);
int32_t gram_view(slimgpu_matrix_t* m, void** dptr, int64_t* ld, int32_t* nrows);
int32_t gram_commit(slimgpu_matrix_t* m);
// the byte planes the handle holds (slim_gpu_planes.h); SLIM_ERROR_INPUT when it holds none
int32_t gram_planes(slimgpu_matrix_t* m, slimgpu_gram_planes_t* out);

// EstimateModelCD + SaveModel on the device matrix.  Returns a host model
// (slim_csr_t with both views) or nullptr with *status set.
// columns/ncolumns (optional): solve exactly these item columns (distinct ids) instead of
// the range [opt.col_begin, opt.col_end); every other column of the model comes back empty.
// rio (optional): warm start from / result into a model resident in HBM (below); with rio->out set
// the host model is not formed and nullptr comes back with *status = SLIM_OK.
struct ResidentIO {
  const slimgpu_model* warm = nullptr;
  slimgpu_model** out = nullptr;
};
slim_csr_t* learn_cd(slimgpu_matrix_t* m, const LearnOptions& opt, const slim_csr_t* imodel,
                     int32_t* status, const int32_t* columns = nullptr, int32_t ncolumns = 0,
                     bool row_view = true, ResidentIO* rio = nullptr);

// Models resident in HBM (model-selection grids: slim_mselect.c:94-113 learns 45 models one from the
// other and needs each on the host only to print its nnz): the solve leaves both views of W on the
// device, the next solve warm-starts from them without an upload, and a fetch to the host (both views,
// the arrays SaveModel would have formed) can run on the DMA engines beside the next solve.
slimgpu_model* learn_resident(slimgpu_matrix_t* m, const LearnOptions& opt, const slimgpu_model* warm,
                              int32_t* status);
// a host model made resident on m's device (slim_gpu_rank.h: SLIMGPU_ModelFromHost)
slimgpu_model* model_from_host(slimgpu_matrix_t* m, const slim_csr_t* W, int32_t* status);
int64_t model_nnz(const slimgpu_model* w);
int32_t model_ncols(const slimgpu_model* w);
int32_t model_fetch_begin(slimgpu_model* w);                      // starts the D2H on a host thread + copy stream
slim_csr_t* model_fetch(slimgpu_model* w, int32_t* status, double* ms = nullptr);  // joins it (or copies now)
void model_free(slimgpu_model* w);

// Replicas: copies of a staged matrix on other devices, owned by (and freed with) the
// primary handle; matrix_adopt_csr hands the borrowed device CSR of a FromDevice matrix over
// to the handle.
void matrix_add_replica(slimgpu_matrix_t* m, slimgpu_matrix_t* replica);
const std::vector<slimgpu_matrix_t*>& matrix_replicas(const slimgpu_matrix_t* m);
void matrix_adopt_csr(slimgpu_matrix_t* m);
int32_t matrix_device(const slimgpu_matrix_t* m);
void matrix_set_setup_ms(slimgpu_matrix_t* m, double ms);

// multi_gpu.cpp: the training matrix replicated on opt.ngpus GPUs of the node (the returned
// handle is the copy on the first device and owns the others) and a solve sharded over all
// copies of a handle, one host thread + stream per device.  With one device these are
// matrix_from_host / learn_cd.
slimgpu_matrix_t* multi_from_host(int32_t nrows, const ssize_t* rowptr, const int32_t* rowind,
                                  const float* rowval, const LearnOptions& opt, int32_t* status);
slim_csr_t* multi_learn(slimgpu_matrix_t* m, const LearnOptions& opt, const slim_csr_t* imodel,
                        int32_t* status, const int32_t* columns = nullptr, int32_t ncolumns = 0);

int32_t device_count();

// topn.hip: top-N lists of every row of `hist` through model W, on the GPU, bit-identical
// to host_csr.cpp::top_n.  counts (optional): list length per user.
int32_t predict_device(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds,
                       int32_t* output, float* scores, int32_t* counts);
// the same with the row view of W already on the device (a resident model: model_row_view)
struct DeviceRowView {
  int32_t nrows = 0, ncols = 0;
  int64_t nnz = 0, max_row = 0;  // max_row: entries of the longest row
  bool rows_sorted = false;      // ids known to ascend inside every row (a resident model records it)
  int32_t device = -1;           // where the arrays live (-1: the current device)
  const int64_t* d_ptr = nullptr;
  const int32_t* d_ind = nullptr;
  const float* d_val = nullptr;
};
int32_t predict_device_view(const DeviceRowView& W, const slim_csr_t* hist, int32_t nrcmds,
                            int32_t* output, float* scores, int32_t* counts);
// slim_gpu_lists.h: lists of up to SLIMGPU_MAX_LIST (up to 128 on the paths of the calls above, beyond on the
// chunk kernel's long-list form); SLIM_ERROR_INPUT with the outputs untouched where nothing on the device serves
// filter (slim_gpu_filter.h; nullptr: none) narrows the candidates; one made for another ncols is refused
int32_t predict_lists(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds,
                      int32_t* output, float* scores, int32_t* counts, slimgpu_filter* filter = nullptr);
int32_t predict_lists_view(const DeviceRowView& W, const slim_csr_t* hist, int32_t nrcmds,
                           int32_t* output, float* scores, int32_t* counts, slimgpu_filter* filter = nullptr);
// filter.hip: the filter object -- validated once, its host description (host_csr.hpp: HostFilter) and the
// device copy that filter_on_device (scorer.hpp) makes on first use
struct HostFilter;
slimgpu_filter* filter_create(int32_t ncols, int32_t nitems, const int32_t* items, int32_t blocked, int32_t xusers,
                              const int64_t* xptr, const int32_t* xind, int32_t* status);
void filter_free(slimgpu_filter* f);
HostFilter filter_host(const slimgpu_filter* f);
// SLIM_OK, or SLIM_ERROR_INPUT with "<who>: ..." as the error text when f was made for another number of items
int32_t filter_check(const char* who, const slimgpu_filter* f, int32_t model_ncols);
// candidates.hip: the candidate set object (slim_gpu_cand.h) -- validated once, its host description (host_csr.hpp:
// HostCandSet) and the device copy that candset_on_device (scorer.hpp) makes on first use -- and the calls that score
// its rows on a device: host model and host histories (every row of trn), or a resident model and rows of the staged
// matrix.  slot_scores may be null; nrcmds == 0: no lists.  SLIM_ERROR_INPUT with the outputs untouched where the
// set does not fit the call or the chunk scorer cannot serve.
struct HostCandSet;
slimgpu_candset* candset_create(int32_t ncols, int32_t nusers, const int64_t* cptr, const int32_t* cind,
                                int32_t* status);
void candset_free(slimgpu_candset* cs);
HostCandSet candset_host(const slimgpu_candset* cs);
// what every call checks of its set before anything is written: the model's width, a row for every selected user
// (users: ascending, nullptr: users [0, nsel)), the list arguments, and for lists rows of at most SLIMGPU_MAX_LIST
int32_t candset_check(const char* who, const slimgpu_candset* cs, int32_t model_ncols, int32_t nsel,
                      const int32_t* users, int32_t nrcmds, const int32_t* output, const float* scores);
// slim_gpu_sample.h: the ids of a set born on the device brought to its host copy (no-op for any other set, and
// from the second call on; throws HipFail / std::bad_alloc); the rows copied out; the sizes
void candset_need_ids(slimgpu_candset* cs);
int32_t candset_fetch_ids(const char* who, slimgpu_candset* cs);  // the same as a status, the failure as the error text
int32_t candset_rows(slimgpu_candset* cs, int64_t* cptr, int32_t* cind);
int32_t candset_info(const slimgpu_candset* cs, int32_t* nrows, int32_t* ncols, int64_t* entries);
// cand_sample.hip: the sampled set of an eval set's users, made on the device; host_csr.cpp has the host form
slimgpu_candset* evalset_sample_candidates(slimgpu_evalset_t* es, int32_t nnegs, uint64_t seed, int32_t* status);
// ... under the weighted rule: weights[ncols] (nullptr: the popularity of the resident matrix's columns)
slimgpu_candset* evalset_sample_candidates_weighted(slimgpu_evalset_t* es, int32_t nnegs, uint64_t seed,
                                                    const uint32_t* weights, int32_t* status);
double last_weighted_sample_kernel_ms();  // the weighted kernel of this thread's most recent such call
int32_t score_candidates(const slim_csr_t* W, const slim_csr_t* trn, slimgpu_candset* cs, int32_t nrcmds,
                         float* slot_scores, int32_t* output, float* scores, int32_t* counts);
int32_t matrix_score_candidates(const slimgpu_model* model, slimgpu_matrix_t* mat, slimgpu_candset* cs, int32_t nusers,
                                const int32_t* users, int32_t nrcmds, float* slot_scores, int32_t* output,
                                float* scores, int32_t* counts);
// explain.hip (slim_gpu_explain.h): the terms behind the slot scores; why_items / why_terms (both or neither) and
// support may be null.  SLIM_ERROR_INPUT / SLIM_ERROR_MEMORY with every output untouched.
int32_t explain_check(const char* who, int32_t nwhy, const int32_t* why_items, const float* why_terms);
int32_t explain_candidates(const slim_csr_t* W, const slim_csr_t* trn, slimgpu_candset* cs, int32_t nwhy,
                           int32_t* why_items, float* why_terms, int32_t* support);
int32_t matrix_explain_candidates(const slimgpu_model* model, slimgpu_matrix_t* mat, slimgpu_candset* cs,
                                  int32_t nusers, const int32_t* users, int32_t nwhy, int32_t* why_items,
                                  float* why_terms, int32_t* support);
slimgpu_list_stats_t& last_list_stats();
int32_t model_row_view(const slimgpu_model* w, DeviceRowView* out);
// the CSR of a staged matrix where it lies (the history of the resident scorer)
struct DeviceCsrView {
  int32_t device = -1, num_cus = 256;
  void* stream = nullptr;  // hipStream_t of the handle
  int32_t nrows = 0, ncols = 0;
  int64_t nnz = 0;
  bool merged = false;     // SLIM_GPU_DUPLICATES=sum changed the rows: they are not the caller's
  const int64_t* d_ptr = nullptr;
  const int32_t* d_ind = nullptr;
  const float* d_val = nullptr;  // nullptr: binary
};
int32_t matrix_csr_view(const slimgpu_matrix_t* m, DeviceCsrView* out);

// resident_eval.hip: a resident model scored and evaluated against the resident matrix (slim_gpu_eval.h:
// SLIMGPU_EvalSetCreateAt & co).  Per evaluation only the four sums and three counts of every list length
// come down.  cutoffs[ncutoffs]: list lengths, ascending; users[nusers]: the evaluated users, ascending
// (nullptr and 0: every user).  model_evaluate fills out[0 .. ncutoffs), which must be the eval set's count.
slimgpu_evalset_t* evalset_create(slimgpu_matrix_t* mat, const slim_csr_t* tst, const int32_t* fmarker,
                                  int32_t fm_ncols, int32_t ncutoffs, const int32_t* cutoffs, int32_t nusers,
                                  const int32_t* users, int32_t* status);
// slim_gpu_rank.h: an eval set with no list length; the rank (and score) of every test entry of its users
// among the user's candidates; HR / ARHR at any cutoffs (out[0 .. ncutoffs)) from those ranks
slimgpu_evalset_t* evalset_create_ranked(slimgpu_matrix_t* mat, const slim_csr_t* tst, const int32_t* fmarker,
                                         int32_t fm_ncols, int32_t nusers, const int32_t* users, int32_t* status);
int64_t evalset_entries(const slimgpu_evalset_t* es);
// filter (slim_gpu_filter.h; nullptr: none) narrows the candidates of the three calls below: a test entry it
// removes stays in every denominator, is a miss at every cutoff and has rank 0 and score 0; a filter made for
// another ncols than the model's is refused before anything is queued
int32_t model_ranks(slimgpu_evalset_t* es, const slimgpu_model* model, int32_t* ranks, float* scores,
                    slimgpu_filter* filter = nullptr);
int32_t model_evaluate_ranked(slimgpu_evalset_t* es, const slimgpu_model* model, int32_t ncutoffs,
                              const int32_t* cutoffs, EvalResult* out, slimgpu_filter* filter = nullptr);
double last_rank_prepass_ms();
void evalset_free(slimgpu_evalset_t* es);
int32_t evalset_cutoffs(const slimgpu_evalset_t* es);
int32_t model_evaluate(slimgpu_evalset_t* es, const slimgpu_model* model, int32_t ncutoffs, EvalResult* out,
                       slimgpu_filter* filter = nullptr);
// slim_gpu_groups.h: while groups are set, every evaluation of the eval set also forms the rows of its groups from
// the records it sums anyway; evalset_group_figures hands out the last evaluation's, out[(ngroups + 1) * ncutoffs]
// with everybody's rows last.  evalset_groups: the number of groups, 0 without.
int32_t evalset_set_groups(slimgpu_evalset_t* es, int32_t ngroups, const int32_t* group_of_user);
int32_t evalset_set_history_bands(slimgpu_evalset_t* es, int32_t nbounds, const int32_t* bounds);
void evalset_clear_groups(slimgpu_evalset_t* es);
int32_t evalset_group_info(const slimgpu_evalset_t* es, int32_t* ngroups, int32_t* members);
int32_t evalset_groups(const slimgpu_evalset_t* es);
int32_t evalset_group_figures(const slimgpu_evalset_t* es, int32_t ncutoffs, EvalResult* out);
// slim_gpu_cand.h: the figures of the candidate lists (score descending, then slot) of the eval set's users at its
// cutoffs; a set of another ncols, with too few rows or with a selected row above SLIMGPU_MAX_LIST is refused
int32_t model_evaluate_candidates(slimgpu_evalset_t* es, const slimgpu_model* model, slimgpu_candset* cs,
                                  int32_t ncutoffs, EvalResult* out);
int32_t matrix_predict(int32_t nrcmds, const slimgpu_model* model, slimgpu_matrix_t* mat, int32_t* output,
                       float* scores);
// users[nusers]: the rows scored, ascending (nullptr and 0: every row); counts may be null
int32_t matrix_predict_lists(int32_t nrcmds, const slimgpu_model* model, slimgpu_matrix_t* mat, int32_t nusers,
                             const int32_t* users, int32_t* output, float* scores, int32_t* counts,
                             slimgpu_filter* filter = nullptr);
// slim_gpu_exposure.h: per-item counts of the places of top-N lists at ncutoffs cutoffs, counted on the device
// (exposure.hip), and their summaries; exposure ([ncutoffs][ncols]) and summary ([ncutoffs]) may be null.  A
// caller's lists uploaded (exposure.hip); the lists of matrix_predict_lists and of model_evaluate counted where
// they are made (resident_eval.hip).  SLIM_ERROR_INPUT with nothing queued or written.
int32_t matrix_list_exposure(slimgpu_matrix_t* mat, const int32_t* fmarker, int32_t fm_ncols, int64_t nlists,
                             int32_t nrcmds, const int32_t* ids, const int32_t* counts, int32_t ncutoffs,
                             const int32_t* cutoffs, uint32_t* exposure, slimgpu_exposure_t* summary);
int32_t matrix_predict_exposure(slimgpu_matrix_t* mat, const slimgpu_model* model, int32_t nrcmds, int32_t nusers,
                                const int32_t* users, slimgpu_filter* filter, const int32_t* fmarker, int32_t fm_ncols,
                                int32_t ncutoffs, const int32_t* cutoffs, uint32_t* exposure,
                                slimgpu_exposure_t* summary);
int32_t model_evaluate_exposure(slimgpu_evalset_t* es, const slimgpu_model* model, slimgpu_filter* filter,
                                int32_t ncutoffs, EvalResult* out, uint32_t* exposure, slimgpu_exposure_t* summary);
slimgpu_eval_stats_t& last_eval_stats();
// split.hip (slim_gpu_split.h): the train half staged on the source's device (the new handle owns its arrays), the
// test half as a host matrix (csr_free releases it).  SLIM_ERROR_INPUT with the outputs untouched on a refusal.
int32_t matrix_split(slimgpu_matrix_t* src, const slimgpu_split_t* split, slimgpu_matrix_t** trn, slim_csr_t** tst);
// facts of a row view, for the scorers: d_facts[0] = entries of its longest row, d_facts[1] = 1 when the
// ids of some row do not ascend strictly (both preset to 0 by the caller).  Queues one kernel on
// `stream` (a hipStream_t); throws HipFail when the launch fails.
void queue_row_facts(void* stream, int num_cus, int32_t nrows, const int64_t* d_ptr, const int32_t* d_ind,
                     int32_t* d_facts);
// the row-order check of a host model once it is staged (the scorers of topn.hip and the 1-vs-k scorer of
// eval.hip): whether the ids of every row ascend strictly.  One kernel on the null stream and four bytes
// down; throws HipFail.
bool rows_ascend_strictly(int num_cus, int32_t nrows, const int64_t* d_ptr, const int32_t* d_ind);

// admm.hip: SLIM_Learn(algo = admm), the reference's dense ADMM solver (estimate.c:38-304) with
// rocBLAS for the panel solves, updates and products and HIP kernels for the rest.
slim_csr_t* learn_admm(int32_t nrows, const ssize_t* rowptr, const int32_t* rowind,
                       const float* rowval, const LearnOptions& opt, int32_t* status);

// eval.hip: HR / ARHR of top-N lists against a test matrix on the GPU (the host loop's figures,
// bit for bit), and the 1-vs-k protocol (every user ranks its own nnegs candidates).
int32_t evaluate_device(int32_t nusers, int32_t nrcmds, const int32_t* lists, const int32_t* counts,
                        const slim_csr_t* tst, const int32_t* fmarker, int32_t fm_ncols,
                        EvalResult* out);
int32_t predict_1vsk_device(const slim_csr_t* W, const slim_csr_t* hist, int32_t nrcmds,
                            int32_t nnegs, const int32_t* negitems, int32_t* output,
                            float* scores);

}  // namespace slimamd
