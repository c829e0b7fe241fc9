// grid_eval.hpp -- the evaluator of a model-selection grid (include/slim_gpu_grid.h): the one owner of what a grid
// holds between its pairs, and the one place that decides how a pair is learnt and evaluated.  Py_SLIM_Mselect*
// (slim_abi.cpp) and slim_mselect (through SLIMGPU_Grid*) are loops over it.
#pragma once
#include <string>
#include <vector>

#include "../../include/slim_gpu_grid.h"
#include "engine.hpp"
#include "host_csr.hpp"

namespace slimamd {
int predict_policy();  // SLIM_PREDICT (slim_abi.cpp)
}

// Whether a grid with these options keeps its models in HBM and evaluates them there (cd, one GPU, SLIM_GPU_RESIDENT
// and SLIM_GPU_EVAL_RESIDENT not 0): the grids that SLIMGPU_GridOpenOn can serve.  Py_SLIM_MselectCV picks its route
// by it.
bool grid_can_open_on(const int32_t* ioptions, const double* doptions);

struct slimgpu_grid {
  // the request, decoded once by open()
  const slim_csr_t* trn = nullptr;  // (borrowed, as is the filter; none for a grid opened on a staged matrix)
  const slim_csr_t* tst = nullptr;
  slimgpu_filter_t* filter = nullptr;
  slimamd::LearnOptions base;
  bool admm = false, keep_on_host = false, eval_on_host = false;  // (SLIM_GPU_RESIDENT=0, SLIM_GPU_EVAL_RESIDENT=0)
  int32_t nrcmds = 10, stride = 1, evalnegs = 0, evalnegpop = 0, evalexpo = 0;
  uint64_t evalseed = 1;
  int32_t nall = 0;          // the users an evaluation of everybody covers
  std::vector<int32_t> sel;  // stride > 1: the evaluated users
  int32_t ngroups = 0, select_group = -1;  // slim_gpu_groups.h (0: no groups); the group the caller's loop selects on
  bool group_rows_stand = false;           // the eval set's group rows are those of the last solved pair
  // what the grid holds between its pairs; the destructor is the only place it is freed
  slimgpu_matrix_t* mat = nullptr;  // (none for ADMM)
  int32_t ncols = 0;                // the marker's width
  int32_t* fmarker = nullptr;
  slimgpu_evalset_t* evalset = nullptr;
  bool ranked = false, resident = false;
  slimgpu_candset* cands = nullptr;
  slimgpu_model* dmodel = nullptr;      // the last pair's model where the models stay in HBM ...
  slim_csr_t* model = nullptr;  // ... and on the host: the model itself, or its copy once asked for

  slimgpu_grid(const slim_csr_t* trn_, const slim_csr_t* tst_, slimgpu_filter_t* filter_)
      : trn(trn_), tst(tst_), filter(filter_) {}
  slimgpu_grid(const slimgpu_grid&) = delete;
  slimgpu_grid& operator=(const slimgpu_grid&) = delete;
  ~slimgpu_grid();

  // the plan: everything is decided, staged and sampled here, before the first solve.  SLIM_OK, or the status of
  // the refusal with its reason as the error text
  int32_t open(const int32_t* ioptions, const double* doptions, int32_t marker_ncols, int32_t nsolves);
  // SLIMGPU_GridOpenOn: the same plan over a matrix that is staged already (trn == nullptr).  The grid owns `staged`
  // once this returns SLIM_OK; on a refusal it stays the caller's
  int32_t open_on(slimgpu_matrix_t* staged, const int32_t* ioptions, const double* doptions, int32_t marker_ncols,
                  int32_t nsolves);
  void describe() const;
  // slim_gpu_groups.h, between open() and the first solve: the eval set forms the group rows of every pair
  int32_t set_groups(int32_t ngroups_, const int32_t* group_of_user, int32_t select_group_);
  int32_t last_groups(slimamd::EvalResult* rows /* [ngroups + 1] */) const;
  int32_t group_members(int32_t* members /* [ngroups + 1] */) const;
  int32_t solve(double l1r, double l2r, slimgpu_grid_cell_t* cell);
  slim_csr_t* host_model(int32_t* status);

 private:
  int32_t decode(const int32_t* ioptions, const double* doptions);
  int32_t check_needs(bool staged);
  void make_evalset();
  int32_t sample_candidates();
  int32_t learn(const slimamd::LearnOptions& opt);
  int32_t evaluate_in_hbm(slimamd::EvalResult* ev, slimgpu_exposure_t* expo);
  int32_t evaluate_lists(slimamd::EvalResult* ev);
};
