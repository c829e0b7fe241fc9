// grid_eval.cpp -- the evaluator of a model-selection grid (grid_eval.hpp, include/slim_gpu_grid.h).
//
// Host code only.  One R goes to HBM for the whole grid (the reference re-runs CreateTrainingMatrix inside every
// SLIM_Learn call, pyapi.c:295-297).  One GPU, CD: the models stay in HBM (engine.hpp: learn_resident) -- a pair is
// warm-started from the previous one without an upload and evaluated where it lies (resident_eval.hip): the test
// rows and the marker go to HBM once, a pair brings down its four sums and three counts.  Above 128 the figures
// come from the ranks of the held-out items (slim_gpu_rank.h), with no lists formed; such a grid runs resident when
// the ranked eval set can be made and on host models, with lists from the long-list scorer, when it cannot.
#include "grid_eval.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace slimamd;

namespace {

// ---- what the modes need (include/slim_gpu_grid.h has the list in words) -------------------------------------------
using G = slimgpu_grid;
enum : unsigned { kNegs = 1, kExposure = 2, kStride = 4, kFilter = 8, kNamed = kNegs | kExposure | kFilter };

struct Feature {
  unsigned id;
  bool (*asked)(const G&);
  const char* needs;  // how every refusal on its behalf begins
};
const Feature kFeatures[] = {
    {kNegs, [](const G& g) { return g.evalnegs != 0; },
     "Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALNEGS needs the candidate evaluation in HBM (cd on one GPU, no filter, "
     "nrcmds <= 128, SLIM_GPU_RESIDENT and SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs)"},
    {kExposure, [](const G& g) { return g.evalexpo != 0; },
     "Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALEXPOSURE needs the evaluation in HBM and lists of at most 128 (cd on one "
     "GPU, SLIM_GPU_RESIDENT and SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs, no sampled "
     "negatives)"},
    {kStride, [](const G& g) { return g.stride > 1; },
     "Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALSTRIDE needs the evaluation in HBM (cd on one GPU, nrcmds >= 1, "
     "SLIM_GPU_RESIDENT and SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs; above 128 a model "
     "the chunk scorer serves)"},
    {kFilter, [](const G& g) { return g.filter != nullptr; },
     "Py_SLIM_MselectFiltered: a filter needs the evaluation in HBM (cd on one GPU, SLIM_GPU_RESIDENT and "
     "SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs, a filter of the models' width)"},
};
// the order in which they are judged (places in kFeatures): before anything is staged, and once the eval set is known
const int kOrderBefore[] = {0, 1, 2, 3}, kOrderStaged[] = {2, 1, 3, 0};

bool several_gpus(const G& g) { return g.base.ngpus > 1; }
bool no_evalset(const G& g) { return !g.evalset; }
bool no_list_length(const G& g) { return g.nrcmds < 1 || g.nrcmds > 128; }
int32_t staged_ncols(const G& g) {
  int32_t nrows = 0, ncols = 0;
  int64_t nnz = 0;
  if (g.mat) matrix_info(g.mat, &nrows, &ncols, &nnz);
  return ncols;
}
std::string nrcmds_is(const G& g) { return "nrcmds is " + std::to_string(g.nrcmds); }
const char kSeveral[] = "the grid runs on several GPUs";

// A row: whose need it is, whether it can only be judged once R is staged and the eval set made, what stands in the
// way, and the words for it: `why`, then what `more` adds.  For each feature the first row that holds is named.
struct Need {
  unsigned who;
  bool staged;
  bool (*unmet)(const G&);
  const char* why;
  std::string (*more)(const G&);
};
const Need kNeeds[] = {
    {kNegs, false, [](const G& g) { return g.evalnegs < 0; }, "SLIM_OPTION_GPU_EVALNEGS must be at least 0, not ",
     [](const G& g) { return std::to_string(g.evalnegs); }},
    {kExposure, false, [](const G& g) { return g.evalexpo != 1; }, "SLIM_OPTION_GPU_EVALEXPOSURE must be 0 or 1, not ",
     [](const G& g) { return std::to_string(g.evalexpo); }},
    {kNegs, false, [](const G& g) { return g.filter != nullptr; },
     "a candidate filter is given: candidate rows take no filter", nullptr},
    {kNamed, false, [](const G& g) { return g.admm; }, "the ADMM solver leaves no model in HBM", nullptr},
    {kNamed, false, several_gpus, kSeveral, nullptr},
    {kNamed, false, [](const G& g) { return g.keep_on_host; }, "SLIM_GPU_RESIDENT=0 keeps the models on the host", nullptr},
    {kNamed, false, [](const G& g) { return g.eval_on_host; }, "SLIM_GPU_EVAL_RESIDENT=0 evaluates through the host",
     nullptr},
    {kNegs, false, no_list_length, "",
     [](const G& g) { return nrcmds_is(g) + ": the candidate lists use the eval set's cutoffs, 1 to 128"; }},
    {kExposure, false, no_list_length, "",
     [](const G& g) { return nrcmds_is(g) + ": the lists behind the evaluation have 1 to 128 places"; }},
    {kStride | kFilter, false, [](const G& g) { return g.nrcmds < 1; }, "", nrcmds_is},
    // (a stride has never said which of the four it was)
    {kStride, false, [](const G& g) { return g.admm || several_gpus(g) || g.keep_on_host || g.eval_on_host; }, "", nullptr},
    {kExposure, false, [](const G& g) { return g.evalnegs > 0; },
     "SLIM_OPTION_GPU_EVALNEGS is on: the exposure of sampled candidate lists is not built", nullptr},
    // once R is staged: replicas on other GPUs, a matrix with merged duplicates, ...
    {kExposure | kFilter, true, [](const G& g) { return g.mat && !matrix_replicas(g.mat).empty(); }, kSeveral, nullptr},
    {kStride, true, no_evalset, "", [](const G&) { return std::string(last_error()); }},
    {kNamed, true, no_evalset, "",
     [](const G&) { return *last_error() ? std::string(last_error()) : std::string("the eval set could not be made"); }},
    {kFilter, true, [](const G& g) { return filter_host(g.filter).ncols != staged_ncols(g); }, "the filter was made for ",
     [](const G& g) {
       return std::to_string(filter_host(g.filter).ncols) + " items, the resident models have " +
              std::to_string(staged_ncols(g));
     }},
};

int32_t refuse(const Feature& f, const std::string& why) {
  set_error(f.needs + (why.empty() ? std::string() : ": " + why));
  return SLIM_ERROR_INPUT;
}

int32_t slot(const int32_t* ioptions, int which, int32_t unset) {
  return !ioptions || ioptions[which] == -1 ? unset : ioptions[which];
}

bool env_is_0(const char* name) {
  const char* e = std::getenv(name);
  return e && std::atoi(e) == 0;
}

// where the models of a grid live: the number of GPUs and the two switches of the environment, read here alone
void read_route(const int32_t* ioptions, LearnOptions* base, bool* keep_on_host, bool* eval_on_host) {
  // (SLIM_GPU_NGPUS for callers that cannot set the slot: the unchanged reference CLIs and Python wrapper)
  if (slot(ioptions, SLIM_OPTION_GPU_NGPUS, -1) == -1)
    if (const char* e = std::getenv("SLIM_GPU_NGPUS")) base->ngpus = std::max(1, std::atoi(e));
  *keep_on_host = env_is_0("SLIM_GPU_RESIDENT");
  *eval_on_host = env_is_0("SLIM_GPU_EVAL_RESIDENT");
}

}  // namespace

bool grid_can_open_on(const int32_t* ioptions, const double* doptions) {
  LearnOptions base = decode_options(ioptions, doptions);
  bool keep_on_host = false, eval_on_host = false;
  read_route(ioptions, &base, &keep_on_host, &eval_on_host);
  return base.algo == SLIM_ALGO_CD && base.ngpus <= 1 && !keep_on_host && !eval_on_host;
}

slimgpu_grid::~slimgpu_grid() {
  csr_free(model);
  model_free(dmodel);
  candset_free(cands);
  evalset_free(evalset);
  std::free(fmarker);
  matrix_free(mat);
}

// the option slots and the environment, each read here and nowhere else; values no grid can have are refused
int32_t slimgpu_grid::decode(const int32_t* ioptions, const double* doptions) {
  base = decode_options(ioptions, doptions);
  if (base.algo != SLIM_ALGO_CD && base.algo != SLIM_ALGO_ADMM) {
    set_error("Py_SLIM_Mselect: unknown algorithm");
    return SLIM_ERROR_INPUT;
  }
  admm = base.algo == SLIM_ALGO_ADMM;
  nrcmds = slot(ioptions, SLIM_OPTION_NRCMDS, 10);
  stride = slot(ioptions, SLIM_OPTION_GPU_EVALSTRIDE, 1);  // every stride-th user only
  if (stride < 1) {
    set_error("Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALSTRIDE must be at least 1");
    return SLIM_ERROR_INPUT;
  }
  read_route(ioptions, &base, &keep_on_host, &eval_on_host);
  // sampled negatives (slim_gpu_cand.h), drawn uniformly or by item popularity (slim_gpu_sample.h); exposure
  evalnegs = slot(ioptions, SLIM_OPTION_GPU_EVALNEGS, 0);
  evalseed = (uint64_t)(uint32_t)slot(ioptions, SLIM_OPTION_GPU_EVALSEED, 1);
  evalnegpop = slot(ioptions, SLIM_OPTION_GPU_EVALNEGPOP, 0);
  evalexpo = slot(ioptions, SLIM_OPTION_GPU_EVALEXPOSURE, 0);
  if (evalnegpop != 0 && (evalnegpop != 1 || evalnegs <= 0)) {
    set_error(evalnegpop != 1
                  ? "Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALNEGPOP must be 0 or 1, not " + std::to_string(evalnegpop)
                  : "Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALNEGPOP weights the sampled negatives and "
                    "SLIM_OPTION_GPU_EVALNEGS is off: there is nothing to weight");
    return SLIM_ERROR_INPUT;
  }
  int32_t trn_rows = trn ? trn->nrows : 0;
  if (!trn) matrix_info(mat, &trn_rows, nullptr, nullptr);
  nall = std::min(trn_rows, tst->nrows);
  if (stride > 1)
    for (int64_t u = 0; u < nall; u += stride) sel.push_back((int32_t)u);
  return SLIM_OK;
}

// Whatever stands in the way of a mode that was asked for is refused, before the first solve: there is no silent
// fall-back to the full-catalogue figures.
int32_t slimgpu_grid::check_needs(bool staged) {
  for (const int at : staged ? kOrderStaged : kOrderBefore) {
    const Feature& f = kFeatures[at];
    if (!f.asked(*this)) continue;
    for (const Need& n : kNeeds)
      if ((n.who & f.id) && n.staged == staged && n.unmet(*this))
        return refuse(f, n.why + (n.more ? n.more(*this) : std::string()));
  }
  return SLIM_OK;
}

// The eval set: listed cutoffs up to 128, ranked above.  Without one (SLIM_GPU_EVAL_RESIDENT=0, or a refusal: a
// matrix whose repeated pairs were merged) a plain grid evaluates through lists; the other modes have no such form.
void slimgpu_grid::make_evalset() {
  const bool may_reside = !admm && matrix_replicas(mat).empty() && nrcmds >= 1 && !keep_on_host;
  resident = may_reside && nrcmds <= 128;
  if (!may_reside || eval_on_host) return;
  const int32_t nsel = (int32_t)sel.size();
  const int32_t* users = sel.empty() ? nullptr : sel.data();
  int32_t status = SLIM_ERROR;
  if (nrcmds <= 128) {
    evalset = evalset_create(mat, tst, fmarker, ncols, 1, &nrcmds, nsel, users, &status);
  } else {
    evalset = evalset_create_ranked(mat, tst, fmarker, ncols, nsel, users, &status);
    ranked = resident = evalset != nullptr;
  }
  if (!evalset && stride == 1 && !filter && !evalexpo) set_error("");  // (a plain grid goes on without it)
}

int32_t slimgpu_grid::open(const int32_t* ioptions, const double* doptions, int32_t marker_ncols, int32_t nsolves) {
  int32_t status = decode(ioptions, doptions);
  if (status == SLIM_OK) status = check_needs(false);
  if (status != SLIM_OK) return status;
  if (!admm) {
    mat = multi_from_host(trn->nrows, trn->rowptr, trn->rowind, trn->rowval, base, &status);
    if (!mat) return status;
    // nsolves solves over one R: the engine may pay for G = R^T R once (cd_gram.hpp)
    matrix_expect_solves(mat, nsolves);
  }
  ncols = marker_ncols > 0 ? marker_ncols  // pyapi.c:255-257
                           : std::max(max_index_plus_one(trn->rowptr[trn->nrows], trn->rowind),
                                      max_index_plus_one(tst->rowptr[tst->nrows], tst->rowind));
  fmarker = head_tail_split(trn->nrows, ncols, trn->rowptr, trn->rowind);
  if (mat) make_evalset();
  status = check_needs(true);
  return status != SLIM_OK ? status : sample_candidates();
}

// the candidate set is drawn once, on the device, from the eval set's users; every pair is evaluated on it
int32_t slimgpu_grid::sample_candidates() {
  if (evalnegs <= 0) return SLIM_OK;
  int32_t status = SLIM_ERROR;
  cands = evalnegpop ? evalset_sample_candidates_weighted(evalset, evalnegs, evalseed, nullptr, &status)
                     : evalset_sample_candidates(evalset, evalnegs, evalseed, &status);
  return cands ? SLIM_OK : refuse(kFeatures[0], last_error());
}

// A grid on a matrix that is staged already (a train half made by SLIMGPU_MatrixSplit): nothing of the training rows
// is on the host, so the models stay in HBM and are evaluated there, or the grid is refused.  The marker is formed
// from the matrix's column pointer: head_tail_split reads the entry count of every item and the count of all entries,
// and the pointer holds both.
int32_t slimgpu_grid::open_on(slimgpu_matrix_t* staged, const int32_t* ioptions, const double* doptions,
                              int32_t marker_ncols, int32_t nsolves) {
  const std::string who = "SLIMGPU_GridOpenOn: ";
  auto refuse_on = [&](const std::string& why) {
    mat = nullptr;  // (the matrix stays the caller's)
    set_error(who + why);
    return (int32_t)SLIM_ERROR_INPUT;
  };
  mat = staged;
  int32_t status = decode(ioptions, doptions);
  if (status == SLIM_OK) status = check_needs(false);
  if (status != SLIM_OK) {
    mat = nullptr;
    return status;
  }
  const char* on_device = "a grid on a staged matrix keeps its models in HBM and evaluates them there: ";
  if (admm) return refuse_on(std::string(on_device) + "the ADMM solver leaves no model in HBM");
  if (several_gpus(*this) || !matrix_replicas(mat).empty()) return refuse_on(std::string(on_device) + kSeveral);
  if (keep_on_host) return refuse_on(std::string(on_device) + "SLIM_GPU_RESIDENT=0 keeps the models on the host");
  if (eval_on_host) return refuse_on(std::string(on_device) + "SLIM_GPU_EVAL_RESIDENT=0 evaluates through the host");
  if (nrcmds < 1) return refuse_on(std::string(on_device) + nrcmds_is(*this));
  int32_t mrows = 0, mcols = 0;
  int64_t mnnz = 0;
  matrix_info(mat, &mrows, &mcols, &mnnz);
  ncols = marker_ncols > 0 ? marker_ncols : std::max(mcols, max_index_plus_one(tst->rowptr[tst->nrows], tst->rowind));
  std::vector<int64_t> cp((size_t)mcols + 1, 0), pop((size_t)ncols, 0);
  if (matrix_get_column_view(mat, cp.data(), nullptr, nullptr, nullptr) != SLIM_OK)
    return refuse_on("the staged matrix has no column view");
  for (int32_t i = 0; i < std::min(ncols, mcols); ++i) pop[(size_t)i] = cp[(size_t)i + 1] - cp[(size_t)i];
  fmarker = head_tail_from_counts(ncols, pop, mnnz);
  make_evalset();
  if (!evalset)
    return refuse_on(std::string(on_device) +
                     (*last_error() ? std::string(last_error()) : std::string("the eval set could not be made")));
  status = check_needs(true);
  if (status == SLIM_OK) status = sample_candidates();
  if (status != SLIM_OK) {
    mat = nullptr;
    return status;
  }
  // (behind the last refusal: a matrix that goes back to the caller goes back as it came)
  matrix_expect_solves(mat, nsolves);
  return SLIM_OK;
}

// Groups ride on the eval set: a grid without one has nothing to form them from, and is refused rather than
// evaluated over everybody.
int32_t slimgpu_grid::set_groups(int32_t ngroups_, const int32_t* group_of_user, int32_t select_group_) {
  const std::string who = "SLIMGPU_GridSetGroups: ";
  auto refuse_input = [&](const std::string& why) {
    set_error(who + why);
    return (int32_t)SLIM_ERROR_INPUT;
  };
  if (ngroups_ >= 1 && (select_group_ < -1 || select_group_ >= ngroups_))
    return refuse_input("select_group " + std::to_string(select_group_) + " is outside [-1, " +
                        std::to_string(ngroups_) + ")");
  if (dmodel || model) return refuse_input("the groups are set before the first solve");
  if (!evalset)
    return refuse_input(
        "groups need the evaluation in HBM (cd on one GPU, nrcmds >= 1, SLIM_GPU_RESIDENT and SLIM_GPU_EVAL_RESIDENT "
        "not 0, a matrix staged without merged pairs)" +
        (*last_error() ? ": " + std::string(last_error()) : std::string()));
  // (the number of groups and the group of every user are the eval set's to judge)
  if (const int32_t rc = evalset_set_groups(evalset, ngroups_, group_of_user); rc != SLIM_OK) return rc;
  ngroups = ngroups_;
  select_group = select_group_;
  return SLIM_OK;
}

int32_t slimgpu_grid::last_groups(EvalResult* rows) const {
  if (ngroups == 0 || !evalset) {
    set_error("SLIMGPU_GridLastGroups: no groups are set on this grid");
    return SLIM_ERROR_INPUT;
  }
  if (!group_rows_stand) {
    set_error("SLIMGPU_GridLastGroups: the last pair was not evaluated per group");
    return SLIM_ERROR_INPUT;
  }
  return evalset_group_figures(evalset, 1, rows);
}

int32_t slimgpu_grid::group_members(int32_t* members) const {
  int32_t n = 0;
  return evalset_group_info(evalset, &n, members);
}

void slimgpu_grid::describe() const {
  if (stride > 1) std::printf("  evaluating every %d-th user: %zu of %d\n", stride, sel.size(), nall);
  if (filter) {
    const HostFilter hflt = filter_host(filter);
    int64_t allowed = hflt.ncols;
    if (hflt.bits) {
      allowed = 0;
      for (int32_t k = 0; k < hflt.ncols; ++k) allowed += (hflt.bits[k >> 5] >> (k & 31)) & 1u;
    }
    std::printf("  item filter: %lld of %d items allowed, %lld exclusion entries\n", (long long)allowed, hflt.ncols,
                (long long)(hflt.xptr ? hflt.xptr[hflt.xusers] : 0));
  }
  if (ngroups > 0)
    std::printf("  user groups: %d, pairs chosen on %s\n", ngroups,
                select_group < 0 ? "everybody" : ("group " + std::to_string(select_group)).c_str());
  if (cands) {
    int64_t entries = 0;
    candset_info(cands, nullptr, nullptr, &entries);
    std::printf("  sampled negatives: nnegs %d, seed %llu, %s%lld candidate entries\n", evalnegs,
                (unsigned long long)evalseed, evalnegpop ? "popularity, " : "", (long long)entries);
  }
}

// the next model, warm-started from the previous pair's, which it replaces
int32_t slimgpu_grid::learn(const LearnOptions& opt) {
  int32_t status = SLIM_ERROR;
  if (resident) {
    csr_free(model);  // (a copy of the previous pair's model that somebody asked for)
    model = nullptr;
    slimgpu_model* prev = dmodel;
    dmodel = learn_resident(mat, opt, prev, &status);
    model_free(prev);
    return dmodel ? SLIM_OK : status;
  }
  slim_csr_t* prev = model;
  // (ADMM ignores the previous model, estimate.c:38)
  model = admm ? learn_admm(trn->nrows, trn->rowptr, trn->rowind, trn->rowval, opt, &status)
               : multi_learn(mat, opt, prev, &status);
  csr_free(prev);
  return model ? SLIM_OK : status;
}

// the planned call: the figures of a resident model, made where it lies
int32_t slimgpu_grid::evaluate_in_hbm(EvalResult* ev, slimgpu_exposure_t* expo) {
  if (!evalset) return SLIM_ERROR;
  if (cands) return model_evaluate_candidates(evalset, dmodel, cands, 1, ev);
  if (ranked) return model_evaluate_ranked(evalset, dmodel, 1, &nrcmds, ev, filter);
  if (evalexpo) return model_evaluate_exposure(evalset, dmodel, filter, 1, ev, nullptr, expo);
  return model_evaluate(evalset, dmodel, 1, ev, filter);
}

// A plain grid without the eval set: top-N of every user on the GPU (bit-identical to the host scorer) and the hits
// counted there; where the device refuses either, the host loop, which needs the host model.
int32_t slimgpu_grid::evaluate_lists(EvalResult* ev) {
  if (!trn) return SLIM_ERROR;  // (a grid on a staged matrix has no host rows to score: it is evaluated in HBM)
  std::vector<int32_t> lists((size_t)trn->nrows * nrcmds, -1), lens((size_t)trn->nrows, 0);
  std::vector<float> lsc((size_t)trn->nrows * nrcmds, 0.0f);
  bool on_gpu;
  if (resident) {
    DeviceRowView wv;
    on_gpu = model_row_view(dmodel, &wv) == SLIM_OK &&
             predict_device_view(wv, trn, nrcmds, lists.data(), lsc.data(), lens.data()) == SLIM_OK;
  } else {
    on_gpu = nrcmds <= 128 ? predict_device(model, trn, nrcmds, lists.data(), lsc.data(), lens.data()) == SLIM_OK
                           : nrcmds <= SLIMGPU_MAX_LIST && predict_policy() != 0 &&
                                 predict_lists(model, trn, nrcmds, lists.data(), lsc.data(), lens.data()) == SLIM_OK;
  }
  if (on_gpu && evaluate_device(nall, nrcmds, lists.data(), lens.data(), tst, fmarker, ncols, ev) == SLIM_OK)
    return SLIM_OK;
  int32_t status = SLIM_ERROR;
  if (!host_model(&status)) return status;
  *ev = on_gpu ? evaluate(model, trn, tst, nrcmds, fmarker, ncols, lists.data(), lens.data())
               : evaluate(model, trn, tst, nrcmds, fmarker, ncols);
  return SLIM_OK;
}

int32_t slimgpu_grid::solve(double l1r, double l2r, slimgpu_grid_cell_t* cell) {
  LearnOptions opt = base;
  opt.l1r = l1r;
  opt.l2r = l2r;
  group_rows_stand = false;
  int32_t status = learn(opt);
  if (status != SLIM_OK) return status;
  *cell = slimgpu_grid_cell_t{};
  cell->l1r = l1r;
  cell->l2r = l2r;
  cell->nnz = resident ? model_nnz(dmodel) : (int64_t)model->rowptr[model->nrows];
  cell->solve_seconds = last_stats().total_ms / 1e3;
  EvalResult ev;
  if (evaluate_in_hbm(&ev, &cell->exposure) != SLIM_OK) {
    // (no silent evaluation of everybody, without the filter, on the whole catalogue, without the exposure, or in
    // place of the groups)
    if (stride > 1 || filter || cands || evalexpo || ngroups > 0) return SLIM_ERROR;
    status = evaluate_lists(&ev);
    if (status != SLIM_OK) return status;
  }
  figures_out(ev, cell->metrics, cell->nvalid);
  group_rows_stand = ngroups > 0;  // (with groups the figures can only have come from the eval set)
  cell->has_exposure = evalexpo;
  return SLIM_OK;
}

slim_csr_t* slimgpu_grid::host_model(int32_t* status) {
  int32_t st = SLIM_ERROR;
  if (!model && dmodel) model = model_fetch(dmodel, &st);
  if (status) *status = model ? SLIM_OK : st;
  return model;
}

// ---- include/slim_gpu_grid.h: the object, call for call ---------------------------------------------------------------
extern "C" {

int32_t SLIMGPU_GridOpen(slim_t* trnhandle, slim_t* tsthandle, int32_t* ioptions, double* doptions, int32_t ncols,
                         int32_t nsolves, slimgpu_filter_t* filter, slimgpu_grid_t** grid) {
  const slim_csr_t* trn = static_cast<slim_csr_t*>(trnhandle);
  const slim_csr_t* tst = static_cast<slim_csr_t*>(tsthandle);
  if (!trn || !tst || !trn->rowptr || !tst->rowptr || !grid) return SLIM_ERROR_INPUT;
  set_error("");
  slimgpu_grid* g = new slimgpu_grid(trn, tst, filter);
  const int32_t status = g->open(ioptions, doptions, ncols, nsolves);
  if (status == SLIM_OK) *grid = g;
  else delete g;
  return status;
}

int32_t SLIMGPU_GridOpenOn(slimgpu_matrix_t* trn, slim_t* tsthandle, int32_t* ioptions, double* doptions,
                           int32_t ncols, int32_t nsolves, slimgpu_filter_t* filter, slimgpu_grid_t** grid) {
  const slim_csr_t* tst = static_cast<slim_csr_t*>(tsthandle);
  if (!trn || !tst || !tst->rowptr || !grid) return SLIM_ERROR_INPUT;
  set_error("");
  slimgpu_grid* g = new slimgpu_grid(nullptr, tst, filter);
  const int32_t status = g->open_on(trn, ioptions, doptions, ncols, nsolves);
  if (status == SLIM_OK) *grid = g;
  else delete g;
  return status;
}

void SLIMGPU_GridDescribe(const slimgpu_grid_t* grid) { grid->describe(); }

int32_t SLIMGPU_GridSolve(slimgpu_grid_t* grid, double l1r, double l2r, slimgpu_grid_cell_t* cell) {
  return grid->solve(l1r, l2r, cell);
}

slim_t* SLIMGPU_GridModel(slimgpu_grid_t* grid, int32_t* status) { return grid->host_model(status); }

int32_t SLIMGPU_GridSetGroups(slimgpu_grid_t* grid, int32_t ngroups, const int32_t* group_of_user,
                              int32_t select_group) {
  set_error("");
  if (!grid || !group_of_user) {
    set_error("SLIMGPU_GridSetGroups: bad arguments (a grid, a group for every user)");
    return SLIM_ERROR_INPUT;
  }
  return grid->set_groups(ngroups, group_of_user, select_group);
}

int32_t SLIMGPU_GridGroupInfo(const slimgpu_grid_t* grid, int32_t* ngroups, int32_t* members) {
  set_error("");
  if (!grid || !ngroups || grid->ngroups == 0) {
    set_error(grid && ngroups ? "SLIMGPU_GridGroupInfo: no groups are set on this grid"
                              : "SLIMGPU_GridGroupInfo: bad arguments (a grid, ngroups)");
    return SLIM_ERROR_INPUT;
  }
  *ngroups = grid->ngroups;
  return members ? grid->group_members(members) : SLIM_OK;
}

int32_t SLIMGPU_GridLastGroups(slimgpu_grid_t* grid, double* metrics, int32_t* nvalid) {
  set_error("");
  if (!grid || !metrics || !nvalid) {
    set_error("SLIMGPU_GridLastGroups: bad arguments (a grid, the outputs)");
    return SLIM_ERROR_INPUT;
  }
  std::vector<EvalResult> rows((size_t)grid->ngroups + 1);
  if (const int32_t rc = grid->last_groups(rows.data()); rc != SLIM_OK) return rc;
  for (int32_t g = 0; g <= grid->ngroups; ++g) figures_out(rows[(size_t)g], metrics + 4 * g, nvalid + 3 * g);
  return SLIM_OK;
}

void SLIMGPU_GridFree(slimgpu_grid_t** grid) {
  if (!grid) return;
  delete *grid;
  *grid = nullptr;
}

}  // extern "C"
