// slim_abi.cpp -- every exported symbol of libslim.so (include/slim.h, slim_gpu.h).
//
// Thin C-ABI shim: decodes the option arrays, moves data between the caller's
// buffers and the engine, never computes a CD update on the host.  SLIM_Learn /
// Py_SLIM_Learn / Py_SLIM_Mselect reach the solver only through
// slimamd::learn_cd (HIP, engine.hip); if no gfx950 device is usable they fail
// with SLIM_ERROR* and a message -- there is no CPU fallback.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "grid_eval.hpp"
#include "host_csr.hpp"

using namespace slimamd;

namespace {

slim_csr_t* as_csr(slim_t* h) { return static_cast<slim_csr_t*>(h); }

// SLIM_Learn body shared by the C and Python entry points (the reference
// duplicates it: src/libslim/api.c:36-95 == src/libslim/pyapi.c:136-198).
slim_csr_t* learn_from_host(int32_t nrows, const ssize_t* rowptr, const int32_t* rowind,
                            const float* rowval, int32_t* ioptions, double* doptions,
                            const slim_csr_t* imodel, int32_t* status) {
  set_error("");
  LearnOptions opt = decode_options(ioptions, doptions);
  if (opt.algo == SLIM_ALGO_ADMM)  // estimate.c:38-304 (MKL-only in the reference): admm.hip
    return learn_admm(nrows, rowptr, rowind, rowval, opt, status);
  if (opt.algo != SLIM_ALGO_CD) {  // api.c:81-84 prints "Algorithm not supported" and exits
    set_error("unknown algorithm: algo must be cd (coordinate descent) or admm");
    *status = SLIM_ERROR_INPUT;
    return nullptr;
  }
  if (opt.simtype < SLIM_SIMTYPE_COS || opt.simtype > SLIM_SIMTYPE_DOTP) {
    set_error("unknown similarity type (neighbors.c:121-123)");
    *status = SLIM_ERROR_INPUT;
    return nullptr;
  }
  // ngpus (option slot 19, or SLIM_GPU_NGPUS in the environment for callers that cannot set
  // it -- the unchanged reference CLIs and Python wrapper): one host thread per device
  if (ioptions == nullptr || ioptions[SLIM_OPTION_GPU_NGPUS] == -1)
    if (const char* e = std::getenv("SLIM_GPU_NGPUS")) opt.ngpus = std::max(1, std::atoi(e));
  slimgpu_matrix_t* mat = multi_from_host(nrows, rowptr, rowind, rowval, opt, status);
  if (!mat) return nullptr;
  slim_csr_t* model = multi_learn(mat, opt, imodel, status);
  if (model && (opt.dbglvl & SLIM_DBG_TIME)) {  // timing.c:27-45
    const slimgpu_stats_t& s = last_stats();
    std::printf("\nTiming Information -------------------------------------------------");
    std::printf("\n Total: \t %7.3lf", (s.setup_ms + s.total_ms) / 1e3);
    std::printf("\n   Setup: \t\t %7.3lf", s.setup_ms / 1e3);
    std::printf("\n   Learn: \t\t %7.3lf", s.total_ms / 1e3);
    std::printf("\n     kernel: \t\t %7.3lf", s.kernel_ms / 1e3);
    std::printf("\n********************************************************************\n");
  }
  matrix_free(mat);
  return model;
}

}  // namespace

// Where Py_SLIM_Predict scores: SLIM_PREDICT=gpu|cpu|auto (default auto: the GPU scorer when
// a device is present and nrcmds <= SLIMGPU_MAX_LIST -- the chunk or the wave kernel up to 128, the
// long-list form of the chunk kernel beyond -- else the host scorer; all give identical lists).
// A refusal of the device (above 128: model rows that do not ascend, a split table beyond 2 GB) falls
// back to the host scorer under auto and is the call's status under gpu.
int slimamd::predict_policy() {
  const char* e = std::getenv("SLIM_PREDICT");
  if (e && std::strcmp(e, "cpu") == 0) return 0;
  if (e && std::strcmp(e, "gpu") == 0) return 2;
  return 1;
}

extern "C" {

// ---------------------------------------------------------------- slim.h ------

int32_t SLIM_iSetDefaults(int32_t* options) {
  for (int i = 0; i < SLIM_NOPTIONS; ++i) options[i] = -1;
  return SLIM_OK;
}

int32_t SLIM_dSetDefaults(double* options) {
  for (int i = 0; i < SLIM_NOPTIONS; ++i) options[i] = -1;
  return SLIM_OK;
}

slim_t* SLIM_Learn(int32_t nrows, ssize_t* rowptr, int32_t* rowind, float* rowval,
                   int32_t* ioptions, double* doptions, slim_t* imodel, int32_t* r_status) {
  int32_t status = SLIM_ERROR;
  slim_csr_t* model =
      learn_from_host(nrows, rowptr, rowind, rowval, ioptions, doptions, as_csr(imodel), &status);
  if (r_status) *r_status = status;
  return model;
}

int32_t SLIM_GetTopN(slim_t* model, int32_t nratings, int32_t* itemids, float* ratings,
                     int32_t* /*ioptions*/, int32_t nrcmds, int32_t* rids, float* rscores) {
  const slim_csr_t* W = as_csr(model);
  if (!W || !W->rowptr || nrcmds < 0) return SLIM_ERROR;
  TopNScratch ws(W->ncols > W->nrows ? W->ncols : W->nrows);
  return top_n(W, nratings, itemids, ratings, nrcmds, rids, rscores, ws);
}

int32_t SLIM_WriteModel(slim_t* model, char* filename) {
  const slim_csr_t* W = as_csr(model);
  if (!W || !W->rowptr) return SLIM_ERROR_INPUT;
  return write_binrow(W, filename) ? SLIM_OK : SLIM_ERROR;
}

slim_t* SLIM_ReadModel(char* filename) {
  slim_csr_t* W = read_binrow(filename);
  if (W) csr_build_index(W, 0);  // api.c:191: add the column view
  return W;
}

void SLIM_FreeModel(slim_t** model) {
  if (!model) return;
  csr_free(as_csr(*model));
  *model = nullptr;
}

int32_t* SLIM_DetermineHeadAndTail(int32_t nrows, int32_t ncols, ssize_t* rowptr,
                                   int32_t* rowind) {
  return head_tail_split(nrows, ncols, rowptr, rowind);
}

// ------------------------------------------------------------ Py_* (pyapi.c) --

int32_t Py_csr_wrapper(int32_t nrows, ssize_t* rowptr, int32_t* rowind, float* rowval,
                       slim_t** matrix_out) {
  slim_csr_t* m = csr_from_rows(nrows, rowptr, rowind, rowval);
  if (!m) return SLIM_ERROR_MEMORY;
  *matrix_out = m;
  return SLIM_OK;
}

int32_t Py_csr_save(slim_t* mathandle, char* fname) {
  const slim_csr_t* m = as_csr(mathandle);
  if (!m || !m->rowptr) return SLIM_ERROR_INPUT;
  return write_text_csr(m, fname) ? SLIM_OK : SLIM_ERROR;
}

int32_t Py_csr_load(slim_t** mathandle, char* fname) {
  slim_csr_t* m = read_text_csr(fname);
  if (!m) return SLIM_ERROR;
  *mathandle = m;
  return SLIM_OK;
}

int32_t Py_csr_free(slim_t* mathandle) {
  csr_free(as_csr(mathandle));
  return SLIM_OK;
}

int32_t Py_csr_stat(slim_t* mathandle, int32_t* nnz) {
  const slim_csr_t* m = as_csr(mathandle);
  if (!m || !m->rowptr) return SLIM_ERROR_INPUT;
  *nnz = (int32_t)m->rowptr[m->nrows];
  return SLIM_OK;
}

int32_t Py_csr_export(slim_t* mathandle, int32_t* indptr, int32_t* indices, float* data) {
  const slim_csr_t* m = as_csr(mathandle);
  if (!m || !m->rowptr) return SLIM_ERROR_INPUT;
  const ssize_t nnz = m->rowptr[m->nrows];
  for (int32_t r = 0; r <= m->nrows; ++r) indptr[r] = (int32_t)m->rowptr[r];
  for (ssize_t k = 0; k < nnz; ++k) indices[k] = m->rowind[k];
  if (m->rowval)
    for (ssize_t k = 0; k < nnz; ++k) data[k] = m->rowval[k];
  return SLIM_OK;
}

int32_t Py_SLIM_Learn(slim_t* trnhandle, int32_t* ioptions, double* doptions,
                      slim_t** model_out) {
  const slim_csr_t* trn = as_csr(trnhandle);
  if (!trn || !trn->rowptr) return SLIM_ERROR_INPUT;
  int32_t status = SLIM_ERROR;
  slim_csr_t* model = learn_from_host(trn->nrows, trn->rowptr, trn->rowind, trn->rowval, ioptions,
                                      doptions, nullptr, &status);
  if (!model) return status;
  *model_out = model;
  return SLIM_OK;
}

// Py_SLIM_Mselect is this with no filter.  How the grid's pairs are learnt and evaluated, what each mode needs and what
// is refused before the first solve is grid_eval.cpp's business; this is the loop over arrayl1 x arrayl2.
// force_exposure / cells: Py_SLIM_MselectExposure (slim_gpu_exposure.h), slot 26 on whatever ioptions says.
// groups (slim_gpu_groups.h; none: ngroups == 0): Py_SLIM_MselectGrouped, the best pairs chosen on select_group.
struct MselectGroups {
  int32_t ngroups = 0;
  const int32_t* group_of_user = nullptr;
  int32_t select_group = -1;
  double* cells = nullptr;  // [nl1 * nl2][ngroups + 1][SLIMGPU_GROUP_CELL]
};
static int32_t mselect_impl(slim_t* trnhandle, slim_t* tsthandle, int32_t* ioptions,
                            double* doptions, double* arrayl1, double* arrayl2, int32_t nl1,
                            int32_t nl2, double* bestl1HR, double* bestl2HR, double* bestHRHR,
                            double* bestARHR, double* bestl1AR, double* bestl2AR, double* bestHRAR,
                            double* bestARAR, slimgpu_filter_t* filter, bool force_exposure, double* cells,
                            const MselectGroups& groups = MselectGroups()) {
  const slim_csr_t* trn = as_csr(trnhandle);
  const slim_csr_t* tst = as_csr(tsthandle);
  if (!trn || !tst || !trn->rowptr || !tst->rowptr) return SLIM_ERROR_INPUT;
  set_error("");
  const int32_t ngroups = groups.ngroups;
  std::vector<int32_t> io(SLIM_NOPTIONS, -1);  // (a private copy: the caller's slot 26 stays as it is)
  if (ioptions) io.assign(ioptions, ioptions + SLIM_NOPTIONS);
  if (force_exposure) io[SLIM_OPTION_GPU_EVALEXPOSURE] = 1;
  slimgpu_grid grid(trn, tst, filter);
  int32_t rc = grid.open(io.data(), doptions, 0, nl1 * nl2);
  if (rc == SLIM_OK && ngroups > 0) rc = grid.set_groups(ngroups, groups.group_of_user, groups.select_group);
  if (rc != SLIM_OK) return rc;
  std::vector<EvalResult> rows((size_t)ngroups + 1);
  std::vector<int32_t> members((size_t)ngroups + 1);
  if (ngroups > 0) grid.group_members(members.data());

  std::printf("------------------------------------------------------------------\n");
  std::printf("SLIM, version %s (MI355X engine)\n", SLIM_VERSION);
  std::printf("------------------------------------------------------------------\n");
  std::printf("  trn matrix, nrows: %d, ncols: %d, nnz: %zd\n", trn->nrows, grid.ncols,
              trn->rowptr[trn->nrows]);
  std::printf("  tst matrix, nrows: %d, ncols: %d, nnz: %zd\n", tst->nrows,
              max_index_plus_one(tst->rowptr[tst->nrows], tst->rowind), tst->rowptr[tst->nrows]);
  std::printf("  optTol: %.2le, niters: %d\n", grid.base.optTol, grid.base.maxniters);
  grid.describe();
  std::printf("\nEstimating & evaluating models...\n\n");

  *bestHRHR = *bestARHR = *bestHRAR = *bestARAR = 0.0;
  for (int32_t a = 0; a < nl1 && rc == SLIM_OK; ++a) {
    for (int32_t b = 0; b < nl2; ++b) {
      doptions[SLIM_OPTION_L1R] = arrayl1[a];  // the reference writes these through
      doptions[SLIM_OPTION_L2R] = arrayl2[b];  // to the caller's array (pyapi.c:288-289)
      slimgpu_grid_cell_t c;
      rc = grid.solve(arrayl1[a], arrayl2[b], &c);
      if (rc != SLIM_OK) break;
      double hr = c.metrics[0], arhr = c.metrics[3];
      int32_t nvalid = c.nvalid[0];
      std::printf("l1r: %.2le l2r: %.2le nnz: %7zd hr: %.4f hr_head: %.4f hr_tail: %.4f "
                  "arhr: %.4f time: %.2lf\n",
                  c.l1r, c.l2r, (ssize_t)c.nnz, hr, c.metrics[1], c.metrics[2], arhr, c.solve_seconds);
      if (c.has_exposure) {  // (the lists of the grid's nrcmds, counted where the evaluation made them)
        const slimgpu_exposure_t& expo = c.exposure;
        std::printf("  exposure@%d: coverage: %.4f tail_share: %.4f gini: %.4f avg_pop: %.2f distinct: %d slots: %lld\n",
                    grid.nrcmds, expo.coverage, expo.tail_share, expo.gini, expo.avg_pop, expo.distinct,
                    (long long)expo.slots);
        if (cells) {
          double* out = cells + (size_t)SLIMGPU_EXPOSURE_CELL * ((size_t)a * (size_t)nl2 + (size_t)b);
          out[0] = c.l1r; out[1] = c.l2r; out[2] = hr; out[3] = arhr;
          out[4] = expo.coverage; out[5] = expo.tail_share; out[6] = expo.gini; out[7] = expo.avg_pop;
        }
      }
      if (ngroups > 0) {  // (formed from the records of the pair's one scoring pass)
        rc = grid.last_groups(rows.data());
        if (rc != SLIM_OK) break;
        for (int32_t g = 0; g <= ngroups; ++g) {
          const EvalResult& r = rows[(size_t)g];
          if (g < ngroups)
            std::printf("  group %d: members: %d hr: %.4f hr_head: %.4f hr_tail: %.4f arhr: %.4f nvalid: %d\n", g,
                        members[(size_t)g], r.hr, r.hr_head, r.hr_tail, r.arhr, r.nvalid);
          if (groups.cells) {
            double* out = groups.cells + (size_t)SLIMGPU_GROUP_CELL *
                                             (((size_t)a * (size_t)nl2 + (size_t)b) * ((size_t)ngroups + 1) + (size_t)g);
            out[0] = c.l1r; out[1] = c.l2r; out[2] = r.hr; out[3] = r.hr_head; out[4] = r.hr_tail; out[5] = r.arhr;
            out[6] = r.nvalid; out[7] = r.nvalid_head; out[8] = r.nvalid_tail;
          }
        }
        if (groups.select_group >= 0) {  // the pairs are chosen on this group's figures
          const EvalResult& r = rows[(size_t)groups.select_group];
          hr = r.hr; arhr = r.arhr; nvalid = r.nvalid;
        }
      }
      if (nvalid < 1) {  // pyapi.c:377-381
        *bestl1HR = c.l1r;
        *bestl2HR = c.l2r;
        rc = SLIM_ERROR;
        break;
      }
      if (hr > *bestHRHR) {
        *bestHRHR = hr;
        *bestARHR = arhr;
        *bestl1HR = c.l1r;
        *bestl2HR = c.l2r;
      }
      if (arhr > *bestARAR) {
        *bestHRAR = hr;
        *bestARAR = arhr;
        *bestl1AR = c.l1r;
        *bestl2AR = c.l2r;
      }
    }
  }
  std::printf("\nDone.\n------------------------------------------------------------------\n");
  return rc;
}

int32_t Py_SLIM_MselectFiltered(slim_t* trnhandle, slim_t* tsthandle, int32_t* ioptions,
                                double* doptions, double* arrayl1, double* arrayl2, int32_t nl1,
                                int32_t nl2, double* bestl1HR, double* bestl2HR, double* bestHRHR,
                                double* bestARHR, double* bestl1AR, double* bestl2AR, double* bestHRAR,
                                double* bestARAR, slimgpu_filter_t* filter) {
  return mselect_impl(trnhandle, tsthandle, ioptions, doptions, arrayl1, arrayl2, nl1, nl2, bestl1HR, bestl2HR,
                      bestHRHR, bestARHR, bestl1AR, bestl2AR, bestHRAR, bestARAR, filter, false, nullptr);
}

int32_t Py_SLIM_MselectExposure(slim_t* trnhandle, slim_t* tsthandle, int32_t* ioptions,
                                double* doptions, double* arrayl1, double* arrayl2, int32_t nl1,
                                int32_t nl2, double* bestl1HR, double* bestl2HR, double* bestHRHR,
                                double* bestARHR, double* bestl1AR, double* bestl2AR, double* bestHRAR,
                                double* bestARAR, slimgpu_filter_t* filter, double* cells) {
  return mselect_impl(trnhandle, tsthandle, ioptions, doptions, arrayl1, arrayl2, nl1, nl2, bestl1HR, bestl2HR,
                      bestHRHR, bestARHR, bestl1AR, bestl2AR, bestHRAR, bestARAR, filter, true, cells);
}

int32_t Py_SLIM_MselectGrouped(slim_t* trnhandle, slim_t* tsthandle, int32_t* ioptions, double* doptions,
                               double* arrayl1, double* arrayl2, int32_t nl1, int32_t nl2, double* bestl1HR,
                               double* bestl2HR, double* bestHRHR, double* bestARHR, double* bestl1AR,
                               double* bestl2AR, double* bestHRAR, double* bestARAR, slimgpu_filter_t* filter,
                               int32_t ngroups, const int32_t* group_of_user, int32_t select_group, double* cells) {
  // the group arguments are judged before anything is staged (slimgpu_grid::set_groups judges them again)
  const char* who = "Py_SLIM_MselectGrouped";
  const slim_csr_t* trn = as_csr(trnhandle);
  const slim_csr_t* tst = as_csr(tsthandle);
  if (!trn || !tst || !trn->rowptr || !tst->rowptr) return SLIM_ERROR_INPUT;
  set_error("");
  std::vector<int64_t> offsets((size_t)std::max(ngroups, 0) + 1);
  if (!group_of_user) {
    set_error(std::string(who) + ": bad arguments (a group for every user)");
    return SLIM_ERROR_INPUT;
  }
  if (const int32_t rc = group_partition(who, 0, nullptr, std::min(trn->nrows, tst->nrows), ngroups, group_of_user,
                                         nullptr, offsets.data());
      rc != SLIM_OK)
    return rc;
  if (select_group < -1 || select_group >= ngroups) {
    set_error(std::string(who) + ": select_group " + std::to_string(select_group) + " is outside [-1, " +
              std::to_string(ngroups) + ")");
    return SLIM_ERROR_INPUT;
  }
  MselectGroups groups;
  groups.ngroups = ngroups; groups.group_of_user = group_of_user; groups.select_group = select_group;
  groups.cells = cells;
  return mselect_impl(trnhandle, tsthandle, ioptions, doptions, arrayl1, arrayl2, nl1, nl2, bestl1HR, bestl2HR,
                      bestHRHR, bestARHR, bestl1AR, bestl2AR, bestHRAR, bestARAR, filter, false, nullptr, groups);
}

int32_t Py_SLIM_Mselect(slim_t* trnhandle, slim_t* tsthandle, int32_t* ioptions,
                        double* doptions, double* arrayl1, double* arrayl2, int32_t nl1,
                        int32_t nl2, double* bestl1HR, double* bestl2HR, double* bestHRHR,
                        double* bestARHR, double* bestl1AR, double* bestl2AR, double* bestHRAR,
                        double* bestARAR) {
  return Py_SLIM_MselectFiltered(trnhandle, tsthandle, ioptions, doptions, arrayl1, arrayl2, nl1, nl2, bestl1HR,
                                 bestl2HR, bestHRHR, bestARHR, bestl1AR, bestl2AR, bestHRAR, bestARAR, nullptr);
}

// The cross-validated grid (slim_gpu_split.h): mselect_impl's loop once per fold, a pair judged by the mean of its
// fold figures.  One route per call: the data staged once and every fold cut where it lies, the grid opened on the
// train half; or, where that cannot serve, every fold split on the host and its grid opened from the host handles.
// pl1 / pl2: the pairs in the order they are solved (Py_SLIM_MselectCV: the product of its two arrays, l1 outer; the
// command-line program: the lines of its l12 file).
static int32_t mselect_cv_impl(const char* who, slim_t* datahandle, int32_t* ioptions, double* doptions,
                               const int32_t npairs, const double* pl1, const double* pl2, const slimgpu_split_t* split,
                               slimgpu_filter_t* filter, double* bestl1HR, double* bestl2HR, double* bestHRHR,
                               double* bestARHR, double* bestl1AR, double* bestl2AR, double* bestHRAR, double* bestARAR,
                               double* cells) {
  const slim_csr_t* data = as_csr(datahandle);
  set_error("");
  if (!data || !data->rowptr || !doptions || !pl1 || !pl2 || npairs < 1 || !bestl1HR || !bestl2HR || !bestHRHR ||
      !bestARHR || !bestl1AR || !bestl2AR || !bestHRAR || !bestARAR) {
    set_error(std::string(who) + ": bad arguments (a matrix, the options, the pairs, the eight outputs)");
    return SLIM_ERROR_INPUT;
  }
  slimgpu_split_t sp = {};
  if (split) sp = *split;
  sp.fold = 0;  // (not read: every fold is run)
  if (const int32_t rc = split_check(who, split ? &sp : nullptr); rc != SLIM_OK) return rc;
  const int32_t F = sp.nfolds;
  const LearnOptions base = decode_options(ioptions, doptions);
  const bool on_device = grid_can_open_on(ioptions, doptions);
  int32_t rc = SLIM_OK;
  slimgpu_matrix_t* staged = nullptr;
  if (on_device) {
    staged = matrix_from_host(data->nrows, data->rowptr, data->rowind, data->rowval, base, &rc);
    if (!staged) return rc;
  }
  std::printf("------------------------------------------------------------------\n");
  std::printf("SLIM, version %s (MI355X engine)\n", SLIM_VERSION);
  std::printf("------------------------------------------------------------------\n");
  std::printf("  data matrix, nrows: %d, ncols: %d, nnz: %zd\n", data->nrows,
              max_index_plus_one(data->rowptr[data->nrows], data->rowind), data->rowptr[data->nrows]);
  std::printf("  cross-validation: %d folds, %s, ", F, sp.mode == SLIMGPU_SPLIT_LEAVE_OUT ? "leave-out" : "folds");
  if (sp.mode == SLIMGPU_SPLIT_LEAVE_OUT) std::printf("nheld: %d, ", sp.nheld);
  std::printf("minkeep: %d, seed: %llu, split on the %s\n", sp.minkeep, (unsigned long long)sp.seed,
              on_device ? "device" : "host");
  std::printf("  optTol: %.2le, niters: %d\n", base.optTol, base.maxniters);

  struct PairSums {
    double hr = 0, arhr = 0, hr_min = 0, hr_max = 0, arhr_min = 0, arhr_max = 0;
  };
  std::vector<PairSums> sums((size_t)npairs);
  *bestHRHR = *bestARHR = *bestHRAR = *bestARAR = 0.0;
  for (int32_t f = 0; f < F && rc == SLIM_OK; ++f) {
    sp.fold = f;
    // the fold's two halves and its grid; the grid owns a staged train half, the host halves are freed behind it
    slim_csr_t *h_trn = nullptr, *h_tst = nullptr;
    slimgpu_grid_t* grid = nullptr;
    if (on_device) {
      slimgpu_matrix_t* d_trn = nullptr;
      rc = matrix_split(staged, &sp, &d_trn, &h_tst);
      if (rc == SLIM_OK) {
        rc = SLIMGPU_GridOpenOn(d_trn, h_tst, ioptions, doptions, 0, npairs, filter, &grid);
        if (rc != SLIM_OK) matrix_free(d_trn);
      }
    } else {
      rc = split_host(data, sp, &h_trn, &h_tst);
      if (rc == SLIM_OK) rc = SLIMGPU_GridOpen(h_trn, h_tst, ioptions, doptions, 0, npairs, filter, &grid);
    }
    if (rc == SLIM_OK) {
      std::printf("\nfold %d of %d: %zd held-out entries\n", f, F, h_tst->rowptr[h_tst->nrows]);
      grid->describe();
      std::printf("\n");
    }
    for (int32_t p = 0; p < npairs && rc == SLIM_OK; ++p) {
      doptions[SLIM_OPTION_L1R] = pl1[p];  // (written through, as Py_SLIM_Mselect writes them)
      doptions[SLIM_OPTION_L2R] = pl2[p];
      slimgpu_grid_cell_t c;
      rc = grid->solve(pl1[p], pl2[p], &c);
      if (rc != SLIM_OK) break;
      const double hr = c.metrics[0], arhr = c.metrics[3];
      std::printf("l1r: %.2le l2r: %.2le nnz: %7zd hr: %.4f hr_head: %.4f hr_tail: %.4f "
                  "arhr: %.4f time: %.2lf\n",
                  c.l1r, c.l2r, (ssize_t)c.nnz, hr, c.metrics[1], c.metrics[2], arhr, c.solve_seconds);
      if (cells) {
        double* out = cells + (size_t)SLIMGPU_CV_CELL * ((size_t)f * (size_t)npairs + (size_t)p);
        out[0] = f; out[1] = c.l1r; out[2] = c.l2r;
        for (int k = 0; k < 4; ++k) out[3 + k] = c.metrics[k];
        for (int k = 0; k < 3; ++k) out[7 + k] = c.nvalid[k];
        out[10] = (double)c.nnz;
      }
      if (c.nvalid[0] < 1) {  // pyapi.c:377-381
        *bestl1HR = c.l1r;
        *bestl2HR = c.l2r;
        rc = SLIM_ERROR;
        break;
      }
      PairSums& s = sums[(size_t)p];
      s.hr += hr;
      s.arhr += arhr;
      s.hr_min = f ? std::min(s.hr_min, hr) : hr;
      s.hr_max = f ? std::max(s.hr_max, hr) : hr;
      s.arhr_min = f ? std::min(s.arhr_min, arhr) : arhr;
      s.arhr_max = f ? std::max(s.arhr_max, arhr) : arhr;
    }
    SLIMGPU_GridFree(&grid);
    csr_free(h_trn);
    csr_free(h_tst);
  }
  matrix_free(staged);
  if (rc == SLIM_OK) {
    std::printf("\nmeans over %d folds\n\n", F);
    for (int32_t p = 0; p < npairs; ++p) {
      const PairSums& s = sums[(size_t)p];
      const double l1 = pl1[p], l2 = pl2[p], hr = s.hr / F, arhr = s.arhr / F;
      std::printf("l1r: %.2le l2r: %.2le hr: %.4f (min %.4f max %.4f) arhr: %.4f (min %.4f max %.4f)\n", l1, l2, hr,
                  s.hr_min, s.hr_max, arhr, s.arhr_min, s.arhr_max);
      if (hr > *bestHRHR) {
        *bestHRHR = hr; *bestARHR = arhr; *bestl1HR = l1; *bestl2HR = l2;
      }
      if (arhr > *bestARAR) {
        *bestHRAR = hr; *bestARAR = arhr; *bestl1AR = l1; *bestl2AR = l2;
      }
    }
  }
  std::printf("\nDone.\n------------------------------------------------------------------\n");
  return rc;
}

int32_t Py_SLIM_MselectCV(slim_t* datahandle, int32_t* ioptions, double* doptions, double* arrayl1, double* arrayl2,
                          int32_t nl1, int32_t nl2, const slimgpu_split_t* split, slimgpu_filter_t* filter,
                          double* bestl1HR, double* bestl2HR, double* bestHRHR, double* bestARHR, double* bestl1AR,
                          double* bestl2AR, double* bestHRAR, double* bestARAR, double* cells) {
  std::vector<double> pl1, pl2;
  for (int32_t a = 0; arrayl1 && arrayl2 && a < nl1; ++a)
    for (int32_t b = 0; b < nl2; ++b) {
      pl1.push_back(arrayl1[a]);
      pl2.push_back(arrayl2[b]);
    }
  return mselect_cv_impl("Py_SLIM_MselectCV", datahandle, ioptions, doptions, (int32_t)pl1.size(), pl1.data(),
                         pl2.data(), split, filter, bestl1HR, bestl2HR, bestHRHR, bestARHR, bestl1AR, bestl2AR, bestHRAR,
                         bestARAR, cells);
}

int32_t SLIMGPU_MselectCVPairs(slim_t* datahandle, int32_t* ioptions, double* doptions, int32_t npairs,
                               const double* l1, const double* l2, const slimgpu_split_t* split,
                               slimgpu_filter_t* filter, double* best, double* cells) {
  if (!best) {
    set_error("SLIMGPU_MselectCVPairs: bad arguments (the eight outputs)");
    return SLIM_ERROR_INPUT;
  }
  return mselect_cv_impl("SLIMGPU_MselectCVPairs", datahandle, ioptions, doptions, npairs, l1, l2, split, filter,
                         best, best + 1, best + 2, best + 3, best + 4, best + 5, best + 6, best + 7, cells);
}

int32_t Py_SLIM_GetTopN(slim_t* model, int32_t nratings, int32_t* itemids, float* ratings,
                        int32_t nrcmds, int32_t* rids, float* rscores, int32_t /*dbglvl*/) {
  return SLIM_GetTopN(model, nratings, itemids, ratings, nullptr, nrcmds, rids, rscores);
}

int32_t Py_SLIM_GetTopN_1vsk(slim_t* model, int32_t nratings, int32_t* itemids, float* ratings,
                             int32_t nrcmds, int32_t* rids, float* rscores, int32_t nnegs,
                             int32_t* negitems, int32_t /*dbglvl*/) {
  const slim_csr_t* W = as_csr(model);
  if (!W || !W->rowptr || nrcmds < 0 || nnegs < 0) return SLIM_ERROR;
  return top_n_1vsk(W, nratings, itemids, ratings, nrcmds, rids, rscores, nnegs, negitems);
}

int32_t SLIMGPU_Predict(int32_t nrcmds, slim_t* slimhandle, slim_t* trnhandle, int32_t* output,
                        float* scores) {
  set_error("");
  return predict_device(as_csr(slimhandle), as_csr(trnhandle), nrcmds, output, scores, nullptr);
}

int32_t Py_SLIM_Predict(int32_t nrcmds, slim_t* slimhandle, slim_t* trnhandle, int32_t* output,
                        float* scores) {
  const slim_csr_t* W = as_csr(slimhandle);
  const slim_csr_t* trn = as_csr(trnhandle);
  if (!W || !trn || !W->rowptr || !trn->rowptr || nrcmds < 0) return SLIM_ERROR;
  const int policy = predict_policy();
  if (policy == 2 || (policy == 1 && nrcmds >= 1 && nrcmds <= SLIMGPU_MAX_LIST && trn->nrows > 0 &&
                      device_count() > 0)) {
    const int32_t rc = nrcmds > 128 ? predict_lists(W, trn, nrcmds, output, scores, nullptr)
                                    : predict_device(W, trn, nrcmds, output, scores, nullptr);
    if (rc == SLIM_OK || policy == 2) return rc;
  }
  TopNScratch ws(W->ncols > W->nrows ? W->ncols : W->nrows);
  std::vector<int32_t> rids(nrcmds);
  std::vector<float> rsc(nrcmds);
  for (int32_t u = 0; u < trn->nrows; ++u) {
    const ssize_t lo = trn->rowptr[u], hi = trn->rowptr[u + 1];
    const int32_t n = top_n(W, (int32_t)(hi - lo), trn->rowind + lo,
                            trn->rowval ? trn->rowval + lo : nullptr, nrcmds, rids.data(),
                            rsc.data(), ws);
    for (int32_t r = 0; r < n; ++r) {
      output[(ssize_t)u * nrcmds + r] = rids[r];
      scores[(ssize_t)u * nrcmds + r] = rsc[r];
    }
  }
  return trn->nrows > 0 ? SLIM_OK : SLIM_ERROR;  // nvalid < 1 => error (pyapi.c:558-562)
}

int32_t Py_SLIM_Predict_1vsk(int32_t nrcmds, int32_t nnegs, slim_t* slimhandle,
                             slim_t* trnhandle, int32_t* negitems, int32_t* output,
                             float* scores) {
  const slim_csr_t* W = as_csr(slimhandle);
  const slim_csr_t* trn = as_csr(trnhandle);
  if (!W || !trn || !W->rowptr || !trn->rowptr || nrcmds < 0 || nnegs < 0) return SLIM_ERROR;
  const int policy = predict_policy();
  // up to 1024 candidates the 1-vs-k kernel serves; above that, and at every nnegs under SLIM_1VSK_KERNEL=chunk,
  // the chunk scorer does through a candidate set with an implicit row pointer (slim_gpu_cand.h): the same
  // results bit for bit
  const char* kenv = std::getenv("SLIM_1VSK_KERNEL");
  const bool chunk = nrcmds >= 1 && nnegs >= 1 && negitems && (nnegs > 1024 || (kenv && std::strcmp(kenv, "chunk") == 0));
  if (policy == 2 || (policy == 1 && nrcmds >= 1 && nnegs >= 1 && (nnegs <= 1024 || chunk) &&
                      trn->nrows > 0 && device_count() > 0)) {
    int32_t rc;
    if (chunk) {
      set_error("");
      std::vector<int64_t> cptr((size_t)std::max(trn->nrows, 0) + 1);
      for (size_t u = 0; u < cptr.size(); ++u) cptr[u] = (int64_t)u * nnegs;
      slimgpu_candset_t* cs = candset_create(W->ncols, std::max(trn->nrows, 0), cptr.data(), negitems, &rc);
      if (cs) rc = score_candidates(W, trn, cs, nrcmds, nullptr, output, scores, nullptr);
      candset_free(cs);
    } else {
      rc = predict_1vsk_device(W, trn, nrcmds, nnegs, negitems, output, scores);
    }
    if (rc == SLIM_OK || policy == 2) return rc;  // (unsorted model rows etc.: host scorer)
  }
  std::vector<int32_t> rids(nrcmds);
  std::vector<float> rsc(nrcmds);
  for (int32_t u = 0; u < trn->nrows; ++u) {
    const ssize_t lo = trn->rowptr[u], hi = trn->rowptr[u + 1];
    const int32_t n = top_n_1vsk(W, (int32_t)(hi - lo), trn->rowind + lo,
                                 trn->rowval ? trn->rowval + lo : nullptr, nrcmds, rids.data(),
                                 rsc.data(), nnegs, negitems + (ssize_t)u * nnegs);
    for (int32_t r = 0; r < n; ++r) {
      output[(ssize_t)u * nrcmds + r] = rids[r];
      scores[(ssize_t)u * nrcmds + r] = rsc[r];
    }
  }
  return trn->nrows > 0 ? SLIM_OK : SLIM_ERROR;
}

// ------------------------------------------------------------- SLIMGPU_* ------

slimgpu_matrix_t* SLIMGPU_MatrixFromHost(int32_t nrows, const ssize_t* rowptr,
                                         const int32_t* rowind, const float* rowval,
                                         int32_t* ioptions, int32_t* r_status) {
  set_error("");
  int32_t status = SLIM_ERROR;
  slimgpu_matrix_t* m =
      multi_from_host(nrows, rowptr, rowind, rowval, decode_options(ioptions, nullptr), &status);
  if (r_status) *r_status = status;
  return m;
}

slimgpu_matrix_t* SLIMGPU_MatrixFromDevice(int32_t nrows, int32_t ncols, const int64_t* d_rowptr,
                                           const int32_t* d_rowind, const float* d_rowval,
                                           int32_t* ioptions, int32_t* r_status) {
  set_error("");
  int32_t status = SLIM_ERROR;
  slimgpu_matrix_t* m = matrix_from_device(nrows, ncols, d_rowptr, d_rowind, d_rowval,
                                           decode_options(ioptions, nullptr), &status);
  if (r_status) *r_status = status;
  return m;
}

void SLIMGPU_MatrixFree(slimgpu_matrix_t** mat) {
  if (!mat) return;
  matrix_free(*mat);
  *mat = nullptr;
}

int32_t SLIMGPU_MatrixInfo(const slimgpu_matrix_t* mat, int32_t* nrows, int32_t* ncols,
                           int64_t* nnz) {
  return matrix_info(mat, nrows, ncols, nnz);
}

int32_t SLIMGPU_MatrixGetColumnView(const slimgpu_matrix_t* mat, int64_t* colptr,
                                    int32_t* colind, float* colval, float* cnorms) {
  return matrix_get_column_view(mat, colptr, colind, colval, cnorms);
}

int32_t SLIMGPU_MatrixColumnCost(const slimgpu_matrix_t* mat, int64_t* cost) {
  return matrix_column_cost(mat, cost);
}

void SLIMGPU_MatrixExpectSolves(slimgpu_matrix_t* mat, int32_t nsolves) {
  matrix_expect_solves(mat, nsolves);
}

int32_t SLIMGPU_MatrixDevice(const slimgpu_matrix_t* mat) { return matrix_device(mat); }

int32_t SLIMGPU_MatrixGramBuildRows(slimgpu_matrix_t* mat, int32_t row_begin, int32_t row_end) {
  set_error("");
  return gram_build_rows(mat, row_begin, row_end);
}

int32_t SLIMGPU_MatrixGramView(slimgpu_matrix_t* mat, void** dptr, int64_t* ld, int32_t* nrows) {
  set_error("");
  return gram_view(mat, dptr, ld, nrows);
}

int32_t SLIMGPU_MatrixGramCommit(slimgpu_matrix_t* mat) {
  set_error("");
  return gram_commit(mat);
}

int32_t SLIMGPU_MatrixGramPlanes(slimgpu_matrix_t* mat, slimgpu_gram_planes_t* out) {
  set_error("");
  return gram_planes(mat, out);
}

slim_t* SLIMGPU_Learn(slimgpu_matrix_t* mat, int32_t* ioptions, double* doptions, slim_t* imodel,
                      int32_t* r_status) {
  set_error("");
  int32_t status = SLIM_ERROR;
  LearnOptions opt = decode_options(ioptions, doptions);
  slim_csr_t* model = nullptr;
  if (opt.algo != SLIM_ALGO_CD) {
    set_error("SLIMGPU_Learn: only algo=cd is implemented");
    status = SLIM_ERROR_INPUT;
  } else {
    model = multi_learn(mat, opt, as_csr(imodel), &status);
  }
  if (r_status) *r_status = status;
  return model;
}

slimgpu_model_t* SLIMGPU_LearnResident(slimgpu_matrix_t* mat, int32_t* ioptions, double* doptions,
                                       const slimgpu_model_t* warm, int32_t* r_status) {
  set_error("");
  int32_t status = SLIM_ERROR;
  LearnOptions opt = decode_options(ioptions, doptions);
  slimgpu_model_t* model = nullptr;
  if (opt.algo != SLIM_ALGO_CD) {
    set_error("SLIMGPU_LearnResident: only algo=cd is implemented");
    status = SLIM_ERROR_INPUT;
  } else {
    model = learn_resident(mat, opt, warm, &status);
  }
  if (r_status) *r_status = status;
  return model;
}

int64_t SLIMGPU_ModelNnz(const slimgpu_model_t* model) { return model_nnz(model); }

int32_t SLIMGPU_ModelFetchBegin(slimgpu_model_t* model) {
  set_error("");
  return model_fetch_begin(model);
}

slim_t* SLIMGPU_ModelFetch(slimgpu_model_t* model, int32_t* r_status) {
  set_error("");
  return model_fetch(model, r_status);
}

void SLIMGPU_ModelFree(slimgpu_model_t** model) {
  if (!model || !*model) return;
  model_free(*model);
  *model = nullptr;
}

int32_t SLIMGPU_ModelPredict(int32_t nrcmds, const slimgpu_model_t* model, slim_t* trnhandle,
                             int32_t* output, float* scores) {
  set_error("");
  DeviceRowView v;
  const int32_t rc = model_row_view(model, &v);
  if (rc != SLIM_OK) return rc;
  return predict_device_view(v, as_csr(trnhandle), nrcmds, output, scores, nullptr);
}

slimgpu_evalset_t* SLIMGPU_EvalSetCreateAt(slimgpu_matrix_t* mat, slim_t* tsthandle, const int32_t* fmarker,
                                           int32_t fm_ncols, int32_t ncutoffs, const int32_t* cutoffs,
                                           int32_t nusers, const int32_t* users, int32_t* r_status) {
  set_error("");
  int32_t status = SLIM_ERROR;
  slimgpu_evalset_t* es =
      evalset_create(mat, as_csr(tsthandle), fmarker, fm_ncols, ncutoffs, cutoffs, nusers, users, &status);
  if (r_status) *r_status = status;
  return es;
}

slimgpu_evalset_t* SLIMGPU_EvalSetCreate(slimgpu_matrix_t* mat, slim_t* tsthandle, const int32_t* fmarker,
                                         int32_t fm_ncols, int32_t nrcmds, int32_t* r_status) {
  return SLIMGPU_EvalSetCreateAt(mat, tsthandle, fmarker, fm_ncols, 1, &nrcmds, 0, nullptr, r_status);
}

void SLIMGPU_EvalSetFree(slimgpu_evalset_t** es) {
  if (!es || !*es) return;
  evalset_free(*es);
  *es = nullptr;
}

int32_t SLIMGPU_ModelEvaluateAt(slimgpu_evalset_t* es, const slimgpu_model_t* model, int32_t ncutoffs,
                                double* metrics, int32_t* nvalid) {
  return SLIMGPU_ModelEvaluateAtFiltered(es, model, nullptr, ncutoffs, metrics, nvalid);
}

int32_t SLIMGPU_ModelEvaluateAtFiltered(slimgpu_evalset_t* es, const slimgpu_model_t* model, slimgpu_filter_t* filter,
                                        int32_t ncutoffs, double* metrics, int32_t* nvalid) {
  set_error("");
  if (!metrics || !nvalid) return SLIM_ERROR_INPUT;
  EvalResult ev[SLIMGPU_MAX_CUTOFFS];
  if (ncutoffs < 1 || ncutoffs > SLIMGPU_MAX_CUTOFFS) {
    set_error("SLIMGPU_ModelEvaluateAt: ncutoffs must be the eval set's number of list lengths");
    return SLIM_ERROR_INPUT;
  }
  const int32_t rc = model_evaluate(es, model, ncutoffs, ev, filter);
  if (rc != SLIM_OK) return rc;
  for (int32_t k = 0; k < ncutoffs; ++k) figures_out(ev[k], metrics + 4 * k, nvalid + 3 * k);
  return SLIM_OK;
}

// the last row of SLIMGPU_ModelEvaluateAt: the longest lists of the eval set
int32_t SLIMGPU_ModelEvaluate(slimgpu_evalset_t* es, const slimgpu_model_t* model, double* metrics,
                              int32_t* nvalid) {
  set_error("");
  if (!metrics || !nvalid) return SLIM_ERROR_INPUT;
  EvalResult ev[SLIMGPU_MAX_CUTOFFS];
  const int32_t ncut = std::max(1, evalset_cutoffs(es));
  const int32_t rc = model_evaluate(es, model, ncut, ev);
  if (rc != SLIM_OK) return rc;
  figures_out(ev[ncut - 1], metrics, nvalid);
  return SLIM_OK;
}

// ---------------------------------------------------- slim_gpu_rank.h ------

slimgpu_evalset_t* SLIMGPU_EvalSetCreateRanked(slimgpu_matrix_t* mat, slim_t* tsthandle, const int32_t* fmarker,
                                               int32_t fm_ncols, int32_t nusers, const int32_t* users,
                                               int32_t* r_status) {
  set_error("");
  int32_t status = SLIM_ERROR;
  slimgpu_evalset_t* es = evalset_create_ranked(mat, as_csr(tsthandle), fmarker, fm_ncols, nusers, users, &status);
  if (r_status) *r_status = status;
  return es;
}

int64_t SLIMGPU_EvalSetEntries(const slimgpu_evalset_t* es) { return evalset_entries(es); }

int32_t SLIMGPU_ModelRanks(slimgpu_evalset_t* es, const slimgpu_model_t* model, int32_t* ranks, float* scores) {
  set_error("");
  return model_ranks(es, model, ranks, scores);
}

int32_t SLIMGPU_ModelRanksFiltered(slimgpu_evalset_t* es, const slimgpu_model_t* model, slimgpu_filter_t* filter,
                                   int32_t* ranks, float* scores) {
  set_error("");
  return model_ranks(es, model, ranks, scores, filter);
}

int32_t SLIMGPU_ModelEvaluateRanked(slimgpu_evalset_t* es, const slimgpu_model_t* model, int32_t ncutoffs,
                                    const int32_t* cutoffs, double* metrics, int32_t* nvalid) {
  return SLIMGPU_ModelEvaluateRankedFiltered(es, model, nullptr, ncutoffs, cutoffs, metrics, nvalid);
}

int32_t SLIMGPU_ModelEvaluateRankedFiltered(slimgpu_evalset_t* es, const slimgpu_model_t* model,
                                            slimgpu_filter_t* filter, int32_t ncutoffs, const int32_t* cutoffs,
                                            double* metrics, int32_t* nvalid) {
  set_error("");
  if (!metrics || !nvalid) return SLIM_ERROR_INPUT;
  EvalResult ev[SLIMGPU_MAX_RANK_CUTOFFS];
  const int32_t rc = model_evaluate_ranked(es, model, ncutoffs, cutoffs, ev, filter);
  if (rc != SLIM_OK) return rc;
  for (int32_t k = 0; k < ncutoffs; ++k) figures_out(ev[k], metrics + 4 * k, nvalid + 3 * k);
  return SLIM_OK;
}

slimgpu_model_t* SLIMGPU_ModelFromHost(slimgpu_matrix_t* mat, slim_t* model, int32_t* r_status) {
  set_error("");
  int32_t status = SLIM_ERROR;
  slimgpu_model_t* dm = model_from_host(mat, as_csr(model), &status);
  if (r_status) *r_status = status;
  return dm;
}

double SLIMGPU_LastRankPrepassMs(void) { return last_rank_prepass_ms(); }

int32_t SLIMGPU_MatrixPredict(int32_t nrcmds, const slimgpu_model_t* model, slimgpu_matrix_t* mat,
                              int32_t* output, float* scores) {
  set_error("");
  return matrix_predict(nrcmds, model, mat, output, scores);
}

// ---------------------------------------------------- slim_gpu_lists.h ------

int32_t SLIMGPU_PredictLists(int32_t nrcmds, slim_t* model, slim_t* trn, int32_t* output, float* scores,
                             int32_t* counts) {
  set_error("");
  return predict_lists(as_csr(model), as_csr(trn), nrcmds, output, scores, counts);
}

int32_t SLIMGPU_ModelPredictLists(int32_t nrcmds, const slimgpu_model_t* model, slim_t* trn, int32_t* output,
                                  float* scores, int32_t* counts) {
  set_error("");
  DeviceRowView v;
  if (!model || nrcmds < 1 || nrcmds > SLIMGPU_MAX_LIST || model_row_view(model, &v) != SLIM_OK) {
    set_error("SLIMGPU_ModelPredictLists: bad arguments (a resident model with a row view, 1 <= nrcmds <= " +
              std::to_string(SLIMGPU_MAX_LIST) + ")");
    return SLIM_ERROR_INPUT;
  }
  return predict_lists_view(v, as_csr(trn), nrcmds, output, scores, counts);
}

int32_t SLIMGPU_MatrixPredictLists(int32_t nrcmds, const slimgpu_model_t* model, slimgpu_matrix_t* mat,
                                   int32_t nusers, const int32_t* users, int32_t* output, float* scores,
                                   int32_t* counts) {
  set_error("");
  return matrix_predict_lists(nrcmds, model, mat, nusers, users, output, scores, counts);
}

// --------------------------------------------------- slim_gpu_filter.h ------

int32_t SLIMGPU_FilterCreate(int32_t ncols, int32_t nitems, const int32_t* items, int32_t blocked, int32_t xusers,
                             const int64_t* xptr, const int32_t* xind, slimgpu_filter_t** out) {
  set_error("");
  if (!out) {
    set_error("SLIMGPU_FilterCreate: bad arguments (out is NULL)");
    return SLIM_ERROR_INPUT;
  }
  int32_t status = SLIM_ERROR;
  *out = filter_create(ncols, nitems, items, blocked, xusers, xptr, xind, &status);
  return status;
}

void SLIMGPU_FilterFree(slimgpu_filter_t* f) { filter_free(f); }

int32_t SLIMGPU_PredictListsFiltered(int32_t nrcmds, slim_t* model, slim_t* trn, slimgpu_filter_t* filter,
                                     int32_t* output, float* scores, int32_t* counts) {
  set_error("");
  return predict_lists(as_csr(model), as_csr(trn), nrcmds, output, scores, counts, filter);
}

int32_t SLIMGPU_ModelPredictListsFiltered(int32_t nrcmds, const slimgpu_model_t* model, slim_t* trn,
                                          slimgpu_filter_t* filter, int32_t* output, float* scores, int32_t* counts) {
  set_error("");
  DeviceRowView v;
  if (!model || nrcmds < 1 || nrcmds > SLIMGPU_MAX_LIST || model_row_view(model, &v) != SLIM_OK) {
    set_error("SLIMGPU_ModelPredictListsFiltered: bad arguments (a resident model with a row view, 1 <= nrcmds <= " +
              std::to_string(SLIMGPU_MAX_LIST) + ")");
    return SLIM_ERROR_INPUT;
  }
  return predict_lists_view(v, as_csr(trn), nrcmds, output, scores, counts, filter);
}

int32_t SLIMGPU_MatrixPredictListsFiltered(int32_t nrcmds, const slimgpu_model_t* model, slimgpu_matrix_t* mat,
                                           int32_t nusers, const int32_t* users, slimgpu_filter_t* filter,
                                           int32_t* output, float* scores, int32_t* counts) {
  set_error("");
  return matrix_predict_lists(nrcmds, model, mat, nusers, users, output, scores, counts, filter);
}

// Py_SLIM_Predict under a filter: the same policy, the device scorer at every length it serves
int32_t Py_SLIM_PredictFiltered(int32_t nrcmds, slim_t* slimhandle, slim_t* trnhandle, slimgpu_filter_t* filter,
                                int32_t* output, float* scores) {
  const slim_csr_t* W = as_csr(slimhandle);
  const slim_csr_t* trn = as_csr(trnhandle);
  if (!W || !trn || !W->rowptr || !trn->rowptr || nrcmds < 0) return SLIM_ERROR;
  set_error("");
  if (const int32_t rc = filter_check("Py_SLIM_PredictFiltered", filter, W->ncols); rc != SLIM_OK) return rc;
  const int policy = predict_policy();
  if (policy == 2 || (policy == 1 && nrcmds >= 1 && nrcmds <= SLIMGPU_MAX_LIST && trn->nrows > 0 &&
                      device_count() > 0)) {
    const int32_t rc = predict_lists(W, trn, nrcmds, output, scores, nullptr, filter);
    if (rc == SLIM_OK || policy == 2) return rc;
  }
  const HostFilter F = filter_host(filter);
  TopNScratch ws(W->ncols > W->nrows ? W->ncols : W->nrows);
  std::vector<int32_t> rids(nrcmds);
  std::vector<float> rsc(nrcmds);
  for (int32_t u = 0; u < trn->nrows; ++u) {
    const ssize_t lo = trn->rowptr[u], hi = trn->rowptr[u + 1];
    const int32_t n = top_n_filtered(W, (int32_t)(hi - lo), trn->rowind + lo, trn->rowval ? trn->rowval + lo : nullptr,
                                     nrcmds, rids.data(), rsc.data(), ws, F, u);
    for (int32_t r = 0; r < n; ++r) {
      output[(ssize_t)u * nrcmds + r] = rids[r];
      scores[(ssize_t)u * nrcmds + r] = rsc[r];
    }
  }
  return trn->nrows > 0 ? SLIM_OK : SLIM_ERROR;
}

// ----------------------------------------------------- slim_gpu_cand.h ------

int32_t SLIMGPU_CandSetCreate(int32_t ncols, int32_t nusers, const int64_t* cptr, const int32_t* cind,
                              slimgpu_candset_t** out) {
  set_error("");
  if (!out) {
    set_error("SLIMGPU_CandSetCreate: bad arguments (out is NULL)");
    return SLIM_ERROR_INPUT;
  }
  int32_t status = SLIM_ERROR;
  *out = candset_create(ncols, nusers, cptr, cind, &status);
  return status;
}

void SLIMGPU_CandSetFree(slimgpu_candset_t* cs) { candset_free(cs); }

int32_t SLIMGPU_ScoreCandidates(slim_t* model, slim_t* trn, slimgpu_candset_t* cs, int32_t nrcmds, float* slot_scores,
                                int32_t* output, float* scores, int32_t* counts) {
  set_error("");
  return score_candidates(as_csr(model), as_csr(trn), cs, nrcmds, slot_scores, output, scores, counts);
}

int32_t SLIMGPU_MatrixScoreCandidates(const slimgpu_model_t* model, slimgpu_matrix_t* mat, slimgpu_candset_t* cs,
                                      int32_t nusers, const int32_t* users, int32_t nrcmds, float* slot_scores,
                                      int32_t* output, float* scores, int32_t* counts) {
  set_error("");
  return matrix_score_candidates(model, mat, cs, nusers, users, nrcmds, slot_scores, output, scores, counts);
}

int32_t SLIMGPU_ModelEvaluateCandidates(slimgpu_evalset_t* es, const slimgpu_model_t* model, slimgpu_candset_t* cs,
                                        int32_t ncutoffs, double* metrics, int32_t* nvalid) {
  set_error("");
  if (!metrics || !nvalid) return SLIM_ERROR_INPUT;
  EvalResult ev[SLIMGPU_MAX_CUTOFFS];
  if (ncutoffs < 1 || ncutoffs > SLIMGPU_MAX_CUTOFFS) {
    set_error("SLIMGPU_ModelEvaluateCandidates: ncutoffs must be the eval set's number of list lengths");
    return SLIM_ERROR_INPUT;
  }
  const int32_t rc = model_evaluate_candidates(es, model, cs, ncutoffs, ev);
  if (rc != SLIM_OK) return rc;
  for (int32_t k = 0; k < ncutoffs; ++k) figures_out(ev[k], metrics + 4 * k, nvalid + 3 * k);
  return SLIM_OK;
}

// the policy of Py_SLIM_Predict: the device scorer under gpu and, with a device, under auto; the host loop under
// cpu and, under auto, where the device refuses.  Both give the same scores and lists.
int32_t Py_SLIM_ScoreCandidates(slim_t* model, slim_t* trnhandle, slimgpu_candset_t* cs, int32_t nrcmds,
                                float* slot_scores, int32_t* output, float* scores, int32_t* counts) {
  const slim_csr_t* W = as_csr(model);
  const slim_csr_t* trn = as_csr(trnhandle);
  if (!W || !trn || !W->rowptr || !trn->rowptr) return SLIM_ERROR;
  set_error("");
  if (const int32_t rc = candset_check("Py_SLIM_ScoreCandidates", cs, W->ncols, trn->nrows, nullptr, nrcmds, output,
                                       scores);
      rc != SLIM_OK)
    return rc;
  const int policy = predict_policy();
  if (policy == 2 || (policy == 1 && trn->nrows > 0 && device_count() > 0)) {
    const int32_t rc = score_candidates(W, trn, cs, nrcmds, slot_scores, output, scores, counts);
    if (rc == SLIM_OK || policy == 2) return rc;
  }
  if (W->rowptr[W->nrows] > 0 && !W->rowval) return SLIM_ERROR;
  // (a set born on the device brings its ids down on first need, as SLIMGPU_CandSetRows does)
  if (const int32_t rc = candset_fetch_ids("Py_SLIM_ScoreCandidates", cs); rc != SLIM_OK) return rc;
  score_candidates_host(W, trn, candset_host(cs), nrcmds, slot_scores, output, scores, counts);
  return SLIM_OK;
}

// -------------------------------------------------- slim_gpu_explain.h ------

int32_t SLIMGPU_ExplainCandidates(slim_t* model, slim_t* trn, slimgpu_candset_t* cs, int32_t nwhy, int32_t* why_items,
                                  float* why_terms, int32_t* support) {
  set_error("");
  return explain_candidates(as_csr(model), as_csr(trn), cs, nwhy, why_items, why_terms, support);
}

int32_t SLIMGPU_MatrixExplainCandidates(const slimgpu_model_t* model, slimgpu_matrix_t* mat, slimgpu_candset_t* cs,
                                        int32_t nusers, const int32_t* users, int32_t nwhy, int32_t* why_items,
                                        float* why_terms, int32_t* support) {
  set_error("");
  return matrix_explain_candidates(model, mat, cs, nusers, users, nwhy, why_items, why_terms, support);
}

// the policy of Py_SLIM_ScoreCandidates; both sides give the same explanations
int32_t Py_SLIM_ExplainCandidates(slim_t* model, slim_t* trnhandle, slimgpu_candset_t* cs, int32_t nwhy,
                                  int32_t* why_items, float* why_terms, int32_t* support) {
  const char* who = "Py_SLIM_ExplainCandidates";
  const slim_csr_t* W = as_csr(model);
  const slim_csr_t* trn = as_csr(trnhandle);
  if (!W || !trn || !W->rowptr || !trn->rowptr) return SLIM_ERROR;
  set_error("");
  if (const int32_t rc = explain_check(who, nwhy, why_items, why_terms); rc != SLIM_OK) return rc;
  if (const int32_t rc = candset_check(who, cs, W->ncols, trn->nrows, nullptr, 0, nullptr, nullptr); rc != SLIM_OK)
    return rc;
  const int policy = predict_policy();
  if (policy == 2 || (policy == 1 && trn->nrows > 0 && device_count() > 0)) {
    const int32_t rc = explain_candidates(W, trn, cs, nwhy, why_items, why_terms, support);
    if (rc == SLIM_OK || policy == 2) return rc;
  }
  if (W->rowptr[W->nrows] > 0 && !W->rowval) return SLIM_ERROR;
  if (const int32_t rc = candset_fetch_ids(who, cs); rc != SLIM_OK) return rc;
  explain_candidates_host(W, trn, candset_host(cs), nwhy, why_items, why_terms, support);
  return SLIM_OK;
}

// ------------------------------------------------- slim_gpu_exposure.h ------

int32_t SLIMGPU_ListExposure(int32_t ncols, const uint32_t* pop, const int32_t* fmarker, int32_t fm_ncols,
                             int64_t nlists, int32_t nrcmds, const int32_t* ids, const int32_t* counts,
                             int32_t ncutoffs, const int32_t* cutoffs, uint32_t* exposure,
                             slimgpu_exposure_t* summary) {
  const char* who = "SLIMGPU_ListExposure";
  set_error("");
  if (const int32_t rc = exposure_lists_check(who, ncols, nlists, nrcmds, ids, counts, ncutoffs, cutoffs);
      rc != SLIM_OK)
    return rc;
  if (fmarker && fm_ncols < 0) {
    set_error(std::string(who) + ": fm_ncols must be at least 0");
    return SLIM_ERROR_INPUT;
  }
  try {
    std::vector<uint32_t> own;
    uint32_t* E = exposure;
    if (!E) {
      own.resize((size_t)ncutoffs * (size_t)ncols);
      E = own.data();
    }
    int64_t outside[SLIMGPU_MAX_CUTOFFS];
    list_exposure_host(ncols, nlists, nrcmds, ids, counts, ncutoffs, cutoffs, E, outside);
    for (int32_t k = 0; summary && k < ncutoffs; ++k)
      exposure_summary(ncols, pop, fmarker, fm_ncols, nlists, E + (size_t)k * (size_t)ncols, outside[k], &summary[k]);
    return SLIM_OK;
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return SLIM_ERROR_MEMORY;
  }
}

int32_t SLIMGPU_MatrixListExposure(slimgpu_matrix_t* mat, const int32_t* fmarker, int32_t fm_ncols, int64_t nlists,
                                   int32_t nrcmds, const int32_t* ids, const int32_t* counts, int32_t ncutoffs,
                                   const int32_t* cutoffs, uint32_t* exposure, slimgpu_exposure_t* summary) {
  set_error("");
  return matrix_list_exposure(mat, fmarker, fm_ncols, nlists, nrcmds, ids, counts, ncutoffs, cutoffs, exposure, summary);
}

int32_t SLIMGPU_MatrixPredictExposure(slimgpu_matrix_t* mat, const slimgpu_model_t* model, int32_t nrcmds,
                                      int32_t nusers, const int32_t* users, slimgpu_filter_t* filter,
                                      const int32_t* fmarker, int32_t fm_ncols, int32_t ncutoffs,
                                      const int32_t* cutoffs, uint32_t* exposure, slimgpu_exposure_t* summary) {
  set_error("");
  return matrix_predict_exposure(mat, model, nrcmds, nusers, users, filter, fmarker, fm_ncols, ncutoffs, cutoffs,
                                 exposure, summary);
}

int32_t SLIMGPU_ModelEvaluateExposure(slimgpu_evalset_t* es, const slimgpu_model_t* model, slimgpu_filter_t* filter,
                                      int32_t ncutoffs, double* metrics, int32_t* nvalid, uint32_t* exposure,
                                      slimgpu_exposure_t* summary) {
  set_error("");
  if (!metrics || !nvalid) return SLIM_ERROR_INPUT;
  EvalResult ev[SLIMGPU_MAX_CUTOFFS];
  if (ncutoffs < 1 || ncutoffs > SLIMGPU_MAX_CUTOFFS) {
    set_error("SLIMGPU_ModelEvaluateExposure: ncutoffs must be the eval set's number of list lengths");
    return SLIM_ERROR_INPUT;
  }
  const int32_t rc = model_evaluate_exposure(es, model, filter, ncutoffs, ev, exposure, summary);
  if (rc != SLIM_OK) return rc;
  for (int32_t k = 0; k < ncutoffs; ++k) figures_out(ev[k], metrics + 4 * k, nvalid + 3 * k);
  return SLIM_OK;
}

// --------------------------------------------------- slim_gpu_groups.h ------

int32_t SLIMGPU_EvalSetSetGroups(slimgpu_evalset_t* es, int32_t ngroups, const int32_t* group_of_user) {
  set_error("");
  return evalset_set_groups(es, ngroups, group_of_user);
}

int32_t SLIMGPU_EvalSetSetHistoryBands(slimgpu_evalset_t* es, int32_t nbounds, const int32_t* bounds) {
  set_error("");
  return evalset_set_history_bands(es, nbounds, bounds);
}

void SLIMGPU_EvalSetClearGroups(slimgpu_evalset_t* es) { evalset_clear_groups(es); }

int32_t SLIMGPU_EvalSetGroupInfo(const slimgpu_evalset_t* es, int32_t* ngroups, int32_t* members) {
  set_error("");
  return evalset_group_info(es, ngroups, members);
}

int32_t SLIMGPU_EvalSetLastGroupFigures(slimgpu_evalset_t* es, int32_t ncutoffs, double* metrics, int32_t* nvalid) {
  set_error("");
  if (!metrics || !nvalid) {
    set_error("SLIMGPU_EvalSetLastGroupFigures: bad arguments (an eval set, the outputs)");
    return SLIM_ERROR_INPUT;
  }
  try {
    // (sized for a number of cutoffs in range: any other differs from the evaluation's and is refused unwritten)
    const int32_t ncut = std::min(std::max(ncutoffs, 1), SLIMGPU_MAX_RANK_CUTOFFS);
    std::vector<EvalResult> rows(((size_t)evalset_groups(es) + 1) * (size_t)ncut);
    if (const int32_t rc = evalset_group_figures(es, ncutoffs, rows.data()); rc != SLIM_OK) return rc;
    for (size_t r = 0; r < rows.size(); ++r) figures_out(rows[r], metrics + 4 * r, nvalid + 3 * r);
    return SLIM_OK;
  } catch (const std::bad_alloc&) {
    set_error("SLIMGPU_EvalSetLastGroupFigures: out of host memory");
    return SLIM_ERROR_MEMORY;
  }
}

int32_t SLIMGPU_GroupPartition(int32_t nsel, const int32_t* users, int32_t nall, int32_t ngroups,
                               const int32_t* group_of_user, int32_t* order, int64_t* offsets) {
  set_error("");
  return group_partition("SLIMGPU_GroupPartition", nsel, users, nall, ngroups, group_of_user, order, offsets);
}

// --------------------------------------------------- slim_gpu_sample.h ------

int32_t SLIMGPU_EvalSetSampleCandidates(slimgpu_evalset_t* es, int32_t nnegs, uint64_t seed,
                                        slimgpu_candset_t** out) {
  set_error("");
  if (!out) {
    set_error("SLIMGPU_EvalSetSampleCandidates: bad arguments (out is NULL)");
    return SLIM_ERROR_INPUT;
  }
  int32_t status = SLIM_ERROR;
  slimgpu_candset_t* cs = evalset_sample_candidates(es, nnegs, seed, &status);
  if (cs) *out = cs;
  return status;
}

extern "C++" {
namespace {
// SLIMGPU_CandSetSample and its weighted form: one check, one host sampler
int32_t candset_sample(const std::string& who, int32_t ncols, slim_t* trnhandle, slim_t* tsthandle, int32_t nusers,
                       const int32_t* users, int32_t nnegs, uint64_t seed, bool weighted, const uint32_t* weights,
                       slimgpu_candset_t** out) {
  set_error("");
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return SLIM_ERROR_INPUT;
  };
  const slim_csr_t* trn = as_csr(trnhandle);
  const slim_csr_t* tst = as_csr(tsthandle);
  if (!out || !trn || !tst || !trn->rowptr || !tst->rowptr) return bad("bad arguments (a history, test rows, out)");
  if (ncols < 1) return bad("ncols must be at least 1, not " + std::to_string(ncols));
  if (nnegs < 1) return bad("nnegs must be at least 1, not " + std::to_string(nnegs));
  const int32_t nall = std::min(trn->nrows, tst->nrows);
  if (users ? nusers < 1 : nusers != 0)
    return bad(users ? "a user list needs at least one user" : "nusers must be 0 without a user list");
  for (int32_t q = 0; q < nusers; ++q) {
    if (users[q] < 0 || users[q] >= nall)
      return bad("user " + std::to_string(users[q]) + " is outside [0, " + std::to_string(nall) + ")");
    if (q > 0 && users[q] <= users[q - 1]) return bad("the user ids must ascend strictly");
  }
  int64_t max_test = 0;
  for (int32_t q = 0, n = users ? nusers : nall; q < n; ++q) {
    const int32_t u = users ? users[q] : q;
    max_test = std::max<int64_t>(max_test, tst->rowptr[u + 1] - tst->rowptr[u]);
  }
  if ((int64_t)nnegs + max_test > SLIMGPU_MAX_LIST)
    return bad("nnegs " + std::to_string(nnegs) + " and the longest selected test row, " + std::to_string(max_test) +
               " entries, give a candidate row above " + std::to_string(SLIMGPU_MAX_LIST) +
               ": the evaluation needs lists");
  try {
    std::vector<uint64_t> wC;  // the weighted rule's prefix table; NULL weights: the popularity of trn's rows
    if (weighted) {
      wC.assign((size_t)ncols + 1, 0);
      if (weights) {
        for (int32_t i = 0; i < ncols; ++i) wC[(size_t)i + 1] = weights[i];
      } else {
        for (ssize_t k = 0; k < trn->rowptr[trn->nrows]; ++k)
          if (trn->rowind[k] >= 0 && trn->rowind[k] < ncols) ++wC[(size_t)trn->rowind[k] + 1];
      }
      for (int32_t i = 0; i < ncols; ++i) wC[(size_t)i + 1] += wC[i];
      if (wC[ncols] == 0) return bad("the weights sum to 0 (T = 0): nothing can be drawn");
    }
    std::vector<int64_t> cptr;
    std::vector<int32_t> cind;
    sample_candidates_host(ncols, trn, tst, nusers, users, nnegs, seed, cptr, cind, weighted ? wC.data() : nullptr);
    cind.push_back(0);  // (an empty set still has an address)
    int32_t status = SLIM_ERROR;
    slimgpu_candset_t* cs = candset_create(ncols, nall, cptr.data(), cind.data(), &status);
    if (cs) *out = cs;
    return status;
  } catch (const std::bad_alloc&) {
    set_error(who + "out of host memory");
    return SLIM_ERROR_MEMORY;
  }
}
}  // namespace
}  // extern "C++"

int32_t SLIMGPU_CandSetSample(int32_t ncols, slim_t* trnhandle, slim_t* tsthandle, int32_t nusers,
                              const int32_t* users, int32_t nnegs, uint64_t seed, slimgpu_candset_t** out) {
  return candset_sample("SLIMGPU_CandSetSample: ", ncols, trnhandle, tsthandle, nusers, users, nnegs, seed, false,
                        nullptr, out);
}

int32_t SLIMGPU_CandSetSampleWeighted(int32_t ncols, slim_t* trnhandle, slim_t* tsthandle, int32_t nusers,
                                      const int32_t* users, int32_t nnegs, uint64_t seed, const uint32_t* weights,
                                      slimgpu_candset_t** out) {
  return candset_sample("SLIMGPU_CandSetSampleWeighted: ", ncols, trnhandle, tsthandle, nusers, users, nnegs, seed,
                        true, weights, out);
}

int32_t SLIMGPU_EvalSetSampleCandidatesWeighted(slimgpu_evalset_t* es, int32_t nnegs, uint64_t seed,
                                                const uint32_t* weights, slimgpu_candset_t** out) {
  set_error("");
  if (!out) {
    set_error("SLIMGPU_EvalSetSampleCandidatesWeighted: bad arguments (out is NULL)");
    return SLIM_ERROR_INPUT;
  }
  int32_t status = SLIM_ERROR;
  slimgpu_candset_t* cs = evalset_sample_candidates_weighted(es, nnegs, seed, weights, &status);
  if (cs) *out = cs;
  return status;
}

double SLIMGPU_LastSampleKernelMs(void) { return last_weighted_sample_kernel_ms(); }

int32_t SLIMGPU_CandSetRows(slimgpu_candset_t* cs, int64_t* cptr, int32_t* cind) {
  set_error("");
  return candset_rows(cs, cptr, cind);
}

int32_t SLIMGPU_CandSetInfo(slimgpu_candset_t* cs, int32_t* nrows, int32_t* ncols, int64_t* entries) {
  set_error("");
  return candset_info(cs, nrows, ncols, entries);
}

int32_t SLIMGPU_LastListStats(slimgpu_list_stats_t* out) {
  if (!out) return SLIM_ERROR_INPUT;
  *out = last_list_stats();
  return SLIM_OK;
}

int32_t SLIMGPU_LastEvalStats(slimgpu_eval_stats_t* out) {
  if (!out) return SLIM_ERROR_INPUT;
  *out = last_eval_stats();
  return SLIM_OK;
}

slim_t* SLIMGPU_LearnColumns(slimgpu_matrix_t* mat, int32_t ncolumns, const int32_t* columns,
                             int32_t* ioptions, double* doptions, slim_t* imodel,
                             int32_t* r_status) {
  set_error("");
  int32_t status = SLIM_ERROR;
  LearnOptions opt = decode_options(ioptions, doptions);
  slim_csr_t* model = nullptr;
  if (opt.algo != SLIM_ALGO_CD || ncolumns < 0 || (ncolumns > 0 && !columns)) {
    set_error("SLIMGPU_LearnColumns: algo must be cd and the column list non-null");
    status = SLIM_ERROR_INPUT;
  } else {
    static const int32_t none = 0;
    model = multi_learn(mat, opt, as_csr(imodel), &status, columns ? columns : &none, ncolumns);
  }
  if (r_status) *r_status = status;
  return model;
}

int32_t SLIMGPU_Predict1vsK(int32_t nrcmds, int32_t nnegs, slim_t* slimhandle, slim_t* trnhandle,
                            int32_t* negitems, int32_t* output, float* scores) {
  set_error("");
  return predict_1vsk_device(as_csr(slimhandle), as_csr(trnhandle), nrcmds, nnegs, negitems, output,
                             scores);
}

int32_t SLIMGPU_Evaluate(int32_t nusers, int32_t nrcmds, const int32_t* lists,
                         const int32_t* counts, slim_t* tsthandle, const int32_t* fmarker,
                         int32_t fm_ncols, double* metrics, int32_t* nvalid) {
  set_error("");
  if (!metrics || !nvalid) return SLIM_ERROR_INPUT;
  EvalResult ev;
  const int32_t rc =
      evaluate_device(nusers, nrcmds, lists, counts, as_csr(tsthandle), fmarker, fm_ncols, &ev);
  if (rc != SLIM_OK) return rc;
  figures_out(ev, metrics, nvalid);
  return SLIM_OK;
}

int32_t SLIMGPU_LastStats(slimgpu_stats_t* out) {
  if (!out) return SLIM_ERROR_INPUT;
  *out = last_stats();
  return SLIM_OK;
}

int32_t SLIMGPU_LastColumnStats(int32_t ncols, int32_t* nacols, int32_t* sweeps, int32_t* conv,
                                int64_t* G, int64_t* D, int64_t* U) {
  const ColumnStats& cs = last_column_stats();
  if ((size_t)ncols > cs.nacols.size()) return SLIM_ERROR_INPUT;
  const size_t n = (size_t)ncols;
  if (nacols) std::memcpy(nacols, cs.nacols.data(), sizeof(int32_t) * n);
  if (sweeps) std::memcpy(sweeps, cs.sweeps.data(), sizeof(int32_t) * n);
  if (conv) std::memcpy(conv, cs.conv.data(), sizeof(int32_t) * n);
  if (G) std::memcpy(G, cs.G.data(), sizeof(int64_t) * n);
  if (D) std::memcpy(D, cs.D.data(), sizeof(int64_t) * n);
  if (U) std::memcpy(U, cs.U.data(), sizeof(int64_t) * n);
  return SLIM_OK;
}

int32_t SLIMGPU_DeviceCount(void) { return device_count(); }

const char* SLIMGPU_LastError(void) { return last_error(); }

}  // extern "C"
