// slim_mselect -- model selection over the (l1, l2) pairs of an l12 file, warm-starting
// every model from the previous one; R is staged in HBM once for the whole grid.
// Usage and options as /root/reference/src/programs/slim_mselect.c and cmdline_mselect.c
// (slim_mselect [options] train-file test-file l12-file).
#include "cli_common.hpp"
using namespace slimcli;

int main(int argc, char** argv) {
  std::vector<OptSpec> specs = {
      {"ifmt", true},    {"binarize", false}, {"optTol", true},  {"niters", true},
      {"nnbrs", true},   {"simtype", true},   {"algo", true},    {"nthreads", true},
      {"nrcmds", true},  {"dbglvl", true},    {"nomodels", false}, {"ngpus", true},
      {"evalstride", true}, {"evalnegs", true}, {"evalseed", true}, {"evalnegpop", false}, {"evalexposure", false}, {"gpukernel", true}, {"help", false}};
  specs.insert(specs.end(), std::begin(kFilterSpecs), std::end(kFilterSpecs));
  Args a = parse_args(argc, argv, specs);
  if (a.has("help") || a.pos.size() != 3) {
    std::printf("\n Usage: slim_mselect [options] train-file test-file l12-file\n"
                "   -ifmt=csr|csrnv|cluto|ijv  -binarize  -optTol=f  -niters=i  -nnbrs=i  -simtype=s\n"
                "   -nrcmds=i  -nthreads=i  -dbglvl=i  -nomodels (do not write '<l1 l2>.model' files)\n"
                "   -ngpus=i   (engine extension: R replicated on i GPUs, every model sharded over them)\n"
                "   -evalstride=i  (engine extension: evaluate users 0, i, 2i, ... only; needs the evaluation in HBM)\n"
                "   -evalnegs=i -evalseed=i  (engine extension: evaluate 1-vs-k on i sampled negatives per user, drawn on\n"
                "   the device with that seed (default 1); needs the evaluation in HBM, nrcmds <= 128 and no filter)\n"
                "   -evalnegpop  (with -evalnegs: draw the negatives in proportion to item popularity, not uniformly)\n"
                "   -evalexposure  (engine extension: one more line per pair on what its lists show -- coverage, tail share,\n"
                "   Gini, mean popularity, counted on the device; needs the evaluation in HBM, nrcmds <= 128, no -evalnegs)\n"
                "   (-nrcmds above 128 is evaluated in HBM from the ranks of the held-out items: no lists are formed)\n"
                "   -gpukernel=i  (engine extension: slimgpu_kernel_et, 0 = the engine's choice; 6 = FSLIM in item space)\n"
                "%s   (engine extension: every pair is evaluated under the filter; a held-out item it removes is a miss;\n"
                "   needs the evaluation in HBM)\n\n",
                kFilterUsage);
    return 0;
  }
  const Fmt fmt = parse_fmt(a.str("ifmt", "csr"));
  for (const auto& p : a.pos)
    if (!file_exists(p)) die("Input file " + p + " does not exist.");
  const int nrcmds = a.integer("nrcmds", 10);
  const int stride = a.integer("evalstride", 1);
  if (stride < 1) die("Invalid -evalstride of " + a.str("evalstride", "") + ".");
  const int evalnegs = a.integer("evalnegs", 0);
  const long long evalseed = a.has("evalseed") ? std::atoll(a.str("evalseed", "1").c_str()) : 1;
  if (evalnegs < 0) die("Invalid -evalnegs of " + a.str("evalnegs", "") + ".");
  if (evalseed < 0 || evalseed > 0xFFFFFFFFll) die("Invalid -evalseed of " + a.str("evalseed", "") + ".");
  const bool evalnegpop = a.has("evalnegpop");
  if (evalnegpop && evalnegs < 1) die("-evalnegpop weights the sampled negatives: it needs -evalnegs.");
  const bool evalexposure = a.has("evalexposure");
  if (evalexposure && evalnegs > 0) die("-evalexposure does not combine with -evalnegs: the exposure of sampled lists is not built.");
  if (evalexposure && (nrcmds < 1 || nrcmds > 128))
    die("-evalexposure needs lists of 1 to 128 places (the lists behind the evaluation), not " + std::to_string(nrcmds) + ".");
  const bool filtered = filter_options(a);
  filter_files_exist(a);
  if (evalnegs > 0 && filtered) die("-evalnegs takes no item filter: candidate rows are scored as they are.");
  if (evalnegs > 0 && nrcmds > 128)
    die("-evalnegs needs nrcmds <= 128 (the candidate lists use the eval set's cutoffs), not " + std::to_string(nrcmds) + ".");
  Csr trn = read_matrix(a.pos[0], fmt), tst = read_matrix(a.pos[1], fmt);
  if (a.has("binarize")) trn.has_val = false;
  const std::string sim = a.str("simtype", "cos");
  banner();
  std::printf("  trnfile: %s, nrows: %d, ncols: %d, nnz: %zd\n", a.pos[0].c_str(), trn.nrows, trn.ncols, trn.nnz());
  std::printf("  tstfile: %s, nrows: %d, ncols: %d, nnz: %zd\n", a.pos[1].c_str(), tst.nrows, tst.ncols, tst.nnz());
  std::printf("  l12file: %s\n", a.pos[2].c_str());

  int32_t io[SLIM_NOPTIONS];
  double dopt[SLIM_NOPTIONS];
  SLIM_iSetDefaults(io);
  SLIM_dSetDefaults(dopt);
  io[SLIM_OPTION_DBGLVL] = a.integer("dbglvl", 0);
  io[SLIM_OPTION_NNBRS] = a.integer("nnbrs", 0);
  io[SLIM_OPTION_SIMTYPE] = sim == "jac" ? SLIM_SIMTYPE_JAC : sim == "dotp" ? SLIM_SIMTYPE_DOTP : SLIM_SIMTYPE_COS;
  io[SLIM_OPTION_ALGO] = SLIM_ALGO_CD;
  io[SLIM_OPTION_NTHREADS] = a.integer("nthreads", 1);
  io[SLIM_OPTION_MAXNITERS] = a.integer("niters", 10000);
  dopt[SLIM_OPTION_OPTTOL] = a.num("optTol", 1e-7);
  if (a.has("ngpus")) io[SLIM_OPTION_GPU_NGPUS] = a.integer("ngpus", 1);
  if (a.has("gpukernel")) io[SLIM_OPTION_GPU_KERNEL] = a.integer("gpukernel", SLIMGPU_KERNEL_AUTO);

  int32_t status = SLIM_ERROR;
  slimgpu_matrix_t* R = SLIMGPU_MatrixFromHost(trn.nrows, trn.ptr.data(), trn.ind.data(),
                                               trn.valptr(), io, &status);
  if (!R) die(std::string("cannot stage the training matrix: ") + SLIMGPU_LastError());
  slim_t* hold = to_handle(trn);
  const int32_t ncols = std::max(trn.ncols, tst.ncols);
  int32_t* fmarker = SLIM_DetermineHeadAndTail(trn.nrows, ncols, trn.ptr.data(), trn.ind.data());

  FILE* lf = std::fopen(a.pos[2].c_str(), "r");
  char line[256];
  {  // one R, as many solves as the file has pairs: let the engine plan for that
    int32_t npairs = 0;
    double l1, l2;
    while (std::fgets(line, sizeof line, lf))
      if (std::sscanf(line, "%lf %lf", &l1, &l2) == 2) ++npairs;
    std::rewind(lf);
    SLIMGPU_MatrixExpectSolves(R, npairs);
  }
  slim_t* model = nullptr;
  slimgpu_model_t* dmodel = nullptr;
  const char* ng_env = std::getenv("SLIM_GPU_NGPUS");
  const char* res_env = std::getenv("SLIM_GPU_RESIDENT");
  const bool resident = !(a.has("ngpus") && a.integer("ngpus", 1) > 1) && !(ng_env && std::atoi(ng_env) > 1) &&
                        !(res_env && std::atoi(res_env) == 0);
  // resident models are evaluated where they lie: the test rows and the marker go to HBM once, a pair
  // brings down its figures only (SLIM_GPU_EVAL_RESIDENT=0, or a refusal: lists through the host)
  const char* evr_env = std::getenv("SLIM_GPU_EVAL_RESIDENT");
  slimgpu_evalset_t* evalset = nullptr;
  const int32_t nall = std::min(trn.nrows, tst.nrows);
  std::vector<int32_t> sel;  // -evalstride: the evaluated users
  if (stride > 1)
    for (int64_t u = 0; u < nall; u += stride) sel.push_back((int32_t)u);
  // lists of more than 128 have no device scorer; the figures then come from the ranks of the held-out items
  const int32_t cutoff = nrcmds;
  bool ranked = false;
  if (resident && nrcmds >= 1 && !(evr_env && std::atoi(evr_env) == 0)) {
    slim_t* th = to_handle(tst);
    if (nrcmds <= 128) {
      evalset = SLIMGPU_EvalSetCreateAt(R, th, fmarker, ncols, 1, &cutoff, (int32_t)sel.size(),
                                        sel.empty() ? nullptr : sel.data(), &status);
    } else {
      evalset = SLIMGPU_EvalSetCreateRanked(R, th, fmarker, ncols, (int32_t)sel.size(),
                                            sel.empty() ? nullptr : sel.data(), &status);
      ranked = evalset != nullptr;
    }
    Py_csr_free(th);
  }
  // the host loop has no subset form: a stride without the evaluation in HBM fails before the first solve
  if (stride > 1 && !evalset)
    die(std::string("-evalstride needs the evaluation in HBM (one GPU, nrcmds >= 1, SLIM_GPU_RESIDENT and "
                    "SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs): ") +
        (nrcmds < 1 ? "nrcmds is " + std::to_string(nrcmds) : std::string(SLIMGPU_LastError())));
  if (evalexposure && (!evalset || ranked))
    die(std::string("-evalexposure needs the evaluation in HBM (one GPU, SLIM_GPU_RESIDENT and SLIM_GPU_EVAL_RESIDENT "
                    "not 0, a matrix staged without merged pairs): ") +
        (!resident ? std::string("the models of this grid do not stay in HBM")
         : evr_env && std::atoi(evr_env) == 0 ? std::string("SLIM_GPU_EVAL_RESIDENT=0") : std::string(SLIMGPU_LastError())));
  // nor is there an evaluation under a filter outside HBM: no silent evaluation on the raw catalogue
  CliFilter flt;
  int32_t rrows = 0, rcols = 0;  // the resident models are as wide as the staged matrix
  int64_t rnnz = 0;
  if (filtered) {
    if (!evalset)
      die(std::string("the item filters need the evaluation in HBM (one GPU, nrcmds >= 1, SLIM_GPU_RESIDENT and "
                      "SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs): ") +
          (!resident ? std::string("the models of this grid do not stay in HBM")
           : evr_env && std::atoi(evr_env) == 0 ? std::string("SLIM_GPU_EVAL_RESIDENT=0")
           : nrcmds < 1 ? "nrcmds is " + std::to_string(nrcmds) : std::string(SLIMGPU_LastError())));
    SLIMGPU_MatrixInfo(R, &rrows, &rcols, &rnnz);
    flt = read_filter(a, rcols, fmt);
  }
  // sampled negatives: the set is drawn once, on the device, from the eval set's users; never a fall-back to the
  // full-catalogue figures
  slimgpu_candset_t* cands = nullptr;
  if (evalnegs > 0) {
    if (!evalset)
      die(std::string("-evalnegs needs the evaluation in HBM (one GPU, nrcmds >= 1, SLIM_GPU_RESIDENT and "
                      "SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs): ") +
          (!resident ? std::string("the models of this grid do not stay in HBM")
           : evr_env && std::atoi(evr_env) == 0 ? std::string("SLIM_GPU_EVAL_RESIDENT=0")
           : nrcmds < 1 ? "nrcmds is " + std::to_string(nrcmds) : std::string(SLIMGPU_LastError())));
    if ((evalnegpop ? SLIMGPU_EvalSetSampleCandidatesWeighted(evalset, evalnegs, (uint64_t)evalseed, nullptr, &cands)
                    : SLIMGPU_EvalSetSampleCandidates(evalset, evalnegs, (uint64_t)evalseed, &cands)) != SLIM_OK)
      die(std::string("-evalnegs: ") + SLIMGPU_LastError());
  }
  if (stride > 1) std::printf("  evaluating every %d-th user: %zu of %d\n", stride, sel.size(), nall);
  if (cands) {
    int64_t entries = 0;
    SLIMGPU_CandSetInfo(cands, nullptr, nullptr, &entries);
    std::printf("  sampled negatives: nnegs %d, seed %llu, %s%lld candidate entries\n", evalnegs,
                (unsigned long long)evalseed, evalnegpop ? "popularity, " : "", (long long)entries);
  }
  if (filtered)
    std::printf("  item filter: %lld of %d items allowed, %lld exclusion entries\n", (long long)flt.allowed, rcols,
                (long long)flt.excluded);
  std::printf("\nEstimating & evaluating models...\n\n");
  double best_hr = 0, best_ar = 0, bh_l1 = 0, bh_l2 = 0, ba_l1 = 0, ba_l2 = 0;
  while (std::fgets(line, sizeof line, lf)) {
    double l1, l2;
    if (std::sscanf(line, "%lf %lf", &l1, &l2) != 2) continue;  // slim_mselect.c:100-101
    dopt[SLIM_OPTION_L1R] = l1;
    dopt[SLIM_OPTION_L2R] = l2;
    // the model stays in HBM (SLIMGPU_LearnResident): warm start without an upload, scored where it
    // lies; with model files wanted it is fetched beside nothing -- the write needs it at once
    // (a model sharded over several GPUs is assembled on the host: SLIMGPU_Learn as before)
    if (!resident) {
      slim_t* next = SLIMGPU_Learn(R, io, dopt, model, &status);  // warm start, :103-113
      SLIM_FreeModel(&model);
      model = next;
    } else {
      slimgpu_model_t* dnext = SLIMGPU_LearnResident(R, io, dopt, dmodel, &status);  // warm start, :103-113
      SLIMGPU_ModelFree(&dmodel);
      dmodel = dnext;
      SLIM_FreeModel(&model);
    }
    if (resident ? !dmodel : !model) {
      std::printf("ERROR: model estimation failed [%.3le %.3le]: rstatus %d\n", l1, l2, status);
      continue;
    }
    slimgpu_stats_t st;
    SLIMGPU_LastStats(&st);
    if (resident && !a.has("nomodels")) {
      model = SLIMGPU_ModelFetch(dmodel, &status);
      if (!model) {
        std::printf("ERROR: model fetch failed [%.3le %.3le]: rstatus %d\n", l1, l2, status);
        continue;
      }
    }
    if (!a.has("nomodels")) {
      std::string name(line);
      while (!name.empty() && (name.back() == '\n' || name.back() == '\r')) name.pop_back();
      write_matrix(static_cast<slim_csr_t*>(model), name + ".model", fmt == Fmt::csrnv ? Fmt::csr : fmt);
    }
    Eval e;
    double em[4];
    int32_t env[3];
    slimgpu_exposure_t expo = {};
    // (one list length: the filtered call's only row is SLIMGPU_ModelEvaluate's; a null filter is no filter)
    const bool evaluated =
        evalset && (cands    ? SLIMGPU_ModelEvaluateCandidates(evalset, dmodel, cands, 1, em, env)
                    : ranked ? SLIMGPU_ModelEvaluateRankedFiltered(evalset, dmodel, flt.handle, 1, &cutoff, em, env)
                    : evalexposure
                        ? SLIMGPU_ModelEvaluateExposure(evalset, dmodel, flt.handle, 1, em, env, nullptr, &expo)
                        : SLIMGPU_ModelEvaluateAtFiltered(evalset, dmodel, flt.handle, 1, em, env)) == SLIM_OK;
    if (!evaluated && (stride > 1 || filtered || cands || evalexposure)) die(std::string("evaluation failed: ") + SLIMGPU_LastError());
    if (evaluated) {
      e.hr = em[0]; e.hr_head = em[1]; e.hr_tail = em[2]; e.arhr = em[3];
      e.nvalid = env[0]; e.nvalid_head = env[1]; e.nvalid_tail = env[2];
    } else {
    std::vector<int32_t> lists((size_t)trn.nrows * nrcmds, -1), lens(trn.nrows, 0);
    std::vector<float> scores((size_t)trn.nrows * nrcmds, 0.0f);
    if (!resident) {
      if (Py_SLIM_Predict(nrcmds, model, hold, lists.data(), scores.data()) != SLIM_OK) continue;
    } else if (SLIMGPU_ModelPredict(nrcmds, dmodel, hold, lists.data(), scores.data()) != SLIM_OK) {
      if (!model) model = SLIMGPU_ModelFetch(dmodel, &status);  // (lists beyond the GPU scorer's 128: host loop)
      if (!model || Py_SLIM_Predict(nrcmds, model, hold, lists.data(), scores.data()) != SLIM_OK) continue;
    }
    for (int32_t u = 0; u < trn.nrows; ++u)
      while (lens[u] < nrcmds && lists[(size_t)u * nrcmds + lens[u]] >= 0) ++lens[u];
    e = evaluate_lists(tst, lists, lens, nrcmds, fmarker, ncols);
    }
    std::printf("l1r: %.2le l2r: %.2le nnz: %7zd hr: %.4f hr_head: %.4f hr_tail: %.4f arhr: %.4f time: %.2lf\n",
                l1, l2, resident ? (ssize_t)SLIMGPU_ModelNnz(dmodel) : static_cast<slim_csr_t*>(model)->rowptr[static_cast<slim_csr_t*>(model)->nrows], e.hr, e.hr_head, e.hr_tail, e.arhr, st.total_ms / 1e3);
    if (evalexposure)
      std::printf("  exposure@%d: coverage: %.4f tail_share: %.4f gini: %.4f avg_pop: %.2f distinct: %d slots: %lld\n",
                  nrcmds, expo.coverage, expo.tail_share, expo.gini, expo.avg_pop, expo.distinct, (long long)expo.slots);
    if (e.hr > best_hr) { best_hr = e.hr; bh_l1 = l1; bh_l2 = l2; }
    if (e.arhr > best_ar) { best_ar = e.arhr; ba_l1 = l1; ba_l2 = l2; }
  }
  std::fclose(lf);
  std::printf("\nbest hr: %.4f at l1 %.4g l2 %.4g; best arhr: %.4f at l1 %.4g l2 %.4g\n", best_hr, bh_l1,
              bh_l2, best_ar, ba_l1, ba_l2);
  std::printf("\nDone.\n------------------------------------------------------------------\n");
  SLIM_FreeModel(&model);
  SLIMGPU_ModelFree(&dmodel);
  SLIMGPU_CandSetFree(cands);
  SLIMGPU_EvalSetFree(&evalset);
  SLIMGPU_FilterFree(flt.handle);
  std::free(fmarker);
  Py_csr_free(hold);
  SLIMGPU_MatrixFree(&R);
  return 0;
}
