// slim_mselect -- model selection over the (l1, l2) pairs of an l12 file, warm-starting
// every model from the previous one; R is staged in HBM once for the whole grid.
// Usage and options as /root/reference/src/programs/slim_mselect.c and cmdline_mselect.c
// (slim_mselect [options] train-file test-file l12-file).  With -cvfolds=F there is ONE data file: the library holds
// items out itself and runs the pairs once per fold (include/slim_gpu_split.h: slim_mselect -cvfolds=F data-file l12-file).
#include "cli_common.hpp"
#include "../../../include/slim_gpu_grid.h"
using namespace slimcli;

int main(int argc, char** argv) {
  std::vector<OptSpec> specs = {
      {"ifmt", true},    {"binarize", false}, {"optTol", true},  {"niters", true},
      {"nnbrs", true},   {"simtype", true},   {"algo", true},    {"nthreads", true},
      {"nrcmds", true},  {"dbglvl", true},    {"nomodels", false}, {"ngpus", true},
      {"evalstride", true}, {"evalnegs", true}, {"evalseed", true}, {"evalnegpop", false}, {"evalexposure", false}, {"gpukernel", true}, {"help", false},
      {"evalgroupfile", true}, {"evalhistbands", true}, {"evalselectgroup", true},
      {"cvfolds", true}, {"cvmode", true}, {"cvheld", true}, {"cvminkeep", true}, {"cvseed", true}};
  specs.insert(specs.end(), std::begin(kFilterSpecs), std::end(kFilterSpecs));
  Args a = parse_args(argc, argv, specs);
  const bool cv = a.has("cvfolds");
  if (cv && !a.has("help") && a.pos.size() == 3)
    die("-cvfolds holds items out of ONE data file: slim_mselect -cvfolds=F [options] data-file l12-file (two files, not "
        "three).");
  for (const char* k : {"cvmode", "cvheld", "cvminkeep", "cvseed"})
    if (a.has(k) && !cv) die(std::string("-") + k + " describes the folds of -cvfolds: it needs -cvfolds.");
  if (a.has("help") || a.pos.size() != (cv ? 2u : 3u)) {
    std::printf("\n Usage: slim_mselect [options] train-file test-file l12-file\n"
                "        slim_mselect -cvfolds=F [options] data-file l12-file\n"
                "   -cvfolds=F [-cvmode=leaveout|folds] [-cvheld=h] [-cvminkeep=m] [-cvseed=s]  (engine extension: one\n"
                "   interactions file; the library holds items out itself, reproducibly from the seed (default 1), and runs\n"
                "   the pairs once per fold; a pair is judged by the mean of its fold figures.  leaveout (default): every\n"
                "   user with at least F * h + m entries holds out h (default 1) in each fold, F * h <= 128; folds: every\n"
                "   entry belongs to one of F >= 2 folds; m (default 1): entries a user's train row must keep.  No model\n"
                "   files are written, and the group options do not combine with it)\n"
                "   -ifmt=csr|csrnv|cluto|ijv  -binarize  -optTol=f  -niters=i  -nnbrs=i  -simtype=s\n"
                "   -nrcmds=i  -nthreads=i  -dbglvl=i  -nomodels (do not write '<l1 l2>.model' files)\n"
                "   -ngpus=i   (engine extension: R replicated on i GPUs, every model sharded over them)\n"
                "   -evalstride=i  (engine extension: evaluate users 0, i, 2i, ... only; needs the evaluation in HBM)\n"
                "   -evalnegs=i -evalseed=i  (engine extension: evaluate 1-vs-k on i sampled negatives per user, drawn on\n"
                "   the device with that seed (default 1); needs the evaluation in HBM, nrcmds <= 128 and no filter)\n"
                "   -evalnegpop  (with -evalnegs: draw the negatives in proportion to item popularity, not uniformly)\n"
                "   -evalexposure  (engine extension: one more line per pair on what its lists show -- coverage, tail share,\n"
                "   Gini, mean popularity, counted on the device; needs the evaluation in HBM, nrcmds <= 128, no -evalnegs)\n"
                "   -evalgroupfile=file | -evalhistbands=b0,b1,..  (engine extension: every pair is also evaluated per user\n"
                "   group, from the same scoring pass: one more line per group.  The file holds one group per user row of the\n"
                "   train-file, 0 .. ngroups-1 or -1 for none; the bands (ascending, >= 1) group the users by the length of\n"
                "   their training row: group g holds those that reach g of the bounds.  Needs the evaluation in HBM)\n"
                "   -evalselectgroup=g  (with either: the best pairs are chosen on group g's figures, not on everybody's;\n"
                "   a group without an evaluated user that has a test row ends the run at the first pair, as the library's\n"
                "   loop does)\n"
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
  // (the seed travels in an option slot, where all 32 bits set reads as "not set")
  if (evalseed < 0 || evalseed >= 0xFFFFFFFFll) die("Invalid -evalseed of " + a.str("evalseed", "") + ".");
  const bool evalnegpop = a.has("evalnegpop");
  if (evalnegpop && evalnegs < 1) die("-evalnegpop weights the sampled negatives: it needs -evalnegs.");
  const bool evalexposure = a.has("evalexposure");
  if (evalexposure && evalnegs > 0) die("-evalexposure does not combine with -evalnegs: the exposure of sampled lists is not built.");
  if (evalexposure && (nrcmds < 1 || nrcmds > 128))
    die("-evalexposure needs lists of 1 to 128 places (the lists behind the evaluation), not " + std::to_string(nrcmds) + ".");
  if (a.has("evalgroupfile") && a.has("evalhistbands"))
    die("The -evalgroupfile and -evalhistbands options cannot be used together.");
  const bool grouped = a.has("evalgroupfile") || a.has("evalhistbands");
  if (a.has("evalselectgroup") && !grouped) die("-evalselectgroup chooses on a user group: it needs -evalgroupfile or -evalhistbands.");
  if (a.has("evalgroupfile") && !file_exists(a.str("evalgroupfile", "")))
    die("Input file " + a.str("evalgroupfile", "") + " does not exist.");
  std::vector<int32_t> bands;
  if (a.has("evalhistbands")) {  // b0,b1,..: integers >= 1, strictly ascending, nothing else
    const std::string list = a.str("evalhistbands", "");
    const char* p = list.c_str();
    for (bool more = true; more;) {
      char* e;
      const long b = std::strtol(p, &e, 10);
      if (e == p || b < 1 || b > 0x7fffffffl || (!bands.empty() && b <= bands.back()) || (*e != ',' && *e != 0) ||
          (int)bands.size() + 1 >= SLIMGPU_MAX_GROUPS)
        die("Invalid -evalhistbands of " + list + ".");
      bands.push_back((int32_t)b);
      more = *e == ',';
      p = e + 1;
    }
  }
  const bool filtered = filter_options(a);
  filter_files_exist(a);
  if (evalnegs > 0 && filtered) die("-evalnegs takes no item filter: candidate rows are scored as they are.");
  if (evalnegs > 0 && nrcmds > 128)
    die("-evalnegs needs nrcmds <= 128 (the candidate lists use the eval set's cutoffs), not " + std::to_string(nrcmds) + ".");
  if (cv && grouped) die("-cvfolds does not combine with -evalgroupfile / -evalhistbands: groups inside a cross-validated grid are not built.");
  slimgpu_split_t split = {};
  if (cv) {
    const std::string mode = a.str("cvmode", "leaveout");
    if (mode != "leaveout" && mode != "folds") die("Invalid -cvmode of " + mode + ": leaveout or folds.");
    split.mode = mode == "folds" ? SLIMGPU_SPLIT_FOLDS : SLIMGPU_SPLIT_LEAVE_OUT;
    split.nfolds = a.integer("cvfolds", 0);
    split.nheld = a.integer("cvheld", 1);
    split.minkeep = a.integer("cvminkeep", 1);
    split.seed = a.has("cvseed") ? std::strtoull(a.str("cvseed", "1").c_str(), nullptr, 10) : 1;
    if (split.nfolds < (split.mode == SLIMGPU_SPLIT_FOLDS ? 2 : 1)) die("Invalid -cvfolds of " + a.str("cvfolds", "") + ".");
    if (split.nheld < 1) die("Invalid -cvheld of " + a.str("cvheld", "") + ".");
    if (split.minkeep < 1) die("Invalid -cvminkeep of " + a.str("cvminkeep", "") + ".");
    if (split.mode == SLIMGPU_SPLIT_LEAVE_OUT && (long long)split.nfolds * split.nheld > SLIMGPU_SPLIT_MAX_HELD)
      die("-cvfolds times -cvheld is above " + std::to_string(SLIMGPU_SPLIT_MAX_HELD) + ".");
  }
  Csr trn = read_matrix(a.pos[0], fmt), tst = cv ? Csr() : read_matrix(a.pos[1], fmt);
  if (a.has("binarize")) trn.has_val = false;
  // the group of every user row of the training matrix: the file's, or the band of the row's length
  std::vector<int32_t> group_of_user;
  int32_t ngroups = 0;
  if (a.has("evalgroupfile")) {
    FILE* gf = std::fopen(a.str("evalgroupfile", "").c_str(), "r");
    long g;
    while (std::fscanf(gf, "%ld", &g) == 1) {
      if (g < -1 || g >= SLIMGPU_MAX_GROUPS) die("bad group " + std::to_string(g) + " in " + a.str("evalgroupfile", ""));
      group_of_user.push_back((int32_t)g);
      ngroups = std::max(ngroups, (int32_t)g + 1);
    }
    if (!std::feof(gf)) die("bad group in " + a.str("evalgroupfile", ""));
    std::fclose(gf);
    if ((int32_t)group_of_user.size() != trn.nrows)
      die("The -evalgroupfile holds " + std::to_string(group_of_user.size()) + " groups, the training matrix has " +
          std::to_string(trn.nrows) + " user rows.");
    if (ngroups < 1) die("The -evalgroupfile puts no user into a group.");
  } else if (!bands.empty()) {
    ngroups = (int32_t)bands.size() + 1;
    for (int32_t u = 0; u < trn.nrows; ++u)
      group_of_user.push_back(
          (int32_t)(std::upper_bound(bands.begin(), bands.end(), (int32_t)(trn.ptr[u + 1] - trn.ptr[u])) - bands.begin()));
  }
  const int select_group = a.integer("evalselectgroup", -1);
  if (a.has("evalselectgroup") && (select_group < 0 || select_group >= ngroups))
    die("Invalid -evalselectgroup of " + a.str("evalselectgroup", "") + ": the groups are 0 to " +
        std::to_string(ngroups - 1) + ".");
  const std::string sim = a.str("simtype", "cos");
  banner();
  const std::string l12file = a.pos[cv ? 1 : 2];
  if (cv) {
    std::printf("  datafile: %s, nrows: %d, ncols: %d, nnz: %zd\n", a.pos[0].c_str(), trn.nrows, trn.ncols, trn.nnz());
  } else {
    std::printf("  trnfile: %s, nrows: %d, ncols: %d, nnz: %zd\n", a.pos[0].c_str(), trn.nrows, trn.ncols, trn.nnz());
    std::printf("  tstfile: %s, nrows: %d, ncols: %d, nnz: %zd\n", a.pos[1].c_str(), tst.nrows, tst.ncols, tst.nnz());
  }
  std::printf("  l12file: %s\n", l12file.c_str());

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

  if (stride > 1) io[SLIM_OPTION_GPU_EVALSTRIDE] = stride;
  if (evalnegs > 0) {
    io[SLIM_OPTION_GPU_EVALNEGS] = evalnegs;
    io[SLIM_OPTION_GPU_EVALSEED] = (int32_t)(uint32_t)evalseed;
    io[SLIM_OPTION_GPU_EVALNEGPOP] = evalnegpop;
  }
  if (evalexposure) io[SLIM_OPTION_GPU_EVALEXPOSURE] = 1;
  io[SLIM_OPTION_NRCMDS] = nrcmds;

  FILE* lf = std::fopen(l12file.c_str(), "r");
  char line[256];
  int32_t npairs = 0;  // one R, as many solves as the file has pairs: the engine plans for that
  for (double l1, l2; std::fgets(line, sizeof line, lf);)
    if (std::sscanf(line, "%lf %lf", &l1, &l2) == 2) ++npairs;
  std::rewind(lf);
  // the filter is as wide as the resident models: the staged matrix's largest id + 1
  CliFilter flt;
  if (filtered) flt = read_filter(a, trn.ind.empty() ? 0 : *std::max_element(trn.ind.begin(), trn.ind.end()) + 1, fmt);
  if (cv) {  // the library's cross-validated driver over the file's pairs: per fold a split and a grid
    std::vector<double> pl1, pl2;
    for (double l1, l2; std::fgets(line, sizeof line, lf);)
      if (std::sscanf(line, "%lf %lf", &l1, &l2) == 2) {
        pl1.push_back(l1);
        pl2.push_back(l2);
      }
    std::fclose(lf);
    if (pl1.empty()) die("The l12 file " + l12file + " holds no pair.");
    slim_t* data = to_handle(trn);
    double best[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::fflush(stdout);
    if (SLIMGPU_MselectCVPairs(data, io, dopt, (int32_t)pl1.size(), pl1.data(), pl2.data(), &split, flt.handle, best,
                               nullptr) != SLIM_OK)
      die(std::string("cannot cross-validate this grid: ") + SLIMGPU_LastError());
    std::printf("\nbest mean hr: %.4f at l1 %.4g l2 %.4g; best mean arhr: %.4f at l1 %.4g l2 %.4g\n", best[2], best[0],
                best[1], best[7], best[4], best[5]);
    SLIMGPU_FilterFree(flt.handle);
    Py_csr_free(data);
    return 0;
  }
  // staging, residency, the eval set, the sampler and how a pair is evaluated: the library's grid (slim_gpu_grid.h),
  // which refuses here, before the first solve, what it cannot evaluate as asked
  slim_t* hold = to_handle(trn);
  slim_t* th = to_handle(tst);
  slimgpu_grid_t* grid = nullptr;
  if (SLIMGPU_GridOpen(hold, th, io, dopt, std::max(trn.ncols, tst.ncols), npairs, flt.handle, &grid) != SLIM_OK)
    die(std::string("cannot evaluate this grid: ") + SLIMGPU_LastError());
  if (grouped && SLIMGPU_GridSetGroups(grid, ngroups, group_of_user.data(), select_group) != SLIM_OK)
    die(std::string("cannot evaluate this grid: ") + SLIMGPU_LastError());
  std::vector<int32_t> members((size_t)ngroups + 1, 0);  // (of the users the grid evaluates: the library's count)
  if (grouped && SLIMGPU_GridGroupInfo(grid, &ngroups, members.data()) != SLIM_OK)
    die(std::string("cannot evaluate this grid: ") + SLIMGPU_LastError());
  std::vector<double> gmet(4 * ((size_t)ngroups + 1));
  std::vector<int32_t> gnv(3 * ((size_t)ngroups + 1));
  SLIMGPU_GridDescribe(grid);
  std::printf("\nEstimating & evaluating models...\n\n");
  double best_hr = 0, best_ar = 0, bh_l1 = 0, bh_l2 = 0, ba_l1 = 0, ba_l2 = 0;
  while (std::fgets(line, sizeof line, lf)) {
    double l1, l2;
    if (std::sscanf(line, "%lf %lf", &l1, &l2) != 2) continue;  // slim_mselect.c:100-101
    slimgpu_grid_cell_t c;
    int32_t status = SLIMGPU_GridSolve(grid, l1, l2, &c);  // warm start from the previous pair, :103-113
    if (status != SLIM_OK) {
      std::printf("ERROR: model estimation failed [%.3le %.3le]: rstatus %d\n", l1, l2, status);
      continue;
    }
    if (!a.has("nomodels")) {  // (a model that stays in HBM is fetched for the write)
      slim_t* model = SLIMGPU_GridModel(grid, &status);
      if (!model) {
        std::printf("ERROR: model fetch failed [%.3le %.3le]: rstatus %d\n", l1, l2, status);
        continue;
      }
      std::string name(line);
      while (!name.empty() && (name.back() == '\n' || name.back() == '\r')) name.pop_back();
      write_matrix(static_cast<slim_csr_t*>(model), name + ".model", fmt == Fmt::csrnv ? Fmt::csr : fmt);
    }
    double hr = c.metrics[0], arhr = c.metrics[3];
    std::printf("l1r: %.2le l2r: %.2le nnz: %7zd hr: %.4f hr_head: %.4f hr_tail: %.4f arhr: %.4f time: %.2lf\n",
                l1, l2, (ssize_t)c.nnz, hr, c.metrics[1], c.metrics[2], arhr, c.solve_seconds);
    if (c.has_exposure)
      std::printf("  exposure@%d: coverage: %.4f tail_share: %.4f gini: %.4f avg_pop: %.2f distinct: %d slots: %lld\n",
                  nrcmds, c.exposure.coverage, c.exposure.tail_share, c.exposure.gini, c.exposure.avg_pop,
                  c.exposure.distinct, (long long)c.exposure.slots);
    if (grouped) {
      if (SLIMGPU_GridLastGroups(grid, gmet.data(), gnv.data()) != SLIM_OK)
        die(std::string("cannot read the group figures: ") + SLIMGPU_LastError());
      for (int32_t g = 0; g < ngroups; ++g)
        std::printf("  group %d: members: %d hr: %.4f hr_head: %.4f hr_tail: %.4f arhr: %.4f nvalid: %d\n", g, members[g],
                    gmet[4 * g], gmet[4 * g + 1], gmet[4 * g + 2], gmet[4 * g + 3], gnv[3 * g]);
      if (select_group >= 0) {  // the best pairs are chosen on this group; without a valid user in it, on nothing
        if (gnv[3 * select_group] < 1)
          die("Group " + std::to_string(select_group) + " has no evaluated user with a test row: no pair can be chosen on it.");
        hr = gmet[4 * select_group];
        arhr = gmet[4 * select_group + 3];
      }
    }
    if (hr > best_hr) { best_hr = hr; bh_l1 = l1; bh_l2 = l2; }
    if (arhr > best_ar) { best_ar = arhr; ba_l1 = l1; ba_l2 = l2; }
  }
  std::fclose(lf);
  std::printf("\nbest hr: %.4f at l1 %.4g l2 %.4g; best arhr: %.4f at l1 %.4g l2 %.4g\n", best_hr, bh_l1,
              bh_l2, best_ar, ba_l1, ba_l2);
  std::printf("\nDone.\n------------------------------------------------------------------\n");
  SLIMGPU_GridFree(&grid);
  SLIMGPU_FilterFree(flt.handle);
  Py_csr_free(th);
  Py_csr_free(hold);
  return 0;
}
