#!/usr/bin/env python3
"""Learn + evaluate per pair of a model-selection grid with everything resident in HBM (reference loop:
src/programs/slim_mselect.c:99-196): the tests/golden/l12file grid on a synthetic configuration, one
held-out item per user as the test set.  Per pair: the solve (SLIMGPU_LearnResident, warm-started from
the previous model), then the evaluation two ways on the same model, interleaved A / B:

  A  lists through the host: SLIMGPU_ModelPredict on the host handle of the training rows (uploads the
     history, brings the lists down) + SLIMGPU_Evaluate (uploads the lists again) -- what
     Py_SLIM_Mselect does with SLIM_GPU_EVAL_RESIDENT=0
  B  SLIMGPU_ModelEvaluate on an eval set staged once (the fused kernel: 40 bytes come down)

and checks that both give the same figures.  Writes the per-pair table, the totals and the achieved
w_bytes / kernel_ms against the 8 TB/s HBM peak to --out.

  python scripts/grid_eval.py [--workload c5] [--scale 1.0] [--pairs 0] [--budget-s 900] [--out FILE]
                              [--stride 1,10,100] [--cutoffs 5,10,20]

--stride: after the grid, the last model evaluated on every K-th user for each K given (an eval set with a
user list, SLIMGPU_EvalSetCreateAt): seconds, kernel time and w_bytes per K.  --cutoffs: the last model
evaluated at these list lengths in ONE pass (SLIMGPU_ModelEvaluateAt), against one pass per length; the
rows of the one pass must equal the single passes.  With SLIM_AMD_LIB pointing at a build from before these
entry points (an A / B run against it) the grid part still runs; --stride and --cutoffs need the new build.

--ranked: instead of the grid, ONE model (the file's first pair) evaluated in the same process, alternating, --runs
times each: (A) SLIMGPU_ModelEvaluate at --nrcmds from the build at --parent-lib (the parent commit's libslim.so, with
a matrix handle, a model and an eval set of its own over the same device arrays; skipped without it), (B) the same
call from this build, (C) SLIMGPU_ModelEvaluateRanked at the cutoff --nrcmds, (D) the same at --ranked-cutoffs.
C and D report the pre-pass (k_test_keys) from its own events; B and C must give the same figures.
With --filtered the variants are instead A, A2 (the parent build's SLIMGPU_ModelEvaluateRanked), B, C, and E / F: B's and
C's calls of this build under a candidate filter (SLIMGPU_ModelEvaluateAtFiltered, SLIMGPU_ModelEvaluateRankedFiltered)
that allows --allow-fraction of the items and excludes --exclusions random items per user.  The bound on B (C) is A's
(A2's) slowest run plus the spread of A's (A2's) runs, all in this one job; every run has --run-limit-s seconds, after
which the process is killed (SIGALRM, no handler).

--pairs 0 (default): the short grid -- the cold pair, three l2 steps and one l1 change; N > 0: the first
N pairs of the file; -1: all of them (each warm-started from the one before it in the list).  The run stops adding pairs when --budget-s is used up and says so.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def head_tail(pop, nnz):
    """SLIM_DetermineHeadAndTail (api.c:215-245) from the items' popularity: 0 head, 1 tail."""
    import numpy as np
    order = np.argsort(-pop, kind="stable")
    before = np.concatenate([[0], np.cumsum(pop[order])[:-1]])
    fm = np.ones(pop.size, np.int32)
    fm[order[(nnz // 2 - before) > 0]] = 0
    return fm


def make_evaluator(mat, T, fm, nrcmds=10, cutoffs=None, users=None):
    """mat.evaluator(); on a build without SLIMGPU_EvalSetCreateAt (SLIM_AMD_LIB, A / B runs): the
    one-length, every-user eval set through SLIMGPU_EvalSetCreate."""
    import numpy as np
    from slim_amd import _lib as _l
    from slim_amd.engine import Evaluator, _wrap_rows
    lib = mat._lib
    if hasattr(lib, "SLIMGPU_EvalSetCreateAt"):
        return mat.evaluator(T, nrcmds=nrcmds, fmarker=fm, cutoffs=cutoffs, users=users)
    assert cutoffs is None and users is None, "this build of the library has no SLIMGPU_EvalSetCreateAt"
    fm = np.ascontiguousarray(fm, dtype=np.int32)
    ht = _wrap_rows(lib, T)
    st = C.c_int32(0)
    h = lib.SLIMGPU_EvalSetCreate(mat.handle, ht, fm, fm.size, int(nrcmds), C.byref(st))
    lib.Py_csr_free(ht)
    assert h, _l.last_error()
    return Evaluator(lib, h, mat, (int(nrcmds),))


class ParentBuild(object):
    """The few entry points run A needs, from another build of the library (its handles are its own)."""

    def __init__(self, path, shape, T, fm, l1, l2, seed):
        import numpy as np
        from slim_amd import _lib as _l
        from slim_amd.engine import _wrap_rows, make_options
        self.lib = lib = C.CDLL(path)
        for table in (_l._SIGNATURES, _l._EVAL_SIGNATURES, _l._RANK_SIGNATURES):
            for name, (res, argt) in table.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, argt
        nrows, ncols, ptr, ind = shape
        iopt, dopt = make_options(device=0)
        st = C.c_int32(0)
        self.mat = C.c_void_p(lib.SLIMGPU_MatrixFromDevice(nrows, ncols, C.c_void_p(ptr.data_ptr()),
                                                           C.c_void_p(ind.data_ptr()), None,
                                                           iopt.ctypes.data_as(C.c_void_p), C.byref(st)))
        assert self.mat, lib.SLIMGPU_LastError()
        iopt, dopt = make_options(l1r=l1, l2r=l2, optTol=1e-7, niters=10000, seed=seed)
        self.model = C.c_void_p(lib.SLIMGPU_LearnResident(self.mat, iopt.ctypes.data_as(C.c_void_p),
                                                          dopt.ctypes.data_as(C.c_void_p), None, C.byref(st)))
        assert self.model, lib.SLIMGPU_LastError()
        self.nnz = int(lib.SLIMGPU_ModelNnz(self.model))
        ht = _wrap_rows(lib, T)
        fm = np.ascontiguousarray(fm, dtype=np.int32)
        self.es = C.c_void_p(lib.SLIMGPU_EvalSetCreate(self.mat, ht, fm, fm.size, 10, C.byref(st)))
        lib.Py_csr_free(ht)
        assert self.es, lib.SLIMGPU_LastError()
        ht = _wrap_rows(lib, T)
        self.esr = C.c_void_p(lib.SLIMGPU_EvalSetCreateRanked(self.mat, ht, fm, fm.size, 0, None, C.byref(st)))
        lib.Py_csr_free(ht)
        assert self.esr, lib.SLIMGPU_LastError()

    def evaluate(self, ranked=False):
        import numpy as np
        from slim_amd import _lib as _l
        from slim_amd.constants import SLIM_OK
        met, nv = np.zeros(4), np.zeros(3, np.int32)
        cut = np.array([10], np.int32)
        t0 = time.time()
        if ranked:
            rc = self.lib.SLIMGPU_ModelEvaluateRanked(self.esr, self.model, 1, cut.ctypes.data_as(C.c_void_p), met, nv)
        else:
            rc = self.lib.SLIMGPU_ModelEvaluate(self.es, self.model, met, nv)
        s = time.time() - t0
        assert rc == SLIM_OK, (rc, self.lib.SLIMGPU_LastError())
        st = _l.EvalStats()
        self.lib.SLIMGPU_LastEvalStats(C.byref(st))
        return s, (met.tolist(), nv.tolist()), st.as_dict(), float(self.lib.SLIMGPU_LastRankPrepassMs()) if ranked else 0.0

    def close(self):
        self.lib.SLIMGPU_EvalSetFree(C.byref(self.esr))
        self.lib.SLIMGPU_EvalSetFree(C.byref(self.es))
        self.lib.SLIMGPU_ModelFree(C.byref(self.model))
        self.lib.SLIMGPU_MatrixFree(C.byref(self.mat))


def ranked_comparison(args, mat, T, fm, shape, say):
    assert args.nrcmds == 10 or not args.parent_lib, "run A is made for nrcmds 10"
    l1, l2 = [tuple(map(float, l.split())) for l in open(os.path.join(ROOT, "tests", "golden", "l12file")) if l.strip()][0]
    model, _ = mat.learn_resident(l1r=l1, l2r=l2, optTol=1e-7, niters=10000, seed=args.seed)
    say("# one model, l1 %g l2 %g: nnz %d" % (l1, l2, model.nnz))
    ev = mat.evaluator(T, nrcmds=args.nrcmds, fmarker=fm)
    evr = mat.evaluator(T, fmarker=fm, ranked=True)
    parent = None
    if args.parent_lib:
        parent = ParentBuild(args.parent_lib, shape, T, fm, l1, l2, args.seed)
        say("# parent build %s: its own handle and eval set over the same device arrays; its model is LEARNED SEPARATELY by "
            "that build with the same options (nnz %d, this build's %d): A evaluates that model, B / C / D this build's"
            % (args.parent_lib, parent.nnz, model.nnz))
    many = [int(v) for v in args.ranked_cutoffs.split(",") if v]
    KEYS = ("hr", "hr_head", "hr_tail", "arhr")
    NK = ("nvalid", "nvalid_head", "nvalid_tail")
    fig = lambda d: ([float(d[k]) for k in KEYS], [int(d[k]) for k in NK])

    def run_b():
        t0 = time.time()
        g = ev.evaluate(model)
        return time.time() - t0, fig(g), ev.stats(), 0.0

    def run_c():
        t0 = time.time()
        g = evr.evaluate_ranked(model, [args.nrcmds])
        return time.time() - t0, fig(g[0]), evr.stats(), evr.prepass_ms()

    def run_d():
        t0 = time.time()
        g = evr.evaluate_ranked(model, many)
        return time.time() - t0, [(r["nrcmds"], r["hr"], r["arhr"]) for r in g], evr.stats(), evr.prepass_ms()

    def run_a():
        return parent.evaluate()

    def run_a2():
        return parent.evaluate(ranked=True)

    variants = ([("A", run_a)] if parent else []) + [("B", run_b), ("C", run_c), ("D", run_d)]
    flt = None
    if args.filtered:
        import numpy as np
        import scipy.sparse as sp
        t0 = time.time()
        rng = np.random.default_rng(args.seed + 7)
        nrows, ncols = shape[0], shape[1]
        allowed = np.flatnonzero(rng.random(ncols) < args.allow_fraction)
        X = sp.csr_matrix((nrows, ncols), dtype=np.float32)      # (by hand: no sort, no merge of repeats)
        X.indices = rng.integers(0, ncols, size=nrows * args.exclusions, dtype=np.int32)
        X.indptr = np.arange(nrows + 1, dtype=np.int64) * args.exclusions
        X.data = np.ones(X.indices.size, np.float32)
        flt = mat.item_filter(allowed=allowed, exclusions=X)
        say("# filter: %d of %d items allowed, %d exclusions per user (%d entries), made in %.1f s"
            % (allowed.size, ncols, args.exclusions, X.indices.size, time.time() - t0))
        del X

        def run_e():
            t0 = time.time()
            g = ev.evaluate(model, filter=flt)
            return time.time() - t0, fig(g), ev.stats(), 0.0

        def run_f():
            t0 = time.time()
            g = evr.evaluate_ranked(model, [args.nrcmds], filter=flt)
            return time.time() - t0, fig(g[0]), evr.stats(), evr.prepass_ms()

        variants = ([("A", run_a), ("A2", run_a2)] if parent else []) + [("B", run_b), ("C", run_c), ("E", run_e),
                                                                        ("F", run_f)]
    if args.run_limit_s > 0:     # every run under its own limit: SIGALRM without a handler ends the process
        import signal

        def limited(f):
            def g():
                signal.alarm(int(args.run_limit_s))
                try:
                    return f()
                finally:
                    signal.alarm(0)
            return g
        variants = [(n, limited(f)) for n, f in variants]
    for name, fn in variants:            # a warm-up of each: workspaces made, code objects loaded
        fn()
    say("# %-3s %-3s %9s %10s %11s %5s %6s %6s %9s | figures" % ("run", "var", "eval_s", "kernel_ms", "prepass_ms", "path",
                                                               "allocs", "d2h", "w_GB"))
    res = {n: [] for n, _ in variants}
    figs = {}
    for r in range(args.runs):
        for name, fn in variants:
            s, f, st, pre = fn()
            res[name].append((st["kernel_ms"], pre))
            figs[name] = f
            say("  %-3d %-3s %9.3f %10.1f %11.1f %5d %6d %6d %9.1f | %s"
                % (r, name, s, st["kernel_ms"], pre, st["path"], st["device_allocs"], st["d2h_bytes"],
                   st["w_bytes"] / 1e9, f))
    assert figs["B"] == figs["C"], "B and C disagree: %r vs %r" % (figs["B"], figs["C"])
    say("# B and C gave equal figures%s" % ("; A (the parent's own model) too" if parent and figs["A"] == figs["B"] else ""))
    for name, _ in variants:
        k = [x[0] for x in res[name]]
        p = [x[1] for x in res[name]]
        say("# %s: kernel_ms %.1f .. %.1f%s" % (name, min(k), max(k), "" if name in ("A", "B", "E") else
                                               ", pre-pass %.1f .. %.1f ms" % (min(p), max(p))))
    if args.filtered:
        assert figs["E"] == figs["F"], "E and F disagree: %r vs %r" % (figs["E"], figs["F"])
        say("# E and F gave equal figures; filtered hr %.6f against %.6f unfiltered" % (figs["E"][0][0], figs["B"][0][0]))
        for mine, theirs in (("B", "A"), ("C", "A2")) if parent else ():
            km, kt = [x[0] for x in res[mine]], [x[0] for x in res[theirs]]
            bound = max(kt) + (max(kt) - min(kt))
            say("# %s against %s: the parent's slowest run %.1f ms + its spread %.1f ms = %.1f ms; this build's slowest "
                "%.1f ms, median %.1f ms: %s" % (mine, theirs, max(kt), max(kt) - min(kt), bound, max(km),
                                                 sorted(km)[len(km) // 2], "inside" if max(km) <= bound else "EXCEEDS"))
        if parent:
            parent.close()
        flt.close()
        ev.close()
        evr.close()
        model.free()
        return
    kb = [x[0] for x in res["B"]]
    kc, pc = [x[0] for x in res["C"]], [x[1] for x in res["C"]]
    say("# C against B: slowest C %.1f ms; B's slowest run plus the pre-pass = %.1f ms: %s"
        % (max(kc), max(kb) + max(pc), "inside" if max(kc) <= max(kb) + max(pc) else "EXCEEDS"))
    if parent:
        ka = [x[0] for x in res["A"]]
        say("# B against A: A's band %.1f .. %.1f ms, B %.1f .. %.1f ms: %s"
            % (min(ka), max(ka), min(kb), max(kb), "inside" if min(ka) <= min(kb) and max(kb) <= max(ka) else "outside"))
        parent.close()
    ev.close()
    evr.close()
    model.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c5")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--nrcmds", type=int, default=10)
    ap.add_argument("--budget-s", type=float, default=900.0)
    ap.add_argument("--no-a", action="store_true", help="skip path A (no host copy of the training rows)")
    ap.add_argument("--stride", default="", help="comma-separated strides K: the last model on every K-th user")
    ap.add_argument("--cutoffs", default="", help="comma-separated list lengths: one pass against one pass each")
    ap.add_argument("--ranked", action="store_true", help="the four-way comparison of the ranked evaluation")
    ap.add_argument("--parent-lib", default="", help="--ranked: libslim.so of the parent commit (run A)")
    ap.add_argument("--runs", type=int, default=4, help="--ranked: runs of each variant")
    ap.add_argument("--ranked-cutoffs", default="5,10,20,50,100,200,500", help="--ranked: the cutoffs of run D")
    ap.add_argument("--filtered", action="store_true", help="--ranked: what a filter costs, and what carrying it costs")
    ap.add_argument("--allow-fraction", type=float, default=0.5, help="--filtered: the allow set's share of the items")
    ap.add_argument("--exclusions", type=int, default=20, help="--filtered: exclusion entries per user")
    ap.add_argument("--run-limit-s", type=float, default=0, help="--ranked: seconds every single run may take (0: no limit)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_eval_c5.txt"))
    args = ap.parse_args()
    import numpy as np
    import scipy.sparse as sp
    import torch
    from slim_amd import _lib as _l
    from slim_amd import synth
    from slim_amd.constants import SLIM_OK
    from slim_amd.engine import DeviceMatrix

    t_start = time.time()
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)

    dev = torch.device("cuda", 0)
    nrows, ncols, target = synth.scaled(args.workload, args.scale) if args.scale != 1 \
        else synth.CONFIGS[args.workload]
    rowptr, rowind, _ = synth.generate_csr(nrows, ncols, target, seed=args.seed, device=dev)
    # one held-out item per user with at least two
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed + 1000)
    deg = rowptr[1:] - rowptr[:-1]
    has = deg >= 2
    off = (torch.rand(nrows, generator=gen, device=dev, dtype=torch.float64) * deg.to(torch.float64)).to(torch.int64)
    pick = (rowptr[:-1] + torch.minimum(off, torch.clamp(deg - 1, min=0)))[has]
    keep = torch.ones(rowind.numel(), dtype=torch.bool, device=dev)
    keep[pick] = False
    tst_ind = rowind[pick].cpu().numpy()
    trn_ind = rowind[keep].contiguous()
    trn_ptr = torch.zeros(nrows + 1, dtype=torch.int64, device=dev)
    trn_ptr[1:] = torch.cumsum(deg - has.to(torch.int64), 0)
    has_h = has.cpu().numpy()
    del rowptr, rowind, keep, pick, off, deg, has
    torch.cuda.synchronize()
    nnz = int(trn_ind.numel())
    T = sp.csr_matrix((np.ones(tst_ind.size, np.float32), tst_ind,
                       np.concatenate([[0], np.cumsum(has_h)]).astype(np.int64)), shape=(nrows, ncols))
    pop = torch.bincount(trn_ind.to(torch.int64), minlength=ncols).cpu().numpy().astype(np.int64)
    fm = head_tail(pop, nnz)
    say("# grid_eval: %s x %.3g: %d users x %d items, %d training entries, %d test entries (one held out per user)"
        % (args.workload, args.scale, nrows, ncols, nnz, T.nnz))
    say("# data ready after %.1f s" % (time.time() - t_start))

    mat = DeviceMatrix.from_device_ptrs(nrows, ncols, trn_ptr.data_ptr(), trn_ind.data_ptr(), 0,
                                        keepalive=(trn_ptr, trn_ind), device=0)
    lib = mat._lib
    if args.ranked:
        ranked_comparison(args, mat, T, fm, (nrows, ncols, trn_ptr, trn_ind), say)
        say("# whole run: %.1f s" % (time.time() - t_start))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        mat.close()
        return
    t0 = time.time()
    ev = make_evaluator(mat, T, fm, nrcmds=args.nrcmds)
    say("# eval set staged once: %.2f s" % (time.time() - t0))
    hr = ht = None
    if not args.no_a:
        t0 = time.time()
        hp = np.ascontiguousarray(trn_ptr.cpu().numpy(), dtype=np.intp)
        hi = trn_ind.cpu().numpy()
        hr = C.c_void_p()
        assert lib.Py_csr_wrapper(nrows, hp, hi, None, C.byref(hr)) == SLIM_OK
        del hp, hi
        from slim_amd.engine import _wrap_rows
        ht = _wrap_rows(lib, T)
        say("# host handles for path A (not timed below): %.1f s" % (time.time() - t0))

    allp = [tuple(map(float, l.split())) for l in open(os.path.join(ROOT, "tests", "golden", "l12file")) if l.strip()]
    if args.pairs == 0:
        first_l1_change = next(k for k, p in enumerate(allp) if p[0] != allp[0][0])
        pairs = allp[:3] + allp[first_l1_change:first_l1_change + 2]
        say("# short grid: the cold pair, two l2 steps, one l1 change, one more l2 step (%d of the file's %d pairs)"
            % (len(pairs), len(allp)))
    else:
        pairs = allp if args.pairs < 0 else allp[:args.pairs]
    mat.expect_solves(len(allp))

    say("# %-5s %-5s %9s | %8s | %8s %9s %4s %6s %5s %9s %7s | %8s | %s"
        % ("l1", "l2", "nnzW", "learn_s", "B eval_s", "kernel_ms", "path", "allocs", "d2h", "w_GB", "TB/s", "A eval_s", "hr arhr"))
    prev = None
    rows = []
    for k, (l1, l2) in enumerate(pairs):
        if time.time() - t_start > args.budget_s:
            say("# budget of %.0f s used up after %d pairs: the remaining %d were not run"
                % (args.budget_s, k, len(pairs) - k))
            break
        t0 = time.time()
        cur, st = mat.learn_resident(warm=prev, l1r=l1, l2r=l2, optTol=1e-7, niters=10000, seed=args.seed)
        learn_s = time.time() - t0
        if prev is not None:
            prev.free()
        prev = cur
        a_s = float("nan")
        want = None
        if hr is not None:     # A first, then B: over the pairs the two alternate A / B / A / B
            ids = np.full(nrows * args.nrcmds, -1, np.int32)
            sc = np.zeros(nrows * args.nrcmds, np.float32)
            met, nv = np.zeros(4), np.zeros(3, np.int32)
            t0 = time.time()
            rc = lib.SLIMGPU_ModelPredict(args.nrcmds, cur.handle, hr, ids.ctypes.data_as(C.c_void_p),
                                          sc.ctypes.data_as(C.c_void_p))
            a1 = time.time() - t0
            assert rc == SLIM_OK, _l.last_error()
            cnt = (ids.reshape(-1, args.nrcmds) >= 0).sum(1).astype(np.int32)   # (the library has them: not timed)
            t0 = time.time()
            rc = lib.SLIMGPU_Evaluate(nrows, args.nrcmds, ids, cnt, ht, fm, fm.size, met, nv)
            a_s = a1 + time.time() - t0
            assert rc == SLIM_OK, _l.last_error()
            want = (met.tolist(), nv.tolist())
            del ids, sc, cnt
        t0 = time.time()
        got = ev.evaluate(cur)
        b_s = time.time() - t0
        es = ev.stats()
        if want is not None:
            have = ([got["hr"], got["hr_head"], got["hr_tail"], got["arhr"]],
                    [got["nvalid"], got["nvalid_head"], got["nvalid_tail"]])
            assert have == want, "A and B disagree: %r vs %r" % (want, have)
        tbs = es["w_bytes"] / max(es["kernel_ms"], 1e-9) / 1e9
        rows.append((learn_s, b_s, a_s, es["w_bytes"], es["kernel_ms"]))
        say("  %-5g %-5g %9d | %8.2f | %8.2f %9.1f %4d %6d %5d %9.1f %7.3f | %8.2f | %.4f %.4f"
            % (l1, l2, cur.nnz, learn_s, b_s, es["kernel_ms"], es["path"], es["device_allocs"], es["d2h_bytes"],
               es["w_bytes"] / 1e9, tbs, a_s, got["hr"], got["arhr"]))
    if rows:
        L, B, A = (sum(r[i] for r in rows) for i in range(3))
        wb, km = sum(r[3] for r in rows), sum(r[4] for r in rows)
        say("# totals over %d pairs: learn %.2f s, evaluate B %.2f s%s" %
            (len(rows), L, B, "" if hr is None else ", evaluate A %.2f s; B / A = %.3f (accepted: <= 1.05); A and B gave "
             "equal figures on every pair" % (A, B / A)))
        say("# scorer: %.1f GB of model rows streamed in %.1f ms of kernel = %.3f TB/s, %.1f %% of the %.0f TB/s HBM peak"
            % (wb / 1e9, km, wb / km / 1e9, 100.0 * wb / km / 1e6 / HBM_PEAK_GBS, HBM_PEAK_GBS / 1e3))
        say("# evaluation is %.0f %% of learn + evaluate (B)" % (100.0 * B / (L + B)))
    def timed(e, many):
        t0 = time.time()
        got = e.evaluate_at(prev) if many else [e.evaluate(prev)]
        return time.time() - t0, got, e.stats()

    strides = [int(v) for v in args.stride.split(",") if v]
    if strides and prev is not None:
        say("# the last model on every K-th user, nrcmds %d (time should follow w_GB)" % args.nrcmds)
        say("# %-6s %10s | %8s %9s %9s %7s | %s" % ("K", "users", "eval_s", "kernel_ms", "w_GB", "TB/s", "hr arhr nvalid"))
        for K in strides:
            users = None if K == 1 else np.arange(0, nrows, K, dtype=np.int32)
            e = make_evaluator(mat, T, fm, nrcmds=args.nrcmds, users=users)
            s, got, es = timed(e, False)
            e.close()
            say("  %-6d %10d | %8.3f %9.1f %9.1f %7.3f | %.4f %.4f %d"
                % (K, nrows if users is None else users.size, s, es["kernel_ms"], es["w_bytes"] / 1e9,
                   es["w_bytes"] / max(es["kernel_ms"], 1e-9) / 1e9, got[0]["hr"], got[0]["arhr"], got[0]["nvalid"]))
    cutoffs = [int(v) for v in args.cutoffs.split(",") if v]
    if cutoffs and prev is not None:
        e = make_evaluator(mat, T, fm, cutoffs=cutoffs)
        s_one, rows_one, es = timed(e, True)
        e.close()
        say("# cutoffs %s in one pass: %.3f s (kernel %.1f ms, d2h %d bytes)" % (cutoffs, s_one, es["kernel_ms"], es["d2h_bytes"]))
        s_sum = 0.0
        for c, row in zip(cutoffs, rows_one):
            e = make_evaluator(mat, T, fm, nrcmds=c)
            s, got, es = timed(e, False)
            e.close()
            s_sum += s
            same = all(got[0][k] == row[k] for k in got[0])
            say("#   nrcmds %3d alone: %.3f s (kernel %.1f ms)  hr %.4f arhr %.4f  %s" %
                (c, s, es["kernel_ms"], row["hr"], row["arhr"], "equal to its row of the one pass" if same else "DIFFERS"))
            assert same, (got[0], row)
        say("# one pass %.3f s against %.3f s for %d single passes: %.2fx" % (s_one, s_sum, len(cutoffs), s_sum / s_one))
    say("# whole run: %.1f s" % (time.time() - t_start))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if prev is not None:
        prev.free()
    ev.close()
    for h in (hr, ht):
        if h is not None:
            lib.Py_csr_free(h)
    mat.close()


if __name__ == "__main__":
    main()
