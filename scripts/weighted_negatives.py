#!/usr/bin/env python3
"""Popularity-weighted negatives at C4 scale: what the weighted device sampler costs (THE WEIGHTED RULE of
include/slim_gpu_sample.h), and what its presence costs the callers of the unchanged uniform sampler.

The model and the users are those of scripts/topn_scale.py and scripts/sampled_eval.py (a synthetic 100K x 100K model
with 2700 entries per row, the first 131 072 users of the synthetic C4 matrix), resident; the test matrix holds one
random item per user.  One job, the runs alternating and repeated, medians:

  (1) uniform nnegs = 99, 999     SLIMGPU_EvalSetSampleCandidates, this build alternating with another build of the
                                  library (--parent-lib: the parent commit's), before any weighted set is made (the
                                  two workers then hold the same).  The only pass / fail figure: this
                                  build's median is no slower than the parent's slowest run plus the parent's own
                                  spread (max - min).
  (2) popularity nnegs = 99, 999  SLIMGPU_EvalSetSampleCandidatesWeighted with NULL weights: seconds beside (1), the
                                  kernel's own milliseconds (SLIMGPU_LastSampleKernelMs), and the mean draws per
                                  accepted negative -- counted by a numpy restatement of the rule on a sample of the
                                  users, whose rows are checked against the device's.
  (3) cliff nnegs = 99            phase 2 as the common path: a few heavy items (weight 4e9), the next 27 % of a
                                  permutation weight 1, the rest 0.  With the heavy items 3 % of the catalogue (3 000
                                  items) phase 1 fills 99 negatives and phase 2 is never reached, so the figure is taken
                                  with 50 heavy items, as the tests have them, and the 3 % vector is reported beside it.
  (4) one evaluation on the popularity set beside the uniform set's and the full catalogue's.

Stated before the run, from the byte model: the ids of a user are read twice (marking, un-marking), a batch of 64
draws costs one hash, one 64 x 64 multiply and about 17 dependent reads of C (0.8 MB: L2-resident, a few microseconds
a batch), the rows and the index sort are the uniform sampler's.  So the weighted kernel should take about 0.5 - 1.5 ms
at 99 negatives (2 batches a user) and 4 - 10 ms at 999 (17 batches), and the call the uniform call's time plus that.

Seconds are wall time of the call.  Every run has its own time limit; the job ends at the first run that fails or
overruns it.

  python scripts/weighted_negatives.py [--parent-lib PATH] [--users 131072] [--rounds 2]
                                       [--out profiles/weighted_negatives.txt]
"""
import argparse
import ctypes as C
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

NNEGS = (99, 999)
CHECKED = 48            # users whose rows the restatement makes, for the draw and pick counts
G = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def restated(np, seed, u, X, nnegs, Cw):
    """The header's rule for one user in Python integers: (negatives, draws until the row was full or the guard
    ended phase 1, phase-2 picks)."""
    n, T = Cw.size - 1, int(Cw[-1])
    base = mix64((seed + G * (u + 1)) & M64)
    key = lambda d: mix64((base + G * (d + 1)) & M64)  # noqa: E731
    taken = np.zeros(n, bool)
    taken[X] = True
    D, out, d = 16 * nnegs + 1024, [], 0
    while d < D and len(out) < nnegs:
        i = int(np.searchsorted(Cw[1:], np.uint64((key(d) * T) >> 64), side="right"))
        d += 1
        if not taken[i]:
            taken[i] = True
            out.append(i)
    picks = 0
    if len(out) < nnegs:
        mass = np.where(taken, 0, np.diff(Cw)).astype(np.uint64)
        while len(out) < nnegs:
            left = int(mass.sum(dtype=np.uint64))
            if left == 0:
                break
            r = (key(D + picks) * left) >> 64
            i = int(np.searchsorted(np.cumsum(mass, dtype=np.uint64), np.uint64(r), side="right"))
            out.append(i)
            mass[i] = 0
            picks += 1
    return out, d, picks


def cliff(np, n, heavy):
    p = np.random.default_rng(78).permutation(n)
    w = np.zeros(n, np.uint32)
    w[p[:heavy]] = 4_000_000_000
    w[p[heavy:heavy + (27 * n) // 100]] = 1
    return w


def worker(args):
    import numpy as np
    import scipy.sparse as sp
    import torch
    from slim_amd import _lib, synth
    from slim_amd.engine import DeviceMatrix, eval_stats
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    nrows, ncols, target = synth.CONFIGS["c4"]
    rowptr, rowind, _ = synth.generate_csr(nrows, ncols, target, seed=1, device=dev)
    U = args.users
    hptr = rowptr[:U + 1].cpu().numpy().astype(np.int64)
    hind = rowind[:int(hptr[-1])].cpu().numpy().astype(np.int32)
    del rowptr, rowind
    torch.cuda.empty_cache()
    n, k = ncols, args.row_nnz
    rng = np.random.default_rng(5)
    wind = ((np.arange(n, dtype=np.int64)[:, None] * 7 + np.arange(k, dtype=np.int64)[None, :] * 37) % n)
    wind = np.sort(wind, axis=1).astype(np.int32).ravel()
    wval = (rng.random(n * k, dtype=np.float32) * 0.01).astype(np.float32)
    wptr = np.arange(n + 1, dtype=np.int64) * k
    R = sp.csr_matrix((np.ones(hind.size, np.float32), hind, hptr), shape=(U, n))
    mat = DeviceMatrix.from_scipy(R, binary=True)
    model = mat.model_from_scipy(sp.csr_matrix((wval, wind, wptr), shape=(n, n)))
    tind = rng.integers(0, n, U).astype(np.int32)
    T = sp.csr_matrix((np.ones(U, np.float32), tind, np.arange(U + 1)), shape=(U, n))
    ev = mat.evaluator(T, fmarker=np.zeros(n, np.int32), cutoffs=(10,))
    weighted = hasattr(lib, "SLIMGPU_EvalSetSampleCandidatesWeighted")
    vectors = {"popularity": "popularity", "cliff50": cliff(np, n, 50), "cliff3pct": cliff(np, n, (3 * n) // 100)}
    counts = np.bincount(hind, minlength=n).astype(np.uint64)
    tables = {"popularity": counts}
    tables.update({name: v.astype(np.uint64) for name, v in vectors.items() if name != "popularity"})
    born = {}
    gpu = "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"))
    print(json.dumps({"ready": True, "gpu": gpu, "users": U, "history_nnz": int(hind.size),
                      "model_nnz": int(wind.size), "weighted": weighted}), flush=True)
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        kind, what, a = word[0], word[1], int(word[2])
        row = {"users": U}
        t0 = time.time()
        if kind == "sample":
            if (what, a) in born:
                born.pop((what, a)).close()
            t0 = time.time()
            born[(what, a)] = ev.sample_candidates(a, seed=1, weights=None if what == "uniform" else vectors[what])
            dt = time.time() - t0
            row["entries"] = int(born[(what, a)].size)
            if what != "uniform":
                row["sampler_kernel_ms"] = round(float(lib.SLIMGPU_LastSampleKernelMs()), 3)
        elif kind == "check":
            # the draws and picks of the rule, by the restatement, on users spread over the set; its rows are the device's
            ptr, ind = born[(what, a)].rows()
            Cw = np.concatenate([[0], np.cumsum(tables[what], dtype=np.uint64)]).astype(np.uint64)
            draws = picks = negs = 0
            for u in range(0, U, U // CHECKED):
                X = np.unique(np.concatenate([hind[hptr[u]:hptr[u + 1]], tind[u:u + 1]]))
                out, d, p = restated(np, 1, u, X, a, Cw)
                if ind[ptr[u]:ptr[u + 1]].tolist() != out + [int(tind[u])]:
                    print(json.dumps({"failed": [kind, what, a], "error": "user %d: the device's row is not the "
                                      "restatement's" % u}), flush=True)
                    return 1
                draws, picks, negs = draws + d, picks + p, negs + len(out)
            dt = time.time() - t0
            nchk = len(range(0, U, U // CHECKED))
            row.update(checked_users=nchk, draws_per_negative=round(draws / max(negs - picks, 1), 3),
                       picks_per_user=round(picks / nchk, 2), negatives_per_user=round(negs / nchk, 2))
        elif kind == "evalc":
            res = ev.evaluate_candidates(model, born[(what, a)])
            dt = time.time() - t0
            row.update(hr=res[0]["hr"], arhr=res[0]["arhr"], nvalid=res[0]["nvalid"])
        else:
            res = ev.evaluate(model)
            dt = time.time() - t0
            row.update(hr=res["hr"], arhr=res["arhr"], nvalid=res["nvalid"])
        row.update(seconds=round(dt, 6))
        if kind in ("evalc", "full"):
            st = eval_stats(lib)
            row.update(kernel_ms=round(st["kernel_ms"], 1), path=st["path"])
        print(json.dumps(row), flush=True)
    return 0


def main():
    from cand_scale import Worker, median
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libslim.so of the parent commit (omit: no comparison (1))")
    ap.add_argument("--users", type=int, default=131072)
    ap.add_argument("--row-nnz", type=int, default=2700)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds one run may take")
    ap.add_argument("--setup-limit", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_negatives.txt"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    U = args.users

    class Mine(Worker):     # (cand_scale's worker process, started on this file)
        def __init__(self, name, lib):
            import subprocess
            env = dict(os.environ)
            if lib:
                env["SLIM_AMD_LIB"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--users", str(U), "--row-nnz", str(args.row_nnz)]
            self.name, self.limit = name, args.limit
            self.child = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=env)
            self.pending = b""

        def ask(self, kind, what, a):
            self.child.stdin.write(("%s %s %d\n" % (kind, what, a)).encode())
            self.child.stdin.flush()
            return self.answer()

    workers = {"new": Mine("new", None)}
    if args.parent_lib:
        workers["parent"] = Mine("parent", args.parent_lib)
    rows, head, verdict = [], {}, "complete"
    # (1) runs first and alone, so that the two workers it compares have done and hold the same: uniform sets only.
    # The weighted sets, which stay allocated for the evaluations, are made after it.
    ab, timed = [], []
    for k in NNEGS:
        if "parent" in workers:
            ab.append(("parent uniform nnegs=%d" % k, "parent", "sample", "uniform", k))
        ab.append(("uniform nnegs=%d" % k, "new", "sample", "uniform", k))
        timed.append(("popularity nnegs=%d" % k, "new", "sample", "popularity", k))
    timed += [("cliff50 nnegs=99", "new", "sample", "cliff50", 99), ("cliff3pct nnegs=99", "new", "sample", "cliff3pct", 99),
              ("evalc popularity nnegs=99", "new", "evalc", "popularity", 99),
              ("evalc uniform nnegs=99", "new", "evalc", "uniform", 99), ("full", "new", "full", "-", 0)]
    first = lambda runs: [("first " + name, wk, kind, what, a) for name, wk, kind, what, a in runs]  # noqa: E731
    checks = [("check %s nnegs=%d" % (what, a), "new", "check", what, a)
              for what, a in (("popularity", 99), ("popularity", 999), ("cliff50", 99), ("cliff3pct", 99))]
    try:
        for name, w in workers.items():
            head = w.answer(args.setup_limit)
            if not head or "ready" not in head:
                verdict = "worker %s did not get ready" % name
                break
            print(name, json.dumps(head), flush=True)
        plan = [(-1, first(ab))] + [(r, ab) for r in range(args.rounds)]
        plan += [(-1, first(timed))] + [(r, timed) for r in range(args.rounds)] + [(args.rounds, checks)]
        for rnd, runs in plan:
            for name, wk, kind, what, a in runs if verdict == "complete" else ():
                row = workers[wk].ask(kind, what, a)
                if row is None or "failed" in row:
                    verdict = "run %s failed or overran its limit of %g s: job ended (%s)" % (name, args.limit, row)
                    break
                row = dict({"run": name, "round": rnd}, **row)
                print(json.dumps(row), flush=True)
                rows.append(row)
    finally:
        for w in workers.values():
            w.end(kill=verdict != "complete")
    secs, kms, chk = {}, {}, {}
    for r in rows:
        secs.setdefault(r["run"], []).append(r["seconds"])
        if "sampler_kernel_ms" in r:
            kms.setdefault(r["run"], []).append(r["sampler_kernel_ms"])
        if r["run"].startswith("check "):
            chk[r["run"][6:]] = r
    lines = ["# scripts/weighted_negatives.py: %d rounds, %d runs, %s" % (args.rounds, len(rows), verdict),
             "# box: %s, %s; %s" % (platform.node(), head.get("gpu", "?") if head else "?", time.strftime("%Y-%m-%d")),
             "# model %d entries (100K x 100K, %d per row), %d users with %d history entries, resident, one held-out item "
             "per user, cutoff 10; seconds = wall time of the call (a sampler call: the draw, the rows, the index sort)"
             % ((head or {}).get("model_nnz", 0), args.row_nnz, U, (head or {}).get("history_nnz", 0)),
             "# expected before the run: weighted kernel 0.5 - 1.5 ms at 99 negatives, 4 - 10 ms at 999; the call = the "
             "uniform call + that"]
    lines += [json.dumps(r) for r in rows]
    med = {k: median(v) for k, v in secs.items()}
    for k in sorted(med):
        lines.append("# %s: median %.5f s (min %.5f .. max %.5f)" % (k, med[k], min(secs[k]), max(secs[k])))
    ok = True
    for k in NNEGS:
        p, q = "parent uniform nnegs=%d" % k, "uniform nnegs=%d" % k
        if p in med and q in med:
            bound = max(secs[p]) + (max(secs[p]) - min(secs[p]))
            met = med[q] <= bound
            ok = ok and met
            lines.append("# (1) uniform sampler, nnegs = %d: this build %.5f s, bound %.5f s (the parent's slowest run %.5f "
                         "+ its spread %.5f): %s" % (k, med[q], bound, max(secs[p]), max(secs[p]) - min(secs[p]),
                                                     "met" if met else "NOT met"))
        else:
            lines.append("# (1) nnegs = %d not measured (no parent library)" % k)
        w = "popularity nnegs=%d" % k
        if w in med and q in med:
            c = chk.get(w, {})
            km = median(kms[w])
            lo, hi = (0.5, 1.5) if k == 99 else (4.0, 10.0)
            lines.append("# (2) popularity, nnegs = %d: %.4f s beside the uniform sampler's %.4f s; the weighted kernel %.3f ms "
                         "(expected %g - %g: %s); %s draws per accepted negative (%s users restated, rows equal)"
                         % (k, med[w], med[q], km, lo, hi, "held" if lo <= km <= hi else "below" if km < lo else "ABOVE",
                            c.get("draws_per_negative", "?"), c.get("checked_users", "?")))
    for name in ("cliff50", "cliff3pct"):
        w = "%s nnegs=99" % name
        if w in med:
            c = chk.get(w, {})
            lines.append("# (3) %s, nnegs = 99: %.4f s, the weighted kernel %.3f ms; %s phase-2 picks per user, %s negatives "
                         "per user (%s users restated, rows equal); popularity at 99: %.4f s"
                         % (name, med[w], median(kms[w]), c.get("picks_per_user", "?"), c.get("negatives_per_user", "?"),
                            c.get("checked_users", "?"), med.get("popularity nnegs=99", float("nan"))))
    e = ("evalc popularity nnegs=99", "evalc uniform nnegs=99", "full")
    if all(x in med for x in e):
        lines.append("# (4) one evaluation: popularity set %.3f s, uniform set %.3f s, full catalogue %.3f s"
                     % tuple(med[x] for x in e))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(l for l in lines if l.startswith("#")))
    sys.exit(0 if verdict == "complete" and ok else 1)


if __name__ == "__main__":
    main()
