#!/usr/bin/env python3
"""Sampled-negative evaluation at C4 scale: what the device sampler and an evaluation on its set cost
(include/slim_gpu_sample.h), and what the split of the candidate set's device copy costs existing callers.

The model and the users are those of scripts/topn_scale.py and scripts/cand_scale.py (a synthetic 100K x 100K model
with 2700 entries per row, the first 131 072 users of the synthetic C4 matrix), resident; the test matrix holds one
random item per user.  One job, the runs alternating and repeated, medians:

  (a) cand k = 100, lists of 64   SLIMGPU_MatrixScoreCandidates on an UPLOADED set, this build alternating with
                                  another build of the library (--parent-lib: the parent commit's).  The only
                                  pass / fail figure: this build's median is no slower than the parent's slowest
                                  run plus the parent's own spread (max - min), and the lists are bit-equal.
  (b) nnegs = 99, 999             SLIMGPU_EvalSetSampleCandidates (the draw, the rows and the index sort: a device-born
                                  set is indexed where it is made), the first SLIMGPU_ModelEvaluateCandidates on the
                                  set, a later one, beside the full-catalogue SLIMGPU_ModelEvaluate on the same
                                  users.  Reported, not judged.

Seconds are wall time of the call.  Every run has its own time limit; the job ends at the first run that fails or
overruns it.

  python scripts/sampled_eval.py [--parent-lib PATH] [--users 131072] [--rounds 2] [--out profiles/sampled_eval.txt]
"""
import argparse
import ctypes as C
import json
import os
import platform
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

NNEGS = (99, 999)


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
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    sampled = hasattr(lib, "SLIMGPU_EvalSetSampleCandidates")
    ev = None
    if sampled:
        T = sp.csr_matrix((np.ones(U, np.float32), rng.integers(0, n, U).astype(np.int32), np.arange(U + 1)), shape=(U, n))
        ev = mat.evaluator(T, fmarker=np.zeros(n, np.int32), cutoffs=(10,))
    g = np.random.default_rng(100 + 100)
    neg = g.integers(0, n, size=(U, 100), dtype=np.int32)
    uploaded = mat.candidate_set((np.arange(U + 1, dtype=np.int64) * 100, neg.ravel()))
    born = {}
    gpu = "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"))
    print(json.dumps({"ready": True, "gpu": gpu, "users": U, "history_nnz": int(hind.size),
                      "model_nnz": int(wind.size)}), flush=True)
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        kind, a = word[0], int(word[1])
        row = {"users": U}
        t0 = time.time()
        if kind == "cand":
            ids, sc, cnt = np.full(U * 64, -1, np.int32), np.zeros(U * 64, np.float32), np.zeros(U, np.int32)
            t0 = time.time()
            rc = lib.SLIMGPU_MatrixScoreCandidates(model.handle, mat.handle, uploaded.handle, 0, None, 64, None, P(ids),
                                                   P(sc), P(cnt))
            dt = time.time() - t0
            if rc != 1:
                print(json.dumps({"failed": [kind, a], "error": _lib.last_error()}), flush=True)
                return 1
            row["crc"] = zlib.crc32(sc.tobytes(), zlib.crc32(ids.tobytes()))
        elif kind == "sample":
            if a in born:
                born.pop(a).close()
            t0 = time.time()
            born[a] = ev.sample_candidates(a, seed=1)
            dt = time.time() - t0
            row["entries"] = int(born[a].size)
        elif kind == "evalc":
            res = ev.evaluate_candidates(model, born[a])
            dt = time.time() - t0
            row.update(hr=res[0]["hr"], arhr=res[0]["arhr"], nvalid=res[0]["nvalid"])
        else:
            res = ev.evaluate(model)
            dt = time.time() - t0
            row.update(hr=res["hr"], arhr=res["arhr"], nvalid=res["nvalid"])
        row.update(seconds=round(dt, 4), users_per_s=round(U / dt, 1))
        if kind != "sample":
            st = eval_stats(lib)
            row.update(kernel_ms=round(st["kernel_ms"], 1), path=st["path"], h2d_bytes=st["h2d_bytes"],
                       device_allocs=st["device_allocs"])
        print(json.dumps(row), flush=True)
    return 0


def main():
    from cand_scale import Worker, median
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libslim.so of the parent commit (omit: no comparison (a))")
    ap.add_argument("--users", type=int, default=131072)
    ap.add_argument("--old-users", type=int, default=8192, help=argparse.SUPPRESS)
    ap.add_argument("--row-nnz", type=int, default=2700)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds one run may take")
    ap.add_argument("--setup-limit", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_eval.txt"))
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

        def ask(self, kind, a):
            self.child.stdin.write(("%s %d\n" % (kind, a)).encode())
            self.child.stdin.flush()
            return self.answer()

    workers = {"new": Mine("new", None)}
    if args.parent_lib:
        workers["parent"] = Mine("parent", args.parent_lib)
    rows, head, verdict = [], {}, "complete"
    first = [("first cand k=100", "new", "cand", 100)]
    if "parent" in workers:
        first.append(("first parent cand k=100", "parent", "cand", 100))
    for k in NNEGS:
        first += [("first sample nnegs=%d" % k, "new", "sample", k), ("first evalc nnegs=%d" % k, "new", "evalc", k)]
    first.append(("first full", "new", "full", 0))
    timed = []
    if "parent" in workers:
        timed.append(("parent cand k=100", "parent", "cand", 100))
    timed.append(("cand k=100", "new", "cand", 100))
    for k in NNEGS:
        timed += [("sample nnegs=%d" % k, "new", "sample", k), ("evalc after sample nnegs=%d" % k, "new", "evalc", k),
                  ("evalc nnegs=%d" % k, "new", "evalc", k)]
    timed.append(("full", "new", "full", 0))
    try:
        for name, w in workers.items():
            head = w.answer(args.setup_limit)
            if not head or "ready" not in head:
                verdict = "worker %s did not get ready" % name
                break
            print(name, json.dumps(head), flush=True)
        for rnd, runs in [(-1, first)] + [(r, timed) for r in range(args.rounds)]:
            for name, wk, kind, a in runs if verdict == "complete" else ():
                row = workers[wk].ask(kind, a)
                if row is None or "failed" in row:
                    verdict = "run %s failed or overran its limit of %g s: job ended (%s)" % (name, args.limit, row)
                    break
                row = dict({"run": name, "round": rnd}, **row)
                print(json.dumps(row), flush=True)
                rows.append(row)
    finally:
        for w in workers.values():
            w.end(kill=verdict != "complete")
    secs, crcs, fig = {}, {}, {}
    for r in rows:
        secs.setdefault(r["run"], []).append(r["seconds"])
        if "crc" in r:
            crcs.setdefault(r["run"].replace("first ", ""), set()).add(r["crc"])
        if "hr" in r:
            fig.setdefault(r["run"].replace("first ", "").replace("after sample ", ""), set()).add((r["hr"], r["arhr"], r["nvalid"]))
    lines = ["# scripts/sampled_eval.py: %d rounds, %d runs, %s" % (args.rounds, len(rows), verdict),
             "# box: %s, %s; %s" % (platform.node(), head.get("gpu", "?") if head else "?", time.strftime("%Y-%m-%d")),
             "# model %d entries (100K x 100K, %d per row), %d users with %d history entries, resident, one held-out item "
             "per user, cutoff 10; seconds = wall time of the call"
             % ((head or {}).get("model_nnz", 0), args.row_nnz, U, (head or {}).get("history_nnz", 0))]
    lines += [json.dumps(r) for r in rows]
    med = {k: median(v) for k, v in secs.items()}
    for k in sorted(med):
        lines.append("# %s: median %.3f s (min %.3f .. max %.3f)" % (k, med[k], min(secs[k]), max(secs[k])))
    ok = True
    p, q = "parent cand k=100", "cand k=100"
    if p in med and q in med:
        bound = max(secs[p]) + (max(secs[p]) - min(secs[p]))
        met = med[q] <= bound
        same = crcs[p] == crcs[q] and len(crcs[q]) == 1
        ok = met and same
        lines.append("# (a) uploaded set, k = 100, lists of 64: this build %.3f s, bound %.3f s (the parent's slowest run "
                     "%.3f + its spread %.3f): %s; lists %s"
                     % (med[q], bound, max(secs[p]), max(secs[p]) - min(secs[p]), "met" if met else "NOT met",
                        "bit-equal" if same else "DIFFER"))
    else:
        lines.append("# (a) not measured (no parent library)")
    for k in NNEGS:
        s, e1, e = "sample nnegs=%d" % k, "evalc after sample nnegs=%d" % k, "evalc nnegs=%d" % k
        if s in med and e in med and "full" in med:
            lines.append("# (b) nnegs = %d, %d users: sampler %.3f s (draw, rows, index sort), the first evaluation of a "
                         "set %.3f s, a later one %.3f s, full catalogue %.3f s: later / full = %.2f; one set of figures "
                         "per seed: %s" % (k, U, med[s], med[e1], med[e], med["full"], med[e] / med["full"],
                                           "yes" if len(fig.get(e, ())) == 1 else "NO"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(l for l in lines if l.startswith("#")))
    sys.exit(0 if verdict == "complete" and ok else 1)


if __name__ == "__main__":
    main()
