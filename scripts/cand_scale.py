#!/usr/bin/env python3
"""Candidate sets at C4 scale: what scoring per-user candidate rows costs (include/slim_gpu_cand.h).

The model and the users are those of scripts/topn_scale.py (a synthetic 100K x 100K model with 2700 entries per
row, the first 131 072 users of the synthetic C4 matrix), resident: the matrix staged, the model made resident
once.  Candidates are uniform random negatives plus one item per user in front.  One job, the runs alternating
and repeated:

  (a) lists N = 64, 1000          SLIMGPU_MatrixPredictLists, this build alternating with another build of the
                                  library (--parent-lib: the parent commit's).  The only pass / fail figure:
                                  this build's median is no slower than the parent's slowest run plus the
                                  parent's own spread (max - min).
  (b) cand k = 100, 1000          SLIMGPU_MatrixScoreCandidates with lists of 64 (no slot scores down), against
                                  lists N = 64 on the same users, and against the old path, SLIMGPU_Predict1vsK
                                  at the same k with lists of 64 on the first --old-users users (host handles:
                                  it uploads the model on every call), beside the new call on those users.
  (c) cand k = 4096 with lists of 4096, k = 10 000 scores only, on the first --big-users users.

Seconds are wall time of the call; kernel_ms is slimgpu_eval_stats_t's.  A set's first call makes its device copy
and is reported apart ("first").  Every run has its own time limit; the job ends at the first run that fails or
overruns it.

  python scripts/cand_scale.py [--parent-lib PATH] [--users 131072] [--rounds 2] [--out profiles/candidate_lists_c4.txt]
"""
import argparse
import ctypes as C
import json
import os
import platform
import select
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIST_N = (64, 1000)
CAND_K = (100, 1000)


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
    UO = min(U, args.old_users)
    hW, hH = C.c_void_p(), C.c_void_p()
    if hasattr(lib, "SLIMGPU_CandSetCreate"):   # (the old path's host handles; the parent build only makes lists)
        assert lib.Py_csr_wrapper(n, wptr.astype(np.intp), wind, P(wval), C.byref(hW)) == 1
        assert lib.Py_csr_wrapper(UO, hptr[:UO + 1].astype(np.intp), hind, None, C.byref(hH)) == 1
    sets = {}

    def negatives(kk, users):
        g = np.random.default_rng(100 + kk)
        neg = g.integers(0, n, size=(users, kk), dtype=np.int32)
        neg[:, 0] = g.integers(0, n, size=users, dtype=np.int32)   # the held-out item
        return neg

    def candset(kk, users):
        if (kk, users) not in sets:
            neg = negatives(kk, users)
            sets[(kk, users)] = (mat.candidate_set((np.arange(users + 1, dtype=np.int64) * kk, neg.ravel())), neg)
        return sets[(kk, users)]

    gpu = "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"))
    print(json.dumps({"ready": True, "gpu": gpu, "users": U, "history_nnz": int(hind.size),
                      "model_nnz": int(wind.size)}), flush=True)
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        kind, a, N, users = word[0], int(word[1]), int(word[2]), int(word[3])
        sel = None if users == U else np.arange(users, dtype=np.int32)
        ids = np.full(max(users * N, 1), -1, np.int32)
        sc = np.zeros(max(users * N, 1), np.float32)
        cnt = np.zeros(users, np.int32)
        slot = None
        if kind == "cand":
            cs, neg = candset(a, users)
            if N == 0:
                slot = np.zeros(cs.size, np.float32)
        t0 = time.time()
        if kind == "lists":
            rc = lib.SLIMGPU_MatrixPredictLists(N, model.handle, mat.handle, 0 if sel is None else users, P(sel), P(ids),
                                                P(sc), P(cnt))
        elif kind == "cand":
            rc = lib.SLIMGPU_MatrixScoreCandidates(model.handle, mat.handle, cs.handle, 0 if sel is None else users,
                                                   P(sel), N, P(slot), P(ids), P(sc), P(cnt))
        else:
            neg = negatives(a, users)
            t0 = time.time()
            rc = lib.SLIMGPU_Predict1vsK(N, a, hW, hH, neg.ravel(), ids, sc)
        dt = time.time() - t0
        if rc != 1:
            print(json.dumps({"failed": [kind, a, N, users], "error": _lib.last_error()}), flush=True)
            return 1
        row = {"users": users, "seconds": round(dt, 3), "users_per_s": round(users / dt, 1),
               "crc": zlib.crc32(sc.tobytes(), zlib.crc32(ids.tobytes()))}
        if kind != "old":
            st = eval_stats(lib)
            row.update(kernel_ms=round(st["kernel_ms"], 1), path=st["path"], h2d_bytes=st["h2d_bytes"],
                       device_allocs=st["device_allocs"])
        print(json.dumps(row), flush=True)
    return 0


class Worker(object):
    def __init__(self, name, args, lib):
        env = dict(os.environ)
        if lib:
            env["SLIM_AMD_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--users", str(args.users), "--row-nnz",
               str(args.row_nnz), "--old-users", str(args.old_users)]
        self.name, self.limit = name, args.limit
        self.child = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=env)
        self.pending = b""

    def answer(self, limit=None):
        """The next JSON line of the worker, None when it ends or stays silent for the limit."""
        fd = self.child.stdout.fileno()
        while True:
            while b"\n" in self.pending:
                raw, self.pending = self.pending.split(b"\n", 1)
                try:
                    return json.loads(raw.decode("utf-8", "replace"))
                except ValueError:
                    continue                  # (a trace line of the library)
            ready, _, _ = select.select([fd], [], [], limit or self.limit)
            chunk = os.read(fd, 1 << 16) if ready else b""
            if not chunk:
                return None
            self.pending += chunk

    def ask(self, kind, a, N, users):
        self.child.stdin.write(("%s %d %d %d\n" % (kind, a, N, users)).encode())
        self.child.stdin.flush()
        return self.answer()

    def end(self, kill):
        if self.child.poll() is None:
            if kill:
                self.child.kill()
            else:
                try:
                    self.child.stdin.write(b"quit\n")
                    self.child.stdin.flush()
                except OSError:
                    pass
        self.child.wait()


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libslim.so of the parent commit (omit: no comparison (a))")
    ap.add_argument("--users", type=int, default=131072)
    ap.add_argument("--old-users", type=int, default=8192, help="users of the runs of SLIMGPU_Predict1vsK")
    ap.add_argument("--big-users", type=int, default=16384, help="users of the runs at k = 4096 and k = 10 000")
    ap.add_argument("--row-nnz", type=int, default=2700)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds one run may take")
    ap.add_argument("--setup-limit", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "candidate_lists_c4.txt"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    U, UO, UB = args.users, min(args.users, args.old_users), min(args.users, args.big_users)
    workers = {"new": Worker("new", args, None)}
    if args.parent_lib:
        workers["parent"] = Worker("parent", args, args.parent_lib)
    rows, head, verdict = [], {}, "complete"
    # (name, worker, kind, k or 0, nrcmds, users); a set's first call is a run of its own before the rounds
    first = [("first cand k=%d" % k, "new", "cand", k, 64, U) for k in CAND_K]
    first += [("first cand k=%d/%d" % (k, UO), "new", "cand", k, 64, UO) for k in CAND_K]
    first += [("first cand k=4096/%d" % UB, "new", "cand", 4096, 4096, UB),
              ("first cand k=10000/%d" % UB, "new", "cand", 10000, 0, UB)]
    timed = []
    for N in LIST_N:
        if "parent" in workers:
            timed.append(("parent lists@%d" % N, "parent", "lists", 0, N, U))
        timed.append(("lists@%d" % N, "new", "lists", 0, N, U))
    for k in CAND_K:
        timed.append(("cand k=%d" % k, "new", "cand", k, 64, U))
    timed.append(("lists@64/%d" % UO, "new", "lists", 0, 64, UO))
    for k in CAND_K:
        timed.append(("cand k=%d/%d" % (k, UO), "new", "cand", k, 64, UO))
        timed.append(("old 1vsk k=%d/%d" % (k, UO), "new", "old", k, 64, UO))
    timed += [("cand k=4096 lists/%d" % UB, "new", "cand", 4096, 4096, UB),
              ("cand k=10000 scores/%d" % UB, "new", "cand", 10000, 0, UB)]
    try:
        for name, w in workers.items():
            head = w.answer(args.setup_limit)
            if not head or "ready" not in head:
                verdict = "worker %s did not get ready" % name
                break
            print(name, json.dumps(head), flush=True)
        for rnd, runs in [(-1, first)] + [(r, timed) for r in range(args.rounds)]:
            for name, wk, kind, a, N, users in runs if verdict == "complete" else ():
                row = workers[wk].ask(kind, a, N, users)
                if row is None or "failed" in row:
                    verdict = "run %s failed or overran its limit of %g s: job ended (%s)" % (name, args.limit, row)
                    break
                row = dict({"run": name, "round": rnd}, **row)
                print(json.dumps(row), flush=True)
                rows.append(row)
    finally:
        for w in workers.values():
            w.end(kill=verdict != "complete")
    secs, crcs = {}, {}
    for r in rows:
        if r["round"] >= 0:
            secs.setdefault(r["run"], []).append(r["seconds"])
            crcs.setdefault(r["run"], set()).add(r["crc"])
    lines = ["# scripts/cand_scale.py: %d rounds, %d runs, %s" % (args.rounds, len(rows), verdict),
             "# box: %s, %s; %s" % (platform.node(), head.get("gpu", "?") if head else "?", time.strftime("%Y-%m-%d")),
             "# model %d entries (100K x 100K, %d per row), %d users with %d history entries, resident; seconds = wall "
             "time of the call" % ((head or {}).get("model_nnz", 0), args.row_nnz, U, (head or {}).get("history_nnz", 0))]
    lines += [json.dumps(r) for r in rows]
    med = {k: median(v) for k, v in secs.items()}
    for k in sorted(med):
        lines.append("# %s: median %.3f s (min %.3f .. max %.3f)" % (k, med[k], min(secs[k]), max(secs[k])))
    ok = True
    for N in LIST_N:
        p, q = "parent lists@%d" % N, "lists@%d" % N
        if p in med and q in med:
            bound = max(secs[p]) + (max(secs[p]) - min(secs[p]))
            met = med[q] <= bound
            ok = ok and met
            lines.append("# (a) N = %d: this build %.3f s, bound %.3f s (the parent's slowest run %.3f + its spread %.3f): "
                         "%s; lists %s" % (N, med[q], bound, max(secs[p]), max(secs[p]) - min(secs[p]),
                                           "met" if met else "NOT met",
                                           "bit-equal" if crcs[p] == crcs[q] and len(crcs[q]) == 1 else "DIFFER"))
            ok = ok and crcs[p] == crcs[q]
        else:
            lines.append("# (a) N = %d: not measured (no parent library)" % N)
    for k in CAND_K:
        c, l = "cand k=%d" % k, "lists@64"
        if c in med and l in med:
            lines.append("# (b) k = %d, %d users: candidates %.3f s / lists@64 %.3f s = %.2f" % (k, U, med[c], med[l],
                                                                                              med[c] / med[l]))
        c, o, l = "cand k=%d/%d" % (k, UO), "old 1vsk k=%d/%d" % (k, UO), "lists@64/%d" % UO
        if c in med and o in med:
            lines.append("# (b) k = %d, %d users: candidates %.3f s, SLIMGPU_Predict1vsK %.3f s (old / new = %.1f), "
                         "lists@64 %.3f s; lists %s" % (k, UO, med[c], med[o], med[o] / med[c], med.get(l, 0),
                                                       "bit-equal" if crcs[c] == crcs[o] else "DIFFER"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(l for l in lines if l.startswith("#")))
    sys.exit(0 if verdict == "complete" and ok else 1)


if __name__ == "__main__":
    main()
