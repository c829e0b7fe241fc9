#!/usr/bin/env python3
"""Explanations at C4 scale: what it costs to say which history items carry a score (include/slim_gpu_explain.h).

The model and the users are those of scripts/cand_scale.py (a synthetic 100K x 100K model with 2700 entries per
row, the first 131 072 users of the synthetic C4 matrix), resident: the matrix staged, the model made resident
once.  Every user's own top 100 comes from one SLIMGPU_MatrixPredictLists; the top 10 are its first ten.  Two
candidate sets hold them.  One job, the runs alternating and repeated:

  score k = 10, 100               SLIMGPU_MatrixScoreCandidates on the set, slot scores down: the existing call that
                                  walks the same histories once and adds the terms
  explain k = 10, 100             SLIMGPU_MatrixExplainCandidates on the same set at nwhy = 3 and nwhy = 16

No figure is fixed in advance: the file records the seconds of the explanation beside the seconds of the scoring
call on the same set, and their ratio.  Seconds are wall time of the call; kernel_ms is slimgpu_eval_stats_t's.  A
set's first call makes its device copy and is reported apart ("first").  Every run has its own time limit; the job
ends at the first run that fails or overruns it.

  python scripts/explain_scale.py [--users 131072] [--rounds 2] [--out profiles/explain_c4.txt]
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

TOP_K = (10, 100)
NWHY = (3, 16)


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
    del wind, wval, wptr, R
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    top, _, counts = model.predict(mat, nrcmds=max(TOP_K), return_counts=True)
    sets = {}
    for kk in TOP_K:
        cnt = np.minimum(counts, kk).astype(np.int64)
        keep = np.arange(kk)[None, :] < cnt[:, None]
        ptr = np.concatenate((np.zeros(1, np.int64), np.cumsum(cnt)))
        sets[kk] = mat.candidate_set((ptr, top[:, :kk][keep]))
    gpu = "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"))
    print(json.dumps({"ready": True, "gpu": gpu, "users": U, "history_nnz": int(hind.size), "model_nnz": n * k,
                      "entries": {str(kk): int(sets[kk].size) for kk in TOP_K}}), flush=True)
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        kind, kk, nwhy = word[0], int(word[1]), int(word[2])
        cs = sets[kk]
        if kind == "score":
            out = (np.zeros(cs.size, np.float32),)
            t0 = time.time()
            rc = lib.SLIMGPU_MatrixScoreCandidates(model.handle, mat.handle, cs.handle, 0, None, 0, P(out[0]), None, None,
                                                   None)
        else:
            out = (np.full(cs.size * nwhy, -1, np.int32), np.zeros(cs.size * nwhy, np.float32),
                   np.zeros(cs.size, np.int32))
            t0 = time.time()
            rc = lib.SLIMGPU_MatrixExplainCandidates(model.handle, mat.handle, cs.handle, 0, None, nwhy, *[P(a) for a in out])
        dt = time.time() - t0
        if rc != 1:
            print(json.dumps({"failed": [kind, kk, nwhy], "error": _lib.last_error()}), flush=True)
            return 1
        crc = 0
        for a in out:
            crc = zlib.crc32(a.tobytes(), crc)
        st = eval_stats(lib)
        row = {"users": U, "entries": int(cs.size), "seconds": round(dt, 3), "kernel_ms": round(st["kernel_ms"], 1),
               "path": st["path"], "h2d_bytes": st["h2d_bytes"], "d2h_bytes": st["d2h_bytes"],
               "device_allocs": st["device_allocs"], "crc": crc}
        if kind == "explain":
            row["mean_support"] = round(float(out[2].mean()), 2)
        print(json.dumps(row), flush=True)
    return 0


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    import subprocess
    from cand_scale import Worker

    class ExplainWorker(Worker):      # cand_scale's pipe to a worker process, with this script's worker behind it
        def __init__(self, args):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--users", str(args.users), "--row-nnz",
                   str(args.row_nnz)]
            self.name, self.limit = "new", args.limit
            self.child = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE)
            self.pending = b""

    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=131072)
    ap.add_argument("--row-nnz", type=int, default=2700)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds one run may take")
    ap.add_argument("--setup-limit", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_c4.txt"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    return run(args, ExplainWorker(args))


def run(args, w):
    rows, head, verdict = [], {}, "complete"
    first = [("first score k=%d" % k, "score", k, 0) for k in TOP_K]
    first += [("first explain k=%d nwhy=%d" % (k, NWHY[0]), "explain", k, NWHY[0]) for k in TOP_K]
    timed = []
    for k in TOP_K:
        timed.append(("score k=%d" % k, "score", k, 0))
        timed += [("explain k=%d nwhy=%d" % (k, nw), "explain", k, nw) for nw in NWHY]
    try:
        head = w.answer(args.setup_limit)
        if not head or "ready" not in head:
            verdict = "the worker did not get ready"
        else:
            print(json.dumps(head), flush=True)
        for rnd, runs in [(-1, first)] + [(r, timed) for r in range(args.rounds)]:
            for name, kind, k, nw in runs if verdict == "complete" else ():
                row = w.ask(kind, k, nw, 0)
                if row is None or "failed" in row:
                    verdict = "run %s failed or overran its limit of %g s: job ended (%s)" % (name, args.limit, row)
                    break
                row = dict({"run": name, "round": rnd}, **row)
                print(json.dumps(row), flush=True)
                rows.append(row)
    finally:
        w.end(kill=verdict != "complete")
    head = head or {}
    secs, kern, crcs = {}, {}, {}
    for r in rows:
        if r["round"] >= 0:
            secs.setdefault(r["run"], []).append(r["seconds"])
            kern.setdefault(r["run"], []).append(r["kernel_ms"])
            crcs.setdefault(r["run"], set()).add(r["crc"])
    lines = ["# scripts/explain_scale.py: %d rounds, %d runs, %s" % (args.rounds, len(rows), verdict),
             "# box: %s, %s; %s" % (platform.node(), head.get("gpu", "?"), time.strftime("%Y-%m-%d")),
             "# model %d entries (100K x 100K, %d per row), %d users with %d history entries, resident; candidate sets: "
             "every user's own top k, %s entries; seconds = wall time of the call, outputs down"
             % (head.get("model_nnz", 0), args.row_nnz, args.users, head.get("history_nnz", 0),
                json.dumps(head.get("entries", {})))]
    lines += [json.dumps(r) for r in rows]
    for name in sorted(secs):
        lines.append("# %s: median %.3f s (min %.3f .. max %.3f), kernel %.1f ms; outputs %s" % (
            name, median(secs[name]), min(secs[name]), max(secs[name]), median(kern[name]),
            "equal in every round" if len(crcs[name]) == 1 else "DIFFER between rounds"))
    ok = all(len(c) == 1 for c in crcs.values())
    for k in TOP_K:
        s = "score k=%d" % k
        for nw in NWHY:
            e = "explain k=%d nwhy=%d" % (k, nw)
            if s in secs and e in secs:
                lines.append("# top %d, nwhy = %d: explanation %.3f s / scoring call %.3f s = %.2f (kernels: %.1f ms / "
                             "%.1f ms = %.2f)" % (k, nw, median(secs[e]), median(secs[s]), median(secs[e]) / median(secs[s]),
                                                  median(kern[e]), median(kern[s]), median(kern[e]) / median(kern[s])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(l for l in lines if l.startswith("#")))
    sys.exit(0 if verdict == "complete" and ok else 1)


if __name__ == "__main__":
    main()
