#!/usr/bin/env python3
"""Host overhead of the scorers' entry points where the kernels are short, and their equality between two builds.

On the golden ml100k split (934 users, 1683 items) a call is mostly its host code: argument checks, staging, events,
statistics.  One model is learned once and saved; every run loads it.  Then, --rounds times, the parent commit's
library (--parent-lib) and this build run one after the other, each in a process of its own under its own time
limit.  A run times each of five calls --reps times after --warmup calls:

  evaluate_at      SLIMGPU_ModelEvaluateAt, cutoffs 5, 10, 20
  ranked           SLIMGPU_ModelEvaluateRanked, cutoffs 1, 5, 10, 20, 50
  candidates       SLIMGPU_ModelEvaluateCandidates, 20 candidates per user, cutoffs 5, 10, 20
  lists16          SLIMGPU_MatrixPredictLists, 10 places, a list of 16 users
  score_cands      SLIMGPU_MatrixScoreCandidates, every user, lists of 10 and the slot scores

Pass / fail, per call: the median of this build's per-round medians is no slower than the parent's slowest round
plus the parent's own spread (max + (max - min) of its per-round medians).  And, for the first and for the second
run of every call in every round, the deterministic fields of slimgpu_eval_stats_t (path, device_allocs, d2h_bytes,
h2d_bytes, w_rows_read, w_bytes), slices and path of slimgpu_list_stats_t and the checksum of everything the call
returned are equal between the two builds, field by field.  Any difference fails the job.

  python scripts/call_overhead.py --parent-lib PATH [--rounds 3] [--out profiles/call_frame_ab.txt]
"""
import argparse
import ctypes as C
import json
import os
import platform
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
CALLS = ("evaluate_at", "ranked", "candidates", "lists16", "score_cands")
FIELDS = ("path", "device_allocs", "d2h_bytes", "h2d_bytes", "w_rows_read", "w_bytes")


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def split():
    from slim_amd.io import read_csr_text
    R = read_csr_text(os.path.join(GOLDEN, "ml100k-train.csr"))
    return R, read_csr_text(os.path.join(GOLDEN, "ml100k-test.csr"), nrows=R.shape[0])


def learn(path):
    """The model of the job, learned once (this build; the solver is not what is compared) and saved."""
    import scipy.sparse as sp
    import torch  # noqa: F401  (before the library, as everywhere)
    from slim_amd.engine import DeviceMatrix
    R, _ = split()
    mat = DeviceMatrix.from_scipy(R)
    W, _ = mat.learn(l1r=1.0, l2r=1.0, niters=100, seed=1)
    W = sp.csr_matrix(W)
    W.sort_indices()
    sp.save_npz(path, W)
    mat.close()
    print(json.dumps({"model_nnz": int(W.nnz)}), flush=True)
    return 0


def worker(args):
    import numpy as np
    import scipy.sparse as sp
    import torch
    from slim_amd import _lib
    from slim_amd.engine import DeviceMatrix, eval_stats, list_stats
    lib = _lib.load()
    R, T = split()
    nu, ni = R.shape
    mat = DeviceMatrix.from_scipy(R)
    model = mat.model_from_scipy(sp.load_npz(args.model))
    ev = mat.evaluator(T, cutoffs=(5, 10, 20))
    rk = mat.evaluator(T, ranked=True)
    k = 20
    cand = ((np.arange(nu, dtype=np.int64)[:, None] * 13 + np.arange(k, dtype=np.int64)[None, :] * 83) % ni)
    cset = mat.candidate_set((np.arange(nu + 1, dtype=np.int64) * k, cand.astype(np.int32).ravel()))
    users = np.arange(16, dtype=np.int32) * 57 + 3
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    met, nv = np.zeros(4 * 8), np.zeros(3 * 8, np.int32)
    rcut = np.array([1, 5, 10, 20, 50], np.int32)
    ids, sc, cnt = np.zeros(nu * 10, np.int32), np.zeros(nu * 10, np.float32), np.zeros(nu, np.int32)
    slot = np.zeros(nu * k, np.float32)
    calls = {
        "evaluate_at": (lambda: lib.SLIMGPU_ModelEvaluateAt(ev.handle, model.handle, 3, met, nv), (met, nv)),
        "ranked": (lambda: lib.SLIMGPU_ModelEvaluateRanked(rk.handle, model.handle, 5, P(rcut), met, nv), (met, nv)),
        "candidates": (lambda: lib.SLIMGPU_ModelEvaluateCandidates(ev.handle, model.handle, cset.handle, 3, met, nv),
                       (met, nv)),
        "lists16": (lambda: lib.SLIMGPU_MatrixPredictLists(10, model.handle, mat.handle, 16, P(users), P(ids), P(sc),
                                                           P(cnt)), (ids, sc, cnt)),
        "score_cands": (lambda: lib.SLIMGPU_MatrixScoreCandidates(model.handle, mat.handle, cset.handle, 0, None, 10,
                                                                  P(slot), P(ids), P(sc), P(cnt)), (slot, ids, sc, cnt)),
    }
    gpu = "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"))
    out = {"gpu": gpu, "users": nu, "items": ni, "model_nnz": model.nnz, "calls": {}}
    for name in CALLS:
        call, outputs = calls[name]
        facts, secs = [], []
        for i in range(args.warmup + args.reps):
            for a in outputs:
                a[:] = 0
            t0 = time.perf_counter()
            rc = call()
            dt = time.perf_counter() - t0
            if rc != 1:
                print(json.dumps({"failed": name, "error": _lib.last_error()}), flush=True)
                return 1
            if i < 2:       # the first and the second run: what must be equal between the builds
                st, ls = eval_stats(lib), list_stats(lib)
                f = {key: st[key] for key in FIELDS}
                if name == "lists16":
                    f.update(list_slices=ls["slices"], list_path=ls["path"])
                crc = 0
                for a in outputs:
                    crc = zlib.crc32(a.tobytes(), crc)
                f["crc"] = crc
                facts.append(f)
            if i >= args.warmup:
                secs.append(dt * 1e6)
        out["calls"][name] = {"facts": facts, "median_us": round(median(secs), 2), "min_us": round(min(secs), 2),
                              "p90_us": round(sorted(secs)[int(0.9 * len(secs))], 2), "max_us": round(max(secs), 2)}
    print(json.dumps(out), flush=True)
    return 0


def run(mode, args, model, lib=None):
    """One process of its own under the time limit; its last JSON line, or None."""
    env = dict(os.environ)
    if lib:
        env["SLIM_AMD_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), mode, "--model", model, "--reps", str(args.reps), "--warmup",
           str(args.warmup)]
    try:
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=args.limit)
    except subprocess.TimeoutExpired:
        return None
    row = None
    for raw in p.stdout.decode("utf-8", "replace").splitlines():
        try:
            row = json.loads(raw)
        except ValueError:
            continue
    return row if p.returncode == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libslim.so of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds one process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "call_frame_ab.txt"))
    ap.add_argument("--model", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--learn", action="store_true")
    args = ap.parse_args()
    if args.learn:
        sys.exit(learn(args.model))
    if args.worker:
        sys.exit(worker(args))
    if not args.parent_lib:
        ap.error("--parent-lib is needed: the job is a comparison")
    rows, verdict, head = [], "complete", {}
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "model.npz")
        if run("--learn", args, model) is None:
            verdict = "the model could not be learned"
        for rnd in range(args.rounds if verdict == "complete" else 0):
            for build, lib in (("parent", args.parent_lib), ("this", None)):
                row = run("--worker", args, model, lib)
                if row is None or "failed" in row:
                    verdict = "round %d, build %s failed or overran its limit of %g s: job ended (%s)" % (
                        rnd, build, args.limit, row)
                    break
                head = row
                rows.append(dict(row, build=build, round=rnd))
                print(json.dumps(rows[-1]), flush=True)
            if verdict != "complete":
                break
    lines = ["# scripts/call_overhead.py: %d rounds, %d calls timed after %d, %s" % (args.rounds, args.reps, args.warmup,
                                                                                   verdict),
             "# box: %s, %s; %s" % (platform.node(), head.get("gpu", "?"), time.strftime("%Y-%m-%d")),
             "# golden ml100k: %s users, %s items, model of %s entries; microseconds = wall time of one call"
             % (head.get("users"), head.get("items"), head.get("model_nnz"))]
    lines += [json.dumps(r) for r in rows]
    ok = verdict == "complete"
    for name in CALLS if ok else ():
        med = {b: [r["calls"][name]["median_us"] for r in rows if r["build"] == b] for b in ("parent", "this")}
        for b in ("parent", "this"):
            lines.append("# %s, %s: per-round medians %s us (fastest call %.1f, slowest %.1f)" % (
                name, b, med[b], min(r["calls"][name]["min_us"] for r in rows if r["build"] == b),
                max(r["calls"][name]["max_us"] for r in rows if r["build"] == b)))
        p = med["parent"]
        bound = max(p) + (max(p) - min(p))
        met = median(med["this"]) <= bound
        facts = {b: [r["calls"][name]["facts"] for r in rows if r["build"] == b] for b in ("parent", "this")}
        diff = []
        for rnd, (fp, ft) in enumerate(zip(facts["parent"], facts["this"])):
            for i in (0, 1):
                diff += ["round %d run %d %s: parent %s, this %s" % (rnd, i + 1, key, fp[i][key], ft[i][key])
                         for key in fp[i] if fp[i][key] != ft[i].get(key)]
        lines.append("# %s: this build %.1f us, bound %.1f us (the parent's slowest round %.1f + its spread %.1f): %s; "
                     "first and second run: %s" % (name, median(med["this"]), bound, max(p), max(p) - min(p),
                                                   "met" if met else "NOT met",
                                                   "every field and checksum equal" if not diff else "DIFFER"))
        lines += ["#   " + d for d in diff]
        ok = ok and met and not diff
    lines.append("# verdict: %s" % ("PASS" if ok else "FAIL"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
