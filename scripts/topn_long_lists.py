#!/usr/bin/env python3
"""Top-N lists of more than 128 at C4 scale: what the long-list form of the chunk scorer costs.

The model and the users are those of scripts/topn_scale.py (a synthetic 100K x 100K model with 2700 entries
per row, the first 131 072 users of the synthetic C4 matrix).  One job, the runs alternating and repeated:

  chunk  N = 64                               SLIMGPU_Predict, the chunk kernel
  wave   N = 128                              SLIMGPU_Predict, the wave kernel
  long   N = 64, 128, 129, 200, 500, 1000, 4096   SLIMGPU_PredictLists (SLIM_TOPN_KERNEL=long up to 128),
                                              with slimgpu_list_stats_t of every run
  host   N = 200, 2 048 users                 Py_SLIM_Predict under SLIM_PREDICT=cpu

Seconds are wall time of the call: upload of the model and the histories, scoring, lists down.  The runs
happen in one worker process; this process gives every run its own time limit and ends the job at the first
run that fails or overruns it.  The figure to meet: long N = 200 takes no longer than wave N = 128.

  python scripts/topn_long_lists.py [--users 131072] [--rounds 2] [--limit 300] [--out profiles/long_lists_c4.txt]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LONG_N = (64, 128, 129, 200, 500, 1000, 4096)
HOST_USERS, HOST_N = 2048, 200


def plan(rounds):
    runs = []
    for r in range(rounds):
        runs.append(("chunk", 64, r))
        runs.append(("long", 64, r))
        runs.append(("wave", 128, r))
        for n in LONG_N[1:]:
            runs.append(("long", n, r))
    runs.append(("host", HOST_N, 0))
    return runs


def worker(args):
    import numpy as np
    import torch
    from slim_amd import _lib, synth
    from slim_amd.engine import list_stats
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    nrows, ncols, target = synth.CONFIGS["c4"]
    rowptr, rowind, _ = synth.generate_csr(nrows, ncols, target, seed=1, device=dev)
    U = args.users
    hptr = rowptr[:U + 1].cpu().numpy().astype(np.intp)
    hind = rowind[:int(hptr[-1])].cpu().numpy()
    hval = np.ones(hind.size, np.float32)
    del rowptr, rowind
    torch.cuda.empty_cache()
    n, k = ncols, args.row_nnz
    rng = np.random.default_rng(5)
    wind = ((np.arange(n, dtype=np.int64)[:, None] * 7 + np.arange(k, dtype=np.int64)[None, :] * 37) % n)
    wind = np.sort(wind, axis=1).astype(np.int32).ravel()
    wval = (rng.random(n * k, dtype=np.float32) * 0.01).astype(np.float32)
    wptr = (np.arange(n + 1, dtype=np.int64) * k).astype(np.intp)
    hW, hH, hH2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.Py_csr_wrapper(n, wptr, wind, wval.ctypes.data_as(C.c_void_p), C.byref(hW)) == 1
    assert lib.Py_csr_wrapper(U, hptr, hind, hval.ctypes.data_as(C.c_void_p), C.byref(hH)) == 1
    U2 = min(U, HOST_USERS)
    assert lib.Py_csr_wrapper(U2, np.ascontiguousarray(hptr[:U2 + 1]), hind, hval.ctypes.data_as(C.c_void_p),
                              C.byref(hH2)) == 1
    gpu = "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"))
    print(json.dumps({"ready": True, "gpu": gpu, "users": U, "history_nnz": int(hind.size),
                      "model_nnz": int(wind.size)}), flush=True)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    kept = {}
    for kind, N, rnd in plan(args.rounds):
        users = U2 if kind == "host" else U
        ids = np.full(users * N, -1, np.int32)
        sc = np.zeros(users * N, np.float32)
        env = {"wave": {"SLIM_TOPN_KERNEL": "wave"}, "host": {"SLIM_PREDICT": "cpu"},
               "long": {"SLIM_TOPN_KERNEL": "long"} if N <= 128 else {}}.get(kind, {})
        os.environ.update(env)
        t0 = time.time()
        if kind == "long":
            rc = lib.SLIMGPU_PredictLists(N, hW, hH, P(ids), P(sc), None)
        elif kind == "host":
            rc = lib.Py_SLIM_Predict(N, hW, hH2, ids, sc)
        else:
            rc = lib.SLIMGPU_Predict(N, hW, hH, ids, sc)
        dt = time.time() - t0
        for key in env:
            del os.environ[key]
        if rc != 1:
            print(json.dumps({"failed": [kind, N, rnd], "error": _lib.last_error()}), flush=True)
            return 1
        row = {"run": kind, "N": N, "round": rnd, "users": users, "seconds": round(dt, 3),
               "users_per_s": round(users / dt, 1)}
        if kind == "long":
            row["stats"] = list_stats(lib)
            assert row["stats"]["path"] == 4
        # the runs check each other: one total order, so a shorter list is the head of a longer one
        ids, sc = ids.reshape(users, N), sc.reshape(users, N)
        if rnd == 0 and (kind, N) in (("chunk", 64), ("wave", 128)):
            kept[N] = (ids, sc)
        if kind == "long" and rnd == 0:
            ref_n = 64 if N == 64 else 128
            if N >= ref_n and ref_n in kept:
                row["head_equals_%s_%d" % ("chunk" if ref_n == 64 else "wave", ref_n)] = bool(
                    np.array_equal(ids[:, :ref_n], kept[ref_n][0]) and np.array_equal(sc[:, :ref_n], kept[ref_n][1]))
            if N == HOST_N:
                kept["long"] = (ids[:U2].copy(), sc[:U2].copy())
        if kind == "host" and "long" in kept:
            row["equals_long_%d" % HOST_N] = bool(np.array_equal(ids, kept["long"][0]) and
                                                 np.array_equal(sc, kept["long"][1]))
        del ids, sc
        print(json.dumps(row), flush=True)
    print(json.dumps({"done": True}), flush=True)
    return 0


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=131072)
    ap.add_argument("--row-nnz", type=int, default=2700)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds one run may take (and the set-up)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_lists_c4.txt"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--users", str(args.users), "--row-nnz",
           str(args.row_nnz), "--rounds", str(args.rounds)]
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE)
    fd = child.stdout.fileno()
    rows, head, verdict = [], {}, "complete"
    pending, over = b"", False
    try:
        while not over:
            ready, _, _ = select.select([fd], [], [], args.limit)   # the limit runs from the last line seen
            if not ready:
                verdict = "a run overran its limit of %g s: job ended" % args.limit
                break
            chunk = os.read(fd, 1 << 16)
            if not chunk:
                verdict = "the worker ended early (exit %s)" % child.wait()
                break
            pending += chunk
            while b"\n" in pending and not over:
                raw, pending = pending.split(b"\n", 1)
                try:
                    row = json.loads(raw.decode("utf-8", "replace"))
                except ValueError:
                    continue                  # (a trace line of the library)
                print(json.dumps(row), flush=True)
                if "ready" in row:
                    head = row
                elif "failed" in row:
                    verdict = "run %s failed: %s" % (row["failed"], row.get("error", ""))
                    over = True
                elif "done" in row:
                    over = True
                else:
                    rows.append(row)
    finally:
        if child.poll() is None and verdict != "complete":
            child.kill()
        child.wait()
    runs = [r for r in rows if "run" in r]
    secs = {}
    for r in runs:
        secs.setdefault((r["run"], r["N"]), []).append(r["seconds"])
    lines = ["# scripts/topn_long_lists.py: %d rounds, %d runs, %s" % (args.rounds, len(runs), verdict),
             "# box: %s, %s; %s" % (platform.node(), head.get("gpu", "?"), time.strftime("%Y-%m-%d")),
             "# model %d entries (100K x 100K, %d per row), %d users with %d history entries; seconds = wall time of "
             "the call (upload, scoring, lists down)" % (head.get("model_nnz", 0), args.row_nnz, head.get("users", 0),
                                                         head.get("history_nnz", 0))]
    lines += [json.dumps(r) for r in runs]
    med = {k: median(v) for k, v in secs.items()}
    lines.append("# medians (seconds): " + ", ".join("%s@%d %.3f" % (k[0], k[1], v) for k, v in sorted(med.items())))
    ok = True
    if ("long", 200) in med and ("wave", 128) in med:
        ok = med[("long", 200)] <= med[("wave", 128)]
        lines.append("# figure to meet: long@200 %.3f s %s wave@128 %.3f s -- %s" % (
            med[("long", 200)], "<=" if ok else ">", med[("wave", 128)], "met" if ok else "NOT met"))
    else:
        ok = False
        lines.append("# figure to meet: not measured")
    if ("long", 64) in med and ("chunk", 64) in med:
        lines.append("# recorded: long@64 / chunk@64 = %.2f (selection by threshold over insertion)" % (
            med[("long", 64)] / med[("chunk", 64)]))
    if ("long", 128) in med and ("wave", 128) in med:
        lines.append("# recorded: wave@128 / long@128 = %.2f" % (med[("wave", 128)] / med[("long", 128)]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(l for l in lines if l.startswith("#")))
    sys.exit(0 if verdict == "complete" and ok else 1)


if __name__ == "__main__":
    main()
