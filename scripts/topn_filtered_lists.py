#!/usr/bin/env python3
"""What a candidate filter (include/slim_gpu_filter.h) costs at C4 scale, and what carrying it costs the
unfiltered lists.

The model and the users are those of scripts/topn_long_lists.py (a synthetic 100K x 100K model with 2700 entries
per row, the first 131 072 users of the synthetic C4 matrix).  One job, the runs alternating and repeated, at
N = 64 (chunk kernel), 128 (wave kernel) and 1000 (long-list form):

  parent    SLIMGPU_PredictLists of another build of the library (--parent-lib: the parent commit's)
  plain     SLIMGPU_PredictLists of this build
  filtered  SLIMGPU_PredictListsFiltered of this build: a random 50 % allow set, 20 random exclusions per user

Seconds are wall time of the call: upload of the model and the histories, scoring, lists down (the call ends on a
device synchronise).  Every build has a worker process of its own, which holds the inputs and runs what it is
told, one run at a time; this process gives every run its own time limit and ends the job at the first run that
fails or overruns it.  Each worker warms every N up on 2 048 users first.  Claims recorded: (a) plain is no slower
than parent beyond the spread of the repeats themselves, (b) filtered equals plain within that spread.

  python scripts/topn_filtered_lists.py --parent-lib PATH [--users 131072] [--rounds 3] [--limit 300]
                                        [--out profiles/filtered_lists_c4.txt]
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

LIST_N = (64, 128, 1000)
WARM_USERS = 2048


def worker(args):
    import numpy as np
    import torch
    from slim_amd import _lib, synth
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
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hW, hH, hH2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.Py_csr_wrapper(n, wptr, wind, P(wval), C.byref(hW)) == 1
    assert lib.Py_csr_wrapper(U, hptr, hind, P(hval), C.byref(hH)) == 1
    U2 = min(U, WARM_USERS)
    assert lib.Py_csr_wrapper(U2, np.ascontiguousarray(hptr[:U2 + 1]), hind, P(hval), C.byref(hH2)) == 1
    # the filter: half of the items, 20 ids per user
    frng = np.random.default_rng(11)
    allowed = np.flatnonzero(frng.random(n) < 0.5).astype(np.int32)
    xind = frng.integers(0, n, size=20 * U, dtype=np.int32)
    xptr = np.arange(U + 1, dtype=np.int64) * 20
    flt = C.c_void_p()
    if hasattr(lib, "SLIMGPU_FilterCreate"):
        assert lib.SLIMGPU_FilterCreate(n, allowed.size, P(allowed), 0, U, P(xptr), P(xind), C.byref(flt)) == 1, \
            _lib.last_error()
    mask = np.zeros(n, bool)
    mask[allowed] = True

    def run(kind, N, hist, users):
        ids = np.full(users * N, -1, np.int32)
        sc = np.zeros(users * N, np.float32)
        cnt = np.zeros(users, np.int32)
        t0 = time.time()
        if kind == "filtered":
            rc = lib.SLIMGPU_PredictListsFiltered(N, hW, hist, flt, P(ids), P(sc), P(cnt))
        else:
            rc = lib.SLIMGPU_PredictLists(N, hW, hist, P(ids), P(sc), P(cnt))
        return rc, time.time() - t0, ids.reshape(users, N), sc, cnt

    for N in LIST_N:
        for kind in ("plain", "filtered") if flt.value else ("plain",):
            rc, _, _, _, _ = run(kind, N, hH2, U2)
            assert rc == 1, _lib.last_error()
    gpu = "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"))
    print(json.dumps({"ready": True, "gpu": gpu, "users": U, "history_nnz": int(hind.size),
                      "model_nnz": int(wind.size), "allowed": int(allowed.size)}), flush=True)
    checked = set()
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        kind, N = word[0], int(word[1])
        rc, dt, ids, sc, cnt = run(kind, N, hH, U)
        if rc != 1:
            print(json.dumps({"failed": [kind, N], "error": _lib.last_error()}), flush=True)
            return 1
        row = {"N": N, "users": U, "seconds": round(dt, 3), "users_per_s": round(U / dt, 1),
               "lists": int(cnt.sum()), "crc": zlib.crc32(sc.tobytes(), zlib.crc32(ids.tobytes()))}
        if kind == "filtered" and N not in checked:   # (once per N: nothing barred is in a list)
            checked.add(N)
            got = ids >= 0
            ok = bool(mask[ids[got]].all())
            for r in range(min(N, 20)):               # rank by rank against the users' 20 exclusions
                col = ids[:, r]
                ok = ok and not bool((xind.reshape(U, 20) == col[:, None])[col >= 0].any())
            row["only_allowed_and_top20_not_excluded"] = ok
        print(json.dumps(row), flush=True)
    return 0


class Worker(object):
    def __init__(self, name, args, lib):
        env = dict(os.environ)
        if lib:
            env["SLIM_AMD_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--users", str(args.users), "--row-nnz",
               str(args.row_nnz)]
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

    def ask(self, kind, N):
        self.child.stdin.write(("%s %d\n" % (kind, N)).encode())
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
    ap.add_argument("--row-nnz", type=int, default=2700)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds one run may take")
    ap.add_argument("--setup-limit", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_lists_c4.txt"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    workers = {"new": Worker("new", args, None)}
    if args.parent_lib:
        workers["parent"] = Worker("parent", args, args.parent_lib)
    rows, head, verdict = [], {}, "complete"
    try:
        for name, w in workers.items():
            head = w.answer(args.setup_limit)
            if not head or "ready" not in head:
                verdict = "worker %s did not get ready" % name
                break
            print(name, json.dumps(head), flush=True)
        for rnd in range(args.rounds if verdict == "complete" else 0):
            for N in LIST_N:
                for run in ("parent", "plain", "filtered"):
                    if run == "parent" and "parent" not in workers:
                        continue
                    w = workers["parent" if run == "parent" else "new"]
                    row = w.ask("plain" if run == "parent" else run, N)
                    if row is None or "failed" in row:
                        verdict = "run %s@%d failed or overran its limit of %g s: job ended (%s)" % (run, N, args.limit, row)
                        break
                    row = dict({"run": run, "round": rnd}, **row)
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                if verdict != "complete":
                    break
            if verdict != "complete":
                break
    finally:
        for w in workers.values():
            w.end(kill=verdict != "complete")
    secs, crcs = {}, {}
    for r in rows:
        secs.setdefault((r["run"], r["N"]), []).append(r["seconds"])
        crcs.setdefault((r["run"], r["N"]), set()).add(r["crc"])
    lines = ["# scripts/topn_filtered_lists.py: %d rounds, %d runs, %s" % (args.rounds, len(rows), verdict),
             "# box: %s, %s; %s" % (platform.node(), head.get("gpu", "?") if head else "?", time.strftime("%Y-%m-%d")),
             "# model %d entries (100K x 100K, %d per row), %d users with %d history entries; the filter: %d of the items "
             "allowed, 20 exclusions per user; seconds = wall time of the call (upload, scoring, lists down)"
             % ((head or {}).get("model_nnz", 0), args.row_nnz, (head or {}).get("users", 0),
                (head or {}).get("history_nnz", 0), (head or {}).get("allowed", 0))]
    lines += [json.dumps(r) for r in rows]
    for N in LIST_N:
        part = []
        for run in ("parent", "plain", "filtered"):
            v = secs.get((run, N))
            if v:
                part.append("%s %.3f (%.3f .. %.3f)" % (run, median(v), min(v), max(v)))
        lines.append("# N = %d, median seconds (min .. max): %s" % (N, ", ".join(part)))
        if ("parent", N) in secs and ("plain", N) in secs:
            same = crcs[("parent", N)] == crcs[("plain", N)] and len(crcs[("plain", N)]) == 1
            lines.append("#   (a) plain / parent = %.3f; spread of the repeats: parent %.1f %%, plain %.1f %%; lists %s"
                         % (median(secs[("plain", N)]) / median(secs[("parent", N)]),
                            100 * (max(secs[("parent", N)]) / min(secs[("parent", N)]) - 1),
                            100 * (max(secs[("plain", N)]) / min(secs[("plain", N)]) - 1),
                            "bit-equal" if same else "DIFFER"))
        if ("filtered", N) in secs and ("plain", N) in secs:
            lines.append("#   (b) filtered / plain = %.3f; spread of the repeats: filtered %.1f %%"
                         % (median(secs[("filtered", N)]) / median(secs[("plain", N)]),
                            100 * (max(secs[("filtered", N)]) / min(secs[("filtered", N)]) - 1)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(l for l in lines if l.startswith("#")))
    sys.exit(0 if verdict == "complete" else 1)


if __name__ == "__main__":
    main()
