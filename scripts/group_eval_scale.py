#!/usr/bin/env python3
"""Per-group evaluation at C4 scale: what the group rows cost on top of the evaluation (include/slim_gpu_groups.h).

The model and the users are those of scripts/topn_scale.py / exposure_scale.py (a synthetic 100K x 100K model with
2700 entries per row, the first 131 072 users of the synthetic C4 matrix), resident.  The test rows hold one random
item per user.  One job, the compared calls alternating, every run under its own time limit:

  evalat K          SLIMGPU_ModelEvaluateAt on an eval set with cutoffs (10) or (5, 10, 20, 64), no groups set
  parent evalat K   the same call of the parent commit's library (--parent-lib), in a process of its own
  grouped K shape   the same call on the same eval set with groups set: 1 group; 8 balanced groups; 64 balanced groups;
                    8 groups with 99 % of the users in one.  The groups are set before the clock starts and cleared
                    after it stops.

(a) the unchanged call must stay inside the parent's slowest run plus the parent's own spread (max + (max - min)), the
rule of the filtered, candidate and sampler profiles.  (b) records the ratio of the grouped call to the ungrouped one
and slimgpu_eval_stats_t's kernel_ms (the time between the eval set's events) with and without groups.  What the byte
and chain counts predict: the group sums read the 40 * K * nsel bytes of records once more (5 - 21 MB here) and their
longest serial chain is the largest group, never longer than the chain over everybody that already runs.

No figure is fixed in advance.  Seconds are wall time of the call.  The first call of every kind is reported apart.
The job ends at the first run that fails or overruns.  C5 is not run by this script.

  python scripts/group_eval_scale.py [--users 131072] [--rounds 3] [--parent-lib libslim_parent.so]
"""
import argparse
import json
import os
import platform
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CUTS = ((10,), (5, 10, 20, 64))
SHAPES = ("1 group", "8 balanced", "64 balanced", "8 groups, 99% in one")


def group_shapes(U):
    import numpy as np
    u = np.arange(U)
    skewed = np.where(u % 100 == 0, 1 + (u // 100) % 7, 0)
    return [(np.zeros(U, np.int32), 1), ((u % 8).astype(np.int32), 8), ((u % 64).astype(np.int32), 64),
            (skewed.astype(np.int32), 8)]


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
    del wind, wval, wptr
    T = sp.csr_matrix((np.ones(U, np.float32), rng.integers(0, n, U).astype(np.int32), np.arange(U + 1)), shape=(U, n))
    fm = (np.bincount(hind, minlength=n) < 3).astype(np.int32)
    evs = [mat.evaluator(T, fmarker=fm, cutoffs=c) for c in CUTS]
    shapes = group_shapes(U)
    gpu = "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"))
    print(json.dumps({"ready": True, "gpu": gpu, "users": U, "ncols": n, "history_nnz": int(hind.size),
                      "model_nnz": n * k}), flush=True)
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        kind, a, s = word[0], int(word[1]), int(word[2])
        ev = evs[a]
        if kind == "grouped":
            ev.set_groups(*shapes[s])
        t0 = time.time()
        fig = ev.evaluate_at(model)
        dt = time.time() - t0
        st = eval_stats(lib)
        out = [np.array([f["hr"], f["arhr"], f["nvalid"]]) for f in fig]
        row = {"seconds": round(dt, 4), "kernel_ms": round(st["kernel_ms"], 3), "path": st["path"],
               "h2d_bytes": st["h2d_bytes"], "d2h_bytes": st["d2h_bytes"], "device_allocs": st["device_allocs"]}
        if kind == "grouped":
            rows = ev.group_figures()
            out += [np.array([r["hr"], r["arhr"], r["nvalid"]]) for g in rows for r in g]
            row["largest_group"] = max(g[0]["members"] for g in rows[:-1])
            ev.clear_groups()
        crc = 0
        for o in out:
            crc = zlib.crc32(np.ascontiguousarray(o).tobytes(), crc)
        row["crc"] = crc
        print(json.dumps(row), flush=True)
    return 0


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    from cand_scale import Worker

    class GroupWorker(Worker):      # cand_scale's pipe to a worker process, with this script's worker behind it
        def __init__(self, name, args, lib):
            env = dict(os.environ)
            if lib:
                env["SLIM_AMD_LIB"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--users", str(args.users), "--row-nnz",
                   str(args.row_nnz)]
            self.name, self.limit = name, args.limit
            self.child = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=env)
            self.pending = b""

    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libslim.so of the parent commit (omit: no comparison (a))")
    ap.add_argument("--users", type=int, default=131072)
    ap.add_argument("--row-nnz", type=int, default=2700)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds one run may take")
    ap.add_argument("--setup-limit", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_eval_c4.txt"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        sys.exit(worker(args))
    new = GroupWorker("new", args, None)
    old = GroupWorker("parent", args, args.parent_lib) if args.parent_lib else None
    rows, head, verdict = [], {}, "complete"
    runs = []
    for a, c in enumerate(CUTS):
        runs.append(("evalat %s" % (c,), new, "evalat", a, 0))
        if old:
            runs.append(("parent evalat %s" % (c,), old, "evalat", a, 0))
        runs += [("grouped %s, %s" % (c, SHAPES[s]), new, "grouped", a, s) for s in range(len(SHAPES))]
    try:
        for w in (new, old):
            got = w.answer(args.setup_limit) if w else {"ready": True}
            if not got or "ready" not in got:
                verdict = "a worker did not get ready"
            elif w is new:
                head = got
        for rnd in range(-1, args.rounds):
            for name, w, kind, a, s in runs if verdict == "complete" else ():
                row = w.ask(kind, a, s, 0)
                if row is None or "failed" in row:
                    verdict = "run %s failed or overran its limit of %g s: job ended" % (name, args.limit)
                    break
                row = dict({"run": name, "round": rnd}, **row)
                print(json.dumps(row), flush=True)
                rows.append(row)
    finally:
        for w in (new, old):
            if w:
                w.end(kill=verdict != "complete")
    secs, kern, crcs = {}, {}, {}
    for r in rows:
        if r["round"] >= 0:
            secs.setdefault(r["run"], []).append(r["seconds"])
            kern.setdefault(r["run"], []).append(r["kernel_ms"])
            crcs.setdefault(r["run"], set()).add(r["crc"])
    lines = ["# scripts/group_eval_scale.py: %d rounds after one first call of every kind, %d runs, %s"
             % (args.rounds, len(rows), verdict),
             "# box: %s, %s; %s" % (platform.node(), head.get("gpu", "?"), time.strftime("%Y-%m-%d")),
             "# model %d entries (100K x 100K, %d per row), %d users with %d history entries, resident; seconds = wall "
             "time of the call; C5: not measured" % (head.get("model_nnz", 0), args.row_nnz, args.users,
                                                     head.get("history_nnz", 0))]
    lines += [json.dumps(r) for r in rows]
    for name in sorted(secs):
        lines.append("# %s: median %.4f s (min %.4f .. max %.4f), kernel %.3f ms; outputs %s" % (
            name, median(secs[name]), min(secs[name]), max(secs[name]), median(kern[name]),
            "equal in every round" if len(crcs[name]) == 1 else "DIFFER between rounds"))
    for c in CUTS:
        plain, parent = "evalat %s" % (c,), "parent evalat %s" % (c,)
        if plain in secs and parent in secs:      # (a)
            p = secs[parent]
            bound = max(p) + (max(p) - min(p))
            lines.append("# (a) cutoffs %s: slowest unchanged call %.4f s, parent's slowest %.4f s + spread %.4f s = %.4f s: %s"
                         % (c, max(secs[plain]), max(p), max(p) - min(p), bound,
                            "inside" if max(secs[plain]) <= bound else "OUTSIDE"))
            lines.append("# (a) cutoffs %s: kernel_ms median %.3f, parent %.3f" % (c, median(kern[plain]),
                                                                                 median(kern[parent])))
        for s in SHAPES:                           # (b)
            name = "grouped %s, %s" % (c, s)
            if name in secs and plain in secs:
                lines.append("# (b) %s: %.4f s / %.4f s = %.4f; kernel_ms %.3f with groups, %.3f without: %+.3f ms" % (
                    name, median(secs[name]), median(secs[plain]), median(secs[name]) / median(secs[plain]),
                    median(kern[name]), median(kern[plain]), median(kern[name]) - median(kern[plain])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(l for l in lines if l.startswith("#")))
    sys.exit(0 if verdict == "complete" else 1)


if __name__ == "__main__":
    main()
