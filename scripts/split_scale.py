#!/usr/bin/env python3
"""The device split at scale (include/slim_gpu_split.h, slim_amd/csrc/split.hip) and the unchanged grid beside it.

One job, the calls alternated, medians of `--rounds` rounds (3):

  the split call   SLIMGPU_MatrixSplit on the C4-shaped synthetic matrix of scripts/topn_scale.py (binary, generated
                   on the device), both modes: wall time of the call, time of its kernels (the mark pass with the scan, and the
                   scatter pass: slimgpu_eval_stats_t.kernel_ms) and of the staging of the train half that the call
                   includes; against (a) a device-to-device copy of the same CSR bytes -- the floor of a pass that
                   reads and rewrites the matrix -- and (b) SLIMGPU_SplitHost plus SLIMGPU_MatrixFromHost of its train
                   half, which is what a caller without the device split pays (--host-rounds, 1: it takes a host
                   thread tens of seconds at 10^9 entries).  The kernels' bytes are the byte model of DESIGN.md:
                   per entry 4 read + 1 written by the mark pass (1 more cleared first), 1 + 4 read and 4 written by
                   the scatter pass; 8 more per entry with ratings.
  the grid         Py_SLIM_Mselect on the ml100k fixture, this build against another build of the library
                   (--parent-lib, the parent commit's), each in a fresh process, alternated.

  python scripts/split_scale.py [--config c4-0.1pct|c4] [--rounds 3] [--parent-lib path] [--out profiles/split_c4.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID_CODE = r"""
import ctypes as C, json, sys, time
sys.path.insert(0, %r)
import numpy as np
from slim_amd import _lib
from slim_amd.engine import make_options
from slim_amd.constants import Opt
from slim_amd.io import read_csr_text
lib = _lib.load()
R = read_csr_text(%r)
T = read_csr_text(%r, nrows=R.shape[0])
def wrap(M):
    h = C.c_void_p()
    lib.Py_csr_wrapper(M.shape[0], np.ascontiguousarray(M.indptr, np.intp), np.ascontiguousarray(M.indices, np.int32),
                       np.ascontiguousarray(M.data, np.float32).ctypes.data_as(C.c_void_p), C.byref(h))
    return h
ht, hs = wrap(R), wrap(T)
times = []
for rep in range(3):
    iopt, dopt = make_options(niters=200, seed=1)
    iopt[Opt.NRCMDS] = 10
    best = [C.c_double(0.0) for _ in range(8)]
    t0 = time.perf_counter()
    rc = lib.Py_SLIM_Mselect(ht, hs, iopt, dopt, np.array([1.0, 2.0, 5.0]), np.array([1.0, 5.0, 10.0]), 3, 3,
                             *[C.byref(b) for b in best])
    times.append(time.perf_counter() - t0)
    assert rc == 1, _lib.last_error()
print("GRID " + json.dumps({"seconds": times, "best": [b.value for b in best]}))
"""


def grid_run(lib_path):
    """Py_SLIM_Mselect three times in a fresh process on the given build: (seconds of the last two, the outputs)."""
    golden = os.path.join(ROOT, "tests", "golden")
    code = GRID_CODE % (ROOT, os.path.join(golden, "ml100k-train.csr"), os.path.join(golden, "ml100k-test.csr"))
    env = dict(os.environ)
    if lib_path:
        env["SLIM_AMD_LIB"] = lib_path
    else:
        env.pop("SLIM_AMD_LIB", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("grid run failed: " + r.stderr[-2000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("GRID ")][-1]
    rec = json.loads(line[5:])
    return rec["seconds"][1:], rec["best"]      # (the first call of a process loads code objects: warm-up)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4-0.1pct")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_c4.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("split_scale.py measures on the GPU: no device found")
    from slim_amd import _lib, synth
    from slim_amd.engine import DeviceMatrix, eval_stats, make_split
    import ctypes as C
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    nrows, ncols, target = synth.CONFIGS[args.config]
    rowptr, rowind, _ = synth.generate_csr(nrows, ncols, target, seed=1, device=dev)
    nnz = int(rowptr[-1].item())
    t0 = time.perf_counter()
    mat = DeviceMatrix.from_device_ptrs(nrows, ncols, rowptr.data_ptr(), rowind.data_ptr(), 0, keepalive=(rowptr, rowind))
    say("matrix %s: %d rows, %d items, %d entries, binary; staged in %.2f s (longest row %d, mean %.1f)"
        % (args.config, nrows, ncols, nnz, time.perf_counter() - t0, int(torch.diff(rowptr).max().item()), nnz / nrows))
    csr_bytes = 4 * nnz + 8 * (nrows + 1)
    model_bytes = 14 * nnz + 4 * 8 * (nrows + 1)    # the kernels' byte model, binary (see the docstring)
    specs = {"leave_out": dict(mode="leave_out", nfolds=5, fold=2, nheld=1, minkeep=1, seed=1),
             "folds": dict(mode="folds", nfolds=5, fold=2, minkeep=1, seed=1)}
    src = torch.empty(csr_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    rec = {k: {"wall": [], "kernel": [], "held": 0} for k in specs}
    copy_ms = []
    for rnd in range(args.rounds + 1):     # round 0 warms every call up and is not counted
        for name, spec in specs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trn, tst = mat.split(**spec)
            wall = time.perf_counter() - t0
            st = eval_stats()
            assert st["h2d_bytes"] == 0
            if rnd:
                rec[name]["wall"].append(wall * 1e3)
                rec[name]["kernel"].append(st["kernel_ms"])
            rec[name].update(held=int(tst.nnz), d2h=int(st["d2h_bytes"]), kept=int(trn.nnz))
            trn.close()
            del tst
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            copy_ms.append(e0.elapsed_time(e1))
    del src, dst
    med = statistics.median
    c = med(copy_ms)
    say("device-to-device copy of the CSR bytes (%d): median %.3f ms of %s -> %.0f GB/s read + written"
        % (csr_bytes, c, ["%.3f" % x for x in copy_ms], 2 * csr_bytes / c / 1e6))
    for name in specs:
        r = rec[name]
        k, w = med(r["kernel"]), med(r["wall"])
        say("split %-9s held %d of %d entries (%d bytes down, 0 up): kernels median %.3f ms of %s = %.2f copies, "
            "%.0f GB/s of the byte model (%d bytes); call wall median %.1f ms of %s (the rest stages the train half)"
            % (name, r["held"], nnz, r["d2h"], k, ["%.3f" % x for x in r["kernel"]], k / c, model_bytes / k / 1e6,
               model_bytes, w, ["%.1f" % x for x in r["wall"]]))
    # (b) what a caller pays today: the rows on the host, SLIMGPU_SplitHost, SLIMGPU_MatrixFromHost of the train half
    if args.host_rounds > 0:
        hptr = rowptr.cpu().numpy().astype(np.intp)
        hind = rowind.cpu().numpy()
        h = C.c_void_p()
        assert lib.Py_csr_wrapper(nrows, hptr, hind, None, C.byref(h)) == 1
        for name, spec in specs.items():
            split_s, stage_s = [], []
            for _ in range(args.host_rounds):
                s = make_split(**{"nheld": 1, **spec})
                a, b = C.c_void_p(), C.c_void_p()
                t0 = time.perf_counter()
                assert lib.SLIMGPU_SplitHost(h, C.byref(s), C.byref(a), C.byref(b)) == 1
                t1 = time.perf_counter()
                v = C.cast(a, C.POINTER(_lib.CsrView)).contents
                n = int(np.ctypeslib.as_array(v.rowptr, shape=(nrows + 1,))[-1])
                iopt = np.full(40, -1, np.int32)
                stt = C.c_int32(0)
                ptr = np.ctypeslib.as_array(v.rowptr, shape=(nrows + 1,)).astype(np.intp)
                ind = np.ctypeslib.as_array(v.rowind, shape=(n,))
                t2 = time.perf_counter()
                m = lib.SLIMGPU_MatrixFromHost(nrows, ptr, ind, None, iopt.ctypes.data_as(C.c_void_p), C.byref(stt))
                t3 = time.perf_counter()
                assert m
                mm = C.c_void_p(m)
                lib.SLIMGPU_MatrixFree(C.byref(mm))
                lib.Py_csr_free(a)
                lib.Py_csr_free(b)
                split_s.append(t1 - t0)
                stage_s.append(t3 - t2)
            say("host  %-9s SLIMGPU_SplitHost median %.2f s + SLIMGPU_MatrixFromHost of its train half %.2f s "
                "(one host thread, %d bytes up) against the device call's %.1f ms"
                % (name, med(split_s), med(stage_s), 4 * rec[name]["kept"] + 8 * (nrows + 1), med(rec[name]["wall"])))
        lib.Py_csr_free(h)
    mat.close()
    # the unchanged grid, this build against the parent's, alternated
    if args.parent_lib:
        runs = {"parent": [], "this": []}
        outs = {}
        for _ in range(args.rounds):
            for who, path in (("parent", os.path.abspath(args.parent_lib)), ("this", None)):
                secs, best = grid_run(path)
                runs[who].extend(secs)
                outs[who] = best
        p, t = runs["parent"], runs["this"]
        spread = max(p) - min(p)
        say("Py_SLIM_Mselect, ml100k, 3 x 3 pairs: parent median %.3f s (min %.3f max %.3f), this build median %.3f s "
            "(min %.3f max %.3f); the yardstick, parent's slowest + parent's spread, is %.3f s: %s; same outputs: %s"
            % (med(p), min(p), max(p), med(t), min(t), max(t), max(p) + spread,
               "inside" if max(t) <= max(p) + spread else "OUTSIDE", outs["parent"] == outs["this"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
