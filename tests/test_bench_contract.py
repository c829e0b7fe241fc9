"""bench.py's contract pieces that can be checked without a GPU: the default configuration is
the one BASELINE.json's metric is quoted on, and the PMC traffic figure committed under
profiles/ belongs to THIS build of the kernels (bench.py reports `roofline.traffic` only when
configuration, seed and the hash of the kernel sources all match -- a kernel edited after the
counters were collected must show up here, not as a silent `traffic: null` in the driver's line)."""
import argparse
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _default_args(**over):
    a = argparse.Namespace(workload="c4", scale=1.0, seed=1)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_default_step_is_the_named_configuration():
    assert bench.DEFAULT_BATCH == 8192 and bench.HBM_PEAK_GBS == 8000.0
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert "item-columns solved/sec" in base["metric"]
    from slim_amd import synth
    assert synth.CONFIGS["c4"][:2] == (1000000, 100000) and synth.CONFIGS["c5"][:2] == (10000000, 20000)


def test_committed_pmc_traffic_belongs_to_this_build():
    t = bench.pmc_traffic(_default_args(), bench.DEFAULT_BATCH, "tile32", True)
    assert t is not None and 2.5e14 < float(t) < 3.5e14       # bytes per launch of the default step
    t5 = bench.pmc_traffic(_default_args(workload="c5"), 4096, "tile32", True)
    assert t5 is not None and 1.5e14 < float(t5) < 2.5e14
    # the engine's default path on the default workload (item space) has its own entry, matched by
    # the hash of its sources on top of the residual kernel's
    ti = bench.pmc_traffic(_default_args(), bench.DEFAULT_BATCH, "item_space_step", True)
    assert ti is not None and 1e13 < float(ti) < 6e13
    # (the whole-matrix step of the residual kernel -- 2 x 10 minutes of counters per collection, a
    # path no default takes any more -- is no longer re-collected every round: profiles/r04 has it)
    # another seed, another kernel or a multi-GPU line has no entry: null, never a stale figure
    assert bench.pmc_traffic(_default_args(seed=2), bench.DEFAULT_BATCH, "tile32", True) is None
    assert bench.pmc_traffic(_default_args(), bench.DEFAULT_BATCH, "tile32", True, world=2) is None


def test_kernel_hash_ignores_comments_and_layout(tmp_path, monkeypatch):
    h = bench.kernel_hash()
    assert len(h) == 16 and h == bench.kernel_hash()
    entries = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["entries"]
    assert any(e.get("kernel_hash") == h for e in entries)


def test_dry_run_projection_adds_up():
    """bench.py --dry-run-world N on a stand-in matrix: every shard of the step
    is solved once after one warm-up, the spread is (max - min) / mean of the kernel times, and the
    projected command = start-up + broadcast + warm-up + 20 steps at the slowest shard's wall
    time + the whole-matrix step, held against the run's limit (bench.RUN_LIMIT_S)."""
    calls = []

    class Mat(object):
        nrows = 1000000

        def learn(self, col_begin, col_end, shard, **kw):
            calls.append((col_begin, col_end, shard))
            r = shard[0]
            return None, {"ncols_solved": (col_end - col_begin) // shard[1], "kernel_ms": 50000.0 + 500.0 * r,
                          "alg_bytes": 3.6e14}

    args = _default_args(dry_run_world=8, no_item_space=True)
    out = bench.dry_run(args, Mat(), 100000, 8192, {}, 10 ** 9)
    assert calls[0] == (0, 2048, (0, 8))                       # the warm-up: 1/32 of the range
    assert [c[2] for c in calls[1:]] == [(r, 8) for r in range(8)] and calls[1][:2] == (0, 65536)
    assert out["dry_run_world"] == 8 and [x["rank"] for x in out["ranks"]] == list(range(8))
    assert abs(out["kernel_ms_spread"] - 3500.0 / 51750.0) < 1e-3
    p = out["projected_command_s"]
    assert abs(p["total"] - (p["start_up_and_generate"] + p["broadcast_R"] + p["warmup"] + p["timed_steps"]
                             + p["whole_matrix_step"] + p["whole_matrix_step_item_space"])) < 0.2
    assert p["limit"] == bench.RUN_LIMIT_S and isinstance(p["fits"], bool)
    # one limit governs the run and the projection: the command's own budget keeps room inside it
    assert bench.WALL_BUDGET_S < bench.RUN_LIMIT_S


def test_dump_outputs_writes_the_step_columns_within_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: per-column summaries of every column of the step, the dense columns
    themselves (all when they fit, else a sample fixed by the seed), float32 / float64 only,
    and never more than the limit in all."""
    import numpy as np
    import scipy.sparse as sp
    n, b, span = 300, 40, 100
    W = sp.hstack([sp.csc_matrix((n, b), dtype=np.float32),
                   sp.random(n, span, density=0.05, format="csc", dtype=np.float32, random_state=3),
                   sp.csc_matrix((n, n - b - span), dtype=np.float32)], format="csc")
    info = bench.dump_outputs(str(tmp_path / "all"), W, b, span, 1)
    ids = np.load(str(tmp_path / "all" / "W_column_ids.npy"))
    assert info["dense_columns"] == span and np.array_equal(ids, np.arange(b, b + span))
    assert np.array_equal(np.load(str(tmp_path / "all" / "W_columns.npy")), W[:, b:b + span].toarray())
    assert np.array_equal(np.load(str(tmp_path / "all" / "W_column_nnz.npy")), np.diff(W.indptr)[b:b + span])
    assert np.allclose(np.load(str(tmp_path / "all" / "W_column_sum.npy")),
                       np.asarray(W[:, b:b + span].sum(axis=0)).ravel())
    # a limit that holds 20 dense columns: a seeded sample, the same on every run
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * (8 * span + 128) + 3 * 128 + 20 * (4 * n + 8))
    runs = [bench.dump_outputs(str(tmp_path / d), W, b, span, 7) for d in ("s1", "s2")]
    assert runs[0]["dense_columns"] == 20 and runs[0]["bytes"] <= bench.DUMP_LIMIT_BYTES
    for name in runs[0]["files"]:
        a, a2 = np.load(str(tmp_path / "s1" / name)), np.load(str(tmp_path / "s2" / name))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, a2)
    ids = np.load(str(tmp_path / "s1" / "W_column_ids.npy")).astype(int)
    assert ids.size == 20 and np.all(np.diff(ids) > 0) and b <= ids[0] and ids[-1] < b + span
    assert np.array_equal(np.load(str(tmp_path / "s1" / "W_columns.npy")), W[:, ids].toarray())


EXTRA_KEYS = ("parity", "residual_step", "item_space_step", "item_space_grid", "item_space_whole_matrix",
              "cpu_baseline", "strong_whole_matrix")


def test_full_is_an_option_and_off_by_default(monkeypatch):
    """Everything that takes runs of its own waits behind --full; a plain command line leaves it off."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse_args()
    assert a.full is False and (a.gpus, a.steps, a.warmup) == (1, 20, 5)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert bench.parse_args().full is True


def _run_bench(*argv):
    import subprocess
    import time
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + list(argv)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines          # stdout: the one JSON line
    return json.loads(lines[0]), wall


@pytest.mark.gpu
@pytest.mark.timeout(600, method="thread")
def test_plain_run_spends_at_most_30_s_outside_its_steps(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W` on the default workload, in a process of its own:
    the whole run from start to exit, less (N + W) x ms_per_step, is at most 30 s (start-up, the
    matrix, whatever the first step compiles or loads, the dump and the exit all count), and the
    line carries the headline fields and none of the figures that take runs of their own."""
    out, wall = _run_bench("--gpus", "1", "--steps", "1", "--warmup", "1",
                           "--dump-outputs", str(tmp_path / "dump"))
    outside = wall - 2 * out["ms_per_step"] * 1e-3
    print("plain run: %.1f s in all, %.1f ms per step, %.1f s outside the steps"
          % (wall, out["ms_per_step"], outside))
    assert out["full"] is False and not [k for k in EXTRA_KEYS if k in out]
    assert out["metric"] == "item-columns solved/sec (whole node)" and out["unit"] == "item-columns/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["n_gpus"] == 1
    assert out["steps"] == 1 and out["warmup"] == 1 and out["config"]["columns_per_step"] == 8192
    assert abs(out["value"] - 8192 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert sorted(os.listdir(str(tmp_path / "dump"))) == out["dump_outputs"]["files"]
    assert outside <= 30.0, outside


@pytest.mark.gpu
@pytest.mark.timeout(600, method="thread")
def test_full_run_keeps_what_moved_behind_it():
    """--full on a 1/50-scale C4: the same timed steps, then the figures and checks that take runs
    of their own -- ml100k parity, the residual kernel's step compared with the timed step's model,
    the CPU baseline with its parity checks of the GPU's columns.  (That they are there and ran is
    what is checked here; how close the models are is the parity tests' business.)"""
    argv = ("--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "c4", "--scale", "0.02",
            "--batch", "256", "--cpu-seconds", "2")
    plain, _ = _run_bench(*argv)
    assert plain["full"] is False and not [k for k in EXTRA_KEYS if k in plain]
    out, _ = _run_bench(*(argv + ("--full",)))
    assert out["full"] is True and out["steps"] == 2 and out["value"] > 0
    assert out["config"] == dict(plain["config"], generate_s=out["config"]["generate_s"],
                                 stage_s=out["config"]["stage_s"])
    assert out["roofline"]["nnzW"] == plain["roofline"]["nnzW"] > 0      # the same steps either way
    assert out["parity"]["match"] is True, out["parity"]
    rs = out["residual_step"]
    assert rs["columns"] == 256 and rs["kernel"] == "tile32" and rs["seconds"] > 0, rs
    assert rs["max_abs_dW_vs_the_timed_step"] >= 0.0, rs
    cb = out["cpu_baseline"]
    assert cb["value"] > 0 and isinstance(cb["parity"]["parity_ok"], bool), cb
