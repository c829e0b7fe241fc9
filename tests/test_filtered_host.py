"""Candidate filters (include/slim_gpu_filter.h) without a device: SLIMGPU_FilterCreate's refusals, the filtered
host scorer behind Py_SLIM_PredictFiltered (SLIM_PREDICT=cpu), SLIM.predict's allowed_items / blocked_items /
exclude with original ids, and slim_predict -allowfile / -blockfile / -exclfile.  The yardstick is the existing,
unfiltered host scorer asked for the full ranking (tests/filtered_cases.py): np.array_equal throughout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, ROOT
from filtered_cases import cases_fixture, make_filter, make_model, same
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK

cases = pytest.fixture(scope="module")(cases_fixture)
BOTH = pytest.mark.parametrize("name", ["floats", "ties"])


def host_filtered(c, n, flt):
    ids = np.full(c.nusers * n, -1, np.int32)
    sc = np.zeros(c.nusers * n, np.float32)
    rc = c.lib.Py_SLIM_PredictFiltered(n, c.hw, c.hr, flt, ids, sc)
    return rc, ids.reshape(-1, n), sc.reshape(-1, n)


def test_the_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "slim_gpu_filter.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b((?:Py|SLIMGPU)_\w+)\s*\(", text))
    assert declared == set(_lib.FILTER_SYMBOLS) and len(declared) == 6
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), "libslim.so does not export %s" % name
    assert '#include "slim_gpu_filter.h"' in open(os.path.join(ROOT, "include", "slim_gpu.h")).read()
    for other in (_lib.EXPORTED_SYMBOLS, _lib.EVAL_SYMBOLS, _lib.EVAL_AT_SYMBOLS, _lib.PLANES_SYMBOLS,
                  _lib.RANK_SYMBOLS, _lib.LIST_SYMBOLS):
        assert not declared & set(other)


def test_filter_create_refuses_bad_input():
    lib = _lib.load()
    good = sp.csr_matrix(np.eye(3, 10, dtype=np.float32))
    for kw, word in (({"allowed": [0, 10]}, "10"), ({"blocked": [-1]}, "-1"), ({"allowed": [3], "X": None}, None)):
        rc, h = make_filter(lib, 10, **kw)
        if word is None:
            assert rc == SLIM_OK and h.value
            lib.SLIMGPU_FilterFree(h)
        else:
            assert rc == SLIM_ERROR_INPUT and not h.value
            assert "SLIMGPU_FilterCreate" in _lib.last_error() and word in _lib.last_error()
    for ptr, ind, word in (([1, 1, 2, 3], [0, 1, 2], "xptr[0]"), ([0, 2, 1, 3], [0, 1, 2], "ascend"),
                           ([0, 1, 2, 3], [0, 1, 10], "10")):
        X = sp.csr_matrix(good)
        X.indptr, X.indices = np.array(ptr, np.int64), np.array(ind, np.int32)
        rc, h = make_filter(lib, 10, X=X)
        assert rc == SLIM_ERROR_INPUT and not h.value and word in _lib.last_error()
    assert lib.SLIMGPU_FilterCreate(10, 0, None, 0, 0, None, None, None) == SLIM_ERROR_INPUT
    lib.SLIMGPU_FilterFree(None)


@BOTH
def test_the_filtered_host_scorer(cases, name, monkeypatch):
    c = cases(name)
    monkeypatch.setenv("SLIM_PREDICT", "cpu")
    rng = np.random.default_rng(41)
    allowed = rng.random(c.ncols) < 0.4
    X = c.exclusions(seed=43, xusers=c.nusers - 10)
    for kw, mask, rows in (({"allowed": np.flatnonzero(allowed)}, allowed, None),
                           ({"blocked": np.flatnonzero(~allowed)}, allowed, None),
                           ({"X": X}, None, X),
                           ({"allowed": np.flatnonzero(allowed), "X": X}, allowed, X),
                           ({"allowed": []}, np.zeros(c.ncols, bool), None),
                           ({"blocked": []}, None, None)):
        rc, flt = make_filter(c.lib, c.ncols, **kw)
        assert rc == SLIM_OK, _lib.last_error()
        try:
            for n in (1, 10, 300, c.ncols):
                rc, ids, sc = host_filtered(c, n, flt)
                assert rc == SLIM_OK and same((ids, sc), c.expected(n, mask, rows)), (name, sorted(kw), n)
        finally:
            c.lib.SLIMGPU_FilterFree(flt)
    # the filters bite, the scratch of the scorer leaves as it came: the unfiltered call is what it was
    want, got = c.expected(10), c.expected(10, allowed, X)
    assert (np.any(want[0] != got[0], axis=1)).sum() >= (want[2] > 0).sum() // 2
    rc, ids, sc = host_filtered(c, 10, None)
    assert rc == SLIM_OK and same((ids, sc), want)
    # a filter made for another number of items
    rc, flt = make_filter(c.lib, c.ncols + 1, allowed=[0])
    assert rc == SLIM_OK
    rc, ids, sc = host_filtered(c, 10, flt)
    c.lib.SLIMGPU_FilterFree(flt)
    assert rc == SLIM_ERROR_INPUT and "Py_SLIM_PredictFiltered" in _lib.last_error()
    assert (ids == -1).all() and (sc == 0).all()


def test_slim_predict_with_original_ids(automotive_triplets, monkeypatch, tmp_path):
    """The Automotive fixture with original ids that are not positions; training needs a device, so
    the model is a synthetic one loaded through the item map of the training matrix."""
    from slim_amd import SLIM, SLIMatrix
    from slim_amd.io import write_csr_text
    monkeypatch.setenv("SLIM_PREDICT", "cpu")
    trn = automotive_triplets[0].copy()
    trn[:, 1] = 1000 + 7 * trn[:, 1]       # (the fixture's item ids are their positions: relabel them)
    trainmat = SLIMatrix(trn)
    write_csr_text(str(tmp_path / "m.csr"), make_model(trainmat.nItems, 8, 12, False, seed=13))
    np.savetxt(str(tmp_path / "map.csv"), trainmat.id2item, fmt="%d")
    model = SLIM()
    model.load_model(str(tmp_path / "m.csr"), str(tmp_path / "map.csv"))
    assert model.nItems == trainmat.nItems and np.array_equal(model.id2item, trainmat.id2item)
    assert not np.array_equal(model.id2item, np.arange(model.nItems))      # original ids are not positions
    n, long_n = 10, model.nItems
    # the unfiltered full ranking from the existing host scorer, then in original ids
    raw = np.full(trainmat.nUsers * long_n, -1, np.int32)
    raw_sc = np.zeros(trainmat.nUsers * long_n, np.float32)
    assert model._lib.Py_SLIM_Predict(long_n, model.handle, trainmat.handle, raw, raw_sc) == SLIM_OK
    raw = raw.reshape(-1, long_n)
    users = list(trainmat.user2id)
    ncand = {u: int((raw[trainmat.user2id[u]] >= 0).sum()) for u in users}
    full = {u: np.asarray(model.id2item)[raw[trainmat.user2id[u]]] for u in users}
    rng = np.random.default_rng(5)
    items = np.asarray(model.id2item)
    unknown = [int(items.max()) + 1000, int(items.max()) + 1001]
    chosen = items[rng.random(items.size) < 0.5].tolist()
    # exclusions: every user's own top 2, plus one event of an item and one of a user the maps do not know
    events = [[u, it, 1.0] for u in users for it in full[u][:min(2, ncand[u])].tolist()]
    events += [[users[0], unknown[0], 1.0], ["nobody", chosen[0], 1.0]]
    excl = SLIMatrix(events, trainmat)
    barred = {u: set(full[u][:min(2, ncand[u])].tolist()) for u in users}

    def survivors(u, ok):
        lst = [it for it in full[u][:ncand[u]].tolist() if ok(u, it)]
        return lst[:n] + [None] * (n - len(lst[:n]))

    def check(out, ok):
        changed = 0
        for u in users:
            want = survivors(u, ok)
            got = out[u].tolist()
            m = sum(w is not None for w in want)
            assert got[:m] == want[:m] and all(g == items[-1] for g in got[m:]), u   # (-1 indexes the map's end)
            changed += got != full[u][:n].tolist()
        return changed

    cs = set(chosen)
    out = model.predict(trainmat, nrcmds=n, allowed_items=chosen + unknown)
    assert check(out, lambda u, it: it in cs) > len(users) // 2
    out = model.predict(trainmat, nrcmds=n, blocked_items=chosen + unknown)
    assert check(out, lambda u, it: it not in cs) > len(users) // 2
    out = model.predict(trainmat, nrcmds=n, exclude=excl)
    assert check(out, lambda u, it: it not in barred[u]) > len(users) // 2
    out = model.predict(trainmat, nrcmds=n, allowed_items=chosen, exclude=excl)
    check(out, lambda u, it: it in cs and it not in barred[u])
    with pytest.raises(TypeError):
        model.predict(trainmat, nrcmds=n, allowed_items=chosen, blocked_items=chosen)


def _cli(*args, cwd, ok=True):
    e = dict(os.environ)
    e["SLIM_PREDICT"] = "cpu"
    p = subprocess.run([os.path.join(ROOT, "slim_amd", "bin", "slim_predict")] + list(args), capture_output=True,
                       text=True, env=e, cwd=cwd, timeout=280)
    assert (p.returncode == 0) == ok, p.stdout + p.stderr
    return p.stdout + p.stderr


def _lists(path):
    out = []
    for line in open(path).read().splitlines():
        t = line.split()
        out.append([(int(t[j]), t[j + 1]) for j in range(0, len(t), 2)])
    return out


def test_slim_predict_command_line(tmp_path, ml100k):
    from slim_amd.io import write_csr_text
    trn = os.path.join(GOLDEN, "ml100k-train.csr")
    nitems = ml100k[0].shape[1]
    mdl = str(tmp_path / "m.model")
    write_csr_text(mdl, make_model(nitems, 30, 40, False, seed=3))
    full_file = str(tmp_path / "full.txt")
    _cli("-nrcmds=%d" % nitems, "-outfile=" + full_file, mdl, trn, cwd=str(tmp_path))
    full = _lists(full_file)
    rng = np.random.default_rng(9)
    chosen = np.flatnonzero(rng.random(nitems) < 0.5)
    ids_file = str(tmp_path / "ids.txt")
    open(ids_file, "w").write("".join("%d\n" % i for i in chosen.tolist() + [nitems + 7]))   # one id beyond the model
    X = sp.lil_matrix((len(full), nitems), dtype=np.float32)
    for u, lst in enumerate(full):
        for it, _ in lst[:3] if u % 4 else []:
            X[u, it] = 1.0
    excl_file = str(tmp_path / "excl.csr")
    write_csr_text(excl_file, sp.csr_matrix(X))
    cs = set(chosen.tolist())
    barred = [set(it for it, _ in lst[:3]) if u % 4 else set() for u, lst in enumerate(full)]
    n = 20
    for opts, ok in ((["-allowfile=" + ids_file], lambda u, it: it in cs),
                     (["-blockfile=" + ids_file], lambda u, it: it not in cs),
                     (["-exclfile=" + excl_file], lambda u, it: it not in barred[u]),
                     (["-allowfile=" + ids_file, "-exclfile=" + excl_file],
                      lambda u, it: it in cs and it not in barred[u])):
        out = str(tmp_path / "out.txt")
        _cli("-nrcmds=%d" % n, "-outfile=" + out, *opts, mdl, trn, cwd=str(tmp_path))
        got = _lists(out)
        assert len(got) == len(full)
        for u, lst in enumerate(full):
            assert got[u] == [e for e in lst if ok(u, e[0])][:n], (opts, u)
    text = _cli("-allowfile=" + ids_file, "-blockfile=" + ids_file, mdl, trn, cwd=str(tmp_path), ok=False)
    assert "-allowfile" in text and "-blockfile" in text
