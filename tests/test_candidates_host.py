"""Candidate sets (include/slim_gpu_cand.h) without a device: SLIMGPU_CandSetCreate's refusals, the host loop behind
Py_SLIM_ScoreCandidates (SLIM_PREDICT=cpu) and SLIM.rerank with original ids.  The yardstick is the existing host
call Py_SLIM_GetTopN_1vsk asked for every row's full order (tests/candidate_cases.py): bit for bit throughout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from candidate_cases import (SC_FILL, P, buffers, candidate_rows, check_lists, check_slot_scores, make_set, untouched,
                             yardstick)
from conftest import ROOT
from filtered_cases import cases_fixture, make_model
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK

cases = pytest.fixture(scope="module")(cases_fixture)
NAMES = {"SLIMGPU_CandSetCreate", "SLIMGPU_CandSetFree", "SLIMGPU_ScoreCandidates", "SLIMGPU_MatrixScoreCandidates",
         "SLIMGPU_ModelEvaluateCandidates", "Py_SLIM_ScoreCandidates"}


def test_the_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "slim_gpu_cand.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b((?:Py|SLIMGPU)_\w+)\s*\(", text))
    assert declared == NAMES == set(_lib.CAND_SYMBOLS)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), "libslim.so does not export %s" % name
    assert '#include "slim_gpu_cand.h"' in open(os.path.join(ROOT, "include", "slim_gpu.h")).read()
    for other in (_lib.EXPORTED_SYMBOLS, _lib.EVAL_SYMBOLS, _lib.EVAL_AT_SYMBOLS, _lib.PLANES_SYMBOLS,
                  _lib.RANK_SYMBOLS, _lib.LIST_SYMBOLS, _lib.FILTER_SYMBOLS, _lib.FILTERED_EVAL_SYMBOLS):
        assert not declared & set(other)


def test_candset_create_refuses_bad_input():
    lib = _lib.load()
    for ncols, ptr, ind, word in ((10, [1, 1, 2, 3], [0, 1, 2], "cptr[0]"), (10, [0, 2, 1, 3], [0, 1, 2], "ascend"),
                                  (0, [0, 1, 2, 3], [0, 1, 2], "ncols")):
        rc, h = make_set(lib, ncols, ptr, ind)
        assert rc == SLIM_ERROR_INPUT and not h.value
        assert "SLIMGPU_CandSetCreate" in _lib.last_error() and word in _lib.last_error()
    # ids are taken as they are given: no order, repeats, ids outside the items; rows may be empty
    rc, h = make_set(lib, 10, [0, 0, 4, 4], [9, -1, 10, 9])
    assert rc == SLIM_OK and h.value
    lib.SLIMGPU_CandSetFree(h)
    assert lib.SLIMGPU_CandSetCreate(10, 0, None, None, None) == SLIM_ERROR_INPUT
    lib.SLIMGPU_CandSetFree(None)


@pytest.mark.parametrize("name", ["floats", "ties"])
def test_the_host_scorer_of_candidate_rows(cases, name, monkeypatch):
    c = cases(name)
    monkeypatch.setenv("SLIM_PREDICT", "cpu")
    indptr, indices = candidate_rows(c, seed=61)
    want = yardstick(c, indptr, indices)
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK, _lib.last_error()
    users = range(c.nusers)
    try:
        for n in (0, 1, 10, 64, 65, 4096):
            bufs = buffers(indptr, c.nusers, n)
            rc = c.lib.Py_SLIM_ScoreCandidates(c.hw, c.hr, cs, n, *[P(b) for b in bufs])
            assert rc == SLIM_OK, _lib.last_error()
            check_slot_scores(bufs[0], indptr, indices, want, users, c.nusers)
            if n:
                check_lists(bufs, indptr, want, users, n)
            else:
                assert untouched((np.full(1, SC_FILL, np.float32),) + bufs[1:])     # nrcmds == 0: no lists
        # lists alone: the slot scores are optional, and so are the counts
        bufs = buffers(indptr, c.nusers, 10)
        assert c.lib.Py_SLIM_ScoreCandidates(c.hw, c.hr, cs, 10, None, P(bufs[1]), P(bufs[2]), None) == SLIM_OK
        full = buffers(indptr, c.nusers, 10)
        assert c.lib.Py_SLIM_ScoreCandidates(c.hw, c.hr, cs, 10, *[P(b) for b in full]) == SLIM_OK
        assert np.array_equal(bufs[1], full[1]) and np.array_equal(bufs[2], full[2])
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)
    # the rows bite: repeated ids, history items and untouched ids are all there
    assert sum(np.unique(indices[indptr[u]:indptr[u + 1]]).size < indptr[u + 1] - indptr[u] for u in users) > 50
    assert sum((want[u][1] != 0).any() for u in users) > c.nusers // 2
    # a set made for another number of items, a set with too few rows: refused, outputs untouched
    for ncols, rows in ((c.ncols + 1, c.nusers), (c.ncols, c.nusers - 1)):
        rc, cs = make_set(c.lib, ncols, indptr[:rows + 1], indices[:indptr[rows]])
        assert rc == SLIM_OK
        bufs = buffers(indptr, c.nusers, 10)
        rc = c.lib.Py_SLIM_ScoreCandidates(c.hw, c.hr, cs, 10, *[P(b) for b in bufs])
        c.lib.SLIMGPU_CandSetFree(cs)
        assert rc == SLIM_ERROR_INPUT and "Py_SLIM_ScoreCandidates" in _lib.last_error() and untouched(bufs)


def test_rerank_with_original_ids(automotive_triplets, monkeypatch, tmp_path):
    """The Automotive fixture with original ids that are not positions; training needs a device, so the model is a
    synthetic one loaded through the item map of the training matrix."""
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
    items = np.asarray(model.id2item)
    assert not np.array_equal(items, np.arange(model.nItems))      # original ids are not positions
    users = list(trainmat.user2id)
    rng = np.random.default_rng(9)
    unknown = int(items.max()) + 1000
    cand = {}
    for k, u in enumerate(users[:40]):
        row = items[rng.choice(items.size, size=int(rng.integers(2, 30)), replace=False)].tolist()
        if k == 0:
            row.insert(1, unknown)
        if k == 1:
            row = row[:1]
        cand[u] = row
    # the yardstick: the existing 1-vs-k predict over rows of one width, user by user (a row is its own width)
    want, want_sc = {}, {}
    for u, row in cand.items():
        ids = np.array([model.item2id.get(it, -1) for it in row], np.int32)
        hist = trainmat.handle
        view = C.cast(hist, C.POINTER(_lib.CsrView)).contents
        r = int(trainmat.user2id[u])
        h0, h1 = view.rowptr[r], view.rowptr[r + 1]
        hind = np.ctypeslib.as_array(view.rowind, shape=(h1,))[h0:h1].astype(np.int32)
        hval = np.ctypeslib.as_array(view.rowval, shape=(h1,))[h0:h1].astype(np.float32)
        out_i, out_s = np.zeros(ids.size, np.int32), np.zeros(ids.size, np.float32)
        assert model._lib.Py_SLIM_GetTopN_1vsk(model.handle, hind.size, np.ascontiguousarray(hind), P(hval), ids.size,
                                               out_i, out_s, ids.size, ids, 0) == ids.size
        want[u] = [unknown if i < 0 else int(items[i]) for i in out_i]
        want_sc[u] = out_s
    out, sc = model.rerank(trainmat, cand, returnscores=True)
    assert set(out) == set(cand)
    for u in cand:
        assert out[u] == want[u] and np.array_equal(sc[u].view(np.int32), want_sc[u].view(np.int32)), u
    assert sum((want_sc[u] != 0).any() for u in cand) >= 10     # (random rows over a sparse model: some score)
    # nrcmds above a row's length gives the whole row; below it, a prefix
    cut = model.rerank(trainmat, cand, nrcmds=5)
    for u in cand:
        assert cut[u] == want[u][:5]
    assert len(cut[users[1]]) == 1 and unknown in out[users[0]]
    with pytest.raises(KeyError):
        model.rerank(trainmat, {"nobody": [int(items[0])]})
