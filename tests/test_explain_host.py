"""Explanations (include/slim_gpu_explain.h) without a device: the host loop behind Py_SLIM_ExplainCandidates
(SLIM_PREDICT=cpu), its refusals, and SLIM.explain with original ids.  The yardstick is numpy over the case's scipy
model (tests/explain_cases.py), itself tied to the existing 1-vs-k scorer by the first test: bit for bit throughout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from candidate_cases import SC_FILL, P, candidate_rows, make_set, yardstick
from conftest import ROOT
from explain_cases import (buffers, check, explain_cases_fixture, history_arrays, positions_of, sum_in_position_order,
                           untouched, yardstick_terms)
from filtered_cases import make_model
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK

cases = pytest.fixture(scope="module")(explain_cases_fixture)
NAMES = {"SLIMGPU_ExplainCandidates", "SLIMGPU_MatrixExplainCandidates", "Py_SLIM_ExplainCandidates"}


@pytest.mark.parametrize("name", ["floats", "ties"])
def test_the_yardsticks_terms_add_up_to_the_existing_scorer(cases, name):
    """No new call: the numpy terms of every slot, added in position order in float32, are the scores of
    Py_SLIM_GetTopN_1vsk (candidate_cases.yardstick), and put the row into its order."""
    c = cases(name)
    indptr, indices = candidate_rows(c, seed=61, long_row=False)
    want = yardstick(c, indptr, indices)
    mine = yardstick_terms(c, indptr, indices)
    scored = 0
    for u in range(c.nusers):
        s = np.array([sum_in_position_order(p, t) for p, _, t in mine[u]], np.float32)
        order = np.lexsort((np.arange(s.size), -s.astype(np.float64)))
        ids, sc = want[u]
        assert np.array_equal(indices[indptr[u]:indptr[u + 1]][order], ids), "user %d: order" % u
        assert np.array_equal(s[order].view(np.int32), sc.view(np.int32)), "user %d: scores" % u
        scored += int((s != 0).sum())
    assert scored > c.nusers


def test_the_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "slim_gpu_explain.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b((?:Py|SLIMGPU)_\w+)\s*\(", text)) == NAMES == set(_lib.EXPLAIN_SYMBOLS)
    assert re.search(r"#define\s+SLIMGPU_MAX_WHY\s+16\b", text) and _lib.MAX_WHY == 16
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), "libslim.so does not export %s" % name
    assert '#include "slim_gpu_explain.h"' in open(os.path.join(ROOT, "include", "slim_gpu_cand.h")).read()


@pytest.mark.parametrize("name", ["floats", "ties", "edges"])
def test_the_host_explanations(cases, name, monkeypatch):
    c = cases(name)
    monkeypatch.setenv("SLIM_PREDICT", "cpu")
    indptr, indices, want = cases.rows(name)
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK, _lib.last_error()
    users = range(c.nusers)
    try:
        for nwhy in (1, 3, 16):
            bufs = buffers(indptr, nwhy)
            rc = c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, nwhy, *[P(b) for b in bufs])
            assert rc == SLIM_OK, _lib.last_error()
            check(bufs, indptr, want, users, c.nusers, nwhy)
        # support alone, and the places without support
        only = buffers(indptr, 3)
        assert c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, 3, None, None, P(only[2])) == SLIM_OK
        full = buffers(indptr, 3)
        assert c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, 3, P(full[0]), P(full[1]), None) == SLIM_OK
        assert untouched((only[0], only[1], full[2]))
        both = buffers(indptr, 3)
        assert c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, 3, *[P(b) for b in both]) == SLIM_OK
        assert np.array_equal(only[2], both[2]) and np.array_equal(full[0], both[0])
        assert np.array_equal(full[1].view(np.int32), both[1].view(np.int32))
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)
    # the case bites: slots with more terms than 16, with ties, with none
    sizes = np.array([t.size for u in users for _, _, t in want[u]])
    assert (sizes == 0).any() and (sizes > 1).sum() > 20
    if name != "floats":
        assert any(t.size > 1 and (t[:-1] == t[1:]).any() for u in users for _, _, t in want[u])
    if name == "edges":
        assert (sizes > 16).any()
        zero = [t for u in users for _, _, t in want[u] if t.size and (t == 0).any()]
        assert zero and any(np.signbit(t[t == 0]).any() and not np.signbit(t[t == 0]).all() for t in zero)


@pytest.mark.parametrize("name", ["floats", "ties", "edges"])
def test_the_terms_of_a_slot_add_up_to_its_score(cases, name, monkeypatch):
    """nwhy = 16: a slot with support <= 16, its terms back in position order and added from 0.0f, gives the slot
    score of Py_SLIM_ScoreCandidates bit for bit."""
    c = cases(name)
    monkeypatch.setenv("SLIM_PREDICT", "cpu")
    indptr, indices, _ = cases.rows(name)
    hptr, hind, _ = history_arrays(c)
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK, _lib.last_error()
    try:
        items, terms, support = buffers(indptr, 16)
        assert c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, 16, P(items), P(terms), P(support)) == SLIM_OK
        slot = np.full(max(int(indptr[-1]), 1), SC_FILL, np.float32)
        assert c.lib.Py_SLIM_ScoreCandidates(c.hw, c.hr, cs, 0, P(slot), None, None, None) == SLIM_OK
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)
    summed = 0
    for u in range(c.nusers):
        hist = hind[hptr[u]:hptr[u + 1]]
        for e in range(int(indptr[u]), int(indptr[u + 1])):
            n = int(support[e])
            assert n >= 0
            if n > 16:
                continue
            pos = positions_of(hist, items[e * 16:e * 16 + n])
            s = sum_in_position_order(pos, terms[e * 16:e * 16 + n])
            assert np.float32(s).view(np.int32) == slot[e].view(np.int32), "user %d entry %d" % (u, e)
            summed += n > 1
    assert summed > 20


def test_refusals_leave_every_buffer_untouched(cases, monkeypatch):
    c = cases("floats")
    monkeypatch.setenv("SLIM_PREDICT", "cpu")
    indptr, indices, _ = cases.rows("floats")
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK
    try:
        for nwhy in (0, 17, -1):
            bufs = buffers(indptr, 17)
            rc = c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, nwhy, *[P(b) for b in bufs])
            assert rc == SLIM_ERROR_INPUT and "Py_SLIM_ExplainCandidates" in _lib.last_error() and untouched(bufs)
            assert "nwhy" in _lib.last_error()
        bufs = buffers(indptr, 3)
        for args in ((P(bufs[0]), None, P(bufs[2])), (None, P(bufs[1]), P(bufs[2]))):
            rc = c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, 3, *args)
            assert rc == SLIM_ERROR_INPUT and "Py_SLIM_ExplainCandidates" in _lib.last_error() and untouched(bufs)
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)
    # a set made for another number of items, a set with too few rows
    for ncols, rows in ((c.ncols + 1, c.nusers), (c.ncols, c.nusers - 1)):
        rc, cs = make_set(c.lib, ncols, indptr[:rows + 1], indices[:indptr[rows]])
        assert rc == SLIM_OK
        bufs = buffers(indptr, 3)
        rc = c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, 3, *[P(b) for b in bufs])
        c.lib.SLIMGPU_CandSetFree(cs)
        assert rc == SLIM_ERROR_INPUT and "Py_SLIM_ExplainCandidates" in _lib.last_error() and untouched(bufs)


def test_explain_with_original_ids(automotive_triplets, monkeypatch, tmp_path, capsys):
    """The Automotive fixture with original ids that are not positions (the model is a synthetic one loaded through
    the item map of the training matrix, as in tests/test_candidates_host.py): SLIM.explain returns original ids and
    the terms of an item add up to the score SLIM.rerank gives it."""
    from slim_amd import SLIM, SLIMatrix
    from slim_amd.io import write_csr_text
    monkeypatch.setenv("SLIM_PREDICT", "cpu")
    trn = automotive_triplets[0].copy()
    trn[:, 1] = 1000 + 7 * trn[:, 1]
    trainmat = SLIMatrix(trn)
    W = make_model(trainmat.nItems, 8, 12, False, seed=13)
    write_csr_text(str(tmp_path / "m.csr"), W)
    np.savetxt(str(tmp_path / "map.csv"), trainmat.id2item, fmt="%d")
    model = SLIM()
    model.load_model(str(tmp_path / "m.csr"), str(tmp_path / "map.csv"))
    items = np.asarray(model.id2item)
    users = list(trainmat.user2id)[:40]
    rng = np.random.default_rng(9)
    unknown = int(items.max()) + 1000
    view = C.cast(trainmat.handle, C.POINTER(_lib.CsrView)).contents
    lists = {}
    for k, u in enumerate(users):
        r = int(trainmat.user2id[u])
        h0, h1 = view.rowptr[r], view.rowptr[r + 1]
        hist = np.ctypeslib.as_array(view.rowind, shape=(h1,))[h0:h1]
        touched = np.unique(W[hist].indices)        # items the history reaches: they have terms
        row = items[rng.choice(touched, size=min(6, touched.size), replace=False)].tolist()
        row += items[rng.choice(items.size, size=4, replace=False)].tolist()
        if k == 0:
            row.insert(1, unknown)
        lists[u] = row
    ranked, scores = model.rerank(trainmat, lists, returnscores=True)
    capsys.readouterr()
    why = model.explain(trainmat, lists, nwhy=16)
    assert "1 candidate items not in the training set." in capsys.readouterr().out
    assert set(why) == set(lists)
    explained = 0
    for u in users:
        r = int(trainmat.user2id[u])
        h0, h1 = view.rowptr[r], view.rowptr[r + 1]
        hist = items[np.ctypeslib.as_array(view.rowind, shape=(h1,))[h0:h1]]       # original ids, history order
        score_of = dict(zip(ranked[u], scores[u]))
        assert len(why[u]) == len(lists[u])
        for it, pairs in zip(lists[u], why[u]):
            if it == unknown:
                assert pairs == []
                continue
            assert len(pairs) <= 16 and all(h in hist for h, _ in pairs)         # original ids of history items
            t = np.array([x for _, x in pairs], np.float32)
            assert (np.diff(t) <= 0).all()
            if lists[u].count(it) == 1 and len(pairs) < 16:
                pos = positions_of(hist, np.array([h for h, _ in pairs]))
                s = sum_in_position_order(pos, t)
                assert np.float32(s).view(np.int32) == np.float32(score_of[it]).view(np.int32), (u, it)
                explained += len(pairs) > 0
    assert explained >= 40
    assert not np.array_equal(items, np.arange(model.nItems))
    with pytest.raises(KeyError):
        model.explain(trainmat, {"nobody": [int(items[0])]})
