"""Exposure of top-N lists (include/slim_gpu_exposure.h) without a device: SLIMGPU_ListExposure, the definition in
code, against its restatement in Python ints and np.bincount -- counters and every field of the summary, each double
bit for bit as float(num) / float(den); the refusals; the argument checks of SLIM.mselect(exposure=...)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from exposure_cases import (P, WORKED, call_host, random_lists, restate, same_summary)
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK, Opt
from slim_amd.engine import list_exposure

NAMES = {"SLIMGPU_ListExposure", "SLIMGPU_MatrixListExposure", "SLIMGPU_MatrixPredictExposure",
         "SLIMGPU_ModelEvaluateExposure", "Py_SLIM_MselectExposure"}


def test_the_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "slim_gpu_exposure.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b((?:Py|SLIMGPU)_\w+)\s*\(", text)) == NAMES == set(_lib.EXPOSURE_SYMBOLS)
    assert re.search(r"SLIM_OPTION_GPU_EVALEXPOSURE\s*=\s*26\b", text) and int(Opt.GPU_EVALEXPOSURE) == 26
    assert re.search(r"#define\s+SLIMGPU_EXPOSURE_CELL\s+8\b", text) and _lib.EXPOSURE_CELL == 8
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), "libslim.so does not export %s" % name
    assert '#include "slim_gpu_exposure.h"' in open(os.path.join(ROOT, "include", "slim_gpu_lists.h")).read()
    assert not NAMES & set(_lib.EXPORTED_SYMBOLS) and len(_lib.EXPORTED_SYMBOLS) == 46
    assert C.sizeof(_lib.Exposure) == 4 * 8 + 2 * 4 + 4 * 8


def test_the_worked_example():
    w = WORKED
    lib = _lib.load()
    rc, E, summ = call_host(lib, w["ncols"], w["ids"], w["counts"], w["cutoffs"], pop=w["pop"], fmarker=w["fmarker"])
    assert rc == SLIM_OK, _lib.last_error()
    assert E.tolist() == [[3, 0, 0, 0, 0, 0], [4, 1, 2, 0, 0, 1]]
    a, b = summ[0], summ[1]
    assert (a.lists, a.slots, a.distinct, a.tail_slots, a.outside, a.ncols) == (3, 3, 1, 0, 0, 6)
    assert (b.lists, b.slots, b.distinct, b.tail_slots, b.outside, b.ncols) == (3, 8, 4, 3, 0, 6)
    assert a.gini == float(15) / float(18) and a.avg_pop == 10.0 and a.coverage == float(1) / float(6)
    assert a.tail_share == 0.0
    assert b.coverage == float(4) / float(6) and b.tail_share == float(3) / float(8)
    assert b.gini == float(26) / float(48) and b.avg_pop == float(53) / float(8)
    # ... and the restatement gives the same
    want_E, want = restate(w["ncols"], w["ids"], w["counts"], w["cutoffs"], pop=w["pop"], fmarker=w["fmarker"])
    assert np.array_equal(E, want_E) and same_summary(summ, want)
    # the Python call
    E2, dicts = list_exposure(w["ids"], w["counts"], w["ncols"], w["cutoffs"], pop=w["pop"], fmarker=w["fmarker"])
    assert np.array_equal(E2, E) and dicts[1]["slots"] == 8 and dicts[1]["nrcmds"] == 3
    assert dicts[1]["gini"] == float(26) / float(48)


@pytest.mark.parametrize("ncols,nlists,N,cutoffs,with_counts,fm_ncols", [
    (50, 400, 10, (10,), True, 50),                          # K = 1, c_{K-1} = nrcmds
    (50, 400, 24, (1, 2, 3, 5, 8, 13, 21, 24), True, 40),    # K = 8, c_0 = 1, marker shorter than the catalogue
    (7, 300, 5, (1, 5), False, 7),                           # counts == NULL
    (1000, 90, 33, (4, 20), True, 1200),                     # most items never shown
    (1, 17, 3, (2, 3), True, 1),                             # one item
])
def test_random_lists_against_the_restatement(ncols, nlists, N, cutoffs, with_counts, fm_ncols):
    lib = _lib.load()
    rng = np.random.default_rng(ncols * 1000 + nlists)
    ids, counts = random_lists(rng, ncols, nlists, N, outside=True)
    if not with_counts:
        counts = None
    pop = rng.integers(0, 2 ** 32, ncols, dtype=np.uint64).astype(np.uint32)
    fmarker = rng.integers(0, 2, fm_ncols).astype(np.int32)
    rc, E, summ = call_host(lib, ncols, ids, counts, cutoffs, pop=pop, fmarker=fmarker)
    assert rc == SLIM_OK, _lib.last_error()
    want_E, want = restate(ncols, ids, counts, cutoffs, pop=pop, fmarker=fmarker)
    assert np.array_equal(E, want_E)
    assert same_summary(summ, want)
    # the case bites: repeats inside a list, ids outside the range, valid ids beyond counts[q]
    assert want[-1]["outside"] > 0
    assert any(np.unique(r[:N if counts is None else c]).size < (N if counts is None else c)
               for r, c in zip(ids, counts if counts is not None else [N] * nlists))
    if counts is not None:
        assert (counts < N).any() and (ids[counts < N, -1] >= 0).all()
    # the summary alone, the counters alone, without pop and marker
    rc, _, s2 = call_host(lib, ncols, ids, counts, cutoffs, pop=pop, fmarker=fmarker, want_E=False)
    assert rc == SLIM_OK and same_summary(s2, want)
    rc, E3, _ = call_host(lib, ncols, ids, counts, cutoffs, want_summary=False)
    assert rc == SLIM_OK and np.array_equal(E3, want_E)
    rc, _, s4 = call_host(lib, ncols, ids, counts, cutoffs)
    bare = restate(ncols, ids, counts, cutoffs)[1]
    assert rc == SLIM_OK and same_summary(s4, bare) and all(b["tail_slots"] == 0 and b["avg_pop"] == 0.0 for b in bare)


def test_no_slot_at_all():
    lib = _lib.load()
    ids = np.arange(12, dtype=np.int32).reshape(4, 3)
    for nlists, counts in ((4, np.zeros(4, np.int32)), (0, None)):
        rc, E, summ = call_host(lib, 20, ids[:nlists], counts, (1, 3), pop=np.ones(20, np.uint32),
                                fmarker=np.ones(20, np.int32))
        assert rc == SLIM_OK, _lib.last_error()
        assert not E.any()
        for s in summ:
            assert (s.lists, s.slots, s.distinct, s.tail_slots, s.outside) == (nlists, 0, 0, 0, 0)
            assert (s.coverage, s.tail_share, s.gini, s.avg_pop) == (0.0, 0.0, 0.0, 0.0)
    # nlists == 0 needs no lists
    cut = np.array([2], np.int32)
    assert lib.SLIMGPU_ListExposure(20, None, None, 0, 0, 3, None, None, 1, P(cut), None, None) == SLIM_OK


def test_the_refusals():
    lib = _lib.load()
    ids = np.zeros((5, 4), np.int32)
    good = np.array([1, 4], np.int32)

    def refused(ncols=10, nlists=5, nrcmds=4, ids_=ids, counts=None, cutoffs=good, K=None):
        E = np.full((8, max(ncols, 1)), 7, np.uint32)
        cut = np.ascontiguousarray(cutoffs, np.int32)
        rc = lib.SLIMGPU_ListExposure(ncols, None, None, 0, nlists, nrcmds, None if ids_ is None else P(ids_),
                                      None if counts is None else P(np.ascontiguousarray(counts, np.int32)),
                                      cut.size if K is None else K, P(cut), P(E), None)
        text = _lib.last_error()
        return rc == SLIM_ERROR_INPUT and text.startswith("SLIMGPU_ListExposure: ") and (E == 7).all()

    assert refused(cutoffs=[4, 1])                    # unsorted
    assert refused(cutoffs=[2, 2])                    # repeated
    assert refused(cutoffs=[0, 3])                    # < 1
    assert refused(cutoffs=[1, 5])                    # the last above nrcmds
    assert refused(nrcmds=64, ids_=np.zeros((5, 64), np.int32), cutoffs=list(range(1, 10)))  # more than 8
    assert refused(K=0)
    assert refused(ncols=0)
    assert refused(nlists=-1)
    assert refused(counts=[0, 1, 5, 2, 3])            # a count above nrcmds
    assert refused(counts=[0, 1, -1, 2, 3])
    assert refused(ids_=None)                         # null lists with nlists > 0
    with pytest.raises(RuntimeError, match="SLIMGPU_ListExposure"):
        list_exposure(ids, None, 10, [3, 2])


def test_mselect_checks_its_exposure_argument():
    from slim_amd import SLIM
    m = SLIM()
    with pytest.raises(TypeError, match="exposure"):
        m.mselect({}, None, None, [1.0], [1.0], 10, exposure="yes")
    with pytest.raises(TypeError, match="exposure"):
        m.mselect({}, None, None, [1.0], [1.0], 10, exposure=1)
    with pytest.raises(TypeError, match="nnegs"):
        m.mselect({}, None, None, [1.0], [1.0], 10, exposure=True, nnegs=50)
