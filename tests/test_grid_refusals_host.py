"""What a model-selection grid refuses before it stages anything (slim_amd/csrc/grid_eval.cpp): the status, the whole
error text and no pair line, on a machine with or without a device.  The texts are those the library gave before
the grid had one owner; two obstacles at once pin which of them is named.  The same through SLIMGPU_GridOpen
(include/slim_gpu_grid.h), which leaves its out argument alone when it refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from filtered_cases import make_filter, wrap
from slim_amd import _lib
from slim_amd.constants import SLIM_ALGO, SLIM_ERROR_INPUT, SLIM_NOPTIONS, SLIM_OK, Opt

NEGS = ("Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALNEGS needs the candidate evaluation in HBM (cd on one GPU, no filter, "
        "nrcmds <= 128, SLIM_GPU_RESIDENT and SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs): ")
EXPO = ("Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALEXPOSURE needs the evaluation in HBM and lists of at most 128 (cd on one "
        "GPU, SLIM_GPU_RESIDENT and SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs, no sampled "
        "negatives): ")
FILT = ("Py_SLIM_MselectFiltered: a filter needs the evaluation in HBM (cd on one GPU, SLIM_GPU_RESIDENT "
        "and SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs, a filter of the models' width): ")
STRIDE = ("Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALSTRIDE needs the evaluation in HBM (cd on one GPU, nrcmds >= 1, "
          "SLIM_GPU_RESIDENT and SLIM_GPU_EVAL_RESIDENT not 0, a matrix staged without merged pairs; above 128 a model "
          "the chunk scorer serves)")
ADMM = "the ADMM solver leaves no model in HBM"
SEVERAL = "the grid runs on several GPUs"
RES0 = "SLIM_GPU_RESIDENT=0 keeps the models on the host"
EVR0 = "SLIM_GPU_EVAL_RESIDENT=0 evaluates through the host"
admm = {Opt.ALGO: SLIM_ALGO["admm"]}

# name: (option slots, environment, with a filter, through Py_SLIM_MselectExposure, the error text)
CASES = {
    "negs_admm": ({Opt.GPU_EVALNEGS: 5, **admm}, {}, False, False, NEGS + ADMM),
    "negs_ngpus": ({Opt.GPU_EVALNEGS: 5}, {"SLIM_GPU_NGPUS": "2"}, False, False, NEGS + SEVERAL),
    "negs_resident0": ({Opt.GPU_EVALNEGS: 5}, {"SLIM_GPU_RESIDENT": "0"}, False, False, NEGS + RES0),
    "negs_eval_resident0": ({Opt.GPU_EVALNEGS: 5}, {"SLIM_GPU_EVAL_RESIDENT": "0"}, False, False, NEGS + EVR0),
    "negs_nrcmds129": ({Opt.GPU_EVALNEGS: 5, Opt.NRCMDS: 129}, {}, False, False,
                       NEGS + "nrcmds is 129: the candidate lists use the eval set's cutoffs, 1 to 128"),
    "negs_minus2": ({Opt.GPU_EVALNEGS: -2}, {}, False, False,
                    NEGS + "SLIM_OPTION_GPU_EVALNEGS must be at least 0, not -2"),
    "negs_filter": ({Opt.GPU_EVALNEGS: 5}, {}, True, False,
                    NEGS + "a candidate filter is given: candidate rows take no filter"),
    "negpop_alone": ({Opt.GPU_EVALNEGPOP: 1}, {}, False, False,
                     "Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALNEGPOP weights the sampled negatives and "
                     "SLIM_OPTION_GPU_EVALNEGS is off: there is nothing to weight"),
    "negpop_2": ({Opt.GPU_EVALNEGS: 5, Opt.GPU_EVALNEGPOP: 2}, {}, False, False,
                 "Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALNEGPOP must be 0 or 1, not 2"),
    "expo_2": ({Opt.GPU_EVALEXPOSURE: 2}, {}, False, False,
               EXPO + "SLIM_OPTION_GPU_EVALEXPOSURE must be 0 or 1, not 2"),
    "expo_negs": ({Opt.GPU_EVALEXPOSURE: 1, Opt.GPU_EVALNEGS: 5}, {}, False, False,
                  EXPO + "SLIM_OPTION_GPU_EVALNEGS is on: the exposure of sampled candidate lists is not built"),
    "expo_nrcmds200": ({Opt.NRCMDS: 200}, {}, False, True,
                       EXPO + "nrcmds is 200: the lists behind the evaluation have 1 to 128 places"),
    "expo_admm": ({Opt.GPU_EVALEXPOSURE: 1, **admm}, {}, False, False, EXPO + ADMM),
    "stride_0": ({Opt.GPU_EVALSTRIDE: 0}, {}, False, False,
                 "Py_SLIM_Mselect: SLIM_OPTION_GPU_EVALSTRIDE must be at least 1"),
    "filter_admm": (admm, {}, True, False, FILT + ADMM),
    "stride3_admm": ({Opt.GPU_EVALSTRIDE: 3, **admm}, {}, False, False, STRIDE),
    # two obstacles at once: which one is named
    "negs_admm_and_filter": ({Opt.GPU_EVALNEGS: 5, **admm}, {}, True, False,
                             NEGS + "a candidate filter is given: candidate rows take no filter"),
    "expo_admm_and_nrcmds200": ({Opt.NRCMDS: 200, **admm}, {}, False, True, EXPO + ADMM),
    "negs_resident0_and_nrcmds129": ({Opt.GPU_EVALNEGS: 5, Opt.NRCMDS: 129}, {"SLIM_GPU_RESIDENT": "0"}, False,
                                     False, NEGS + RES0),
    "negs_ngpus_and_expo": ({Opt.GPU_EVALNEGS: 5, Opt.GPU_EVALEXPOSURE: 1}, {"SLIM_GPU_NGPUS": "2"}, False, False,
                            NEGS + SEVERAL),
    "stride3_and_filter_admm": ({Opt.GPU_EVALSTRIDE: 3, **admm}, {}, True, False, STRIDE),
}
L1 = np.array([1.0, 2.0])
L2 = np.array([0.5])


def test_the_names_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slim_gpu_grid.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(SLIMGPU_\w+)\s*\(", text))
    assert declared == set(_lib.GRID_SYMBOLS) and len(declared) == 5
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), "libslim.so does not export %s" % name
    assert C.sizeof(_lib.GridCell) == 8 * 3 + 8 * 4 + 4 * 4 + C.sizeof(_lib.Exposure) + 8


@pytest.fixture(scope="module")
def small():
    """12 users, 9 items; every user holds one item out."""
    lib = _lib.load()
    rng = np.random.default_rng(7)
    R = sp.csr_matrix((rng.random((12, 9)) < 0.4).astype(np.float32))
    T = sp.csr_matrix((np.ones(12, np.float32), (np.arange(12), np.arange(12) % 9)), shape=(12, 9))
    assert R.getnnz(axis=0).min() > 0
    trn, tst = wrap(lib, R), wrap(lib, T)
    rc, flt = make_filter(lib, 9, blocked=[2, 5])
    assert rc == SLIM_OK
    yield lib, trn, tst, flt
    lib.SLIMGPU_FilterFree(flt)
    for h in (trn, tst):
        lib.Py_csr_free(h)


def options(slots):
    iopt, dopt = np.full(SLIM_NOPTIONS, -1, np.int32), np.full(SLIM_NOPTIONS, -1.0)
    iopt[Opt.ALGO], iopt[Opt.MAXNITERS] = SLIM_ALGO["cd"], 20
    for k, v in slots.items():
        iopt[k] = v
    return iopt, dopt


def set_env(monkeypatch, env):
    for k in ("SLIM_GPU_NGPUS", "SLIM_GPU_RESIDENT", "SLIM_GPU_EVAL_RESIDENT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name", list(CASES))
def test_refused_before_staging(small, monkeypatch, capfd, name):
    lib, trn, tst, flt = small
    slots, env, filtered, exposure, text = CASES[name]
    set_env(monkeypatch, env)
    iopt, dopt = options(slots)
    best = [C.c_double(0.0) for _ in range(8)]
    args = [trn, tst, iopt, dopt, L1, L2, 2, 1] + [C.byref(b) for b in best]
    capfd.readouterr()
    if exposure:
        rc = lib.Py_SLIM_MselectExposure(*(args + [flt if filtered else None, None]))
    elif filtered:
        rc = lib.Py_SLIM_MselectFiltered(*(args + [flt]))
    else:
        rc = lib.Py_SLIM_Mselect(*args)
    C.CDLL(None).fflush(None)
    out = capfd.readouterr().out
    print(repr(_lib.last_error()))
    assert rc == SLIM_ERROR_INPUT
    assert _lib.last_error() == text
    assert "l1r:" not in out and "Estimating" not in out, out


@pytest.mark.parametrize("name", ["negs_admm", "expo_nrcmds200", "filter_admm"])
def test_a_refused_open_leaves_its_out_argument_alone(small, monkeypatch, name):
    lib, trn, tst, flt = small
    slots, env, filtered, exposure, text = CASES[name]
    set_env(monkeypatch, env)
    iopt, dopt = options({**slots, **({Opt.GPU_EVALEXPOSURE: 1} if exposure else {})})
    mark = 0x5A5A5A5A
    grid = C.c_void_p(mark)
    rc = lib.SLIMGPU_GridOpen(trn, tst, iopt, dopt, 0, 2, flt if filtered else None, C.byref(grid))
    assert rc == SLIM_ERROR_INPUT and _lib.last_error() == text
    assert grid.value == mark


def test_freeing_no_grid_is_a_no_op():
    lib = _lib.load()
    grid = C.c_void_p(None)
    lib.SLIMGPU_GridFree(C.byref(grid))
    assert grid.value is None
    lib.SLIMGPU_GridFree(None)
