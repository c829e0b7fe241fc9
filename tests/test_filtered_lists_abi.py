"""Refusals of the filtered list calls (include/slim_gpu_filter.h) on the device: SLIM_ERROR_INPUT, a
SLIMGPU_LastError text, outputs untouched -- a filter made for another number of items at each of the three entry
points, the bounds of slim_gpu_lists.h under a filter, and SLIMGPU_FilterCreate's own checks."""
import numpy as np
import pytest
import scipy.sparse as sp

from filtered_cases import P, cases_fixture, make_filter
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK

pytestmark = pytest.mark.gpu
cases = pytest.fixture(scope="module")(cases_fixture)


def untouched_call(fn, n, nslots, *args):
    ids = np.full((8, nslots), -1, np.int32)
    sc = np.zeros((8, nslots), np.float32)
    cnt = np.full(8, -7, np.int32)
    rc = fn(n, *args, P(ids), P(sc), P(cnt))
    return rc, bool((ids == -1).all() and (sc == 0).all() and (cnt == -7).all()), _lib.last_error()


def test_refusals_leave_the_outputs_untouched(cases):
    c = cases("ties")
    lib = c.lib
    entries = ((lib.SLIMGPU_PredictListsFiltered, lambda f: (c.hw, c.hr, f)),
               (lib.SLIMGPU_ModelPredictListsFiltered, lambda f: (c.model.handle, c.hr, f)),
               (lib.SLIMGPU_MatrixPredictListsFiltered, lambda f: (c.model.handle, c.mat.handle, 0, None, f)))
    # a filter made for another number of items
    for ncols in (c.ncols - 1, c.ncols + 1):
        rc, flt = make_filter(lib, ncols, allowed=[0, 5])
        assert rc == SLIM_OK
        for fn, args in entries:
            for n in (10, 128, 300):
                rc, clean, err = untouched_call(fn, n, n, *args(flt))
                assert rc == SLIM_ERROR_INPUT and clean and str(ncols) in err and str(c.ncols) in err, fn.__name__
        lib.SLIMGPU_FilterFree(flt)
    # the bounds of the list calls hold under a filter
    rc, flt = make_filter(lib, c.ncols, allowed=[0, 5])
    assert rc == SLIM_OK
    for fn, args in entries:
        for n in (4097, 0, -3):
            rc, clean, err = untouched_call(fn, n, 4097, *args(flt))
            assert rc == SLIM_ERROR_INPUT and clean and err, fn.__name__
    lib.SLIMGPU_FilterFree(flt)
    # ids out of range and a bad xptr never make a filter
    good = sp.csr_matrix(np.eye(3, c.ncols, dtype=np.float32))
    for kw in ({"allowed": [c.ncols]}, {"blocked": [-1]}):
        rc, h = make_filter(lib, c.ncols, **kw)
        assert rc == SLIM_ERROR_INPUT and not h.value and "SLIMGPU_FilterCreate" in _lib.last_error()
    for ptr, ind in (([1, 1, 2, 3], [0, 1, 2]), ([0, 2, 1, 3], [0, 1, 2]), ([0, 1, 2, 3], [0, 1, c.ncols])):
        X = sp.csr_matrix(good)
        X.indptr, X.indices = np.array(ptr, np.int64), np.array(ind, np.int32)
        rc, h = make_filter(lib, c.ncols, X=X)
        assert rc == SLIM_ERROR_INPUT and not h.value and "SLIMGPU_FilterCreate" in _lib.last_error()
