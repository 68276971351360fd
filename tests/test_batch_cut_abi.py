"""Cuts without a device: the symbols, LPG_BATCH_MAX_CUTS and the methods are
declared, and the refusals that do not depend on the parent batch are answered
with LPG_ERR_ARG before any HIP call, *child cleared and the offending index
named. The refusals that read the parent's shapes (src, rows, the cap, the
child's dimensions, a Big-M parent, nmask) need a batch, which needs a device:
tests/test_gpu_batch_cut.py has them."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


def test_symbols_constant_and_methods(lib):
    import linearprogramming_amd as lpg
    from linearprogramming_amd import _lib
    names = {name for name, _, _ in _lib.PROTOTYPES}
    assert {"lpg_batch_cut_select", "lpg_batch_cut"} <= names
    for name in ("lpg_batch_cut_select", "lpg_batch_cut"):
        assert getattr(lib, name)
    assert lpg.BATCH_MAX_CUTS == _lib.BATCH_MAX_CUTS == 1024
    header = open(_lib.os.path.join(_lib._SRC_ROOT, "include", "lpg.h")).read()
    assert "#define LPG_BATCH_MAX_CUTS 1024" in header
    for method in ("cut_select", "cut"):
        assert callable(getattr(lpg.BatchEngine, method)) and callable(getattr(lpg.RaggedBatchEngine, method))
    import inspect
    from linearprogramming_amd import frontend as F
    for fn in (F.solve_ilp, F.solve_ilp_text):
        p = inspect.signature(fn).parameters
        assert p["cut_rounds"].default == 0 and p["max_cuts"].default == 8


def _ptr(a, dtype, ctype):
    if a is None:
        return None, None
    arr = np.ascontiguousarray(a, dtype=dtype)
    return arr, arr.ctypes.data_as(ctype)


def _cut(lib, n, src, first, rows, mask, child=True):
    from linearprogramming_amd import _lib
    out = ctypes.c_void_p(1)
    keep = [_ptr(src, np.int64, _lib.c_int64_p), _ptr(first, np.int64, _lib.c_int64_p), _ptr(rows, np.int64, _lib.c_int64_p),
            _ptr(mask, np.uint8, _lib.c_uint8_p)]
    rc = lib.lpg_batch_cut(ctypes.byref(out) if child else None, None, n, *[p for _, p in keep], 4, 0)
    return rc, out, lib.lpg_batch_last_error(None).decode()


ONES = [1, 1, 1, 1]


@pytest.mark.parametrize("n,src,first,rows,mask,words", [
    (0, [0], [0, 1], [0], ONES, ["n = 0"]),
    (-2, [0], [0, 1], [0], ONES, ["n = -2"]),
    (1, None, [0, 1], [0], ONES, ["src is NULL"]),
    (1, [0], None, [0], ONES, ["first is NULL"]),
    (1, [0], [0, 1], None, ONES, ["rows is NULL"]),
    (1, [0], [0, 1], [0], None, ["mask is NULL"]),
    (2, [0, 0], [1, 2, 3], [0, 0, 0], ONES, ["first[0] = 1"]),
    (3, [0, 0, 0], [0, 1, 1, 2], [0, 0], ONES, ["first[2] = 1", "first[1] = 1"]),          # an empty interval
    (3, [0, 0, 0], [0, 2, 1, 3], [0, 1, 2], ONES, ["first[2] = 1", "first[1] = 2"]),       # a descending one
    (3, [0, 0, 0], [0, 0, 0, 0], [0], ONES, ["first[1] = 0", "first[0] = 0"]),             # the first offending index
    (2, [0, 0], [0, 1, 2], [0, 0], ONES, ["parent is NULL"]),
])
def test_cut_refuses_before_any_device_work_and_names_the_index(lib, n, src, first, rows, mask, words):
    from linearprogramming_amd import _lib
    rc, out, msg = _cut(lib, n, src, first, rows, mask)
    assert rc == _lib.ERR_ARG
    assert not out.value                                 # *child cleared
    assert msg.startswith("lpg_batch_cut:"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_null_child_is_an_error_not_a_crash(lib):
    from linearprogramming_amd import _lib
    rc, _, msg = _cut(lib, 1, [0], [0, 1], [0], ONES, child=False)
    assert rc == _lib.ERR_ARG and "lpg_batch_cut: child is NULL" in msg


@pytest.mark.parametrize("mask,ncut,rows,int_tol,max_cuts,words", [
    (None, True, True, 1e-6, 8, ["mask is NULL"]),
    (ONES, False, True, 1e-6, 8, ["ncut is NULL"]),
    (ONES, True, False, 1e-6, 8, ["rows is NULL"]),
    (ONES, True, True, 1e-6, 0, ["max_cuts = 0"]),
    (ONES, True, True, 1e-6, -5, ["max_cuts = -5"]),
    (ONES, True, True, 0.5, 8, ["int_tol 0.5 outside [0, 0.5)"]),
    (ONES, True, True, -1e-9, 8, ["int_tol", "outside [0, 0.5)"]),
    (ONES, True, True, float("nan"), 8, ["int_tol", "outside [0, 0.5)"]),
    (ONES, True, True, 1e-6, 8, ["batch is NULL"]),
])
def test_cut_select_refuses_before_it_looks_at_the_batch(lib, mask, ncut, rows, int_tol, max_cuts, words):
    from linearprogramming_amd import _lib
    mk, mp = _ptr(mask, np.uint8, _lib.c_uint8_p)
    nc, rw = np.zeros(1, dtype=np.int64), np.zeros(8, dtype=np.int64)
    rc = lib.lpg_batch_cut_select(None, mp, 4, 0, int_tol, max_cuts, nc.ctypes.data_as(_lib.c_int64_p) if ncut else None,
                                  rw.ctypes.data_as(_lib.c_int64_p) if rows else None)
    msg = lib.lpg_batch_last_error(None).decode()
    assert rc == _lib.ERR_ARG and msg.startswith("lpg_batch_cut_select:"), msg
    for w in words:
        assert w in msg, (w, msg)
