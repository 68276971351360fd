"""Scenarios without a device: the symbols, prototypes and methods are
declared, and the refusals that do not depend on the parent batch are answered
before any HIP call, naming the call and the argument. The refusals that read
the parent (a Big-M parent, src, ident, a non-finite rhs) need a batch, which
needs a device: tests/test_gpu_batch_scenario.py has them."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


def test_symbols_prototypes_and_methods(lib):
    import linearprogramming_amd as lpg
    from linearprogramming_amd import _lib, frontend
    protos = {name: (res, args) for name, res, args in _lib.PROTOTYPES}
    assert protos["lpg_batch_scenario"] == (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int64,
                                                           _lib.c_int64_p, _lib.c_int64_p, _lib.c_double_p])
    assert protos["lpg_batch_set_rhs"] == (ctypes.c_int, [ctypes.c_void_p, _lib.c_int64_p, _lib.c_double_p])
    for name in ("lpg_batch_scenario", "lpg_batch_set_rhs"):
        assert getattr(lib, name)
    header = open(_lib.os.path.join(_lib._SRC_ROOT, "include", "lpg.h")).read()
    assert "int  lpg_batch_scenario(lpg_batch **child, lpg_batch *parent, int64_t n, const int64_t *src," in header
    assert "int  lpg_batch_set_rhs(lpg_batch *b, const int64_t *ident, const double *rhs);" in header
    for method in ("scenario", "set_rhs"):
        assert callable(getattr(lpg.BatchEngine, method)) and callable(getattr(lpg.RaggedBatchEngine, method))
    assert callable(frontend.solve_scenarios)


def _scenario(lib, n, src, ident, rhs, child=True):
    from linearprogramming_amd import _lib
    out = ctypes.c_void_p(1)
    arr = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((src, np.int64), (ident, np.int64), (rhs, np.float64))]
    ptr = [None if a is None else a.ctypes.data_as(t) for a, t in zip(arr, (_lib.c_int64_p, _lib.c_int64_p, _lib.c_double_p))]
    rc = lib.lpg_batch_scenario(ctypes.byref(out) if child else None, None, n, *ptr)
    return rc, out, lib.lpg_batch_last_error(None).decode()


@pytest.mark.parametrize("n,src,ident,rhs,words", [
    (0, [0], [1], [1.0], ["n = 0"]),
    (-2, [0], [1], [1.0], ["n = -2"]),
    (0, None, None, None, ["n = 0"]),                       # n before the arrays
    (1, None, [1], [1.0], ["src is NULL"]),
    (1, [0], None, [1.0], ["ident is NULL"]),
    (1, [0], [1], None, ["rhs is NULL"]),
    (1, None, None, None, ["src is NULL"]),                 # the first of them
    (2, [0, 0], [1], [1.0, 2.0], ["parent is NULL"]),
    (1, [7], [0], [float("nan")], ["parent is NULL"]),       # what needs a parent is not looked at without one
])
def test_scenario_refuses_before_any_device_work_and_names_the_argument(lib, n, src, ident, rhs, words):
    from linearprogramming_amd import _lib
    rc, out, msg = _scenario(lib, n, src, ident, rhs)
    assert rc == _lib.ERR_ARG
    assert not out.value                                 # *child cleared
    assert msg.startswith("lpg_batch_scenario:"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_null_arguments_are_errors_not_crashes(lib):
    from linearprogramming_amd import _lib
    rc, _, msg = _scenario(lib, 1, [0], [1], [1.0], child=False)
    assert rc == _lib.ERR_ARG and msg.startswith("lpg_batch_scenario:") and "child is NULL" in msg
    ident, rhs = np.ones(1, dtype=np.int64), np.ones(1)
    assert lib.lpg_batch_set_rhs(None, ident.ctypes.data_as(_lib.c_int64_p), rhs.ctypes.data_as(_lib.c_double_p)) == _lib.ERR_ARG
    msg = lib.lpg_batch_last_error(None).decode()
    assert msg.startswith("lpg_batch_set_rhs:") and "batch is NULL" in msg
