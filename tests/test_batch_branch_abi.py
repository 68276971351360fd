"""Branching without a device: the symbols and lpg_branch_t are declared, and
the refusals that do not depend on the parent batch are answered before any
HIP call, naming the offending index. The refusals that read the parent's
shapes (src, row, the child's dimensions, a Big-M parent, nmask) need a batch,
which needs a device: tests/test_gpu_batch_branch.py has them."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


def test_symbols_constants_and_struct_size(lib):
    import linearprogramming_amd as lpg
    from linearprogramming_amd import _lib
    assert ctypes.sizeof(_lib.Branch) == 24
    assert [f[0] for f in _lib.Branch._fields_] == ["row", "col", "value"]
    names = {name for name, _, _ in _lib.PROTOTYPES}
    assert {"lpg_batch_branch_select", "lpg_batch_branch", "lpg_batch_active_columns"} <= names
    for name in ("lpg_batch_branch_select", "lpg_batch_branch", "lpg_batch_active_columns"):
        assert getattr(lib, name)
    assert (lpg.BRANCH_MOST_FRACTIONAL, lpg.BRANCH_FIRST) == (0, 1)
    header = open(_lib.os.path.join(_lib._SRC_ROOT, "include", "lpg.h")).read()
    assert "#define LPG_BRANCH_MOST_FRACTIONAL 0" in header and "#define LPG_BRANCH_FIRST           1" in header
    for method in ("branch_select", "branch", "active_columns"):
        assert callable(getattr(lpg.BatchEngine, method)) and callable(getattr(lpg.RaggedBatchEngine, method))


def _branch(lib, n, src, row, d, child=True):
    from linearprogramming_amd import _lib
    out = ctypes.c_void_p(1)
    arr = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((src, np.int64), (row, np.int64), (d, np.int8))]
    ptr = [None if a is None else a.ctypes.data_as(t) for a, t in zip(arr, (_lib.c_int64_p, _lib.c_int64_p, _lib.c_int8_p))]
    rc = lib.lpg_batch_branch(ctypes.byref(out) if child else None, None, n, *ptr)
    return rc, out, lib.lpg_batch_last_error(None).decode()


@pytest.mark.parametrize("n,src,row,d,words", [
    (0, [0], [0], [1], ["n = 0"]),
    (-3, [0], [0], [1], ["n = -3"]),
    (1, None, [0], [1], ["src is NULL"]),
    (1, [0], None, [1], ["row is NULL"]),
    (1, [0], [0], None, ["dir is NULL"]),
    (3, [0, 0, 0], [0, 0, 0], [1, -1, 0], ["dir[2] = 0"]),
    (3, [0, 0, 0], [0, 0, 0], [1, 2, -3], ["dir[1] = 2"]),          # the first offending index
    (2, [0, 0], [0, 0], [-1, 1], ["parent is NULL"]),
])
def test_branch_refuses_before_any_device_work_and_names_the_index(lib, n, src, row, d, words):
    from linearprogramming_amd import _lib
    rc, out, msg = _branch(lib, n, src, row, d)
    assert rc == _lib.ERR_ARG
    assert not out.value                                 # *child cleared
    assert msg.startswith("lpg_batch_branch:"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_null_arguments_are_errors_not_crashes(lib):
    from linearprogramming_amd import _lib
    rc, _, msg = _branch(lib, 1, [0], [0], [1], child=False)
    assert rc == _lib.ERR_ARG and "child is NULL" in msg
    mask = np.ones(4, dtype=np.uint8)
    out = (_lib.Branch * 1)()
    assert lib.lpg_batch_branch_select(None, mask.ctypes.data_as(_lib.c_uint8_p), 4, 0, 1e-6, 0, out) == _lib.ERR_ARG
    assert b"batch is NULL" in lib.lpg_batch_last_error(None)
    assert lib.lpg_batch_active_columns(None, 0, None, None) == _lib.ERR_ARG


def test_text_variables_and_integer_mask():
    from linearprogramming_amd import frontend as F
    text = "OF {\n\tmax:z=-x1+4x2+x3\n}\nST {\n\tx1>=-2;\n\tx1+2x2+x3<=1;\n\tx2>=0;\n\tx3<=0\n}\n"
    assert F.text_variables(text) == ["x1", "x2", "x3"]
    sm = F.build_smatrix(text)
    it = sm.vars.get("x1")
    mask = F.integer_mask(sm, ["x1", "x3"])
    want = {it.former, it.latter, "x3"}                   # both columns of the free x1, the inverted column of x3
    assert {v for v, k in zip(sm.names, mask) if k} == want and mask.dtype == np.uint8
    assert sm.inverted[sm.names.index("x3")]
    assert not F.integer_mask(sm, []).any()
    with pytest.raises(F.FrontendError, match="x9"):
        F.integer_mask(sm, ["x9"])
