"""Goal batches without a device: the new prototypes and LPG_GOAL_MAX_LEVELS in
include/lpg.h and _lib.py, lpg_batch_info_t unchanged, and every refusal of
lpg_batch_create_goal / lpg_batch_solve_goal that needs no batch, with its
message. The refusals of lpg_batch_solve_goal that need a batch (NULL cost, the
two pitches, max_pivots, the rule) happen before any launch too, but a batch
needs a device: tests/test_gpu_batch_goal.py has them.
"""
from __future__ import annotations

import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "lpg.h")


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


def test_header_and_bindings_agree():
    from linearprogramming_amd import _lib
    import linearprogramming_amd as lpg
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert ("int lpg_batch_create_goal(lpg_batch **out, int device, int64_t count, int64_t m, int64_t ncols, int nlevels, "
            "uint32_t flags);") in hdr
    assert ("int lpg_batch_solve_goal(lpg_batch *b, const double *cost, int64_t ld_lp, int64_t ld_level, int64_t max_pivots, "
            "int rule, lpg_result *res, double *attain );") in hdr
    assert "#define LPG_GOAL_MAX_LEVELS 8" in hdr and _lib.GOAL_MAX_LEVELS == 8 == lpg.GOAL_MAX_LEVELS
    lib = _lib.load()
    create, solve = lib.lpg_batch_create_goal, lib.lpg_batch_solve_goal
    assert create.restype is ctypes.c_int and solve.restype is ctypes.c_int
    assert create.argtypes == [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                               ctypes.c_int, ctypes.c_uint32]
    assert solve.argtypes == [ctypes.c_void_p, _lib.c_double_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                              ctypes.POINTER(_lib.Result), _lib.c_double_p]


def test_batch_info_is_still_64_bytes_and_ends_with_nobj():
    from linearprogramming_amd import _lib
    names = [f[0] for f in _lib.BatchInfo._fields_]
    assert names[-2:] == ["nobj", "pad"] and ctypes.sizeof(_lib.BatchInfo) == 64
    hdr = open(HEADER).read()
    body = hdr[hdr.index("typedef struct {\n    int64_t count, m, ncols, ld;"):hdr.index("} lpg_batch_info_t;")]
    assert body.rstrip().endswith("int32_t pad;") and "int32_t nobj;" in body and "goal batch" in body


def test_null_arguments(lib):
    from linearprogramming_amd import _lib
    res = (_lib.Result * 1)()
    cost = (ctypes.c_double * 4)()
    assert lib.lpg_batch_solve_goal(None, cost, 4, 4, 10, 0, res, None) == _lib.ERR_ARG
    assert b"NULL" in lib.lpg_batch_last_error(None)
    assert lib.lpg_batch_create_goal(None, 0, 4, 4, 9, 3, 0) == _lib.ERR_ARG
    assert b"NULL" in lib.lpg_batch_last_error(None)


@pytest.mark.parametrize("count,m,ncols,nlevels,flags,words", [
    (4, 4, 9, 0, 0, ["nlevels = 0", "1..8"]),
    (4, 4, 9, 9, 0, ["nlevels = 9", "LPG_GOAL_MAX_LEVELS"]),
    (4, 4, 9, -1, 0, ["nlevels = -1"]),
    (0, 4, 9, 3, 0, ["count"]),
    (4, 0, 9, 3, 0, ["m"]),
    (4, 4, 1, 3, 0, ["ncols"]),
    (4, 4, 9, 3, 0x4, ["flags"]),                   # LPG_FLAG_BIG_M
    (4, 4, 9, 3, 0x8, ["flags"]),                   # LPG_FLAG_EAGER
    (4, 4, 9, 3, 0x2, ["flags"]),                   # LPG_FLAG_NO_SKIP
    (4, 4, 8193, 3, 0, ["lpg_create"]),             # ncols > LPG_BATCH_MAX_DIM
    (4, 8190, 9, 3, 0, ["m + 3 = 8193", "lpg_create"]),     # m + K > LPG_BATCH_MAX_DIM (K = 2 takes this m)
    (4, 8185, 9, 8, 0, ["m + 8 = 8193", "lpg_create"]),
    (1 << 20, 2045, 9, 3, 0, ["count * (m + 3)", "2^31"]),  # count * (m + K) = 2^31 exactly
    (1 << 20, 2040, 9, 8, 0, ["count * (m + 8)", "2^31"]),
])
def test_create_goal_refuses_bad_arguments_with_a_message(lib, count, m, ncols, nlevels, flags, words):
    from linearprogramming_amd import _lib
    b = ctypes.c_void_p(1)
    assert lib.lpg_batch_create_goal(ctypes.byref(b), 0, count, m, ncols, nlevels, flags) == _lib.ERR_ARG
    assert not b.value                                   # *out cleared
    msg = lib.lpg_batch_last_error(None).decode()
    assert msg.startswith("lpg_batch_create_goal:") and all(w in msg for w in words), msg


def test_python_wrapper_names_the_constructor_and_the_kinds_exclude_each_other():
    import linearprogramming_amd as lpg
    with pytest.raises(lpg.LPGError, match="lpg_batch_create_goal rc=-1.*nlevels = 9"):
        lpg.BatchEngine(4, 4, 9, levels=9)
    with pytest.raises(lpg.LPGError, match="lpg_batch_create_goal rc=-1.*bad shape"):
        lpg.BatchEngine(0, 4, 9, levels=3)
    with pytest.raises(lpg.LPGError, match="exclude each other"):
        lpg.BatchEngine(4, 4, 9, big_m=True, levels=2)


def test_ragged_batches_still_have_one_or_two_objective_rows(lib):
    from linearprogramming_amd import _lib
    b = ctypes.c_void_p(1)
    arr = (ctypes.c_int64 * 2)(4, 5)
    assert lib.lpg_batch_create_ragged(ctypes.byref(b), 0, 2, arr, arr, 3, 0) == _lib.ERR_ARG
    assert b"nobj = 3" in lib.lpg_batch_last_error(None)
