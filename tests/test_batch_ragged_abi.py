"""Ragged batches without a device: lpg_batch_create_ragged refuses bad
arguments before any HIP call and names the first offending LP, NULL handles
to the packed and _ragged calls are errors, and BatchEngine.ragged raises with
the library's message."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


def _i64(xs):
    from linearprogramming_amd import _lib
    a = np.ascontiguousarray(xs, dtype=np.int64)
    return a, a.ctypes.data_as(_lib.c_int64_p)


def _create(lib, count, m, ncols, nobj=1, flags=0):
    b = ctypes.c_void_p(1)
    km, pm = (None, None) if m is None else _i64(m)
    kn, pn = (None, None) if ncols is None else _i64(ncols)
    rc = lib.lpg_batch_create_ragged(ctypes.byref(b), 0, count, pm, pn, nobj, flags)
    del km, kn
    return rc, b, lib.lpg_batch_last_error(None).decode()


@pytest.mark.parametrize("count,m,ncols,nobj,flags,words", [
    (3, None, [9, 9, 9], 1, 0, ["m is NULL"]),
    (3, [4, 4, 4], None, 1, 0, ["ncols is NULL"]),
    (0, [4], [9], 1, 0, ["count"]),
    (-2, [4], [9], 1, 0, ["count"]),
    (3, [4, 4, 0], [9, 9, 9], 1, 0, ["LP 2", "m = 0"]),                    # the third LP has no row
    (3, [4, 0, 0], [9, 9, 1], 1, 0, ["LP 1", "m = 0"]),                    # the first offending LP is named
    (3, [4, 4, 4], [9, 1, 9], 1, 0, ["LP 1", "ncols = 1"]),
    (2, [4, 8192], [9, 9], 1, 0, ["LP 1", "m + 1 = 8193", "lpg_create"]),  # m + 1 > LPG_BATCH_MAX_DIM
    (2, [8191, 4], [9, 9], 2, 0, ["LP 0", "m + 2 = 8193", "lpg_create"]),  # m + 2 > LPG_BATCH_MAX_DIM (plain: fine)
    (2, [4, 4], [9, 8193], 1, 0, ["LP 1", "ncols = 8193", "lpg_create"]),
    (2, [4, 4], [9, 9], 1, 0x4, ["flags"]),                                 # LPG_FLAG_BIG_M: nobj says it
    (2, [4, 4], [9, 9], 1, 0x8, ["flags"]),                                 # LPG_FLAG_EAGER
    (2, [4, 4], [9, 9], 1, 0x2, ["flags"]),                                 # LPG_FLAG_NO_SKIP
    (2, [4, 4], [9, 9], 0, 0, ["nobj = 0"]),
    (2, [4, 4], [9, 9], 3, 0, ["nobj = 3"]),
])
def test_create_ragged_refuses_bad_arguments_and_names_the_lp(lib, count, m, ncols, nobj, flags, words):
    from linearprogramming_amd import _lib
    rc, b, msg = _create(lib, count, m, ncols, nobj, flags)
    assert rc == _lib.ERR_ARG
    assert not b.value                                   # *out cleared
    assert msg.startswith("lpg_batch_create_ragged:"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_create_ragged_refuses_more_rows_than_2_31(lib):
    """262144 LPs of m + 1 = 8192 rows hold 2^31 rows; one LP fewer would pass this check."""
    from linearprogramming_amd import _lib
    count = 1 << 18
    rc, b, msg = _create(lib, count, np.full(count, 8191), np.full(count, 2))
    assert rc == _lib.ERR_ARG and not b.value
    assert "2^31" in msg and f"LP {count - 1}" in msg, msg


def test_out_null_is_an_argument_error(lib):
    from linearprogramming_amd import _lib
    k, p = _i64([4])
    assert lib.lpg_batch_create_ragged(None, 0, 1, p, p, 1, 0) == _lib.ERR_ARG
    assert b"NULL" in lib.lpg_batch_last_error(None)


def test_null_handles_to_the_new_calls_are_errors_not_crashes(lib):
    from linearprogramming_amd import _lib
    shp = _lib.BatchShape()
    buf = np.zeros(4)
    ibuf, ip = _i64([2, 2])
    res = (_lib.Result * 1)()
    dp = buf.ctypes.data_as(_lib.c_double_p)
    assert lib.lpg_batch_shape(None, 0, ctypes.byref(shp)) == _lib.ERR_ARG
    assert lib.lpg_batch_shape(None, 0, None) == _lib.ERR_ARG
    assert lib.lpg_batch_load_packed(None, 0, 1, dp, None) == _lib.ERR_ARG
    assert lib.lpg_batch_get_rows_packed(None, 0, 1, dp) == _lib.ERR_ARG
    assert lib.lpg_batch_get_basis_packed(None, 0, 1, ip) == _lib.ERR_ARG
    assert lib.lpg_batch_set_objective_packed(None, dp) == _lib.ERR_ARG
    assert lib.lpg_batch_solve_two_phase_ragged(None, ip, None, 10, 0, res) == _lib.ERR_ARG
    assert lib.lpg_batch_solve_big_m_ragged(None, ip, None, 10, 0, res) == _lib.ERR_ARG
    assert b"NULL" in lib.lpg_batch_last_error(None)


def test_python_wrapper_raises_with_the_message():
    import linearprogramming_amd as lpg
    with pytest.raises(lpg.LPGError, match=r"lpg_batch_create_ragged rc=-1.*LP 1: ncols = 1"):
        lpg.BatchEngine.ragged([(4, 9), (4, 1), (0, 9)])
    with pytest.raises(lpg.LPGError, match=r"lpg_batch_create_ragged rc=-1.*LP 0: m \+ 2 = 8193"):
        lpg.BatchEngine.ragged([(8191, 9)], big_m=True)
    with pytest.raises(lpg.LPGError, match="count"):
        lpg.BatchEngine.ragged([])
    with pytest.raises(lpg.LPGError, match="shapes"):
        lpg.BatchEngine.ragged([4, 9])


def test_batch_shape_is_64_bytes_and_declared():
    from linearprogramming_amd import _lib
    assert ctypes.sizeof(_lib.BatchShape) == 64
    names = {name for name, _, _ in _lib.PROTOTYPES}
    assert {"lpg_batch_create_ragged", "lpg_batch_shape", "lpg_batch_load_packed", "lpg_batch_get_rows_packed",
            "lpg_batch_get_basis_packed", "lpg_batch_set_objective_packed", "lpg_batch_solve_two_phase_ragged",
            "lpg_batch_solve_big_m_ragged"} <= names
