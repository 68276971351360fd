"""lpg_assign's host-side validation and build wiring (no GPU: every check here
is answered before the library touches a device; a batch's device side is made
by the first call that passes its checks)."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


@pytest.fixture()
def batch(lib):
    """Two 2 x 3 problems; no device has been touched."""
    a = ctypes.c_void_p()
    assert lib.lpg_assign_create(ctypes.byref(a), 0, 2, 2, 3, 0) == 0
    yield a
    lib.lpg_assign_destroy(a)


def dp(x):
    from linearprogramming_amd import _lib
    return x.ctypes.data_as(_lib.c_double_p)


@pytest.mark.parametrize("count,nr,nc,flags,word", [
    (0, 2, 2, 0, "count"),
    (2, 0, 2, 0, "nr"),
    (2, 3, 2, 0, "transposed"),             # nr > nc
    (2, 2, 8193, 0, "LPG_BATCH_MAX_DIM"),   # a dimension over the cap
    (2, 2, 2, 0x2, "flags"),
    (2, 2, 2, 0x80000000, "flags"),
])
def test_create_refuses_bad_arguments_with_a_message(lib, count, nr, nc, flags, word):
    from linearprogramming_amd import _lib
    a = ctypes.c_void_p(1)
    assert lib.lpg_assign_create(ctypes.byref(a), 0, count, nr, nc, flags) == _lib.ERR_ARG
    assert not a.value                                   # *out cleared
    msg = lib.lpg_assign_last_error(None).decode()
    assert "lpg_assign_create" in msg and word in msg, msg


def test_python_wrapper_raises_with_the_message():
    import linearprogramming_amd as lpg
    with pytest.raises(lpg.LPGError, match="rc=-1.*bad shape"):
        lpg.AssignmentBatch(4, 5, 4)


def test_null_handles_and_out_pointers_are_errors_not_crashes(lib, batch):
    from linearprogramming_amd import _lib
    lib.lpg_assign_destroy(None)
    assert lib.lpg_assign_create(None, 0, 1, 1, 1, 0) == _lib.ERR_ARG
    c = np.zeros(6)
    assert lib.lpg_assign_load(None, 0, 1, dp(c), 3) == _lib.ERR_ARG
    assert lib.lpg_assign_generate(None, 1, 10) == _lib.ERR_ARG
    assert lib.lpg_assign_solve(None, None) == _lib.ERR_ARG
    assert lib.lpg_assign_get(None, 0, 1, None, None, None) == _lib.ERR_ARG
    assert lib.lpg_assign_info(None, None) == _lib.ERR_ARG
    assert "NULL" in lib.lpg_assign_last_error(None).decode()
    assert lib.lpg_assign_info(batch, None) == _lib.ERR_ARG
    assert "out is NULL" in lib.lpg_assign_last_error(batch).decode()
    assert lib.lpg_assign_load(batch, 0, 1, None, 3) == _lib.ERR_ARG
    assert "costs is NULL" in lib.lpg_assign_last_error(batch).decode()


def test_info_reports_shape_and_form(lib, batch):
    from linearprogramming_amd import _lib
    i = _lib.AssignInfo()
    assert lib.lpg_assign_info(batch, ctypes.byref(i)) == 0
    assert (i.count, i.nr, i.nc) == (2, 2, 3)
    assert i.form == _lib.ASSIGN_FORM_WAVE and i.tier == _lib.BATCH_TIER_LDS
    assert i.lds_bytes == 4 * 8 * (2 * 3 + 2)


def test_load_refuses_a_bad_range_and_pitch(lib, batch):
    from linearprogramming_amd import _lib
    c = np.zeros((2, 2, 3))
    assert lib.lpg_assign_load(batch, 0, 2, dp(c), 2) == _lib.ERR_ARG
    assert "ld 2 < nc = 3" in lib.lpg_assign_last_error(batch).decode()
    for first, n in ((-1, 1), (0, 0), (1, 2), (3, 1)):
        assert lib.lpg_assign_load(batch, first, n, dp(c), 3) == _lib.ERR_ARG, (first, n)
        assert "outside the batch" in lib.lpg_assign_last_error(batch).decode()


@pytest.mark.parametrize("value,word", [(float("nan"), "NaN"), (float("-inf"), "-inf"), (2.0 ** 1001, "cap"),
                                        (-(2.0 ** 1001), "cap")])
def test_load_refuses_a_bad_entry_and_names_it(lib, batch, value, word):
    from linearprogramming_amd import _lib
    c = np.zeros((2, 2, 3))
    c[0, 0, 1] = float("inf")                 # +inf is a forbidden pair, not an error
    c[0, 1, 0] = 2.0 ** 1000                  # the cap itself passes
    c[1, 1, 2] = value
    assert lib.lpg_assign_load(batch, 0, 2, dp(c), 3) == _lib.ERR_ARG
    msg = lib.lpg_assign_last_error(batch).decode()
    assert "lpg_assign_load" in msg and "problem 1, entry (1, 2)" in msg and word in msg, msg
    # the problem's index is the batch's, not the call's
    assert lib.lpg_assign_load(batch, 1, 1, dp(c[1:]), 3) == _lib.ERR_ARG
    assert "problem 1, entry (1, 2)" in lib.lpg_assign_last_error(batch).decode()


def test_generate_refuses_a_bad_range(lib, batch):
    from linearprogramming_amd import _lib
    for r in (0, -5, (1 << 53) + 1):
        assert lib.lpg_assign_generate(batch, 1, r) == _lib.ERR_ARG
        assert "range" in lib.lpg_assign_last_error(batch).decode()


def test_solve_and_get_before_costs(lib, batch):
    from linearprogramming_amd import _lib
    assert lib.lpg_assign_solve(batch, None) == _lib.ERR_STATE
    assert "problem 0 has no costs" in lib.lpg_assign_last_error(batch).decode()
    col = np.zeros(4, dtype=np.int64)
    assert lib.lpg_assign_get(batch, 0, 2, col.ctypes.data_as(_lib.c_int64_p), None, None) == _lib.ERR_STATE
    assert lib.lpg_assign_get(batch, 0, 2, None, None, None) == _lib.ERR_ARG
    assert "all NULL" in lib.lpg_assign_last_error(batch).decode()
    assert lib.lpg_assign_get(batch, 1, 2, col.ctypes.data_as(_lib.c_int64_p), None, None) == _lib.ERR_ARG
    assert "outside the batch" in lib.lpg_assign_last_error(batch).decode()


def test_every_source_list_names_the_assignment_file():
    """As tests/test_batch_abi.py's check for lpg_batch.hip: the product objects and the two lab libraries are
    built from explicit lists."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    kobjs = re.search(r"^KOBJS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "$(OBJDIR)/lpg_assign.o" in kobjs
    for target in ("tools/probe/liblpg_phases.so", "tools/probe/liblpg_pub.so"):
        rule = re.search(r"^" + re.escape(target) + r":(.*)\n\t.*\n\t(.*)$", mk, flags=re.M)
        assert rule, target
        assert "$(CSRC)/lpg_assign.hip" in rule.group(1), target      # prerequisites
        assert "$(CSRC)/lpg_assign.hip" in rule.group(2), target      # the compile line
