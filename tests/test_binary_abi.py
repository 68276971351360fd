"""lpg_binary's host-side validation and build wiring (no GPU: every check here
is answered before the library touches a device; a batch's device side is made
by the first call that passes its checks)."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

M, N = 3, 4


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


@pytest.fixture()
def batch(lib):
    """Two problems of 3 rows and 4 columns; no device has been touched."""
    b = ctypes.c_void_p()
    assert lib.lpg_binary_create(ctypes.byref(b), 0, 2, M, N, 0, 0) == 0
    yield b
    lib.lpg_binary_destroy(b)


def dp(x):
    from linearprogramming_amd import _lib
    return x.ctypes.data_as(_lib.c_double_p)


def ip(x):
    from linearprogramming_amd import _lib
    return x.ctypes.data_as(_lib.c_int32_p)


def good(count=2, m=M, n=N):
    return np.ones((count, m, n)), np.zeros((count, m), dtype=np.int32), np.ones((count, m)), np.ones((count, n))


def load(lib, b, A, sense, rhs, c, first=0):
    return lib.lpg_binary_load(b, first, A.shape[0], dp(A), A.shape[2], ip(sense), dp(rhs), dp(c))


@pytest.mark.parametrize("count,m,n,split,flags,word", [
    (0, 2, 2, 0, 0, "count"),
    (2, 0, 2, 0, 0, "bad shape"),
    (2, 257, 2, 0, 0, "m <= 256"),
    (2, 2, 0, 0, 0, "bad shape"),
    (2, 2, 65, 0, 0, "n <= 64"),
    (2, 2, 2, -1, 0, "split"),
    (2, 2, 2, 3, 0, "split"),               # split > n
    (2, 2, 64, 11, 0, "split"),             # split > 10
    (1 << 22, 2, 64, 10, 0, "2^31"),        # count * 2^split
    (2, 2, 2, 0, 0x2, "flags"),
    (2, 2, 2, 0, 0x80000000, "flags"),
])
def test_create_refuses_bad_arguments_with_a_message(lib, count, m, n, split, flags, word):
    from linearprogramming_amd import _lib
    b = ctypes.c_void_p(1)
    assert lib.lpg_binary_create(ctypes.byref(b), 0, count, m, n, split, flags) == _lib.ERR_ARG
    assert not b.value                                   # *out cleared
    msg = lib.lpg_binary_last_error(None).decode()
    assert "lpg_binary_create" in msg and word in msg, msg


@pytest.mark.parametrize("m,n,split", [(256, 64, 10), (1, 1, 1), (1, 1, 0), (2, 3, 3)])
def test_create_accepts_the_limits(lib, m, n, split):
    b = ctypes.c_void_p()
    assert lib.lpg_binary_create(ctypes.byref(b), 0, 1, m, n, split, 1) == 0
    lib.lpg_binary_destroy(b)


def test_python_wrapper_raises_with_the_message():
    import linearprogramming_amd as lpg
    with pytest.raises(lpg.LPGError, match="rc=-1.*bad shape"):
        lpg.BinaryBatch(4, 5, 65)
    with lpg.BinaryBatch(2, M, N) as b:
        with pytest.raises(lpg.LPGError, match="shapes"):
            b.load(np.zeros((2, M, N + 1)), np.zeros((2, M)), np.zeros((2, M)), np.zeros((2, N)))


def test_null_handles_and_pointers_are_errors_not_crashes(lib, batch):
    from linearprogramming_amd import _lib
    A, sense, rhs, c = good()
    lib.lpg_binary_destroy(None)
    assert lib.lpg_binary_create(None, 0, 1, 1, 1, 0, 0) == _lib.ERR_ARG
    assert load(lib, None, A, sense, rhs, c) == _lib.ERR_ARG
    assert lib.lpg_binary_generate(None, 1, 0) == _lib.ERR_ARG
    assert lib.lpg_binary_solve(None, 0, None) == _lib.ERR_ARG
    assert lib.lpg_binary_get(None, 0, 1, None) == _lib.ERR_ARG
    assert lib.lpg_binary_occupancy(None, None) == _lib.ERR_ARG
    assert lib.lpg_binary_info(None, None) == _lib.ERR_ARG
    assert "NULL" in lib.lpg_binary_last_error(None).decode()
    assert lib.lpg_binary_info(batch, None) == _lib.ERR_ARG
    assert "out is NULL" in lib.lpg_binary_last_error(batch).decode()
    assert lib.lpg_binary_occupancy(batch, None) == _lib.ERR_ARG
    assert "resident_waves is NULL" in lib.lpg_binary_last_error(batch).decode()
    for k, word in enumerate(("A", "sense", "rhs", "c")):
        args = [dp(A), N, ip(sense), dp(rhs), dp(c)]
        args[k + (k > 0)] = None
        assert lib.lpg_binary_load(batch, 0, 2, *args) == _lib.ERR_ARG
        assert f"{word} is NULL" in lib.lpg_binary_last_error(batch).decode()


def test_info_reports_shape_split_and_instantiation(lib, batch, monkeypatch):
    from linearprogramming_amd import _lib
    i = _lib.BinaryInfo()
    assert lib.lpg_binary_info(batch, ctypes.byref(i)) == 0
    assert (i.count, i.m, i.n, i.split, i.rows_per_lane, i.tier) == (2, M, N, 0, 1, _lib.BATCH_TIER_LDS)
    assert i.lds_bytes == 4 * 8 * (M * N + N) and i.chunk == 4096 and i.launches == 0
    # (m, n, split) -> rows per lane, tier, LDS: four, two or one problem per workgroup
    for m, n, split, rpl, tier, lds in ((64, 64, 0, 1, 0, 4 * 8 * 65 * 64), (65, 33, 1, 2, 0, 2 * 8 * 66 * 33),
                                        (128, 63, 0, 2, 1, 0), (129, 64, 0, 4, 1, 0), (256, 64, 1, 4, 1, 0),
                                        (256, 64, 2, 4, 0, 8 * 257 * 64), (256, 64, 10, 4, 0, 8 * 257 * 64)):
        b = ctypes.c_void_p()
        assert lib.lpg_binary_create(ctypes.byref(b), 0, 3, m, n, split, 0) == 0
        assert lib.lpg_binary_info(b, ctypes.byref(i)) == 0
        assert (i.rows_per_lane, i.tier, i.lds_bytes, i.split) == (rpl, tier, lds, split), (m, n, split)
        lib.lpg_binary_destroy(b)
    monkeypatch.setenv("LPG_BINARY_TIER", "global")
    monkeypatch.setenv("LPG_BINARY_CHUNK", "3")
    b = ctypes.c_void_p()
    assert lib.lpg_binary_create(ctypes.byref(b), 0, 3, M, N, 0, 0) == 0
    assert lib.lpg_binary_info(b, ctypes.byref(i)) == 0
    assert (i.tier, i.lds_bytes, i.chunk) == (_lib.BATCH_TIER_GLOBAL, 0, 3)
    lib.lpg_binary_destroy(b)
    monkeypatch.setenv("LPG_BINARY_CHUNK", "0")
    assert lib.lpg_binary_create(ctypes.byref(b), 0, 3, M, N, 0, 0) == _lib.ERR_ARG
    assert "LPG_BINARY_CHUNK" in lib.lpg_binary_last_error(None).decode()


def test_load_refuses_a_bad_range_and_pitch(lib, batch):
    from linearprogramming_amd import _lib
    A, sense, rhs, c = good()
    assert lib.lpg_binary_load(batch, 0, 2, dp(A), N - 1, ip(sense), dp(rhs), dp(c)) == _lib.ERR_ARG
    assert "ldA 3 < n = 4" in lib.lpg_binary_last_error(batch).decode()
    for first, n in ((-1, 1), (0, 0), (1, 2), (3, 1)):
        assert lib.lpg_binary_load(batch, first, n, dp(A), N, ip(sense), dp(rhs), dp(c)) == _lib.ERR_ARG, (first, n)
        assert "outside the batch" in lib.lpg_binary_last_error(batch).decode()


POSITIONS = [(0, 0, 0), (1, 1, 2), (1, M - 1, N - 1)]      # the first, a middle and the last entry of the batch
BAD = [(float("nan"), "NaN"), (float("inf"), "infinite"), (float("-inf"), "infinite"), (0.5, "not an integer"),
       (2.0 ** 52 + 1, "LPG_BINARY_SUM_CAP"), (-(2.0 ** 60), "LPG_BINARY_SUM_CAP")]


@pytest.mark.parametrize("q,i,j", POSITIONS)
@pytest.mark.parametrize("value,word", BAD)
def test_load_refuses_a_bad_matrix_entry_and_names_it(lib, batch, value, word, q, i, j):
    from linearprogramming_amd import _lib
    A, sense, rhs, c = good()
    A[q, i, j] = value
    assert load(lib, batch, A, sense, rhs, c) == _lib.ERR_ARG
    msg = lib.lpg_binary_last_error(batch).decode()
    assert "lpg_binary_load" in msg and f"problem {q}, row {i}, entry {j}" in msg and word in msg, msg
    assert "nothing was loaded" in msg
    assert lib.lpg_binary_solve(batch, 0, None) == _lib.ERR_STATE          # indeed nothing
    if q == 1:                                           # the problem's index is the batch's, not the call's
        assert load(lib, batch, A[1:], sense[1:], rhs[1:], c[1:], first=1) == _lib.ERR_ARG
        assert f"problem 1, row {i}, entry {j}" in lib.lpg_binary_last_error(batch).decode()


@pytest.mark.parametrize("q,j", [(0, 0), (1, 2), (1, N - 1)])
@pytest.mark.parametrize("value,word", BAD)
def test_load_refuses_a_bad_cost_and_names_it(lib, batch, value, word, q, j):
    from linearprogramming_amd import _lib
    A, sense, rhs, c = good()
    c[q, j] = value
    assert load(lib, batch, A, sense, rhs, c) == _lib.ERR_ARG
    msg = lib.lpg_binary_last_error(batch).decode()
    assert "lpg_binary_load" in msg and f"problem {q}, cost {j}" in msg and word in msg, msg


@pytest.mark.parametrize("q,i", [(0, 0), (1, 1), (1, M - 1)])
@pytest.mark.parametrize("value,word", [(float("nan"), "NaN"), (float("inf"), "infinite"), (float("-inf"), "infinite"),
                                        (-1.5, "not an integer"), (2.0 ** 53 + 2, "LPG_BINARY_RHS_CAP"),
                                        (-(2.0 ** 53) - 2, "LPG_BINARY_RHS_CAP")])
def test_load_refuses_a_bad_right_hand_side_and_names_it(lib, batch, value, word, q, i):
    from linearprogramming_amd import _lib
    A, sense, rhs, c = good()
    rhs[q, i] = value
    assert load(lib, batch, A, sense, rhs, c) == _lib.ERR_ARG
    msg = lib.lpg_binary_last_error(batch).decode()
    assert f"problem {q}, row {i}: the right-hand side" in msg and word in msg, msg


@pytest.mark.parametrize("q,i", [(0, 0), (1, 1), (1, M - 1)])
@pytest.mark.parametrize("value", [-2, 2, 1 << 20])
def test_load_refuses_a_bad_sense_and_names_it(lib, batch, value, q, i):
    from linearprogramming_amd import _lib
    A, sense, rhs, c = good()
    sense[q, i] = value
    assert load(lib, batch, A, sense, rhs, c) == _lib.ERR_ARG
    msg = lib.lpg_binary_last_error(batch).decode()
    assert f"problem {q}, row {i}: sense {value} outside" in msg, msg


def test_the_caps_themselves_pass(lib, batch):
    """A row's sum of |a| and the sum of |c| at 2^52 and a right-hand side at 2^53 are accepted: the refusal names
    a later entry, one above its cap. (A load that passes every check goes on to the device, which this file
    never touches, so acceptance is shown by what the scan walks past.)"""
    from linearprogramming_amd import _lib
    A, sense, rhs, c = good()
    A[0, 0] = [2.0 ** 52 - 3, -1, 1, 1]                   # sum |a| = 2^52
    A[0, 1] = [-(2.0 ** 52), 0, 0, -0.0]
    rhs[0, 0], rhs[0, 1] = 2.0 ** 53, -(2.0 ** 53)
    c[0] = [-(2.0 ** 51), 2.0 ** 51, 0, 0]                # sum |c| = 2^52
    sense[0] = [-1, 0, 1]
    A[1, 2] = [2.0 ** 52 - 3, -1, 1, 2]                   # one above, reached at the last entry
    assert load(lib, batch, A, sense, rhs, c) == _lib.ERR_ARG
    msg = lib.lpg_binary_last_error(batch).decode()
    assert "problem 1, row 2, entry 3" in msg and "LPG_BINARY_SUM_CAP" in msg, msg
    A[1, 2] = 1
    c[1] = [2.0 ** 51, -(2.0 ** 51), 0, 1]                # one above
    assert load(lib, batch, A, sense, rhs, c) == _lib.ERR_ARG
    msg = lib.lpg_binary_last_error(batch).decode()
    assert "problem 1, cost 3" in msg and "LPG_BINARY_SUM_CAP" in msg, msg


def test_generate_refuses_an_unknown_kind(lib, batch):
    from linearprogramming_amd import _lib
    for kind in (-1, 1, 7):
        assert lib.lpg_binary_generate(batch, 1, kind) == _lib.ERR_ARG
        assert "kind" in lib.lpg_binary_last_error(batch).decode()


def test_solve_and_get_before_data(lib, batch):
    from linearprogramming_amd import _lib
    assert lib.lpg_binary_solve(batch, 0, None) == _lib.ERR_STATE
    assert "problem 0 has no data" in lib.lpg_binary_last_error(batch).decode()
    x = np.zeros(2 * N, dtype=np.int8)
    assert lib.lpg_binary_get(batch, 0, 2, x.ctypes.data_as(_lib.c_int8_p)) == _lib.ERR_STATE
    assert "no solve" in lib.lpg_binary_last_error(batch).decode()
    assert lib.lpg_binary_get(batch, 0, 2, None) == _lib.ERR_ARG
    assert "x is NULL" in lib.lpg_binary_last_error(batch).decode()
    assert lib.lpg_binary_get(batch, 1, 2, x.ctypes.data_as(_lib.c_int8_p)) == _lib.ERR_ARG
    assert "outside the batch" in lib.lpg_binary_last_error(batch).decode()


def test_every_source_list_names_the_binary_file():
    """As tests/test_assign_abi.py's check for lpg_assign.hip: the product objects and the two lab libraries are
    built from explicit lists."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    kobjs = re.search(r"^KOBJS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "$(OBJDIR)/lpg_binary.o" in kobjs
    for target in ("tools/probe/liblpg_phases.so", "tools/probe/liblpg_pub.so"):
        rule = re.search(r"^" + re.escape(target) + r":(.*)\n\t.*\n\t(.*)$", mk, flags=re.M)
        assert rule, target
        assert "$(CSRC)/lpg_binary.hip" in rule.group(1), target      # prerequisites
        assert "$(CSRC)/lpg_binary.hip" in rule.group(2), target      # the compile line


def test_every_prototype_of_the_header_is_bound(lib):
    from linearprogramming_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lpg.h")).read()
    declared = set(re.findall(r"\b(lpg_binary_[a-z_]+)\s*\(", hdr)) - {"lpg_binary_result"}
    bound = {name for name, _, _ in _lib.PROTOTYPES if name.startswith("lpg_binary_")}
    assert declared == bound and len(bound) == 9
    assert ctypes.sizeof(_lib.BinaryResult) == 24 and ctypes.sizeof(_lib.BinaryInfo) == 64
