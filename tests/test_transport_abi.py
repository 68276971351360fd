"""lpg_transport's host-side validation and build wiring (no GPU: every check
here is answered before the library touches a device; a batch's device side is
made by the first call that passes its checks)."""
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
    t = ctypes.c_void_p()
    assert lib.lpg_transport_create(ctypes.byref(t), 0, 2, 2, 3, 0) == 0
    yield t
    lib.lpg_transport_destroy(t)


def dp(x):
    from linearprogramming_amd import _lib
    return x.ctypes.data_as(_lib.c_double_p)


def good():
    """Costs, supplies and demands of two balanced 2 x 3 problems."""
    c = np.arange(12, dtype=np.float64).reshape(2, 2, 3)
    s = np.array([[4.0, 5.0], [0.0, 6.0]])
    d = np.array([[3.0, 3.0, 3.0], [6.0, 0.0, 0.0]])
    return c, s, d


def load(lib, batch, c, s, d, first=0, n=2):
    return lib.lpg_transport_load(batch, first, n, dp(c), 3, dp(s), dp(d))


@pytest.mark.parametrize("count,nr,nc,flags,word", [
    (0, 2, 2, 0, "count"),
    (2, 0, 2, 0, "nr"),
    (2, 2, 0, 0, "nc"),
    (2, 2, 4095, 0, "LPG_TRANSPORT_MAX_NODES"),     # nr + nc = 4097
    (2, 4097, 1, 0, "LPG_TRANSPORT_MAX_NODES"),
    (2, 2, 2, 0x4, "flags"),
    (2, 2, 2, 0x80000000, "flags"),
    (1 << 30, 2, 2, 0, "2^31"),
])
def test_create_refuses_bad_arguments_with_a_message(lib, count, nr, nc, flags, word):
    from linearprogramming_amd import _lib
    t = ctypes.c_void_p(1)
    assert lib.lpg_transport_create(ctypes.byref(t), 0, count, nr, nc, flags) == _lib.ERR_ARG
    assert not t.value                                   # *out cleared
    msg = lib.lpg_transport_last_error(None).decode()
    assert "lpg_transport_create" in msg and word in msg, msg


def test_create_accepts_the_node_cap_and_more_rows_than_columns(lib):
    from linearprogramming_amd import _lib
    for nr, nc, flags in ((2, 4094, 0), (4095, 1, 0x2), (1, 1, 0x3)):
        t = ctypes.c_void_p()
        assert lib.lpg_transport_create(ctypes.byref(t), 0, 1, nr, nc, flags) == 0
        i = _lib.TransportInfo()
        assert lib.lpg_transport_info(t, ctypes.byref(i)) == 0
        assert (i.count, i.nr, i.nc, i.start) == (1, nr, nc, flags & 0x2)
        lib.lpg_transport_destroy(t)


def test_python_wrapper_raises_with_the_message():
    import linearprogramming_amd as lpg
    with pytest.raises(lpg.LPGError, match="rc=-1.*bad shape"):
        lpg.TransportBatch(4, 0, 4)
    with pytest.raises(lpg.LPGError, match="start"):
        lpg.TransportBatch(4, 2, 4, start="vogel")


def test_null_handles_and_out_pointers_are_errors_not_crashes(lib, batch):
    from linearprogramming_amd import _lib
    c, s, d = good()
    lib.lpg_transport_destroy(None)
    assert lib.lpg_transport_create(None, 0, 1, 1, 1, 0) == _lib.ERR_ARG
    assert lib.lpg_transport_load(None, 0, 1, dp(c), 3, dp(s), dp(d)) == _lib.ERR_ARG
    assert lib.lpg_transport_generate(None, 1, 10, 5) == _lib.ERR_ARG
    assert lib.lpg_transport_solve(None, 10, 0, None) == _lib.ERR_ARG
    assert lib.lpg_transport_get(None, 0, 1, None, None, None, None) == _lib.ERR_ARG
    assert lib.lpg_transport_info(None, None) == _lib.ERR_ARG
    assert "NULL" in lib.lpg_transport_last_error(None).decode()
    assert lib.lpg_transport_info(batch, None) == _lib.ERR_ARG
    assert "out is NULL" in lib.lpg_transport_last_error(batch).decode()
    for k, word in enumerate(("costs", "supply", "demand")):
        args = [dp(c), 3, dp(s), dp(d)]
        args[(0, 2, 3)[k]] = None
        assert lib.lpg_transport_load(batch, 0, 2, *args) == _lib.ERR_ARG
        assert f"{word} is NULL" in lib.lpg_transport_last_error(batch).decode()


def test_info_reports_shape_form_and_chunk(lib, batch):
    from linearprogramming_amd import _lib
    i = _lib.TransportInfo()
    assert lib.lpg_transport_info(batch, ctypes.byref(i)) == 0
    assert (i.count, i.nr, i.nc) == (2, 2, 3)
    assert i.form == _lib.TRANSPORT_FORM_WAVE and i.tier == _lib.BATCH_TIER_LDS
    assert i.start == _lib.TRANSPORT_START_LEAST_COST and i.chunk >= 1 and i.launches == 0
    assert i.lds_bytes == 4 * (32 * 5 + 8 * 6)


@pytest.mark.parametrize("nr,nc,form,tier,lds", [
    (32, 32, 0, 0, 4 * (32 * 64 + 8 * 1024)),            # the last shape of the wave form
    (32, 33, 1, 0, 32 * 65 + 8 * 32 * 33),
    (134, 134, 1, 0, 32 * 268 + 8 * 134 * 134),          # the last square whose C fits beside the node state
    (135, 135, 1, 1, 32 * 270),
    (2, 4094, 1, 1, 32 * 4096),
])
def test_forms_and_tiers_by_shape(lib, nr, nc, form, tier, lds):
    from linearprogramming_amd import _lib
    t = ctypes.c_void_p()
    assert lib.lpg_transport_create(ctypes.byref(t), 0, 1, nr, nc, 0) == 0
    i = _lib.TransportInfo()
    assert lib.lpg_transport_info(t, ctypes.byref(i)) == 0
    lib.lpg_transport_destroy(t)
    assert (i.form, i.tier, i.lds_bytes) == (form, tier, lds)
    assert i.lds_bytes <= 150 * 1024


def test_load_refuses_a_bad_range_and_pitch(lib, batch):
    from linearprogramming_amd import _lib
    c, s, d = good()
    assert lib.lpg_transport_load(batch, 0, 2, dp(c), 2, dp(s), dp(d)) == _lib.ERR_ARG
    assert "ld 2 < nc = 3" in lib.lpg_transport_last_error(batch).decode()
    for first, n in ((-1, 1), (0, 0), (1, 2), (3, 1)):
        assert load(lib, batch, c, s, d, first, n) == _lib.ERR_ARG, (first, n)
        assert "outside the batch" in lib.lpg_transport_last_error(batch).decode()


@pytest.mark.parametrize("value,word", [(float("nan"), "NaN"), (float("inf"), "infinite"), (float("-inf"), "infinite"),
                                        (2.5, "not an integer"), (2.0 ** 40 + 1, "cap"), (-(2.0 ** 40) - 1, "cap")])
def test_load_refuses_a_bad_cost_and_names_it(lib, batch, value, word):
    from linearprogramming_amd import _lib
    c, s, d = good()
    c[0, 1, 0] = -5.0                         # negative costs are fine
    c[1, 1, 2] = value
    assert load(lib, batch, c, s, d) == _lib.ERR_ARG
    msg = lib.lpg_transport_last_error(batch).decode()
    assert "lpg_transport_load" in msg and "problem 1, cost (1, 2)" in msg and word in msg, msg
    # the problem's index is the batch's, not the call's
    assert load(lib, batch, c[1:], s[1:], d[1:], 1, 1) == _lib.ERR_ARG
    assert "problem 1, cost (1, 2)" in lib.lpg_transport_last_error(batch).decode()


@pytest.mark.parametrize("value,word", [(float("nan"), "NaN"), (float("inf"), "infinite"), (-1.0, "negative"),
                                        (0.5, "not an integer"), (2.0 ** 54, "2^53")])
@pytest.mark.parametrize("side", ["supply", "demand"])
def test_load_refuses_a_bad_amount_and_names_it(lib, batch, side, value, word):
    from linearprogramming_amd import _lib
    c, s, d = good()
    (s if side == "supply" else d)[1, 1] = value
    assert load(lib, batch, c, s, d) == _lib.ERR_ARG
    msg = lib.lpg_transport_last_error(batch).decode()
    assert f"problem 1, {side} 1 is" in msg and word in msg, msg


def test_load_refuses_an_unbalanced_problem_and_gives_both_sums(lib, batch):
    from linearprogramming_amd import _lib
    c, s, d = good()
    d[1, 2] = 1.0
    assert load(lib, batch, c, s, d) == _lib.ERR_ARG
    msg = lib.lpg_transport_last_error(batch).decode()
    assert "problem 1 is not balanced" in msg and "sum to 6," in msg and "to 7" in msg, msg


def test_load_refuses_sums_and_products_past_2_53(lib, batch):
    from linearprogramming_amd import _lib
    c, s, d = good()
    c[:] = 0.0
    s[0], d[0] = [2.0 ** 52, 2.0 ** 52 + 2], [2.0 ** 53, 1.0, 1.0]
    assert load(lib, batch, c, s, d) == _lib.ERR_ARG
    msg = lib.lpg_transport_last_error(batch).decode()
    assert "problem 0" in msg and "supplies sum to 9007199254740994, above 2^53" in msg, msg
    # the sum itself at 2^53 passes the sum check; a cost of 2 then carries the product past 2^53: integer arithmetic
    s[0], d[0] = [2.0 ** 52, 2.0 ** 52], [2.0 ** 53, 0.0, 0.0]
    c[0, 1, 1] = -2.0
    assert load(lib, batch, c, s, d) == _lib.ERR_ARG
    msg = lib.lpg_transport_last_error(batch).decode()
    assert "problem 0" in msg and "max |c| x sum of supplies = 2 x 9007199254740992 exceeds 2^53" in msg, msg
    # 2^40 x 2^13 is exactly 2^53 and passes every check (then the load wants a device, which is not this test's)
    s[0], d[0] = [2.0 ** 12, 2.0 ** 12], [2.0 ** 13, 0.0, 0.0]
    c[0, 1, 1] = -(2.0 ** 40)
    s[1, 1] = -1.0                            # the next problem stops the call before any device work
    assert load(lib, batch, c, s, d) == _lib.ERR_ARG
    assert "problem 1, supply 1 is negative" in lib.lpg_transport_last_error(batch).decode()


def test_generate_refuses_bad_ranges(lib, batch):
    from linearprogramming_amd import _lib
    for r, q, word in ((0, 5, "range"), ((1 << 40) + 2, 5, "range"), (10, 0, "qmax"), (10, -3, "qmax"),
                       (1 << 40, 1 << 13, "2^53"), (2, (1 << 53), "2^53")):
        assert lib.lpg_transport_generate(batch, 1, r, q) == _lib.ERR_ARG, (r, q)
        assert word in lib.lpg_transport_last_error(batch).decode()


def test_solve_and_get_refusals(lib, batch):
    from linearprogramming_amd import _lib
    for it in (0, -1):
        assert lib.lpg_transport_solve(batch, it, 0, None) == _lib.ERR_ARG
        assert "max_iters" in lib.lpg_transport_last_error(batch).decode()
    assert lib.lpg_transport_solve(batch, 10, 2, None) == _lib.ERR_ARG
    assert "rule 2" in lib.lpg_transport_last_error(batch).decode()
    assert lib.lpg_transport_solve(batch, 10, 0, None) == _lib.ERR_STATE
    assert "problem 0 has no data" in lib.lpg_transport_last_error(batch).decode()
    x = np.zeros(12)
    assert lib.lpg_transport_get(batch, 0, 2, dp(x), None, None, None) == _lib.ERR_STATE
    assert lib.lpg_transport_get(batch, 0, 2, None, None, None, None) == _lib.ERR_ARG
    assert "all NULL" in lib.lpg_transport_last_error(batch).decode()
    assert lib.lpg_transport_get(batch, 1, 2, dp(x), None, None, None) == _lib.ERR_ARG
    assert "outside the batch" in lib.lpg_transport_last_error(batch).decode()


def test_a_bad_chunk_in_the_environment_is_refused(lib, monkeypatch):
    from linearprogramming_amd import _lib
    for bad in ("0", "-4", "seven", "7x"):
        monkeypatch.setenv("LPG_TRANSPORT_CHUNK", bad)
        t = ctypes.c_void_p(1)
        assert lib.lpg_transport_create(ctypes.byref(t), 0, 1, 2, 2, 0) == _lib.ERR_ARG and not t.value
        assert "LPG_TRANSPORT_CHUNK" in lib.lpg_transport_last_error(None).decode()
    monkeypatch.setenv("LPG_TRANSPORT_CHUNK", "7")
    t = ctypes.c_void_p()
    assert lib.lpg_transport_create(ctypes.byref(t), 0, 1, 2, 2, 0) == 0
    i = _lib.TransportInfo()
    lib.lpg_transport_info(t, ctypes.byref(i))
    lib.lpg_transport_destroy(t)
    assert i.chunk == 7


def test_the_front_end_refuses_bad_models_before_any_device_work():
    from linearprogramming_amd import frontend
    with pytest.raises(frontend.FrontendError, match="model 0 has shapes"):
        frontend.solve_transportation([([[1, 2]], [1, 2], [3])])
    with pytest.raises(frontend.FrontendError, match="negative or not finite"):
        frontend.solve_transportation([([[1, 2]], [-1], [3, 4])])
    with pytest.raises(frontend.FrontendError, match="wrong sign"):
        frontend.solve_transportation([([[1, float("-inf")]], [3], [1, 2])])
    with pytest.raises(frontend.FrontendError, match="outside the caps"):
        frontend.solve_transportation([([[2.0 ** 30, float("inf")], [0, 1]], [2.0 ** 20, 1], [1, 2.0 ** 20])])


def test_every_source_list_names_the_transportation_file():
    """As tests/test_assign_abi.py's check: the product objects and the two lab libraries are built from explicit lists."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    kobjs = re.search(r"^KOBJS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "$(OBJDIR)/lpg_transport.o" in kobjs
    for target in ("tools/probe/liblpg_phases.so", "tools/probe/liblpg_pub.so"):
        rule = re.search(r"^" + re.escape(target) + r":(.*)\n\t.*\n\t(.*)$", mk, flags=re.M)
        assert rule, target
        assert "$(CSRC)/lpg_transport.hip" in rule.group(1), target      # prerequisites
        assert "$(CSRC)/lpg_transport.hip" in rule.group(2), target      # the compile line
