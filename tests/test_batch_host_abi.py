"""The host scaffold the batch families share (csrc/lpg_host.h), seen through
the C ABI without a GPU: every family keeps an error buffer of its own for the
calls that have no handle, and a handle whose device side cannot be made
answers with a device error every time, stays unloaded and is destroyed
cleanly (a setup that fails is taken down, and the next call starts it
afresh)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


def dp(x):
    from linearprogramming_amd import _lib
    return x.ctypes.data_as(_lib.c_double_p)


# per family: create(lib, handle, count) of the tiny shape, load(lib, handle, first, n) of valid data, solve, and
# the words of the "not loaded" refusal
def _assign_create(lib, h, count):
    return lib.lpg_assign_create(ctypes.byref(h), 0, count, 2, 3, 0)


def _assign_load(lib, h, first, n):
    c = np.arange(6.0 * n).reshape(n, 2, 3)
    return lib.lpg_assign_load(h, first, n, dp(c), 3)


def _transport_create(lib, h, count):
    return lib.lpg_transport_create(ctypes.byref(h), 0, count, 2, 3, 0)


def _transport_load(lib, h, first, n):
    c = np.arange(6.0 * n).reshape(n, 2, 3)
    s, d = np.tile([4.0, 5.0], (n, 1)), np.tile([3.0, 3.0, 3.0], (n, 1))
    return lib.lpg_transport_load(h, first, n, dp(c), 3, dp(s), dp(d))


def _binary_create(lib, h, count):
    return lib.lpg_binary_create(ctypes.byref(h), 0, count, 1, 2, 0, 0)


def _binary_load(lib, h, first, n):
    from linearprogramming_amd import _lib
    A, rhs, c = np.ones((n, 1, 2)), np.ones((n, 1)), np.ones((n, 2))
    sense = np.full((n, 1), -1, dtype=np.int32)
    return lib.lpg_binary_load(h, first, n, dp(A), 2, sense.ctypes.data_as(_lib.c_int32_p), dp(rhs), dp(c))


FAMILIES = {
    "assign": dict(count=2, create=_assign_create, load=_assign_load, solve=lambda lib, h: lib.lpg_assign_solve(h, None),
                   missing="has no costs yet"),
    "transport": dict(count=2, create=_transport_create, load=_transport_load,
                      solve=lambda lib, h: lib.lpg_transport_solve(h, 100, 0, None), missing="has no data yet"),
    "binary": dict(count=1, create=_binary_create, load=_binary_load, solve=lambda lib, h: lib.lpg_binary_solve(h, 0, None),
                   missing="has no data yet"),
}


def last_error(lib, family, h=None):
    return getattr(lib, f"lpg_{family}_last_error")(h).decode()


def test_every_family_has_its_own_buffer_for_calls_without_a_handle(lib):
    from linearprogramming_amd import _lib
    h = ctypes.c_void_p()
    assert lib.lpg_assign_create(ctypes.byref(h), 0, 0, 2, 3, 0) == _lib.ERR_ARG
    assign = last_error(lib, "assign")
    assert assign.startswith("lpg_assign_create: bad shape count=0"), assign
    assert lib.lpg_transport_create(ctypes.byref(h), 0, 0, 2, 3, 0) == _lib.ERR_ARG
    assert lib.lpg_binary_create(ctypes.byref(h), 0, 0, 1, 2, 0, 0) == _lib.ERR_ARG
    assert lib.lpg_batch_create(ctypes.byref(h), 0, 0, 2, 4, 0) == _lib.ERR_ARG
    assert last_error(lib, "assign") == assign
    for family in ("transport", "binary", "batch"):
        msg = last_error(lib, family)
        assert msg.startswith(f"lpg_{family}_create: bad shape count=0"), (family, msg)
    # and the other way round: a later refusal of assign's leaves the other three alone
    before = {f: last_error(lib, f) for f in ("transport", "binary", "batch")}
    assert lib.lpg_assign_create(ctypes.byref(h), 0, 1, 3, 2, 0) == _lib.ERR_ARG
    assert "nr=3" in last_error(lib, "assign")
    assert {f: last_error(lib, f) for f in before} == before


def test_a_refusal_with_a_handle_reaches_the_handle_and_the_family_buffer(lib):
    from linearprogramming_amd import _lib
    for family, f in FAMILIES.items():
        h = ctypes.c_void_p()
        assert f["create"](lib, h, f["count"]) == 0
        assert f["load"](lib, h, f["count"], 1) == _lib.ERR_ARG          # one past the batch
        msg = last_error(lib, family, h)
        want = f"lpg_{family}_load: problems [{f['count']}, {f['count'] + 1}) outside the batch of {f['count']} (need n >= 1)"
        assert msg == want, msg
        assert last_error(lib, family) == msg
        getattr(lib, f"lpg_{family}_destroy")(h)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_without_a_device_every_call_that_needs_one_says_so_and_nothing_is_loaded(lib, family):
    import linearprogramming_amd as lpg
    from linearprogramming_amd import _lib
    if lpg.device_count() > 0:
        pytest.skip("needs a machine without a GPU")
    f = FAMILIES[family]
    h = ctypes.c_void_p()
    assert f["create"](lib, h, f["count"]) == 0
    for _ in range(2):                                                   # the second call starts the setup afresh
        assert f["load"](lib, h, 0, f["count"]) == _lib.ERR_DEVICE
        msg = last_error(lib, family, h)
        assert msg.startswith(f"lpg_{family}_load: ") and "hipSetDevice(0)" in msg, msg
    assert f["load"](lib, h, f["count"] - 1, 1) == _lib.ERR_DEVICE          # the last problem alone: refused as well
    assert f["solve"](lib, h) == _lib.ERR_STATE
    msg = last_error(lib, family, h)
    assert msg.startswith(f"lpg_{family}_solve: problem 0 {f['missing']}"), msg
    getattr(lib, f"lpg_{family}_destroy")(h)
