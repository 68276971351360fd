"""Ranging without a device: the symbol, the prototype, the header line and the
methods are declared, and the refusals that do not depend on the batch (`out`,
`ident`, `b` NULL, in that order) are answered before any HIP call, naming the
call and the argument. The refusals that read the batch (the group rule, a
Big-M batch, an ident entry out of range) need a batch, which needs a device:
tests/test_gpu_batch_ranging.py has them."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


def test_symbol_prototype_header_and_methods(lib):
    import dataclasses

    import linearprogramming_amd as lpg
    from linearprogramming_amd import _lib, frontend
    protos = {name: (res, args) for name, res, args in _lib.PROTOTYPES}
    assert protos["lpg_batch_ranging"] == (ctypes.c_int, [ctypes.c_void_p, _lib.c_int64_p, ctypes.POINTER(_lib.RangingOut)])
    assert lib.lpg_batch_ranging
    header = open(_lib.os.path.join(_lib._SRC_ROOT, "include", "lpg.h")).read()
    assert "int  lpg_batch_ranging(lpg_batch *b, const int64_t *ident, const lpg_ranging_t *out);" in header
    assert "} lpg_ranging_t;" in header
    fields = ["dual", "cost_lo", "cost_hi", "cost_lo_at", "cost_hi_at", "rhs_lo", "rhs_hi", "rhs_lo_at", "rhs_hi_at"]
    assert [f for f, _ in _lib.RangingOut._fields_] == fields           # the struct's order is the header's
    assert ctypes.sizeof(_lib.RangingOut) == 9 * ctypes.sizeof(ctypes.c_void_p)
    assert [f.name for f in dataclasses.fields(lpg.Ranging)] == fields
    assert all(getattr(lpg.Ranging(), f) is None for f in fields)
    assert callable(lpg.BatchEngine.ranging) and callable(lpg.RaggedBatchEngine.ranging)
    assert callable(frontend.sensitivity_batch) and issubclass(frontend.LPSensitivity, frontend.LPSolution)


def _call(lib, b, ident, out):
    from linearprogramming_amd import _lib
    ip = None if ident is None else np.ascontiguousarray(ident, dtype=np.int64).ctypes.data_as(_lib.c_int64_p)
    rc = lib.lpg_batch_ranging(b, ip, None if out is None else ctypes.byref(out))
    return rc, lib.lpg_batch_last_error(None).decode()


@pytest.mark.parametrize("ident,out,words", [
    (None, False, "out is NULL"),                  # out before ident before the batch
    ([1], False, "out is NULL"),
    (None, True, "ident is NULL"),
    ([1], True, "batch is NULL"),
    ([0], True, "batch is NULL"),                  # what needs a batch is not looked at without one
])
def test_refusals_that_need_no_batch_come_first_and_name_the_argument(lib, ident, out, words):
    from linearprogramming_amd import _lib
    rc, msg = _call(lib, None, ident, _lib.RangingOut() if out else None)
    assert rc == _lib.ERR_ARG
    assert msg.startswith("lpg_batch_ranging:") and words in msg, msg
