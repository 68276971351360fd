"""Big-M batches without a device: lpg_batch_create_big_m and
lpg_batch_solve_big_m refuse bad arguments before any HIP call, and
frontend.engine_arrays (the tableau builder solve() and solve_batch() share),
loaded into a CPU oracle with two objective rows, solves the golden models
that need artificials to the recorded answers by Big-M.
"""
from __future__ import annotations

import ctypes
import os
from fractions import Fraction

import pytest

import batch3_cases as b3
from conftest import ROOT
from oracle.lpo import RULE_BLAND, RULE_DANTZIG
from test_batch_two_phase_abi import KNOWN_Z

from linearprogramming_amd import frontend as F

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


def test_null_batch_is_an_argument_error(lib):
    from linearprogramming_amd import _lib
    res = (_lib.Result * 1)()
    assert lib.lpg_batch_solve_big_m(None, 2, None, 0, 10, 0, res) == _lib.ERR_ARG
    assert b"NULL" in lib.lpg_batch_last_error(None)
    assert lib.lpg_batch_create_big_m(None, 0, 4, 4, 9, 0) == _lib.ERR_ARG
    assert b"NULL" in lib.lpg_batch_last_error(None)


@pytest.mark.parametrize("count,m,ncols,flags,word", [
    (0, 4, 9, 0, "count"),                 # count = 0
    (4, 0, 9, 0, "m"),                     # m = 0
    (4, 4, 1, 0, "ncols"),                 # ncols < 2
    (4, 4, 9, 0x4, "flags"),               # LPG_FLAG_BIG_M: the constructor says it, not a flag
    (4, 4, 9, 0x8, "flags"),               # LPG_FLAG_EAGER
    (4, 4, 9, 0x2, "flags"),               # LPG_FLAG_NO_SKIP
    (4, 4, 8193, 0, "lpg_create"),         # ncols > 8192: points to the single-LP engine
    (4, 8191, 9, 0, "lpg_create"),         # m + 2 > 8192 (a plain batch takes m = 8191)
    (1 << 20, 2046, 9, 0, "2^31"),         # count * (m + 2) = 2^31 (a plain batch: count * (m + 1) < 2^31)
])
def test_create_big_m_refuses_bad_arguments_with_a_message(lib, count, m, ncols, flags, word):
    from linearprogramming_amd import _lib
    b = ctypes.c_void_p(1)
    rc = lib.lpg_batch_create_big_m(ctypes.byref(b), 0, count, m, ncols, flags)
    assert rc == _lib.ERR_ARG
    assert not b.value                                   # *out cleared
    msg = lib.lpg_batch_last_error(None).decode()
    assert msg and word in msg and msg.startswith("lpg_batch_create_big_m:"), msg


def test_python_wrapper_names_the_constructor():
    import linearprogramming_amd as lpg
    with pytest.raises(lpg.LPGError, match="lpg_batch_create_big_m rc=-1.*bad shape"):
        lpg.BatchEngine(0, 4, 9, big_m=True)
    with pytest.raises(lpg.LPGError, match="lpg_batch_create rc=-1.*flags"):
        lpg.BatchEngine(4, 4, 9, flags=lpg._lib.FLAG_BIG_M)


def test_batch_info_ends_with_nobj():
    from linearprogramming_amd import _lib
    names = [f[0] for f in _lib.BatchInfo._fields_]
    assert names[-2:] == ["nobj", "pad"] and ctypes.sizeof(_lib.BatchInfo) == 64
    hdr = open(os.path.join(ROOT, "include", "lpg.h")).read()
    body = hdr[hdr.index("typedef struct {\n    int64_t count, m, ncols, ld;"):hdr.index("} lpg_batch_info_t;")]
    assert body.rstrip().endswith("int32_t pad;") and "int32_t nobj;" in body


def test_solve_batch_refuses_an_unknown_method_before_any_work():
    with pytest.raises(F.FrontendError, match="unknown method 'bigm'"):
        F.solve_batch([], method="bigm")
    with pytest.raises(TypeError):
        F.solve_batch([], None, 0, "big_m")                # method is keyword-only
    assert F.solve_batch([], method="big_m") == [] and F.solve_batch([], method="dual") == []


def _lacking_models():
    out = []
    for d in ("lp", "lp_extra"):
        for name in sorted(os.listdir(os.path.join(GOLDEN, d))):
            try:
                sm = F.build_smatrix(open(os.path.join(GOLDEN, d, name), "rb").read())
            except F.FrontendError:
                continue
            if F.engine_arrays(sm)[4]:
                out.append((name, sm))
    return out


@pytest.mark.parametrize("rule", [RULE_DANTZIG, RULE_BLAND])
def test_engine_arrays_solve_by_big_m_on_the_oracle(rule):
    models = _lacking_models()
    assert sorted(name for name, _ in models) == sorted(b3.LACKING_MODELS)
    for name, sm in models:
        r = b3.oracle_model_big_m(sm, rule)
        assert r.status == b3.LACKING_MODELS[name], (name, r)
        if name in KNOWN_Z:
            # a handful of pivots on small rationals: a few ulps of the objective (tests/test_batch_two_phase_abi.py)
            z = (Fraction(r.objective) + sm.constant) / sm.zcoef
            assert abs(z - KNOWN_Z[name]) <= Fraction(1, 10 ** 12) * max(1, abs(KNOWN_Z[name])), (name, float(z))
        else:
            assert name == "m_ray_infeasible.txt" and r.pivots == (1 if rule == RULE_DANTZIG else 0)
