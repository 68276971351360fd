"""The two-phase batch without a device: the new entry points refuse a NULL
handle before any HIP call, and frontend.engine_arrays (the tableau builder
solve() and solve_batch() share) hands the engine arrays that the CPU oracle
solves to the recorded answers.
"""
from __future__ import annotations

import ctypes
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from oracle.lpo import Oracle

from linearprogramming_amd import frontend as F

GOLDEN = os.path.join(ROOT, "tests", "golden")
STATUS = {1: "OPTIMAL", 2: "UNBOUNDED", 3: "INFEASIBLE", 4: "ITER_LIMIT", 5: "NUMERIC"}
# the optima of the models that need artificials (no transcript of the reference's own solve
# exists for them: kat_cases.json records "canonical": false), as tests/test_frontend.py's KNOWN
KNOWN_Z = {"a3_min_eq_neg.txt": Fraction(31, 3), "a5_lack_row.txt": Fraction(6), "a7_identity_quirk.txt": Fraction(2)}


def _models():
    out = []
    for d in ("lp", "lp_extra"):
        for name in sorted(os.listdir(os.path.join(GOLDEN, d))):
            try:
                out.append((name, F.build_smatrix(open(os.path.join(GOLDEN, d, name), "rb").read())))
            except F.FrontendError:
                pass
    return out


def test_null_batch_is_an_argument_error():
    import linearprogramming_amd as lpg
    lib = lpg.load()
    res = (lpg._lib.Result * 1)()
    af = ctypes.c_int64(-7)
    assert lib.lpg_batch_solve_two_phase(None, 2, None, 0, 10, 0, res) == -1
    assert b"NULL" in lib.lpg_batch_last_error(None)
    assert lib.lpg_batch_generate_artificial(None, 4, 1, ctypes.byref(af)) == -1
    assert af.value == -7
    assert lib.lpg_batch_set_objective(None, None, 0) == -1


def test_engine_arrays_layout():
    for name, sm in _models():
        rows, basis, cost, nc0, nlack = F.engine_arrays(sm)
        m = len(sm.rows)
        assert nc0 == len(sm.names) + 1 and rows.shape == (m, nc0 + nlack) and cost.shape == (nc0 + nlack,), name
        assert np.array_equal(rows[:, :nc0], np.array([[float(x) for x in r] for r in sm.rows])), name
        # every basic column is a true unit column; the artificials are nc0.. in row order
        for i in range(m):
            col = rows[:, basis[i]]
            assert col[i] == 1.0 and np.count_nonzero(col) == 1, (name, i)
        arts = [int(b) for b in basis if b >= nc0]
        assert arts == list(range(nc0, nc0 + nlack)), name
        assert np.array_equal(cost[:nc0 - 1], [float(c) for c in sm.costs]) and not cost[nc0 - 1:].any(), name


def test_engine_arrays_solve_to_the_recorded_answers_on_the_oracle():
    recorded = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "kat_cases.json")))}
    seen = set()
    for name, sm in _models():
        rows, basis, cost, nc0, nlack = F.engine_arrays(sm)
        m, nc = rows.shape
        o = Oracle(m, nc)
        T = np.zeros((m + 1, nc))
        T[:m] = rows
        o.load_tableau(T, basis)
        if nlack:
            r = o.solve_two_phase(nc0, cost[:nc - 1].copy(), 10_000)
        else:
            o.set_objective(cost[:nc - 1].copy())
            r = o.solve(10_000)
        o.close()
        seen.add(STATUS[r.status])
        case = recorded.get(name)
        if case and "dantzig" in case:
            assert nlack == 0 and STATUS[r.status] == case["dantzig"]["status"], (name, r)
            if r.status == 1:
                # a handful of pivots on small rationals: a few ulps of the objective
                assert abs(r.objective - case["dantzig"]["objective_f64"]) <= 1e-12 * max(1.0, abs(r.objective)), name
        if name in KNOWN_Z:
            assert nlack > 0 and r.status == 1, (name, r)
            z = (Fraction(r.objective) + sm.constant) / sm.zcoef
            assert abs(z - KNOWN_Z[name]) <= Fraction(1, 10 ** 12) * max(1, abs(KNOWN_Z[name])), (name, float(z))
    assert {"OPTIMAL", "UNBOUNDED", "INFEASIBLE"} <= seen


def test_batch_groups_keep_input_order():
    models = _models()
    sms = [sm for _, sm in models] * 2                 # every model twice: 2nd copies join the 1st ones' groups
    groups = F.batch_groups(sms)
    firsts = [v[0] for v in groups.values()]
    assert firsts == sorted(firsts)                    # keys in order of first appearance
    assert all(v == sorted(v) for v in groups.values())
    assert sorted(i for v in groups.values() for i in v) == list(range(len(sms)))
    n = len(models)
    for (m, nc0, nlack), v in groups.items():
        assert all(i + n in v for i in v if i < n)
        for i in v:
            rows, _, _, c0, nl = F.engine_arrays(sms[i])
            assert (rows.shape[0], c0, nl) == (m, nc0, nlack)
