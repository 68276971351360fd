"""The ranging definition and the device cases, on the CPU oracle (no GPU).

1. The definition of include/lpg.h's "ranging", as tests/ranging_cases.py
   states it in numpy, means what it says: on exact interval LPs (integral
   tableaus, so every ratio is exact) a cost or a right-hand side moved to an
   end of its range leaves the basis optimal (the oracle answers OPTIMAL with 0
   pivots), moved one beyond it does not, every interval contains 0 and the
   objective moves by dual[i] * delta.
2. The census: the device cases of tests/test_gpu_batch_ranging.py hold every
   class of decision k_batch_ranging makes at least FLOOR times, counted against
   the kernel's partition (ranging_cases.LANES, WAVES, BLOCK), so those tests
   are not vacuous.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ranging_cases as rc  # noqa: E402
from oracle.lpo import Oracle  # noqa: E402

FLOOR = 3
EPS = 1e-9


def _answer(T, basis, dual):
    o = Oracle(T.shape[0] - 1, T.shape[1])
    o.load_tableau(T, basis)
    r = o.solve_dual(rc.BUDGET) if dual else o.solve(rc.BUDGET)
    o.close()
    return r


def _stays(r):
    return r.status == rc.OPTIMAL and r.pivots == 0


def _cost_moved(T, basis, j, delta):
    """The solved tableau with the max-form cost of column j moved by delta, in the same basis."""
    m = T.shape[0] - 1
    C = T.copy()
    rows = np.flatnonzero(basis == j)
    if rows.size == 0:
        C[m, j] = T[m, j] - delta
    else:
        C[m] = T[m] + delta * T[rows[0]]
        C[m, j] = 0.0
    return C


def _rhs_moved(T, h, delta):
    """The solved tableau with the right-hand side whose unit column was h moved by delta."""
    C = T.copy()
    C[:, 0] = T[:, 0] + delta * T[:, h]
    return C


@pytest.mark.parametrize("m,n", [(12, 20), (40, 30)])
def test_the_ranges_are_the_ranges(m, n):
    inside = outside = 0
    for seed in (1, 2, 3, 4):
        T, basis, nact, ident, status = rc.solve_oracle(rc.lp("primal", m, n, seed))
        assert status == rc.OPTIMAL
        assert np.array_equal(T, np.round(T)), "the interval LPs are integral: every ratio is exact"
        R = rc.ranging_of(T, basis, nact, ident, EPS, status)
        z = T[m, 0]
        for lo, hi in ((R["cost_lo"], R["cost_hi"]), (R["rhs_lo"], R["rhs_hi"])):
            assert (lo <= 0).all() and (hi >= 0).all(), "every interval contains 0"
        for j in range(1, T.shape[1]):
            for end, step in ((R["cost_lo"][j - 1], -1.0), (R["cost_hi"][j - 1], 1.0)):
                if np.isfinite(end):
                    assert _stays(_answer(_cost_moved(T, basis, j, end), basis, False)), (seed, "cost", j, end)
                    assert not _stays(_answer(_cost_moved(T, basis, j, end + step), basis, False)), (seed, "cost", j, end)
                    inside, outside = inside + 1, outside + 1
        for i in range(m):
            for end, step in ((R["rhs_lo"][i], -1.0), (R["rhs_hi"][i], 1.0)):
                if np.isfinite(end):
                    r = _answer(_rhs_moved(T, ident[i], end), basis, True)
                    assert _stays(r), (seed, "rhs", i, end)
                    assert r.objective == z + R["dual"][i] * end, (seed, "rhs", i, end)
                    assert not _stays(_answer(_rhs_moved(T, ident[i], end + step), basis, True)), (seed, "rhs", i, end)
                    inside, outside = inside + 1, outside + 1
    print(f"({m}, {n}): {inside} inside and {outside} outside checks")
    assert inside >= 100 and outside == inside


def test_an_lp_that_is_not_optimal_is_not_ranged():
    T, basis, nact, ident, status = rc.solve_oracle(rc.lp("interval_art", 12, 20, 1))
    assert status == rc.INFEASIBLE
    R = rc.ranging_of(T, basis, nact, ident, EPS, status)
    for f in rc.FIELDS:
        if f.endswith("_at"):
            assert (R[f] == (0 if f.startswith("cost") else -1)).all()
        else:
            assert np.isnan(R[f]).all()


_CENSUS = {}


def census(name):
    """The classes of one device case, summed over its LPs (computed once)."""
    if name not in _CENSUS:
        tot = {"not_optimal": 0, "nact_below_N": 0}
        for c in rc.CASES[name]:
            T, basis, nact, ident, status = rc.solve_oracle(c)
            if status != rc.OPTIMAL:
                tot["not_optimal"] += 1
                continue
            tot["nact_below_N"] += int(nact < T.shape[1] - 1)
            for k, v in rc.ties_of(T, basis, nact, ident, EPS).items():
                tot[k] = tot.get(k, 0) + v
        _CENSUS[name] = tot
    return _CENSUS[name]


# the classes of ties k_batch_ranging resolves in different places, and the case that must hold each. The cost
# phase: in a lane's stride (equal lanes, so different 64-column groups) and in the wave's butterfly (different
# lanes). The right-hand-side phase walks serially, so its one class is "a tie at all"; at m > BLOCK a lane takes
# a second frame row, and the ties 64 rows apart are the ones a split over waves would have had to carry.
@pytest.mark.parametrize("name,cls", [
    ("interval-70x150", "cost_ties"), ("interval-70x150", "cost_ties_xlane"), ("interval-70x150", "cost_ties_inlane"),
    ("interval-70x150", "cost_ties_xgroup"), ("interval-40x300", "cost_ties_xgroup"), ("interval-40x300", "cost_ties_inlane"),
    ("interval-300x40", "rhs_ties"), ("interval-300x40", "rhs_ties_xgroup"), ("interval-300x40", "rhs_ties_xlane_row"),
    ("interval-70x150", "rhs_ties"), ("interval-12x20", "cost_ties_xlane")])
def test_census_ties(name, cls):
    got = census(name)
    print(name, got)
    assert got[cls] >= FLOOR, (name, cls, got)


def test_census_other_classes():
    """Over all device cases: bounds without a candidate on either side, degenerate rows, LPs that are not
    OPTIMAL, LPs with nact < N."""
    tot = {}
    for name in rc.CASES:
        for k, v in census(name).items():
            tot[k] = tot.get(k, 0) + v
    print(tot)
    for cls in ("no_candidate", "degenerate_rows", "not_optimal", "nact_below_N"):
        assert tot[cls] >= FLOOR, (cls, tot)
    assert census("interval_art-12x20")["not_optimal"] == 3      # INFEASIBLE, OPTIMAL, INFEASIBLE, INFEASIBLE
    assert census("artificial-8x8")["nact_below_N"] == 4 and census("artificial-33x33")["nact_below_N"] == 4


def test_the_ragged_case_mixes_kinds_and_statuses():
    sts = [rc.solve_oracle(c)[4] for c in rc.RAGGED]
    assert len(rc.RAGGED) == 6 and sts.count(rc.OPTIMAL) >= 4 and rc.INFEASIBLE in sts
    assert len({(c["m"], c["n"]) for c in rc.RAGGED}) == 6
