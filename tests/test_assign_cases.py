"""The definition of the assignment problem (include/lpg.h "assignment", restated
in tests/assign_cases.py) against brute force, scipy and its own certificate,
and a census of the cases tests/test_gpu_assign.py runs. No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import assign_cases as ac

# kind -> cases per sense; 30% of +inf rarely leaves a small problem infeasible, so that kind gets more
INT_KINDS = {"int3": 20, "int49": 20, "inf30": 60, "rows": 20, "const": 20, "blocked": 5}


def small_cases():
    """(kind, maximize, C) for every integer kind and sense, nr 1..6, nc up to nr + 2."""
    rng = np.random.default_rng(20220518)
    out = []
    for kind, n in INT_KINDS.items():
        for mx in (False, True):
            for _ in range(n):
                nr = int(rng.integers(1, 7))
                nc = nr + int(rng.integers(0, 3))
                out.append((kind, mx, ac.problem(kind, nr, nc, rng)))
    return out


CASES = small_cases()


def test_the_restatement_finds_the_brute_force_optimum():
    multi = infeasible = 0
    for kind, mx, C in CASES:
        r = ac.hungarian(C, mx)
        best, n = ac.brute_force(C, mx)
        if best is None:
            assert r["status"] == ac.INFEASIBLE, (kind, mx, C)
            assert np.isnan(r["objective"]) and (r["col"] == -1).all()
            infeasible += 1
            continue
        assert r["status"] == ac.OPTIMAL, (kind, mx, C)
        assert r["objective"] == best, (kind, mx, C, r["objective"], best)
        assert sorted(set(r["col"].tolist())) == sorted(r["col"].tolist())        # an injection
        assert C[np.arange(C.shape[0]), r["col"]].sum() == best
        multi += n > 1
    # the committed seed gives 109 cases with more than one optimal assignment and 13 infeasible ones of 290;
    # the floors are half of that
    assert multi >= 54 and infeasible >= 6, (multi, infeasible)


def test_the_restatement_agrees_with_scipy():
    opt = pytest.importorskip("scipy.optimize")
    checked = 0
    for kind, mx, C in CASES:
        r = ac.hungarian(C, mx)
        if r["status"] != ac.OPTIMAL:
            with pytest.raises(ValueError):
                opt.linear_sum_assignment(C, maximize=mx)
            continue
        # scipy refuses +inf in a maximisation's matrix after negating it; state that sense as a minimisation
        D = ac.sensed(C, mx)
        rows, cols = opt.linear_sum_assignment(D)
        assert D[rows, cols].sum() == (-r["objective"] if mx else r["objective"]), (kind, mx, C)
        checked += 1
    assert checked >= 150


def test_the_certificate_holds_exactly_on_integer_costs():
    for kind, mx, C in CASES:
        r = ac.hungarian(C, mx)
        nr, nc = C.shape
        assert 1 <= r["steps"] <= nr * (nr + 1) // 2
        # in the sense the algorithm ran in: a maximisation's u, v and costs negated back
        D = ac.sensed(C, mx)
        u, v = (-r["u"], -r["v"]) if mx else (r["u"], r["v"])
        if r["status"] != ac.OPTIMAL:
            continue
        fin = np.isfinite(D)
        assert ((u[:, None] + v[None, :])[fin] <= D[fin]).all(), (kind, mx, C)
        assert (u + v[r["col"]] == D[np.arange(nr), r["col"]]).all(), (kind, mx, C)
        assert (v <= 0).all()
        free = np.setdiff1d(np.arange(nc), r["col"])
        assert (v[free] == 0).all()


def test_the_gpu_cases_hold_the_ties_they_claim():
    """A census of the batches tests/test_gpu_assign.py compares bit for bit (up to 70 columns: the larger ones
    take the restatement seconds each and add only more of the same). The floors are half of what the committed
    seeds give, written beside each."""
    multi = infeasible = tie_steps = neg_steps = negzero_steps = 0
    for s in ac.SMALL + ac.MIXED + ac.WAVE_LINE + ac.FORCED_GLOBAL:
        for kind, C in zip(s["kinds"], ac.costs_of(s)):
            trace = []
            r = ac.hungarian(C, s["maximize"], trace=trace)
            infeasible += r["status"] == ac.INFEASIBLE
            tie_steps += sum(1 for n, _ in trace if n >= 2)
            negzero_steps += sum(1 for _, d in trace if d == 0 and np.signbit(d))
            if kind == "frac" and not s["maximize"]:
                # a minimisation's reduced costs are non-negative in exact arithmetic: these are roundings
                neg_steps += sum(1 for _, d in trace if d < 0)
            if s["shape"][0] <= 6 and kind != "frac":
                multi += ac.brute_force(C, s["maximize"])[1] > 1
    assert multi >= 10, multi                    # 20 problems with more than one optimal assignment
    assert infeasible >= 3, infeasible           # 3: the two blocked 6 x 6 and a 2 x 2 with 30% +inf (all of them)
    assert tie_steps >= 39000, tie_steps         # 79155 steps with two or more columns at the minimum
    assert neg_steps >= 10, neg_steps            # 20 steps of minimised k/10 problems with delta < 0
    assert negzero_steps >= 33, negzero_steps    # 67 steps with delta == -0


def test_transposed_and_rectangular_orientation():
    """nr < nc leaves columns free, and every free column keeps v == 0."""
    rng = np.random.default_rng(7)
    C = ac.problem("int49", 3, 7, rng)
    r = ac.hungarian(C)
    assert r["status"] == ac.OPTIMAL and len(set(r["col"].tolist())) == 3
    assert r["objective"] == ac.brute_force(C)[0]
