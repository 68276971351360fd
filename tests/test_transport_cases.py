"""The numpy statement of the transportation method (tests/transport_cases.py)
held to HiGHS, to its own certificate, to the assignment statement and to its
budget rule, and a census of what the device cases hold (no GPU)."""
from __future__ import annotations

import numpy as np
import pytest

import assign_cases as ac
import transport_cases as tc

STARTS = (tc.LEAST_COST, tc.NORTHWEST)
RULES = (tc.DANTZIG, tc.BLAND)


def small_problems(n, seed):
    rng = np.random.default_rng(seed)
    kinds = ("c2", "c99", "zeros", "big", "const")
    return [tc.problem(kinds[k % len(kinds)], int(rng.integers(1, 9)), int(rng.integers(1, 9)), rng) for k in range(n)]


def certificate(C, s, d, r, maximize):
    """Exact on integers: the flows are a plan, the basis a spanning tree, (u, v) dual feasible and tight on it."""
    nr, nc = C.shape
    x, u, v, basis = r["x"], r["u"], r["v"], r["basis"]
    assert (x >= 0).all() and (x.sum(axis=1) == s).all() and (x.sum(axis=0) == d).all()
    assert r["objective"] == (C * x).sum()
    assert basis.shape == (nr + nc - 1,) and (np.diff(basis) > 0).all() and 0 <= basis[0] and basis[-1] < nr * nc
    assert (x.ravel()[np.setdiff1d(np.arange(nr * nc), basis)] == 0).all()
    parent = list(range(nr + nc))                          # nr + nc - 1 edges without a cycle: a spanning tree

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for e in basis:
        a, b = find(int(e) // nc), find(nr + int(e) % nc)
        assert a != b, "the basis has a cycle"
        parent[a] = b
    red = C - u[:, None] - v[None, :]
    assert (red <= 0).all() if maximize else (red >= 0).all()
    assert (red.ravel()[basis] == 0).all()
    assert u[0] == 0


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("rule", RULES, ids=["dantzig", "bland"])
def test_objective_equals_highs_and_the_certificate_holds(start, rule):
    from scipy.optimize import linprog
    for k, (C, s, d) in enumerate(small_problems(80, [1, rule, STARTS.index(start)])):
        nr, nc = C.shape
        A = np.zeros((nr + nc, nr * nc))
        for i in range(nr):
            A[i, i * nc:(i + 1) * nc] = 1.0
        for j in range(nc):
            A[nr + j, j::nc] = 1.0
        for mx in (False, True):
            r = tc.solve(C, s, d, mx, start, rule)
            assert r["status"] == tc.OPTIMAL, (k, mx)
            certificate(C, s, d, r, mx)
            lp = linprog(-C.ravel() if mx else C.ravel(), A_eq=A, b_eq=np.concatenate([s, d]), method="highs")
            assert lp.status == 0 and abs((-lp.fun if mx else lp.fun) - r["objective"]) <= 1e-6 * max(1.0, abs(r["objective"]))


@pytest.mark.parametrize("n", [3, 6, 9])
def test_unit_instances_reach_the_assignment_statements_objective(n):
    rng = np.random.default_rng(n)
    for kind in ("unit", "unit2"):
        for mx in (False, True):
            C, s, d = tc.problem(kind, n, n, rng)
            want = ac.hungarian(C, mx)["objective"]
            for start in STARTS:
                for rule in RULES:
                    r = tc.solve(C, s, d, mx, start, rule)
                    assert r["status"] == tc.OPTIMAL and r["objective"] == want
                    assert np.isin(r["x"], (0.0, 1.0)).all()


def test_a_split_budget_ends_in_the_bits_of_one_call():
    rng = np.random.default_rng(3)
    cut = 0
    for kind in ("c2", "c99", "zeros"):
        C, s, d = tc.problem(kind, 9, 11, rng)
        for start in STARTS:
            for rule in RULES:
                one = tc.solve(C, s, d, False, start, rule)
                for budgets in ([1, 1, 1, 1000], [2, 1000], [one["iterations"] or 1, 1]):
                    st = tc.Statement(C, s, d, False, start)
                    for b in budgets:
                        st.solve(b, rule)
                        cut += st.status == tc.ITER_LIMIT
                    got = st.result()
                    for f in tc.FIELDS:
                        assert np.array_equal(np.asarray(got[f]), np.asarray(one[f])), (kind, start, rule, budgets, f)
    assert cut >= 10                                       # budgets did cut


def test_a_budget_of_exactly_the_iterations_needed_is_sufficient():
    C, s, d = tc.problem("c99", 7, 8, np.random.default_rng(4))
    need = tc.solve(C, s, d, start=tc.NORTHWEST)["iterations"]
    assert need >= 2
    assert tc.solve(C, s, d, start=tc.NORTHWEST, budgets=[need])["status"] == tc.OPTIMAL
    short = tc.solve(C, s, d, start=tc.NORTHWEST, budgets=[need - 1])
    assert short["status"] == tc.ITER_LIMIT and short["iterations"] == need - 1


def test_census_of_the_device_cases_and_every_one_ends_optimal_inside_the_default_budget(capsys):
    """A condition, not a measurement: every device case that no budget cuts on purpose is LPG_OPTIMAL within
    50 (nr + nc) iterations under the statement alone; and the cases hold what they are there for."""
    total = {}
    problems = worst = 0
    for s in tc.DEVICE_CASES:
        nr, nc = s["shape"]
        for r in tc.reference(s):
            assert r["status"] == tc.OPTIMAL and r["iterations"] <= tc.default_budget(nr, nc), tc.name(s)
            worst = max(worst, r["iterations"] / (nr + nc))
            problems += 1
            for k, v in r["census"].items():
                total[k] = total.get(k, 0) + v
    for s in tc.CUT:
        assert any(r["status"] == tc.ITER_LIMIT for r in tc.reference(s)), tc.name(s)
    with capsys.disabled():
        print(f"\ntransport device cases: {problems} problems, at most {worst:.1f} (nr + nc) iterations; census {total}")
    assert total["entering_ties"] >= 100 and total["leaving_ties"] >= 100
    assert total["zero_basic_at_start"] >= 100 and total["zero_basic_at_end"] >= 100 and total["degenerate_steps"] >= 100
    assert total["optimal_at_start"] >= 20 and total["zero_amounts"] >= 50
