"""The goal-programme statement (tests/goal_cases.py) on the CPU: it is the
committed oracle's Big-M at K = 2 and its primal simplex at K = 1, bit for bit;
its optima carry a certificate in exact arithmetic; the sequential method with
scipy.optimize.linprog reaches the same levels; the front end's arrays solve the
textbook model; and the device cases of tests/test_gpu_batch_goal.py exercise
what they are there for (the census).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import batch_cases as bc
import goal_cases as gc
from goal_cases import BLAND, DANTZIG, INFEASIBLE, ITER_LIMIT, OPTIMAL, UNBOUNDED
from oracle.lpo import Oracle

RULES = [DANTZIG, BLAND]

# measured over small_cases() with scipy 1.15.3 (HiGHS): the largest |statement - linprog| / max(1, |linprog|) of any level
SEQUENTIAL_MEASURED = 2.94e-14


# ---- the statement against the oracle ------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("budgets", [[100000], [3, 100000], [0, 5, 100000]])
@pytest.mark.parametrize("m,n", [(8, 8), (13, 9), (33, 33)])
def test_two_levels_are_the_oracles_big_m(m, n, budgets, rule):
    A, basis, costs, af = gc.artificial(m, n, 2, 3, bc.SEED)
    for b in range(3):
        res, T, bas, lk, lr, attain = gc.statement(A[b], basis[b], costs[b], budgets, rule)
        o = Oracle(m, n + m + 1, nobj=2)
        T0 = np.zeros((m + 2, n + m + 1))
        T0[:m] = A[b]
        o.load_tableau(T0, basis[b])
        for c, budget in enumerate(budgets):
            r = o.solve_big_m(af, np.append(costs[b, 1], 0.0), budget, rule)
            # Big-M's INFEASIBLE is the statement's OPTIMAL / UNBOUNDED: the statement has no feasibility test
            assert res[c].status == r.status or (r.status == INFEASIBLE and res[c].status in (OPTIMAL, UNBOUNDED))
            assert res[c].pivots == r.pivots
        k, rr = o.get_log()
        assert np.array_equal(k, lk) and np.array_equal(rr, lr) and np.array_equal(o.get_basis(), bas)
        assert np.array_equal(bc.bits(o.get_rows()), bc.bits(T)) and np.array_equal(bc.bits(attain), bc.bits(T[m:, 0]))
        o.close()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("budgets", [[100000], [3, 100000]])
@pytest.mark.parametrize("m,n", [(8, 8), (13, 9), (33, 33)])
def test_one_level_is_the_oracles_primal_simplex(m, n, budgets, rule):
    A, basis, costs, _ = gc.artificial(m, n, 1, 3, bc.SEED)
    for b in range(3):
        res, T, bas, lk, lr, _ = gc.statement(A[b], basis[b], costs[b], budgets, rule)
        o = Oracle(m, n + m + 1)
        T0 = np.zeros((m + 1, n + m + 1))
        T0[:m] = A[b]
        o.load_tableau(T0, basis[b])
        for c, budget in enumerate(budgets):
            o.set_objective(np.append(costs[b, 0], 0.0))          # every call of the statement starts from fresh rows
            r = o.solve(budget, rule)
            assert (res[c].status, res[c].pivots) == (r.status, r.pivots)
        k, rr = o.get_log()
        assert np.array_equal(k, lk) and np.array_equal(rr, lr) and np.array_equal(o.get_basis(), bas)
        assert np.array_equal(bc.bits(o.get_rows()), bc.bits(T))
        o.close()


# ---- the integer-data cases of up to 12 rows --------------------------------------------

def small_cases():
    """(name, A, basis, costs) of the textbook literal and the graded cases of up to 12 rows."""
    out = [("textbook",) + gc.textbook()]
    for h, g, n, K, B, seed in gc.GRADED:
        if h + g <= 12:
            out += [(f"graded{(h, g, n, K)}#{b}",) + gc.graded(h, g, n, K, seed + b) for b in range(B)]
    return out


def exact_tableau(A, basis, costs):
    """B^-1 [b | A] and the K objective rows of the basis, in fractions.Fraction."""
    m, nc = A.shape
    M = [[Fraction(float(x)) for x in row] for row in A]
    for i in range(m):                                  # Gauss-Jordan on the basic columns, row i's pivot in column basis[i]
        k = int(basis[i])
        p = next(r for r in range(i, m) if M[r][k] != 0)
        M[i], M[p] = M[p], M[i]
        piv = M[i][k]
        M[i] = [x / piv for x in M[i]]
        for r in range(m):
            if r != i and M[r][k] != 0:
                f = M[r][k]
                M[r] = [x - f * y for x, y in zip(M[r], M[i])]
    # row i holds the unit of column basis[i], as row i of the float tableau does
    D = []
    for c in costs:
        cf = [Fraction(float(x)) for x in c]
        cB = [cf[int(basis[i]) - 1] for i in range(m)]
        D.append([sum(cB[i] * M[i][j] for i in range(m)) - (cf[j - 1] if j else 0) for j in range(nc)])
    return M, D


@pytest.mark.parametrize("rule", RULES)
def test_optima_carry_an_exact_certificate(rule):
    exact_runs = 0
    for name, A, basis, costs in small_cases():
        res, T, bas, _, _, attain = gc.statement(A, basis, costs, [100000], rule)
        assert res[-1].status == OPTIMAL, name
        m = A.shape[0]
        M, D = exact_tableau(A, bas, costs)
        assert all(M[i][0] >= 0 for i in range(m)), name
        nonbasic = [j for j in range(1, A.shape[1]) if j not in set(bas.tolist())]
        for j in nonbasic:
            lex = [D[k][j] for k in range(len(D))]
            first = next((x for x in lex if x != 0), 0)
            assert first >= 0, (name, j, lex)
        xb_exact = {int(bas[i]): M[i][0] for i in range(m)}
        if all(Fraction(float(T[i, 0])) == xb_exact[int(bas[i])] for i in range(m)) and \
                all(Fraction(float(T[m + k, j])) == D[k][j] for k in range(len(D)) for j in range(A.shape[1])):
            exact_runs += 1
            assert [Fraction(float(a)) for a in attain] == [D[k][0] for k in range(len(D))], name
    print("float runs that were exact in every entry:", exact_runs)
    assert exact_runs >= 1            # the textbook literal at the least: the check above is not vacuous


# ---- the sequential method with scipy ------------------------------------------------------

def sequential_linprog(A, basis, costs):
    """K linprog solves: level k minimises its weighted deviation with the earlier levels' optima as constraints.
    The rows of A are equalities over columns 1..N >= 0 (slacks and deviations are columns)."""
    from scipy.optimize import linprog
    Aeq, beq = A[:, 1:], A[:, 0]
    extra_A, extra_b, levels = [], [], []
    for c in costs:
        r = linprog(-c, A_eq=np.vstack([Aeq] + extra_A), b_eq=np.concatenate([beq, extra_b]), bounds=(0, None),
                    method="highs")
        assert r.status == 0, r.message
        levels.append(r.fun)
        extra_A.append(-c[None, :])
        extra_b.append(r.fun)
    return np.array(levels)


def test_the_sequential_method_reaches_the_same_levels():
    """Largest relative difference measured over these cases: 2.94e-14 (SEQUENTIAL_MEASURED); ten times that is asserted.
    HiGHS's own tolerances enter, so the bound is measured, not derived."""
    worst = 0.0
    for name, A, basis, costs in small_cases():
        res, _, _, _, _, attain = gc.statement(A, basis, costs, [100000], DANTZIG)
        assert res[-1].status == OPTIMAL
        want = sequential_linprog(A, basis, costs)
        got = -attain                                   # the weighted deviations
        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))))
    print("largest relative difference:", worst)
    assert worst <= 10 * SEQUENTIAL_MEASURED


# ---- the front end over the statement ----------------------------------------------------------

def front(model, rule=DANTZIG):
    from linearprogramming_amd import frontend as F
    arrays = F.goal_arrays(model)
    rows, basis, costs = arrays[:3]
    res, T, bas, _, _, attain = gc.statement(rows, basis, costs, [50 * sum(rows.shape)], rule)
    return F._goal_readout(model, arrays, res[-1].status, res[-1].pivots, attain, T[:rows.shape[0], 0], bas), arrays


@pytest.mark.parametrize("rule", RULES)
def test_frontend_textbook_model(rule):
    sol, arrays = front(gc.textbook_model(), rule)
    A, basis, costs = gc.textbook()
    assert np.array_equal(arrays[0], A) and np.array_equal(arrays[1], basis) and np.array_equal(arrays[2], costs)
    assert arrays[3:] == (0, 3)
    assert sol.status == "OPTIMAL" and np.array_equal(sol.x, [2.0, 4.0]) and np.array_equal(sol.attained, [0.0, 0.0, 0.0])
    assert np.array_equal(sol.under, [2.0, 0.0, 0.0]) and np.array_equal(sol.over, [0.0, 0.0, 0.0])


def test_frontend_hard_rows_targets_and_limits():
    from linearprogramming_amd import frontend as F
    # a hard = row: x1 + x2 = 6 (an artificial, so device level 0 is theirs); goals x1 >= 4 (P1), x2 >= 4 (P2)
    eq = F.GoalModel(A=[[1, 1]], sense=[0], b=[6], G=[[1, 0], [0, 1]], target=[4, 4], under=[(1, 1.0), (2, 1.0)],
                     over=[None, None])
    sol, arrays = front(eq)
    assert arrays[3:] == (1, 2) and arrays[2].shape[0] == 3 and arrays[2][0, -1] == -1.0
    assert sol.status == "OPTIMAL" and np.array_equal(sol.x, [4.0, 2.0]) and np.array_equal(sol.attained, [0.0, 2.0])
    # a hard >= row that contradicts a hard <= row
    bad = F.GoalModel(A=[[1, 1], [1, 0]], sense=[-1, 1], b=[6, 7], G=[[1, 0]], target=[4], under=[(1, 1.0)], over=[None])
    sol, _ = front(bad)
    assert sol.status == "INFEASIBLE" and np.isnan(sol.x).all()
    # the same rows written with negative right-hand sides, and a negative target: -x1 + x2 + d- - d+ = -1
    neg = F.GoalModel(A=[[-1, -1]], sense=[1], b=[-6], G=[[-1, 1]], target=[-1], under=[(1, 1.0)], over=[(2, 1.0)])
    sol, arrays = front(neg)
    rows, basis = arrays[0], arrays[1]
    assert rows[0, 0] == 6.0 and rows[1, 0] == 1.0 and basis.tolist() == [5, 4]       # the slack; d+ holds +1 after the flip
    assert sol.status == "OPTIMAL" and sol.under[0] == 0.0 and sol.over[0] == 0.0 and np.array_equal(sol.attained, [0.0, 0.0])
    assert sol.x[1] - sol.x[0] == -1.0
    with pytest.raises(F.FrontendError, match="8 priority levels"):
        F.goal_arrays(F.GoalModel(A=[], sense=[], b=[], G=[[1.0]], target=[1], under=[(8, 1.0)], over=[None]))
    with pytest.raises(F.FrontendError, match="weight > 0"):
        F.goal_arrays(F.GoalModel(A=[], sense=[], b=[], G=[[1.0]], target=[1], under=[(1, 0.0)], over=[None]))
    assert F.solve_goal([]) == []


# ---- the census of the device cases: a condition, not a measurement -------------------------------

def census(s):
    tot = {"pricings": 0, "arm": 0, "ties": 0, "classes": {}}
    for rule in RULES:
        c = {}
        want = gc.run_statement({**s, "rule": rule}, census=c)
        assert (want["status"] == OPTIMAL).all()
        for key in ("pricings", "arm", "ties"):
            tot[key] += c.get(key, 0)
        for cls, cnt in c.get("classes", {}).items():
            tot["classes"][cls] = tot["classes"].get(cls, 0) + cnt
    return tot


@pytest.mark.parametrize("h,g,n,K,B,seed", gc.GRADED)
def test_census_of_the_graded_cases(h, g, n, K, B, seed):
    """Both rules together. Found: (2, 3, 3, 3): pivots 32 / 52 / 25, the arm decides 13 of 109 pricings, 7 ties;
    (4, 8, 8, 4): 73 / 137 / 169 / 18, 137 of 397, 10; (6, 16, 16, 8): classes 0..4 (34 / 138 / 181 / 43 / 13),
    225 of 409, 15; (8, 9, 300, 3): 34 / 134 / 430, 77 of 598, 17; the longest run 206 pivots (Bland)."""
    c = census(gc.graded_spec(h, g, n, K, B, seed))
    print((h, g, n, K), c)
    if K <= 4:
        assert sorted(c["classes"]) == list(range(K))
    else:
        assert len(c["classes"]) >= 5
    assert c["ties"] >= 3 and c["arm"] >= 10


def test_census_of_the_literals():
    c = census(gc.spec("ladder", B=1))
    assert sorted(c["classes"]) == list(range(8)) and all(v == 2 for v in c["classes"].values())
    c = census(gc.spec("textbook", B=1))
    assert set(c["classes"]) >= {1, 2}
