"""The scenario restatement as tests/scenario_cases.py states it in numpy
(include/lpg.h, "scenarios"), without a device: column 0 restated for another
right-hand side plus the oracle's dual simplex ends where that scenario's LP
has its optimum, checked in exact arithmetic, or INFEASIBLE where a cold solve
says so; and the cases are not copies of one another (some scenarios need dual
pivots, some none)."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import branch_cases as br
import scenario_cases as sc

DENSE = [(8, 8), (5, 7), (16, 12)]
ART = [(8, 8), (16, 16)]


def _solve_exact(M, rhs):
    """x with M x = rhs over the rationals (M square and regular), by Gauss-Jordan elimination."""
    n = len(M)
    a = [[Fraction(v) for v in row] + [Fraction(r)] for row, r in zip(M, rhs)]
    for c in range(n):
        p = next(i for i in range(c, n) if a[i][c] != 0)
        a[c], a[p] = a[p], a[c]
        inv = 1 / a[c][c]
        a[c] = [v * inv for v in a[c]]
        for i in range(n):
            if i != c and a[i][c] != 0:
                f = a[i][c]
                a[i] = [v - f * w for v, w in zip(a[i], a[c])]
    return [row[n] for row in a]


def _walk(m, n, kind):
    """LP 0 of the case through the restatement and the oracle: (T0, ident, nact, the scenarios, one
    (status, pivots, final basis) per scenario)."""
    T0, ident, T, basis, nact, r = sc.solved_parent(m, n, sc.SEED, kind)
    assert r.status == sc.OPTIMAL and not (basis > nact).any()
    S = sc.scenarios(T0[:-1, 0], kind == 0)
    ends = []
    for rhs in S:
        x = br.oracle_dual(*sc.child_of(T, basis, nact, ident, rhs))
        ends.append((int(x["status"][0]), int(x["pivots"][0]), x["basis"][0]))
    return T0, ident, nact, S, ends


def _cold_status(T0, ident, rhs, m, n, kind):
    from oracle.lpo import Oracle
    T = T0.copy()
    T[:m, 0] = rhs
    o = Oracle(m, n + m + 1)
    o.load_tableau(T, ident)
    r = o.solve_two_phase(br.art_first_of(m, n), None, sc.BUDGET) if kind == 2 else o.solve(sc.BUDGET)
    o.close()
    return r.status


def _assert_exact_optimum(T0, nact, rhs, fb):
    """The basis fb is primal and dual feasible for max c.x, A x = rhs, x >= 0 over columns 1..nact, the columns
    behind nact held at zero: x_B = B^-1 rhs >= 0 and d_j = c_B B^-1 a_j - c_j >= 0, exactly."""
    m = T0.shape[0] - 1
    assert (fb >= 1).all() and (fb <= nact).all(), fb
    A, c = T0[:m], -T0[m]                                   # column j of A is A[:, j]; c_j = -(the loaded objective row)
    B = [[A[i, j] for j in fb] for i in range(m)]
    xB = _solve_exact(B, rhs)
    assert all(v >= 0 for v in xB), [float(v) for v in xB if v < 0]
    y = _solve_exact([[A[i, j] for i in range(m)] for j in fb], [c[j] for j in fb])     # B^T y = c_B
    for j in range(1, nact + 1):
        d = sum(y[i] * Fraction(A[i, j]) for i in range(m)) - Fraction(c[j])
        assert d >= 0, (j, float(d))


@pytest.mark.parametrize("m,n", DENSE)
def test_dense_scenarios_end_at_their_exact_optimum_or_infeasible(m, n):
    T0, ident, nact, S, ends = _walk(m, n, 0)
    for c, (rhs, (status, pivots, fb)) in enumerate(zip(S, ends)):
        if c == len(S) - 1:
            assert status == sc.INFEASIBLE                   # rhs[m // 2] = -1 on a row of non-negative coefficients
            assert (T0[m // 2, 1:] >= 0).all() and rhs[m // 2] == -1.0
            continue
        assert status == sc.OPTIMAL == _cold_status(T0, ident, rhs, m, n, 0)
        _assert_exact_optimum(T0, nact, rhs, fb)
    assert ends[0][1] == 0                                   # scenario 0 is the parent's own right-hand side
    assert any(p > 0 for _, p, _ in ends) and any(p == 0 for _, p, _ in ends)


@pytest.mark.parametrize("m,n,infeasible", [(8, 8, 2), (16, 16, 4)])
def test_artificial_scenarios_agree_with_a_cold_two_phase(m, n, infeasible):
    T0, ident, nact, S, ends = _walk(m, n, 2)
    assert nact == br.art_first_of(m, n) - 1
    for rhs, (status, pivots, fb) in zip(S, ends):
        assert status in (sc.OPTIMAL, sc.INFEASIBLE)
        assert status == _cold_status(T0, ident, rhs, m, n, 2)
        if status == sc.OPTIMAL:
            _assert_exact_optimum(T0, nact, rhs, fb)
    assert sum(1 for st, _, _ in ends if st == sc.INFEASIBLE) == infeasible


def test_rhs_column_order_and_frame():
    # B^-1 in columns 2 and 3 (the frame's e_0 and e_1), an objective row; the sums in ascending i
    T = np.array([[9.0, 1.0, 0.5, -0.25], [9.0, 0.0, 1e-17, 1.0], [9.0, 2.0, 3.0, -1.0]])
    col = sc.rhs_column(T, [2, 3], [4.0, 8.0])
    assert np.array_equal(col, [0.5 * 4 - 0.25 * 8, 8.0, 3.0 * 4 - 8.0])       # 1e-17 * 4 + 8 rounds to 8
    assert np.array_equal(sc.rhs_column(T, [3, 2], [8.0, 4.0]), [0.0, 8.0, 4.0])
    big = np.array([[0.0, 1.0, 1.0, 1.0]])
    assert sc.rhs_column(big, [1, 2, 3], [1e16, 1.0, -1e16])[0] == 0.0        # (1e16 + 1) - 1e16 in that order
    assert sc.rhs_column(big, [1, 2, 3], [1e16, -1e16, 1.0])[0] == 1.0
    C, cb, na = sc.child_of(T, np.array([2, 3]), 3, [2, 3], [4.0, 8.0])
    assert np.array_equal(C[:, 1:], T[:, 1:]) and np.array_equal(C[:, 0], col) and na == 3 and cb.tolist() == [2, 3]
    assert T[0, 0] == 9.0                                    # the parent is not written


def test_recipe_is_fixed():
    b = np.arange(1.0, 6.0)
    S, S2 = sc.scenarios(b, True), sc.scenarios(b, True, draw=1)
    assert S.shape == (8, 5) and np.array_equal(S[0], b) and np.array_equal(S2[0], b)
    rng = np.random.default_rng(11)
    first = [b * (0.2 + 2.5 * rng.random(5)) for _ in range(7)]
    assert np.array_equal(S[1:7], first[:6]) and S[7, 2] == -1.0 and np.array_equal(np.delete(S[7], 2), np.delete(first[6], 2))
    assert np.array_equal(S2[1], b * (0.2 + 2.5 * rng.random(5)))             # the second draw goes on
    assert np.array_equal(sc.scenarios(b, False)[7], first[6])
    assert np.array_equal(sc.scenarios(b, True, nscen=4), S[:4])
