"""The Gomory mixed-integer cut as tests/cut_cases.py states it in numpy
(include/lpg.h, "cuts"), without a device: every cut of the chosen models
holds at every integer point of the model and cuts the fractional vertex off,
the edge values of the statement, and the reference walk with cut rounds.

The models: of the integer-coefficient texts under tests/golden/lp/ only
a3_min_eq_neg has a fractional relaxation (a5_lack_row, a8_gcd, kat_min_ge,
kat_negative_rhs and kat_wyndor have integral vertices, kat_unbounded none);
next to it three hand-written models of two or three variables in a small box.
Every one of them has a candidate row at its root (asserted below)."""
from __future__ import annotations

import numpy as np
import pytest

import cut_cases as cc

INT_TOL, EPS_OPT = 1e-6, 1e-9


MODELS = cc.MODELS


@pytest.fixture(scope="module")
def points():
    """name -> integer_points of the model, enumerated once."""
    return {name: cc.integer_points(text, box) for name, (text, box, _, _) in MODELS.items()}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_listed_optimum_is_the_enumerated_one(name, points):
    _, _, sense, z = MODELS[name]
    X, users, obj, _ = points[name]
    assert len(X) > 0
    assert abs((obj.max() if sense == "max" else -obj.max()) - z) < 1e-9      # obj is the max-form objective


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("rounds", [1, 2])
def test_cuts_hold_at_every_integer_point_and_cut_the_vertex_off(name, rounds, points):
    """Cuts from every candidate row of the root, and (rounds = 2) from every candidate row of the LP re-solved
    with the first round's cuts, whose slacks count as continuous."""
    text = MODELS[name][0]
    sm, mask, (T, basis, nact, _), r = cc.root_of(text)
    assert r.status == cc.OPTIMAL
    X = points[name][0]
    N = X.shape[1]
    assert nact == N                                          # the columns behind nact are the artificials
    for rnd in range(rounds):
        m = T.shape[0] - 1
        rows = cc.select_rows(T, basis, m, mask, INT_TOL, cc.MAX_CUTS)
        if rnd == 0:
            assert len(rows) > 0, "the model has no candidate row: the test would be empty"
        if not len(rows):
            break
        G = cc.cut_rows_of(T, basis, nact, mask, rows)
        vertex = np.zeros(nact + 1)
        vertex[basis[basis <= nact]] = T[:m, 0][basis <= nact]
        for t in range(len(rows)):
            g, f0 = -G[t, 1:nact + 1], -G[t, 0]
            # the cut g . x >= f0 over columns 1..nact; the slacks of earlier cuts are s = g' . x - f0'
            assert (X @ g - f0 >= -EPS_OPT).all(), (name, rnd, rows[t], float((X @ g - f0).min()))
            assert f0 - vertex[1:] @ g > INT_TOL
            assert (G[t, nact + 1:] == 0.0).all()
        if rnd + 1 < rounds:
            k = len(rows)
            X = np.hstack([X, X @ (-G[:, 1:nact + 1]).T + G[:, 0][None, :]])     # the new slack columns at the points
            assert (X[:, N:] >= -EPS_OPT).all()
            C, cb, nact2 = cc.cut_child_of(T, basis, nact, mask, rows)
            res = cc.br.oracle_dual(C, cb, nact2, 1 << 40)
            assert int(res["status"][0]) == cc.OPTIMAL
            # the artificial columns behind nact moved right by k; drop them so that columns 1..nact + k line up with X
            keep = np.r_[0:nact2 + 1]
            T, basis, nact, N = res["rows"][0][:, keep], res["basis"][0], nact2, N + k


def test_a_tiny_negative_right_hand_side_gives_f0_zero_and_finite_coefficients():
    T = np.array([[-1e-20, 1.0, 0.5, -0.25, 2.75, -1.5], [0.0, 0.0, -1.0, -1.0, -1.0, -1.0]])
    assert (-1e-20) - np.floor(-1e-20) == 1.0                 # what the guard in frac is for
    G = cc.cut_rows_of(T, np.array([1]), 5, np.array([1, 1, 1, 0, 0]), [0])
    assert G[0, 0] == 0.0 and np.isfinite(G).all()
    # f0 = 0 and rho = 0: an integer column keeps only an integral part of zero, a continuous one its positive part
    assert np.array_equal(np.abs(G[0]), [0.0, 0.0, 0.0, 0.0, 2.75, 0.0])
    assert float(cc.frac(np.float64(-1e-20))) == 0.0 and float(cc.frac(np.float64(-0.25))) == 0.75


def test_basic_columns_get_exact_zeros_by_membership_not_by_value():
    # columns 2 and 4 are basic (rows 0 and 1); the source row stores 1.0 and -0.0 there, and 0.3 in the basic
    # column of the other row (what a tableau never holds, but the rule does not look)
    T = np.array([[2.5, 0.75, 1.0, -0.5, 0.3, 0.25],
                  [1.5, 0.25, -0.0, 0.5, 1.0, -0.75],
                  [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]])
    basis = np.array([2, 4])
    for mask in (np.ones(5, dtype=np.uint8), np.array([0, 1, 0, 0, 1], dtype=np.uint8)):
        G = cc.cut_rows_of(T, basis, 5, mask, [0, 1])
        assert (G[:, [2, 4]] == 0.0).all()
        assert (G[:, [1, 3, 5]] != 0.0).all()
    # columns behind nact (inert artificials) as well
    G = cc.cut_rows_of(T, basis, 4, np.ones(5, dtype=np.uint8), [0])
    assert G[0, 5] == 0.0 and G[0, 3] != 0.0
    # the values: f0 = 0.5, rho = 1; integer 0.75 -> 1 * (1 - 0.75), integer -0.5 -> frac 0.5 <= f0, 0.25 -> 0.25
    G = cc.cut_rows_of(T, basis, 5, np.ones(5, dtype=np.uint8), [0])
    assert np.array_equal(G[0], [-0.5, -0.25, -0.0, -0.5, -0.0, -0.25])
    # continuous: a >= 0 -> a, a < 0 -> rho * (-a)
    G = cc.cut_rows_of(T, basis, 5, np.zeros(5, dtype=np.uint8), [0])
    assert np.array_equal(G[0], [-0.5, -0.75, -0.0, -0.5, -0.0, -0.25])


def test_child_layout():
    T = np.arange(24, dtype=np.float64).reshape(4, 6) / 8.0 + 0.125
    basis = np.array([2, 5, 3])                               # nact = 4: column 5 is an artificial that stayed basic
    C, cb, na = cc.cut_child_of(T, basis, 4, np.ones(4, dtype=np.uint8), [2, 0])
    G = cc.cut_rows_of(T, basis, 4, np.ones(4, dtype=np.uint8), [2, 0])
    assert C.shape == (6, 8) and na == 6
    assert np.array_equal(C[[0, 1, 2, 5]][:, :5], T[:, :5]) and np.array_equal(C[[0, 1, 2, 5]][:, 7], T[:, 5])
    assert np.array_equal(C[3:5, :5], G[:, :5]) and np.array_equal(C[3:5, 7], G[:, 5])
    assert np.array_equal(C[:, 5:7], [[0, 0], [0, 0], [0, 0], [1, 0], [0, 1], [0, 0]])
    assert np.array_equal(cb, [2, 7, 3, 5, 6])


def test_select_rows_order_ties_and_cap():
    T = np.zeros((6, 9))
    T[:5, 0] = [2.5, 7.25, 4.5, 3.0, 1.75]
    basis = np.array([5, 2, 3, 7, 1])
    ones = np.ones(8, dtype=np.uint8)
    # rows 0 and 2 at distance 0.5: the smaller column (3, row 2) first; then 0.25 twice: column 1 (row 4), column 2
    assert cc.select_rows(T, basis, 5, ones, INT_TOL, 8).tolist() == [2, 0, 4, 1]
    assert cc.select_rows(T, basis, 5, ones, INT_TOL, 3).tolist() == [2, 0, 4]
    assert cc.select_rows(T, basis, 5, np.array([1, 1, 0, 1, 1, 1, 1, 1]), INT_TOL, 8).tolist() == [0, 4, 1]
    assert cc.select_rows(T, basis, 5, np.zeros(8, dtype=np.uint8), INT_TOL, 8).size == 0


@pytest.mark.parametrize("name", sorted(MODELS))
def test_reference_walk_with_cut_rounds_reaches_the_enumerated_optimum(name):
    text, _, _, z = MODELS[name]
    for rounds in (0, 1, 2):
        w = cc.reference_walk(text, cut_rounds=rounds, node_limit=200)
        assert w["status"] == "OPTIMAL" and abs(w["z"] - z) < 1e-9, (rounds, w)
        assert w["nodes"] <= 200
    assert cc.reference_walk(text, cut_rounds=0, node_limit=200) == cc.br.reference_walk(text, node_limit=200)


def test_cut_rounds_save_node_lps_on_two_phase():
    """The two-phase model: 7 node LPs without cuts; the root and one LP with the root's two cuts with them."""
    text = MODELS["two_phase"][0]
    plain, cut = cc.reference_walk(text, cut_rounds=0), cc.reference_walk(text, cut_rounds=2)
    assert (plain["nodes"], cut["nodes"]) == (7, 2)
    assert cut["nodes"] < plain["nodes"] and cut["depth"] == 1
