"""Branching on the device (include/lpg.h, "branching") against its numpy
statement and the CPU oracle (tests/branch_cases.py), bit for bit: the
children lpg_batch_branch makes, what lpg_batch_branch_select picks, the
re-solve of the children by solve_dual, a second level, the host refusals that
need a parent batch, and frontend.solve_ilp_text against the reference walk."""
from __future__ import annotations

import numpy as np
import pytest

import batch_cases as bc
import branch_cases as br

pytestmark = pytest.mark.gpu

# (m, n): ncols = n + m + 1
# (96, 160) is the global-tier shape: ncols 257, its tableau does not fit in LDS
SHAPES = [(1, 1), (5, 6), (8, 8), (33, 33), (37, 92), (20, 43), (8, 291), (96, 160)]
LDS_SHAPES = SHAPES[:-1]                                   # every LDS-tier shape also runs forced to the global tier


def _check(s, got):
    br.check_selection(s, got)
    want = br.expected(s, got)
    for level in range(1, s["levels"] + 1):
        assert got[f"{level}/built/src"].size > 0
        br.assert_level(got, want, level)
    return want


@pytest.mark.parametrize("m,n", SHAPES)
def test_children_and_their_resolve_equal_numpy_and_the_oracle(m, n):
    """A dense batch, every LP branched both ways: the children as built equal numpy's, and after solve_dual
    the oracle's, bit for bit."""
    s = br.spec("dense", m, n, B=4)
    got = br.run_batch(s)
    assert (got["parent/status"] == br.OPTIMAL).all()
    assert got["1/built/src"].size == 2 * s["B"]            # every LP of these has a fractional basic variable
    _check(s, got)
    nc = n + m + 1
    assert (got["1/built/ncols"] == nc + 1).all() and (got["1/built/m"] == m + 1).all()
    assert (got["1/built/nact"] == nc).all()
    assert (got["1/built/ld"] == ((nc + 1 + 63) & ~63)).all()
    if (m, n) == (37, 92):
        # ncols 130 -> 131: the pitch stays 192 here; (20, 43) is the shape whose child needs the next pitch
        assert got["parent/ld"][0] == 192 and got["1/built/ld"][0] == 192
    if (m, n) == (20, 43):
        assert got["parent/ld"][0] == 64 and got["1/built/ld"][0] == 128
    if (m, n) == (96, 160):
        assert (got["1/built/tier"] == 1).all()
    if (m, n) in ((1, 1), (5, 6)):
        # a single row, or few: x >= ceil(v) leaves the polytope (the CPU walk of these LPs says so too)
        assert set(got["1/solved/status"].tolist()) == {br.OPTIMAL, br.INFEASIBLE}


def test_lds_tier_shapes_forced_to_the_global_tier(tmp_path):
    specs = [br.spec("dense", m, n, B=4) for m, n in LDS_SHAPES]
    for s, got in zip(specs, br.in_subprocess(specs, {"LPG_BATCH_TIER": "global"}, tmp_path)):
        assert (got["parent/tier"] == 1).all() and (got["1/built/tier"] == 1).all()
        _check(s, got)


def test_n_differs_from_count_with_src_repeating_and_descending():
    s = br.spec("dense", 8, 8, B=4, pattern="repeat")
    got = br.run_batch(s)
    src = got["1/built/src"]
    assert src.size != s["B"] and (np.diff(src[:4]) < 0).all() and len(set(src.tolist())) < src.size
    _check(s, got)


@pytest.mark.parametrize("m,n", [(8, 8), (33, 33)])
def test_two_phase_parent_keeps_the_artificials_out_of_pricing(m, n):
    s = br.spec("art", m, n, B=4)
    got = br.run_batch(s)
    af = br.art_first_of(m, n)
    assert (got["parent/nact"] == af - 1).all() and (got["1/built/nact"] == af).all()
    _check(s, got)


def test_ragged_parent_gives_a_ragged_child_on_both_tiers():
    s = br.spec("ragged", lps=[[2, 2], [8, 8], [33, 33], [96, 160]])
    got = br.run_batch(s)
    src = got["1/built/src"]
    assert np.array_equal(got["1/built/m"], got["parent/m"][src] + 1)
    assert np.array_equal(got["1/built/ncols"], got["parent/ncols"][src] + 1)
    assert np.array_equal(got["1/built/art_first"], got["parent/art_first"][src] + 1)
    assert set(got["1/built/tier"].tolist()) == {0, 1}
    _check(s, got)


def test_ragged_two_phase_parent_resolves_with_its_artificials_shifted():
    """Every LP has its own art_first; the child's is one larger and its artificials stay out of the dual pricing."""
    lps = [[2, 2], [8, 8], [33, 33], [96, 160]]
    s = br.spec("ragged_art", lps=lps)
    got = br.run_batch(s)
    af = np.array([br.art_first_of(m, n) for m, n in lps])
    src = got["1/built/src"]
    assert src.size > 0
    assert np.array_equal(got["parent/art_first"], af) and np.array_equal(got["parent/nact"], af - 1)
    assert np.array_equal(got["1/built/art_first"], af[src] + 1) and np.array_equal(got["1/built/nact"], af[src])
    assert (got["1/built/ncols"] > got["1/built/nact"] + 1).all()      # artificial columns behind the new slack
    _check(s, got)


@pytest.mark.parametrize("kind,m,n", [("dense", 8, 8), ("dense", 33, 33), ("art", 8, 8)])
def test_two_levels(kind, m, n):
    s = br.spec(kind, m, n, B=4, levels=2)
    got = br.run_batch(s)
    _check(s, got)
    assert (got["2/built/ncols"] == n + m + 3).all()


# ---------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------
def _loaded(T, basis):
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(T.shape[0], T.shape[1] - 1, T.shape[2])
    e.load(T, basis)
    return e


@pytest.mark.parametrize("rule", [br.MOST_FRACTIONAL, br.FIRST])
def test_selection_equals_the_numpy_rule(rule):
    m, n, B = 33, 33, 6
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(B, m, n + m + 1)
    try:
        e.generate(n, bc.SEED, 0)
        e.solve(br.BUDGET)
        T, basis = e.get_rows(), e.get_basis()
        rng = np.random.default_rng(7)
        nmask = n + m - 5                                   # nmask < ncols - 1
        holes = (rng.random(nmask) < 0.6).astype(np.uint8)
        per_lp = (rng.random((B, nmask)) < 0.5).astype(np.uint8)
        per_lp[B - 1] = 0                                   # an LP without integer columns
        for mask in (holes, per_lp):
            row, col, val = e.branch_select(mask, 1e-6, rule)
            for q in range(B):
                want = br.select_row(T[q], basis[q], m, mask if mask.ndim == 1 else mask[q], 1e-6, rule)
                assert (row[q], col[q]) == want[:2], (q, row[q], col[q], want)
                assert bc.bits(val[q]) == bc.bits(want[2])
        assert row[B - 1] == -1 and col[B - 1] == -1
    finally:
        e.close()


def test_integral_lps_and_the_tie_at_equal_distance():
    m, nc = 3, 8
    T = np.zeros((3, m + 1, nc))
    basis = np.tile(np.array([5, 2, 7]), (3, 1))
    for q in range(3):
        for i in range(m):
            T[q, i, basis[q, i]] = 1.0
    T[0, :m, 0] = [2.5, 7.5, 4.25]        # columns 5 and 2 at distance 0.5: the smaller column, row 1, wins
    T[1, :m, 0] = [3.0, 0.0, 11.0]        # integral
    T[2, :m, 0] = [3.0, 4.0 + 1e-7, 6.0 - 1e-7]   # within int_tol
    e = _loaded(T, basis)
    try:
        for rule in (br.MOST_FRACTIONAL, br.FIRST):
            row, col, val = e.branch_select(np.ones(nc - 1, dtype=np.uint8), 1e-6, rule)
            assert (row[0], col[0], val[0]) == (1, 2, 7.5)
            assert row[1] == col[1] == -1 and row[2] == col[2] == -1
        row, col, _ = e.branch_select(np.array([1, 0, 1, 1, 1, 1, 1], dtype=np.uint8))
        assert (row[0], col[0]) == (0, 5)                   # column 2 masked out
    finally:
        e.close()


# ---------------------------------------------------------------------------
# the host refusals that need a parent batch (tests/test_batch_branch_abi.py has the others)
# ---------------------------------------------------------------------------
def test_refusals_name_the_index_and_leave_the_parent_alone():
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(3, 4, 9)
    g = lpg.BatchEngine.ragged([(4, 9), (2, 5)])
    bm = lpg.BatchEngine(2, 4, 9, big_m=True)
    try:
        e.generate(4, bc.SEED, 0)
        before = bc.bits(e.get_rows()).copy()
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*src\[1\] = 3 outside"):
            e.branch([0, 3], [0, 0], [1, 1])
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*src\[0\] = -1 outside"):
            e.branch([-1], [0], [1])
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*row\[2\] = 4 outside the rows 0\.\.3 of LP 1"):
            e.branch([0, 0, 1], [0, 3, 4], [1, -1, 1])
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*row\[1\] = 2 outside the rows 0\.\.1 of LP 1"):
            g.branch([0, 1], [3, 2], [1, 1])
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*dir\[1\] = 0"):
            e.branch([0, 0], [0, 0], [1, 0])
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*n = 0"):
            e.branch([], [], [])
        with pytest.raises(lpg.LPGError, match=r"rc=-4.*Big-M"):
            bm.branch([0], [0], [1])
        with pytest.raises(lpg.LPGError, match=r"rc=-4.*Big-M"):
            bm.branch_select(np.ones(8, dtype=np.uint8))
        for mask, tol, rule, word in ((np.ones(9), 1e-6, 0, "nmask 9 outside 1..8"), (np.ones(0), 1e-6, 0, "nmask 0"),
                                      (np.ones(8), 0.5, 0, "int_tol"), (np.ones(8), -1.0, 0, "int_tol"),
                                      (np.ones(8), float("nan"), 0, "int_tol"), (np.ones(8), 1e-6, 2, "rule 2")):
            with pytest.raises(lpg.LPGError, match="rc=-1.*" + word):
                e.branch_select(mask, tol, rule)
        assert np.array_equal(bc.bits(e.get_rows()), before)
    finally:
        for x in (e, g, bm):
            x.close()


def test_child_dimension_over_the_limit_is_refused():
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(1, 1, 8192)
    try:
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*child 0 of LP 0.*ncols \+ 1 = 8193"):
            e.branch([0], [0], [1])
    finally:
        e.close()


# ---------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------
def _text(of, st):
    return "OF {\n\t%s\n}\nST {\n\t%s\n}\n" % (of, ";\n\t".join(st))


def _nonneg(n):
    return [f"x{i}>=0" for i in range(1, n + 1)]


MODELS = {
    "two_var": _text("max:z=5x1+8x2", ["x1+x2<=6", "5x1+9x2<=45"] + _nonneg(2)),
    "knapsack": _text("max:z=8x1+11x2+6x3+4x4", ["5x1+7x2+4x3+3x4<=14", "x1<=1", "x2<=1", "x3<=1", "x4<=1"] + _nonneg(4)),
    "two_phase": _text("min:z=3x1+2x2+4x3", ["2x1+2x2+2x3>=7", "3x1-x2+x3=2", "x1+3x3<=9"] + _nonneg(3)),
    "three_var": _text("max:z=7x1+3x2+5x3", ["6x1+4x2+5x3<=23", "3x1+7x2+2x3<=19", "4x1+x2+6x3<=17"] + _nonneg(3)),
    "infeasible": _text("max:z=2x1+x2", ["2x1+2x2=3"] + _nonneg(2)),
    # x1 free: -2 at the optimum through its `latter` column; the tree branches on x2
    "free_negative": _text("max:z=-x1+4x2", ["x1>=-2", "x1+2x2<=1", "x2>=0"]),
    # x1 free, fractional in the relaxation (x1 - x2 = 1/2 and x1 + x2 = 3 meet at (7/4, 5/4))
    "free_fractional": _text("max:z=x1+x2", ["x1+x2<=3", "2x1-2x2<=1", "2x1-2x2>=-3", "x2>=0"]),
    # x1 <= 0: its inverted column
    "nonpositive": _text("max:z=-3x1+2x2", ["-2x1+2x2<=7", "x1>=-3", "x2<=3", "x1<=0", "x2>=0"]),
}
# model -> (status, round(z), the user's variables rounded, nodes, depth): the optimum is brute force's over
# the model's small box, nodes and depth the reference walk's on the CPU (most fractional, int_tol 1e-6)
LISTED = {
    "two_var": ("OPTIMAL", 40, {"x1": 0, "x2": 5}, 9, 5),
    "knapsack": ("OPTIMAL", 21, {"x1": 0, "x2": 1, "x3": 1, "x4": 1}, 13, 5),
    "two_phase": ("OPTIMAL", 11, {"x1": 1, "x2": 2, "x3": 1}, 7, 4),
    "three_var": ("OPTIMAL", 24, {"x1": 3, "x2": 1, "x3": 0}, 15, 5),
    "infeasible": ("INFEASIBLE", None, {}, 9, 4),
    "free_negative": ("OPTIMAL", 6, {"x1": -2, "x2": 1}, 3, 2),
    "free_fractional": ("OPTIMAL", 3, {"x1": 1, "x2": 2}, 3, 2),
    "nonpositive": ("OPTIMAL", 9, {"x1": -3, "x2": 0}, 5, 3),
}


def _same_as_walk(sol, ref):
    assert (sol.status, sol.nodes, sol.depth, sol.pivots) == (ref["status"], ref["nodes"], ref["depth"], ref["pivots"])
    if ref["z"] is None:
        assert np.isnan(sol.z) and not sol.variables
    else:
        assert bc.bits(sol.z) == bc.bits(ref["z"])
        assert sol.variables.keys() == ref["variables"].keys()
        for k, v in ref["variables"].items():
            assert bc.bits(sol.variables[k]) == bc.bits(v), k


@pytest.mark.parametrize("name", sorted(MODELS))
def test_solve_ilp_text_equals_the_reference_walk_and_the_listed_optimum(name):
    from linearprogramming_amd import frontend as F
    ref = br.reference_walk(MODELS[name], node_limit=100)
    assert ref["nodes"] < 100
    sol = F.solve_ilp_text(MODELS[name])
    _same_as_walk(sol, ref)
    status, z, x, nodes, depth = LISTED[name]
    assert (sol.status, sol.nodes, sol.depth) == (status, nodes, depth)
    if z is not None:
        assert round(sol.z) == z and abs(sol.z - z) < 1e-9
        assert {k: round(sol.variables[k]) for k in x} == x


def test_mixed_only_x1_integer():
    from linearprogramming_amd import frontend as F
    ref = br.reference_walk(MODELS["three_var"], integer=["x1"])
    sol = F.solve_ilp_text(MODELS["three_var"], integer=["x1"])
    _same_as_walk(sol, ref)
    assert sol.status == "OPTIMAL" and abs(sol.variables["x1"] - round(sol.variables["x1"])) < 1e-9
    assert abs(sol.variables["x2"] - round(sol.variables["x2"])) > 0.1      # the others stay continuous
    assert sol.z > 24.0 + 1e-9                              # better than the all-integer optimum


def test_node_limit():
    from linearprogramming_amd import frontend as F
    ref = br.reference_walk(MODELS["three_var"], node_limit=3)
    sol = F.solve_ilp_text(MODELS["three_var"], node_limit=3)
    _same_as_walk(sol, ref)
    assert sol.status == "NODE_LIMIT" and 3 < sol.nodes < 15


def test_first_rule_reaches_the_same_optimum():
    from linearprogramming_amd import frontend as F
    ref = br.reference_walk(MODELS["knapsack"], rule=br.FIRST, node_limit=100)
    sol = F.solve_ilp_text(MODELS["knapsack"], rule=br.FIRST)
    _same_as_walk(sol, ref)
    assert sol.status == "OPTIMAL" and round(sol.z) == 21
