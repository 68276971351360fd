"""The single-LP engine's tie cases (tests/engine_tie_cases.py) on the CPU: what
tests/test_gpu_engine_ties.py compares lpg.Engine with is the oracle, so here
the oracle's side is pinned without a device, and the cases are shown not to
be vacuous for the engine's geometry.

- The census (tie_cases.census with the engine's boundaries): every case ties
  at least 3 times, summed over its two LPs, across every boundary its shape
  has: the 256-row and 512-column blocks of k_prep_d / k_select_d at
  (300, 600), the slices of a forced split into 7 workgroups, and at (70, 150)
  the rank boundaries of a row partition over 2 and over 3 ranks. Pricing under
  Bland has no ties (tie_cases.floors_of's rule). Big-M prices both classes.
  Every tableau on the way holds the exactness premise (census asserts it).
- Every log is longer than twice the block size assigned to it on every path
  (the dual's 128-pivot block excepted, which no log of the dual reaches).
- oracle/fraction_oracle.py, the exact second statement of the tie rules,
  gives the same pivots, basis and tableau as lpo.c at (70, 150).
- The geometry restated in engine_tie_cases.py is what the shapes are chosen
  for: ties can straddle row blocks and column blocks only at (300, 600).

Measured here (two LPs per case): at (300, 600) ratio ties across 256-row
blocks 30 .. 134 in the primal, two-phase and Big-M cases, pricing ties across
512-column blocks 99 .. 116 under Dantzig, the dual 43 leaving-row ties across
row blocks and 37 entering-column ties across column blocks, 21 ties among
class-1 Big-M columns; at (70, 150) ratio ties across the rank boundaries
7 .. 36 (the dual's leaving row 8 and 11), across slices of 10 rows and 32
columns 17 .. 67. Logs: 67 .. 305 pivots at (300, 600) (the dual 17 and 30),
33 .. 92 at (70, 150) (the dual 9 and 14).
"""
from __future__ import annotations

import numpy as np
import pytest

import batch_cases as bc
import engine_tie_cases as ec
import tie_cases as tc
from oracle import fraction_oracle
from oracle.lpo import Oracle

CASES = ec.cases()


def test_the_geometry_the_shapes_were_chosen_for():
    (M, N), (m, n) = ec.LARGE, ec.SMALL
    assert M > ec.D_ROWS and N + M + 1 > ec.D_COLS                    # ties can straddle the pair's blocks
    assert m <= ec.D_ROWS and n + m + 1 <= ec.D_COLS                  # and cannot at the small shape
    assert ec.slice_widths(m, n + m + 1, ec.SPLIT_WG) == (10, 32)
    assert ec.slice_widths(M, N + M + 1, ec.SPLIT_WG) == (43, 129)
    assert ec.rank_rows(m, 2) == [0, 35, 70] and ec.rank_rows(m, 3) == [0, 23, 46, 70]
    for s in CASES:
        for block in {ec.block_of(s, p) for p in ec.paths_of(s)} - {0, ec.DUAL_WIDE_BLOCK}:
            assert ec.fits_all_column(s["m"], ec.ncols_of(s), block, ec.SPLIT_WG)
            assert ec.fits_region(s["m"], s["n"], block, ec.SPLIT_WG)
    for s in ec.two_bank_cases():
        assert 64 < ec.TWO_BANK_BLOCK <= 96
        assert ec.fits_all_column(s["m"], ec.ncols_of(s), ec.TWO_BANK_BLOCK, ec.SPLIT_WG)
        assert ec.fits_region(s["m"], s["n"], ec.TWO_BANK_BLOCK, ec.SPLIT_WG)


def test_blocks_of_and_the_extra_census_keys():
    assert tc.blocks_of([0, 255, 256, 511, 512], 256).tolist() == [0, 0, 1, 1, 2]
    assert tc.blocks_of([0, 22, 23, 45, 46, 69], [23, 46]).tolist() == [0, 0, 1, 1, 2, 2]
    b = {"d": 512, "slice": 32}
    st = dict.fromkeys(list(tc.KEYS) + tc.bounds_keys({"price": b}), 0)
    tc._where(st, "price", np.array([510, 511]), b, np.array([511, 512]))    # columns 511 and 512: two column blocks
    tc._where(st, "price", np.array([0, 30]), b, np.array([1, 31]))           # columns 1 and 31: one slice
    tc._where(st, "price", np.array([30, 31]), b, np.array([31, 32]))         # columns 31 and 32: two slices
    assert (st["price"], st["price_xd"], st["price_xslice"]) == (3, 1, 2)


@pytest.mark.parametrize("s", CASES, ids=ec.case_id)
def test_census_floors(s):
    c = tc.census_of(s, ec.bounds_of(s))             # asserts the exactness premise on every tableau it meets
    need = ec.floors_of(s)
    assert need and all(c[k] >= 3 for k in need), ({k: c[k] for k in need}, c)
    shape = (s["m"], s["n"])
    rows, cols = ("price", "ratio") if s["method"] == "dual" else ("ratio", "price")
    assert f"{rows}_xslice" in need and (f"{rows}_xd" in need) == (shape == ec.LARGE)
    assert (f"{rows}_xrank2" in need and f"{rows}_xrank3" in need) == (shape == ec.SMALL)
    if not (s["rule"] == tc.RULE_BLAND and cols == "price"):
        assert f"{cols}_xslice" in need and (f"{cols}_xd" in need) == (shape == ec.LARGE)
    if s["method"] == "big_m":
        assert c["price_two_classes"] >= 3
        if s["rule"] == tc.RULE_DANTZIG:
            assert c["price_cls1"] >= 3
    # the batch's keys are still counted, as without bounds
    plain = tc.census_of(s)
    assert all(plain[k] == c[k] for k in tc.KEYS)


@pytest.mark.parametrize("s", CASES, ids=ec.case_id)
def test_every_log_covers_two_whole_blocks(s):
    c = tc.census_of(s, ec.bounds_of(s))
    for path in ec.paths_of(s):
        block = ec.block_of(s, path)
        if path == "dual-wide":                      # one partial block: no log of the dual is that long
            assert 0 < c["minlog"] and c["maxlog"] < block
        else:
            assert c["minlog"] > 2 * block, (path, block, c["minlog"])
    want = tc.run_oracle(s)
    assert want["loglen"].min() == c["minlog"] and want["loglen"].max() == c["maxlog"] < s["reserve_log"]
    assert (want["pivots"] == want["loglen"]).all()


@pytest.mark.parametrize("s", ec.two_bank_cases(), ids=ec.case_id)
def test_two_bank_logs(s):
    assert tc.census_of(s, ec.bounds_of(s))["minlog"] > 2 * ec.TWO_BANK_BLOCK


@pytest.mark.parametrize("rule", [tc.RULE_DANTZIG, tc.RULE_BLAND])
def test_fraction_oracle_agrees_exactly(rule):
    m, n = ec.SMALL
    s = ec.case(m, n, "primal", rule)
    want = tc.run_oracle(s)
    for q in range(2):
        T, basis = tc.build_lp(s, q)
        f = fraction_oracle.solve(T.tolist(), basis.tolist(), "bland" if rule else "dantzig", 20000)
        w = ec.lp_of(want, q)
        assert f["pivots"] == list(zip(w["logk"].tolist(), w["logr"].tolist()))
        assert f["basis"] == w["basis"][0].tolist() and f["status"] == "OPTIMAL" and w["status"][0] == tc.OPTIMAL
        F = np.array([[float(x) for x in row] for row in f["tableau"]])
        assert np.array_equal(bc.bits(F), bc.bits(w["rows"][0]))


@pytest.mark.parametrize("method,rule", tc.METHODS)
def test_a_run_continued_by_further_calls_ends_where_one_call_ends(method, rule):
    """What test_gpu_engine_ties.py's budget-limited calls are compared with: the oracle in calls of RESUME_BUDGETS
    with the costs passed each time. The arithmetic is exact, so every call's re-pricing from the costs gives the
    objective rows the pivots had left, and the run ends with the log, basis and tableau of one long call."""
    s = ec.case(*ec.LARGE, method, rule)
    one = tc.run_oracle(s)
    for q in range(2):
        w, r = ec.lp_of(one, q), ec.oracle_resumed(s, q)
        assert r["calls"][0, 0] == tc.ITER_LIMIT and r["calls"][-1, 0] == w["status"][0]
        for key in ("pivots", "basis", "logk", "logr"):
            assert np.array_equal(r[key], w[key]), key
        assert np.array_equal(bc.bits(r["rows"]), bc.bits(w["rows"]))


def test_nonfinite_variants_on_the_oracle():
    """The NaN row in rank 0 and the best row in rank 1; the dual's NaN ratio and its least ratio in two column
    blocks: a NaN ratio loses in both."""
    T, basis, s = ec.nan_ratio_across_ranks()
    w = ec.oracle_lp(T, basis, s)
    assert (w["status"][0], w["pivots"][0], w["logk"].tolist(), w["logr"].tolist()) == (tc.OPTIMAL, 1, [1], [40])
    for nparts in (1, 2):
        o = Oracle(70, T.shape[1])
        o.load_tableau(T, basis)
        o.solve(1, 0, nparts)
        assert [x.tolist() for x in o.get_log()] == [[1], [40]]
        o.close()
    T, basis, s = ec.dual_nan_ratio_across_column_blocks()
    w = ec.oracle_lp(T, basis, s)
    assert w["pivots"][0] >= 1 and (w["logk"][0], w["logr"][0]) == (600, 0)
