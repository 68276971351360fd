"""The tie, tolerance-boundary and non-finite cases of tests/tie_cases.py on
the CPU: what tests/test_gpu_batch_ties.py compares the device with is the
oracle, so here the oracle's side is pinned without a device.

- The census: every interval case the GPU file runs ties where its shape can
  (tie_cases.floors_of), at least 3 times per class, and every tableau on the
  way holds the exactness premise (entries in {-1, 0, 1}); so the GPU cases
  cannot pass vacuously.
- oracle/fraction_oracle.py, an exact second statement of the tie rules
  ("smallest j", "smallest row", under Bland "smallest basic column"), gives
  the same pivots, basis, status and, converted to float, the same tableau bit
  for bit: the arithmetic is exact, so there is no tolerance.
- The comparisons with the tolerances are strict: at least 3 pivots per case
  would differ under <= / >=.
- Non-finite entries: what the oracle does with them, and that a NaN ratio
  loses wherever its row sits.
"""
from __future__ import annotations

import numpy as np
import pytest

import batch_cases as bc
import tie_cases as tc
from oracle import fraction_oracle
from oracle.lpo import Oracle

CASES = tc.interval_cases()
BOUNDARY_CASES = tc.boundary_cases()


def test_the_shapes_sit_on_the_tiers_the_gpu_tests_expect():
    """(70, 200) is beyond the LDS tier's 150 KiB (156944 bytes), (70, 150) is the m > 64 shape within it, and no
    m > 256 fits."""
    tiers = {(m, n): [tc.expected_tier(m, n, nobj) for nobj in (1, 2)] for m, n in tc.SHAPES}
    assert tiers == {(40, 300): [0, 0], (70, 200): [1, 1], (70, 150): [0, 0], (300, 40): [1, 1], (12, 20): [0, 0]}


@pytest.mark.parametrize("s", CASES + BOUNDARY_CASES, ids=tc.case_id)
def test_census_floors(s):
    c = tc.census_of(s)                              # asserts the exactness premise on every tableau it meets
    need = tc.floors_of(s, s["m"], s["n"])
    assert all(c[k] >= 3 for k in need), ({k: c[k] for k in need}, c)
    assert 0 < c["maxlog"] <= s["reserve_log"]
    if s["method"] == "big_m":                       # the class arm of pp_better
        assert c["price_two_classes"] >= 3
        # ties among class-1 columns need pivots at which no M part is negative; the 150 equality rows of
        # (300, 40) over 40 columns are infeasible, so its runs end while class 0 still prices (1 such tie in 8 LPs)
        if s["rule"] == tc.RULE_DANTZIG and s["m"] <= 256:
            assert c["price_cls1"] >= 3
    if s["eps"] is not None:
        assert c["boundary"] >= 3, c


def test_census_counts_by_wave_and_thread():
    st = dict.fromkeys(tc.KEYS, 0)
    tc._where(st, "price", [3, 40])
    tc._where(st, "price", [3, 64])
    tc._where(st, "price", [3, 100, 259])
    assert (st["price"], st["price_xwave"], st["price_thread"]) == (3, 2, 1)


@pytest.mark.parametrize("rule", [tc.RULE_DANTZIG, tc.RULE_BLAND])
@pytest.mark.parametrize("m,n", [(12, 20), (40, 300)])
def test_fraction_oracle_agrees_exactly(m, n, rule):
    for q in range(2):
        T, basis = tc.interval_lp(m, n, tc.SEED + q, "primal")
        o = Oracle(m, n + m + 1)
        o.load_tableau(T, basis)
        res = o.solve(20000, rule)
        f = fraction_oracle.solve(T.tolist(), basis.tolist(), "bland" if rule else "dantzig", 20000)
        lk, lr = o.get_log()
        assert f["pivots"] == list(zip(lk.tolist(), lr.tolist())) and len(lk) >= 10
        assert f["basis"] == o.get_basis().tolist()
        assert f["status"] == "OPTIMAL" and res.status == tc.OPTIMAL
        F = np.array([[float(x) for x in row] for row in f["tableau"]])
        assert np.array_equal(bc.bits(F), bc.bits(o.get_rows()))
        o.close()


@pytest.mark.parametrize("s", [s for s in BOUNDARY_CASES if s["scale"] == 1], ids=tc.case_id)
def test_an_entry_on_eps_opt_is_not_eligible(s):
    """Setting (a): the runs that end OPTIMAL leave reduced costs (the dual: right-hand sides) of exactly -1."""
    want = tc.run_oracle(s)
    done = np.flatnonzero(want["status"] == tc.OPTIMAL)
    assert done.size >= 1
    m, n = s["m"], s["n"]
    left = [want["rows"][q][:m, 0].min() if s["method"] == "dual" else want["rows"][q][m, 1:].min() for q in done]
    assert min(left) == -1.0 and max(left) <= 0.0 and (np.array(left) == -1.0).sum() >= 1


# ---- non-finite entries -----------------------------------------------------

def _bad(case, rule=0):
    """(status, pivots, log) of the non-finite LP of the case, and the whole oracle result."""
    w = tc.run_oracle(tc.nonfinite_spec(case, rule))
    lo, n = int(w["loglen"][:tc.BAD_LP].sum()), int(w["loglen"][tc.BAD_LP])
    log = list(zip(w["logk"][lo:lo + n].tolist(), w["logr"][lo:lo + n].tolist()))
    return int(w["status"][tc.BAD_LP]), int(w["pivots"][tc.BAD_LP]), log, w


@pytest.mark.parametrize("rule", [tc.RULE_DANTZIG, tc.RULE_BLAND])
def test_numeric_rule_of_the_oracle(rule):
    """A b that is NaN or -inf gives theta = 0, so its row is chosen at once and the LP stops NUMERIC; a finite b
    whose ratio overflows loses the ratio test and the LP is solved."""
    for case in ("nan_b", "inf_b", "nan_ratio_only"):
        assert _bad(case, rule)[:3] == (tc.NUMERIC, 0, [])
    status, pivots, log, w = _bad("overflowing_ratio", rule)
    assert status == tc.OPTIMAL and pivots >= 20 and 7 not in [r for _, r in log]
    others = np.arange(8) != tc.BAD_LP
    assert (w["status"][others] == tc.OPTIMAL).all()


@pytest.mark.parametrize("rule", [tc.RULE_DANTZIG, tc.RULE_BLAND])
@pytest.mark.parametrize("case,best", [("nan_ratio", 33), ("nan_ratio_stride", 257)])
def test_nan_ratio_loses_to_every_number(case, best, rule):
    status, pivots, log, w = _bad(case, rule)
    assert (status, pivots, log) == (tc.OPTIMAL, 1, [(1, best)])
    assert np.isnan(w["rows"][tc.BAD_LP]).any() and w["objective"][tc.BAD_LP] == 50.0


@pytest.mark.parametrize("rule", [tc.RULE_DANTZIG, tc.RULE_BLAND])
@pytest.mark.parametrize("nparts", [1, 2, 3, 7])
@pytest.mark.parametrize("nan_row", [0, 1, 69])
def test_nan_ratio_does_not_depend_on_where_its_row_sits(nan_row, nparts, rule):
    """The first eligible row, a later one, the last one; and in every row-block partition (test_oracle.py's
    test_partition_invariance on a NaN ratio)."""
    m, n = 70, 20
    T, basis = tc.nonfinite_batch("nan_ratio")
    o = Oracle(m, n + m + 1)
    o.load_tableau(tc.nan_ratio_lp(T[0], m, n, nan_row=nan_row), basis[0])
    res = o.solve(1, rule, nparts)
    lk, lr = o.get_log()
    assert (res.pivots, lk.tolist(), lr.tolist()) == (1, [1], [33])
    o.close()


def test_two_nan_ratios_order_by_key():
    """nan_ratio_only: rows 5 and 9 both hold b = a = +inf; the smaller key wins, and its pivot element is not
    finite: NUMERIC. The Bland key is the basic column, so swapping the two basic columns swaps nothing else."""
    m, n = 37, 70
    T, basis = tc.nonfinite_batch("nan_ratio_only")
    for rule, swap in ((0, False), (1, False), (1, True)):
        b = basis[tc.BAD_LP].copy()
        if swap:
            b[[5, 9]] = b[[9, 5]]
        o = Oracle(m, n + m + 1)
        o.load_tableau(T[tc.BAD_LP], b)
        out = o.ratio(1, rule, 0)
        assert np.isnan(out[0]) and out[3] == (9 if swap else 5)
        assert o.solve(10, rule).status == tc.NUMERIC
        o.close()


def test_dual_has_no_numeric_rule():
    """b_7 = -inf: row 7 leaves, the pivot makes every other right-hand side +inf and the objective -inf, and the
    dual reports OPTIMAL after that one pivot: neither the oracle nor the kernel has a NUMERIC rule for the dual."""
    status, pivots, log, w = _bad("dual_inf_b")
    assert (status, pivots, log) == (tc.OPTIMAL, 1, [(7, 7)])
    assert w["objective"][tc.BAD_LP] == -np.inf
    others = np.arange(8) != tc.BAD_LP
    assert (w["status"][others] == tc.ITER_LIMIT).all() and (w["pivots"][others] == 5).all()


def test_dual_nan_ratio_in_a_stride_of_256():
    status, pivots, log, w = _bad("dual_nan_ratio_stride")
    assert pivots >= 1 and log[0] == (258, 0)


def test_dual_nan_ratio_loses_to_every_number():
    """The dual's entering column: d_j = +inf over a = -inf is a NaN ratio, and it loses wherever column j is."""
    m, n = 12, 20
    o0 = Oracle(m, n + m + 1)
    o0.generate(n, bc.SEED, 3)
    T0, basis = o0.get_rows(), o0.get_basis()
    o0.close()
    logs = []
    for j in (1, 2, n):
        T = T0.copy()
        T[:m, 0] = -1.0
        T[0, 0] = -2.0                               # row 0 leaves
        T[0, 1:n + 1] = -1.0
        T[m, 1:n + 1] = 2.0 + np.arange(n)
        T[m, 5] = 0.5                                # column 5 holds the least ratio
        T[0, j], T[m, j] = -np.inf, np.inf
        o = Oracle(m, n + m + 1)
        o.load_tableau(T, basis)
        o.solve_dual(1)
        logs.append((o.get_log()[0].tolist(), o.get_log()[1].tolist()))
        o.close()
    assert logs == [([5], [0])] * 3
