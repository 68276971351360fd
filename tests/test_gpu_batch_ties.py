"""lpg_batch where its comparators have to break ties, sit on a tolerance or
meet a non-finite entry (tests/tie_cases.py), bit for bit against the CPU
oracle per LP: status, pivots, objective bits, basis, the whole log and the
whole tableau (batch_cases.assert_same), no tolerance anywhere.

The generator's LPs never tie (continuous random data), so the tie-breaking
arms of pp_better (v equal, then j; the class arm of Big-M pricing) and of
cand_better (theta equal, then the row or, under Bland, the basic column) run
only here, at the three levels of a block's argmin: the lanes of a wave, the
four waves, and a thread's strided loop. tests/test_tie_cases.py counts, on
the CPU, that every case below ties at every level its shape reaches.
"""
from __future__ import annotations

import numpy as np
import pytest

import batch_cases as bc
import branch_cases as br
import cut_cases as cc
import tie_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.interval_cases()
LDS_CASES = [s for s in CASES if tc.expected_tier(s["m"], s["n"], tc.nobj_of(s)) == tc.TIER_LDS]
NONFINITE_CASES = [tc.nonfinite_spec(case, rule) for case in tc.NONFINITE for rule in (0, 1)
                   if not (tc.NONFINITE[case][4] == "dual" and rule)]


def check(s):
    got, want = tc.run_batch(s), tc.run_oracle(s)
    assert int(got["tier"]) == tc.expected_tier(s["m"], s["n"], tc.nobj_of(s))
    bc.assert_same(got, want)
    return got, want


# ---- interval LPs: ties at most pivots, exact arithmetic --------------------

@pytest.mark.parametrize("s", CASES, ids=tc.case_id)
def test_interval_lps(s):
    got, want = check(s)
    assert (want["loglen"] == want["pivots"]).all() and want["pivots"].sum() >= 15


def test_lds_shapes_on_the_global_tier(tmp_path):
    assert len(LDS_CASES) == 3 * len(tc.METHODS)
    for s, got in zip(LDS_CASES, tc.in_subprocess(LDS_CASES, {"LPG_BATCH_TIER": "global"}, tmp_path)):
        assert int(got["tier"]) == tc.TIER_GLOBAL, tc.case_id(s)
        bc.assert_same(got, tc.run_oracle(s))


def test_lds_shapes_resumed_in_front_of_every_pivot(tmp_path):
    """LPG_BATCH_CHUNK=1: the tie decision is the first thing a launch does."""
    for s, got in zip(LDS_CASES, tc.in_subprocess(LDS_CASES, {"LPG_BATCH_CHUNK": "1"}, tmp_path)):
        assert int(got["tier"]) == tc.TIER_LDS and int(got["chunk"]) == 1, tc.case_id(s)
        bc.assert_same(got, tc.run_oracle(s))


# ---- ragged batches: both tiers in one call ---------------------------------

@pytest.mark.parametrize("method,rule", [("primal", 0), ("primal", 1), ("dual", 0), ("two_phase", 0), ("big_m", 0)])
def test_ragged(method, rule):
    s = tc.ragged_spec(method, rule)
    got, want = tc.run_batch(s), tc.run_oracle(s)
    tiers = [tc.expected_tier(m, n, tc.nobj_of(s)) for m, n in tc.shapes_of(s)]
    assert got["tier"].tolist() == tiers and set(tiers) == {tc.TIER_LDS, tc.TIER_GLOBAL}
    bc.assert_same(got, want)
    assert want["pivots"].min() >= 1


# ---- entries that sit on a tolerance ----------------------------------------

@pytest.mark.parametrize("s", tc.boundary_cases(), ids=tc.case_id)
def test_tolerance_boundaries(s):
    check(s)


# ---- non-finite entries ------------------------------------------------------

def _check_nonfinite(s, got):
    want = tc.run_oracle(s)
    signs = tc.assert_same_nonfinite(got, want)
    others = np.arange(tc.count_of(s)) != tc.BAD_LP
    assert not np.isnan(want["rows"][others]).any()           # so the other LPs were compared bit for bit
    assert np.array_equal(bc.bits(got["rows"][others]), bc.bits(want["rows"][others]))
    return signs


@pytest.mark.parametrize("s", NONFINITE_CASES, ids=tc.case_id)
def test_nonfinite_lp_among_finite_ones(s):
    m, n = tc.NONFINITE[s["nonfinite"]][:2]
    got = tc.run_batch(s)
    assert int(got["tier"]) == tc.expected_tier(m, n)
    signs = _check_nonfinite(s, got)
    print(f"{tc.case_id(s)}: sign bits set among the device's NaNs: {signs.tolist()}")


def test_nonfinite_lps_on_the_global_tier(tmp_path):
    for s, got in zip(NONFINITE_CASES, tc.in_subprocess(NONFINITE_CASES, {"LPG_BATCH_TIER": "global"}, tmp_path)):
        assert int(got["tier"]) == tc.TIER_GLOBAL, tc.case_id(s)
        _check_nonfinite(s, got)


# ---- one branch and one cut level on integral parents ------------------------

def test_nothing_to_branch_on_or_to_cut():
    """A solved interval parent at (40, 300): every basic value is an integer, so branch_select reports no row and
    cut_select no cut for every LP (the "nothing to do" path at a width above one wave), as the numpy statements."""
    import linearprogramming_amd as lpg
    s = tc.spec(40, 300)
    m, n, B = s["m"], s["n"], s["B"]
    built = [tc.build_lp(s, q) for q in range(B)]
    with lpg.BatchEngine(B, m, n + m + 1) as e:
        e.load(np.array([T for T, _ in built]), np.array([b for _, b in built]))
        res = e.solve(20000, 0)
        assert all(r.status == tc.OPTIMAL for r in res)
        rows, basis = e.get_rows(), e.get_basis()
        assert np.array_equal(bc.bits(rows), bc.bits(tc.run_oracle(s)["rows"]))
        mask = np.ones(n + m, dtype=np.uint8)
        for rule in (br.MOST_FRACTIONAL, br.FIRST):
            row, col, value = e.branch_select(mask, 1e-6, rule)
            assert (row == -1).all() and (col == -1).all()
            for q in range(B):
                assert br.select_row(rows[q], basis[q], m, mask, 1e-6, rule) == (-1, -1, 0.0)
        cuts = e.cut_select(mask, 1e-6, 8)
        for q in range(B):
            assert len(cuts[q]) == 0 and len(cc.select_rows(rows[q], basis[q], m, mask, 1e-6, 8)) == 0
        assert (rows[:, :m, 0] % 1.0 == 0.0).all()
