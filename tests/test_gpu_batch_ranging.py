"""Ranging on the device (include/lpg.h, "ranging") against its numpy statement
(tests/ranging_cases.py), bit for bit, on the tableau the batch itself returns:
batches of one shape and a ragged one, children of branch() and cut(),
tolerance edges, non-finite entries, the refusals that need a batch, no side
effects, the groups one by one, lpgcli --ranging, and
frontend.sensitivity_batch against re-solves of the moved models."""
from __future__ import annotations

import copy
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ranging_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-9


def _range_and_compare(e, res, ident, eps=EPS):
    state = rc.state_of(e, res)
    got = rc.device_ranging(e, ident)
    want = rc.expected(state, ident, eps)
    rc.assert_same(got, want)
    return state, got


@pytest.mark.parametrize("name", list(rc.CASES))
def test_every_array_equals_the_numpy_statement(name):
    cases = rc.CASES[name]
    e, res, ident = rc.solved_engine(cases)
    try:
        state, got = _range_and_compare(e, res, ident)
        tier = e.info.tier
    finally:
        e.close()
    m, n = cases[0]["m"], cases[0]["n"]
    st = state["status"]
    if name == "interval_art-12x20":
        assert st == [rc.INFEASIBLE, rc.OPTIMAL, rc.INFEASIBLE, rc.INFEASIBLE]
        dual, at = got["dual"].reshape(4, m), got["rhs_lo_at"].reshape(4, m)
        assert np.isnan(dual[[0, 2, 3]]).all() and not np.isnan(dual[1]).any()
        assert (at[[0, 2, 3]] == -1).all() and (got["cost_hi_at"].reshape(4, -1)[[0, 2, 3]] == 0).all()
    else:
        assert st == [rc.OPTIMAL] * 4
        assert (got["cost_lo"] <= 0).all() and (got["rhs_hi"] >= 0).all()
    if cases[0]["kind"] in ("artificial", "interval_art"):
        nact = state["nact"][1]
        assert nact < n + m and (np.array(ident) > nact).any()                   # ident behind nact
        inert = got["cost_hi"].reshape(4, -1)[1, nact:]
        assert np.isposinf(inert).all()
    if name == "dense-130x130":
        assert tier == 1                                                         # the global tier solved it


def test_a_ragged_batch_of_six_shapes_with_its_own_art_first_per_lp():
    e, res, ident = rc.solved_engine(rc.RAGGED, ragged=True)
    try:
        state, got = _range_and_compare(e, res, ident)
        r = e.ranging(ident)
    finally:
        e.close()
    assert len(set(state["status"])) > 1 and state["status"].count(rc.OPTIMAL) >= 4
    for q, c in enumerate(rc.RAGGED):                                            # one array per LP, of the LP's shape
        assert r.dual[q].shape == (c["m"],) and r.cost_hi_at[q].shape == (state["rows"][q].shape[1] - 1,)
    assert all(na < T.shape[1] - 1 for na, T in zip(state["nact"], state["rows"]))


@pytest.mark.parametrize("how", ["branch", "cut"])
def test_a_child_resolved_by_solve_dual_with_ident_extended_by_its_new_slacks(how):
    cases = rc.uniform("dense", 12, 10)
    e, res, ident = rc.solved_engine(cases)
    ch = None
    try:
        mask = np.ones(10 + 12, dtype=np.uint8)
        nact = e.active_columns(0)[0]
        if how == "branch":
            rows, _, _ = e.branch_select(mask)
            src = np.array([q for q in range(e.count) if rows[q] >= 0], dtype=np.int64)
            ch = e.branch(src, rows[src], np.array([(-1, 1)[q % 2] for q in src], dtype=np.int8))
            grow = 1
        else:
            per = e.cut_select(mask, max_cuts=2)
            src = np.array([q for q in range(e.count) if len(per[q]) == 2], dtype=np.int64)
            ch = e.cut(src, [per[q] for q in src], mask)
            grow = 2
        assert src.size >= 2
        cres = ch.solve_dual(rc.BUDGET)
        cident = [np.concatenate([ident[q], nact + 1 + np.arange(grow)]) for q in src]
        state, _ = _range_and_compare(ch, cres, cident)
        assert rc.OPTIMAL in state["status"]
    finally:
        if ch is not None:
            ch.close()
        e.close()


def _loaded(T, basis):
    """A batch of the hand-made tableaus T [B, m+1, ncols], solved: every one is optimal as it stands (0 pivots)."""
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(T.shape[0], T.shape[1] - 1, T.shape[2])
    e.load(T, basis)
    res = e.solve(rc.BUDGET)
    assert [(r.status, r.pivots) for r in res] == [(rc.OPTIMAL, 0)] * T.shape[0]
    return e, res


def _hand_made():
    """m = 3, columns 1..4 nonbasic, 5..7 the basis: d = 1, 2, 3, 4 and b = 1, 2, 3."""
    T = np.zeros((1, 4, 8))
    T[0, :3, 0] = [1.0, 2.0, 3.0]
    T[0, 3, 1:5] = [1.0, 2.0, 3.0, 4.0]
    T[0, [0, 1, 2], [5, 6, 7]] = 1.0
    return T, np.array([[5, 6, 7]], dtype=np.int64)


def test_tolerance_edges_eps_is_no_candidate_the_next_double_is():
    up, dn = np.nextafter(EPS, 1.0), np.nextafter(-EPS, -1.0)
    T, basis = _hand_made()
    T[0, 0, 1:5] = [EPS, up, -EPS, dn]        # row 0: columns 1 and 3 sit on the tolerance, 2 and 4 just beyond it
    T[0, 1, 1:5] = [EPS, -EPS, 0.0, 0.0]      # row 1: nothing beyond it
    T[0, :3, 1] = [EPS, up, dn]               # column 1 as a frame column (ident[0] = 1): rows 1 and 2 beyond it
    ident = np.array([[1, 6, 7]], dtype=np.int64)
    e, res = _loaded(T, basis)
    try:
        _, got = _range_and_compare(e, res, ident)
    finally:
        e.close()
    # cost of basic column 5 (row 0): candidates 2 (lower) and 4 (upper) only
    assert (got["cost_lo_at"][4], got["cost_hi_at"][4]) == (2, 4)
    assert got["cost_lo"][4] == -2.0 / up and got["cost_hi"][4] == -4.0 / dn
    # cost of basic column 6 (row 1): its entries are eps, -eps and (column 1) the next double up
    assert (got["cost_lo_at"][5], got["cost_hi_at"][5]) == (1, 0) and np.isposinf(got["cost_hi"][5])
    # right-hand side of frame row 0 through column 1: row 0 on the tolerance, row 1 lower, row 2 upper
    assert (got["rhs_lo_at"][0], got["rhs_hi_at"][0]) == (1, 2)
    assert got["rhs_lo"][0] == -2.0 / up and got["rhs_hi"][0] == -3.0 / dn


def test_a_nan_ratio_loses_to_a_number_and_alone_gives_none():
    inf = np.inf
    T, basis = _hand_made()
    T[0, 3, 1] = inf                          # d_1 = +inf
    T[0, 0, 1:5] = [inf, 1.0, 0.0, 0.0]       # row 0: x = a = +inf in column 1 (q NaN), a finite candidate in column 2
    T[0, 1, 1:5] = [inf, 0.0, 0.0, 0.0]       # row 1: the NaN alone
    T[0, 2, 0] = inf                          # b_2 = +inf
    T[0, :3, 2] = [1.0, 0.0, inf]             # frame column 2: row 2 has x = a = +inf, row 0 a finite candidate
    T[0, :3, 3] = [0.0, 0.0, inf]             # frame column 3: the NaN alone
    ident = np.array([[2, 3, 7]], dtype=np.int64)
    e, res = _loaded(T, basis)
    try:
        _, got = _range_and_compare(e, res, ident)
    finally:
        e.close()
    assert (got["cost_lo_at"][4], got["cost_lo"][4]) == (2, -2.0)
    assert got["cost_lo_at"][5] == 0 and np.isneginf(got["cost_lo"][5])
    assert (got["rhs_lo_at"][0], got["rhs_lo"][0]) == (0, -1.0)
    assert got["rhs_lo_at"][1] == -1 and np.isneginf(got["rhs_lo"][1])


def test_refusals_that_need_a_batch():
    import linearprogramming_amd as lpg
    from linearprogramming_amd import _lib as L
    lib = L.load()
    m, nc = 4, 9
    ident = np.arange(5, 9, dtype=np.int64)
    ip = np.tile(ident, 2).ctypes.data_as(L.c_int64_p)
    buf = [np.zeros(2 * nc) for _ in range(4)]

    def call(e, ip, **fields):
        out = L.RangingOut()
        for f, a in fields.items():
            setattr(out, f, a.ctypes.data_as(L.c_int64_p if a.dtype == np.int64 else L.c_double_p))
        rc_ = lib.lpg_batch_ranging(e._b, ip, out)
        return rc_, lib.lpg_batch_last_error(e._b).decode()

    with lpg.BatchEngine(2, m, nc) as e:
        e.generate(4)
        e.solve()
        code, msg = call(e, ip)                                                   # no group at all
        assert code == L.ERR_ARG and msg.startswith("lpg_batch_ranging:") and "none of dual" in msg
        code, msg = call(e, ip, cost_lo=buf[0], cost_hi=buf[1], cost_lo_at=buf[2].astype(np.int64))
        assert code == L.ERR_ARG and "3 of cost_lo, cost_hi, cost_lo_at, cost_hi_at" in msg
        code, msg = call(e, ip, dual=buf[0], rhs_hi=buf[1])
        assert code == L.ERR_ARG and "1 of rhs_lo, rhs_hi, rhs_lo_at, rhs_hi_at" in msg
        bad = np.tile(ident, 2)
        bad[6] = nc                                                               # row 2 of LP 1: one past the last column
        code, msg = call(e, bad.ctypes.data_as(L.c_int64_p), dual=buf[0])
        assert code == L.ERR_ARG and msg.startswith("lpg_batch_ranging:") and "row 2 of LP 1" in msg and "1..8" in msg
        with pytest.raises(lpg.LPGError, match="ident of shape"):
            e.ranging(ident[:3])
    with lpg.BatchEngine(2, m, nc, big_m=True) as e:
        code, msg = call(e, ip, dual=buf[0])
        assert code == L.ERR_STATE and msg.startswith("lpg_batch_ranging:") and "Big-M batch" in msg
        code, msg = call(e, ip)                                                   # the group rule before the kind
        assert code == L.ERR_ARG


def test_the_batch_is_unchanged_and_each_group_alone_gives_the_same_bits():
    cases = rc.CASES["artificial-8x8"]
    e, res, ident = rc.solved_engine(cases)
    try:
        before = rc.state_of(e, res)
        logs = [e.get_log(q) for q in range(e.count)]
        full = rc.device_ranging(e, ident)
        for group, fields in rc.GROUPS.items():
            want = {g: g == group for g in rc.GROUPS}
            r = e.ranging(np.array(ident), **want)
            alone = rc.device_ranging(e, ident, **want)
            assert sorted(alone) == sorted(fields)
            assert all(getattr(r, f) is None for f in rc.FIELDS if f not in fields)
            rc.assert_same(alone, full, fields)
        after = rc.state_of(e, res)
        for q in range(e.count):
            assert np.array_equal(rc.bits(before["rows"][q]), rc.bits(after["rows"][q]))
            assert np.array_equal(before["basis"][q], after["basis"][q])
            assert all(np.array_equal(a, b) for a, b in zip(logs[q], e.get_log(q)))
        assert before["nact"] == after["nact"]
        again = e.solve(rc.BUDGET)                            # finished LPs keep their results: nothing was reset
        assert [(r.status, r.pivots, r.objective) for r in again] == [(r.status, r.pivots, r.objective) for r in res]
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["dense", "artificial"])
def test_lpgcli_ranging_counts_and_digest_equal_pythons(kind):
    import linearprogramming_amd as lpg
    m = n = 8
    B, seed = 64, 20220518
    cli = os.path.join(ROOT, "host", "lpgcli")
    p = subprocess.run([cli, "--synthetic", str(m), str(n), "--batch", str(B), "--kind", kind, "--seed", str(seed), "--ranging"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])["ranging"]
    with lpg.BatchEngine(B, m, n + m + 1) as e:
        if kind == "artificial":
            res = e.solve_two_phase(e.generate_artificial(n, seed))
        else:
            e.generate(n, seed)
            res = e.solve()
        ident = [np.array([rc.tc.unit_column(m, n, i, 2 if kind == "artificial" else 0) for i in range(m)])] * B
        got = rc.device_ranging(e, ident)
    assert line["ranged"] == sum(r.status == rc.OPTIMAL for r in res) > 0
    for f in ("cost_lo", "cost_hi", "rhs_lo", "rhs_hi"):
        assert line["finite_" + f] == int(np.isfinite(got[f]).sum())
    assert line["digest"] == f"{rc.digest(got):016x}"


# ---------------------------------------------------------------------------
# frontend.sensitivity_batch
# ---------------------------------------------------------------------------
MODELS = ["testdata_max", "a3_min_eq_neg", "kat_min_ge", "kat_negative_rhs"]


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", "lp", name + ".txt"), encoding="utf-8") as f:
        return f.read()


def _moved(sm, i, delta):
    """sm with the standard-form right-hand side of row i moved by delta; a row whose right-hand side turns
    negative is stated negated, as standardization would have (it then lacks a basic column)."""
    s2 = copy.copy(sm)
    s2.rows = [list(r) for r in sm.rows]
    s2.rows[i][0] = sm.rows[i][0] + Fraction(delta)
    if s2.rows[i][0] < 0:
        s2.rows[i] = [-x for x in s2.rows[i]]
    return s2


@pytest.mark.parametrize("name", MODELS)
def test_sensitivity_batch_against_resolves_of_the_moved_model(name):
    from linearprogramming_amd import frontend as fe
    sm = fe.build_smatrix(_golden(name))
    base = fe.sensitivity_batch([sm])[0]
    plain = fe.solve_batch([sm])[0]
    for f in ("status", "pivots", "z", "columns", "variables", "method"):
        assert getattr(base, f) == getattr(plain, f), f
    assert base.status == "OPTIMAL"
    m = len(sm.rows)
    assert len(base.shadow) == len(base.rhs_range) == len(base.basis) == m
    assert list(base.cost_range) == sm.display_names
    moved, what = [], []
    for i, (lo, hi, _) in enumerate(base.rhs_range):
        b = float(sm.rows[i][0])
        assert lo <= b <= hi
        lo, hi = lo - b, hi - b
        delta = (lo + hi) / 2 if np.isfinite(lo) and np.isfinite(hi) else 1.0 if np.isinf(hi) else -1.0
        moved.append(_moved(sm, i, delta))
        what.append((i, delta, True))
        for end in (lo, hi):
            if np.isfinite(end) and end != 0:
                moved.append(_moved(sm, i, 2 * end))
                what.append((i, 2 * end, False))
    sols = fe.sensitivity_batch(moved)
    tol = 1e-9 * max(1.0, abs(base.z))
    for (i, delta, inside), sol in zip(what, sols):
        same = sol.status == "OPTIMAL" and sorted(sol.basis) == sorted(base.basis)
        print(name, "row", i, "delta", delta, "inside" if inside else "beyond", sol.status, "same basis" if same else "another")
        if inside:
            assert same, (i, delta, sol.status, sol.basis, base.basis)
            assert abs((sol.z - base.z) - base.shadow[i] * delta) <= tol, (i, delta, sol.z, base.z, base.shadow[i])
        else:
            assert not same, (i, delta)
