"""Scenarios on the device (include/lpg.h, "scenarios") against their numpy
statement and the CPU oracle (tests/scenario_cases.py), bit for bit: the
children lpg_batch_scenario makes, their re-solve by solve_dual, set_rhs on the
solved children and the solve after it, the parent left alone, the host
refusals that need a parent batch, and frontend.solve_scenarios against a CPU
walk of the same steps."""
from __future__ import annotations

import os

import numpy as np
import pytest

import batch_cases as bc
import scenario_cases as sc

pytestmark = pytest.mark.gpu

# (kind, m, n): ncols = n + m + 1
SHAPES = [("dense", 8, 8), ("dense", 5, 7), ("dense", 16, 12), ("art", 8, 8), ("art", 16, 16)]


def _check(s, got):
    want = sc.expected(s, got)
    assert got["1/built/src"].size > 0
    for level in (1, 2) if s["second"] else (1,):
        sc.assert_stage(got, want, level)
    # the parent read back after scenario() is the parent read back before it
    assert np.array_equal(bc.bits(got["after/rows"]), bc.bits(got["parent/rows"]))
    return want


@pytest.mark.parametrize("kind,m,n", SHAPES)
def test_children_their_resolve_and_set_rhs_equal_numpy_and_the_oracle(kind, m, n):
    """Every LP of a batch of 2 under the recipe's 8 scenarios; then set_rhs with the second draw on the solved
    children, INFEASIBLE ones included, and solve_dual again."""
    s = sc.spec(kind, m, n, B=2, second=True)
    got = sc.run_batch(s)
    assert (got["parent/status"] == sc.OPTIMAL).all()
    assert np.array_equal(got["1/built/src"], np.repeat([0, 1], 8))
    _check(s, got)
    nc = n + m + 1
    assert (got["1/built/ncols"] == nc).all() and (got["1/built/m"] == m).all()
    assert np.array_equal(got["1/built/nact"], got["parent/nact"][got["1/built/src"]])
    assert (got["1/built/ld"] == got["parent/ld"][0]).all()
    st, pv = got["1/solved/status"], got["1/solved/pivots"]
    assert set(st.tolist()) == {sc.OPTIMAL, sc.INFEASIBLE}
    assert pv[0] == 0 and pv[8] == 0                         # scenario 0 is the LP's own right-hand side
    if kind == "dense":
        assert st[7] == st[15] == sc.INFEASIBLE and (pv > 0).any()
    else:
        assert (got["1/built/ncols"] > got["1/built/nact"] + 1).all()      # the inert artificial columns came along
        assert (st[:8] == sc.INFEASIBLE).sum() == {8: 2, 16: 4}[m]


def test_n_differs_from_count_with_src_repeating_and_descending():
    s = sc.spec("dense", 8, 8, B=3, pattern="repeat")
    got = sc.run_batch(s)
    src = got["1/built/src"]
    assert src.size != s["B"] and (np.diff(src[:3]) < 0).all() and len(set(src.tolist())) < src.size
    _check(s, got)


@pytest.mark.parametrize("kind,lps", [("ragged", [[8, 8], [5, 7], [16, 12]]), ("ragged_art", [[8, 8], [16, 16]])])
def test_ragged_parent_gives_a_ragged_child(kind, lps):
    s = sc.spec(kind, lps=lps, second=True)
    got = sc.run_batch(s)
    src = got["1/built/src"]
    assert (got["parent/status"] == sc.OPTIMAL).all()
    assert np.array_equal(got["1/built/m"], got["parent/m"][src]) and np.array_equal(got["1/built/ncols"], got["parent/ncols"][src])
    assert np.array_equal(got["1/built/art_first"], got["parent/art_first"][src])
    if kind == "ragged_art":
        assert np.array_equal(got["parent/art_first"], [sc.br.art_first_of(m, n) for m, n in lps])
    _check(s, got)


def test_more_rows_than_a_workgroup_has_threads():
    s = sc.spec("dense", 260, 3, B=1, nscen=4)
    got = sc.run_batch(s)
    assert got["parent/status"][0] == sc.OPTIMAL and got["parent/nact"][0] % 2 == 1
    _check(s, got)
    assert got["1/solved/pivots"].tolist() == [0, 3, 1, 7]


def test_an_lp_whose_staging_needs_more_than_64_kib_of_lds():
    """m = 5500: ident and rhs take 66000 bytes of dynamic LDS, above the limit a kernel has without asking for
    more. A loaded identity frame with a row of twos as the objective: scenario() and set_rhs against rhs_column."""
    import linearprogramming_amd as lpg
    m = 5500
    T = np.zeros((1, m + 1, m + 2))
    T[0, np.arange(m), 1 + np.arange(m)] = 1.0
    T[0, m, 1:m + 1] = 2.0
    T[0, :m, m + 1] = 0.5
    ident = 1 + np.arange(m)
    rhs = np.random.default_rng(11).random((2, m))
    with lpg.BatchEngine(1, m, m + 2) as e:
        e.load(T, ident[None])
        with e.scenario([0], rhs[:1], ident) as ch:
            want = T[0].copy()
            want[:, 0] = sc.rhs_column(T[0], ident, rhs[0])
            assert np.array_equal(bc.bits(ch.get_rows()[0]), bc.bits(want))
            ch.set_rhs(rhs[1:], ident)
            want[:, 0] = sc.rhs_column(T[0], ident, rhs[1])
            assert np.array_equal(bc.bits(ch.get_rows()[0]), bc.bits(want))
            assert np.array_equal(ch.get_basis()[0], ident)


@pytest.mark.parametrize("env", [{"LPG_BATCH_TIER": "global"}, {"LPG_SCENARIO_WALK": "tile"}])
def test_forced_to_the_global_tier_and_with_the_other_walk(env, tmp_path):
    specs = [sc.spec("dense", 8, 8, second=True), sc.spec("art", 8, 8, second=True)]
    if "LPG_SCENARIO_WALK" in env:
        specs.append(sc.spec("dense", 260, 3, B=1, nscen=4))
    for s, got in zip(specs, sc.in_subprocess(specs, env, tmp_path)):
        if "LPG_BATCH_TIER" in env:
            assert (got["parent/tier"] == 1).all() and (got["1/built/tier"] == 1).all()
        _check(s, got)


# ---------------------------------------------------------------------------
# the host refusals that need a parent batch (tests/test_batch_scenario_abi.py has the others)
# ---------------------------------------------------------------------------
def test_refusals_name_the_index_and_leave_the_parent_alone():
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(3, 4, 9)
    g = lpg.BatchEngine.ragged([(4, 9), (2, 5)])
    bm = lpg.BatchEngine(2, 4, 9, big_m=True)
    try:
        e.generate(4, bc.SEED, 0)
        before = bc.bits(e.get_rows()).copy()
        ident, rhs = np.arange(5, 9), np.ones((2, 4))
        with pytest.raises(lpg.LPGError, match=r"lpg_batch_scenario rc=-4.*Big-M"):
            bm.scenario([0], np.ones((1, 4)), ident)
        with pytest.raises(lpg.LPGError, match=r"lpg_batch_set_rhs rc=-4.*Big-M"):
            bm.set_rhs(np.ones((2, 4)), ident)
        with pytest.raises(lpg.LPGError, match=r"rc=-1: lpg_batch_scenario: src\[1\] = 3 outside"):
            e.scenario([0, 3], rhs, ident)
        with pytest.raises(lpg.LPGError, match=r"rc=-1: lpg_batch_scenario: src\[0\] = -1 outside"):
            e.scenario([-1, 0], rhs, ident)
        bad = np.tile(ident, (3, 1))
        bad[1, 2] = 9
        with pytest.raises(lpg.LPGError, match=r"rc=-1: lpg_batch_scenario: ident\[6\] = 9 \(row 2 of LP 1\) outside the columns 1\.\.8"):
            e.scenario([0, 0], rhs, bad)
        bad[1, 2], bad[0, 3] = 7, 0
        with pytest.raises(lpg.LPGError, match=r"rc=-1: lpg_batch_set_rhs: ident\[3\] = 0 \(row 3 of LP 0\)"):
            e.set_rhs(np.ones((3, 4)), bad)
        with pytest.raises(lpg.LPGError, match=r"rc=-1: lpg_batch_scenario: ident\[5\] = 5 \(row 1 of LP 1\) outside the columns 1\.\.4"):
            g.scenario([0], [np.ones(4)], [ident, np.array([3, 5])])
        for x in (float("nan"), float("inf")):
            r = rhs.copy()
            r[1, 2] = x
            with pytest.raises(lpg.LPGError, match=r"rc=-1: lpg_batch_scenario: rhs\[6\] = .*\(row 2 of child 1\) is not finite"):
                e.scenario([2, 0], r, ident)
        r = np.ones((3, 4))
        r[2, 0] = float("nan")
        with pytest.raises(lpg.LPGError, match=r"rc=-1: lpg_batch_set_rhs: rhs\[8\] = .*\(row 0 of LP 2\) is not finite"):
            e.set_rhs(r, ident)
        with pytest.raises(lpg.LPGError, match=r"rc=-1: lpg_batch_scenario: n = 0"):
            e.scenario([], np.ones((0, 4)), ident)
        with pytest.raises(lpg.LPGError, match=r"rhs of shape \(2, 3\)"):
            e.scenario([0, 0], np.ones((2, 3)), ident)
        assert np.array_equal(bc.bits(e.get_rows()), before)
    finally:
        for x in (e, g, bm):
            x.close()


# ---------------------------------------------------------------------------
# the front end
# ---------------------------------------------------------------------------
def _golden(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lp", name + ".txt"), encoding="utf-8") as f:
        return f.read()


def _variants(text, swaps):
    """The text, and one more per entry of swaps: every (old, new) of it replaced once."""
    out = [text]
    for sw in swaps:
        t = text
        for old, new in sw:
            assert t.count(old) == 1
            t = t.replace(old, new)
        out.append(t)
    return out


MODELS = {
    "kat_wyndor": [[("x1<=4", "x1<=3"), ("2x2<=12", "2x2<=8")], [("3x1+2x2<=18", "3x1+2x2<=6"), ("x1<=4", "x1<=5")]],
    "a3_min_eq_neg": [[("x1+x2+x3>=4", "x1+x2+x3>=6"), ("2x1-x2=1", "2x1-x2=3")], [("x1+3x3<=9", "x1+3x3<=2"), ("2x1-x2=1", "2x1-x2=5")]],
}


def _cpu_walk(texts):
    """solve_scenarios' steps on the CPU: the first model's root on the oracle (tests/cut_cases.py root_of), column
    0 restated by rhs_column per model, the oracle's dual simplex, frontend._readout."""
    import cut_cases as cc
    from linearprogramming_amd import frontend as F
    _, _, (T, basis, nact, _), r = cc.root_of(texts[0])
    assert r.status == sc.OPTIMAL
    out = []
    for t in texts:
        sm = F.build_smatrix(t)
        rows, ident, _, _, _ = F.engine_arrays(sm)
        x = sc.br.oracle_dual(*sc.child_of(T, basis, nact, ident, rows[:, 0]), 1 << 40)
        sol = F.LPSolution(sc.br.bc_status(x["status"][0]), int(x["pivots"][0]), method="scenario_dual")
        if sol.status == "OPTIMAL":
            F._readout(sm, sol, float(x["objective"][0]), x["rows"][0][:-1, 0], x["basis"][0], T.shape[1])
        out.append(sol)
    return out


@pytest.mark.parametrize("name", sorted(MODELS))
def test_solve_scenarios_equals_the_cpu_walk_and_solve(name):
    from linearprogramming_amd import frontend as F
    texts = _variants(_golden(name), MODELS[name])
    sms = [F.build_smatrix(t) for t in texts]
    sols = F.solve_scenarios(sms)
    assert len(sols) == 3
    for sol, ref, sm in zip(sols, _cpu_walk(texts), sms):
        cold = F.solve(sm)
        assert sol.status == cold.status == ref.status == "OPTIMAL"
        assert (sol.pivots, sol.method) == (ref.pivots, "scenario_dual")
        assert bc.bits(sol.z) == bc.bits(ref.z) and abs(sol.z - cold.z) < 1e-9
        for got, want in ((sol.columns, ref.columns), (sol.variables, ref.variables)):
            assert got.keys() == want.keys()
            for k, v in want.items():
                assert bc.bits(got[k]) == bc.bits(v), k
    assert sols[0].pivots == 0 and any(s.pivots > 0 for s in sols)


def test_solve_scenarios_refuses_a_model_that_differs_in_a_coefficient():
    from linearprogramming_amd import frontend as F
    text = _golden("kat_wyndor")
    sms = [F.build_smatrix(t) for t in (text, text.replace("2x2<=12", "2x2<=8"), text.replace("3x1+2x2<=18", "3x1+4x2<=18"))]
    with pytest.raises(F.FrontendError, match="model 2 differs"):
        F.solve_scenarios(sms)
