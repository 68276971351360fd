"""The 0-1 definition itself (tests/binary_cases.py enumerate01, the numpy
statement of include/lpg.h "0-1 programs") against brute force in the search
order and against scipy's MILP solver, the generator's planted points, the
front end's text handling with the device call stubbed by the statement, and a
census of the case list tests/test_gpu_binary.py runs. No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import binary_cases as bc

SHAPES = ((1, 1), (1, 2), (2, 3), (3, 5), (5, 7), (4, 10), (6, 12), (13, 12))


def small_problems():
    for m, n in SHAPES:
        for mx in (False, True):
            s = bc.spec(m, n, mx, seed=3)
            A, sense, rhs, c = bc.data_of(s)
            for q, kind in enumerate(s["kinds"]):
                yield f"{kind}-{m}x{n}-{'max' if mx else 'min'}", A[q], sense[q], rhs[q], c[q], mx


def test_the_statement_equals_brute_force_in_the_search_order():
    ties = infeasible = 0
    for what, A, sense, rhs, c, mx in small_problems():
        status, obj, x, nopt = bc.brute_force(A, sense, rhs, c, mx)
        r = bc.enumerate01(A, sense, rhs, c, mx)
        assert r["status"] == status, what
        assert (r["x"] == x).all(), (what, r["x"], x)
        if status == bc.OPTIMAL:
            assert r["objective"] == obj and np.signbit(r["objective"]) == np.signbit(obj), what
            assert r["objective"] == float(np.asarray(c) @ r["x"]), what
        else:
            assert np.isnan(r["objective"]) and r["found"] == 0, what
        ties += nopt >= 2
        infeasible += status == bc.INFEASIBLE
        for split in {1, min(3, len(c)), len(c) if len(c) <= 7 else 2}:
            rs = bc.enumerate_split(A, sense, rhs, c, mx, split)
            assert (rs["status"], rs["found"]) == (r["status"], r["found"]), (what, split)
            assert (rs["x"] == r["x"]).all(), (what, split)
            assert np.array([rs["objective"]]).view(np.uint64) == np.array([r["objective"]]).view(np.uint64), (what, split)
    assert ties >= 20 and infeasible >= 20          # the first-optimal-point rule and both ends were exercised


def test_budgeted_statement_is_a_prefix_of_the_unbudgeted_one():
    for what, A, sense, rhs, c, mx in small_problems():
        full = bc.enumerate01(A, sense, rhs, c, mx)
        for k in (1, 2, full["nodes"] - 1, full["nodes"], full["nodes"] + 1):
            if k < 1:
                continue
            cut = bc.enumerate01(A, sense, rhs, c, mx, max_nodes=k)
            if k >= full["nodes"]:
                assert cut["status"] == full["status"] and cut["nodes"] == full["nodes"], (what, k)
            else:
                assert cut["status"] == bc.ITER_LIMIT and cut["nodes"] == k, (what, k)
                if cut["found"] and full["found"]:
                    assert cut["inc"] >= full["inc"], (what, k)


def test_the_statement_equals_scipy_milp():
    opt = pytest.importorskip("scipy.optimize")
    if not hasattr(opt, "milp"):
        pytest.skip("this scipy has no milp")
    for what, A, sense, rhs, c, mx in small_problems():
        L, U = bc.bounds(sense, rhs)
        res = opt.milp(-c if mx else c, constraints=opt.LinearConstraint(A, L, U), integrality=np.ones(len(c)),
                       bounds=opt.Bounds(0, 1))
        r = bc.enumerate01(A, sense, rhs, c, mx)
        assert (res.status == 0) == (r["status"] == bc.OPTIMAL), (what, res.status, res.message)
        if r["status"] == bc.OPTIMAL:
            assert round(-res.fun if mx else res.fun) == r["objective"], what


@pytest.mark.parametrize("m,n", [(1, 1), (1, 2), (2, 1), (5, 3), (7, 4), (16, 64), (256, 64), (63, 64), (40, 9)])
def test_generated_problems_are_feasible_at_their_planted_point(m, n):
    for key in (20220518, 7, (1 << 64) - 1):
        A, sense, rhs, c, xp = bc.generate(m, n, key)
        L, U = bc.bounds(sense, rhs)
        act = A @ xp
        assert ((L <= act) & (act <= U)).all()
        assert (np.count_nonzero(A, axis=1) <= 3).all() and np.abs(A).max() <= 4 and np.abs(c).max() <= 9
        assert (A == np.floor(A)).all() and (c == np.floor(c)).all()
        for i in range(m):                                   # the band: consecutive columns from floor(i (n - 3) / (m - 1))
            nz = np.flatnonzero(A[i])
            s = (i * (n - 3)) // (m - 1) if (m > 1 and n > 3) else 0
            assert nz.size == 0 or (s <= nz.min() and nz.max() < s + min(3, n))
    if m >= 40:
        kinds = np.bincount(bc.generate(m, n, 1)[1] + 1, minlength=3)
        assert kinds[1] > m // 4 and kinds[0] > 0 and kinds[2] > 0       # about half equalities, both one-sided kinds


# ---- the front end's text handling, the device call stubbed by the statement --

def _stub(calls):
    def batch(A, sense, rhs, c, maximize, split, max_nodes, device):
        calls.append((A.copy(), sense.copy(), rhs.copy(), c.copy(), maximize))
        refs = [bc.enumerate_split(A[q], sense[q], rhs[q], c[q], maximize, split or 0, max_nodes) for q in range(len(A))]
        return [(r["status"], r["found"], r["nodes"], r["objective"]) for r in refs], np.stack([r["x"] for r in refs])
    return batch


def _text(of, st):
    return "OF {\n\t%s\n}\nST {\n\t%s\n}\n" % (of, ";\n\t".join(st))


def test_text_rows_are_scaled_and_strict_relations_tightened(monkeypatch):
    from linearprogramming_amd import frontend
    text = _text("max:z=1/2x1+1/3x2+x3", ["1/2x1+1/4x2+x3<3/2", "x1+x2>1", "x1>=0", "x2+x3=1", "3x1-2x3>=-1", "x2+x3<=3/2"])
    A, sense, rhs, c, mx, names, scale, offset = frontend.binary_model(text)
    assert names == ["x1", "x2", "x3"] and mx and scale == 6 and offset == 0
    assert (c == [3, 2, 6]).all()
    assert (A == [[2, 1, 4], [1, 1, 0], [0, 1, 1], [3, 0, -2], [0, 2, 2]]).all()
    assert (sense == [-1, 1, 0, 1, -1]).all()
    assert (rhs == [5, 2, 1, -1, 3]).all()        # < 6 is <= 5, > 1 is >= 2; x1 >= 0 is no row
    calls = []
    monkeypatch.setattr(frontend, "_binary_batch", _stub(calls))
    sol = frontend.solve_binary_text(text)
    # x1 = x2 = 1 by row 1, then x3 = 0 by row 2: the only feasible point
    assert sol.status == "OPTIMAL" and sol.names == names and (sol.x == [1, 1, 0]).all()
    assert sol.objective == 5 / 6                            # the model's own scale
    # order="cost": the device saw the columns by descending |c|: x3, x1, x2
    assert (calls[0][3] == [[6, 3, 2]]).all() and (calls[0][0][0, 0] == [4, 2, 1]).all()


def test_text_minimisation_with_a_constant_and_an_infeasible_model(monkeypatch):
    from linearprogramming_amd import frontend
    monkeypatch.setattr(frontend, "_binary_batch", _stub([]))
    sol = frontend.solve_binary_text(_text("min:z=3x1+2x2+4x3+5", ["2x1+2x2+2x3>=3", "x1+x3<=1"]))
    assert sol.status == "OPTIMAL" and (sol.x == [1, 1, 0]).all() and sol.objective == 10.0
    sol = frontend.solve_binary_text(_text("min:z=x1+x2", ["x1+x2>2"]))
    assert sol.status == "INFEASIBLE" and np.isnan(sol.objective) and (sol.x == -1).all()
    with pytest.raises(frontend.FrontendError, match="x2 <= 0"):
        frontend.solve_binary_text(_text("min:z=x1+x2", ["x1+x2>=1", "x2<=0"]))


def test_solve_binary_groups_by_shape_orders_by_cost_and_maps_x_back(monkeypatch):
    from linearprogramming_amd import frontend
    calls = []
    monkeypatch.setattr(frontend, "_binary_batch", _stub(calls))
    rng = np.random.default_rng(11)
    shapes = [(3, 5), (4, 6), (3, 5), (2, 2), (4, 6)]
    models = [bc.problem("mixed", m, n, rng) for m, n in shapes]
    for order in ("cost", None):
        calls.clear()
        sols = frontend.solve_binary(models, order=order)
        assert sorted(c[0].shape for c in calls) == [(1, 2, 2), (2, 3, 5), (2, 4, 6)]
        for (A, sense, rhs, c), sol in zip(models, sols):
            status, obj, x, _ = bc.brute_force(A, sense, rhs, c)
            assert sol.status == ("OPTIMAL" if status == bc.OPTIMAL else "INFEASIBLE")
            if status == bc.OPTIMAL:
                assert sol.objective == obj and float(c @ sol.x) == obj
                L, U = bc.bounds(sense, rhs)
                assert ((L <= A @ sol.x) & (A @ sol.x <= U)).all()
            if order is None:
                assert (sol.x == x).all()
    assert (frontend.binary_order([1, -5, 5, 0, 2], "cost") == [1, 2, 4, 0, 3]).all()
    with pytest.raises(frontend.FrontendError, match="order"):
        frontend.solve_binary(models, order="weight")


# ---- the census of the GPU test's case list -----------------------------------

def test_census_of_the_gpu_cases():
    """What tests/test_gpu_binary.py must have run, so that its list cannot hide a failure; and every unbudgeted
    case ends in the statement within 20,000 nodes (a condition on the inputs: the GPU test has no budget there)."""
    ms, ns, counts = set(), set(), set()
    tied = inf_row = inf_combo = first = 0
    for s in bc.UNBUDGETED:
        refs = bc.reference(s)
        A, sense, rhs, c = bc.data_of(s)
        ms.add(s["shape"][0])
        ns.add(s["shape"][1])
        counts.add(len(refs))
        for q, (kind, r) in enumerate(zip(s["kinds"], refs)):
            assert r["status"] in (bc.OPTIMAL, bc.INFEASIBLE), (bc.name(s), q)
            assert r["nodes"] <= 20000 * (1 << s["split"]), (bc.name(s), q, r["nodes"])
            one = bc.enumerate01(A[q], sense[q], rhs[q], c[q], s["maximize"]) if s["split"] else r
            assert one["nodes"] <= 20000, (bc.name(s), q)
            inf_row += kind == "inf_row" and r["status"] == bc.INFEASIBLE
            inf_combo += kind == "inf_combo" and r["status"] == bc.INFEASIBLE and s["shape"][0] >= 2
            first += r["nodes"] == 1 and r["status"] == bc.OPTIMAL and s["split"] == 0
            if s["shape"][1] <= 12 and r["status"] == bc.OPTIMAL:
                tied += bc.brute_force(A[q], sense[q], rhs[q], c[q], s["maximize"])[3] >= 2
    assert ms >= {1, 63, 64, 65, 128, 129, 256}
    assert ns >= {1, 2, 31, 32, 33, 63, 64}
    assert counts >= {1, 5, 131} and all(k % 4 for k in counts)
    assert tied >= 10 and inf_row >= 10 and inf_combo >= 10 and first >= 10
    # an infeasible-in-combination problem passes each row's own test at the root
    s = bc.spec(5, 7, kinds=("inf_combo",))
    A, sense, rhs, c = bc.data_of(s)
    L, U = bc.bounds(sense[0], rhs[0])
    assert ((np.minimum(0, A[0]).sum(axis=1) <= U) & (np.maximum(0, A[0]).sum(axis=1) >= L)).all()
    assert bc.reference(s)[0]["status"] == bc.INFEASIBLE and bc.reference(s)[0]["nodes"] > 1
    # searches that outlast the default chunk, so that a solve makes several launches
    assert all(max(r["nodes"] for r in bc.reference(s)) > 2 * 4096 for s in bc.DEEP)
    # budgets: a cut with no incumbent and a cut with one, and later steps that still run
    with_inc = without = 0
    for s in bc.BUDGETED:
        used = 0
        for step in bc.BUDGET_STEPS[:-1]:
            used += step
            for r in bc.reference(s, used):
                with_inc += r["status"] == bc.ITER_LIMIT and r["found"] == 1
                without += r["status"] == bc.ITER_LIMIT and r["found"] == 0
    assert with_inc >= 3 and without >= 3
    for s in bc.CUT_ONLY:
        refs = bc.reference(s, s["budgets"][0])
        assert all(r["status"] == bc.ITER_LIMIT and r["nodes"] == s["budgets"][0] for r in refs)
        assert any(r["found"] for r in refs)
