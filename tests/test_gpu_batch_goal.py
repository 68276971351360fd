"""lpg_batch_solve_goal on the device: goal batches, (m+K) x ncols tableaus with
the objective row of priority level k in row m + k, priced by class
(linearprogramming_amd/csrc/lpg_batch.hip k_batch_goal, batch_price_goal), bit
for bit against the statement of include/lpg.h restated over the CPU oracle
(tests/goal_cases.py): the status after every call, pivot count, objective and
attain bits, last (entering, leaving), basis, the whole log and the whole
(m+K) x ncols tableau, no tolerance anywhere. A case counts only if the
statement shows the property it is there for; that is asserted on the
statement's result.
"""
from __future__ import annotations

import ctypes
import json

import numpy as np
import pytest

import batch3_cases as b3
import batch_cases as bc
import goal_cases as gc
from goal_cases import ITER_LIMIT, NUMERIC, OPTIMAL, UNBOUNDED, graded_spec, spec
from oracle.lpo import RULE_BLAND, RULE_DANTZIG, Oracle

pytestmark = pytest.mark.gpu

TIER_LDS, TIER_GLOBAL = 0, 1
RULES = [RULE_DANTZIG, RULE_BLAND]

_statement_cache, _device_cache = {}, {}


def statement_of(s):
    """run_statement(s), computed once per distinct case and shared (never modified)."""
    key = json.dumps(s, sort_keys=True)
    if key not in _statement_cache:
        _statement_cache[key] = gc.run_statement(s)
    return _statement_cache[key]


def device_of(s):
    key = json.dumps(s, sort_keys=True)
    if key not in _device_cache:
        _device_cache[key] = gc.run_batch(s)
    return _device_cache[key]


def check(s, tier=None, nonfinite=False):
    got, want = device_of(s), statement_of(s)
    if tier is not None:
        assert int(got["tier"]) == tier
    assert int(got["nobj"]) == want["attain"].shape[1] and got["rows"].shape == want["rows"].shape
    gc.assert_same(got, want, nonfinite)
    return got, want


def graded_specs():
    return [graded_spec(h, g, n, K, B, seed, rule=rule) for h, g, n, K, B, seed in gc.GRADED for rule in RULES]


# ---- the literals ---------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
def test_textbook(rule):
    got, want = check(spec("textbook", B=4, rule=rule), TIER_LDS)
    assert got["rows"].shape == (4, 7, 10) and (want["status"] == OPTIMAL).all()
    if rule == RULE_DANTZIG:
        assert (want["pivots"] == 2).all() and want["logk"][:2].tolist() == [2, 1]
    x = np.zeros((4, 10))
    for b in range(4):
        x[b, got["basis"][b]] = got["rows"][b, :4, 0]
    assert np.array_equal(x[:, 1:3], [[2.0, 4.0]] * 4) and np.array_equal(got["attain"], np.zeros((4, 3)))


@pytest.mark.parametrize("rule", RULES)
def test_ladder_ranks_class_before_value(rule):
    got, want = check(spec("ladder", B=2, rule=rule), TIER_LDS)
    assert got["rows"].shape == (2, 24, 33) and (want["status"] == OPTIMAL).all()
    assert want["logk"].tolist() == list(range(1, 9)) * 2          # the columns in level order, x_8's |d| the largest
    assert np.array_equal(got["attain"], np.zeros((2, 8)))


# ---- the graded cases of the census: every class, ties, the blocking arm ----------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("h,g,n,K,B,seed", gc.GRADED)
def test_graded_cases(h, g, n, K, B, seed, rule):
    got, want = check(graded_spec(h, g, n, K, B, seed, rule=rule), TIER_LDS)
    assert (want["status"] == OPTIMAL).all() and want["pivots"].min() >= 1


def test_graded_cases_on_the_global_tier(tmp_path):
    specs = graded_specs()
    for s, got in zip(specs, bc.in_subprocess("goal_cases", specs, {"LPG_BATCH_TIER": "global"}, tmp_path)):
        assert int(got["tier"]) == TIER_GLOBAL
        gc.assert_same(got, statement_of(s))


@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_graded_cases_at_small_chunks(chunk, tmp_path):
    specs = graded_specs()
    for s, got in zip(specs, bc.in_subprocess("goal_cases", specs, {"LPG_BATCH_CHUNK": str(chunk)}, tmp_path)):
        assert int(got["chunk"]) == chunk
        gc.assert_same(got, statement_of(s))


# ---- K = 1 and K = 2 against the oracle's own solvers ------------------------------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("m,n", [(8, 8), (37, 70)])
def test_two_levels_are_big_m(m, n, rule):
    s = spec("artificial", B=4, rule=rule, m=m, n=n, K=2, seed=bc.SEED, budgets=[50 * (m + n)])
    got, _ = check(s, TIER_LDS)
    A, basis, costs, af = gc.artificial(m, n, 2, 4, bc.SEED)
    for b in range(4):
        o = Oracle(m, n + m + 1, nobj=2)
        T = np.zeros((m + 2, n + m + 1))
        T[:m] = A[b]
        o.load_tableau(T, basis[b])
        r = o.solve_big_m(af, np.append(costs[b, 1], 0.0), 50 * (m + n), rule)
        # Big-M's INFEASIBLE is the statement's OPTIMAL / UNBOUNDED with the artificial level still negative
        assert got["status"][b] == r.status or (r.status == b3.INFEASIBLE and got["status"][b] in (OPTIMAL, UNBOUNDED))
        assert got["pivots"][b] == r.pivots and (got["entering"][b], got["leaving"][b]) == (r.entering, r.leaving)
        assert np.array_equal(bc.bits(got["rows"][b]), bc.bits(o.get_rows())) and np.array_equal(got["basis"][b], o.get_basis())
        o.close()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("m,n", [(8, 8), (37, 70)])
def test_one_level_is_the_primal_simplex(m, n, rule):
    s = spec("artificial", B=4, rule=rule, m=m, n=n, K=1, seed=bc.SEED, budgets=[50 * (m + n)])
    got, _ = check(s, TIER_LDS)
    A, basis, costs, _ = gc.artificial(m, n, 1, 4, bc.SEED)
    for b in range(4):
        o = Oracle(m, n + m + 1)
        T = np.zeros((m + 1, n + m + 1))
        T[:m] = A[b]
        o.load_tableau(T, basis[b])
        o.set_objective(np.append(costs[b, 0], 0.0))
        r = o.solve(50 * (m + n), rule)
        assert (got["status"][b], got["pivots"][b], got["entering"][b], got["leaving"][b]) == \
            (r.status, r.pivots, r.entering, r.leaving)
        assert np.array_equal(bc.bits(got["rows"][b]), bc.bits(o.get_rows())) and np.array_equal(got["basis"][b], o.get_basis())
        o.close()


# ---- budgets ---------------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
def test_budgets(rule):
    h, g, n, K, _, seed = gc.GRADED[1]
    base = graded_spec(h, g, n, K, 16, seed, rule=rule, only=3)
    p = int(statement_of(base)["pivots"][0])
    assert p >= 4
    for budgets, status, pivots in (([0], ITER_LIMIT, 0), ([p], OPTIMAL, p), ([p - 1], ITER_LIMIT, p - 1),
                                    ([p // 2, 100000], OPTIMAL, None)):
        got, want = check({**base, "budgets": budgets})
        assert want["status"][0] == status and (pivots is None or want["pivots"][0] == pivots)
        if len(budgets) == 2:
            assert want["calls"][:, 0].tolist() == [ITER_LIMIT, OPTIMAL] and want["pivots"][0] >= p // 2


# ---- pricing edges, statuses -------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
def test_pricing_edges(rule):
    names, _, _, _ = gc.edges()
    got, want = check(spec("edges", B=len(names), rule=rule, budgets=[1]), TIER_LDS, nonfinite=True)
    first = dict(zip(names, np.where(want["pivots"] > 0, want["entering"], -1).tolist()))
    assert first["minus_eps_not_eligible"] == -1 and first["below_minus_eps_eligible"] == 2
    assert first["plus_eps_does_not_block"] == 1 and first["above_plus_eps_blocks"] == -1
    assert first["nan_and_inf_block"] == -1 and first["nan_below_the_class_is_ignored"] == 3
    assert first["blocked_at_the_second_level"] == 2
    if rule == RULE_DANTZIG:
        assert first["minus_inf_wins_its_class"] == 3 and first["class_before_value"] == 4
    else:
        assert first["minus_inf_wins_its_class"] == 1 and first["class_before_value"] == 1


@pytest.mark.parametrize("rule", RULES)
def test_unbounded_and_numeric(rule):
    got, want = check(spec("statuses", B=3, rule=rule), TIER_LDS, nonfinite=True)
    assert want["status"].tolist() == [UNBOUNDED, NUMERIC, OPTIMAL]
    if rule == RULE_DANTZIG:
        assert want["pivots"][0] == 1          # level 0 was optimal first: the ray is found at level 1


# ---- the tier boundary ---------------------------------------------------------------

@pytest.mark.parametrize("K", [3, 8])
def test_tier_boundary(K):
    g = gc.boundary_goals(K)
    assert gc.lds_bytes(2 + g, 11 + 2 * g, K) <= 150 * 1024 < gc.lds_bytes(3 + g, 13 + 2 * g, K)
    for goals, tier in ((g, TIER_LDS), (g + 1, TIER_GLOBAL)):
        got, want = check(graded_spec(2, goals, 8, K, 2, 100, budgets=[40]), tier)
        assert want["pivots"].max() <= 40 and set(want["status"].tolist()) <= {ITER_LIMIT, OPTIMAL}


# ---- the kinds are kept apart ----------------------------------------------------------

def _guard_calls(lpg, e):
    """Every lpg_batch_* call that a goal batch refuses, with arguments that pass the checks in front of the kind's."""
    L = lpg._lib
    lib, b = e.lib, e._b
    res = (L.Result * e.count)()
    i64 = np.zeros(4 * e.m * e.count + 8, dtype=np.int64)
    i64[:] = 1
    f64 = np.zeros(e.count * e.ncols * (e.m + 8))
    u8 = np.ones(e.ncols * e.count, dtype=np.uint8)
    i8 = np.ones(4, dtype=np.int8)
    ip, dp = i64.ctypes.data_as(L.c_int64_p), f64.ctypes.data_as(L.c_double_p)
    up, i8p = u8.ctypes.data_as(L.c_uint8_p), i8.ctypes.data_as(L.c_int8_p)
    child = ctypes.c_void_p()
    first = np.array([0, 1, 2], dtype=np.int64)
    rng = L.RangingOut()
    rng.dual = dp
    br = (L.Branch * e.count)()
    keep = (i64, f64, u8, i8, first)
    return keep, child, [
        ("lpg_batch_solve", lambda: lib.lpg_batch_solve(b, 10, 0, res)),
        ("lpg_batch_solve_dual", lambda: lib.lpg_batch_solve_dual(b, 10, res)),
        ("lpg_batch_solve_two_phase", lambda: lib.lpg_batch_solve_two_phase(b, 2, None, 0, 10, 0, res)),
        ("lpg_batch_solve_big_m", lambda: lib.lpg_batch_solve_big_m(b, 2, None, 0, 10, 0, res)),
        ("lpg_batch_generate", lambda: lib.lpg_batch_generate(b, 1, 1, 0)),
        ("lpg_batch_generate_artificial", lambda: lib.lpg_batch_generate_artificial(b, 1, 1, None)),
        ("lpg_batch_set_objective", lambda: lib.lpg_batch_set_objective(b, dp, e.ncols)),
        ("lpg_batch_set_active_columns", lambda: lib.lpg_batch_set_active_columns(b, 1)),
        ("lpg_batch_branch_select", lambda: lib.lpg_batch_branch_select(b, up, 1, 0, 1e-6, 0, br)),
        ("lpg_batch_branch", lambda: lib.lpg_batch_branch(ctypes.byref(child), b, 1, ip, ip, i8p)),
        ("lpg_batch_cut_select", lambda: lib.lpg_batch_cut_select(b, up, 1, 0, 1e-6, 1, ip, ip)),
        ("lpg_batch_cut", lambda: lib.lpg_batch_cut(ctypes.byref(child), b, 1, ip, first.ctypes.data_as(L.c_int64_p), ip, up, 1, 0)),
        ("lpg_batch_scenario", lambda: lib.lpg_batch_scenario(ctypes.byref(child), b, 1, ip, ip, dp)),
        ("lpg_batch_set_rhs", lambda: lib.lpg_batch_set_rhs(b, ip, dp)),
        ("lpg_batch_ranging", lambda: lib.lpg_batch_ranging(b, ip, ctypes.byref(rng))),
        ("lpg_batch_load_packed", lambda: lib.lpg_batch_load_packed(b, 0, 1, dp, None)),
        ("lpg_batch_get_rows_packed", lambda: lib.lpg_batch_get_rows_packed(b, 0, 1, dp)),
        ("lpg_batch_get_basis_packed", lambda: lib.lpg_batch_get_basis_packed(b, 0, 1, ip)),
        ("lpg_batch_set_objective_packed", lambda: lib.lpg_batch_set_objective_packed(b, dp)),
        ("lpg_batch_solve_two_phase_ragged", lambda: lib.lpg_batch_solve_two_phase_ragged(b, ip, None, 10, 0, res)),
        ("lpg_batch_solve_big_m_ragged", lambda: lib.lpg_batch_solve_big_m_ragged(b, ip, None, 10, 0, res)),
    ]


@pytest.mark.parametrize("K", [1, 2, 3])
def test_every_other_call_refuses_a_goal_batch(K):
    import linearprogramming_amd as lpg
    A, basis, costs = gc.textbook()
    T = np.zeros((2, 4 + K, 10))
    T[:, :4] = A
    with lpg.BatchEngine(2, 4, 10, levels=K) as e:
        e.load(T, np.array([basis, basis]))
        assert e.info.nobj == K
        keep, child, calls = _guard_calls(lpg, e)
        for name, call in calls:
            assert call() == lpg._lib.ERR_STATE, name
            msg = e.lib.lpg_batch_last_error(e._b).decode()
            assert msg.startswith(name + ":") and "lpg_batch_solve_goal" in msg and "goal batch" in msg, msg
            assert not child.value
        # nothing has moved or pivoted
        assert np.array_equal(e.get_rows(), T) and np.array_equal(e.get_basis(), [basis, basis])
        res, attain = e.solve_goal(costs[:K], 100)
        assert all(r.status == OPTIMAL for r in res) and attain.shape == (2, K)
        del keep


def test_solve_goal_refuses_plain_and_big_m_batches():
    import linearprogramming_amd as lpg
    A, basis, costs = gc.textbook()
    for big_m, word in ((False, "lpg_batch_create_goal"), (True, "Big-M batch")):
        nobj = 2 if big_m else 1
        T = np.zeros((2, 4 + nobj, 10))
        T[:, :4] = A
        with lpg.BatchEngine(2, 4, 10, big_m=big_m) as e:
            e.load(T, np.array([basis, basis]))
            with pytest.raises(lpg.LPGError, match=f"lpg_batch_solve_goal rc=-4.*{word}.*nothing has"):
                e.solve_goal(costs[:nobj], 100)
            assert np.array_equal(e.get_rows(), T) and np.array_equal(e.get_basis(), [basis, basis])
            assert e.get_log(0)[0].size == 0


def test_solve_goal_refuses_bad_arguments_before_any_launch():
    import linearprogramming_amd as lpg
    L = lpg._lib
    A, basis, costs = gc.textbook()
    T = np.zeros((2, 7, 10))
    T[:, :4] = A
    c = np.ascontiguousarray(np.array([costs, costs]))
    cp = c.ctypes.data_as(L.c_double_p)
    with lpg.BatchEngine(2, 4, 10, levels=3) as e:
        e.load(T, np.array([basis, basis]))
        res = (L.Result * 2)()
        for args, word in (((None, 27, 9, 10, 0), "cost is NULL"), ((cp, 27, 8, 10, 0), "ld_level 8 < N = 9"),
                           ((cp, 26, 9, 10, 0), "ld_lp 26 < nlevels * ld_level"), ((cp, 27, 9, -1, 0), "max_pivots < 0"),
                           ((cp, 27, 9, 10, 2), "rule 2")):
            assert e.lib.lpg_batch_solve_goal(e._b, *args, res, None) == L.ERR_ARG, word
            msg = e.lib.lpg_batch_last_error(e._b).decode()
            assert msg.startswith("lpg_batch_solve_goal:") and word in msg, msg
        assert np.array_equal(e.get_rows(), T) and e.get_log(0)[0].size == 0        # nothing has pivoted
        assert e.lib.lpg_batch_solve_goal(e._b, cp, 27, 9, 100, 0, res, None) == 0   # attain may be NULL
        assert [r.status for r in res] == [OPTIMAL, OPTIMAL]


# ---- the front end -------------------------------------------------------------------

def test_frontend_solve_goal_on_a_mixed_list():
    from linearprogramming_amd import frontend as F
    tb = gc.textbook_model()
    # a hard = row and a hard >= row (two artificials, so three device levels), a negative target, three variables
    other = F.GoalModel(A=[[1, 1, 1], [1, 0, 0]], sense=[0, 1], b=[6, 1], G=[[1, 2, 0], [1, -1, 1]], target=[10, -1],
                        under=[(1, 2.0), (2, 1.0)], over=[None, (2, 3.0)])
    infeasible = F.GoalModel(A=[[1, 1, 1], [1, 0, 0]], sense=[0, 1], b=[6, 7], G=[[1, 2, 0], [1, -1, 1]], target=[10, -1],
                             under=[(1, 2.0), (2, 1.0)], over=[None, (2, 3.0)])
    models = [tb, other, infeasible, tb, other]
    for rule in RULES:
        sols = F.solve_goal(models, rule=rule)
        assert [s.status for s in sols] == ["OPTIMAL", "OPTIMAL", "INFEASIBLE", "OPTIMAL", "OPTIMAL"]
        assert np.array_equal(sols[0].x, [2.0, 4.0]) and np.array_equal(sols[0].attained, [0.0, 0.0, 0.0])
        for mod, sol in zip(models, sols):
            arrays = F.goal_arrays(mod)
            rows, basis, costs = arrays[:3]
            res, T, bas, _, _, attain = gc.statement(rows, basis, costs, [50 * (rows.shape[0] + rows.shape[1])], rule)
            want = F._goal_readout(mod, arrays, res[-1].status, res[-1].pivots, attain, T[:rows.shape[0], 0], bas)
            assert (sol.status, sol.pivots) == (want.status, want.pivots)
            for a, w in ((sol.x, want.x), (sol.under, want.under), (sol.over, want.over), (sol.attained, want.attained)):
                assert np.array_equal(bc.bits(a), bc.bits(w))
