"""lpg_batch_solve_big_m on the device: Big-M batches, (m+2) x ncols tableaus
with the M part of the objective in row m and the real part in row m + 1,
priced lexicographically (linearprogramming_amd/csrc/lpg_batch.hip
k_batch_big_m), bit for bit against oracle.lpo.Oracle(nobj=2).solve_big_m run
once per LP: the status after every call, pivot count, objective bits, last
(entering, leaving), basis, the whole log and the whole (m+2) x ncols tableau,
no tolerance anywhere (tests/batch_cases.py assert_same). Every solve has a
finite budget, 50 * (m + n) unless the case says otherwise. A case counts
only if the oracle shows the property it is there for; that is asserted on
the oracle's result. Also frontend.solve_batch's methods and the CLI.
"""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

import batch3_cases as b3
import batch_cases as bc
from batch3_cases import INFEASIBLE, ITER_LIMIT, OPTIMAL, UNBOUNDED, literal, spec
from conftest import ROOT
from oracle.lpo import GEN_ARTIFICIAL, GEN_DENSE, RULE_BLAND, RULE_DANTZIG, Oracle

pytestmark = pytest.mark.gpu

TIER_LDS, TIER_GLOBAL = 0, 1
CLI = os.path.join(ROOT, "host", "lpgcli")
LP_DIRS = [os.path.join(ROOT, "tests", "golden", d) for d in ("lp", "lp_extra")]

# (95, 95) is the last square shape whose m + 2 rows fit the LDS cap (150,904 of 153,600 bytes);
# (96, 96) needs 154,024 and goes to device memory, while a plain batch of that shape (152,472) stays in LDS
LDS_SHAPES = [(2, 2), (5, 6), (8, 8), (33, 33), (37, 70), (64, 64), (95, 95)]
GLOBAL_SHAPES = [(96, 96), (96, 160), (130, 130)]
RULES = [RULE_DANTZIG, RULE_BLAND]

_oracle_cache, _device_cache = {}, {}


def oracle_of(s):
    """run_oracle(s), computed once per distinct case and shared (never modified)."""
    key = json.dumps(s, sort_keys=True)
    if key not in _oracle_cache:
        _oracle_cache[key] = b3.run_oracle(s)
    return _oracle_cache[key]


def device_of(s):
    """run_batch(s) at the default chunk and tier, once per distinct case."""
    key = json.dumps(s, sort_keys=True)
    if key not in _device_cache:
        _device_cache[key] = b3.run_batch(s)
    return _device_cache[key]


def check(s, tier=None):
    got, want = device_of(s), oracle_of(s)
    if tier is not None:
        assert int(got["tier"]) == tier
    assert int(got["nobj"]) == 2 and got["rows"].shape[1] == s["m"] + 2
    bc.assert_same(got, want)
    return got, want


def in_subprocess(specs, env, tmp_path):
    """The cases on the device in a fresh process under `env` (tests/batch_worker.py)."""
    return bc.in_subprocess("batch3_cases", specs, env, tmp_path)


def _shape_property(m, n, want):
    if m == n:
        assert (want["status"] == OPTIMAL).all() and (want["pivots"] == m).all()
    else:
        assert (want["status"] == UNBOUNDED).all() and want["pivots"].min() >= 2


# ---- 1, 2: shapes per tier, both rules ---------------------------------------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("m,n", LDS_SHAPES)
def test_lds_tier_shapes(m, n, rule):
    got, want = check(spec(m, n, rule=rule), TIER_LDS)
    _shape_property(m, n, want)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("m,n", GLOBAL_SHAPES)
def test_global_tier_shapes(m, n, rule):
    got, want = check(spec(m, n, rule=rule), TIER_GLOBAL)
    _shape_property(m, n, want)


def test_the_tier_boundary_counts_the_second_objective_row():
    import linearprogramming_amd as lpg
    with lpg.BatchEngine(8, 95, 191, big_m=True) as e:
        assert (e.info.tier, e.info.lds_bytes, e.info.nobj) == (TIER_LDS, 150904, 2)
    with lpg.BatchEngine(8, 96, 193, big_m=True) as e:
        assert (e.info.tier, e.info.nobj) == (TIER_GLOBAL, 2)
    with lpg.BatchEngine(8, 96, 193) as e:                     # the plain batch of that shape still fits
        assert (e.info.tier, e.info.lds_bytes, e.info.nobj) == (TIER_LDS, 152472, 1)


def test_both_tiers_on_the_same_data(tmp_path):
    specs = [spec(m, n, rule=rule) for m, n in LDS_SHAPES for rule in RULES]
    for s, got in zip(specs, in_subprocess(specs, {"LPG_BATCH_TIER": "global"}, tmp_path)):
        assert int(got["tier"]) == TIER_GLOBAL
        bc.assert_same(got, oracle_of(s))


# ---- 3: infeasible, redundant, zero-level artificials and plain LPs in one batch ----

MIXED = [spec(8, 8, construct="mixed4"), spec(37, 70, construct="mixed4")]


def test_mixed_batch_and_independence():
    seen = set()
    for s, rest in zip(MIXED, (OPTIMAL, UNBOUNDED)):
        got, want = check(s, TIER_LDS)
        # LP b: (driveout, inconsistent, redundant, plain)[b % 4]
        assert all(want["status"][b] == (INFEASIBLE if b in (1, 5) else rest) for b in range(8))
        seen |= set(want["status"].tolist())
        # LP i of the batch = the same LP solved alone
        for i in (0, 1, 2, 7):
            alone = b3.run_batch({**s, "only": i})
            for key in ("status", "pivots", "entering", "leaving", "basis"):
                assert np.array_equal(alone[key][0], got[key][i]), (i, key)
            assert np.array_equal(bc.bits(alone["objective"][0]), bc.bits(got["objective"][i]))
            assert np.array_equal(bc.bits(alone["rows"][0]), bc.bits(got["rows"][i]))
            lo = int(got["loglen"][:i].sum())
            assert np.array_equal(alone["logk"], got["logk"][lo:lo + int(got["loglen"][i])])
            assert np.array_equal(alone["logr"], got["logr"][lo:lo + int(got["loglen"][i])])
    assert seen == {OPTIMAL, UNBOUNDED, INFEASIBLE}


@pytest.mark.parametrize("construct,m,n,status,kept", [("inconsistent", 8, 8, INFEASIBLE, None),
                                                       ("inconsistent", 33, 33, INFEASIBLE, None),
                                                       ("inconsistent", 37, 70, INFEASIBLE, None),
                                                       ("redundant", 8, 8, OPTIMAL, 1),
                                                       ("redundant", 33, 33, OPTIMAL, 1),
                                                       ("driveout", 8, 8, OPTIMAL, 2)])
def test_inconsistent_redundant_and_zero_level_artificials(construct, m, n, status, kept):
    s = spec(m, n, construct=construct)
    got, want = check(s)
    assert (want["status"] == status).all()
    if kept is not None:
        # Big-M has no drive-out: the artificials stay basic (at a level the feasibility test takes for zero)
        assert ((want["basis"] >= b3.art_first_of(s)).sum(axis=1) == kept).all()


# ---- 4: infeasible with a ray ------------------------------------------------------

LITERALS = [literal("inf_ray"), literal("inf_ray", rule=RULE_BLAND), literal("a5_inf"), literal("a5_inf", rule=RULE_BLAND)]


@pytest.mark.parametrize("rule", RULES)
def test_infeasible_with_a_ray(rule):
    s = literal("inf_ray", rule=rule)
    assert b3.art_first_of(s) == 3
    got, want = check(s, TIER_LDS)
    assert (want["status"] == INFEASIBLE).all()
    # the plain loop on the same two objective rows ends on the ray: UNBOUNDED; solve_big_m turns it into INFEASIBLE
    o = Oracle(2, 5, nobj=2)
    o.load_tableau(b3.INF_RAY, [3, 4])
    o.set_objective_m([0.0, 0.0, -1.0, -1.0])
    o.set_objective([1.0, 0.0, 0.0, 0.0])
    r = o.solve(100, rule)
    assert r.status == UNBOUNDED and o.get_rows()[2, 0] < 0
    assert r.pivots == want["pivots"][0]
    o.close()


@pytest.mark.parametrize("rule", RULES)
def test_a5_and_inf_side_by_side(rule):
    s = literal("a5_inf", rule=rule)
    assert b3.art_first_of(s) == 4 and b3.costs_of(s)[0, 3] == 7.0
    got, want = check(s, TIER_LDS)
    assert want["status"].tolist() == [OPTIMAL, INFEASIBLE, OPTIMAL, INFEASIBLE]
    assert want["objective"][0] == want["objective"][2] == 6.0
    assert want["rows"][0, 2, 0] == 0.0                        # M part of z is zero: no artificial left positive


# ---- 5: budgets and resumption --------------------------------------------------------

BUDGETS = [spec(8, 8, budgets=[3]), spec(37, 70, budgets=[7])]
TWO_CALLS = [spec(37, 70, budgets=[7, 50 * 107], cost="explicit"), spec(37, 70, budgets=[7, 50 * 107])]


def test_budget_inside_the_loop():
    for s in BUDGETS:
        got, want = check(s)
        assert (want["status"] == ITER_LIMIT).all() and (want["pivots"] == s["budgets"][0]).all()


EXACT = spec(8, 8, budgets=[8])


def test_budget_equal_to_the_pivot_count_reports_optimal():
    full = oracle_of(spec(8, 8))
    assert (full["pivots"] == 8).all()
    got, want = check(EXACT)
    assert (want["status"] == OPTIMAL).all() and (want["pivots"] == 8).all()       # through the peek
    bc.assert_same(got, full)


@pytest.mark.parametrize("s", TWO_CALLS, ids=["explicit", "none"])
def test_two_calls_equal_the_oracle_called_twice(s):
    got, want = check(s)
    assert (want["calls"][0] == ITER_LIMIT).all() and (want["calls"][1] == UNBOUNDED).all()
    assert (want["pivots"] > 7).all()
    if s["cost"] == "none":
        # the second call took its costs from row m + 1 as the first call left it: another problem than one call solves
        one = oracle_of(spec(37, 70))
        assert not np.array_equal(bc.bits(want["rows"]), bc.bits(one["rows"]))


# ---- 6: explicit costs ---------------------------------------------------------------

@pytest.mark.parametrize("m,n", [(8, 8), (37, 70)])
def test_explicit_per_lp_costs(m, n):
    s = spec(m, n, cost="explicit")
    c = b3.costs_of(s)
    N, af = b3.ncols_of(s) - 1, b3.art_first_of(s)
    assert c.shape[1] == N + 3 and len({c[b].tobytes() for b in range(8)}) == 8
    assert (c[:, af - 1:N] == 7.0).all() and (c[:, N:] == 1e300).all()
    got, want = check(s)
    none = check(spec(m, n))[1]
    assert not np.array_equal(bc.bits(want["objective"]), bc.bits(none["objective"]))
    # the 7.0 at the artificial columns left no trace: the same costs with zeros there give the same bits
    c[:, af - 1:N] = 0.0
    bc.assert_same(b3.run_oracle(s, cost=c), want)


# ---- 7: small chunks: every launch ends after one, three or seven units of work --------

# every case of sections 3 to 5, at every shape they run at
CHUNKED = (MIXED + [spec(8, 8, construct="inconsistent"), spec(33, 33, construct="inconsistent"),
                    spec(37, 70, construct="inconsistent"), spec(8, 8, construct="redundant"),
                    spec(33, 33, construct="redundant"), spec(8, 8, construct="driveout")] +
           LITERALS + BUDGETS + [EXACT] + TWO_CALLS)


@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_small_chunks_equal_the_oracle(chunk, tmp_path):
    for s, got in zip(CHUNKED, in_subprocess(CHUNKED, {"LPG_BATCH_CHUNK": str(chunk)}, tmp_path)):
        assert int(got["chunk"]) == chunk
        bc.assert_same(got, oracle_of(s))


# ---- 8: generator ---------------------------------------------------------------------

@pytest.mark.parametrize("m,n", [(8, 8), (37, 70)])
def test_generate_artificial_on_a_big_m_batch_equals_the_oracle(m, n):
    import linearprogramming_amd as lpg
    with lpg.BatchEngine(8, m, n + m + 1, big_m=True) as e:
        af = e.generate_artificial(n, bc.SEED)
        rows, basis = e.get_rows(), e.get_basis()
    assert af == 1 + n + (m + 1) // 2 and rows.shape == (8, m + 2, n + m + 1)
    for b in range(8):
        o = Oracle(m, n + m + 1, nobj=2)
        o.generate(n, bc.SEED + b, GEN_ARTIFICIAL)
        assert np.array_equal(bc.bits(rows[b]), bc.bits(o.get_rows())), b
        assert np.array_equal(basis[b], o.get_basis()), b
        assert not rows[b, m].any() and (rows[b, m + 1, 1:n + 1] < 0).all()     # zero M row, objective in row m + 1
        o.close()


# ---- 9: validation ----------------------------------------------------------------------

def test_host_side_validation_on_a_live_batch():
    import linearprogramming_amd as lpg
    m, n = 5, 6
    N = n + m
    with lpg.BatchEngine(4, m, N + 1, big_m=True) as e:
        af = e.generate_artificial(n, bc.SEED)
        before, basis = e.get_rows(), e.get_basis()

        def unchanged():
            assert np.array_equal(bc.bits(e.get_rows()), bc.bits(before)) and np.array_equal(e.get_basis(), basis)
            assert all(len(e.get_log(b)[0]) == 0 for b in range(4))

        for bad in (1, N + 1):
            with pytest.raises(lpg.LPGError, match="rc=-1.*lpg_batch_solve_big_m.*art_first"):
                e.solve_big_m(bad, None, 100)
            unchanged()
        with pytest.raises(lpg.LPGError, match="rc=-1.*lpg_batch_solve_big_m.*rule"):
            e.solve_big_m(af, None, 100, 7)
        unchanged()
        with pytest.raises(lpg.LPGError, match="rc=-1.*lpg_batch_solve_big_m.*ld_cost"):
            e.solve_big_m(af, np.zeros((4, N - 1)), 100)
        unchanged()
        with pytest.raises(lpg.LPGError, match="rc=-1.*lpg_batch_solve_big_m.*max_pivots"):
            e.solve_big_m(af, None, -1)
        unchanged()
        # the calls of a plain batch refuse a Big-M batch
        for name, call in (("lpg_batch_solve", lambda: e.solve(100)),
                           ("lpg_batch_solve_dual", lambda: e.solve_dual(100)),
                           ("lpg_batch_solve_two_phase", lambda: e.solve_two_phase(af, None, 100)),
                           ("lpg_batch_set_objective", lambda: e.set_objective(np.ones(N))),
                           ("lpg_batch_set_active_columns", lambda: e.set_active_columns(n)),
                           ("lpg_batch_generate", lambda: e.generate(n, 1, GEN_DENSE))):
            with pytest.raises(lpg.LPGError, match=f"rc=-4: {name}:.*nothing has pivoted"):
                call()
            unchanged()
        with pytest.raises(lpg.LPGError, match="want \\[n, 7, 12\\]"):
            e.load(np.zeros((4, m + 1, N + 1)))
        res = e.solve_big_m(af, None, 100)                     # and the batch is still usable
        assert all(r.status == UNBOUNDED for r in res)
    with lpg.BatchEngine(4, m, N + 1) as e:                    # and a plain batch refuses Big-M
        af = e.generate_artificial(n, bc.SEED)
        before, basis = e.get_rows(), e.get_basis()
        with pytest.raises(lpg.LPGError, match="rc=-4: lpg_batch_solve_big_m:.*nothing has pivoted"):
            e.solve_big_m(af, None, 100)
        assert np.array_equal(bc.bits(e.get_rows()), bc.bits(before)) and np.array_equal(e.get_basis(), basis)
        assert e.info.nobj == 1 and before.shape[1] == m + 1
    with pytest.raises(lpg.LPGError, match="rc=-1.*flags"):
        lpg.BatchEngine(4, m, N + 1, flags=lpg._lib.FLAG_BIG_M)


# ---- 10, 11: frontend.solve_batch(method=...) -----------------------------------------------

def _same_solution(a, b):
    def fbits(d):
        return {k: np.float64(v).view(np.int64) for k, v in d.items()}
    return (a.status == b.status and a.pivots == b.pivots and a.method == b.method and
            np.float64(a.z).view(np.int64) == np.float64(b.z).view(np.int64) and
            list(a.columns) == list(b.columns) and fbits(a.columns) == fbits(b.columns) and
            list(a.variables) == list(b.variables) and fbits(a.variables) == fbits(b.variables))


@pytest.mark.parametrize("rule", RULES)
def test_solve_batch_big_m_equals_solve_on_the_golden_models(rule):
    """Every model file build_smatrix accepts, twice over in one call, under both
    rules -- except Beale's LP under Dantzig's rule, which cycles for good
    (tests/test_gpu_batch_two_phase.py says why); Bland's rule solves it."""
    from linearprogramming_amd import frontend as F
    names, sms = [], []
    for d in LP_DIRS:
        for name in sorted(os.listdir(d)):
            if name == "kat_beale_cycling.txt" and rule == RULE_DANTZIG:
                continue
            try:
                sms.append(F.build_smatrix(open(os.path.join(d, name), "rb").read()))
                names.append(name)
            except F.FrontendError:
                pass                                           # not a model (testdata_shipped.txt)
    assert len(sms) >= 12
    lacking = {name: b3.oracle_model_big_m(sm, rule) for name, sm in zip(names, sms) if F.engine_arrays(sm)[4]}
    assert {k: v.status for k, v in lacking.items()} == b3.LACKING_MODELS
    assert lacking["m_ray_infeasible.txt"].pivots == (1 if rule == RULE_DANTZIG else 0)
    want = [F.solve(sm, method="big_m", rule=rule) for sm in sms]
    got = F.solve_batch(sms * 2, rule, method="big_m")
    assert len(got) == 2 * len(sms)
    for q, g in enumerate(got):
        assert _same_solution(g, want[q % len(sms)]), (names[q % len(sms)], g)
    assert {g.method for g in got} == {"primal", "big_m"}
    for name, w in zip(names, want):
        if name in lacking:
            assert (w.method, w.status, w.pivots) == ("big_m", bc_status(lacking[name].status), lacking[name].pivots)
    # positional callers and the default method are what they were
    two = F.solve_batch(sms, rule)
    assert {g.method for g in two} == {"primal", "two_phase"}


def bc_status(code):
    from oracle.lpo import STATUS_NAMES
    return STATUS_NAMES[code]


DUAL_LP = "OF {\n\tmin:z=2x1+3x2\n}\nST {\n\tx1+x2>=4;\n\tx1+3x2>=6;\n\tx1>=0;\n\tx2>=0\n}\n"
DUAL_LP3 = "OF {\n\tmin:z=x1+2x2+3x3\n}\nST {\n\tx1+x2+x3>=3;\n\tx1+2x3>=2;\n\tx2+x3<=5;\n\tx1>=0;\n\tx2>=0;\n\tx3>=0\n}\n"


def _dual_sweep():
    import copy
    from fractions import Fraction
    from linearprogramming_amd import frontend as F
    sms = []
    for text, count in ((DUAL_LP, 8), (DUAL_LP3, 3)):
        base = F.build_smatrix(text, dual=True)
        for k in range(count):
            sm = copy.deepcopy(base)
            for r in sm.rows:
                r[0] = r[0] * (1 + Fraction(k, 8))
            sms.append(sm)
    return sms[:4] + sms[8:] + sms[4:8]                        # the second shape in the middle of the first


def test_solve_batch_dual_on_a_right_hand_side_sweep():
    from linearprogramming_amd import frontend as F
    sms = _dual_sweep()
    groups = F.batch_groups(sms)
    assert sorted(len(v) for v in groups.values()) == [3, 8] and all(k[2] == 0 for k in groups)
    got = F.solve_batch(sms, method="dual")
    want = [F.solve(sm, method="dual") for sm in sms]
    assert all(_same_solution(g, w) for g, w in zip(got, want))
    assert all(w.status == "OPTIMAL" and w.method == "dual" for w in want) and any(w.pivots >= 1 for w in want)
    assert len({w.z for w in want}) >= 8


def test_solve_batch_dual_checks_every_model_before_any_device_work(monkeypatch):
    from linearprogramming_amd import engine as E
    from linearprogramming_amd import frontend as F
    created = []

    class Counting(E.BatchEngine):
        def __init__(self, *a, **kw):
            created.append(a)
            super().__init__(*a, **kw)

    monkeypatch.setattr(E, "BatchEngine", Counting)
    sms = _dual_sweep()
    sms.insert(5, F.build_smatrix("OF {\n max:z=x1\n}\nST {\n x1<=3;\n x1>=0\n}\n", dual=True))
    with pytest.raises(F.FrontendError, match="model 5.*dual feasible"):
        F.solve_batch(sms, method="dual")
    sms[5] = F.build_smatrix(DUAL_LP)                          # the primal form: rows without a slack basis
    with pytest.raises(F.FrontendError, match="model 5.*slack basis"):
        F.solve_batch(sms, method="dual")
    assert created == []
    del sms[5]
    assert len(F.solve_batch(sms, method="dual")) == 11 and len(created) == 2


# ---- 12: the plain-C host -------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(CLI), reason="host/lpgcli not built")
@pytest.mark.parametrize("rule", RULES)
def test_cli_batch_big_m(rule):
    p = subprocess.run([CLI, "--synthetic", "8", "8", "--kind", "artificial", "--big-m", "--batch", "16"] +
                       (["--rule", "bland"] if rule == RULE_BLAND else []), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    got = json.loads(lines[0])
    assert (got["m"], got["ncols"], got["batch"], got["tier"], got["method"]) == (8, 17, 16, "lds", "big-m")
    assert got["rule"] == ("bland" if rule == RULE_BLAND else "dantzig")
    assert sum(got["statuses"].values()) == 16 and got["statuses"]["OPTIMAL"] == 16
    want = oracle_of(spec(8, 8, B=16, rule=rule, budgets=[1 << 40]))
    assert (want["status"] == OPTIMAL).all() and got["pivots"] == int(want["pivots"].sum())
