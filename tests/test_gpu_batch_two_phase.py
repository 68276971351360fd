"""lpg_batch_solve_two_phase on the device: artificial LPs, both phases and the
transition in one launch (linearprogramming_amd/csrc/lpg_batch.hip
k_batch_two_phase), bit for bit against oracle.lpo.Oracle.solve_two_phase run
once per LP: the status after every call, pivot count, objective bits, last
(entering, leaving), basis, the whole log and the whole (m+1) x ncols tableau,
no tolerance anywhere (tests/batch_cases.py assert_same). Every solve has a
finite budget, 50 * (m + n) unless the case says otherwise. A case counts
only if the oracle shows the property it is there for; that is asserted on
the oracle's result.
"""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

import batch2_cases as b2
import batch_cases as bc
from batch2_cases import INFEASIBLE, ITER_LIMIT, OPTIMAL, UNBOUNDED, spec
from conftest import ROOT
from oracle.lpo import GEN_ARTIFICIAL, RULE_BLAND, RULE_DANTZIG, Oracle

pytestmark = pytest.mark.gpu

TIER_LDS, TIER_GLOBAL = 0, 1
CLI = os.path.join(ROOT, "host", "lpgcli")
LP_DIRS = [os.path.join(ROOT, "tests", "golden", d) for d in ("lp", "lp_extra")]

LDS_SHAPES = [(2, 2), (5, 6), (8, 8), (33, 33), (37, 70), (64, 64)]
GLOBAL_SHAPES = [(96, 160), (130, 130)]
RULES = [RULE_DANTZIG, RULE_BLAND]

_oracle_cache, _device_cache = {}, {}


def oracle_of(s):
    """run_oracle(s), computed once per distinct case and shared (never modified)."""
    key = json.dumps(s, sort_keys=True)
    if key not in _oracle_cache:
        _oracle_cache[key] = b2.run_oracle(s)
    return _oracle_cache[key]


def device_of(s):
    """run_batch(s) at the default chunk and tier, once per distinct case."""
    key = json.dumps(s, sort_keys=True)
    if key not in _device_cache:
        _device_cache[key] = b2.run_batch(s)
    return _device_cache[key]


def check(s, tier=None):
    got, want = device_of(s), oracle_of(s)
    if tier is not None:
        assert int(got["tier"]) == tier
    bc.assert_same(got, want)
    return got, want


def in_subprocess(specs, env, tmp_path):
    """The cases on the device in a fresh process under `env` (tests/batch_worker.py)."""
    return bc.in_subprocess("batch2_cases", specs, env, tmp_path)


# ---- 1, 2: shapes per tier, both rules ---------------------------------------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("m,n", LDS_SHAPES)
def test_lds_tier_shapes(m, n, rule):
    got, want = check(spec(m, n, rule=rule), TIER_LDS)
    if m == n:
        assert (want["status"] == OPTIMAL).all() and (want["pivots"] == m).all()
    else:
        assert (want["status"] == UNBOUNDED).all() and want["pivots"].min() >= 2


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("m,n", GLOBAL_SHAPES)
def test_global_tier_shapes(m, n, rule):
    got, want = check(spec(m, n, rule=rule), TIER_GLOBAL)
    assert want["pivots"].min() >= 48


def test_both_tiers_on_the_same_data(tmp_path):
    specs = [spec(m, n, rule=rule) for m, n in LDS_SHAPES for rule in RULES]
    for s, got in zip(specs, in_subprocess(specs, {"LPG_BATCH_TIER": "global"}, tmp_path)):
        assert int(got["tier"]) == TIER_GLOBAL
        bc.assert_same(got, oracle_of(s))


# ---- 3: drive-out, inconsistent, redundant and plain LPs in one batch ---------

MIXED = [spec(8, 8, construct="mixed4"), spec(37, 70, construct="mixed4")]
DRIVEOUT = [spec(8, 8, construct="driveout"), spec(37, 70, construct="driveout")]


def test_mixed_batch_and_independence():
    seen = set()
    for s in MIXED:
        got, want = check(s, TIER_LDS)
        p1 = b2.phase_one(s)
        # LP b: (drive-out, inconsistent, redundant, plain)[b % 4]
        assert all(want["status"][b] == INFEASIBLE for b in (1, 5))
        assert len(set(want["status"].tolist())) >= 2
        seen |= set(want["status"].tolist())
        # an LP with drive-outs reached phase II: phase I ended feasible with usable rows, phase II pivoted
        assert any(p1[b][3] >= 1 and want["status"][b] in (OPTIMAL, UNBOUNDED) and want["pivots"][b] > p1[b][1]
                   for b in (0, 4))
        # redundant: the artificial stays basic (no usable column) and the LP still reaches phase II
        af = b2.art_first_of(s)
        assert all((want["basis"][b] >= af).sum() == 1 and p1[b][3] == 0 and want["status"][b] != INFEASIBLE
                   for b in (2, 6))
        # LP i of the batch = the same LP solved alone
        for i in (0, 1, 2, 7):
            alone = b2.run_batch({**s, "only": i})
            for key in ("status", "pivots", "entering", "leaving", "basis"):
                assert np.array_equal(alone[key][0], got[key][i]), (i, key)
            assert np.array_equal(bc.bits(alone["objective"][0]), bc.bits(got["objective"][i]))
            assert np.array_equal(bc.bits(alone["rows"][0]), bc.bits(got["rows"][i]))
            lo = int(got["loglen"][:i].sum())
            assert np.array_equal(alone["logk"], got["logk"][lo:lo + int(got["loglen"][i])])
    # OPTIMAL, UNBOUNDED and INFEASIBLE between the two batches (each shape's feasible LPs share one outcome)
    assert len(seen) >= 3


@pytest.mark.parametrize("construct,m,n,status,kept", [("inconsistent", 8, 8, INFEASIBLE, 1),
                                                       ("inconsistent", 33, 33, INFEASIBLE, 1),
                                                       ("redundant", 8, 8, OPTIMAL, 1),
                                                       ("redundant", 33, 33, OPTIMAL, 1)])
def test_inconsistent_and_redundant_rows(construct, m, n, status, kept):
    s = spec(m, n, construct=construct)
    got, want = check(s)
    assert (want["status"] == status).all()
    assert ((want["basis"] >= b2.art_first_of(s)).sum(axis=1) == kept).all()
    assert all(p[3] == 0 for p in b2.phase_one(s))          # no usable column: nothing to drive out


def test_drive_outs_on_negative_pivots():
    for s, status in zip(DRIVEOUT, (OPTIMAL, UNBOUNDED)):
        got, want = check(s)
        p1 = b2.phase_one(s)
        assert (want["status"] == status).all() and all(p[0] == OPTIMAL and p[3] == 2 for p in p1)
        m, n, af = s["m"], s["n"], b2.art_first_of(s)
        lo = 0
        for b in range(s["B"]):
            k, r = (want[key][lo:lo + int(want["loglen"][b])] for key in ("logk", "logr"))
            lo += int(want["loglen"][b])
            # exactly the two drive-out pivots follow phase I: rows 3 and 5 on structural columns n and n - 1
            assert list(zip(k[p1[b][1]:p1[b][1] + 2], r[p1[b][1]:p1[b][1] + 2])) == [(n, 3), (n - 1, 5)]
            assert (want["basis"][b] < af).all()


# ---- 4: budgets ------------------------------------------------------------------

def test_budget_inside_phase_one():
    for s in (spec(37, 70, budgets=[7]), spec(8, 8, budgets=[3])):
        got, want = check(s)
        assert (want["status"] == ITER_LIMIT).all() and (want["pivots"] == s["budgets"][0]).all()
        assert (want["objective"] < 0).all()                 # the phase-I objective, still negative


def test_budget_20_ends_in_phase_two_beside_infeasible():
    s = spec(33, 33, construct="mixed4", budgets=[20])
    got, want = check(s)
    p1 = b2.phase_one(s)
    in_two = [b for b in range(8) if want["status"][b] == ITER_LIMIT and p1[b][0] == OPTIMAL]
    assert in_two and all(want["pivots"][b] == 20 > p1[b][1] for b in in_two)
    assert (want["status"] == INFEASIBLE).any()


def test_budget_equal_to_the_pivot_count_reports_optimal():
    full = oracle_of(spec(8, 8, construct="redundant"))
    exact = int(full["pivots"].min())
    got, want = check(spec(8, 8, construct="redundant", budgets=[exact]))
    first = int(np.argmin(full["pivots"]))
    assert got["status"][first] == OPTIMAL and got["pivots"][first] == exact      # through the peek
    assert (full["pivots"] > exact).any() and (got["status"][full["pivots"] > exact] == ITER_LIMIT).all()


TWO_CALLS = spec(37, 70, budgets=[7, 50 * 107], cost="explicit")


def test_two_calls_with_an_explicit_cost_equal_the_oracle_called_twice():
    got, want = check(TWO_CALLS)
    assert (want["calls"][0] == ITER_LIMIT).all() and (want["calls"][1] != ITER_LIMIT).all()


# ---- 5: small chunks: every launch ends after one or three units of work -------------

CHUNKED = MIXED + DRIVEOUT + [spec(37, 70, budgets=[7]), spec(33, 33, construct="mixed4", budgets=[20]), TWO_CALLS,
                              spec(37, 70, rule=RULE_BLAND), spec(96, 160)]


@pytest.mark.parametrize("chunk", [1, 3])
def test_small_chunks_equal_the_default(chunk, tmp_path):
    for s, got in zip(CHUNKED, in_subprocess(CHUNKED, {"LPG_BATCH_CHUNK": str(chunk)}, tmp_path)):
        assert int(got["chunk"]) == chunk
        bc.assert_same(got, oracle_of(s))
        bc.assert_same(got, device_of(s))


# ---- 6: costs -----------------------------------------------------------------------

@pytest.mark.parametrize("m,n", [(8, 8), (37, 70)])
def test_explicit_per_lp_costs_and_none(m, n):
    s = spec(m, n, cost="explicit")
    c = b2.costs_of(s)
    assert c.shape[1] > b2.ncols_of(s) - 1 and len({c[b].tobytes() for b in range(8)}) == 8
    got, want = check(s)
    none = check(spec(m, n))[1]
    assert not np.array_equal(bc.bits(want["objective"]), bc.bits(none["objective"]))


# ---- 7: generator -----------------------------------------------------------------

@pytest.mark.parametrize("m,n", [(37, 70), (5, 6)])
def test_generate_artificial_equals_the_oracle(m, n):
    import linearprogramming_amd as lpg
    with lpg.BatchEngine(8, m, n + m + 1) as e:
        af = e.generate_artificial(n, bc.SEED)
        rows, basis = e.get_rows(), e.get_basis()
    assert af == 1 + n + (m + 1) // 2
    for b in range(8):
        o = Oracle(m, n + m + 1)
        o.generate(n, bc.SEED + b, GEN_ARTIFICIAL)
        assert np.array_equal(bc.bits(rows[b]), bc.bits(o.get_rows())), b
        assert np.array_equal(basis[b], o.get_basis()), b
        assert (basis[b][1::2] >= af).all() and (basis[b][0::2] < af).all()


# ---- 8: validation ------------------------------------------------------------------

def test_host_side_validation_on_a_live_batch():
    import linearprogramming_amd as lpg
    m, n = 5, 6
    N = n + m
    with lpg.BatchEngine(4, m, N + 1) as e:
        af = e.generate_artificial(n, bc.SEED)
        before, basis = e.get_rows(), e.get_basis()
        for bad, what in ((1, "art_first"), (N + 1, "art_first")):
            with pytest.raises(lpg.LPGError, match=f"rc=-1.*{what}"):
                e.solve_two_phase(bad, None, 100)
        with pytest.raises(lpg.LPGError, match="rc=-1.*rule"):
            e.solve_two_phase(af, None, 100, 7)
        with pytest.raises(lpg.LPGError, match="rc=-1.*ld_cost"):
            e.solve_two_phase(af, np.zeros((4, N - 1)), 100)
        with pytest.raises(lpg.LPGError, match="rc=-1.*max_pivots"):
            e.solve_two_phase(af, None, -1)
        assert np.array_equal(bc.bits(e.get_rows()), bc.bits(before)) and np.array_equal(e.get_basis(), basis)
        assert all(len(e.get_log(b)[0]) == 0 for b in range(4))
        with pytest.raises(lpg.LPGError, match="rc=-1"):
            e.generate(n, 1, GEN_ARTIFICIAL)                   # lpg_batch_generate keeps refusing kind 2
        res = e.solve_two_phase(af, None, 100)                 # and the batch is still usable
        assert all(r.status == UNBOUNDED for r in res)


# ---- 9: frontend.solve_batch ----------------------------------------------------------

def _same_solution(a, b):
    def fbits(d):
        return {k: np.float64(v).view(np.int64) for k, v in d.items()}
    return (a.status == b.status and a.pivots == b.pivots and a.method == b.method and
            np.float64(a.z).view(np.int64) == np.float64(b.z).view(np.int64) and
            list(a.columns) == list(b.columns) and fbits(a.columns) == fbits(b.columns) and
            list(a.variables) == list(b.variables) and fbits(a.variables) == fbits(b.variables))


@pytest.mark.parametrize("rule", RULES)
def test_solve_batch_equals_solve_on_the_golden_models(rule):
    """Every model file build_smatrix accepts, under both rules -- except Beale's
    LP under Dantzig's rule: it cycles for good (tests/test_oracle.py; the oracle
    is still at it after 10^6 pivots) and neither solve() nor solve_batch() takes
    a budget, so that one pair would never return. Bland's rule solves it."""
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
    groups = F.batch_groups(sms)
    assert any(k[2] > 0 for k in groups) and any(k[2] == 0 for k in groups) and any(len(v) > 1 for v in groups.values())
    got = F.solve_batch(sms, rule=rule)
    assert len(got) == len(sms)
    for name, sm, g in zip(names, sms, got):
        assert _same_solution(g, F.solve(sm, rule=rule)), (name, g)
    assert {g.method for g in got} == {"primal", "two_phase"}
    assert {"OPTIMAL", "UNBOUNDED", "INFEASIBLE"} <= {g.status for g in got}


def test_solve_batch_on_a_right_hand_side_sweep():
    import copy
    from fractions import Fraction
    from linearprogramming_amd import frontend as F
    base = F.build_smatrix(open(os.path.join(LP_DIRS[0], "a3_min_eq_neg.txt"), "rb").read())
    sms = []
    for k in range(8):
        sm = copy.deepcopy(base)
        for r in sm.rows:
            r[0] = r[0] * (1 + Fraction(k, 8))
        sms.append(sm)
    assert list(F.batch_groups(sms).values()) == [list(range(8))]
    got = F.solve_batch(sms)
    want = [F.solve(sm) for sm in sms]
    assert all(_same_solution(g, w) for g, w in zip(got, want))
    assert all(w.status == "OPTIMAL" and w.method == "two_phase" for w in want)
    assert len({w.z for w in want}) == 8


# ---- 10: the plain-C host ---------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(CLI), reason="host/lpgcli not built")
@pytest.mark.parametrize("rule", RULES)
def test_cli_batch_artificial(rule):
    p = subprocess.run([CLI, "--synthetic", "8", "8", "--kind", "artificial", "--batch", "16"] +
                       (["--rule", "bland"] if rule == RULE_BLAND else []), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    got = json.loads(lines[0])
    assert (got["m"], got["ncols"], got["batch"], got["tier"], got["method"]) == (8, 17, 16, "lds", "two-phase")
    assert sum(got["statuses"].values()) == 16 and got["statuses"]["OPTIMAL"] == 16
    want = oracle_of(spec(8, 8, B=16, rule=rule, budgets=[1 << 40]))
    assert got["pivots"] == int(want["pivots"].sum())
