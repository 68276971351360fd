"""lpg_batch on the device: many small LPs in one launch, one workgroup per LP
(linearprogramming_amd/csrc/lpg_batch.hip), bit for bit against the CPU
oracle run once per LP: status, pivot count, objective bits, basis, the whole
log and the whole (m+1) x ncols tableau, no tolerance anywhere
(tests/batch_cases.py assert_same). Every solve has a finite budget,
50 * (m + n) unless the case says otherwise.
"""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

import batch_cases as bc
from batch_cases import spec
from conftest import ROOT
from oracle.lpo import GEN_DEGENERATE, GEN_DENSE, GEN_DUAL, RULE_BLAND, Oracle

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT = 1, 2, 3, 4
TIER_LDS, TIER_GLOBAL = 0, 1
CLI = os.path.join(ROOT, "host", "lpgcli")

LDS_SHAPES = [(2, 2), (5, 6), (37, 70), (20, 300), (120, 3), (64, 128)]
GLOBAL_SHAPES = [(96, 160), (130, 60), (300, 10)]

_oracle_cache = {}


def oracle_of(s):
    """run_oracle(s), computed once per distinct case and shared (never modified)."""
    key = json.dumps(s, sort_keys=True)
    if key not in _oracle_cache:
        _oracle_cache[key] = bc.run_oracle(s)
    return _oracle_cache[key]


def check(s, tier=None):
    got, want = bc.run_batch(s), oracle_of(s)
    if tier is not None:
        assert int(got["tier"]) == tier
    bc.assert_same(got, want)
    return got, want


def in_subprocess(specs, env, tmp_path):
    """The cases on the device in a fresh process under `env` (tests/batch_worker.py)."""
    return bc.in_subprocess("batch_cases", specs, env, tmp_path)


# ---- shapes per tier -------------------------------------------------------

@pytest.mark.parametrize("m,n", LDS_SHAPES)
def test_lds_tier_shapes(m, n):
    check(spec(m, n), TIER_LDS)


@pytest.mark.parametrize("m,n", GLOBAL_SHAPES)
def test_global_tier_shapes(m, n):
    check(spec(m, n), TIER_GLOBAL)


def test_kat_tableau_next_to_other_lps():
    """The 2 x 5 tableau of __graft_entry__.smoke() (z* = 12) as LP 1 of 3."""
    got, _ = check(spec(2, 2, B=3, construct="kat", budgets=[10]), TIER_LDS)
    assert got["status"][1] == OPTIMAL and abs(got["objective"][1] + 19 / 3 - 12.0) < 1e-12


def test_both_tiers_on_the_same_data(tmp_path):
    specs = [spec(m, n) for m, n in LDS_SHAPES]
    for s, got in zip(specs, in_subprocess(specs, {"LPG_BATCH_TIER": "global"}, tmp_path)):
        assert int(got["tier"]) == TIER_GLOBAL
        bc.assert_same(got, oracle_of(s))


# ---- more LPs than can be resident -----------------------------------------

def test_600_lps_of_one_per_cu():
    got, want = check(spec(64, 128, B=600), TIER_LDS)
    assert (want["status"] == OPTIMAL).all() and want["pivots"].min() >= 20


def test_3000_tiny_lps():
    got, want = check(spec(8, 8, B=3000), TIER_LDS)
    assert (want["status"] == OPTIMAL).all()


# ---- mixed outcomes, independence ------------------------------------------

def test_mixed_outcomes_in_one_batch_and_independence():
    s = spec(37, 70, construct="mixed")
    got, want = check(s, TIER_LDS)
    assert (want["status"][:4] == UNBOUNDED).all() and want["pivots"][:4].min() >= 1
    assert want["status"][4] == OPTIMAL and want["pivots"][4] == 0
    assert (want["status"][5:] == OPTIMAL).all() and want["pivots"][5:].min() >= 1
    # LP i of the batch = the same LP solved alone
    for i in (0, 4, 7):
        alone = bc.run_batch({**s, "only": i})
        for key in ("status", "pivots", "entering", "leaving", "basis"):
            assert np.array_equal(alone[key][0], got[key][i]), (i, key)
        assert np.array_equal(bc.bits(alone["objective"][0]), bc.bits(got["objective"][i]))
        assert np.array_equal(bc.bits(alone["rows"][0]), bc.bits(got["rows"][i]))
        lo = int(got["loglen"][:i].sum())
        assert np.array_equal(alone["logk"], got["logk"][lo:lo + int(got["loglen"][i])])


def test_budget_7_ends_every_lp_at_the_iteration_limit():
    got, want = check(spec(37, 70, budgets=[7]))
    assert (want["status"] == ITER_LIMIT).all() and (want["pivots"] == 7).all()


# ---- Bland, degeneracy, the log capacity -----------------------------------

def test_bland_degenerate():
    got, want = check(spec(33, 33, kind=GEN_DEGENERATE, rule=RULE_BLAND, reserve_log=50 * 66))
    assert want["pivots"].min() >= 50 and (want["loglen"] == want["pivots"]).all()


def test_bland_degenerate_long_mixed_run():
    got, want = check(spec(64, 64, kind=GEN_DEGENERATE, rule=RULE_BLAND, budgets=[6400], reserve_log=6400))
    assert set(want["status"].tolist()) == {OPTIMAL, ITER_LIMIT}
    assert (want["loglen"] == want["pivots"]).all()


def test_default_log_capacity_counts_but_does_not_record():
    s = spec(33, 33, kind=GEN_DEGENERATE, rule=RULE_BLAND)
    got, want = check(s)
    cap = 2 * (33 + bc.ncols_of(s))
    assert int(got["logcap"]) == cap
    over = want["pivots"] > cap
    assert over.any()
    assert (got["loglen"][over] == cap).all() and (got["pivots"][over] > cap).all()


@pytest.mark.parametrize("m,n", [(16, 16), (33, 33)])
def test_dantzig_degenerate(m, n):
    check(spec(m, n, kind=GEN_DEGENERATE))


# ---- continuation, chunks, the peek ----------------------------------------

CONTINUATION = [spec(37, 70, budgets=[7, 50 * 107]), spec(37, 70), spec(96, 160, budgets=[7, 50 * 256]),
                spec(33, 33, kind=GEN_DEGENERATE, rule=RULE_BLAND, budgets=[7, 3300], reserve_log=3400),
                spec(40, 24, kind=GEN_DUAL, dual=True, budgets=[3, 50 * 64])]


def test_two_calls_equal_one():
    got, _ = check(CONTINUATION[0])
    one, _ = check(CONTINUATION[1])
    assert (got["calls"][0] == ITER_LIMIT).all()
    for key in ("status", "pivots", "basis", "logk", "logr"):
        assert np.array_equal(got[key], one[key])
    assert np.array_equal(bc.bits(got["rows"]), bc.bits(one["rows"]))
    for s in CONTINUATION[2:]:
        check(s)


@pytest.mark.parametrize("chunk", [1, 3])
def test_small_chunks_equal_the_default(chunk, tmp_path):
    for s, got in zip(CONTINUATION, in_subprocess(CONTINUATION, {"LPG_BATCH_CHUNK": str(chunk)}, tmp_path)):
        assert int(got["chunk"]) == chunk
        bc.assert_same(got, oracle_of(s))


GLOBAL_CHUNKED = [spec(5, 6), spec(12, 20, kind=GEN_DUAL, dual=True),
                  spec(16, 16, kind=GEN_DEGENERATE, rule=RULE_BLAND, reserve_log=50 * 32)]


def test_global_tier_under_small_chunks(tmp_path):
    """Plain, dual and Bland on the global tier, resumed every 3 pivots."""
    env = {"LPG_BATCH_TIER": "global", "LPG_BATCH_CHUNK": "3"}
    for s, got in zip(GLOBAL_CHUNKED, in_subprocess(GLOBAL_CHUNKED, env, tmp_path)):
        assert int(got["tier"]) == TIER_GLOBAL and int(got["chunk"]) == 3
        bc.assert_same(got, oracle_of(s))


def test_budget_equal_to_the_pivot_count_reports_optimal():
    full = oracle_of(spec(37, 70))
    exact = int(full["pivots"].min())
    got, want = check(spec(37, 70, budgets=[exact]))
    first = int(np.argmin(full["pivots"]))
    assert got["status"][first] == OPTIMAL and got["pivots"][first] == exact
    assert (got["status"][full["pivots"] > exact] == ITER_LIMIT).all()


# ---- setters ---------------------------------------------------------------

def test_active_columns_and_tolerances_are_honoured():
    plain = oracle_of(spec(37, 70))
    got, want = check(spec(37, 70, nact=20))
    assert not np.array_equal(want["pivots"], plain["pivots"]) or not np.array_equal(want["logk"], plain["logk"])
    assert want["logk"].max() <= 20
    got, want = check(spec(37, 70, eps=[0.05, 0.5]))
    assert not np.array_equal(want["logk"], plain["logk"]) or not np.array_equal(want["logr"], plain["logr"])


# ---- dual ------------------------------------------------------------------

@pytest.mark.parametrize("m,n,tier", [(12, 20, TIER_LDS), (40, 24, TIER_LDS), (64, 64, TIER_LDS), (96, 160, TIER_GLOBAL)])
def test_dual(m, n, tier):
    got, want = check(spec(m, n, kind=GEN_DUAL, dual=True), tier)
    assert (want["status"] == OPTIMAL).all() and want["pivots"].min() >= 1


def test_dual_infeasible():
    got, want = check(spec(40, 24, kind=GEN_DUAL, dual=True, construct="dual_infeasible"))
    assert (want["status"] == INFEASIBLE).all() and want["pivots"].min() >= 1


def test_dual_refuses_a_batch_that_is_not_dual_feasible():
    import linearprogramming_amd as lpg
    with lpg.BatchEngine(8, 37, 108) as e:
        e.generate(70, bc.SEED, GEN_DENSE)
        before, basis = e.get_rows(), e.get_basis()
        with pytest.raises(lpg.LPGError, match=r"rc=-4.*LP 0 "):
            e.solve_dual(100)
        assert np.array_equal(bc.bits(e.get_rows()), bc.bits(before)) and np.array_equal(e.get_basis(), basis)
        assert all(len(e.get_log(b)[0]) == 0 for b in range(8))


def test_host_side_validation_on_a_live_batch():
    import linearprogramming_amd as lpg
    with lpg.BatchEngine(4, 5, 12) as e:
        T = np.zeros((4, 6, 12))
        for bad in (0, 12):
            with pytest.raises(lpg.LPGError, match="rc=-1.*basis"):
                e.load(T, np.full((4, 5), bad))
        with pytest.raises(lpg.LPGError, match="rc=-1"):
            e.load(T[:2], np.ones((2, 5)), first=3)            # LPs 3, 4 of 4
        with pytest.raises(lpg.LPGError, match="rc=-1"):
            e.get_log(4)
        with pytest.raises(lpg.LPGError, match="rc=-1"):
            e.get_rows(2, 3)
        with pytest.raises(lpg.LPGError, match="rc=-1"):
            e.generate(5, 1, GEN_DENSE)                        # ncols != n + m + 1
        with pytest.raises(lpg.LPGError, match="rc=-1"):
            e.generate(6, 1, 2)                                # artificial LPs need two phases
        with pytest.raises(lpg.LPGError, match="rc=-1"):
            e.solve(10, 7)
        with pytest.raises(lpg.LPGError, match="rc=-1"):
            e.set_active_columns(12)


# ---- generator -------------------------------------------------------------

@pytest.mark.parametrize("kind", [GEN_DENSE, GEN_DEGENERATE, GEN_DUAL])
@pytest.mark.parametrize("m,n", [(37, 70), (5, 6)])
def test_generator_equals_the_oracle(m, n, kind):
    import linearprogramming_amd as lpg
    with lpg.BatchEngine(8, m, n + m + 1) as e:
        e.generate(n, bc.SEED, kind)
        rows, basis = e.get_rows(), e.get_basis()
    for b in range(8):
        o = Oracle(m, n + m + 1)
        o.generate(n, bc.SEED + b, kind)
        assert np.array_equal(bc.bits(rows[b]), bc.bits(o.get_rows())), b
        assert np.array_equal(basis[b], o.get_basis()), b


# ---- the plain-C host ------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(CLI), reason="host/lpgcli not built")
@pytest.mark.parametrize("dual", [False, True])
def test_cli_batch(dual):
    p = subprocess.run([CLI, "--synthetic", "37", "70", "--batch", "16"] + (["--dual"] if dual else []),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    got = json.loads(lines[0])
    assert (got["m"], got["ncols"], got["batch"], got["tier"]) == (37, 108, 16, "lds")
    assert sum(got["statuses"].values()) == 16 and got["statuses"]["OPTIMAL"] == 16
    want = oracle_of(spec(37, 70, B=16, kind=GEN_DUAL if dual else GEN_DENSE, dual=dual, budgets=[1 << 40]))
    assert got["pivots"] == int(want["pivots"].sum())
    assert got["seconds"] > 0 and got["lps_per_s"] > 0 and got["pivots_per_s"] > 0
