"""lpg.Engine where its decision code has to break ties, sit on a tolerance or
meet a non-finite entry (tests/engine_tie_cases.py), bit for bit against the
CPU oracle: the status after every call, status, pivot count, objective bits,
basis, the whole log and all m + nobj rows by batch_cases.bits (so -0 and +0
differ), no tolerance anywhere. On a row partition: every rank's log and
basis, the replicated objective rows and the stacked row blocks.

The generator's LPs never tie, so on them the tie-breaking arms never run:
k_pivot_block's fetch of the records that share the least key (every record
form: PK1, Big-M's two objective rows, Bland's j-keyed records), rec_min /
key_less on the ratio records, the t == 0 hand-over from k_select_d, region
mode's spare slots, the second lane bank; the second stage of k_prep_d /
k_select_d, of the generic pair (LPG_SLOW_PIVOT=1) and of the eager kernels;
dual_cand / ratio_cand and the d_j <= 0 arm of the dual; the exchange of the
ranks' best candidates. The interval LPs here tie at most pivots and are
exact, and tests/test_engine_tie_cases.py counts on the CPU that each case
ties across every boundary of the engine's geometry that its shape has. The
two-phase and Big-M interval LPs all end INFEASIBLE (phase I / the M part
decides), so phase II and the drive-out see no ties here.

Every path asserts through e.info that it is the path it claims to be
(engine_tie_cases.info_checks) and that no persistent launch fell back.

Column skipping. The engine's update kernels leave alone every column whose
pivot-row entry P_j is zero, where the oracle computes fma(-C_i, P_j, t) for
every entry. These cases found the two places where that is not the same
bits: t = -0 becomes +0 unless the product is -0 too (the dual makes -0s:
P_j = 0 / negative pivot, and the -A it is loaded with), and with a
non-finite C_i the product is NaN (likewise the column trade writes the
columns that entered the basis as unit vectors). On every dual path the rows
differed from the oracle's in the sign of zeros (779 .. 22372 entries a run,
nothing else), and nan_ratio_stride kept numbers where the oracle has NaN
(first at row 1, column 22). The engine now updates every column once a
context has loaded a -0 or a non-finite entry or runs the dual (lpg_ctx.hip
exact_mode), so the default configuration is held to the bits here, and
LPG_NO_SKIP=1 is run beside it on the cases that found it.
"""
from __future__ import annotations

import numpy as np
import pytest

import engine_tie_cases as ec
import tie_cases as tc

pytestmark = pytest.mark.gpu

CASES = ec.cases()
SKIPPING = (None, ec.NO_SKIP)              # the default column skipping, and LPG_NO_SKIP=1


@pytest.fixture(scope="module", autouse=True)
def lpg():
    import linearprogramming_amd as lpg
    lpg.load()
    assert lpg.device_count() >= 1, "no GPU visible"
    return lpg


def _rows(s, extra_env, nonfinite=False):
    """How the rows are compared: by their bits, everywhere."""
    return "bits"


def _single(s, path, block=None, extra_env=None, rows=None):
    block = ec.block_of(s, path) if block is None else block
    want = tc.run_oracle(s)
    for q in range(2):
        got, info = ec.run_single(s, q, path, block, extra_env=extra_env)
        ec.assert_same(got, ec.lp_of(want, q), rows=rows or _rows(s, extra_env))
        if path == "dual-wide":
            assert 0 < got["pivots"][0] < block
        elif block:
            assert got["pivots"][0] > 2 * block      # at least two whole blocks
        if path in ("region", "split-region") and s["method"] != "big_m":
            assert info.region == 1, "the loaded tableau left region mode"


# ---- interval LPs: every case on every single-rank path that takes its method ----

def _interval_params():
    """The forced split on the region slices repeats, for two-phase, what "split" and "region" cross, and Big-M has
    no region slices (it asserts region == 0 there): `extended`; the primal cases keep every path."""
    out = []
    for s in CASES:
        for path in ec.paths_of(s):
            extra = path == "split-region" and s["method"] in ("two_phase", "big_m")
            out.append(pytest.param(s, path, id=f"{ec.case_id(s)}-{path}", marks=pytest.mark.extended if extra else ()))
    return out


@pytest.mark.parametrize("s,path", _interval_params())
def test_interval_lps(s, path):
    """dual-wide: the dual inside one partial block of 128 (its logs are 30 pivots at most), so no whole block is
    covered there and neither is the two-bank prefetch of k_dual_row_d, which starts at 64 pending pivots; the
    host's flow around a 128-pivot block and the read-out's flush of a partial one are."""
    for extra_env in SKIPPING if s["method"] == "dual" else SKIPPING[:1]:
        _single(s, path, extra_env=extra_env)


@pytest.mark.parametrize("path", ["persistent", "split", "pair"])
@pytest.mark.parametrize("s", ec.two_bank_cases(), ids=ec.case_id)
def test_interval_lps_second_lane_bank(s, path):
    """Blocks of 80 pivots: from 65 pending slots on the per-slot scalars take a second lane bank."""
    _single(s, path, ec.TWO_BANK_BLOCK)


# ---- interrupted runs: the tied decisions arrive through the t == 0 hand-over and the slice reload ----

PIECES = (5, 9, "b", 17, 1, 2, "b", 7, 3, 11, 33, 40)
RESUMED = [("dual", 0, "dual-deferred"), ("dual", 0, "dual-eager"), ("two_phase", 0, "region"),
           ("two_phase", 1, "persistent"), ("big_m", 0, "persistent"), ("big_m", 1, "pair")]


@pytest.mark.parametrize("path", ["persistent", "region", "pair"])
@pytest.mark.parametrize("rule", [tc.RULE_DANTZIG, tc.RULE_BLAND])
def test_primal_in_enqueued_pieces(rule, path):
    """lpg_enqueue in pieces of 5, 9, 17, ... pivots with reads of column 0 in between (each flushes inside a
    block): every launch after the first starts at a pending index > 0; lpg_solve finishes the run."""
    s = ec.case(*ec.LARGE, "primal", rule)
    want = tc.run_oracle(s)
    for q in range(2):
        n, pieces = int(want["loglen"][q]), []
        for p in PIECES:                              # stop short of the end: the solve call takes the last pivots
            if p != "b" and sum(x for x in pieces if x != "b") + p > n - 3:
                break
            pieces.append(p)
        assert sum(x for x in pieces if x != "b") > ec.block_of(s, path) and "b" in pieces
        got, _ = ec.run_single(s, q, path, pieces=pieces)
        ec.assert_same(got, ec.lp_of(want, q))


def _resumed(method, rule, path, extra_env=None, rows=None):
    s = ec.case(*ec.LARGE, method, rule)
    for q in range(2):
        want = ec.oracle_resumed(s, q)
        assert want["calls"][0, 0] == tc.ITER_LIMIT and want["calls"][-1, 0] != tc.ITER_LIMIT
        got, _ = ec.run_single(s, q, path, budgets=ec.RESUME_BUDGETS, explicit_costs=True, extra_env=extra_env)
        ec.assert_same(got, want, rows=rows or _rows(s, extra_env))


@pytest.mark.parametrize("method,rule,path", RESUMED)
def test_methods_in_budget_limited_calls(method, rule, path):
    """The dual, two-phase and Big-M have no enqueue: repeated budget-limited calls instead (tests/test_dual.py's
    test_gpu_dual_budget_and_resume), the costs passed to every call, the status after every call compared too.
    Each call settles the pending block, so the next starts from a flushed tableau inside what one long call runs
    as one block. tests/test_engine_tie_cases.py checks that the oracle so continued ends where one call ends."""
    for extra_env in SKIPPING if method == "dual" else SKIPPING[:1]:
        _resumed(method, rule, path, extra_env)


# ---- entries that sit on a tolerance ----------------------------------------

def _boundaries(s, extra_env=None, rows=None):
    want = tc.run_oracle(s)
    paths = {"dual-eager": {"LPG_DEFER": "0"}, "dual-deferred": {"LPG_DEFER": "8"}} if s["method"] == "dual" else \
        {"default": {}, "pair": {"LPG_PERSIST": "0"}, "eager": {"LPG_DEFER": "0"}}
    for name, env in paths.items():
        for q in range(s["B"]):
            T, basis = tc.build_lp(s, q)
            got, info = ec.solve_lp(T, basis, s, {**env, **(extra_env or {})}, s["budgets"], eps=s["eps"])
            if s["method"] != "dual":
                assert (info.pivot_wg > 0) == (name == "default"), name
            assert (info.defer_k == 0) == (name in ("eager", "dual-eager")), name
            ec.assert_same(got, ec.lp_of(want, q), rows=rows or _rows(s, extra_env))


@pytest.mark.parametrize("s", tc.boundary_cases(), ids=tc.case_id)
def test_tolerance_boundaries(s):
    """All 8 LPs of every boundary spec, one Engine each, lpg_set_tolerances as the spec says: reduced costs (the
    dual: right-hand sides) of exactly -eps_opt, pivot-column (pivot-row) entries of exactly eps_piv. The default
    path, the pair and eager; the dual eager and deferred."""
    for extra_env in SKIPPING if s["method"] == "dual" else SKIPPING[:1]:
        _boundaries(s, extra_env)


# ---- non-finite entries ------------------------------------------------------

NAN_PATHS = ["persistent", "split", "pair", "generic", "eager"]


def _nan_ratio_row_block(rule, path, extra_env=None, rows=None):
    s = tc.nonfinite_spec("nan_ratio_stride", rule)
    T, basis = tc.nonfinite_batch("nan_ratio_stride")
    m, n = tc.NONFINITE["nan_ratio_stride"][:2]
    rw = ec.slice_widths(m, n + m + 1, ec.SPLIT_WG)[0]
    assert 1 // ec.D_ROWS != 257 // ec.D_ROWS and 1 // rw != 257 // rw
    shape = dict(s, m=m, n=n)
    block = 0 if path == "eager" else 32
    got, _ = ec.solve_lp(T[tc.BAD_LP], basis[tc.BAD_LP], shape, {**ec.env_of(shape, path, block), **(extra_env or {})},
                         s["budgets"], path, block)
    w = ec.lp_of(tc.run_oracle(s), tc.BAD_LP)
    assert (w["logk"][0], w["logr"][0]) == (1, 257) and np.isnan(w["rows"]).any()
    ec.assert_same(got, w, nonfinite=True, rows=rows or _rows(s, extra_env, nonfinite=True))


@pytest.mark.parametrize("path", NAN_PATHS)
@pytest.mark.parametrize("rule", [tc.RULE_DANTZIG, tc.RULE_BLAND])
def test_nan_ratio_in_another_row_block(rule, path):
    """tie_cases' nan_ratio_stride on the engine: the NaN row is 1 and the best row 257, in different row blocks of
    k_select_d and different slices of k_pivot_block; the NaN ratio loses."""
    for extra_env in SKIPPING:
        _nan_ratio_row_block(rule, path, extra_env)


def _nan_ratio_rank(extra_env=None, rows=None):
    T, basis, s = ec.nan_ratio_across_ranks()
    w = ec.oracle_lp(T, basis, s)
    assert (w["logk"][0], w["logr"][0]) == (1, 40) and np.isnan(w["rows"]).any()
    parts = ec.run_threads(T, basis, s, 2, 8, budget=s["budgets"][0], extra_env=extra_env)
    ec.assert_ranks_same(parts, w, 70, 2, 8, nonfinite=True, rows=rows or _rows(s, extra_env, nonfinite=True))


def test_nan_ratio_in_another_rank():
    """Over ranks the block-end column trade is on by default, and it writes the columns that entered the basis as
    unit vectors without computing them, where the oracle's arithmetic puts a NaN into the NaN row: the ranks agree
    to leave it off once one of them has loaded a non-finite entry."""
    _nan_ratio_rank()
    _nan_ratio_rank({**ec.NO_SKIP, "LPG_NO_REORDER": "1"})


def _dual_nonfinite(case, block, extra_env=None, rows=None):
    if case == "wide":
        T, basis, s = ec.dual_nan_ratio_across_column_blocks()
        w = ec.oracle_lp(T, basis, s)
    else:
        s = tc.nonfinite_spec(case)
        Tb, bb = tc.nonfinite_batch(case)
        T, basis, w = Tb[tc.BAD_LP], bb[tc.BAD_LP], ec.lp_of(tc.run_oracle(s), tc.BAD_LP)
    got, info = ec.solve_lp(T, basis, s, {"LPG_DEFER": str(block), **(extra_env or {})}, s["budgets"])
    assert info.defer_k == block
    ec.assert_same(got, w, nonfinite=True, rows=rows or _rows(s, extra_env, nonfinite=True))
    assert not np.isfinite(w["rows"]).all() and w["pivots"][0] >= 1


@pytest.mark.parametrize("block", [0, 8])
@pytest.mark.parametrize("case", ["dual_inf_b", "dual_nan_ratio_stride", "wide"])
def test_dual_nonfinite(case, block):
    """b_7 = -inf, and a NaN ratio d_j / -a_rj = +inf / +inf that must lose to the least ratio, which sits in the
    same thread's stride (column 258) or, "wide", in another column block (column 600 of 700), through
    Engine.solve_dual, eager and deferred."""
    for extra_env in SKIPPING:
        _dual_nonfinite(case, block, extra_env)


# ---- the row partition -------------------------------------------------------

@pytest.fixture
def shared_gpu(monkeypatch):
    """As tests/test_gpu_dist.py: the ranks of these tests share one GPU, and say so."""
    monkeypatch.setenv("LPG_PUSH_SHARED_QUEUES", "1")
    monkeypatch.setenv("LPG_PUSH_SHARED_DEVICE", "1")


def _threads(method, rule, world, extra_env=None, rows=None):
    s = ec.case(*ec.SMALL, method, rule)
    block = ec.block_of(s, "dual-deferred" if method == "dual" else "pair")
    want = tc.run_oracle(s)
    for q in range(2):
        T, basis = tc.build_lp(s, q)
        parts = ec.run_threads(T, basis, s, world, block, extra_env=extra_env)
        assert all(p["wg"] == 0 for p in parts)
        ec.assert_ranks_same(parts, ec.lp_of(want, q), s["m"], world, block, rows=rows or _rows(s, extra_env))
        assert parts[0]["pivots"] > 2 * block


@pytest.mark.parametrize("world", ec.WORLDS)
@pytest.mark.parametrize("method,rule", tc.METHODS)
def test_ranks_as_threads(method, rule, world):
    """(70, 150) over 2 and 3 ranks, every rank a thread with the whole tableau loaded, the candidates exchanged
    through the host collectives: a theta tie between two ranks is decided by the key in the second stage, where
    the winner must be its owner's own minimum."""
    for extra_env in SKIPPING if method == "dual" else SKIPPING[:1]:
        _threads(method, rule, world, extra_env)


@pytest.mark.parametrize("method,rule,world,mr", ec.PUSH_CASES)
def test_ranks_as_processes_with_the_owner_push(shared_gpu, method, rule, world, mr):
    """Separate processes, the owner push attached: by default k_pivot_block's multi-rank form (the ranks' best
    candidates through xpush_best), LPG_PERSIST_MR=0 the pair around the push. The dual attaches the push and does
    not use it, as in tests/test_gpu_dist.py."""
    s = ec.case(*ec.SMALL, method, rule)
    block = ec.block_of(s, "dual-deferred" if method == "dual" else "pair")
    parts = ec.run_processes(s, 0, world, block, mr)
    ec.assert_ranks_same(parts, ec.lp_of(tc.run_oracle(s), 0), s["m"], world, block)
    assert all(p["exchange"] in (1, 2) for p in parts)
    if method != "dual":
        assert all((p["wg"] > 0) == (mr is None) for p in parts) and len({p["wg"] for p in parts}) == 1
    assert parts[0]["pivots"] > 2 * block


# ---- when the engine skips columns --------------------------------------------

def test_columns_are_skipped_until_a_signed_zero_or_the_dual():
    """lpg_ctx.hip exact_mode: a tableau loaded without -0 and without non-finite entries keeps column skipping
    (fewer bytes updated than with LPG_NO_SKIP=1, the same log); one -0 among the loaded entries, or the dual,
    and the context updates every column, as LPG_NO_SKIP=1 does."""
    import linearprogramming_amd as lpg

    def run(T, basis, env, dual=False):
        with ec.environment({"LPG_DEFER": "0", **env}):
            e = lpg.Engine(basis.shape[0], T.shape[1])
        try:
            e.load_rows(0, T)
            e.set_basis(basis)
            e.set_timing(True)
            e.get_timing()
            res = e.solve_dual(20000) if dual else e.solve(20000, 0)
            return e.get_timing().update_bytes, res.pivots, [x.tolist() for x in e.get_log()]
        finally:
            e.close()

    s = ec.case(*ec.SMALL, "primal", 0)
    T, basis = tc.build_lp(s, 0)
    signed = T.copy()
    i, j = np.argwhere(T[:s["m"], 1:s["n"] + 1] == 0.0)[0]
    signed[i, 1 + j] = -0.0
    clean, every, after_zero = run(T, basis, {}), run(T, basis, ec.NO_SKIP), run(signed, basis, {})
    assert clean[1:] == every[1:] == after_zero[1:] and clean[1] > 16
    assert 0 < clean[0] < every[0] == after_zero[0]
    d = ec.case(*ec.SMALL, "dual", 0)
    T, basis = tc.build_lp(d, 0)
    assert run(T, basis, {}, dual=True) == run(T, basis, ec.NO_SKIP, dual=True)
