"""Batches of 0-1 programs on the device (include/lpg.h, "0-1 programs")
against the numpy statement (tests/binary_cases.py), bit for bit on status,
found, objective, x and nodes: every problem kind across the census shapes
(tests/test_binary_cases.py checks the list), both senses, both tiers, the
three rows-per-lane instantiations, small chunks, budget steps, splits, the
generator, the front end and lpgcli --binary."""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

import binary_cases as bc
from conftest import ROOT

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 0, 1


def check(s, tier=None, rpl=None):
    got = bc.run_batch(s)
    bc.assert_same(got, bc.stacked(bc.reference(s)), bc.name(s))
    if tier is not None:
        assert int(got["tier"]) == tier, bc.name(s)
    if rpl is not None:
        assert int(got["rows_per_lane"]) == rpl, bc.name(s)
    return got


@pytest.mark.parametrize("s", bc.SMALL + bc.ONE, ids=bc.name)
def test_every_kind_at_small_shapes(s):
    got = check(s, LDS, 1)
    assert int(got["chunk"]) == 4096 and int(got["launches"]) == 1


@pytest.mark.parametrize("s", bc.MANY, ids=bc.name)
def test_131_problems_whose_waves_end_at_different_nodes(s):
    got = check(s, LDS, 1)
    assert len(set(got["nodes"].tolist())) >= 10 and set(got["status"].tolist()) == {bc.OPTIMAL, bc.INFEASIBLE}


@pytest.mark.parametrize("s", bc.CENSUS, ids=bc.name)
def test_the_census_shapes(s):
    m, n = s["shape"]
    got = check(s, LDS if 4 * 8 * (m * n + n) <= 150 * 1024 else GLOBAL, 1 if m <= 64 else 2 if m <= 128 else 4)
    k = s["kinds"]
    assert got["status"][k.index("inf_row")] == bc.INFEASIBLE and (got["x"][k.index("inf_row")] == -1).all()
    assert got["status"][k.index("inf_combo")] == bc.INFEASIBLE and np.isnan(got["objective"][k.index("inf_combo")])
    assert got["nodes"][k.index("first")] == 1 and got["status"][k.index("first")] == bc.OPTIMAL


@pytest.mark.parametrize("s", bc.DEEP, ids=bc.name)
def test_searches_of_several_launches(s):
    got = check(s, None, 1)
    assert int(got["launches"]) == -(-int(got["nodes"].max()) // 4096) and int(got["launches"]) >= 2


def test_every_instantiation_ran():
    """Rows per lane 1, 2, 4 in both tiers: the census covers five of the six, RPL4_LDS the last."""
    seen = set()
    for s in bc.CENSUS[::2] + bc.RPL4_LDS:
        got = check(s)
        seen.add((int(got["rows_per_lane"]), int(got["tier"])))
    assert seen == {(r, t) for r in (1, 2, 4) for t in (LDS, GLOBAL)} - {(1, GLOBAL)}
    # (1, GLOBAL) arises only when forced: test_forced_global_tier


def test_forced_global_tier(tmp_path):
    for s, got in zip(bc.FORCED_GLOBAL, bc.in_subprocess(bc.FORCED_GLOBAL, {"LPG_BINARY_TIER": "global"}, tmp_path)):
        assert int(got["tier"]) == GLOBAL and int(got["lds_bytes"]) == 0
        bc.assert_same(got, bc.stacked(bc.reference(s)), bc.name(s) + " global tier")
    assert int(bc.in_subprocess(bc.FORCED_GLOBAL[:1], {"LPG_BINARY_TIER": "global"}, tmp_path)[0]["rows_per_lane"]) == 1


@pytest.mark.parametrize("chunk", [1, 3])
def test_small_chunks_end_in_the_same_bits(tmp_path, chunk):
    for s, got in zip(bc.CHUNKED, bc.in_subprocess(bc.CHUNKED, {"LPG_BINARY_CHUNK": str(chunk)}, tmp_path)):
        assert int(got["chunk"]) == chunk
        want = bc.stacked(bc.reference(s))
        bc.assert_same(got, want, bc.name(s) + f" chunk {chunk}")
        longest = max(r["nodes"] for r in _sub_references(s))
        assert int(got["launches"]) == -(-longest // chunk)


def _sub_references(s):
    """enumerate01 of every sub-search of spec s (the launches of a solve follow the longest one)."""
    A, sense, rhs, c = bc.data_of(s)
    return [bc.enumerate01(A[q], sense[q], rhs[q], c[q], s["maximize"], tuple((k >> t) & 1 for t in range(s["split"])))
            for q in range(len(A)) for k in range(1 << s["split"])]


@pytest.mark.parametrize("s", bc.BUDGETED, ids=bc.name)
def test_a_solve_in_budget_steps(s):
    """max_nodes 1, then 7, then none: each intermediate result is the statement cut at the same count, the end
    the one-call result."""
    got = bc.run_batch(dict(s, budgets=list(bc.BUDGET_STEPS)))
    used = 0
    for k, step in enumerate(bc.BUDGET_STEPS):
        used += step
        want = bc.stacked(bc.reference(s, used if step else 0))
        bc.assert_same(got, want, bc.name(s) + f" after step {k}", prefix=f"step{k}_")
    one_call = check(s)
    bc.assert_same(got, one_call, bc.name(s) + " steps against one call")
    assert (got["step0_status"] == bc.ITER_LIMIT).any() and (got["step1_status"] == bc.ITER_LIMIT).any()
    cut = got["step0_status"] == bc.ITER_LIMIT
    assert np.isnan(got["step0_objective"][cut & (got["step0_found"] == 0)]).all()
    assert (got["step0_x"][cut & (got["step0_found"] == 0)] == -1).all()


@pytest.mark.parametrize("s", bc.CUT_ONLY, ids=bc.name)
def test_a_search_that_does_not_end_is_cut(s):
    got = bc.run_batch(s)
    bc.assert_same(got, bc.stacked(bc.reference(s, s["budgets"][0])), bc.name(s))
    assert (got["status"] == bc.ITER_LIMIT).all() and (got["nodes"] == s["budgets"][0]).all()


@pytest.mark.parametrize("s", bc.SPLITS, ids=bc.name)
def test_splits_agree_on_objective_and_x(s):
    got = check(s)
    whole = bc.stacked(bc.reference(dict(s, split=0)))
    for f in ("status", "found", "x"):
        assert (got[f] == whole[f]).all(), f
    assert (got["objective"].view(np.uint64) == whole["objective"].view(np.uint64)).all()
    if s["split"] == s["shape"][1]:
        assert (got["nodes"] == 1 << s["split"]).all()           # every sub-search is a single leaf


def test_a_second_load_resets_the_searches():
    import linearprogramming_amd as lpg
    first, second = bc.spec(5, 7, seed=1), bc.spec(5, 7, seed=2)
    with lpg.BinaryBatch(9, 5, 7) as b:
        b.load(*bc.data_of(first))
        b.solve(3)                                               # left in mid-search
        b.load(*bc.data_of(second))
        bc.assert_same(bc.results_of(b.solve(), b.get()), bc.stacked(bc.reference(second)), "second load")
        again = b.solve()                                        # nothing is running: nothing moves
        bc.assert_same(bc.results_of(again, b.get()), bc.stacked(bc.reference(second)), "solve again")
        assert b.info.launches == 0
        assert (b.get(first=3, n=2) == bc.stacked(bc.reference(second))["x"][3:5]).all()


@pytest.mark.parametrize("m,n", [(1, 1), (5, 3), (40, 9), (70, 64)])
def test_generate_is_the_numpy_statement_of_the_generator(m, n):
    import linearprogramming_amd as lpg
    count, seed = 5, 20220518
    for mx in (False, True):
        with lpg.BinaryBatch(count, m, n, maximize=mx) as b:
            b.generate(seed)
            got = bc.results_of(b.solve(), b.get())
        want = bc.stacked([bc.enumerate01(*bc.generate(m, n, seed + q)[:4], mx) for q in range(count)])
        bc.assert_same(got, want, f"generate {m}x{n} max={mx}")
        assert (got["status"] == bc.OPTIMAL).all()


def test_frontend_solves_mixed_shapes_in_input_order():
    from linearprogramming_amd import frontend
    rng = np.random.default_rng(5)
    shapes = [(3, 5), (40, 33), (3, 5), (1, 1), (70, 64), (40, 33), (6, 12)]
    kinds = ["mixed", "banded", "cover", "first", "banded", "equal", "knapsack"]
    models = [bc.problem(k, m, n, rng) for k, (m, n) in zip(kinds, shapes)]
    for mx in (False, True):
        for split in (None, 1):
            sols = frontend.solve_binary(models, maximize=mx, split=split)
            assert len(sols) == len(models)
            for (A, sense, rhs, c), sol in zip(models, sols):
                perm = frontend.binary_order(c, "cost")
                assert (np.abs(c[perm])[:-1] >= np.abs(c[perm])[1:]).all()
                r = bc.enumerate01(A[:, perm], sense, rhs, c[perm], mx)
                x = np.full(len(c), -1, dtype=np.int8)
                x[perm] = r["x"]
                assert sol.status == {bc.OPTIMAL: "OPTIMAL", bc.INFEASIBLE: "INFEASIBLE"}[r["status"]]
                assert np.array([sol.objective]).view(np.uint64) == np.array([r["objective"]]).view(np.uint64)
                assert (sol.x == x).all()
    s0 = frontend.solve_binary(models, order=None, split=0)
    for (A, sense, rhs, c), sol in zip(models, s0):
        r = bc.enumerate01(A, sense, rhs, c)
        assert sol.nodes == r["nodes"] and (sol.x == r["x"]).all()
    # split=None: the smallest split that fills the device, from the occupancy query
    import linearprogramming_amd as lpg
    sp = frontend.binary_split(1, 70, 64)
    with lpg.BinaryBatch(1, 70, 64, split=sp) as b:
        waves = b.resident_waves
    assert waves > 0 and waves % 4 == 0
    assert sp == 10 or (1 << sp) >= waves
    if sp > 0:
        with lpg.BinaryBatch(1, 70, 64, split=sp - 1) as b:
            assert (1 << (sp - 1)) < b.resident_waves
    assert frontend.binary_split(1 << 20, 3, 5) == 0


def test_text_model_on_the_device():
    from linearprogramming_amd import frontend
    text = "OF {\n\tmax:z=8x1+11x2+6x3+4x4\n}\nST {\n\t5x1+7x2+4x3+3x4<=14;\n\tx1>=0\n}\n"
    sol = frontend.solve_binary_text(text)
    assert sol.status == "OPTIMAL" and sol.objective == 21.0 and (sol.x == [0, 1, 1, 1]).all()
    assert sol.names == ["x1", "x2", "x3", "x4"]


def fnv1a(h, data: bytes) -> int:
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("mx,split,max_nodes", [(False, 0, 0), (True, 2, 0), (False, 1, 40)], ids=["min", "max-split2", "cut40"])
def test_lpgcli_binary_counts_and_digest_equal_pythons(mx, split, max_nodes):
    import linearprogramming_amd as lpg
    m, n, B, seed = 40, 33, 37, 20220518
    cli = os.path.join(ROOT, "host", "lpgcli")
    p = subprocess.run([cli, "--binary", str(m), str(n), "--batch", str(B), "--seed", str(seed), "--split", str(split),
                        "--max-nodes", str(max_nodes)] + (["--max"] if mx else []), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    with lpg.BinaryBatch(B, m, n, split=split, maximize=mx) as b:
        b.generate(seed)
        res = b.solve(max_nodes)
        x = b.get()
        info = b.info
    assert (line["m"], line["n"], line["batch"], line["split"], line["tier"], line["rows_per_lane"]) == (m, n, B, split, "lds", 1)
    assert line["sense"] == ("max" if mx else "min") and line["chunk"] == info.chunk and line["launches"] == info.launches
    assert line["statuses"] == {name: sum(r.status == code for r in res)
                                for name, code in (("OPTIMAL", 1), ("INFEASIBLE", 3), ("ITER_LIMIT", 4))}
    assert line["statuses"]["INFEASIBLE"] == 0 and (line["statuses"]["ITER_LIMIT"] > 0) == (max_nodes > 0)
    assert line["nodes"] == sum(r.nodes for r in res) and line["found"] == sum(r.found for r in res)
    assert line["digest"] == f"{fnv1a(0xcbf29ce484222325, x.tobytes()):016x}"
    want = bc.stacked([bc.enumerate_split(*bc.generate(m, n, seed + q)[:4], mx, split, max_nodes) for q in range(B)])
    bc.assert_same(bc.results_of(res, x), want, "lpgcli's batch")
