"""Batches of transportation problems on the device (include/lpg.h,
"transportation") against the numpy statement (tests/transport_cases.py), bit
for bit on status, iterations, objective, x, u, v and basis: the shapes where
the code takes another path (the node cap, the wave / workgroup line, a
thread's stride over the cells, the LDS / global tier line, the forced form
and tier), both rules, both starts, both senses, degenerate data, budgets and
chunks, the generator, the front end, and the other device routes to the same
optimum (AssignmentBatch, BatchEngine.solve_two_phase, lpgcli --transport)."""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

import transport_cases as tc
from conftest import ROOT

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 0, 1
WAVE, WORKGROUP = 0, 1


def check(s, tier=None, form=None):
    got = tc.run_batch(s)
    tc.assert_same(got, tc.stacked(tc.reference(s)), tc.name(s))
    if tier is not None:
        assert int(got["tier"]) == tier, tc.name(s)
    if form is not None:
        assert int(got["form"]) == form, tc.name(s)
    return got


@pytest.mark.parametrize("s", tc.SMALL, ids=tc.name)
def test_seven_problems_leave_an_idle_wave(s):
    got = check(s, LDS, WAVE)
    assert (got["status"] == tc.OPTIMAL).all()


@pytest.mark.parametrize("s", tc.CAP, ids=tc.name)
def test_the_node_cap(s):
    got = check(s, GLOBAL, WORKGROUP)              # 32 bytes a node take 128 KiB: C stays in device memory
    assert (got["status"] == tc.OPTIMAL).all()


@pytest.mark.parametrize("s", tc.FORM_LINE, ids=tc.name)
def test_the_wave_workgroup_line(s):
    check(s, LDS, WAVE if sum(s["shape"]) <= 64 else WORKGROUP)


def test_the_workgroup_form_forced_below_the_line(tmp_path):
    forced = tc.in_subprocess(tc.FORCED_WORKGROUP, {"LPG_TRANSPORT_FORM": "workgroup"}, tmp_path)
    for s, got in zip(tc.FORCED_WORKGROUP, forced):
        assert int(got["form"]) == WORKGROUP and int(got["tier"]) == LDS
        tc.assert_same(got, tc.stacked(tc.reference(s)), tc.name(s) + " workgroup form")


@pytest.mark.parametrize("s", tc.STRIDE_LINE, ids=tc.name)
def test_the_stride_boundaries_of_the_pricing_sweep(s):
    check(s, LDS)


@pytest.mark.parametrize("s", tc.TIER_LINE, ids=tc.name)
def test_the_lds_global_tier_line(s):
    check(s, LDS if s["shape"][0] <= 134 else GLOBAL, WORKGROUP)


def test_forced_global_tier(tmp_path):
    for s, got in zip(tc.FORCED_GLOBAL, tc.in_subprocess(tc.FORCED_GLOBAL, {"LPG_TRANSPORT_TIER": "global"}, tmp_path)):
        assert int(got["tier"]) == GLOBAL and int(got["form"]) == WORKGROUP
        tc.assert_same(got, tc.stacked(tc.reference(s)), tc.name(s) + " global tier")


@pytest.mark.parametrize("s", tc.UNIT + tc.UNIT_BLAND, ids=tc.name)
def test_unit_squares_agree_with_the_statement_and_with_the_assignment_batch(s):
    import linearprogramming_amd as lpg
    got = check(s)
    assert (got["status"] == tc.OPTIMAL).all()
    C = tc.data_of(s)[0]
    with lpg.AssignmentBatch(C.shape[0], C.shape[1], C.shape[2], maximize=s["maximize"]) as a:
        a.load(C)
        res = a.solve()
    assert [r.objective for r in res] == got["objective"].tolist()


@pytest.mark.parametrize("s", tc.MIXED, ids=tc.name)
def test_mixed_batch_whose_problems_end_after_different_iteration_counts(s):
    got = check(s, LDS, WAVE)
    assert got["iterations"][0] == 0 and len(set(got["iterations"].tolist())) >= 4


@pytest.mark.parametrize("s", tc.BUDGETS, ids=tc.name)
def test_split_budgets_end_in_the_bits_of_one_call(s):
    got = check(s)
    assert (got["status"] == tc.OPTIMAL).all()
    tc.assert_same(got, tc.stacked(tc.reference(dict(s, budgets=None))), tc.name(s) + " against one call")


@pytest.mark.parametrize("s", tc.CUT, ids=tc.name)
def test_a_budget_that_cuts_mid_solve(s):
    got = check(s)
    assert (got["status"] == tc.ITER_LIMIT).any()
    cut = got["status"] == tc.ITER_LIMIT
    assert (got["iterations"][cut] == sum(s["budgets"])).all()


@pytest.mark.parametrize("chunk", [1, 7])
def test_small_chunks_through_the_environment(chunk, tmp_path):
    for s, got in zip(tc.CHUNKED, tc.in_subprocess(tc.CHUNKED, {"LPG_TRANSPORT_CHUNK": str(chunk)}, tmp_path)):
        assert int(got["chunk"]) == chunk
        tc.assert_same(got, tc.stacked(tc.reference(s)), tc.name(s) + f" chunk {chunk}")
        # a launch applies at most `chunk` iterations and prices once more: the last one finds the optimum
        assert int(got["launches"]) == max(1, -(-int(got["iterations"].max()) // chunk))


def test_generate_is_the_numpy_statement_of_the_generator():
    import linearprogramming_amd as lpg
    from oracle import lpo
    count, nr, nc, seed, rng, qmax = 6, 5, 7, 20220518, 10, 6
    C = np.array([[[np.floor(lpo.uniform(seed + q, i * nc + j) * rng) for j in range(nc)] for i in range(nr)]
                  for q in range(count)])
    S = np.array([[1 + np.floor(lpo.uniform(seed + q, nr * nc + i) * qmax) for i in range(nr)] for q in range(count)])
    D = np.array([[1 + np.floor(lpo.uniform(seed + q, nr * nc + nr + j) * qmax) for j in range(nc)] for q in range(count)])
    for q in range(count):
        diff = S[q].sum() - D[q].sum()
        if diff > 0:
            D[q, -1] += diff
        else:
            S[q, -1] -= diff
    assert C.min() == 0 and C.max() == rng - 1 and S.min() >= 1 and (S.sum(axis=1) == D.sum(axis=1)).all()
    for mx in (False, True):
        with lpg.TransportBatch(count, nr, nc, maximize=mx) as t:
            t.generate(seed, rng, qmax)
            res = t.solve()
            x, u, v, basis = t.get()
        want = tc.stacked([tc.solve(C[q], S[q], D[q], mx) for q in range(count)])
        got = {"status": np.array([r.status for r in res]), "iterations": np.array([r.iterations for r in res]),
               "objective": np.array([r.objective for r in res]), "x": x, "u": u, "v": v, "basis": basis}
        tc.assert_same(got, want, f"generate max={mx}")


def test_a_second_load_resets_only_the_problems_it_writes():
    import linearprogramming_amd as lpg
    first, second = tc.spec(5, 7, seed=1), tc.spec(5, 7, seed=2)
    with lpg.TransportBatch(7, 5, 7) as t:
        t.load(*tc.data_of(first))
        t.solve()
        C, S, D = tc.data_of(second)
        t.load(C[3:5], S[3:5], D[3:5], first=3)
        res = t.solve()
        x, u, v, basis = t.get()
    want = list(tc.reference(first))
    want[3:5] = tc.reference(second)[3:5]
    got = {"status": np.array([r.status for r in res]), "iterations": np.array([r.iterations for r in res]),
           "objective": np.array([r.objective for r in res]), "x": x, "u": u, "v": v, "basis": basis}
    tc.assert_same(got, tc.stacked(want), "second load")


def test_the_simplex_engine_agrees_on_the_transportation_lp():
    """The route a caller had before: nr nc columns, nr + nc equality rows, as many artificials, two phases. The
    constraint matrix is totally unimodular and the data are integers, so the LP's objective is exact as well."""
    import linearprogramming_amd as lpg
    nr, nc, B = 4, 5, 8
    s = tc.spec(nr, nc, seed=7, kinds=("c2", "c99", "zeros", "big", "c99", "c2", "big", "const"))
    C, S, D = tc.data_of(s)
    m, nx = nr + nc, nr * nc
    ncols = 1 + nx + m
    T = np.zeros((B, m + 1, ncols))
    T[:, :nr, 0], T[:, nr:m, 0] = S, D
    for i in range(nr):
        for j in range(nc):
            T[:, i, 1 + i * nc + j] = 1.0
            T[:, nr + j, 1 + i * nc + j] = 1.0
    for r in range(m):
        T[:, r, 1 + nx + r] = 1.0
    basis = np.tile(np.arange(1 + nx, 1 + nx + m, dtype=np.int64), (B, 1))
    cost = np.zeros((B, ncols - 1))
    cost[:, :nx] = -C.reshape(B, nx)                               # the engine maximises
    with lpg.BatchEngine(B, m, ncols) as e:
        e.load(T, basis)
        lp = e.solve_two_phase(1 + nx, cost)
    got = check(s)
    for q in range(B):
        assert lp[q].status == lpg.OPTIMAL and got["status"][q] == tc.OPTIMAL
        assert -lp[q].objective == got["objective"][q], q


def test_frontend_on_unbalanced_mixed_shapes_and_a_forbidden_route():
    from linearprogramming_amd import frontend
    inf = float("inf")
    rng = np.random.default_rng(11)
    models = [
        (rng.integers(0, 20, size=(3, 4)), [5, 6, 7], [4, 4, 4, 4]),            # 2 units of supply stay
        (rng.integers(0, 20, size=(3, 4)), [3, 3, 3], [4, 4, 4, 4]),            # 7 units of demand are not served
        (rng.integers(0, 20, size=(5, 2)), [1, 2, 3, 4, 5], [7, 8]),            # balanced, another shape
        ([[1, inf], [inf, 1]], [3, 4], [3, 4]),                                 # forbidden routes, feasible
        ([[1, inf], [inf, 1]], [3, 4], [4, 3]),                                 # the optimum needs a forbidden route
        (rng.integers(0, 20, size=(3, 4)), [5, 6, 7], [4, 4, 4, 6]),            # balanced 3 x 4
    ]
    sols = frontend.solve_transportation(models)
    assert [s.status for s in sols] == ["OPTIMAL", "OPTIMAL", "OPTIMAL", "OPTIMAL", "INFEASIBLE", "OPTIMAL"]
    for (C, s, d), sol in zip(models, sols):
        C, s, d = np.asarray(C, dtype=np.float64), np.asarray(s, dtype=np.float64), np.asarray(d, dtype=np.float64)
        assert sol.x.shape == C.shape and sol.u.shape == s.shape and sol.v.shape == d.shape
        if sol.status != "OPTIMAL":
            assert np.isnan(sol.objective)
            continue
        assert (sol.x.sum(axis=1) + sol.unused == s).all() and (sol.x.sum(axis=0) + sol.unmet == d).all()
        assert sol.objective == (np.where(sol.x > 0, C, 0.0) * sol.x).sum()
        # the statement on the model with its dummy line gives the same optimum
        diff = s.sum() - d.sum()
        Cd = np.where(np.isinf(C), 1000.0, C)
        if diff > 0:
            Cd, d = np.hstack([Cd, np.zeros((len(s), 1))]), np.append(d, diff)
        elif diff < 0:
            Cd, s = np.vstack([Cd, np.zeros((1, len(d)))]), np.append(s, -diff)
        assert tc.solve(Cd, s, d)["objective"] == sol.objective
    assert sols[0].unused.sum() == 2 and sols[0].unmet.sum() == 0
    assert sols[1].unmet.sum() == 7 and sols[1].unused.sum() == 0
    assert sols[3].objective == 7.0
    mx = frontend.solve_transportation(models[:3], maximize=True)
    for k, ((C, s, d), sol) in enumerate(zip(models[:3], mx)):
        assert sol.status == "OPTIMAL" and sol.objective == (np.asarray(C, dtype=np.float64) * sol.x).sum()
        assert sol.objective >= sols[k].objective


def fnv1a(h, data: bytes) -> int:
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("mx,nw,bland", [(False, False, False), (True, True, True)], ids=["min-lc-dantzig", "max-nw-bland"])
def test_lpgcli_transport_counts_and_digest_equal_pythons(mx, nw, bland):
    import linearprogramming_amd as lpg
    nr, nc, B, seed = 6, 9, 37, 20220518
    cli = os.path.join(ROOT, "host", "lpgcli")
    args = [cli, "--transport", str(nr), str(nc), "--batch", str(B), "--seed", str(seed), "--range", "20", "--qmax", "5"]
    args += (["--max"] if mx else []) + (["--start", "nw"] if nw else []) + (["--rule", "bland"] if bland else [])
    p = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    with lpg.TransportBatch(B, nr, nc, maximize=mx, start="northwest" if nw else "least_cost") as t:
        t.generate(seed, 20, 5)
        res = t.solve(rule=lpg.RULE_BLAND if bland else lpg.RULE_DANTZIG)
        x, u, v, basis = t.get()
    assert (line["nr"], line["nc"], line["batch"], line["tier"], line["form"]) == (nr, nc, B, "lds", "wave")
    assert (line["sense"], line["start"], line["rule"]) == ("max" if mx else "min", "northwest" if nw else "least_cost",
                                                            "bland" if bland else "dantzig")
    assert line["statuses"] == {"OPTIMAL": B, "ITER_LIMIT": 0} and all(r.status == lpg.OPTIMAL for r in res)
    assert line["iterations"] == sum(r.iterations for r in res) > 0
    h = 0xcbf29ce484222325
    for arr in (x, u, v, basis):
        h = fnv1a(h, arr.tobytes())
    assert line["digest"] == f"{h:016x}"
