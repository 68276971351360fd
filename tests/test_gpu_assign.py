"""Batches of assignment problems on the device (include/lpg.h, "assignment")
against the numpy restatement (tests/assign_cases.py), bit for bit on status,
col, u, v, objective and steps: every case kind at the shapes where the code
takes another path (the idle wave, the wave / workgroup line, the register /
LDS state line, the LDS / global tier line, the forced form and tier), the
generator, a second load, the front end, the simplex engine on the same
problems stated as LPs, and lpgcli --assign."""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pytest

import assign_cases as ac
from conftest import ROOT

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 0, 1
WAVE, WORKGROUP = 0, 1


def name(s):
    return f"{s['shape'][0]}x{s['shape'][1]}-{'max' if s['maximize'] else 'min'}"


def check(s, tier=None, form=None):
    got = ac.run_batch(s)
    ac.assert_same(got, ac.stacked(ac.reference(s)), name(s))
    if tier is not None:
        assert int(got["tier"]) == tier, name(s)
    if form is not None:
        assert int(got["form"]) == form, name(s)
    return got


@pytest.mark.parametrize("s", ac.SMALL, ids=name)
def test_seven_problems_leave_an_idle_wave(s):
    check(s, LDS, WAVE)


@pytest.mark.parametrize("s", ac.MIXED, ids=name)
def test_mixed_batch_whose_waves_end_at_different_steps(s):
    got = check(s, LDS, WAVE)
    assert got["status"][0] == ac.INFEASIBLE and (got["col"][0] == -1).all() and np.isnan(got["objective"][0])
    assert len(set(got["steps"].tolist())) >= 4


@pytest.mark.parametrize("s", ac.WAVE_LINE, ids=name)
def test_the_wave_workgroup_line(s):
    check(s, LDS, WAVE if s["shape"][1] <= 64 else WORKGROUP)


def test_64_columns_in_both_forms(tmp_path):
    specs = [ac.spec(64, 64), ac.spec(64, 64, True)]
    forced = ac.in_subprocess(specs, {"LPG_ASSIGN_FORM": "workgroup"}, tmp_path)
    for s, got in zip(specs, forced):
        assert int(got["form"]) == WORKGROUP and int(got["tier"]) == LDS
        ac.assert_same(got, ac.stacked(ac.reference(s)), name(s) + " workgroup form")
        ac.assert_same(got, check(s, LDS, WAVE), name(s) + " workgroup form against wave form")


@pytest.mark.parametrize("s", ac.STATE_LINE, ids=name)
def test_the_register_lds_state_line(s):
    check(s, GLOBAL, WORKGROUP)


@pytest.mark.parametrize("s", ac.TIER_LINE, ids=name)
def test_the_lds_global_tier_line(s):
    check(s, LDS if s["shape"][0] <= 138 else GLOBAL, WORKGROUP)


def test_forced_global_tier(tmp_path):
    for s, got in zip(ac.FORCED_GLOBAL, ac.in_subprocess(ac.FORCED_GLOBAL, {"LPG_ASSIGN_TIER": "global"}, tmp_path)):
        assert int(got["tier"]) == GLOBAL and int(got["form"]) == WORKGROUP
        ac.assert_same(got, ac.stacked(ac.reference(s)), name(s) + " global tier")


@pytest.mark.parametrize("s", ac.STATE_SPILL, ids=name)
def test_column_state_in_lds_and_beyond_it(s):
    import linearprogramming_amd as lpg
    got = check(s, GLOBAL, WORKGROUP)
    with lpg.AssignmentBatch(1, *s["shape"]) as a:
        # u alone where the 28 bytes a column no longer fit beside it
        assert (a.info.lds_bytes == 8 * s["shape"][0]) == (s["shape"][1] == 5500)
    assert (got["status"] == ac.OPTIMAL).all()


def test_generate_is_the_numpy_statement_of_the_generator():
    import linearprogramming_amd as lpg
    from oracle import lpo
    count, nr, nc, seed, rng = 5, 5, 7, 20220518, 10
    C = np.array([[[np.floor(lpo.uniform(seed + q, i * nc + j) * rng) for j in range(nc)] for i in range(nr)]
                  for q in range(count)])
    assert C.min() == 0 and C.max() == rng - 1
    for mx in (False, True):
        with lpg.AssignmentBatch(count, nr, nc, maximize=mx) as a:
            a.generate(seed, rng)
            res = a.solve()
            col, u, v = a.get()
        want = ac.stacked([ac.hungarian(c, mx) for c in C])
        got = {"status": np.array([r.status for r in res]), "steps": np.array([r.steps for r in res]),
               "objective": np.array([r.objective for r in res]), "col": col, "u": u, "v": v}
        ac.assert_same(got, want, f"generate max={mx}")


def test_a_second_load_and_solve_on_the_same_batch():
    import linearprogramming_amd as lpg
    first, second = ac.spec(5, 7, seed=1), ac.spec(5, 7, seed=2)
    with lpg.AssignmentBatch(7, 5, 7) as a:
        for s in (first, second):
            a.load(ac.costs_of(s))
            res = a.solve()
            col, u, v = a.get()
            got = {"status": np.array([r.status for r in res]), "steps": np.array([r.steps for r in res]),
                   "objective": np.array([r.objective for r in res]), "col": col, "u": u, "v": v}
            ac.assert_same(got, ac.stacked(ac.reference(s)), f"load {s['seed']}")
        # one problem replaced: the others solve as before
        a.load(ac.costs_of(first)[3:4], first=3)
        res = a.solve()
        want = ac.reference(second)
        want[3] = ac.reference(first)[3]
        assert [(r.status, r.steps, r.objective) for r in res] == [(w["status"], w["steps"], w["objective"]) for w in want]
        part = a.get(first=3, n=2)
        assert (part[0] == np.stack([want[3]["col"], want[4]["col"]])).all()


def test_frontend_solves_a_mixed_list_in_input_order():
    from linearprogramming_amd import frontend
    rng = np.random.default_rng(5)
    shapes = [(3, 3), (3, 5), (5, 3), (3, 3), (1, 4), (70, 66), (3, 5)]
    mats = [ac.problem("int3" if k % 2 else "inf30", nr, nc, rng) for k, (nr, nc) in enumerate(shapes)]
    for mx in (False, True):
        sols = frontend.solve_assignment(mats, maximize=mx)
        assert len(sols) == len(mats)
        for C, sol in zip(mats, sols):
            tr = C.shape[0] > C.shape[1]
            r = ac.hungarian(C.T if tr else C, mx)
            assert sol.status == ("OPTIMAL" if r["status"] == ac.OPTIMAL else "INFEASIBLE")
            assert sol.steps == r["steps"]
            assert np.array([sol.objective]).view(np.uint64) == np.array([r["objective"]]).view(np.uint64)
            if tr:
                asg = np.full(C.shape[0], -1, dtype=np.int64)
                if r["status"] == ac.OPTIMAL:
                    asg[r["col"]] = np.arange(C.shape[1])
                u, v = r["v"], r["u"]
            else:
                asg, u, v = r["col"], r["u"], r["v"]
            assert sol.assignment.shape == (C.shape[0],) and (sol.assignment == asg).all()
            assert (sol.u.view(np.uint64) == u.view(np.uint64)).all() and sol.u.shape == (C.shape[0],)
            assert (sol.v.view(np.uint64) == v.view(np.uint64)).all() and sol.v.shape == (C.shape[1],)
            if sol.status == "OPTIMAL":
                picked = sol.assignment >= 0
                assert C[np.arange(C.shape[0])[picked], sol.assignment[picked]].sum() == sol.objective


@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("mx", [False, True], ids=["min", "max"])
def test_the_simplex_engine_agrees_on_the_assignment_lp(n, mx):
    """The route a caller had before: n^2 columns, 2 n equality rows, 2 n artificials, two phases. The constraint
    matrix is totally unimodular, so with integer costs every tableau entry is an integer and the objective exact."""
    import linearprogramming_amd as lpg
    B = 16
    rng = np.random.default_rng([n, int(mx)])
    C = rng.integers(0, 50, size=(B, n, n)).astype(np.float64)
    m, nx = 2 * n, n * n
    ncols = 1 + nx + m
    T = np.zeros((B, m + 1, ncols))
    T[:, :m, 0] = 1.0
    for i in range(n):
        for j in range(n):
            T[:, i, 1 + i * n + j] = 1.0            # row i is assigned once
            T[:, n + j, 1 + i * n + j] = 1.0        # column j is used once
    for r in range(m):
        T[:, r, 1 + nx + r] = 1.0
    basis = np.tile(np.arange(1 + nx, 1 + nx + m, dtype=np.int64), (B, 1))
    cost = np.zeros((B, ncols - 1))
    cost[:, :nx] = (C if mx else -C).reshape(B, nx)                # the engine maximises
    with lpg.BatchEngine(B, m, ncols) as e:
        e.load(T, basis)
        lp = e.solve_two_phase(1 + nx, cost)
        xb = e.get_rows()[:, :m, 0]
    with lpg.AssignmentBatch(B, n, n, maximize=mx) as a:
        a.load(C)
        res = a.solve()
    for q in range(B):
        assert lp[q].status == lpg.OPTIMAL and res[q].status == lpg.OPTIMAL
        assert (lp[q].objective if mx else -lp[q].objective) == res[q].objective, q
        assert np.isin(xb[q], (0.0, 1.0)).all(), (q, xb[q])


def fnv1a(h, data: bytes) -> int:
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("mx", [False, True], ids=["min", "max"])
def test_lpgcli_assign_counts_and_digest_equal_pythons(mx):
    import linearprogramming_amd as lpg
    nr = nc = 8
    B, seed = 64, 20220518
    cli = os.path.join(ROOT, "host", "lpgcli")
    p = subprocess.run([cli, "--assign", str(nr), str(nc), "--batch", str(B), "--seed", str(seed)] + (["--max"] if mx else []),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    with lpg.AssignmentBatch(B, nr, nc, maximize=mx) as a:
        a.generate(seed, 100)
        res = a.solve()
        col, u, v = a.get()
    assert (line["nr"], line["nc"], line["batch"], line["tier"], line["form"]) == (nr, nc, B, "lds", "wave")
    assert line["sense"] == ("max" if mx else "min")
    assert line["statuses"] == {"OPTIMAL": sum(r.status == lpg.OPTIMAL for r in res),
                                "INFEASIBLE": sum(r.status == 3 for r in res)}
    assert line["statuses"]["OPTIMAL"] == B
    assert line["steps"] == sum(r.steps for r in res)
    h = 0xcbf29ce484222325
    for arr in (col, u, v):
        h = fnv1a(h, arr.tobytes())
    assert line["digest"] == f"{h:016x}"
