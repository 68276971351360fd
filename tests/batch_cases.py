"""Batch-solver test plumbing (tests/test_gpu_batch.py, tests/batch_worker.py).

A case is a JSON-able dict ("spec"); run_batch(spec) runs it on the device
through BatchEngine, run_oracle(spec) runs every LP of it through the CPU
oracle, one Oracle per LP, and assert_same compares the two bit for bit:
status, pivot count, objective bits, last (entering, leaving), basis, the
whole log and the whole (m+1) x ncols tableau. Both return the same dict of
arrays, so a device run made in a fresh subprocess (another tier, another
chunk) travels back as an .npz file.

spec keys: m, n, B, kind (generator), seed, rule, budgets (one solve call
each; default [50 * (m + n)]), dual, construct ("gen": the device generator;
"mixed", "kat", "dual_infeasible": tableaus built on the host by
build_tableaus and loaded), reserve_log, nact, eps ([eps_piv, eps_opt]),
only (solve LP `only` alone in a batch of 1).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

SEED = 20220518


def spec(m, n, B=8, kind=0, rule=0, **kw):
    s = {"m": m, "n": n, "B": B, "kind": kind, "seed": SEED, "rule": rule, "budgets": [50 * (m + n)], "dual": False,
         "construct": "gen", "reserve_log": None, "nact": None, "eps": None, "only": None}
    s.update(kw)
    return s


def ncols_of(s):
    return s["n"] + s["m"] + 1


def build_tableaus(s):
    """(T[B, m+1, ncols], basis[B, m]) of the LPs before any pivot."""
    from oracle.lpo import Oracle
    m, n, B = s["m"], s["n"], s["B"]
    T = np.zeros((B, m + 1, ncols_of(s)))
    basis = np.zeros((B, m), dtype=np.int64)
    for b in range(B):
        o = Oracle(m, ncols_of(s))
        o.generate(n, s["seed"] + b, s["kind"])
        T[b], basis[b] = o.get_rows(), o.get_basis()
        o.close()
    c = s["construct"]
    if c == "mixed":
        # LPs 0..3: structural column 1 + b negated in every constraint row (a ray: UNBOUNDED);
        # LP 4: a non-negative objective row (OPTIMAL at once); the rest plain
        for b in range(4):
            T[b, :m, 1 + b] *= -1.0
        T[4, m, :] = np.abs(T[4, m, :])
    elif c == "kat":
        # LP 1: Source/testdata.txt with `max:` (z* = 12), as __graft_entry__.smoke() loads it
        assert (m, n) == (2, 2)
        T[1] = np.array([[51 / 14, 1, 9 / 14, 1, 0], [1 / 3, 2, -1, 0, 1], [0, -1, -1, 0, 0]])
        basis[1] = [3, 4]
    elif c == "dual_infeasible":
        # LP b: row b's structural entries made non-negative: b_b < 0 with no negative entry left
        for b in range(B):
            T[b, b, 1:n + 1] = np.abs(T[b, b, 1:n + 1])
    elif c != "gen":
        raise ValueError(c)
    if s["only"] is not None:
        T, basis = T[s["only"]:s["only"] + 1], basis[s["only"]:s["only"] + 1]
    return T, basis


def _pack(results, rows, basis, logs, calls, logcap):
    return {
        "status": np.array([r.status for r in results], dtype=np.int64),
        "pivots": np.array([r.pivots for r in results], dtype=np.int64),
        "objective": np.array([r.objective for r in results], dtype=np.float64),
        "entering": np.array([r.entering for r in results], dtype=np.int64),
        "leaving": np.array([r.leaving for r in results], dtype=np.int64),
        "rows": rows, "basis": basis,
        "loglen": np.array([len(k) for k, _ in logs], dtype=np.int64),
        "logk": np.concatenate([k for k, _ in logs] + [np.zeros(0, dtype=np.int64)]),
        "logr": np.concatenate([r for _, r in logs] + [np.zeros(0, dtype=np.int64)]),
        "calls": np.array(calls, dtype=np.int64),          # [call, LP] -> status after that call
        "logcap": np.array(logcap, dtype=np.int64),
    }


def in_subprocess(cases, specs, env, tmp_path):
    """run_batch of module `cases` on every spec, on the device in a fresh process under `env` (tests/batch_worker.py)."""
    sp, out = tmp_path / "specs.json", tmp_path / "out.npz"
    sp.write_text(json.dumps(specs))
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "batch_worker.py")
    p = subprocess.run([sys.executable, worker, cases, str(sp), str(out)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, **env})
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(out)
    return [{k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(f"{i}/")} for i in range(len(specs))]


def solve_and_read_back(e, budgets, solve, info_keys=("tier", "chunk")):
    """solve(budget) once per budget on BatchEngine e, then the read-back: _pack's dict plus info's `info_keys`."""
    calls = []
    for budget in budgets:
        res = solve(budget)
        calls.append([r.status for r in res])
    info = e.info
    out = _pack(res, e.get_rows(), e.get_basis(), [e.get_log(b) for b in range(len(res))], calls, info.log_capacity)
    for key in info_keys:
        out[key] = np.array(getattr(info, key), dtype=np.int64)
    return out


def oracle_loop(T, basis, budgets, solve, logcap, prepare=None, nobj=1):
    """LP b of (T, basis) through an Oracle of its own: load, prepare(o), solve(o, b, budget) once per budget;
    then _pack's dict, the log clipped to `logcap` (the batch records the first `capacity` pivots)."""
    from oracle.lpo import Oracle
    m, nc = T.shape[1] - nobj, T.shape[2]
    results, rows, bas, logs, calls = [], [], [], [], [[] for _ in budgets]
    for b in range(T.shape[0]):
        o = Oracle(m, nc, nobj=nobj)
        o.load_tableau(T[b], basis[b])
        if prepare is not None:
            prepare(o)
        for c, budget in enumerate(budgets):
            r = solve(o, b, budget)
            calls[c].append(r.status)
        results.append(r)
        rows.append(o.get_rows())
        bas.append(o.get_basis())
        k, rr = o.get_log()
        logs.append((k[:logcap], rr[:logcap]))
        o.close()
    return _pack(results, np.array(rows), np.array(bas), logs, calls, logcap)


def run_batch(s):
    """The case on the device; also returns info.tier / chunk."""
    import linearprogramming_amd as lpg
    B = 1 if s["only"] is not None else s["B"]
    e = lpg.BatchEngine(B, s["m"], ncols_of(s))
    try:
        if s["construct"] == "gen" and s["only"] is None:
            e.generate(s["n"], s["seed"], s["kind"])
        else:
            e.load(*build_tableaus(s))
        if s["reserve_log"] is not None:
            e.reserve_log(s["reserve_log"])
        if s["nact"] is not None:
            e.set_active_columns(s["nact"])
        if s["eps"] is not None:
            e.set_tolerances(*s["eps"])
        return solve_and_read_back(e, s["budgets"], lambda budget: e.solve_dual(budget) if s["dual"] else
                                   e.solve(budget, s["rule"]))
    finally:
        e.close()


def run_oracle(s):
    """Every LP of the case through oracle.lpo.Oracle, one at a time."""
    def prepare(o):
        if s["nact"] is not None:
            o.set_active_columns(s["nact"])
        if s["eps"] is not None:
            o.set_tolerances(*s["eps"])

    T, basis = build_tableaus(s)
    logcap = s["reserve_log"] if s["reserve_log"] is not None else 2 * (s["m"] + ncols_of(s))
    return oracle_loop(T, basis, s["budgets"], lambda o, b, budget: o.solve_dual(budget) if s["dual"] else
                       o.solve(budget, s["rule"]), logcap, prepare)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same(got, want):
    for key in ("calls", "status", "pivots", "entering", "leaving", "basis", "logcap", "loglen", "logk", "logr"):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    assert np.array_equal(bits(got["objective"]), bits(want["objective"])), "objective bits"
    diff = np.argwhere(bits(got["rows"]) != bits(want["rows"]))
    assert diff.size == 0, ("tableau differs first at [LP, row, column]", diff[0].tolist())
