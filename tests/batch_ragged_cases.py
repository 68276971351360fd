"""Ragged-batch test plumbing (tests/test_gpu_batch_ragged.py,
tests/batch_worker.py), in the style of tests/batch_cases.py.

A case is a JSON-able dict; run_batch(spec) runs it on the device through
BatchEngine.ragged, run_oracle(spec) runs every LP of it through an
oracle.lpo.Oracle of its own, and batch_cases.assert_same compares the two bit
for bit: the status after every call, pivot count, objective bits, last
(entering, leaving), basis, the whole log and the whole tableau. The LPs have
different shapes, so "rows" and "basis" are the packed arrays: LP after LP,
each dense.

spec keys:
  lps      one [m, n, seed, construct] per LP, in batch order: LP = the generator's
           LP of n structural columns and m rows (ncols = n + m + 1) with that
           seed, then `construct` applied on the host
  kind     "plain"  generator kind 0, solve(budget, rule)
           "dual"   generator kind 3, solve_dual(budget)
           "art"    generator kind 2 (artificials from 1 + n + ceil(m/2) on), solve_two_phase
           "bigm"   the same LPs with a zero M row, in a Big-M batch, solve_big_m
  rule, budgets (one solve call each), cost ("none" / "explicit", for "art" and "bigm")

construct: None; "plain": "ray" (structural column 1 negated in every
constraint row: UNBOUNDED), "optimal" (a non-negative objective row: OPTIMAL
at once); "dual": "dual_infeasible" (d_1 = -1); "art" / "bigm":
batch2_cases' "inconsistent", "redundant", "driveout".
"""
from __future__ import annotations

import json

import numpy as np

import batch2_cases as b2
import batch_cases as bc

SEED = bc.SEED
GEN = {"plain": 0, "dual": 3, "art": 2, "bigm": 2}
LDS_CAP, LDS_CU = 150 * 1024, 160 * 1024


def lps_of(shapes, constructs=None, seed=SEED):
    """[m, n, seed + q, construct] for shapes[q] = (m, n)."""
    constructs = constructs or {}
    return [[m, n, seed + q, constructs.get(q)] for q, (m, n) in enumerate(shapes)]


def spec(lps, kind="plain", rule=0, budgets=None, cost="none"):
    return {"lps": [list(x) for x in lps], "kind": kind, "rule": rule, "budgets": budgets or [20000], "cost": cost}


def nobj_of(s):
    return 2 if s["kind"] == "bigm" else 1


def lds_bytes(m, ncols, nobj=1):
    """include/lpg.h: [tableau of m + nobj rows at pitch ncols | 1] P C [int32 basis], in bytes."""
    rows = m + nobj
    return 8 * (ncols + rows + rows * (ncols | 1) + (m + 1) // 2)


def group_of(lds, tier):
    """The launch group of an LP by the rule of include/lpg.h: 0 on the global tier, 1 on the LDS tier."""
    return 0 if tier == 1 or lds > LDS_CAP else 1


def fit_on_a_cu(lds):
    """Workgroups of `lds` bytes of LDS that fit on a CU: 160 KiB, and at most eight workgroups of four waves."""
    return min(8, LDS_CU // lds)


def art_first_of(m, n):
    return 1 + n + (m + 1) // 2


def build_lp(s, q):
    """(T[m + nobj, ncols], basis[m]) of LP q before any pivot."""
    from oracle.lpo import Oracle
    m, n, seed, construct = s["lps"][q]
    nc = n + m + 1
    o = Oracle(m, nc)
    o.generate(n, seed, GEN[s["kind"]])
    T, basis = o.get_rows(), o.get_basis()
    o.close()
    if construct == "ray":
        T[:m, 1] *= -1.0
    elif construct == "optimal":
        T[m, :] = np.abs(T[m, :])
    elif construct == "dual_infeasible":
        T[m, 1] = -1.0
    elif construct is not None:
        b2._apply(T, m, n, construct)
    if s["kind"] == "bigm":
        T2 = np.zeros((m + 2, nc))
        T2[:m], T2[m + 1] = T[:m], T[m]
        T = T2
    return T, basis


def cost_of(s, q):
    """None, or LP q's [N] real costs: on the structural columns, zeros elsewhere (Big-M: 7.0 at the artificials,
    which the method must take as 0)."""
    if s["cost"] == "none":
        return None
    m, n = s["lps"][q][:2]
    c = np.zeros(n + m)
    c[:n] = [1.0 + ((7 * q + 3 * j) % 11) / 8.0 for j in range(n)]
    if s["kind"] == "bigm":
        c[art_first_of(m, n) - 1:] = 7.0
    return c


def logcap_of(s):
    """The default log capacity of the batch: 2 * (max m + max ncols)."""
    return 2 * (max(x[0] for x in s["lps"]) + max(x[0] + x[1] + 1 for x in s["lps"]))


def _solver(s, q):
    m, n = s["lps"][q][:2]
    cost = cost_of(s, q)
    cc = (lambda: None if cost is None else cost.copy())
    if s["kind"] == "plain":
        return lambda o, b, budget: o.solve(budget, s["rule"])
    if s["kind"] == "dual":
        return lambda o, b, budget: o.solve_dual(budget)
    if s["kind"] == "art":
        return lambda o, b, budget: o.solve_two_phase(art_first_of(m, n), cc(), budget, s["rule"])
    return lambda o, b, budget: o.solve_big_m(art_first_of(m, n), cc(), budget, s["rule"])


def _merge(parts):
    out = {}
    for key in ("status", "pivots", "objective", "entering", "leaving", "loglen", "logk", "logr"):
        out[key] = np.concatenate([p[key] for p in parts])
    out["rows"] = np.concatenate([p["rows"].ravel() for p in parts])
    out["basis"] = np.concatenate([p["basis"].ravel() for p in parts])
    out["calls"] = np.concatenate([p["calls"] for p in parts], axis=1)
    out["logcap"] = parts[0]["logcap"]
    return out


_ORACLE = {}


def run_oracle(s):
    """Every LP of the case through an Oracle of its own (computed once per spec; do not modify the result)."""
    key = json.dumps(s, sort_keys=True)
    if key not in _ORACLE:
        parts = []
        for q in range(len(s["lps"])):
            T, basis = build_lp(s, q)
            parts.append(bc.oracle_loop(T[None], basis[None], s["budgets"], _solver(s, q), logcap_of(s), nobj=nobj_of(s)))
        _ORACLE[key] = _merge(parts)
    return _ORACLE[key]


def engine_for(s):
    """The loaded ragged BatchEngine of the case."""
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine.ragged([(m, n + m + 1) for m, n, _, _ in s["lps"]], big_m=s["kind"] == "bigm")
    built = [build_lp(s, q) for q in range(len(s["lps"]))]
    e.load([T for T, _ in built], [b for _, b in built])
    return e


def solve_fn(e, s):
    """budget -> one solve call of the case's kind on the ragged BatchEngine e."""
    n = len(s["lps"])
    af = [art_first_of(m, nn) for m, nn, _, _ in s["lps"]]
    costs = None if s["cost"] == "none" else [cost_of(s, q) for q in range(n)]
    if s["kind"] == "plain":
        return lambda budget: e.solve(budget, s["rule"])
    if s["kind"] == "dual":
        return lambda budget: e.solve_dual(budget)
    if s["kind"] == "art":
        return lambda budget: e.solve_two_phase(af, costs, budget, s["rule"])
    return lambda budget: e.solve_big_m(af, costs, budget, s["rule"])


def read_back(e, res, calls):
    """batch_cases._pack's dict (rows and basis packed) plus every LP's tier, lds_bytes and group, and info's chunk."""
    info = e.info
    out = bc._pack(res, np.concatenate([r.ravel() for r in e.get_rows()]), np.concatenate(e.get_basis()),
                   [e.get_log(q) for q in range(e.count)], calls, info.log_capacity)
    shp = [e.shape(q) for q in range(e.count)]
    out["tier"] = np.array([x.tier for x in shp], dtype=np.int64)
    out["lds"] = np.array([x.lds_bytes for x in shp], dtype=np.int64)
    out["group"] = np.array([x.group for x in shp], dtype=np.int64)
    out["chunk"] = np.array(info.chunk, dtype=np.int64)
    return out


def run_batch(s):
    """The case on the device."""
    e = engine_for(s)
    try:
        solve, calls = solve_fn(e, s), []
        for budget in s["budgets"]:
            res = solve(budget)
            calls.append([r.status for r in res])
        return read_back(e, res, calls)
    finally:
        e.close()


def in_subprocess(specs, env, tmp_path):
    return bc.in_subprocess("batch_ragged_cases", specs, env, tmp_path)
