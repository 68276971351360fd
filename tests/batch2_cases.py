"""Two-phase batch test plumbing (tests/test_gpu_batch_two_phase.py,
tests/batch_worker.py), in the style of tests/batch_cases.py.

A case is a JSON-able dict; run_batch(spec) runs it on the device through
BatchEngine.solve_two_phase, run_oracle(spec) runs every LP of it through
oracle.lpo.Oracle.solve_two_phase, one Oracle per LP, and
batch_cases.assert_same compares the two bit for bit: the status after every
call, pivot count, objective bits, last (entering, leaving), basis, the whole
log and the whole (m+1) x ncols tableau.

Every LP starts as the generator's artificial LP (kind 2, seed + LP index):
rows 0, 2, .. are `<= 0` rows with slacks, rows 1, 3, .. equalities with
artificials from art_first = 1 + n + ceil(m/2) on. spec keys: m, n, B, seed,
rule, budgets (one solve_two_phase call each; default [50 * (m + n)]),
construct, cost ("none": cost=None; "explicit": a cost array, different for
every LP, of pitch N + 3), only (solve LP `only` alone in a batch of 1).

construct, applied to LP b on the host (then the batch is loaded, not generated):
  "gen"           nothing (the device generator runs instead)
  "inconsistent"  row 3's structural part := row 1's, b_3 = b_1 + 1: infeasible
  "redundant"     row 3's [b | structural] := row 1's: one artificial stays basic at zero, no usable column
  "driveout"      rows 3 and 5: b = 0, structural part zero except -1 at structural column n resp. n - 1:
                  their artificials stay basic at zero after phase I and are driven out on negative pivots
  "mixed4"        LP b gets ("driveout", "inconsistent", "redundant", nothing)[b % 4]
"""
from __future__ import annotations

import numpy as np

import batch_cases as bc

SEED = bc.SEED
GEN_ARTIFICIAL = 2
OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, NUMERIC = 1, 2, 3, 4, 5


def spec(m, n, B=8, rule=0, **kw):
    s = {"m": m, "n": n, "B": B, "seed": SEED, "rule": rule, "budgets": [50 * (m + n)], "construct": "gen",
         "cost": "none", "only": None}
    s.update(kw)
    return s


def ncols_of(s):
    return s["n"] + s["m"] + 1


def art_first_of(s):
    return 1 + s["n"] + (s["m"] + 1) // 2


def _apply(T, m, n, what):
    if what == "inconsistent":
        T[3, 1:n + 1] = T[1, 1:n + 1]
        T[3, 0] = T[1, 0] + 1.0
    elif what == "redundant":
        T[3, :n + 1] = T[1, :n + 1]
    elif what == "driveout":
        for row, col in ((3, n), (5, n - 1)):
            T[row, :n + 1] = 0.0
            T[row, col] = -1.0
    elif what is not None:
        raise ValueError(what)


def build_tableaus(s):
    """(T[B, m+1, ncols], basis[B, m]) of the LPs before any pivot."""
    from oracle.lpo import Oracle
    m, n, B = s["m"], s["n"], s["B"]
    T = np.zeros((B, m + 1, ncols_of(s)))
    basis = np.zeros((B, m), dtype=np.int64)
    for b in range(B):
        o = Oracle(m, ncols_of(s))
        o.generate(n, s["seed"] + b, GEN_ARTIFICIAL)
        T[b], basis[b] = o.get_rows(), o.get_basis()
        o.close()
        c = s["construct"]
        _apply(T[b], m, n, ("driveout", "inconsistent", "redundant", None)[b % 4] if c == "mixed4" else
               (None if c == "gen" else c))
    if s["only"] is not None:
        T, basis = T[s["only"]:s["only"] + 1], basis[s["only"]:s["only"] + 1]
    return T, basis


def costs_of(s):
    """None, or the [B, N + 3] cost array: LP b's real costs on the structural columns, zeros elsewhere."""
    if s["cost"] == "none":
        return None
    assert s["cost"] == "explicit"
    N = ncols_of(s) - 1
    c = np.zeros((s["B"], N + 3))
    for b in range(s["B"]):
        c[b, :s["n"]] = [1.0 + ((7 * b + 3 * j) % 11) / 8.0 for j in range(s["n"])]
        c[b, N:] = 1e300                              # the padding is never read
    if s["only"] is not None:
        c = c[s["only"]:s["only"] + 1]
    return c


def run_batch(s):
    """The case on the device; also returns info.tier / chunk."""
    import linearprogramming_amd as lpg
    B = 1 if s["only"] is not None else s["B"]
    e = lpg.BatchEngine(B, s["m"], ncols_of(s))
    try:
        if s["construct"] == "gen" and s["only"] is None:
            af = e.generate_artificial(s["n"], s["seed"])
            assert af == art_first_of(s)
        else:
            e.load(*build_tableaus(s))
        cost = costs_of(s)
        return bc.solve_and_read_back(e, s["budgets"], lambda budget: e.solve_two_phase(art_first_of(s), cost, budget,
                                                                                        s["rule"]))
    finally:
        e.close()


def run_oracle(s):
    """Every LP of the case through Oracle.solve_two_phase, one at a time."""
    nc, cost = ncols_of(s), costs_of(s)
    T, basis = build_tableaus(s)
    return bc.oracle_loop(T, basis, s["budgets"], lambda o, b, budget: o.solve_two_phase(
        art_first_of(s), None if cost is None else cost[b, :nc - 1].copy(), budget, s["rule"]), 2 * (s["m"] + nc))


def phase_one(s):
    """Phase I of the first call replayed by hand on the oracle, per LP:
    (status, pivots, phase-I objective, rows whose basic artificial has a usable real column)."""
    from oracle.lpo import Oracle
    m, nc, af = s["m"], ncols_of(s), art_first_of(s)
    T, basis = build_tableaus(s)
    c1 = np.zeros(nc - 1)
    c1[af - 1:] = -1.0
    out = []
    for b in range(T.shape[0]):
        o = Oracle(m, nc)
        o.load_tableau(T[b], basis[b])
        o.set_objective(c1)
        r = o.solve(s["budgets"][0], s["rule"])
        R, bs = o.get_rows(), o.get_basis()
        usable = sum(1 for i in range(m) if bs[i] >= af and (np.abs(R[i, 1:af]) > 1e-9).any())
        out.append((r.status, r.pivots, r.objective, usable))
        o.close()
    return out
