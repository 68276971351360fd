"""Big-M batch test plumbing (tests/test_gpu_batch_big_m.py,
tests/batch_worker.py), in the style of tests/batch2_cases.py.

A case is a JSON-able dict; run_batch(spec) runs it on the device through a
Big-M BatchEngine and solve_big_m, run_oracle(spec) runs every LP of it
through oracle.lpo.Oracle(m, ncols, nobj=2).solve_big_m, one Oracle per LP, and
batch_cases.assert_same compares the two bit for bit: the status after every
call, pivot count, objective bits, last (entering, leaving), basis, the whole
log and the whole (m+2) x ncols tableau.

The generated LPs are batch2_cases.build_tableaus' (the generator's artificial
LP, seed + LP index, then `construct` applied on the host) with the objective
row moved to row m + 1 and a zero M row m. spec keys: m, n, B, seed, rule,
budgets (one solve_big_m call each; default [50 * (m + n)]), construct, cost,
only (solve LP `only` alone in a batch of 1), art_first (None: the
generator's 1 + n + ceil(m/2)).

construct: batch2_cases' ("gen", "inconsistent", "redundant", "driveout",
"mixed4"), or one of the small literal batches of tests/test_big_m.py:
  "inf_ray"  B copies of INF_RAY (infeasible, with a ray of the real objective), art_first 3
  "a5_inf"   A5, INF, A5, INF, ... (optimal at z = 6 / infeasible), art_first 4

cost: "none" (cost=None: -1 x row m + 1 as it stands at the call) or
"explicit": a cost array of pitch N + 3, different for every LP; its entries
at the artificial columns are 7.0 (the method must take them as 0) and its
padding 1e300 (never read).
"""
from __future__ import annotations

import numpy as np

import batch2_cases as b2
import batch_cases as bc

SEED = bc.SEED
OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, NUMERIC = 1, 2, 3, 4, 5

# tests/test_big_m.py's tableaus: [b | x1 x2 | ...], rows 2 and 3 the (empty) M and real objective rows
# A5: max x1 + 2 x2; x1 + x2 = 3; x1 - x2 <= 1
A5 = np.array([[3.0, 1, 1, 0, 1], [1.0, 1, -1, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
INF = np.array([[2.0, 1, 1, 0, 1], [1.0, 1, 1, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
# max x1; x2 = 1, x2 = 2 (artificials a1, a2): infeasible, and x1's column (0, 0)
# is a ray of the real objective once the M part is optimal (a2 = 1 left)
INF_RAY = np.array([[1.0, 0, 1, 1, 0], [2.0, 0, 1, 0, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
LITERAL = {"inf_ray": ([INF_RAY], [[3, 4]], [[1.0, 0.0, 0.0, 0.0]], 3),
           "a5_inf": ([A5, INF], [[4, 3], [4, 3]], [[1.0, 2.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]], 4)}


def spec(m, n, B=8, rule=0, **kw):
    s = {"m": m, "n": n, "B": B, "seed": SEED, "rule": rule, "budgets": [50 * (m + n)], "construct": "gen",
         "cost": "none", "only": None, "art_first": None}
    s.update(kw)
    return s


def literal(construct, B=4, rule=0, **kw):
    """A batch of tests/test_big_m.py's 2-row tableaus; their costs are explicit."""
    return spec(2, 2, B=B, rule=rule, construct=construct, cost="explicit", art_first=LITERAL[construct][3],
                budgets=[100], **kw)


def ncols_of(s):
    return s["n"] + s["m"] + 1


def art_first_of(s):
    return s["art_first"] if s["art_first"] is not None else b2.art_first_of(s)


def build_tableaus(s):
    """(T[B, m+2, ncols], basis[B, m]) of the LPs before any pivot: row m (M part) zero, row m + 1 the objective."""
    m, B, nc = s["m"], s["B"], ncols_of(s)
    if s["construct"] in LITERAL:
        tabs, bases, _, _ = LITERAL[s["construct"]]
        T = np.array([tabs[b % len(tabs)] for b in range(B)])
        basis = np.array([bases[b % len(bases)] for b in range(B)], dtype=np.int64)
    else:
        T1, basis = b2.build_tableaus({**s, "only": None})
        T = np.zeros((B, m + 2, nc))
        T[:, :m] = T1[:, :m]
        T[:, m + 1] = T1[:, m]
    if s["only"] is not None:
        T, basis = T[s["only"]:s["only"] + 1], basis[s["only"]:s["only"] + 1]
    return T, basis


def costs_of(s):
    """None, or the [B, N + 3] cost array (7.0 at the artificial columns, 1e300 in the padding)."""
    if s["cost"] == "none":
        return None
    assert s["cost"] == "explicit"
    N, af = ncols_of(s) - 1, art_first_of(s)
    if s["construct"] in LITERAL:
        lit = LITERAL[s["construct"]][2]
        c = np.zeros((s["B"], N + 3))
        for b in range(s["B"]):
            c[b, :N] = lit[b % len(lit)]
        c[:, N:] = 1e300
        if s["only"] is not None:
            c = c[s["only"]:s["only"] + 1]
    else:
        c = b2.costs_of(s)
    c[:, af - 1:N] = 7.0
    return c


def run_batch(s):
    """The case on the device; also returns info.tier / chunk / nobj."""
    import linearprogramming_amd as lpg
    B = 1 if s["only"] is not None else s["B"]
    e = lpg.BatchEngine(B, s["m"], ncols_of(s), big_m=True)
    try:
        if s["construct"] == "gen" and s["only"] is None:
            af = e.generate_artificial(s["n"], s["seed"])
            assert af == art_first_of(s)
        else:
            e.load(*build_tableaus(s))
        cost = costs_of(s)
        return bc.solve_and_read_back(e, s["budgets"], lambda budget: e.solve_big_m(art_first_of(s), cost, budget, s["rule"]),
                                      info_keys=("tier", "chunk", "nobj"))
    finally:
        e.close()


def run_oracle(s, cost=None):
    """Every LP of the case through Oracle(nobj=2).solve_big_m, one at a time (cost: instead of costs_of(s))."""
    nc = ncols_of(s)
    T, basis = build_tableaus(s)
    cost = costs_of(s) if cost is None else cost
    return bc.oracle_loop(T, basis, s["budgets"], lambda o, b, budget: o.solve_big_m(
        art_first_of(s), None if cost is None else cost[b, :nc - 1].copy(), budget, s["rule"]), 2 * (s["m"] + nc), nobj=2)


# the golden models whose rows lack a basic column, and how Big-M ends on them under both rules
LACKING_MODELS = {"a3_min_eq_neg.txt": OPTIMAL, "a5_lack_row.txt": OPTIMAL, "a7_identity_quirk.txt": OPTIMAL,
                  "m_ray_infeasible.txt": INFEASIBLE}


def oracle_model_big_m(sm, rule=0):
    """frontend.engine_arrays(sm) loaded into an nobj = 2 oracle (both objective rows zero) and solved by Big-M."""
    from linearprogramming_amd import frontend as F
    from oracle.lpo import Oracle
    rows, basis, cost, nc0, nlack = F.engine_arrays(sm)
    m, nc = rows.shape
    assert nlack > 0
    o = Oracle(m, nc, nobj=2)
    T = np.zeros((m + 2, nc))
    T[:m] = rows
    o.load_tableau(T, basis)
    r = o.solve_big_m(nc0, cost[:nc - 1].copy(), 10_000, rule)
    o.close()
    return r
