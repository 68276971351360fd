"""Scenario test plumbing (tests/test_scenario_cases.py,
tests/test_gpu_batch_scenario.py, tests/batch_worker.py), in the style of
tests/branch_cases.py.

The numpy statement of include/lpg.h's "scenarios": rhs_column (column 0 of a
tableau restated for another right-hand side), child_of (the tableau, basis
and active columns lpg_batch_scenario makes). Only products and sums of two
doubles are used, in the order of the device, each a single IEEE rounding in
numpy as there, so every comparison is bit for bit.

run_batch(spec) runs a case on the device and returns arrays (so that a run
under LPG_BATCH_TIER=global travels back from tests/batch_worker.py);
expected(spec, got) is the same dict from numpy and the oracle.

The scenarios of an LP with right-hand side b (m entries), fixed so that the
cases are the ones the counts in tests/test_scenario_cases.py were taken on:
rng = numpy.random.default_rng(11) once per LP; scenario 0 is b itself,
scenario c = 1..7 is b * (0.2 + 2.5 * rng.random(m)), drawn in that order; for
the dense kind the last scenario also has rhs[m // 2] = -1.0 (that row has
non-negative coefficients and a slack: infeasible by construction). A second
draw (set_rhs) goes on with the same generator.

spec keys: kind, m, n, B, lps as tests/branch_cases.py's; pattern ("both":
every LP under every scenario; "repeat": n != count, src descending and
repeating); nscen (scenarios per LP); second (True: set_rhs on the solved
children with the second draw, and solve_dual again).
"""
from __future__ import annotations

import numpy as np

import batch_cases as bc
import branch_cases as br

SEED = bc.SEED
OPTIMAL, INFEASIBLE = br.OPTIMAL, br.INFEASIBLE
BUDGET = br.BUDGET
NSCEN = 8


# ---------------------------------------------------------------------------
# the numpy statement
# ---------------------------------------------------------------------------
def rhs_column(T, ident, rhs):
    """Column 0 of every row of T [m+1, ncols] for the right-hand side rhs [m], stated in the frame in which
    column ident[i] was e_i: acc = 0.0; for i = 0..m-1: acc = acc + T[:, ident[i]] * rhs[i]."""
    acc = np.zeros(T.shape[0])
    with np.errstate(all="ignore"):
        for i in range(len(rhs)):
            acc = acc + T[:, int(ident[i])] * np.float64(rhs[i])
    return acc


def child_of(T, basis, nact, ident, rhs):
    """(T', basis', nact') of the scenario child of (T [m+1, ncols], basis [m], active columns 1..nact): the
    same LP, column 0 restated."""
    C = T.copy()
    C[:, 0] = rhs_column(T, ident, rhs)
    return C, np.array(basis, dtype=np.int64), nact


def scenarios(b, dense, nscen=NSCEN, draw=0):
    """The first nscen of the recipe's NSCEN scenarios: [nscen, m]; draw = 1: the second draw of the same generator."""
    rng = np.random.default_rng(11)
    m = len(b)
    out = []
    for d in range(draw + 1):
        out = [np.array(b, dtype=np.float64)] + [b * (0.2 + 2.5 * rng.random(m)) for _ in range(NSCEN - 1)]
    if dense:
        out[-1][m // 2] = -1.0
    return np.array(out[:nscen])


def generated(m, n, seed, kind):
    """(T [m+1, ncols], basis [m]) of the oracle's generator, before any pivot."""
    from oracle.lpo import Oracle
    o = Oracle(m, n + m + 1)
    o.generate(n, seed, kind)
    T, basis = o.get_rows(), o.get_basis()
    o.close()
    return T, basis


def solved_parent(m, n, seed, kind):
    """The LP of the generator solved on the oracle as the device cases solve their parents: (T0, ident, T,
    basis, nact, result), T0 the tableau before any pivot and ident its basis."""
    from oracle.lpo import Oracle
    T0, ident = generated(m, n, seed, kind)
    o = Oracle(m, n + m + 1)
    o.load_tableau(T0, ident)
    if kind == 2:
        r = o.solve_two_phase(br.art_first_of(m, n), None, BUDGET)
        nact = br.art_first_of(m, n) - 1
    else:
        r = o.solve(BUDGET)
        nact = n + m
    T, basis = o.get_rows(), o.get_basis()
    o.close()
    return T0, ident, T, basis, nact, r


# ---------------------------------------------------------------------------
# device cases
# ---------------------------------------------------------------------------
def spec(kind, m=None, n=None, B=2, lps=None, pattern="both", nscen=NSCEN, second=False):
    return {"kind": kind, "m": m, "n": n, "B": B, "lps": lps, "pattern": pattern, "levels": 1, "nscen": nscen,
            "second": second}


def _jobs(s, count):
    """(src, scenario index) per child."""
    k = s["nscen"]
    if s["pattern"] == "repeat":
        src = list(range(count - 1, -1, -1)) + [count - 1] * 2 + [0]
        return np.array(src, dtype=np.int64), [(c + 1) % k for c in range(len(src))]
    return np.repeat(np.arange(count, dtype=np.int64), k), list(range(k)) * count


def _per_lp(e, arrays):
    """One array per LP for a ragged engine, one 2-D array for an engine of one shape."""
    return list(arrays) if e.info.pad else np.array(arrays)


def run_batch(s):
    """The case on the device. Keys: parent/* (the solved parent), ident, src, 1/rhs (packed), 1/built/* (the
    children as lpg_batch_scenario made them), 1/solved/* (after solve_dual), after/rows (the parent read back
    after scenario()); with `second`: 2/rhs, 2/built/* (the same engine after set_rhs), 2/solved/*."""
    e, res = br._parent_engine(s)
    engines = [e]
    out = {}
    none = np.zeros(0, dtype=np.int64)
    try:
        shapes = br.shapes_of(s)
        dense = s["kind"] in ("dense", "ragged")
        start = [generated(m, n, SEED + q, 0 if dense else 2) for q, (m, n) in enumerate(shapes)]
        ident = [b for _, b in start]
        sets = [[scenarios(T[:-1, 0], dense, s["nscen"], d) for T, _ in start] for d in (0, 1)]
        br._level_arrays(out, "parent", e, none, none, none.astype(np.int8), res)
        src, idx = _jobs(s, e.count)
        out["ident"] = np.concatenate(ident)
        rhs = [sets[0][q][k] for q, k in zip(src, idx)]
        out["1/rhs"] = np.concatenate(rhs)
        ch = e.scenario(src, _per_lp(e, rhs), _per_lp(e, ident))
        engines.append(ch)
        out["after/rows"] = np.concatenate([np.array(r).ravel() for r in e.get_rows()])
        br._level_arrays(out, "1/built", ch, src, none, none.astype(np.int8), None)
        br._level_arrays(out, "1/solved", ch, src, none, none.astype(np.int8), ch.solve_dual(BUDGET))
        if s["second"]:
            rhs = [sets[1][q][k] for q, k in zip(src, idx)]
            out["2/rhs"] = np.concatenate(rhs)
            ch.set_rhs(_per_lp(ch, rhs), _per_lp(ch, [ident[q] for q in src]))
            br._level_arrays(out, "2/built", ch, src, none, none.astype(np.int8), None)
            br._level_arrays(out, "2/solved", ch, src, none, none.astype(np.int8), ch.solve_dual(BUDGET))
        return out
    finally:
        for x in engines:
            x.close()


def expected(s, got):
    """The same arrays as run_batch's stages from numpy and the oracle, starting from the parent tableaus the
    device run read back (got["parent/*"]; the parent solve itself is tests/test_gpu_batch*.py's subject). Stage
    2 continues from stage 1's solved tableaus, each LP its own source."""
    T, basis, nact = br._split(got, "parent")
    src = got["1/built/src"]
    ms = [t.shape[0] - 1 for t in T]
    at = np.concatenate([[0], np.cumsum(ms)])
    ident = [got["ident"][at[q]:at[q + 1]] for q in range(len(T))]
    out = {}
    for level in (1, 2) if s["second"] else (1,):
        rhs, r0 = got[f"{level}/rhs"], 0
        built = []
        for c, q in enumerate(src):
            p = q if level == 1 else c                     # the tableau restated: the parent's LP q, or child c itself
            built.append(child_of(T[p], basis[p], nact[p], ident[q], rhs[r0:r0 + ms[q]]))
            r0 += ms[q]
        solved = [br.oracle_dual(C, cb, na) for C, cb, na in built]
        out[f"{level}/built/rows"] = np.concatenate([C.ravel() for C, _, _ in built])
        out[f"{level}/built/basis"] = np.concatenate([cb for _, cb, _ in built])
        out[f"{level}/built/nact"] = np.array([na for _, _, na in built], dtype=np.int64)
        out[f"{level}/built/m"] = np.array([C.shape[0] - 1 for C, _, _ in built], dtype=np.int64)
        out[f"{level}/built/ncols"] = np.array([C.shape[1] for C, _, _ in built], dtype=np.int64)
        out[f"{level}/built/art_first"] = got["parent/art_first"][src]
        out[f"{level}/solved/rows"] = np.concatenate([x["rows"].ravel() for x in solved])
        out[f"{level}/solved/basis"] = np.concatenate([x["basis"].ravel() for x in solved])
        for key in ("status", "pivots", "objective", "loglen"):
            out[f"{level}/solved/{key}"] = np.concatenate([x[key] for x in solved])
        T = [x["rows"][0] for x in solved]
        basis = [x["basis"][0] for x in solved]
        nact = [na for _, _, na in built]
    return out


def assert_stage(got, want, level):
    """br.assert_level, and the child's art_first."""
    br.assert_level(got, want, level)
    assert np.array_equal(got[f"{level}/built/art_first"], want[f"{level}/built/art_first"])


def in_subprocess(specs, env, tmp_path):
    return bc.in_subprocess("scenario_cases", specs, env, tmp_path)
