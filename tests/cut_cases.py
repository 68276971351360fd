"""Cut test plumbing (tests/test_cut_cases.py, tests/test_gpu_batch_cut.py,
tests/batch_worker.py), in the style of tests/branch_cases.py.

The numpy statement of include/lpg.h's "cuts": select_rows (what
lpg_batch_cut_select lists), cut_rows_of (the Gomory mixed-integer cut rows),
cut_child_of (the tableau, basis and active columns lpg_batch_cut makes), and
reference_walk: frontend.solve_ilp's cut rounds and branch-and-bound restated
on the CPU, every LP solved by an oracle.lpo.Oracle of its own, in the same
order. Only floor, subtraction, one division per cut, multiplication, negation
and comparisons are used, each a single IEEE rounding in numpy as on the
device, so every comparison is bit for bit.

run_batch(spec) runs a case on the device and returns arrays (so that a run
under LPG_BATCH_TIER=global travels back from tests/batch_worker.py);
expected(spec, got) is the same dict from numpy and the oracle.

spec keys: kind, m, n, B, lps as tests/branch_cases.py's; k ("1": the most
fractional row; "2": the two most fractional, given in descending row order;
"all": every candidate; "uneven": 1 + c % 3 rows for child c, a ragged child);
pattern ("each": one child per LP; "repeat": src repeating and descending, the
children of one source with different row sets); mask ("shared": one mask with
holes; "per_lp": a different one per LP); pre ("branch": the parent batch is
first branched both ways and re-solved, and the cuts are made on those
children); levels (1 or 2: a second round of cuts on the OPTIMAL children).
"""
from __future__ import annotations

import os

import numpy as np

import batch_cases as bc
import branch_cases as br

OPTIMAL, INFEASIBLE = br.OPTIMAL, br.INFEASIBLE
BUDGET = br.BUDGET
MAX_CUTS = 1024                                            # LPG_BATCH_MAX_CUTS


# ---------------------------------------------------------------------------
# the numpy statement
# ---------------------------------------------------------------------------
def frac(x):
    """x - floor(x), and 0.0 where that difference rounds to 1.0 (a tiny negative x)."""
    f = x - np.floor(x)
    return np.where(f >= 1.0, 0.0, f)


def select_rows(T, basis, m, mask, int_tol, max_cuts):
    """The rows lpg_batch_cut_select lists for one LP: select_row's candidates, largest distance first, ties to
    the smallest column, at most max_cuts."""
    cand = []
    for i in range(m):
        bj = int(basis[i])
        if not (1 <= bj <= len(mask) and mask[bj - 1]):
            continue
        v = T[i, 0]
        f = v - np.floor(v)
        f1 = 1.0 - f
        dist = f if f < f1 else f1
        if dist > int_tol:
            cand.append((-dist, bj, i))
    return np.array([i for _, _, i in sorted(cand)[:max_cuts]], dtype=np.int64)


def cut_rows_of(T, basis, nact, mask, rows):
    """The GMI cut rows of one LP over the parent's columns, [len(rows), ncols]: -f0 in column 0, -g_j in column
    j. T [m+1, ncols], basis [m], active columns 1..nact, mask over columns 1..len(mask)."""
    nc = T.shape[1]
    basis = np.asarray(basis, dtype=np.int64)
    basic = np.zeros(nc, dtype=bool)
    basic[basis[(basis >= 0) & (basis < nc)]] = True
    integer = np.zeros(nc, dtype=bool)
    n = min(len(mask), nc - 1)
    integer[1:n + 1] = np.asarray(mask[:n]) != 0
    out = np.zeros((len(rows), nc))
    with np.errstate(all="ignore"):
        for t, r in enumerate(rows):
            a = T[r]
            f0 = np.float64(frac(a[0]))
            rho = f0 / (np.float64(1.0) - f0)
            f = frac(a)
            gi = np.where(f <= f0, f, rho * (1.0 - f))
            gc = np.where(a >= 0.0, a, rho * (-a))
            g = np.where(integer, gi, gc)
            g[basic] = 0.0
            g[nact + 1:] = 0.0
            out[t] = -g
            out[t, 0] = -f0
    return out


def cut_child_of(T, basis, nact, mask, rows):
    """(T', basis', nact') of the child of (T [m+1, ncols], basis [m], active columns 1..nact) with one cut per
    row of `rows`: columns 0..nact in place, the k slacks, what lay behind nact; rows m..m+k-1, the objective
    last."""
    m, nc, k = T.shape[0] - 1, T.shape[1], len(rows)
    G = cut_rows_of(T, basis, nact, mask, rows)
    C = np.zeros((m + k + 1, nc + k))
    src = np.vstack([T[:m], G, T[m:]])
    C[:, :nact + 1] = src[:, :nact + 1]
    C[:, nact + 1 + k:] = src[:, nact + 1:]
    C[m + np.arange(k), nact + 1 + np.arange(k)] = 1.0
    cb = np.zeros(m + k, dtype=np.int64)
    cb[:m] = np.where(basis > nact, basis + k, basis)
    cb[m:] = nact + 1 + np.arange(k)
    return C, cb, nact + k


# ---------------------------------------------------------------------------
# device cases
# ---------------------------------------------------------------------------
def spec(kind, m=None, n=None, B=4, lps=None, k="1", pattern="each", mask="shared", pre=None, levels=1):
    return {"kind": kind, "m": m, "n": n, "B": B, "lps": lps, "k": k, "pattern": pattern, "mask": mask, "pre": pre,
            "levels": levels}


def mask_of(s, count=None):
    """The case's mask over every structural and slack column of the widest LP, with holes: [nmask], or
    [count, nmask] with a different one per LP."""
    nmask = max(n + m for m, n in br.shapes_of(s))
    j = np.arange(nmask)
    if s["mask"] == "per_lp":
        return np.array([(j + q) % 3 != 2 for q in range(count)], dtype=np.uint8)
    return (j % 3 != 2).astype(np.uint8)


def _jobs(s, cand, status):
    """(src, rows per child) of the case over the LPs that are OPTIMAL and have a candidate row."""
    ok = [q for q in range(len(cand)) if len(cand[q]) and status[q] == OPTIMAL]
    if s["pattern"] == "repeat":
        src = [q for q in reversed(ok)] + ok[-1:] * 2 + ok[:1]
    else:
        src = list(ok)
    per = []
    for c, q in enumerate(src):
        cq = cand[q]
        if s["pattern"] == "repeat":                       # two rows from a window that moves with the child
            per.append(np.array([cq[(c + u) % len(cq)] for u in range(min(2, len(cq)))], dtype=np.int64))
        elif s["k"] == "1":
            per.append(cq[:1])
        elif s["k"] == "2":
            per.append(np.sort(cq[:2])[::-1].copy())       # given in descending row order
        elif s["k"] == "uneven":
            per.append(cq[:1 + c % 3])
        else:
            per.append(cq)
    return np.array(src, dtype=np.int64), per


def _store_jobs(out, tag, src, per, cand):
    out[f"{tag}/first"] = np.concatenate([[0], np.cumsum([len(r) for r in per])]).astype(np.int64)
    out[f"{tag}/cutrows"] = np.concatenate(per + [np.zeros(0, dtype=np.int64)])
    out[f"{tag}/ncand"] = np.array([len(x) for x in cand], dtype=np.int64)
    out[f"{tag}/cand"] = np.concatenate(list(cand) + [np.zeros(0, dtype=np.int64)])


def run_batch(s):
    """The case on the device. Keys: parent/* (the solved batch the cuts start from), and per level L: L/built/*
    (the children as lpg_batch_cut made them, with src, first, cutrows: the jobs, and ncand, cand: what
    lpg_batch_cut_select listed for every LP of the level's parent) and L/solved/* (after solve_dual)."""
    e, res = br._parent_engine(s)
    engines = [e]
    out = {}
    none = np.zeros(0, dtype=np.int64)
    try:
        if s["pre"] == "branch":
            pick, _, _ = e.branch_select(np.ones(max(n + m for m, n in br.shapes_of(s)), dtype=np.uint8))
            ok = np.array([q for q in range(e.count) if pick[q] >= 0 and res[q].status == OPTIMAL], dtype=np.int64)
            src = np.repeat(ok, 2)
            e = e.branch(src, pick[src], np.tile(np.array([-1, 1], dtype=np.int8), len(ok)))
            engines.append(e)
            res = e.solve_dual(BUDGET)
        br._level_arrays(out, "parent", e, none, none, none.astype(np.int8), res)
        status = out["parent/status"]
        mask = mask_of(s, e.count)
        out["mask"] = mask
        for level in range(1, s["levels"] + 1):
            cand = e.cut_select(mask, 1e-6, MAX_CUTS)
            src, per = _jobs(s, cand, status)
            ch = e.cut(src, per, mask)
            engines.append(ch)
            out[f"{level}/ragged"] = np.array(int(ch.info.pad), dtype=np.int64)
            for stage, r in (("built", None), ("solved", ch.solve_dual)):
                r = r(BUDGET) if r else None
                br._level_arrays(out, f"{level}/{stage}", ch, src, none, none.astype(np.int8), r)
                _store_jobs(out, f"{level}/{stage}", src, per, cand)
            e, status = ch, out[f"{level}/solved/status"]
        return out
    finally:
        for x in engines:
            x.close()


def expected(s, got):
    """The same arrays as run_batch's levels from numpy and the oracle, starting from the tableaus the device run
    read back under parent/* and following the device's jobs (check_selection holds them against select_rows)."""
    T, basis, nact = br._split(got, "parent")
    mask = got["mask"]
    out = {}
    for level in range(1, s["levels"] + 1):
        src, first, rows = (got[f"{level}/built/{key}"] for key in ("src", "first", "cutrows"))
        built = [cut_child_of(T[q], basis[q], nact[q], mask if mask.ndim == 1 else mask[q], rows[first[c]:first[c + 1]])
                 for c, q in enumerate(src)]
        solved = [br.oracle_dual(C, cb, na) for C, cb, na in built]
        out[f"{level}/built/rows"] = np.concatenate([C.ravel() for C, _, _ in built])
        out[f"{level}/built/basis"] = np.concatenate([cb for _, cb, _ in built])
        out[f"{level}/built/nact"] = np.array([na for _, _, na in built], dtype=np.int64)
        out[f"{level}/built/m"] = np.array([C.shape[0] - 1 for C, _, _ in built], dtype=np.int64)
        out[f"{level}/built/ncols"] = np.array([C.shape[1] for C, _, _ in built], dtype=np.int64)
        out[f"{level}/solved/rows"] = np.concatenate([x["rows"].ravel() for x in solved])
        out[f"{level}/solved/basis"] = np.concatenate([x["basis"].ravel() for x in solved])
        for key in ("status", "pivots", "objective", "loglen"):
            out[f"{level}/solved/{key}"] = np.concatenate([x[key] for x in solved])
        T = [x["rows"][0] for x in solved]
        basis = [x["basis"][0] for x in solved]
        nact = [na for _, _, na in built]
    return out


def check_selection(s, got, int_tol=1e-6):
    """What lpg_batch_cut_select listed for every LP of every level's parent is select_rows' list."""
    T, basis, _ = br._split(got, "parent")
    mask = got["mask"]
    for level in range(1, s["levels"] + 1):
        ncand, cand = got[f"{level}/built/ncand"], got[f"{level}/built/cand"]
        at = np.concatenate([[0], np.cumsum(ncand)])
        assert len(ncand) == len(T)
        for q in range(len(T)):
            want = select_rows(T[q], basis[q], T[q].shape[0] - 1, mask if mask.ndim == 1 else mask[q], int_tol, MAX_CUTS)
            assert np.array_equal(cand[at[q]:at[q + 1]], want), (level, q, cand[at[q]:at[q + 1]], want)
        T, basis, _ = br._split(got, f"{level}/solved")


def in_subprocess(specs, env, tmp_path):
    return bc.in_subprocess("cut_cases", specs, env, tmp_path)


# ---------------------------------------------------------------------------
# the models of the validity and driver tests
# ---------------------------------------------------------------------------
_HERE = os.path.dirname(os.path.abspath(__file__))


def _text(of, st):
    return "OF {\n\t%s\n}\nST {\n\t%s\n}\n" % (of, ";\n\t".join(st))


def _nonneg(n):
    return [f"x{i}>=0" for i in range(1, n + 1)]


def _golden(name):
    with open(os.path.join(_HERE, "golden", "lp", name + ".txt"), encoding="utf-8") as f:
        return f.read()


# model -> (text, the integer box of the user's variables: it holds every feasible point, or for the unbounded
# polyhedron of a3_min_eq_neg a part around the optimum, sense, the optimum over the box by enumeration)
MODELS = {
    "a3_min_eq_neg": (_golden("a3_min_eq_neg"), {"x1": (0, 9), "x2": (0, 12), "x3": (-12, 0)}, "min", 13),
    "two_var": (_text("max:z=5x1+8x2", ["x1+x2<=6", "5x1+9x2<=45"] + _nonneg(2)), {"x1": (0, 6), "x2": (0, 6)}, "max", 40),
    "three_var": (_text("max:z=7x1+3x2+5x3", ["6x1+4x2+5x3<=23", "3x1+7x2+2x3<=19", "4x1+x2+6x3<=17"] + _nonneg(3)),
                  {"x1": (0, 4), "x2": (0, 3), "x3": (0, 3)}, "max", 24),
    "two_phase": (_text("min:z=3x1+2x2+4x3", ["2x1+2x2+2x3>=7", "3x1-x2+x3=2", "x1+3x3<=9"] + _nonneg(3)),
                  {"x1": (0, 9), "x2": (0, 28), "x3": (0, 3)}, "min", 11),
}


def same_as_walk(sol, ref):
    """An ILPSolution of frontend.solve_ilp_text equals a reference walk's dict, floats bit for bit."""
    assert (sol.status, sol.nodes, sol.depth, sol.pivots) == (ref["status"], ref["nodes"], ref["depth"], ref["pivots"])
    if ref["z"] is None:
        assert np.isnan(sol.z) and not sol.variables
    else:
        assert bc.bits(sol.z) == bc.bits(ref["z"])
        assert sol.variables.keys() == ref["variables"].keys()
        for k, v in ref["variables"].items():
            assert bc.bits(sol.variables[k]) == bc.bits(v), k


# ---------------------------------------------------------------------------
# the driver's walk on the CPU
# ---------------------------------------------------------------------------
def root_of(text, integer=None):
    """The root relaxation of frontend.solve_ilp_text's model on an Oracle: (sm, mask, (T, basis, nact,
    objective), result)."""
    from linearprogramming_amd import frontend as F
    from oracle.lpo import Oracle
    if integer is None:
        integer = F.text_variables(text)
    sm = F.build_smatrix(text)
    mask = br.integer_columns(sm, integer)
    rows, basis, cost, nc0, nlack = F.engine_arrays(sm)
    m, nc = rows.shape
    o = Oracle(m, nc)
    T = np.zeros((m + 1, nc))
    T[:m] = rows
    o.load_tableau(T, basis)
    if nlack:
        r = o.solve_two_phase(nc0, cost[:nc - 1].copy())
        nact = nc0 - 1
    else:
        o.set_objective(cost[:nc - 1].copy())
        r = o.solve()
        nact = nc - 1
    root = (o.get_rows(), o.get_basis(), nact, r.objective)
    o.close()
    return sm, mask, root, r


def reference_walk(text, integer=None, int_tol=1e-6, node_limit=100000, rule=br.MOST_FRACTIONAL, cut_rounds=0, max_cuts=8):
    """frontend.solve_ilp_text's walk, one Oracle per LP: a dict of status, pivots, nodes, depth, objective (the
    incumbent's max-form objective), z and variables. After an OPTIMAL root up to cut_rounds rounds: the
    max_cuts most fractional rows (none: the rounds end), their cuts, solve_dual, one more node; INFEASIBLE
    or any other non-OPTIMAL status ends the walk with it. Then tests/branch_cases.py reference_walk's tree
    from that LP."""
    from linearprogramming_amd import frontend as F
    sm, mask, root, r = root_of(text, integer)
    out = {"status": br.bc_status(r.status), "pivots": int(r.pivots), "nodes": 1, "depth": 1, "objective": None, "z": None,
           "variables": {}}
    if r.status != OPTIMAL:
        return out
    for _ in range(cut_rounds):
        Tq, bq, na, _ = root
        rows = select_rows(Tq, bq, Tq.shape[0] - 1, mask, int_tol, max_cuts)
        if not len(rows):
            break
        C, cb, cna = cut_child_of(Tq, bq, na, mask, rows)
        res = br.oracle_dual(C, cb, cna, 1 << 40)
        out["nodes"] += 1
        out["pivots"] += int(res["pivots"][0])
        if int(res["status"][0]) != OPTIMAL:
            out["status"] = br.bc_status(res["status"][0])
            return out
        root = (res["rows"][0], res["basis"][0], cna, float(res["objective"][0]))
    level, best = [root], None
    while level:
        if out["nodes"] > node_limit:
            out["status"] = "NODE_LIMIT"
            break
        picks = [br.select_row(Tq, bq, Tq.shape[0] - 1, mask, int_tol, rule) for Tq, bq, _, _ in level]
        cand = None
        for q, p in enumerate(picks):
            if p[0] < 0 and (cand is None or level[q][3] > level[cand][3]):
                cand = q
        if cand is not None and (best is None or level[cand][3] > best[3]):
            best = level[cand]
        kids = []
        for q, p in enumerate(picks):
            if p[0] < 0 or (best is not None and level[q][3] <= best[3]):
                continue
            Tq, bq, na, _ = level[q]
            for d in (-1, 1):
                C, cb, cna = br.child_of(Tq, bq, na, p[0], d)
                kids.append((br.oracle_dual(C, cb, cna, 1 << 40), cna))
        out["nodes"] += len(kids)
        out["pivots"] += sum(int(res["pivots"][0]) for res, _ in kids)
        other = [int(res["status"][0]) for res, _ in kids if int(res["status"][0]) not in (OPTIMAL, INFEASIBLE)]
        if other:
            out["status"] = br.bc_status(other[0])
            return out
        nxt = [(res["rows"][0], res["basis"][0], cna, float(res["objective"][0])) for res, cna in kids
               if int(res["status"][0]) == OPTIMAL]
        if nxt:
            out["depth"] += 1
        level = nxt
    if out["status"] == "OPTIMAL" and best is None:
        out["status"] = "INFEASIBLE"
    if best is not None:
        Tq, bq, _, obj = best
        sol = F._readout(sm, F.LPSolution("OPTIMAL", 0), obj, Tq[:Tq.shape[0] - 1, 0], bq, Tq.shape[1])
        out["objective"], out["z"], out["variables"] = obj, sol.z, sol.variables
    return out


# ---------------------------------------------------------------------------
# integer points of a small model, for the validity of the cuts
# ---------------------------------------------------------------------------
def integer_points(text, box):
    """Every point of the user's integer box (a dict name -> (lo, hi)) that the model's standard form admits, as
    full column vectors x [points, N] over columns 1..N (structural columns and slacks), with the user's
    values [points, variables] and the max-form objective of each."""
    import itertools
    from linearprogramming_amd import frontend as F
    sm = F.build_smatrix(text)
    rows, _, cost, nc0, _ = F.engine_arrays(sm)
    A, b = rows[:, 1:nc0], rows[:, 0]
    N = nc0 - 1
    names = list(box)
    structural = np.zeros(N, dtype=bool)
    pts, users = [], []
    for vals in itertools.product(*[range(lo, hi + 1) for lo, hi in (box[v] for v in names)]):
        x = np.zeros(N)
        good = True
        for name, val in zip(names, vals):
            it = sm.vars.get(name)
            if it.relation == 0 and it.former:
                x[sm.names.index(it.former)], x[sm.names.index(it.latter)] = max(val, 0), max(-val, 0)
                structural[[sm.names.index(it.former), sm.names.index(it.latter)]] = True
            else:
                j = sm.names.index(name)
                x[j] = -val if sm.inverted[j] else val
                structural[j] = True
                good &= x[j] >= 0
        if good:
            pts.append(x)
            users.append(vals)
    X = np.array(pts)
    # the slacks: every non-structural column is a unit column of one row, with coefficient +1 or -1
    S = A[:, ~structural]
    assert all(np.count_nonzero(S[:, j]) == 1 and abs(S[:, j]).sum() == 1.0 for j in range(S.shape[1]))
    resid = b[None, :] - X[:, structural] @ A[:, structural].T               # [points, m]
    slack = resid @ S                                                          # s_j = +-(b_i - a_i . x)
    X[:, ~structural] = slack
    feasible = (slack >= 0).all(axis=1) & (np.abs(X @ A.T - b[None, :]) < 1e-9).all(axis=1)
    X = X[feasible]
    return X, np.array(users)[feasible], X @ cost[:N], names
