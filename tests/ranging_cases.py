"""Ranging test plumbing (tests/test_ranging_cases.py,
tests/test_gpu_batch_ranging.py), in the style of tests/scenario_cases.py.

The numpy statement of include/lpg.h's "ranging": ranging_of (the nine output
arrays of one LP). It follows the header operation for operation: one negation
and one IEEE division per candidate, strict comparisons against eps_piv, NaN
ratios out, the largest (lower bound) or smallest (upper bound) ratio, equal
ratios to the smallest index. Every comparison with the device is bit for bit
(bits()).

The kernel's partition, as constants, so that the census of
tests/test_ranging_cases.py counts against what k_batch_ranging does:
cost phase: one wave of LANES lanes per basic row, lane (k - 1) % LANES takes
column k, so two candidates of a bound meet inside a lane's stride when their
lanes are equal (they then sit in different LANES-column groups) and in the
wave's butterfly when they differ; WAVES waves take the rows r % WAVES, which
never brings two candidates of one bound together. Right-hand-side phase: one
lane per frame row walks the rows r = 0..m-1 serially (RHS_SERIAL), so every
pair of candidates of a bound meets inside that one walk, whatever their
distance; frame rows BLOCK apart share a lane.

A device case is a list of LPs, lp(kind, m, n, seed): "dense" and
"artificial" are the oracle's generator (kinds 0 and 2), "primal" and
"interval_art" tests/tie_cases.py's exact interval LPs in those two forms. A
uniform case has one shape and kind; a ragged one mixes them: every LP of it is
solved two-phase with its own art_first, and an LP without artificial columns
gets one empty column behind its last (art_first = N), never basic.
"""
from __future__ import annotations

import numpy as np

import batch_cases as bc
import tie_cases as tc

SEED = bc.SEED
OPTIMAL, INFEASIBLE = 1, 3
BUDGET = 20000
LANES, WAVES, BLOCK = 64, 4, 256
COST_LANE_STRIDES = "columns"      # the index a lane strides in the cost phase
RHS_SERIAL = True                  # a lane walks all rows of its frame row's column
FIELDS = ("dual", "cost_lo", "cost_hi", "cost_lo_at", "cost_hi_at", "rhs_lo", "rhs_hi", "rhs_lo_at", "rhs_hi_at")
GROUPS = {"dual": ("dual",), "cost": FIELDS[1:5], "rhs": FIELDS[5:]}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


# ---------------------------------------------------------------------------
# the numpy statement
# ---------------------------------------------------------------------------
def candidates(x, a, eps, upper):
    """(q, is a candidate) of the entries (x, a): q = (-x) / a; lower: a > eps, upper: a < -eps; NaN q: none."""
    with np.errstate(all="ignore"):
        q = (-x) / a
    return q, ((a < -eps) if upper else (a > eps)) & ~np.isnan(q)


def bound(x, a, idx, eps, upper, none):
    """One bound over the candidates (x[t], a[t], idx[t]), idx ascending: (the winner's q, its index), or
    (-inf / +inf, none)."""
    q, c = candidates(x, a, eps, upper)
    if not c.any():
        return (np.inf if upper else -np.inf), none
    best = q[c].min() if upper else q[c].max()
    t = np.flatnonzero(c & (q == best))[0]            # equal ratios (-0 == +0): the smallest index
    return q[t], int(idx[t])


def tied(x, a, idx, eps, upper):
    """The indices of the candidates that compare equal to the winner of the bound (one entry: no tie)."""
    q, c = candidates(x, a, eps, upper)
    if not c.any():
        return np.zeros(0, dtype=np.int64)
    best = q[c].min() if upper else q[c].max()
    return np.asarray(idx)[c & (q == best)]


def ranging_of(T, basis, nact, ident, eps, status):
    """The nine arrays of include/lpg.h's "ranging" for one LP: T [m+1, ncols] as get_rows returns it, basis [m],
    active columns 1..nact, ident [m], eps = eps_piv, status the LP's."""
    m, N = T.shape[0] - 1, T.shape[1] - 1
    out = {"dual": np.full(m, np.nan), "cost_lo": np.full(N, np.nan), "cost_hi": np.full(N, np.nan),
           "cost_lo_at": np.zeros(N, dtype=np.int64), "cost_hi_at": np.zeros(N, dtype=np.int64),
           "rhs_lo": np.full(m, np.nan), "rhs_hi": np.full(m, np.nan),
           "rhs_lo_at": np.full(m, -1, dtype=np.int64), "rhs_hi_at": np.full(m, -1, dtype=np.int64)}
    if status != OPTIMAL:
        return out
    ident = np.asarray(ident, dtype=np.int64)
    obj = T[m]
    out["dual"] = obj[ident].copy()
    # costs
    row_of = np.full(N + 1, -1, dtype=np.int64)
    row_of[np.asarray(basis, dtype=np.int64)] = np.arange(m)
    ks = np.array([k for k in range(1, nact + 1) if row_of[k] < 0], dtype=np.int64)
    for j in range(1, N + 1):
        if j > nact:
            lo, lo_at, hi, hi_at = -np.inf, 0, np.inf, 0
        elif row_of[j] < 0:
            lo, lo_at, hi, hi_at = -np.inf, 0, obj[j], j
        else:
            r = row_of[j]
            lo, lo_at = bound(obj[ks], T[r, ks], ks, eps, False, 0)
            hi, hi_at = bound(obj[ks], T[r, ks], ks, eps, True, 0)
        out["cost_lo"][j - 1], out["cost_lo_at"][j - 1], out["cost_hi"][j - 1], out["cost_hi_at"][j - 1] = lo, lo_at, hi, hi_at
    # right-hand sides
    rs = np.arange(m)
    for i in range(m):
        h = ident[i]
        out["rhs_lo"][i], out["rhs_lo_at"][i] = bound(T[:m, 0], T[:m, h], rs, eps, False, -1)
        out["rhs_hi"][i], out["rhs_hi_at"][i] = bound(T[:m, 0], T[:m, h], rs, eps, True, -1)
    return out


def ties_of(T, basis, nact, ident, eps):
    """The census of one OPTIMAL LP against the kernel's partition: counts of bounds by where their equal best
    candidates sit, and of the other classes the device cases must hold."""
    m, N = T.shape[0] - 1, T.shape[1] - 1
    st = dict.fromkeys(("cost_ties", "cost_ties_xlane", "cost_ties_inlane", "cost_ties_xgroup", "rhs_ties",
                        "rhs_ties_xgroup", "rhs_ties_xlane_row", "no_candidate", "degenerate_rows"), 0)
    row_of = np.full(N + 1, -1, dtype=np.int64)
    row_of[np.asarray(basis, dtype=np.int64)] = np.arange(m)
    ks = np.array([k for k in range(1, nact + 1) if row_of[k] < 0], dtype=np.int64)
    for j in range(1, nact + 1):
        if row_of[j] < 0:
            continue
        sides = [tied(T[m, ks], T[row_of[j], ks], ks, eps, up) for up in (False, True)]
        st["no_candidate"] += all(len(w) == 0 for w in sides)
        for w in sides:
            if len(w) < 2:
                continue
            lane, group = (w - 1) % LANES, (w - 1) // LANES
            st["cost_ties"] += 1
            st["cost_ties_xlane"] += len(set(lane)) > 1
            st["cost_ties_inlane"] += len(set(lane)) < len(lane)
            st["cost_ties_xgroup"] += len(set(group)) > 1
    rs = np.arange(m)
    for i in range(m):
        sides = [tied(T[:m, 0], T[:m, int(ident[i])], rs, eps, up) for up in (False, True)]
        st["no_candidate"] += all(len(w) == 0 for w in sides)
        for w in sides:
            if len(w) < 2:
                continue
            st["rhs_ties"] += 1
            st["rhs_ties_xgroup"] += len(set(w // LANES)) > 1
    st["rhs_ties_xlane_row"] = int(m > BLOCK)              # frame rows BLOCK apart share a lane
    st["degenerate_rows"] = int((T[:m, 0] == 0).sum())
    return st


# ---------------------------------------------------------------------------
# the LPs
# ---------------------------------------------------------------------------
def lp(kind, m, n, seed=None):
    return {"kind": kind, "m": m, "n": n, "seed": seed}


def uniform(kind, m, n, B=4, seed=None):
    """B LPs of one kind and shape; seeds seed, seed + 1, ..."""
    s0 = (SEED if kind in ("dense", "artificial") else 1) if seed is None else seed
    return [lp(kind, m, n, s0 + q) for q in range(B)]


def build_lp(c):
    """(T [m+1, n+m+1], basis [m], art_first or None) of the LP before any pivot."""
    m, n = c["m"], c["n"]
    if c["kind"] in ("dense", "artificial"):
        from oracle.lpo import Oracle
        o = Oracle(m, n + m + 1)
        o.generate(n, c["seed"], 2 if c["kind"] == "artificial" else 0)
        T, basis = o.get_rows(), o.get_basis()
        o.close()
    else:
        T, basis = tc.interval_lp(m, n, c["seed"], "artificial" if c["kind"] == "interval_art" else "primal")
    return T, basis, tc.art_first_of(m, n) if c["kind"] in ("artificial", "interval_art") else None


def solve_oracle(c):
    """The LP solved on the oracle as the device cases solve it: (T, basis, nact, ident, status)."""
    from oracle.lpo import Oracle
    T0, ident, af = build_lp(c)
    o = Oracle(T0.shape[0] - 1, T0.shape[1])
    o.load_tableau(T0, ident)
    r = o.solve_two_phase(af, None, BUDGET) if af else o.solve(BUDGET)
    T, basis = o.get_rows(), o.get_basis()
    o.close()
    return T, basis, (af - 1 if af else T0.shape[1] - 1), ident, r.status


def solved_engine(cases, ragged=False):
    """(engine, results, ident per LP) of the cases loaded and solved on the device."""
    import linearprogramming_amd as lpg
    built = [build_lp(c) for c in cases]
    if ragged:
        tabs, afs = [], []
        for T, _, af in built:
            if af is None:                                  # one empty column behind the last: art_first = N
                T = np.hstack([T, np.zeros((T.shape[0], 1))])
                af = T.shape[1] - 1
            tabs.append(T)
            afs.append(af)
        e = lpg.BatchEngine.ragged([(T.shape[0] - 1, T.shape[1]) for T in tabs])
        e.load(tabs, [b for _, b, _ in built])
        res = e.solve_two_phase(afs, None, BUDGET)
    else:
        T0, _, af = built[0]
        e = lpg.BatchEngine(len(built), T0.shape[0] - 1, T0.shape[1])
        e.load(np.array([T for T, _, _ in built]), np.array([b for _, b, _ in built]))
        res = e.solve_two_phase(af, None, BUDGET) if af else e.solve(BUDGET)
    return e, res, [b for _, b, _ in built]


def state_of(e, res):
    """What ranging_of needs of every LP, read back from the batch: rows, basis (one array per LP), nact, status."""
    rows, bas = e.get_rows(), e.get_basis()
    return {"rows": [np.array(r) for r in rows], "basis": [np.array(b) for b in bas],
            "nact": [e.active_columns(q)[0] for q in range(e.count)], "status": [r.status for r in res]}


def device_ranging(e, ident, **groups):
    """e.ranging as {field: one flat array over the LPs}, whatever the engine's class."""
    per_lp = isinstance(ident, list) and e.info.pad
    r = e.ranging(ident if per_lp else np.array(ident), **groups)
    return {f: np.concatenate([np.ravel(x) for x in getattr(r, f)]) for f in FIELDS if getattr(r, f) is not None}


def expected(state, ident, eps=1e-9):
    """ranging_of every LP of state_of's dict, as device_ranging lays it out."""
    per = [ranging_of(T, b, na, idt, eps, st)
           for T, b, na, idt, st in zip(state["rows"], state["basis"], state["nact"], ident, state["status"])]
    return {f: np.concatenate([p[f] for p in per]) for f in FIELDS}


def assert_same(got, want, fields=FIELDS):
    for f in fields:
        g, w = bits(got[f]), bits(want[f])
        assert g.shape == w.shape, f"{f}: {g.shape} against {w.shape}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{f}: {bad.size} of {g.size} differ, first at {bad[0]}: {got[f][bad[0]]!r} against {want[f][bad[0]]!r}"


def digest(arrays):
    """The 64-bit FNV-1a digest of the nine arrays' bytes in FIELDS order, as host/lpgcli.c --ranging prints it."""
    h = 0xcbf29ce484222325
    for f in FIELDS:
        for byte in np.ascontiguousarray(arrays[f]).tobytes():
            h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---------------------------------------------------------------------------
# the device cases (tests/test_gpu_batch_ranging.py runs them, tests/test_ranging_cases.py counts what they hold)
# ---------------------------------------------------------------------------
CASES = {
    "dense-3x4": uniform("dense", 3, 4),                    # fewer rows than waves
    "dense-5x3": uniform("dense", 5, 3),                    # one partial wave of columns
    "dense-37x70": uniform("dense", 37, 70),                # ncols between 64 and 128
    "dense-64x128": uniform("dense", 64, 128),
    "dense-130x130": uniform("dense", 130, 130),            # the global-tier solve in front
    "artificial-8x8": uniform("artificial", 8, 8),          # nact < N, ident behind nact, kept artificials
    "artificial-33x33": uniform("artificial", 33, 33),
    "interval-12x20": uniform("primal", 12, 20),
    "interval_art-12x20": uniform("interval_art", 12, 20),  # the mixed statuses: NaN / none outputs
    "interval-70x150": uniform("primal", 70, 150),          # ties across lanes and in a lane's stride
    "interval-40x300": uniform("primal", 40, 300),          # ncols > 256
    "interval-300x40": uniform("primal", 300, 40),          # m > 256: a lane takes two frame rows
}
RAGGED = [lp("dense", 3, 4, SEED), lp("artificial", 33, 33, SEED + 1), lp("primal", 70, 150, 2), lp("interval_art", 12, 20, 1),
          lp("dense", 37, 70, SEED + 2), lp("artificial", 8, 8, SEED + 3)]
