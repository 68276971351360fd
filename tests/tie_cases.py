"""Tie, tolerance-boundary and non-finite batch cases (tests/test_tie_cases.py,
tests/test_gpu_batch_ties.py, tests/batch_worker.py), in the style of
tests/batch_cases.py.

The generator's LPs are continuous random data: no two reduced costs and no two
positive ratios are ever equal, nothing sits on a tolerance and everything is
finite, so the tie-breaking arms of pp_better / cand_better never run on them.
The LPs here are the opposite: interval_lp builds consecutive-ones (interval)
matrices, which are totally unimodular, with small integer b and c, so every
tableau entry stays in {-1, 0, 1}, every right-hand side, reduced cost and ratio
a small integer, every operation exact, and most pivots tie. census() walks the
oracle pivot by pivot and counts the ties by where the tied candidates sit in a
256-thread argmin (different waves: index // 64 differ; the same thread:
index % 256 equal), so the CPU tests can demand that the GPU cases are not
vacuous. A caller with another geometry passes its boundaries (census's
`bounds`; tests/engine_tie_cases.py: the single-LP engine's row and column
blocks, slices and ranks) and gets the ties that straddle them counted too.

A case is a JSON-able dict; run_batch(spec) runs it on the device,
run_oracle(spec) runs every LP through an Oracle of its own (computed once per
spec), and batch_cases.assert_same compares the two bit for bit.

spec keys: m, n, B, seed (LP b is interval_lp(m, n, seed + b, form)), method
("primal", "dual", "two_phase", "big_m"; it fixes the form), rule, budgets,
reserve_log, eps ([eps_piv, eps_opt] or None), scale (constraint rows, b
included, times this), lps (a ragged batch: [[m, n, seed], ...] instead of m, n,
B, seed), nonfinite (a non-finite case name: tableaus from nonfinite_batch).
"""
from __future__ import annotations

import json

import numpy as np

import batch_cases as bc
from batch_ragged_cases import lds_bytes

SEED = 1
RULE_DANTZIG, RULE_BLAND = 0, 1
OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, NUMERIC = 1, 2, 3, 4, 5
TIER_LDS, TIER_GLOBAL = 0, 1
LDS_CAP = 150 * 1024
FORM = {"primal": "primal", "dual": "dual", "two_phase": "artificial", "big_m": "artificial"}

# (40, 300): nact > 256: pricing ties across waves and inside a thread's stride; (70, 200) and (70, 150): m > 64,
# ratio ties across waves, the first beyond the LDS tier's 150 KiB and the second within; (300, 40): m > 256, ratio
# ties inside a thread's stride; (12, 20): every candidate in one wave
SHAPES = [(40, 300), (70, 200), (70, 150), (300, 40), (12, 20)]
BOUNDARY_SHAPES = [(40, 300), (300, 40)]
# eps_piv, eps_opt, scale: (a) reduced costs of exactly -1 (dual: b_i = -1) sit on eps_opt; (b) after a pivot on a 2
# the pivot row holds entries of exactly 1 = eps_piv
BOUNDARY = {"a": ([0.5, 1.0], 1), "b": ([1.0, 1e-9], 2)}


def unit_column(m, n, i, kind):
    """oracle lpo_unit_column / lpg_device.h unit_column."""
    if kind != 2:
        return 1 + n + i
    return 1 + n + (m + 1) // 2 + i // 2 if i & 1 else 1 + n + i // 2


def art_first_of(m, n):
    return 1 + n + (m + 1) // 2


def interval_lp(m, n, seed, form, shuffle=False):
    """(T[m+1, n+m+1], basis[m]): column j has ones in rows lo .. hi-1. "primal": A x <= b, b in 1..4, objective row
    -(1..3); "dual": -A x <= -b, b in 1..3, objective row +(1..3) (dual feasible, primal infeasible); "artificial":
    A x = b on odd rows (artificial unit columns), <= on even rows (slacks), laid out as the generator's kind 2.
    shuffle: the rows of A permuted (still totally unimodular), so that rows 256 apart, which no interval of at most
    m // 3 rows holds, meet in a column and can tie inside one thread's stride."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, m, n)
    hi = np.minimum(m, lo + 1 + rng.integers(0, max(1, m // 3), n))
    A = np.zeros((m, n))
    for j in range(n):
        A[lo[j]:hi[j], j] = 1.0
    if shuffle:
        A = A[np.random.default_rng([seed, 1]).permutation(m)]
    T = np.zeros((m + 1, n + m + 1))
    if form == "dual":
        T[:m, 0] = -(1.0 + rng.integers(0, 3, m))
        T[:m, 1:n + 1] = -A
        T[m, 1:n + 1] = 1.0 + rng.integers(0, 3, n)
    else:
        T[:m, 0] = 1.0 + rng.integers(0, 4, m)
        T[:m, 1:n + 1] = A
        T[m, 1:n + 1] = -(1.0 + rng.integers(0, 3, n))
    basis = np.array([unit_column(m, n, i, 2 if form == "artificial" else 0) for i in range(m)], dtype=np.int64)
    T[np.arange(m), basis] = 1.0
    return T, basis


def spec(m=None, n=None, method="primal", rule=0, B=8, **kw):
    s = {"m": m, "n": n, "B": B, "seed": SEED, "method": method, "rule": rule, "budgets": [20000], "reserve_log": None,
         "eps": None, "scale": 1, "lps": None, "nonfinite": None}
    s.update(kw)
    if s["reserve_log"] is None and s["lps"] is None and s["nonfinite"] is None:
        s["reserve_log"] = 4000                      # every run here is shorter (test_tie_cases.py checks)
    return s


# seeds at which the 8 LPs meet every floor. The dual at (300, 40) leaves rows uncovered and mostly ends INFEASIBLE
# after a few pivots, so few seeds bring enough LPs to a decision on the boundary; under setting (b) the 40
# structural columns of (300, 40) rarely tie with a slack beyond column 64
BOUNDARY_SEED = {(300, 40, "a", "dual"): 946, (300, 40, "b", "dual"): 4, (300, 40, "b", "primal"): 29}


def boundary_spec(m, n, which, method):
    eps, scale = BOUNDARY[which]
    return spec(m, n, method, eps=list(eps), scale=scale, seed=BOUNDARY_SEED.get((m, n, which, method), SEED))


def ragged_spec(method, rule=0):
    """The shapes interleaved, two LPs each: both tiers in one call."""
    return spec(method=method, rule=rule, lps=[[m, n, SEED + 10 * q + i] for i in range(2) for q, (m, n) in enumerate(SHAPES)])


METHODS = [("primal", RULE_DANTZIG), ("primal", RULE_BLAND), ("dual", RULE_DANTZIG), ("two_phase", RULE_DANTZIG),
           ("two_phase", RULE_BLAND), ("big_m", RULE_DANTZIG), ("big_m", RULE_BLAND)]


def interval_cases():
    """Every uniform interval case the GPU file runs: the shapes under every method and rule."""
    return [spec(m, n, method, rule) for m, n in SHAPES for method, rule in METHODS]


def boundary_cases():
    """The two tolerance settings, primal and dual, at BOUNDARY_SHAPES."""
    return [boundary_spec(m, n, w, method) for m, n in BOUNDARY_SHAPES for w in "ab" for method in ("primal", "dual")]


def case_id(s):
    tag = s["nonfinite"] or ("ragged" if s["lps"] is not None else f"{s['m']}x{s['n']}")
    eps = "" if s["eps"] is None else "-" + [w for w in BOUNDARY if BOUNDARY[w][1] == s["scale"]][0]
    return f"{tag}-{s['method']}{eps}-{'bland' if s['rule'] else 'dantzig'}"


def shapes_of(s):
    return [(m, n) for m, n, _ in s["lps"]] if s["lps"] is not None else [(s["m"], s["n"])] * s["B"]


def nobj_of(s):
    return 2 if s["method"] == "big_m" else 1


def expected_tier(m, n, nobj=1):
    """include/lpg.h: the LDS tier where tableau, P, C and the basis fit 150 KiB."""
    return TIER_LDS if lds_bytes(m, n + m + 1, nobj) <= LDS_CAP else TIER_GLOBAL


def build_lp(s, q):
    """(T[m + nobj, ncols], basis[m]) of LP q before any pivot."""
    if s["nonfinite"] is not None:
        T, basis = nonfinite_batch(s["nonfinite"])
        return T[q], basis[q]
    (m, n), seed = shapes_of(s)[q], (s["lps"][q][2] if s["lps"] is not None else s["seed"] + q)
    T, basis = interval_lp(m, n, seed, FORM[s["method"]], shuffle=m > 256)
    T[:m, :n + 1] *= float(s["scale"])
    if s["method"] == "big_m":                       # row m the (zero) M part, row m + 1 the objective
        T = np.vstack([T[:m], np.zeros((1, T.shape[1])), T[m:]])
    return T, basis


def count_of(s):
    return NONFINITE[s["nonfinite"]][2] if s["nonfinite"] is not None else len(shapes_of(s))


def _oracle_solver(s, m, n):
    if s["method"] == "primal":
        return lambda o, b, budget: o.solve(budget, s["rule"])
    if s["method"] == "dual":
        return lambda o, b, budget: o.solve_dual(budget)
    if s["method"] == "two_phase":
        return lambda o, b, budget: o.solve_two_phase(art_first_of(m, n), None, budget, s["rule"])
    return lambda o, b, budget: o.solve_big_m(art_first_of(m, n), None, budget, s["rule"])


def logcap_of(s):
    if s["reserve_log"] is not None:
        return s["reserve_log"]
    if s["nonfinite"] is not None:
        m, n = NONFINITE[s["nonfinite"]][:2]
        return 2 * (m + n + m + 1)
    return 2 * (max(m for m, _ in shapes_of(s)) + max(m + n + 1 for m, n in shapes_of(s)))


_ORACLE = {}


def run_oracle(s):
    """Every LP of the case through an Oracle of its own (computed once per spec; do not modify the result). A
    ragged case gives rows and basis packed, LP after LP."""
    from batch_ragged_cases import _merge
    key = json.dumps(s, sort_keys=True)
    if key not in _ORACLE:
        def prepare(o):
            if s["eps"] is not None:
                o.set_tolerances(*s["eps"])
        parts = []
        for q in range(count_of(s)):
            T, basis = build_lp(s, q)
            m = basis.shape[0]
            n = T.shape[1] - m - 1
            parts.append(bc.oracle_loop(T[None], basis[None], s["budgets"], _oracle_solver(s, m, n), logcap_of(s), prepare,
                                        nobj=nobj_of(s)))
        out = _merge(parts)
        if s["lps"] is None:
            m = parts[0]["basis"].shape[1]
            out["rows"] = out["rows"].reshape(len(parts), m + nobj_of(s), -1)
            out["basis"] = out["basis"].reshape(len(parts), m)
        _ORACLE[key] = out
    return _ORACLE[key]


def _solve_fn(e, s, af):
    if s["method"] == "primal":
        return lambda budget: e.solve(budget, s["rule"])
    if s["method"] == "dual":
        return lambda budget: e.solve_dual(budget)
    if s["method"] == "two_phase":
        return lambda budget: e.solve_two_phase(af, None, budget, s["rule"])
    return lambda budget: e.solve_big_m(af, None, budget, s["rule"])


def run_batch(s):
    """The case on the device; also returns tier and chunk (a ragged case: every LP's tier)."""
    import linearprogramming_amd as lpg
    built = [build_lp(s, q) for q in range(count_of(s))]
    if s["lps"] is not None:
        from batch_ragged_cases import read_back
        e = lpg.BatchEngine.ragged([(m, n + m + 1) for m, n in shapes_of(s)], big_m=s["method"] == "big_m")
        try:
            e.load([T for T, _ in built], [b for _, b in built])
            solve, calls = _solve_fn(e, s, [art_first_of(m, n) for m, n in shapes_of(s)]), []
            for budget in s["budgets"]:
                res = solve(budget)
                calls.append([r.status for r in res])
            return read_back(e, res, calls)
        finally:
            e.close()
    m = built[0][1].shape[0]
    nc = built[0][0].shape[1]
    e = lpg.BatchEngine(len(built), m, nc, big_m=s["method"] == "big_m")
    try:
        e.load(np.array([T for T, _ in built]), np.array([b for _, b in built]))
        if s["reserve_log"] is not None:
            e.reserve_log(s["reserve_log"])
        if s["eps"] is not None:
            e.set_tolerances(*s["eps"])
        return bc.solve_and_read_back(e, s["budgets"], _solve_fn(e, s, art_first_of(m, nc - m - 1)))
    finally:
        e.close()


def in_subprocess(specs, env, tmp_path):
    return bc.in_subprocess("tie_cases", specs, env, tmp_path)


# ---------------------------------------------------------------------------
# non-finite entries
# ---------------------------------------------------------------------------
# name -> (m, n, B, generator kind, method, budget); the bad LP is LP 3, the others the generator's LPs
NONFINITE = {
    "nan_b": (37, 70, 8, 0, "primal", 1000),
    "inf_b": (37, 70, 8, 0, "primal", 1000),
    "overflowing_ratio": (37, 70, 8, 0, "primal", 1000),
    "nan_ratio": (70, 20, 8, 0, "primal", 1000),
    "nan_ratio_stride": (300, 20, 8, 0, "primal", 1000),
    "nan_ratio_only": (37, 70, 8, 0, "primal", 1000),
    "dual_inf_b": (37, 70, 8, 3, "dual", 5),
    "dual_nan_ratio_stride": (12, 300, 8, 3, "dual", 5),
}
BAD_LP = 3


def nan_ratio_lp(T, m, n, nan_row=1, best_row=33):
    """Column 1 all ones and the first to enter, b_i = 2 + i except b_best = 0.5, and b = a = +inf in row nan_row,
    whose ratio is NaN: the pivot is (1, best_row) wherever nan_row is."""
    T = T.copy()
    T[:m, 1] = 1.0
    T[:m, 0] = 2.0 + np.arange(m)
    T[best_row, 0] = 0.5
    T[nan_row, 0] = T[nan_row, 1] = np.inf
    T[m, 1] = -100.0
    return T


def make_nonfinite(case, T, m, n):
    """The generator's tableau T [m+1, ncols] with the case's entries put in."""
    T = T.copy()
    if case == "nan_b":
        T[7, 0] = np.nan
    elif case == "inf_b":
        T[7, 0] = -np.inf
    elif case == "overflowing_ratio":                # b finite, b / a overflows for the entering column
        T[7, 0] = 1e308
        T[7, 1:n + 1] = 1e-10
    elif case == "nan_ratio":
        T = nan_ratio_lp(T, m, n)
    elif case == "nan_ratio_stride":                 # the NaN row and the best row in one thread's stride
        T = nan_ratio_lp(T, m, n, nan_row=1, best_row=257)
    elif case == "nan_ratio_only":                   # every eligible row of the entering column: b = a = +inf
        T[:m, 1] = 0.0
        T[[5, 9], 0] = T[[5, 9], 1] = np.inf
        T[m, 1] = -100.0
    elif case == "dual_inf_b":
        T[7, 0] = -np.inf
    elif case == "dual_nan_ratio_stride":            # row 0 leaves; column 2's ratio +inf / +inf is NaN, column 258,
        T[:m, 0] = -1.0                              # in the same thread's stride, holds the least
        T[0, 0] = -2.0
        T[0, 1:n + 1] = -1.0
        T[m, 1:n + 1] = 2.0 + np.arange(n)
        T[m, 258] = 0.5
        T[0, 2], T[m, 2] = -np.inf, np.inf
    else:
        raise ValueError(case)
    return T


_NONFINITE = {}


def nonfinite_batch(case):
    """(T[B, m+1, ncols], basis[B, m]): the generator's LPs of seeds bc.SEED .. + B - 1, LP 3 made non-finite."""
    from oracle.lpo import Oracle
    if case not in _NONFINITE:
        m, n, B, kind = NONFINITE[case][:4]
        T = np.zeros((B, m + 1, n + m + 1))
        basis = np.zeros((B, m), dtype=np.int64)
        for b in range(B):
            o = Oracle(m, n + m + 1)
            o.generate(n, bc.SEED + b, kind)
            T[b], basis[b] = o.get_rows(), o.get_basis()
            o.close()
        T[BAD_LP] = make_nonfinite(case, T[BAD_LP], m, n)
        _NONFINITE[case] = (T, basis)
    return _NONFINITE[case]


def nonfinite_spec(case, rule=0):
    method, budget = NONFINITE[case][4:]
    return spec(method=method, rule=rule, nonfinite=case, budgets=[budget])


def assert_same_nonfinite(got, want):
    """assert_same, a NaN's sign and payload left out: where the oracle's entry is a NaN the device's must be one,
    everywhere else the bits are equal. Returns the sign bits of the device's NaNs (measured on an MI355X: every
    NaN of these cases has it set, as x86's default NaN has; that is not part of the contract)."""
    for key in ("calls", "status", "pivots", "entering", "leaving", "basis", "logcap", "loglen", "logk", "logr"):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    for key in ("objective", "rows"):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (key, "NaN-ness differs first at", np.argwhere(np.isnan(g) != nan)[0].tolist())
        diff = np.argwhere((bc.bits(g) != bc.bits(w)) & ~nan)
        assert diff.size == 0, (key, "differs first at", diff[0].tolist())
    g = np.asarray(got["rows"])
    return np.unique(bc.bits(g[np.isnan(g)]) < 0)


# ---------------------------------------------------------------------------
# the census: the oracle walked one pivot at a time
# ---------------------------------------------------------------------------
KEYS = ("pivots", "price", "price_xwave", "price_thread", "price_cls1", "price_two_classes", "ratio", "ratio_pos",
        "ratio_zero", "ratio_xwave", "ratio_thread", "boundary")


def blocks_of(pos, b):
    """The block each position falls in: b an int, blocks of that width (pos // b); b a sorted list of first
    positions of the blocks after block 0 (the ranks of a row partition: [m * r // world for r in 1 .. world-1])."""
    pos = np.asarray(pos)
    return pos // b if isinstance(b, (int, np.integer)) else np.searchsorted(np.asarray(b), pos, side="right")


def bounds_keys(bounds):
    """The census keys that `bounds` adds: "<class>_x<name>" per boundary kind, class "ratio" or "price"."""
    return [f"{what}_x{name}" for what, names in sorted((bounds or {}).items()) for name in names]


def _where(stats, what, idx, bounds=None, pos=None):
    """Count one tie of the candidates at positions idx of a 256-thread argmin. bounds: {name: b}, further boundary
    kinds of this class (blocks_of): stats[what + "_x" + name] counts the ties whose candidates sit in more than one
    block; pos: their positions in that geometry where they are not idx (a column's physical index j = idx + 1)."""
    idx = np.asarray(idx)
    stats[what] += 1
    stats[what + "_xwave"] += len(set((idx // 64).tolist())) > 1
    stats[what + "_thread"] += len(set((idx % 256).tolist())) < len(idx)
    for name, b in (bounds or {}).items():
        stats[f"{what}_x{name}"] += len(set(blocks_of(idx if pos is None else pos, b).tolist())) > 1


def _argmin_ties(v, key):
    """(winner, tied): v's minimum, ties to the smallest key; positions into v."""
    tied = np.flatnonzero(v == v.min())
    return tied[np.argmin(key[tied])], tied


def price_np(R, m, nobj, nact, rule, eps_opt, strict=True):
    """lpo.c price on the rows R: (entering column or -1, the columns tied with it, its class, classes present)."""
    lt = (lambda x, y: x < y) if strict else (lambda x, y: x <= y)
    dR = R[m + nobj - 1, 1:nact + 1]
    if nobj == 1:
        cls = np.where(lt(dR, -eps_opt), 0, -1)
        v = dR
    else:
        dM = R[m, 1:nact + 1]
        c0 = lt(dM, -eps_opt)
        c1 = ~c0 & (dM <= eps_opt) & lt(dR, -eps_opt)
        cls = np.where(c0, 0, np.where(c1, 1, -1))
        v = np.where(c0, dM, dR)
    el = np.flatnonzero(cls >= 0)
    if el.size == 0:
        return -1, el, -1, set()
    if rule == RULE_BLAND:
        return int(el[0]) + 1, el[:1] + 1, int(cls[el[0]]), set(cls[el].tolist())
    top = el[cls[el] == cls[el].min()]
    w, tied = _argmin_ties(v[top], top)
    return int(top[w]) + 1, top[tied] + 1, int(cls[top[w]]), set(cls[el].tolist())


def ratio_np(R, basis, m, k, rule, eps_piv, strict=True):
    """lpo.c ratio_block on finite rows: (leaving row or -1, the rows tied with it, theta)."""
    a, b = R[:m, k], R[:m, 0]
    el = np.flatnonzero(a > eps_piv if strict else a >= eps_piv)
    if el.size == 0:
        return -1, el, 0.0
    theta = np.where(b[el] > 0.0, b[el] / a[el], 0.0)
    w, tied = _argmin_ties(theta, basis[el] if rule == RULE_BLAND else el)
    return int(el[w]), el[tied], float(theta[w])


def dual_np(R, m, nact, eps_piv, eps_opt, strict=True):
    """lpo.c lpo_solve_dual's choice: (leaving row or -1, rows tied, entering column or -1, columns tied)."""
    b = R[:m, 0]
    el = np.flatnonzero(b < -eps_opt if strict else b <= -eps_opt)
    if el.size == 0:
        return -1, el, -1, el
    w, tied = _argmin_ties(b[el], el)
    r, rt = int(el[w]), el[tied]
    a, d = R[r, 1:nact + 1], R[m, 1:nact + 1]
    ec = np.flatnonzero(a < -eps_piv if strict else a <= -eps_piv)
    if ec.size == 0:
        return r, rt, -1, ec
    v = np.where(d[ec] > 0.0, d[ec] / -a[ec], 0.0)
    w, tied = _argmin_ties(v, ec)
    return r, rt, int(ec[w]) + 1, ec[tied] + 1


def check_exact(R, m, scale):
    """The exactness premise: constraint entries in {-1, 0, 1} and everything an integer (scale 2: halves, within 2)."""
    A = R[:m, 1:]
    if scale == 1:
        assert np.isin(A, (-1.0, 0.0, 1.0)).all(), "a constraint entry outside {-1, 0, 1}"
        assert np.array_equal(R, np.rint(R)) and np.abs(R).max() < 2 ** 20
    else:
        assert np.array_equal(2 * R, np.rint(2 * R)) and np.abs(A).max() <= 2.0 and np.abs(R).max() < 2 ** 20


def _walk_primal(o, m, nobj, nact, rule, eps, scale, st, budget=20000, bounds=None):
    """lpo_solve on oracle o, one pivot per call, every choice redone in numpy and counted. Returns the status."""
    eps_piv, eps_opt = eps
    for _ in range(budget):
        R, basis = o.get_rows(), o.get_basis()
        check_exact(R, m, scale)
        k, kt, cls, present = price_np(R, m, nobj, nact, rule, eps_opt)
        k2 = price_np(R, m, nobj, nact, rule, eps_opt, strict=False)[0]
        if k < 0:
            st["boundary"] += k2 != k
            return OPTIMAL
        r, rt, theta = ratio_np(R, basis, m, k, rule, eps_piv)
        r2 = ratio_np(R, basis, m, k2, rule, eps_piv, strict=False)[0]
        st["boundary"] += (k2, r2) != (k, r)
        if r < 0:
            return UNBOUNDED
        if len(kt) > 1:
            _where(st, "price", kt - 1, (bounds or {}).get("price"), kt)
            st["price_cls1"] += cls == 1
        st["price_two_classes"] += len(present) > 1
        if len(rt) > 1:
            _where(st, "ratio", rt, (bounds or {}).get("ratio"))
            st["ratio_pos" if theta > 0 else "ratio_zero"] += 1
        before = o.solve(0, rule).pivots
        res = o.solve(1, rule)
        lk, lr = o.get_log()
        assert res.pivots == before + 1 and (lk[-1], lr[-1]) == (k, r), ("numpy and the oracle differ", k, r, lk[-1], lr[-1])
        st["pivots"] += 1
    return ITER_LIMIT


def _walk_dual(o, m, nact, eps, scale, st, budget=20000, bounds=None):
    eps_piv, eps_opt = eps
    for _ in range(budget):
        R = o.get_rows()
        check_exact(R, m, scale)
        r, rt, k, kt = dual_np(R, m, nact, eps_piv, eps_opt)
        r2, _, k2, _ = dual_np(R, m, nact, eps_piv, eps_opt, strict=False)
        st["boundary"] += (k2, r2) != (k, r)
        if r < 0:
            return OPTIMAL
        if k < 0:
            return INFEASIBLE
        if len(rt) > 1:
            _where(st, "price", rt, (bounds or {}).get("price"))   # the leaving row plays pricing's part
        if len(kt) > 1:
            _where(st, "ratio", kt - 1, (bounds or {}).get("ratio"), kt)
            st["ratio_pos" if R[m, k] > 0 else "ratio_zero"] += 1
        # solve_dual(1) would test dual feasibility again in front of every pivot, which one long call does not do
        # (tolerance setting (b) leaves it on the way): numpy's pivot is applied, and census() compares the log
        o.pivot(k, r)
        st["pivots"] += 1
    return ITER_LIMIT


def census(T, basis, method, rule, eps=(1e-9, 1e-9), scale=1, bounds=None):
    """One LP walked through the oracle a pivot at a time (solve(1) / solve_dual(1), get_rows in front of each),
    every pivot choice redone in numpy. Counts: pivots; price (pricing ties; the dual: leaving-row ties), of them
    price_xwave (tied candidates in different waves) and price_thread (in the same thread), price_cls1 (Big-M: ties
    among class-1 columns), price_two_classes (Big-M: pivots that priced both classes); ratio (ratio ties; the dual:
    entering-column ties) = ratio_pos (theta > 0) + ratio_zero, ratio_xwave, ratio_thread; boundary (pivots whose
    (k, r) differs under <= / >=). The index of a candidate is the column minus 1 (pricing, the dual's entering
    column) or the row (ratio test, the dual's leaving row). The log must equal the whole method's on a fresh oracle.
    bounds: {"ratio": {name: b}, "price": {name: b}}, the boundaries of the caller's geometry per class (blocks_of;
    rows are counted by row, columns by their physical index j, column 0 included, so for the dual "price" takes row
    boundaries and "ratio" column boundaries): the keys bounds_keys(bounds) count the ties whose candidates fall on
    both sides of one."""
    from oracle.lpo import Oracle
    st = dict.fromkeys(list(KEYS) + bounds_keys(bounds), 0)
    nobj = 2 if method == "big_m" else 1
    m, nc = basis.shape[0], T.shape[1]
    N, n = nc - 1, nc - 1 - m
    af = art_first_of(m, n)

    def fresh():
        o = Oracle(m, nc, nobj=nobj)
        o.load_tableau(T, basis)
        o.set_tolerances(*eps)
        return o

    o, ref = fresh(), fresh()
    if method == "primal":
        status = _walk_primal(o, m, 1, N, rule, eps, scale, st, bounds=bounds)
        want = ref.solve(20000, rule)
    elif method == "dual":
        status = _walk_dual(o, m, N, eps, scale, st, bounds=bounds)
        want = ref.solve_dual(20000)
    elif method == "two_phase":                      # lpo_solve_two_phase by hand
        cost = -T[m, 1:].copy()
        c1 = np.zeros(N)
        c1[af - 1:] = -1.0
        o.set_objective(c1)
        status = _walk_primal(o, m, 1, N, rule, eps, scale, st, bounds=bounds)
        R = o.get_rows()
        if status == OPTIMAL and not R[m, 0] < -1e-9 * max(1.0, np.abs(R[:m, 0]).sum()):
            for i in range(m):
                if o.get_basis()[i] >= af:
                    use = np.flatnonzero(np.abs(o.get_rows()[i, 1:af]) > eps[0])
                    if use.size:
                        o.pivot(int(use[0]) + 1, i)
            o.set_active_columns(af - 1)
            o.set_objective(cost)
            status = _walk_primal(o, m, 1, af - 1, rule, eps, scale, st, bounds=bounds)
        else:
            status = INFEASIBLE
        want = ref.solve_two_phase(af, None, 20000, rule)
    else:                                            # lpo_solve_big_m by hand
        cr = -T[m + 1, 1:].copy()
        cm = np.zeros(N)
        cr[af - 1:] = 0.0
        cm[af - 1:] = -1.0
        o.set_objective_m(cm)
        o.set_objective(cr)
        status = _walk_primal(o, m, 2, N, rule, eps, scale, st, bounds=bounds)
        R = o.get_rows()
        if status in (OPTIMAL, UNBOUNDED) and R[m, 0] < -1e-9 * max(1.0, np.abs(R[:m, 0]).sum()):
            status = INFEASIBLE
        want = ref.solve_big_m(af, None, 20000, rule)
    assert status == want.status, (status, want.status)
    for a, b in zip(o.get_log(), ref.get_log()):
        assert np.array_equal(a, b), "the walk's log is not the method's"
    assert np.array_equal(bc.bits(o.get_rows()), bc.bits(ref.get_rows()))
    st["loglen"] = len(ref.get_log()[0])
    o.close()
    ref.close()
    return st


_CENSUS = {}


def census_of(s, bounds=None):
    """census summed over the LPs of case s (computed once per spec and bounds), plus "maxlog", the longest log,
    and "minlog", the shortest."""
    key = json.dumps([s, bounds], sort_keys=True)
    if key not in _CENSUS:
        keys = list(KEYS) + bounds_keys(bounds)
        tot = dict.fromkeys(keys, 0)
        tot["maxlog"], tot["minlog"] = 0, 1 << 62
        for q in range(count_of(s)):
            T, basis = build_lp(s, q)
            st = census(T, basis, s["method"], s["rule"], tuple(s["eps"]) if s["eps"] else (1e-9, 1e-9), s["scale"], bounds)
            for k in keys:
                tot[k] += int(st[k])
            tot["maxlog"] = max(tot["maxlog"], st["loglen"])
            tot["minlog"] = min(tot["minlog"], st["loglen"])
        _CENSUS[key] = tot
    return _CENSUS[key]


def floors_of(s, m, n):
    """The tie classes shape (m, n) can produce under case s, each of which must occur at least 3 times: ties among
    columns in different waves where nact > 64 and in one thread where n > 256, ties among rows in different waves
    where m > 64 and in one thread where m > 256. Pricing under Bland takes the first eligible column: it has no
    ties, so its floors are the ratio test's. The same-thread floor of the columns asks for n > 256, not nact > 256:
    at (70, 200) and (300, 40) the columns from 257 on are slacks and artificials, whose reduced costs are
    multipliers that meet the least reduced cost of a structural column only by accident (0 to 2 such ties per case
    of 8 LPs over 50 runs of seeds), so those shapes cannot be made to produce the class; (40, 300) does."""
    nact = n + m
    rows, cols = ("price", "ratio") if s["method"] == "dual" else ("ratio", "price")
    if s["method"] == "dual" and s["scale"] == 2:
        nact = n                                     # a < -eps_piv = -1 leaves the -2s, which only structural columns hold
    need = []
    if not (cols == "price" and s["rule"] == RULE_BLAND):
        need += [cols] + ([cols + "_xwave"] if nact > 64 else []) + ([cols + "_thread"] if n > 256 else [])
    need += [rows] + ([rows + "_xwave"] if m > 64 else []) + ([rows + "_thread"] if m > 256 else [])
    return need
