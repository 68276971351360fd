"""Goal-batch test plumbing (tests/test_goal_cases.py, tests/test_gpu_batch_goal.py,
tests/batch_worker.py), in the style of tests/batch3_cases.py.

The statement of include/lpg.h's "goal programmes" section, restated on the CPU
with no new oracle code: the decisions (pricing classes, the winner, the ratio
test, the order of the checks) are numpy comparisons and one division, the
arithmetic is the committed oracle's. oracle/lpo.c's lpo_pivot gives every row
but r the same fma, so a goal tableau of m + K rows loaded into an
Oracle(m + K - 1, ncols) -- the first K - 1 objective rows as extra "constraint"
rows -- is updated exactly by Oracle.pivot(k, r), and Oracle.set_objective on an
m-row oracle yields each objective row.

A case is a JSON-able dict; build(spec) gives (A[B, m, ncols], basis[B, m],
costs[B, K, N]); run_batch(spec) runs it on the device through a goal
BatchEngine, run_statement(spec) through the statement, one LP at a time, and
assert_same compares the two bit for bit: batch_cases.assert_same plus attain.

spec keys: case (a generator or literal below) with its parameters, B, rule,
budgets (one solve_goal call each), only (solve LP `only` alone in a batch of 1).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import batch_cases as bc

RUNNING, OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, NUMERIC = 0, 1, 2, 3, 4, 5
DANTZIG, BLAND = 0, 1
EPS = 1e-9


# ---------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------

def classes(D, eps_opt, block=True):
    """(class, value) of every column of the K rows D[K, N]: the first level k with d_k < -eps (class -1: not
    eligible); a level before it that is not within [-eps, eps] blocks the column (``block=False``: the mutation
    of the census, which walks past a positive or NaN level)."""
    K, N = D.shape
    cls, val, open_ = np.full(N, -1, dtype=np.int64), np.zeros(N), np.ones(N, dtype=bool)
    for k in range(K):
        neg = D[k] < -eps_opt
        take = open_ & neg
        cls[take], val[take] = k, D[k][take]
        open_ &= ~neg
        if block:
            open_ &= D[k] <= eps_opt
    return cls, val


def winner(cls, val, rule):
    """The entering column (1-based) or -1, and how many columns tie at the winning (class, value)."""
    el = np.flatnonzero(cls >= 0)
    if el.size == 0:
        return -1, 0
    if rule == BLAND:
        return int(el[0]) + 1, 1
    e2 = el[cls[el] == cls[el].min()]
    e3 = e2[val[e2] == val[e2].min()]
    return int(e3[0]) + 1, int(e3.size)


def ratio_row(T, m, k, basis, rule, eps_piv):
    """lpo.c ratio_block / cand_less over rows 0..m-1 of column k: the leaving row or -1."""
    best = None
    with np.errstate(all="ignore"):
        for i in range(m):
            a = T[i, k]
            if not (a > eps_piv):
                continue
            b = T[i, 0]
            cand = (b / a if b > 0.0 else np.float64(0.0), int(basis[i]) if rule == BLAND else i, i)
            if best is None:
                best = cand
                continue
            an, bn = cand[0] != cand[0], best[0] != best[0]
            if an != bn:
                less = bn
            elif not an and cand[0] != best[0]:
                less = cand[0] < best[0]
            else:
                less = cand[1] < best[1]
            if less:
                best = cand
    return -1 if best is None else best[2]


class Statement:
    """One goal programme: load, then solve(costs, budget, rule) as often as wanted. ``census``: a dict that
    collects, per pricing, what tests/test_goal_cases.py's census counts."""

    def __init__(self, A, basis, K, eps=(EPS, EPS), census=None):
        from oracle.lpo import Oracle
        self.m, self.ncols, self.K = A.shape[0], A.shape[1], K
        self.eps_piv, self.eps_opt = eps
        self.T = np.zeros((self.m + K, self.ncols))
        self.T[:self.m] = A
        self.basis = np.array(basis, dtype=np.int64)
        self.small = Oracle(self.m, self.ncols)
        self.big = Oracle(self.m + K - 1, self.ncols)
        self.pivots, self.last_k, self.last_r, self.logk, self.logr = 0, -1, -1, [], []
        self.census = census

    def close(self):
        self.small.close()
        self.big.close()

    def _objective_rows(self, costs):
        m = self.m
        self.small.load_tableau(self.T[:m + 1], self.basis)
        for k in range(self.K):
            self.small.set_objective(np.append(costs[k], 0.0))     # N costs; the trailing entry is never read
            self.T[m + k] = self.small.get_rows(m, 1)[0]

    def solve(self, costs, budget, rule):
        m, K = self.m, self.K
        self._objective_rows(np.asarray(costs, dtype=np.float64))
        self.big.load_tableau(self.T, np.append(self.basis, np.ones(K - 1, dtype=np.int64)))
        done = 0
        while True:
            cls, val = classes(self.T[m:, 1:], self.eps_opt)
            k, ties = winner(cls, val, rule)
            if self.census is not None and k >= 0:
                alt, _ = winner(*classes(self.T[m:, 1:], self.eps_opt, block=False), rule)
                c = self.census
                c["pricings"] = c.get("pricings", 0) + 1
                c["arm"] = c.get("arm", 0) + (alt != k)
                c["ties"] = c.get("ties", 0) + (rule == DANTZIG and ties > 1)
            if k < 0:
                status = OPTIMAL
                break
            if done >= budget:
                status = ITER_LIMIT
                break
            r = ratio_row(self.T, m, k, self.basis, rule, self.eps_piv)
            if r < 0:
                status = UNBOUNDED
                break
            if not np.isfinite(self.T[r, k]) or not np.isfinite(self.T[r, 0]):
                status = NUMERIC
                break
            if self.census is not None:
                self.census.setdefault("classes", {})
                self.census["classes"][int(cls[k - 1])] = self.census["classes"].get(int(cls[k - 1]), 0) + 1
            self.big.pivot(k, r)
            self.T = self.big.get_rows()
            self.basis[r] = k
            self.logk.append(k)
            self.logr.append(r)
            self.pivots, self.last_k, self.last_r = self.pivots + 1, k, r
            done += 1
        return SimpleNamespace(status=status, pivots=self.pivots, objective=self.T[m + K - 1, 0], entering=self.last_k,
                               leaving=self.last_r)


def statement(A, basis, costs, budgets, rule, eps=(EPS, EPS), census=None):
    """One LP through the statement, one solve call per budget: (results per call, T[m + K, ncols], basis, log k,
    log r, attain[K])."""
    costs = np.asarray(costs, dtype=np.float64)
    s = Statement(np.asarray(A, dtype=np.float64), basis, costs.shape[0], eps, census)
    try:
        res = [s.solve(costs, budget, rule) for budget in budgets]
        return res, s.T.copy(), s.basis.copy(), np.array(s.logk, dtype=np.int64), np.array(s.logr, dtype=np.int64), \
            s.T[s.m:, 0].copy()
    finally:
        s.close()


# ---------------------------------------------------------------------------
# the literals and generators
# ---------------------------------------------------------------------------

def textbook():
    """min P1 d1+, P2 (d2- + d2+), P3 d3-;  2x1 + x2 <= 11;  x1 - x2 + d1- - d1+ = 0;  x1 + 2x2 + d2- - d2+ = 10;
    8x1 + 10x2 + d3- - d3+ = 56. Columns [b | x1 x2 | d1- d1+ d2- d2+ d3- d3+ | s]: OPTIMAL after two pivots
    (classes 1, 2) at x = (2, 4), every level attained."""
    A = np.array([[11.0, 2, 1, 0, 0, 0, 0, 0, 0, 1],
                  [0.0, 1, -1, 1, -1, 0, 0, 0, 0, 0],
                  [10.0, 1, 2, 0, 0, 1, -1, 0, 0, 0],
                  [56.0, 8, 10, 0, 0, 0, 0, 1, -1, 0]])
    basis = np.array([9, 3, 5, 7], dtype=np.int64)
    costs = np.zeros((3, 9))
    costs[0, 3] = -1.0                     # d1+ (column 4)
    costs[1, 4] = costs[1, 5] = -1.0       # d2-, d2+
    costs[2, 6] = -1.0                     # d3-
    return A, basis, costs


def textbook_model():
    """textbook() as a frontend.GoalModel."""
    from linearprogramming_amd import frontend as F
    return F.GoalModel(A=[[2, 1]], sense=[-1], b=[11], G=[[1, -1], [1, 2], [8, 10]], target=[0, 10, 56],
                       under=[None, (2, 1.0), (3, 1.0)], over=[(1, 1.0), (2, 1.0), None])


def ladder():
    """K = 8, m = 16, 33 columns: hard row k  x_k + s_k = 10 + k, goal k  x_k + d- - d+ = 2 + k at level k with
    weight k + 1 on d-. Before any pivot d_k[x_k] = -(k + 1): the lower levels have the larger |d|, so a pricing
    that ranks value before class enters x_8 first; the statement enters x_1, x_2, ..., x_8, d-_k leaving."""
    K = 8
    A, basis, costs = np.zeros((16, 33)), np.zeros(16, dtype=np.int64), np.zeros((K, 32))
    for k in range(K):
        A[k, 0], A[k, 1 + k], A[k, 25 + k] = 10.0 + k, 1.0, 1.0
        A[8 + k, 0], A[8 + k, 1 + k], A[8 + k, 9 + 2 * k], A[8 + k, 10 + 2 * k] = 2.0 + k, 1.0, 1.0, -1.0
        basis[k], basis[8 + k] = 25 + k, 9 + 2 * k
        costs[k, 9 + 2 * k - 1] = -(k + 1.0)
    return A, basis, costs


def graded(hard, goals, n, K, seed):
    """Hard rows a.x <= b, a in 1..5, b in 30..59; goal i at level i % K, coefficients 1..4 at density 0.5 (one at
    least), target randint(2, 6) * (1 + 3 * level), weight 1..3 on its under-achievement. The graded targets are
    what spreads the pivots over the classes. Columns [b | x | d-_1 d+_1 .. | slacks]."""
    rng = np.random.RandomState(seed)
    m, ncols = hard + goals, 1 + n + 2 * goals + hard
    A, basis, costs = np.zeros((m, ncols)), np.zeros(m, dtype=np.int64), np.zeros((K, ncols - 1))
    for i in range(hard):
        A[i, 1:1 + n] = rng.randint(1, 6, size=n)
        A[i, 0] = rng.randint(30, 60)
        A[i, 1 + n + 2 * goals + i] = 1.0
        basis[i] = 1 + n + 2 * goals + i
    for i in range(goals):
        level = i % K
        coef = rng.randint(1, 5, size=n) * (rng.random_sample(n) < 0.5)
        if not coef.any():
            coef[rng.randint(n)] = rng.randint(1, 5)
        r, dm = hard + i, 1 + n + 2 * i
        A[r, 1:1 + n] = coef
        A[r, 0] = rng.randint(2, 7) * (1 + 3 * level)
        A[r, dm], A[r, dm + 1] = 1.0, -1.0
        basis[r] = dm
        costs[level, dm - 1] = -float(rng.randint(1, 4))
    return A, basis, costs


def edges():
    """Pricing edges, K = 3, m = 2, columns [b | x1..x4 | s1 s2] on the unit basis (s1, s2) with zero basic costs,
    so that d_k[j] = -c_k[j] exactly. One LP per edge; (name, d[K][4]) with the rest zero."""
    nan, inf, e = np.nan, np.inf, EPS
    below, above = np.nextafter(-e, -np.inf), np.nextafter(e, np.inf)
    lps = [
        ("minus_eps_not_eligible", [[-e, 0, 0, 0], [0] * 4, [0] * 4]),
        ("below_minus_eps_eligible", [[0, below, 0, 0], [0] * 4, [0] * 4]),
        ("plus_eps_does_not_block", [[e, 0, 0, 0], [-1.0, 0, 0, 0], [0] * 4]),
        ("above_plus_eps_blocks", [[above, 0, 0, 0], [-1.0, 0, 0, 0], [0] * 4]),
        ("nan_and_inf_block", [[nan, inf, 0, 0], [-1.0, -1.0, 0, 0], [0, 0, 0, 0]]),
        ("minus_inf_wins_its_class", [[0, -1.0, -inf, -2.0], [-5.0, 0, 0, 0], [0] * 4]),
        ("nan_below_the_class_is_ignored", [[0, 0, 0, 0], [0, 0, -1.0, 0], [0, 0, nan, -3.0]]),
        ("class_before_value", [[0, 0, 0, -1.0], [-5.0, -7.0, 0, 0], [-9.0, 0, 0, 0]]),
        ("blocked_at_the_second_level", [[0, 0, 0, 0], [1.0, 0, 0, 0], [-1.0, -0.5, 0, 0]]),
    ]
    B = len(lps)
    A, basis, costs = np.zeros((B, 2, 7)), np.zeros((B, 2), dtype=np.int64), np.zeros((B, 3, 6))
    for q, (_, d) in enumerate(lps):
        A[q, :, 0] = [2.0 + q, 3.0 + q]
        A[q, :, 1:5] = [[1.0, 2.0, 1.0, 3.0], [2.0, 1.0, 1.0, 1.0]]
        A[q, 0, 5] = A[q, 1, 6] = 1.0
        basis[q] = [5, 6]
        costs[q, :, :4] = -np.array(d, dtype=np.float64)
    return [name for name, _ in lps], A, basis, costs


def statuses():
    """K = 2, m = 2, columns [b | x1 x2 | s1 s2]. LP 0 UNBOUNDED: x2 enters at level 0, then x1 (column (0, -1)) is
    a ray at level 1. LP 1 NUMERIC: the entering column's entry in row 0 is +inf (ratio 0, the pivot element).
    LP 2: OPTIMAL after one pivot."""
    A = np.array([[[2.0, 0, 1, 1, 0], [3.0, -1, 1, 0, 1]],
                  [[1.0, np.inf, 1, 1, 0], [3.0, 1, 1, 0, 1]],
                  [[2.0, 1, 1, 1, 0], [3.0, 1, 2, 0, 1]]])
    basis = np.array([[3, 4]] * 3, dtype=np.int64)
    costs = np.zeros((3, 2, 4))
    costs[0, 0, 1], costs[0, 1, 0] = 1.0, 1.0
    costs[1, 0, 2] = -1.0                  # c_B of row 0 is -1: d_0[x1] = -inf, and x1's entry in row 0 is the pivot element
    costs[2, 1, 1] = 1.0
    return A, basis, costs


def artificial(m, n, K, B, seed):
    """The generator's artificial LPs (lpo_generate kind 2, seed + LP) as goal programmes of K = 1 (the real
    costs) or K = 2 (level 0: -1 on the artificial columns; level 1: the real costs, 0 on the artificials: Big-M).
    Returns build()'s triple and art_first."""
    from oracle.lpo import Oracle
    nc = n + m + 1
    af = 1 + n + (m + 1) // 2
    A, basis, costs = np.zeros((B, m, nc)), np.zeros((B, m), dtype=np.int64), np.zeros((B, K, nc - 1))
    for b in range(B):
        o = Oracle(m, nc)
        o.generate(n, seed + b, 2)
        T = o.get_rows()
        o.close()
        A[b], basis[b] = T[:m], o_basis(m, n)
        real = -T[m, 1:]
        if K == 1:
            costs[b, 0] = real
        else:
            costs[b, 0, af - 1:] = -1.0
            costs[b, 1, :af - 1] = real[:af - 1]
    return A, basis, costs, af


def o_basis(m, n):
    return np.array([(1 + n + (m + 1) // 2 + i // 2) if i & 1 else (1 + n + i // 2) for i in range(m)], dtype=np.int64)


def lds_bytes(m, ncols, K):
    """lpg_batch.hip's LDS-tier footprint of a tableau of m + K rows."""
    rows = m + K
    return 8 * (ncols + rows + rows * (ncols | 1) + (m + 1) // 2)


def boundary_goals(K, hard=2, n=8, cap=150 * 1024):
    """g: graded(hard, g, n, K) is the last shape on the LDS tier, graded(hard, g + 1, n, K) the first beyond it."""
    g = 1
    while lds_bytes(hard + g + 1, 1 + n + 2 * (g + 1) + hard, K) <= cap:
        g += 1
    return g


def spec(case, B=8, rule=0, **kw):
    s = {"case": case, "B": B, "rule": rule, "budgets": [100000], "only": None, "seed": 100, "hard": 0, "goals": 0, "n": 0,
         "K": 0, "m": 0}
    s.update(kw)
    return s


def graded_spec(hard, goals, n, K, B, seed=100, rule=0, **kw):
    return spec("graded", B=B, rule=rule, hard=hard, goals=goals, n=n, K=K, seed=seed, **kw)


def build(s):
    """(A[B, m, ncols], basis[B, m], costs[B, K, N]) of the case."""
    c, B = s["case"], s["B"]
    if c == "textbook" or c == "ladder":
        A, basis, costs = textbook() if c == "textbook" else ladder()
        out = (np.array([A] * B), np.array([basis] * B), np.array([costs] * B))
    elif c == "graded":
        lps = [graded(s["hard"], s["goals"], s["n"], s["K"], s["seed"] + b) for b in range(B)]
        out = tuple(np.array([lp[i] for lp in lps]) for i in range(3))
    elif c == "edges":
        out = edges()[1:]
    elif c == "statuses":
        out = statuses()
    elif c == "artificial":
        out = artificial(s["m"], s["n"], s["K"], B, s["seed"])[:3]
    else:
        raise ValueError(c)
    if s["only"] is not None:
        out = tuple(a[s["only"]:s["only"] + 1] for a in out)
    return out


def _pack(results_per_lp, rows, basis, logs, attain, logcap):
    calls = [[res[c].status for res in results_per_lp] for c in range(len(results_per_lp[0]))]
    out = bc._pack([res[-1] for res in results_per_lp], rows, basis, logs, calls, logcap)
    out["attain"] = np.asarray(attain, dtype=np.float64)
    return out


def run_statement(s, census=None):
    """Every LP of the case through the statement."""
    A, basis, costs = build(s)
    m, nc = A.shape[1], A.shape[2]
    logcap = 2 * (m + nc)
    per_lp, rows, bas, logs, attain = [], [], [], [], []
    for b in range(A.shape[0]):
        res, T, bs, lk, lr, at = statement(A[b], basis[b], costs[b], s["budgets"], s["rule"], census=census)
        per_lp.append(res)
        rows.append(T)
        bas.append(bs)
        logs.append((lk[:logcap], lr[:logcap]))
        attain.append(at)
    return _pack(per_lp, np.array(rows), np.array(bas), logs, attain, logcap)


def run_batch(s):
    """The case on the device; also returns info.tier / chunk / nobj."""
    import linearprogramming_amd as lpg
    A, basis, costs = build(s)
    B, m, nc = A.shape
    K = costs.shape[1]
    T = np.zeros((B, m + K, nc))
    T[:, :m] = A
    # the costs travel with padding that must never be read: 3 doubles behind every level, 5 behind every LP
    padded = np.full((B, K * (nc - 1 + 3) + 5), 1e300)
    for k in range(K):
        padded[:, k * (nc + 2):k * (nc + 2) + nc - 1] = costs[:, k]
    e = lpg.BatchEngine(B, m, nc, levels=K)
    try:
        e.load(T, basis)
        calls, attain, res = [], None, None
        for budget in s["budgets"]:
            r = (lpg._lib.Result * B)()
            attain = np.zeros((B, K))
            e._check(e.lib.lpg_batch_solve_goal(e._b, padded.ctypes.data_as(lpg._lib.c_double_p), padded.shape[1], nc + 2, budget,
                                                s["rule"], r, attain.ctypes.data_as(lpg._lib.c_double_p)), "lpg_batch_solve_goal")
            res = [SimpleNamespace(status=x.status, pivots=x.pivots, objective=x.objective, entering=x.entering,
                                   leaving=x.leaving) for x in r]
            calls.append([x.status for x in res])
        info = e.info
        out = bc._pack(res, e.get_rows(), e.get_basis(), [e.get_log(b) for b in range(B)], calls, info.log_capacity)
        out["attain"] = attain
        for key in ("tier", "chunk", "nobj"):
            out[key] = np.array(getattr(info, key), dtype=np.int64)
        return out
    finally:
        e.close()


def assert_same(got, want, nonfinite=False):
    """batch_cases.assert_same plus attain; ``nonfinite``: tie_cases.assert_same_nonfinite's rule for NaNs (where
    the statement's entry is a NaN the device's must be one, its sign and payload left out)."""
    if not nonfinite:
        bc.assert_same(got, want)
        assert np.array_equal(bc.bits(got["attain"]), bc.bits(want["attain"])), ("attain", got["attain"], want["attain"])
        return
    for key in ("calls", "status", "pivots", "entering", "leaving", "basis", "logcap", "loglen", "logk", "logr"):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    for key in ("objective", "attain", "rows"):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (key, "NaN-ness differs first at", np.argwhere(np.isnan(g) != nan)[0].tolist())
        diff = np.argwhere((bc.bits(g) != bc.bits(w)) & ~nan)
        assert diff.size == 0, (key, "differs first at", diff[0].tolist())


# the graded cases of the census and of tests/test_gpu_batch_goal.py: (hard, goals, n, K, B, seed). LP b of a case is
# graded(.., seed + b); the seeds were chosen by walking the statement (tests/test_goal_cases.py's census), which
# the smallest shape meets at few seeds only: (2, 3, 3, 3) has some 110 pricings in all
GRADED = [(2, 3, 3, 3, 16, 500), (4, 8, 8, 4, 16, 100), (6, 16, 16, 8, 8, 100), (8, 9, 300, 3, 4, 100)]
