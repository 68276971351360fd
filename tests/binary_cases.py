"""0-1 programs as include/lpg.h ("0-1 programs") states them, restated in
numpy operation for operation, and the cases the binary tests share.

`enumerate01` is the definition: implicit enumeration, depth first, preferred
value first, column 0 outermost. On the integer data the library admits every
operation below is exact, so the device is held to it bit for bit
(tests/test_gpu_binary.py) and the definition itself to brute force in the same
order (tests/test_binary_cases.py). `enumerate_split` is the split reduction
on top of it, `generate` the library's generator restated.

A spec is a JSON-able dict {"shape": [m, n], "maximize": bool, "seed": int,
"kinds": [...], "split": int}: one batch with one problem per entry of
`kinds`. `run_batch` runs a spec on the device (also from
tests/batch_worker.py, for the runs under LPG_BINARY_TIER / LPG_BINARY_CHUNK,
which a batch reads when it is created).
"""
from __future__ import annotations

import functools
import json
import os
import subprocess
import sys

import numpy as np

OPTIMAL, INFEASIBLE, ITER_LIMIT = 1, 3, 4
INF = float("inf")
M64 = (1 << 64) - 1


def bounds(sense, rhs):
    """The two-sided form L <= a.x <= U of every row."""
    sense, rhs = np.asarray(sense), np.asarray(rhs, dtype=np.float64)
    return np.where(sense < 0, -INF, rhs), np.where(sense > 0, INF, rhs)


def enumerate01(A, sense, rhs, c, maximize=False, prefix=(), max_nodes=0):
    """include/lpg.h "0-1 programs", steps 1-3. `prefix`: per column t < len(prefix) 0 for its first value, 1 for
    its second; those levels are never unfixed (the sub-search of "Split"). max_nodes > 0: stop before visiting
    node max_nodes + 1. Returns a dict of status, found, objective (caller's sense; NaN if none), x [n] int8 (-1
    throughout if none), nodes, and inc, the internal minimising value."""
    A = np.asarray(A, dtype=np.float64) + 0.0
    m, n = A.shape
    c = np.asarray(c, dtype=np.float64)
    c = (0.0 - c) if maximize else (c + 0.0)
    L, U = bounds(sense, rhs)
    p = c < 0
    lo = np.minimum(0.0, A).sum(axis=1)
    hi = np.maximum(0.0, A).sum(axis=1)
    comp = A[:, p].sum(axis=1)
    z = float(np.minimum(0.0, c).sum())
    x = np.zeros(n, dtype=np.int8)

    def terms(j, v):
        a = A[:, j]
        if v:
            tl, th = np.maximum(0.0, a), np.minimum(0.0, a)
        else:
            tl, th = np.maximum(0.0, -a), -np.maximum(0.0, a)
        if v != p[j]:
            return tl, th, (a if v else -a), abs(c[j])
        return tl, th, 0.0, 0.0

    split = len(prefix)
    for t, second in enumerate(prefix):
        v = int(not p[t]) if second else int(p[t])
        tl, th, tc, tz = terms(t, v)
        lo, hi, comp, z = lo + tl, hi + th, comp + tc, z + tz
        x[t] = v
    d = split
    second = [False] * n
    inc, inc_x, nodes, running = INF, None, 0, True
    while running:
        if max_nodes > 0 and nodes >= max_nodes:
            break
        nodes += 1
        if z >= inc:
            prune = True
        elif (lo > U).any() or (hi < L).any():
            prune = True
        elif ((L <= comp) & (comp <= U)).all():
            inc = z
            inc_x = x.copy()
            inc_x[d:] = p[d:]
            prune = True
        else:
            prune = False
        if not prune:
            v = int(p[d])
            tl, th, tc, tz = terms(d, v)
            lo, hi, comp, z = lo + tl, hi + th, comp + tc, z + tz
            x[d], second[d] = v, False
            d += 1
            continue
        while d > split and second[d - 1]:
            d -= 1
            tl, th, tc, tz = terms(d, int(x[d]))
            lo, hi, comp, z = lo - tl, hi - th, comp - tc, z - tz
            x[d], second[d] = 0, False
        if d == split:
            running = False
            break
        d -= 1
        v = int(x[d])
        tl, th, tc, tz = terms(d, v)
        lo, hi, comp, z = lo - tl, hi - th, comp - tc, z - tz
        tl, th, tc, tz = terms(d, v ^ 1)
        lo, hi, comp, z = lo + tl, hi + th, comp + tc, z + tz
        x[d], second[d] = v ^ 1, True
        d += 1
    found = inc_x is not None
    return {"status": ITER_LIMIT if running else OPTIMAL if found else INFEASIBLE, "found": int(found),
            "objective": ((0.0 - inc) if maximize else inc) if found else float("nan"),
            "x": inc_x if found else np.full(n, -1, dtype=np.int8), "nodes": nodes, "inc": inc}


def enumerate_split(A, sense, rhs, c, maximize=False, split=0, max_nodes=0):
    """The problem as 2^split sub-searches that share no incumbent, and the reduction of lpg.h "Split": the
    smallest inc, x of the first sub-search in search order that reaches it, nodes summed; max_nodes per sub-search."""
    subs = []
    for k in range(1 << split):
        prefix = tuple((k >> t) & 1 for t in range(split))
        subs.append((prefix, enumerate01(A, sense, rhs, c, maximize, prefix, max_nodes)))
    subs.sort(key=lambda pr: pr[0])                          # search order: column 0 outermost, first value first
    best = None
    for _, r in subs:
        if r["found"] and (best is None or r["inc"] < best["inc"]):
            best = r
    running = any(r["status"] == ITER_LIMIT for _, r in subs)
    n = np.asarray(A).shape[1]
    return {"status": ITER_LIMIT if running else OPTIMAL if best else INFEASIBLE, "found": int(best is not None),
            "objective": best["objective"] if best else float("nan"),
            "x": best["x"] if best else np.full(n, -1, dtype=np.int8), "nodes": sum(r["nodes"] for _, r in subs),
            "inc": best["inc"] if best else INF}


def search_order(c, maximize=False):
    """Every point of {0,1}^n, [2^n, n], in the search order: column 0 outermost, a column's preferred value first."""
    c = np.asarray(c, dtype=np.float64)
    n = len(c)
    p = (((0.0 - c) if maximize else c) < 0).astype(np.int64)
    k = np.arange(1 << n, dtype=np.int64)[:, None]
    second = (k >> (n - 1 - np.arange(n))[None, :]) & 1      # point k: column 0 is the top bit of k
    return (second ^ p[None, :]).astype(np.float64)


def brute_force(A, sense, rhs, c, maximize=False):
    """All 2^n points in the search order: (status, objective, x of the first optimal point, number of optimal points)."""
    A, c = np.asarray(A, dtype=np.float64), np.asarray(c, dtype=np.float64)
    L, U = bounds(sense, rhs)
    X = search_order(c, maximize)
    act = X @ A.T
    ok = ((L[None, :] <= act) & (act <= U[None, :])).all(axis=1)
    if not ok.any():
        return INFEASIBLE, float("nan"), np.full(len(c), -1, dtype=np.int8), 0
    val = X @ c
    key = np.where(ok, -val if maximize else val, INF)
    first = int(np.argmin(key))                              # the first of the equal ones
    return OPTIMAL, float(val[first]) + 0.0, X[first].astype(np.int8), int(np.count_nonzero(key == key[first]))


# ---- the library's generator, restated ---------------------------------------

def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniform01(key, idx):
    """The engine's generator draw (oracle lpo_uniform)."""
    return float(splitmix64((key ^ ((idx * 0x9E3779B97F4A7C15) & M64)) & M64) >> 11) * 2.0 ** -53


def generate(m, n, key):
    """lpg_binary_generate's problem of key = seed + q (LPG_BINARY_GEN_BANDED): A, sense, rhs, c, the planted point."""
    key &= M64
    w = min(3, n)
    A = np.zeros((m, n))
    sense, rhs = np.zeros(m, dtype=np.int32), np.zeros(m)
    xp = np.array([uniform01(key, 4 * m + j) < 0.5 for j in range(n)], dtype=np.int8)
    for i in range(m):
        s = (i * (n - 3)) // (m - 1) if (m > 1 and n > 3) else 0
        for t in range(w):
            A[i, s + t] = np.floor(uniform01(key, 4 * i + t) * 9.0) - 4.0
        act = float(A[i] @ xp)
        r = uniform01(key, 4 * i + 3)
        if r < 0.5:
            sense[i], rhs[i] = 0, act
        elif r < 0.75:
            sense[i], rhs[i] = -1, act + 1.0
        else:
            sense[i], rhs[i] = 1, act - 1.0
    c = np.array([np.floor(uniform01(key, 4 * m + n + j) * 19.0) - 9.0 for j in range(n)])
    return A, sense, rhs, c, xp


# ---- problem kinds -----------------------------------------------------------
# banded: the generator's planted problems. knapsack, cover, mixed: dense, for n <= 12 only (dense problems of
# (8, 24) pass 50,000 nodes). equal, zero, first, inf_row, inf_combo: the banded problem with its costs or some
# rows replaced, so they end at every shape the banded problem ends at.
SMALL_KINDS = ("banded", "knapsack", "cover", "mixed", "equal", "zero", "inf_row", "inf_combo", "first")
LARGE_KINDS = ("banded", "equal", "zero", "inf_row", "inf_combo", "first")


def problem(kind, m, n, rng):
    seed = int(rng.integers(1, 1 << 40))
    if kind in ("banded", "equal", "zero", "first", "inf_row", "inf_combo"):
        A, sense, rhs, c, _ = generate(m, n, seed)
        if kind == "banded":
            pass
        elif kind == "equal":                             # every point of one weight costs the same: many optima
            c = np.full(n, 3.0)
        elif kind == "zero":                               # every feasible point is optimal
            c = np.zeros(n)
        elif kind == "first":                              # no row can be violated: the root's completion is feasible
            sense[:] = -1
            rhs = np.maximum(0.0, A).sum(axis=1)
        elif kind == "inf_row" or m < 2:                   # one row asks for more than its largest activity
            i = m // 2
            sense[i], rhs[i] = 1, np.maximum(0.0, A[i]).sum() + 1.0
        else:                                              # two rows, each feasible alone, exclude each other
            k = min(2, n)
            A[0], A[m - 1] = 0.0, 0.0
            A[0, :k], A[m - 1, :k] = 1.0, 1.0
            sense[0], rhs[0] = 1, float(k)
            sense[m - 1], rhs[m - 1] = -1, float(k - 1)
        return A, sense, rhs, c
    if kind == "knapsack":                                 # max value under weight rows, stated as a minimisation
        A = rng.integers(1, 10, size=(m, n)).astype(np.float64)
        return A, np.full(m, -1, dtype=np.int32), np.floor(A.sum(axis=1) / 2.0), -rng.integers(1, 10, size=n).astype(np.float64)
    if kind == "cover":
        A = (rng.random((m, n)) < 0.4).astype(np.float64)
        A[np.arange(m), rng.integers(0, n, size=m)] = 1.0
        return A, np.full(m, 1, dtype=np.int32), np.ones(m), rng.integers(1, 4, size=n).astype(np.float64)
    if kind == "mixed":
        A = rng.integers(-5, 6, size=(m, n)).astype(np.float64)
        xp = rng.integers(0, 2, size=n).astype(np.float64)
        sense = rng.integers(-1, 2, size=m).astype(np.int32)
        return A, sense, A @ xp - sense, rng.integers(-9, 10, size=n).astype(np.float64)
    raise ValueError(kind)


def spec(m, n, maximize=False, seed=0, kinds=SMALL_KINDS, split=0):
    return {"shape": [m, n], "maximize": bool(maximize), "seed": int(seed), "kinds": list(kinds), "split": int(split)}


def name(s):
    return f"{s['shape'][0]}x{s['shape'][1]}-{'max' if s['maximize'] else 'min'}-s{s['split']}-b{len(s['kinds'])}-{s['seed']}"


def data_of(s):
    """(A [count, m, n], sense [count, m], rhs [count, m], c [count, n]) of spec s; split plays no part."""
    m, n = s["shape"]
    rng = np.random.default_rng([20220518, m, n, int(s["maximize"]), s["seed"]])
    ps = [problem(k, m, n, rng) for k in s["kinds"]]
    return tuple(np.stack([p[f] for p in ps]) for f in range(4))


@functools.lru_cache(maxsize=None)
def _reference(key, max_nodes):
    s = json.loads(key)
    A, sense, rhs, c = data_of(s)
    return [enumerate_split(A[q], sense[q], rhs[q], c[q], s["maximize"], s["split"], max_nodes) for q in range(len(A))]


def reference(s, max_nodes=0):
    """enumerate_split() of every problem of spec s, cut at max_nodes per sub-search; computed once per process."""
    return _reference(json.dumps(s, sort_keys=True), int(max_nodes))


def stacked(refs):
    """A list of enumerate01 / enumerate_split results as the arrays run_batch returns."""
    return {"status": np.array([r["status"] for r in refs], dtype=np.int64),
            "found": np.array([r["found"] for r in refs], dtype=np.int64),
            "nodes": np.array([r["nodes"] for r in refs], dtype=np.int64),
            "objective": np.array([r["objective"] for r in refs], dtype=np.float64),
            "x": np.stack([r["x"] for r in refs]).astype(np.int8)}


def results_of(res, x):
    return {"status": np.array([r.status for r in res], dtype=np.int64),
            "found": np.array([r.found for r in res], dtype=np.int64),
            "nodes": np.array([r.nodes for r in res], dtype=np.int64),
            "objective": np.array([r.objective for r in res], dtype=np.float64), "x": x}


def run_data(A, sense, rhs, c, maximize=False, split=0, budgets=(0,)):
    """A batch on the device, solved in the budget steps given: the arrays of `stacked` after the last step (and
    under "k/" those after step k), and tier, rows_per_lane, chunk, launches."""
    import linearprogramming_amd as lpg
    A = np.asarray(A, dtype=np.float64)
    with lpg.BinaryBatch(A.shape[0], A.shape[1], A.shape[2], split=split, maximize=maximize) as b:
        b.load(A, sense, rhs, c)
        out = {}
        for k, mn in enumerate(budgets):
            got = results_of(b.solve(mn), b.get())
            for f, v in got.items():
                out[f"step{k}_{f}"] = v
        out.update(got)
        info = b.info
        out.update(tier=np.int64(info.tier), rows_per_lane=np.int64(info.rows_per_lane), chunk=np.int64(info.chunk),
                   launches=np.int64(info.launches), lds_bytes=np.int64(info.lds_bytes))
        return out


def run_batch(s):
    return run_data(*data_of(s), maximize=s["maximize"], split=s["split"], budgets=tuple(s.get("budgets", (0,))))


FIELDS = ("status", "found", "nodes", "objective", "x")


def assert_same(got, want, what="", prefix=""):
    """Bit for bit: integers equal, doubles compared as their 64-bit patterns (so -0 != +0 and NaN == NaN)."""
    for f in FIELDS:
        g, w = np.asarray(got[prefix + f]), np.asarray(want[f])
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        if w.dtype == np.float64:
            g, w = np.ascontiguousarray(g, dtype=np.float64).view(np.uint64), np.ascontiguousarray(w).view(np.uint64)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {f} differs at {bad[:5].tolist()} ({bad.shape[0]} entries)"


def in_subprocess(specs, env, tmp_path):
    """run_batch of every spec in a child process under `env` (tests/batch_worker.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    sp, op = os.path.join(str(tmp_path), "specs.json"), os.path.join(str(tmp_path), "out.npz")
    with open(sp, "w") as f:
        json.dump(specs, f)
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(here, "batch_worker.py"), "binary_cases", sp, op], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(op)
    return [{k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(f"{i}/")} for i in range(len(specs))]


# ---- the batches tests/test_gpu_binary.py runs --------------------------------
# every kind at small shapes, both senses; 9 problems: the last workgroup has idle waves
SMALL = [spec(m, n, mx) for (m, n) in ((3, 5), (5, 7), (4, 12)) for mx in (False, True)]
ONE = [spec(2, 3, kinds=("mixed",)), spec(1, 1, True, kinds=("banded",))]
# 131 problems in one batch: 33 workgroups, the last with one wave at work
MANY = [spec(5, 7, mx, seed=7, kinds=[SMALL_KINDS[k % 9] for k in range(131)]) for mx in (False, True)]
# the census shapes (m >= n - 1, where the banded problems end): 6 problems each. By rows per lane and tier:
# 1 / LDS up to (64, 32); 2 / LDS (65, 33); 2 / global (128, 63); 4 / global (129, 64), (256, 64) at split 0.
CENSUS_SHAPES = ((1, 1), (1, 2), (63, 31), (64, 32), (65, 33), (128, 63), (129, 64), (256, 64), (63, 64))
CENSUS = [spec(m, n, mx, kinds=LARGE_KINDS) for k, (m, n) in enumerate(CENSUS_SHAPES) for mx in (False, True)]
# searches of thousands of nodes (up to 13,227), past the default chunk: several launches
DEEP = [spec(48, 64, True, kinds=LARGE_KINDS), spec(40, 56, kinds=LARGE_KINDS), spec(24, 40, kinds=LARGE_KINDS)]
# four rows per lane in LDS: few columns, or sub-searches that share one copy of the problem
RPL4_LDS = [spec(129, 8, kinds=LARGE_KINDS[:5]), spec(256, 64, True, kinds=LARGE_KINDS, split=2)]
FORCED_GLOBAL = [spec(5, 7, True), spec(65, 33, kinds=LARGE_KINDS, split=1)]
CHUNKED = [spec(5, 7), spec(65, 33, True, kinds=LARGE_KINDS), spec(4, 5, split=2)]
SPLITS = [spec(4, 5, mx, split=sp) for sp in (0, 1, 3, 5) for mx in (False, True)]
# budget steps: after 1 node nothing has an incumbent but "first"; after 8 some have one and run on. (16, 64)
# does not end within 200,000 nodes: it is only ever cut.
BUDGET_STEPS = (1, 7, 0)
BUDGETED = [spec(5, 7), spec(65, 33, True, kinds=LARGE_KINDS), spec(4, 5, split=1)]
CUT_ONLY = [dict(spec(16, 64, kinds=("banded", "equal", "banded")), budgets=[3000])]
UNBUDGETED = SMALL + ONE + MANY + CENSUS + DEEP + RPL4_LDS + FORCED_GLOBAL + CHUNKED + SPLITS + BUDGETED
