"""The assignment problem as include/lpg.h ("assignment") states it, restated
in numpy operation for operation, and the cases the assignment tests share.

`hungarian` is the definition: every elementwise numpy operation below is the
one IEEE operation the header names, in the header's order, so the device is
held to it bit for bit (tests/test_gpu_assign.py) and the definition itself to
brute force (tests/test_assign_cases.py).

A spec is a JSON-able dict {"shape": [nr, nc], "maximize": bool, "seed": int,
"kinds": [...]}: one batch with one problem per entry of `kinds`. `run_batch`
runs a spec on the device (also from tests/batch_worker.py, for the runs under
LPG_ASSIGN_TIER / LPG_ASSIGN_FORM, which a batch reads when it is created).
"""
from __future__ import annotations

import functools
import itertools
import json
import os
import subprocess
import sys

import numpy as np

OPTIMAL, INFEASIBLE = 1, 3
INF = float("inf")

# one problem of each kind: small-range integers (many optima, many equal
# minv), wider integers, 30% forbidden pairs, identical rows, a constant
# matrix, tenths (inexact sums: roundings, slightly negative and -0 reduced costs)
KINDS = ("int3", "int49", "inf30", "rows", "const", "frac", "int3")


def sensed(C, maximize):
    """The matrix the algorithm runs on: finite costs negated for a maximisation, +inf kept."""
    C = np.asarray(C, dtype=np.float64)
    return np.where(np.isinf(C), C, -C) if maximize else C.copy()


def hungarian(C, maximize=False, trace=None):
    """include/lpg.h "assignment", steps 1-4. Returns a dict of status, col [nr]
    int64, u [nr], v [nc], objective, steps. `trace`, a list, receives per step
    (columns at the minimum, delta)."""
    C = np.asarray(C, dtype=np.float64)
    nr, nc = C.shape
    D = sensed(C, maximize)
    u, v = np.zeros(nr), np.zeros(nc)
    rowof = np.full(nc, -1, dtype=np.int64)
    steps, status = 0, OPTIMAL
    for i in range(nr):
        minv = np.full(nc, INF)
        way = np.full(nc, -1, dtype=np.int64)
        used = np.zeros(nc, dtype=bool)
        i0, j0 = i, -1
        while True:
            steps += 1
            if j0 >= 0:
                used[j0] = True
            free = ~used
            cur = (D[i0] - u[i0]) - v                      # two roundings, in this order
            take = free & (cur < minv)
            minv = np.where(take, cur, minv)
            way = np.where(take, j0, way)
            idx = np.flatnonzero(free & (minv < INF))
            if idx.size == 0:
                status = INFEASIBLE
                break
            j1 = int(idx[np.argmin(minv[idx])])            # `<`, -0 == +0, ties to the smallest j
            delta = minv[j1]                               # the bits as they stand
            if trace is not None:
                trace.append((int(np.count_nonzero(minv[idx] == delta)), float(delta)))
            u[i] = u[i] + delta
            uj = np.flatnonzero(used)
            u[rowof[uj]] = u[rowof[uj]] + delta            # the rows of used columns are distinct
            v[uj] = v[uj] - delta
            minv[free] = minv[free] - delta
            j0 = j1
            if rowof[j0] < 0:
                break
            i0 = int(rowof[j0])
        if status != OPTIMAL:
            break
        while j0 >= 0:
            jn = int(way[j0])
            rowof[j0] = rowof[jn] if jn >= 0 else i
            j0 = jn
    col = np.full(nr, -1, dtype=np.int64)
    objective = float("nan")
    if status == OPTIMAL:
        for j in range(nc):
            if rowof[j] >= 0:
                col[rowof[j]] = j
        objective = 0.0
        for i in range(nr):
            objective = objective + C[i, col[i]]
    if maximize:
        u, v = -u, -v
    return {"status": status, "col": col, "u": u, "v": v, "objective": objective, "steps": steps}


def brute_force(C, maximize=False):
    """(best objective or None, number of optimal injections) over every injection rows -> columns
    with finite costs; exact on integer costs."""
    C = np.asarray(C, dtype=np.float64)
    nr, nc = C.shape
    best, n = None, 0
    rows = np.arange(nr)
    for p in itertools.permutations(range(nc), nr):
        s = C[rows, list(p)].sum()
        if not np.isfinite(s):
            continue
        if best is None or (s > best if maximize else s < best):
            best, n = s, 1
        elif s == best:
            n += 1
    return best, n


def problem(kind, nr, nc, rng):
    if kind == "int3":
        return rng.integers(0, 4, size=(nr, nc)).astype(np.float64)
    if kind == "int49":
        return rng.integers(0, 50, size=(nr, nc)).astype(np.float64)
    if kind == "inf30":
        C = rng.integers(0, 50, size=(nr, nc)).astype(np.float64)
        C[rng.random((nr, nc)) < 0.3] = INF
        return C
    if kind == "rows":
        return np.tile(rng.integers(0, 50, size=(1, nc)).astype(np.float64), (nr, 1))
    if kind == "const":
        return np.full((nr, nc), float(rng.integers(0, 50)))
    if kind == "frac":
        return rng.integers(0, 50, size=(nr, nc)).astype(np.float64) / 10.0
    if kind == "blocked":                                  # a row with no allowed column: infeasible for sure
        C = rng.integers(0, 50, size=(nr, nc)).astype(np.float64)
        C[nr // 2, :] = INF
        return C
    raise ValueError(kind)


def spec(nr, nc, maximize=False, seed=0, kinds=KINDS):
    return {"shape": [nr, nc], "maximize": bool(maximize), "seed": int(seed), "kinds": list(kinds)}


def costs_of(s):
    """[count, nr, nc] of spec s."""
    nr, nc = s["shape"]
    rng = np.random.default_rng([20220518, nr, nc, int(s["maximize"]), s["seed"]])
    return np.stack([problem(k, nr, nc, rng) for k in s["kinds"]])


@functools.lru_cache(maxsize=None)
def _reference(key):
    s = json.loads(key)
    return [hungarian(C, s["maximize"]) for C in costs_of(s)]


def reference(s):
    """hungarian() of every problem of spec s, computed once per process."""
    return _reference(json.dumps(s, sort_keys=True))


def stacked(refs):
    """A list of hungarian() results as the arrays run_batch returns."""
    return {"status": np.array([r["status"] for r in refs], dtype=np.int64),
            "steps": np.array([r["steps"] for r in refs], dtype=np.int64),
            "objective": np.array([r["objective"] for r in refs]),
            "col": np.stack([r["col"] for r in refs]),
            "u": np.stack([r["u"] for r in refs]),
            "v": np.stack([r["v"] for r in refs])}


def run_costs(C, maximize=False):
    """A batch of the matrices C [count, nr, nc] on the device: the arrays of `stacked`, and tier, form."""
    import linearprogramming_amd as lpg
    C = np.asarray(C, dtype=np.float64)
    with lpg.AssignmentBatch(C.shape[0], C.shape[1], C.shape[2], maximize=maximize) as a:
        a.load(C)
        res = a.solve()
        col, u, v = a.get()
        info = a.info
        return {"status": np.array([r.status for r in res], dtype=np.int64),
                "steps": np.array([r.steps for r in res], dtype=np.int64),
                "objective": np.array([r.objective for r in res]),
                "col": col, "u": u, "v": v,
                "tier": np.int64(info.tier), "form": np.int64(info.form)}


def run_batch(s):
    return run_costs(costs_of(s), s["maximize"])


FIELDS = ("status", "steps", "col", "objective", "u", "v")


def assert_same(got, want, what=""):
    """Bit for bit: integers equal, doubles compared as their 64-bit patterns (so -0 != +0 and NaN == NaN)."""
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
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
    r = subprocess.run([sys.executable, os.path.join(here, "batch_worker.py"), "assign_cases", sp, op], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(op)
    return [{k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(f"{i}/")} for i in range(len(specs))]


# ---- the batches tests/test_gpu_assign.py runs ------------------------------
# 7 problems: the wave form's last workgroup has an idle wave
SMALL = [spec(nr, nc, mx) for (nr, nc) in ((1, 1), (2, 2), (5, 7)) for mx in (False, True)]
# 9 problems of 6 x 6, mixed: waves of one workgroup end at very different step counts
MIXED = [spec(6, 6, mx, kinds=("blocked", "const", "int3", "int49", "inf30", "frac", "rows", "int3", "inf30"))
         for mx in (False, True)]
WAVE_LINE = [spec(nr, nc, mx) for (nr, nc) in ((63, 63), (64, 64), (64, 70), (65, 65)) for mx in (False, True)]
STATE_LINE = [spec(200, nc, mx) for nc in (256, 257) for mx in (False, True)]
TIER_LINE = [spec(n, n, mx) for n in (138, 139) for mx in (False, True)]
FORCED_GLOBAL = [spec(9, 12), spec(70, 70, True)]
# the column state of a global-tier problem in LDS, and beyond it in device memory (28 bytes a column)
STATE_SPILL = [spec(3, 5400, kinds=("int3", "inf30", "frac")), spec(3, 5500, True, kinds=("int3", "inf30", "frac"))]
