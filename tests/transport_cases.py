"""The transportation problem as include/lpg.h ("transportation") states it,
restated in numpy operation for operation, and the cases the transportation
tests share.

`Statement` is the definition: a start (northwest corner or least cost), then
potentials / pricing / closed loop until no reduced cost is negative or the
call's budget is used up. All data are integers held in fp64, so every
operation is exact and the device is held to it bit for bit
(tests/test_gpu_transport.py); the definition itself is held to HiGHS and to
its own certificate (tests/test_transport_cases.py).

A spec is a JSON-able dict {"shape": [nr, nc], "maximize", "start", "rule",
"seed", "kinds", "budgets"}: one batch with one problem per entry of `kinds`,
solved by one call per entry of `budgets` (None: one call of 50 (nr + nc)).
`run_batch` runs a spec on the device (also from tests/batch_worker.py, for the
runs under LPG_TRANSPORT_FORM / _TIER / _CHUNK, which a batch reads when it is
created).
"""
from __future__ import annotations

import functools
import json
import os
import subprocess
import sys

import numpy as np

RUNNING, OPTIMAL, ITER_LIMIT = 0, 1, 4
DANTZIG, BLAND = 0, 1
LEAST_COST, NORTHWEST = "least_cost", "northwest"


def internal_costs(C, maximize):
    """The matrix the method runs on: 0.0 - c for a maximisation, c + 0.0 otherwise (no -0.0 inside)."""
    C = np.asarray(C, dtype=np.float64)
    return 0.0 - C if maximize else C + 0.0


def start_northwest(s, d):
    nr, nc = len(s), len(d)
    i = j = 0
    rs, rd = s[0], d[0]
    cells, flows = [], []
    for k in range(nr + nc - 1):
        x = min(rs, rd)
        cells.append(i * nc + j)
        flows.append(x)
        rs, rd = rs - x, rd - x
        if k == nr + nc - 2:
            break
        if rs == 0 and i < nr - 1:
            i += 1
            rs = s[i]
        else:
            j += 1
            rd = d[j]
    return cells, flows


def start_least_cost(D, s, d):
    nr, nc = D.shape
    rs, rd = np.array(s, dtype=np.float64), np.array(d, dtype=np.float64)
    ro, co = np.ones(nr, dtype=bool), np.ones(nc, dtype=bool)
    cells, flows = [], []
    for k in range(nr + nc - 1):
        masked = np.where(ro[:, None] & co[None, :], D, np.inf).ravel()
        e = int(np.argmin(masked))                         # the smallest cost, ties to the smallest cell index
        i, j = divmod(e, nc)
        x = min(rs[i], rd[j])
        cells.append(e)
        flows.append(x)
        rs[i], rd[j] = rs[i] - x, rd[j] - x
        if k == nr + nc - 2:
            break
        if rs[i] == 0 and (rd[j] != 0 or ro.sum() > 1):
            ro[i] = False
        else:
            co[j] = False
    return cells, flows


class Statement:
    """One problem's state: the cell list in slot order, the flows, iterations, status."""

    def __init__(self, C, s, d, maximize=False, start=LEAST_COST):
        self.C = np.asarray(C, dtype=np.float64)
        self.nr, self.nc = self.C.shape
        self.maximize = bool(maximize)
        self.D = internal_costs(self.C, maximize)
        s, d = np.asarray(s, dtype=np.float64), np.asarray(d, dtype=np.float64)
        cells, flows = start_northwest(s, d) if start == NORTHWEST else start_least_cost(self.D, s, d)
        self.cells = np.array(cells, dtype=np.int64)
        self.flows = np.array(flows, dtype=np.float64)
        self.iterations, self.status = 0, RUNNING
        self.max_depth = 0

    def potentials(self):
        """pot [nr + nc] (rows, then columns), pred (the slot of the tree cell towards row 0), depth."""
        nr, nc = self.nr, self.nc
        nn = nr + nc
        ci, cj = self.cells // nc, self.cells % nc + nr
        cost = self.D.ravel()[self.cells]
        pot = np.zeros(nn)
        pred = np.full(nn, -1, dtype=np.int64)
        depth = np.full(nn, -1, dtype=np.int64)
        known = np.zeros(nn, dtype=bool)
        known[0], depth[0] = True, 0
        level = 1
        while not known.all():
            kr, kc = known[ci], known[cj]
            f = np.flatnonzero(kr ^ kc)
            assert f.size, "the basis is not a spanning tree"
            src, dst = np.where(kr[f], ci[f], cj[f]), np.where(kr[f], cj[f], ci[f])
            pot[dst] = cost[f] - pot[src]
            pred[dst], depth[dst], known[dst] = f, level, True
            level += 1
        return pot, pred, depth

    def solve(self, max_iters, rule=DANTZIG, trace=None):
        """One call: at most max_iters iterations. `trace`, a list, receives per iteration
        (cells at the smallest delta, minus cells at theta, theta)."""
        assert max_iters >= 1
        if self.status == OPTIMAL:
            return self
        nr, nc = self.nr, self.nc
        done = 0
        while True:
            pot, pred, depth = self.potentials()
            self.max_depth = max(self.max_depth, int(depth.max()))
            delta = (self.D - pot[:nr, None]) - pot[None, nr:]
            flat = delta.ravel()
            neg = np.flatnonzero(flat < 0)
            if neg.size == 0:
                self.status = OPTIMAL
                break
            if done == max_iters:
                self.status = ITER_LIMIT
                break
            e = int(neg[0]) if rule == BLAND else int(np.argmin(flat))
            a, b = nr + e % nc, e // nc                    # from the column of the entering cell to its row
            minus, plus, ka, kb = [], [], 0, 0
            while a != b:
                if depth[a] >= depth[b]:
                    slot = int(pred[a])
                    (minus if ka % 2 == 0 else plus).append(slot)
                    ka += 1
                    ce = int(self.cells[slot])
                    a = nr + ce % nc if a < nr else ce // nc
                else:
                    slot = int(pred[b])
                    (minus if kb % 2 == 0 else plus).append(slot)
                    kb += 1
                    ce = int(self.cells[slot])
                    b = nr + ce % nc if b < nr else ce // nc
            theta = self.flows[minus].min()
            at = [m for m in minus if self.flows[m] == theta]
            leave = min(at, key=lambda m: self.cells[m])
            if trace is not None:
                trace.append((int(np.count_nonzero(flat == flat.min())), len(at), float(theta)))
            self.flows[minus] -= theta
            self.flows[plus] += theta
            self.cells[leave], self.flows[leave] = e, theta
            self.iterations += 1
            done += 1
        return self

    def result(self):
        nr, nc = self.nr, self.nc
        pot, _, _ = self.potentials()
        x = np.zeros(nr * nc)
        x[self.cells] = self.flows
        objective = float((self.D.ravel()[self.cells] * self.flows).sum())      # exact integers: any order
        u, v = pot[:nr], pot[nr:]
        if self.maximize:
            u, v, objective = 0.0 - u, 0.0 - v, 0.0 - objective
        return {"status": self.status, "iterations": self.iterations, "objective": objective,
                "x": x.reshape(nr, nc), "u": u, "v": v, "basis": np.sort(self.cells)}


def default_budget(nr, nc):
    return 50 * (nr + nc)


def solve(C, s, d, maximize=False, start=LEAST_COST, rule=DANTZIG, budgets=None, trace=None):
    st = Statement(C, s, d, maximize, start)
    trace = [] if trace is None else trace
    zero_at_start = int(np.count_nonzero(st.flows == 0))
    for b in budgets or [default_budget(*np.asarray(C).shape)]:
        st.solve(b, rule, trace)
    r = st.result()
    r["max_depth"] = st.max_depth
    # what the problem holds (tests/test_transport_cases.py, the census)
    r["census"] = {"entering_ties": sum(t[0] >= 2 for t in trace), "leaving_ties": sum(t[1] >= 2 for t in trace),
                   "degenerate_steps": sum(t[2] == 0 for t in trace), "zero_basic_at_start": zero_at_start,
                   "zero_basic_at_end": int(np.count_nonzero(st.flows == 0)), "optimal_at_start": int(st.iterations == 0),
                   "zero_amounts": int(np.count_nonzero(np.asarray(s) == 0) + np.count_nonzero(np.asarray(d) == 0))}
    return r


# ---- case builders ------------------------------------------------------------
KINDS = ("c2", "c99", "zeros", "const", "c2", "big", "c99")


def balanced(s, d):
    """The side with the smaller sum gets the difference added to its last entry."""
    s, d = s.astype(np.float64), d.astype(np.float64)
    diff = s.sum() - d.sum()
    if diff > 0:
        d[-1] += diff
    else:
        s[-1] -= diff
    return s, d


def problem(kind, nr, nc, rng):
    """(C, s, d) of one kind: c2 costs 0..2 (ties everywhere), c99 costs 0..99, zeros with zero supplies and
    demands, const a constant matrix (optimal at the start), big quantities up to 1000, unit supply = demand = 1."""
    if kind == "unit":
        assert nr == nc
        return rng.integers(0, 100, size=(nr, nc)).astype(np.float64), np.ones(nr), np.ones(nc)
    if kind == "unit2":
        assert nr == nc
        return rng.integers(0, 3, size=(nr, nc)).astype(np.float64), np.ones(nr), np.ones(nc)
    hi = {"c2": 3, "c99": 100, "zeros": 10, "const": 1, "big": 100}[kind]
    C = rng.integers(0, hi, size=(nr, nc)).astype(np.float64)
    if kind == "const":
        C += float(rng.integers(0, 50))
    q = 1000 if kind == "big" else 9
    s, d = rng.integers(1, q + 1, size=nr), rng.integers(1, q + 1, size=nc)
    if kind == "zeros":
        s[rng.random(nr) < 0.4] = 0
        d[rng.random(nc) < 0.4] = 0
    return (C,) + balanced(s, d)


def spec(nr, nc, maximize=False, start=LEAST_COST, rule=DANTZIG, seed=0, kinds=KINDS, budgets=None):
    return {"shape": [nr, nc], "maximize": bool(maximize), "start": start, "rule": int(rule), "seed": int(seed),
            "kinds": list(kinds), "budgets": budgets}


def data_of(s):
    """(C [count, nr, nc], supply [count, nr], demand [count, nc]) of spec s."""
    nr, nc = s["shape"]
    rng = np.random.default_rng([20220518, nr, nc, int(s["maximize"]), s["seed"]])
    ps = [problem(k, nr, nc, rng) for k in s["kinds"]]
    return tuple(np.stack([p[k] for p in ps]) for k in range(3))


@functools.lru_cache(maxsize=None)
def _reference(key):
    s = json.loads(key)
    C, S, D = data_of(s)
    return [solve(C[q], S[q], D[q], s["maximize"], s["start"], s["rule"], s["budgets"]) for q in range(C.shape[0])]


def reference(s):
    """The statement's result for every problem of spec s, computed once per process."""
    return _reference(json.dumps(s, sort_keys=True))


FIELDS = ("status", "iterations", "objective", "x", "u", "v", "basis")


def stacked(refs):
    """A list of results as the arrays run_batch returns."""
    return {f: (np.array([r[f] for r in refs], dtype=np.float64 if f == "objective" else np.int64)
                if f in ("status", "iterations", "objective") else np.stack([r[f] for r in refs])) for f in FIELDS}


def run_data(C, S, D, maximize=False, start=LEAST_COST, rule=DANTZIG, budgets=None):
    """A batch on the device: the arrays of `stacked`, and tier, form, chunk, launches."""
    import linearprogramming_amd as lpg
    C = np.asarray(C, dtype=np.float64)
    with lpg.TransportBatch(C.shape[0], C.shape[1], C.shape[2], maximize=maximize, start=start) as t:
        t.load(C, S, D)
        for b in budgets or [None]:
            res = t.solve(b, rule)
        x, u, v, basis = t.get()
        info = t.info
        return {"status": np.array([r.status for r in res], dtype=np.int64),
                "iterations": np.array([r.iterations for r in res], dtype=np.int64),
                "objective": np.array([r.objective for r in res]),
                "x": x, "u": u, "v": v, "basis": basis,
                "tier": np.int64(info.tier), "form": np.int64(info.form), "chunk": np.int64(info.chunk),
                "launches": np.int64(info.launches)}


def run_batch(s):
    return run_data(*data_of(s), s["maximize"], s["start"], s["rule"], s["budgets"])


def assert_same(got, want, what=""):
    """Bit for bit: integers equal, doubles compared as their 64-bit patterns."""
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
    r = subprocess.run([sys.executable, os.path.join(here, "batch_worker.py"), "transport_cases", sp, op], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(op)
    return [{k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(f"{i}/")} for i in range(len(specs))]


def name(s):
    return (f"{s['shape'][0]}x{s['shape'][1]}-{'max' if s['maximize'] else 'min'}-{s['start']}-"
            f"{'bland' if s['rule'] else 'dantzig'}" + (f"-b{'+'.join(map(str, s['budgets']))}" if s["budgets"] else ""))


# ---- the batches tests/test_gpu_transport.py runs -------------------------------
# 7 problems: the wave form's last workgroup has an idle wave; every rule, start and sense
SMALL = [spec(nr, nc, mx, st, rule) for (nr, nc, mx, st, rule) in (
    (1, 1, False, LEAST_COST, DANTZIG), (1, 5, False, NORTHWEST, DANTZIG), (5, 1, True, LEAST_COST, BLAND),
    (4, 5, False, LEAST_COST, DANTZIG), (4, 5, True, NORTHWEST, DANTZIG), (4, 5, False, NORTHWEST, BLAND),
    (4, 5, True, LEAST_COST, BLAND), (6, 7, False, NORTHWEST, DANTZIG), (6, 7, True, LEAST_COST, DANTZIG))]
# the node cap: everything is basic in 4095 x 1; two rows of 4094 columns
CAP = [spec(2, 4094, kinds=("c2", "c99", "zeros")), spec(4095, 1, kinds=("c2", "zeros")),
       spec(2, 4094, True, NORTHWEST, kinds=("c99",))]
# nr + nc = 63, 64, 65: the wave / workgroup line
FORM_LINE = [spec(nr, nc, mx, st, kinds=("c2", "c99", "zeros", "const", "big"))
             for (nr, nc) in ((31, 32), (32, 32), (30, 34), (32, 33)) for (mx, st) in ((False, LEAST_COST), (True, NORTHWEST))]
FORCED_WORKGROUP = [spec(31, 32), spec(32, 32, True, NORTHWEST), spec(4, 5, rule=BLAND), spec(1, 1)]
# nr * nc = 255, 256, 257, 1025: a thread's stride of the pricing sweep
STRIDE_LINE = [spec(nr, nc, kinds=("c2", "c99", "zeros")) for (nr, nc) in ((15, 17), (16, 16), (1, 257), (25, 41))] + \
              [spec(5, 51, True, NORTHWEST, kinds=("c2", "c99")), spec(16, 16, True, NORTHWEST, BLAND, kinds=("c2", "c99"))]
# the last shape whose C fits the LDS beside 32 bytes a node, and the first that does not
TIER_LINE = [spec(n, n, mx, kinds=("c2", "c99", "zeros")) for n in (134, 135) for mx in (False, True)]
FORCED_GLOBAL = [spec(9, 12), spec(40, 40, True, NORTHWEST, kinds=("c2", "c99", "zeros")), spec(134, 134, kinds=("c2",))]
# supply = demand = 1 squares: as degenerate as they come
UNIT = [spec(n, n, mx, st, kinds=("unit", "unit2", "unit")) for n in (8, 16, 32)
        for (mx, st) in ((False, LEAST_COST), (True, NORTHWEST))]
UNIT_BLAND = [spec(n, n, False, st, BLAND, kinds=("unit", "unit2")) for n in (8, 16) for st in (LEAST_COST, NORTHWEST)]
# problems of one batch that end after very different iteration counts, 0 among them
MIXED = [spec(9, 11, mx, NORTHWEST, kinds=("const", "c99", "c2", "zeros", "big", "const", "c99", "c2", "big"))
         for mx in (False, True)]
# a budget that cuts mid-solve, continued by later calls: the bits of one sufficient call
BUDGETS = [spec(12, 14, False, NORTHWEST, DANTZIG, budgets=[3, 1, 550]), spec(12, 14, True, LEAST_COST, BLAND, budgets=[2, 2, 1300]),
           spec(40, 50, False, NORTHWEST, DANTZIG, kinds=("c2", "c99", "zeros"), budgets=[5, 4500])]
CUT = [spec(12, 14, False, NORTHWEST, DANTZIG, budgets=[3]), spec(40, 50, False, NORTHWEST, kinds=("c2", "c99"), budgets=[5, 2])]
CHUNKED = [spec(12, 14, False, NORTHWEST), spec(6, 7, True, LEAST_COST, BLAND), spec(40, 50, kinds=("c2", "c99"))]

DEVICE_CASES = SMALL + CAP + FORM_LINE + FORCED_WORKGROUP + STRIDE_LINE + TIER_LINE + FORCED_GLOBAL + UNIT + UNIT_BLAND + \
    MIXED + BUDGETS + CHUNKED
