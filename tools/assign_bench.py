#!/usr/bin/env python3
"""Batches of assignment problems on the MI355X: lpg_assign_solve against the
routes a caller had without it.

    python tools/assign_bench.py [--out FILE.jsonl] [--repeats 5] [--shapes 8x8x4096,...]

Per shape (integer costs 0..99 from lpg_assign_generate, restated here in numpy
so that the other legs see the same matrices):
  a  lpg_assign_solve: the call (host clock around it; it ends in a device
     synchronise and the copy of the results) and the kernel alone (device
     events around the launch, lpg_assign_info.kernel_ms)
  b  the same problems as assignment LPs (nr + nc equality rows, nr * nc
     columns, nr + nc artificials) through BatchEngine.solve_two_phase, where
     that tableau is within LPG_BATCH_MAX_DIM; on the first problems of the
     batch only where the host-side tableaus of all of them would pass 1 GiB
     (the count is reported and the time is per problem)
  c  scipy.optimize.linear_sum_assignment in a loop on the CPU (left out
     where scipy does not import)
  d  the workgroup form (LPG_ASSIGN_FORM=workgroup) where the wave form is
     the default (nc <= 64)
The legs are first checked against each other on every result (a against d
bit for bit; the objectives of b and c against a's, exact on integer costs),
then warmed up and timed in `repeats` alternating rounds; the figures are
median, min and max. One JSON line per shape.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import linearprogramming_amd as lpg  # noqa: E402

SEED, RANGE = 20220518, 100
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def generated(count, nr, nc, seed=SEED, rng=RANGE):
    """lpg_assign_generate's matrices: floor(uniform01(seed + q, i * nc + j) * range)."""
    with np.errstate(over="ignore"):
        idx = np.arange(nr * nc, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        key = np.uint64(seed) + np.arange(count, dtype=np.uint64)
        bits = splitmix64(key[:, None] ^ idx[None, :])
    u = (bits >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.floor(u * float(rng)).reshape(count, nr, nc)


def stats(ts):
    return {"median_ms": round(1e3 * statistics.median(ts), 4), "min_ms": round(1e3 * min(ts), 4),
            "max_ms": round(1e3 * max(ts), 4)}


class AssignLeg:
    def __init__(self, count, nr, nc, form=None):
        old = os.environ.pop("LPG_ASSIGN_FORM", None)
        if form:
            os.environ["LPG_ASSIGN_FORM"] = form          # read by lpg_assign_create
        try:
            self.a = lpg.AssignmentBatch(count, nr, nc)
        finally:
            os.environ.pop("LPG_ASSIGN_FORM", None)
            if old is not None:
                os.environ["LPG_ASSIGN_FORM"] = old
        self.a.generate(SEED, RANGE)
        self.kernel = []

    def run(self):
        t0 = time.perf_counter()
        res = self.a.solve()
        dt = time.perf_counter() - t0
        self.kernel.append(1e-3 * self.a.info.kernel_ms)
        return dt, res

    def results(self):
        _, res = self.run()
        col, u, v = self.a.get()
        return res, col, u, v


class LpLeg:
    """The first `count` problems as LPs in one BatchEngine; reloaded before every timed solve."""

    def __init__(self, C):
        count, nr, nc = C.shape
        self.m, nx = nr + nc, nr * nc
        self.ncols = 1 + nx + self.m
        T = np.zeros((count, self.m + 1, self.ncols))
        T[:, :self.m, 0] = 1.0
        for i in range(nr):
            T[:, i, 1 + i * nc:1 + (i + 1) * nc] = 1.0
            T[:, nr + np.arange(nc), 1 + i * nc + np.arange(nc)] = 1.0
        T[:, np.arange(self.m), 1 + nx + np.arange(self.m)] = 1.0
        self.T = T
        self.basis = np.tile(np.arange(1 + nx, 1 + nx + self.m, dtype=np.int64), (count, 1))
        self.cost = np.zeros((count, self.ncols - 1))
        self.cost[:, :nx] = -C.reshape(count, nx)          # the engine maximises
        self.art = 1 + nx
        self.e = lpg.BatchEngine(count, self.m, self.ncols, flags=0x1)   # LPG_FLAG_NO_LOG

    def run(self):
        self.e.load(self.T, self.basis)
        t0 = time.perf_counter()
        res = self.e.solve_two_phase(self.art, self.cost)
        return time.perf_counter() - t0, res


def scipy_leg(C):
    try:
        from scipy.optimize import linear_sum_assignment
    except Exception:
        return None

    def run():
        t0 = time.perf_counter()
        obj = [C[q][linear_sum_assignment(C[q])].sum() for q in range(C.shape[0])]
        return time.perf_counter() - t0, obj
    return run


def bench_shape(nr, nc, count, repeats):
    C = generated(count, nr, nc)
    a = AssignLeg(count, nr, nc)
    info = a.a.info
    res, col, u, v = a.results()
    obj = np.array([r.objective for r in res])
    line = {"nr": nr, "nc": nc, "batch": count, "tier": "lds" if info.tier == 0 else "global",
            "form": "wave" if info.form == 0 else "workgroup", "lds_bytes": int(info.lds_bytes),
            "steps": int(sum(r.steps for r in res)), "optimal": int(sum(r.status == lpg.OPTIMAL for r in res))}
    assert line["optimal"] == count
    assert (C[np.arange(count)[:, None], np.arange(nr)[None, :], col].sum(axis=1) == obj).all(), "generator restatement"
    legs = {"a": a.run}
    d = None
    if info.form == 0:
        d = AssignLeg(count, nr, nc, "workgroup")
        assert d.a.info.form == 1
        rd, cd, ud, vd = d.results()
        assert [(r.status, r.steps, r.objective) for r in rd] == [(r.status, r.steps, r.objective) for r in res]
        assert (cd == col).all() and (ud.view(np.uint64) == u.view(np.uint64)).all() and \
            (vd.view(np.uint64) == v.view(np.uint64)).all(), "wave and workgroup forms differ"
        legs["d"] = d.run
    b = None
    if 1 + nr * nc + nr + nc <= 8192:
        per = 8 * (nr + nc + 1) * (1 + nr * nc + nr + nc)
        nb = max(1, min(count, (1 << 30) // per))
        b = LpLeg(C[:nb])
        _, rb = b.run()
        assert all(r.status == lpg.OPTIMAL for r in rb), "an assignment LP did not end OPTIMAL"
        assert (np.array([-r.objective for r in rb]) == obj[:nb]).all(), "the LP route's objective differs"
        line["b_problems"], line["b_pivots"], line["b_tier"] = nb, int(sum(r.pivots for r in rb)), \
            "lds" if b.e.info.tier == 0 else "global"
        legs["b"] = b.run
    c = scipy_leg(C)
    if c is not None:
        _, oc = c()
        assert (np.array(oc) == obj).all(), "scipy's objective differs"
        legs["c"] = c
    for run in legs.values():                               # warm-up
        run()
    a.kernel.clear()
    if d:
        d.kernel.clear()
    times = {k: [] for k in legs}
    for _ in range(repeats):                                # alternating
        for k, run in legs.items():
            times[k].append(run()[0])
    line["a_call"] = stats(times["a"])
    line["a_kernel"] = stats(a.kernel)
    if d:
        line["d_call"], line["d_kernel"] = stats(times["d"]), stats(d.kernel)
        line["wave_over_workgroup_kernel"] = round(statistics.median(a.kernel) / statistics.median(d.kernel), 3)
    if b:
        line["b_call"] = stats(times["b"])
        per_a = statistics.median(times["a"]) / count
        per_b = statistics.median(times["b"]) / line["b_problems"]
        line["b_over_a_per_problem"] = round(per_b / per_a, 1)
    if c is not None:
        line["c_call"] = stats(times["c"])
        line["c_over_a"] = round(statistics.median(times["c"]) / statistics.median(times["a"]), 1)
    line["a_us_per_problem"] = round(1e6 * statistics.median(times["a"]) / count, 3)
    a.a.close()
    if d:
        d.a.close()
    if b:
        b.e.close()
    return line


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="8x8x4096,32x32x4096,64x64x1024,128x128x1024,256x256x256")
    args = ap.parse_args(argv)
    out = open(args.out, "w") if args.out else None
    for spec in args.shapes.split(","):
        nr, nc, count = (int(x) for x in spec.split("x"))
        line = json.dumps(bench_shape(nr, nc, count, args.repeats))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
