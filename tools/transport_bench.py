#!/usr/bin/env python3
"""Batches of transportation problems on the MI355X: lpg_transport_solve
against the routes a caller had without it.

    python tools/transport_bench.py [--out FILE.jsonl] [--repeats 5] [--shapes 4x5x4096,...]
    python tools/transport_bench.py --chunks 8,32,128,512,100000 --shapes 16x16x4096,64x64x1024

Per shape (lpg_transport_generate's problems, costs 0..99 and amounts 1..9,
restated here in numpy so that the other legs see the same data):
  a  TransportBatch.solve from the least-cost start: the call (host clock
     around it; it ends in a device synchronise and the copy of the results)
     and the kernels alone (device events around every launch, summed:
     lpg_transport_info.kernel_ms). The problems are generated again before
     every solve, outside the clock, because a solved batch has nothing to do.
  b  the same problems as LPs (nr + nc equality rows, nr * nc columns, nr + nc
     artificials) through BatchEngine.solve_two_phase, where that tableau is
     within LPG_BATCH_MAX_DIM; on the first problems of the batch only where
     the host-side tableaus of all of them would pass 1 GiB (the count is
     reported and the time is per problem)
  c  scipy.optimize.linprog (HiGHS) in a loop on the CPU, the first 128 models
     (left out where scipy does not import; timed three times only where one
     pass takes more than three seconds)
  d  the workgroup form (LPG_TRANSPORT_FORM=workgroup) where the wave form is
     the default (nr + nc <= 64)
  n  the northwest-corner start
The legs are first checked against each other on every result (a against d bit
for bit; the objectives of b, c and n against a's, exact on integer data), then
warmed up and timed in `repeats` alternating rounds; the figures are median,
min and max. One JSON line per shape. With --chunks: leg a only, once per
LPG_TRANSPORT_CHUNK value, alternating, one JSON line per shape.
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

SEED, RANGE, QMAX = 20220518, 100, 9


def splitmix64(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def generated(count, nr, nc, seed=SEED, rng=RANGE, qmax=QMAX):
    """lpg_transport_generate's problems (include/lpg.h, "Generator"): C, supply, demand."""
    n = nr * nc + nr + nc
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        key = np.uint64(seed) + np.arange(count, dtype=np.uint64)
        bits = splitmix64(key[:, None] ^ idx[None, :])
    u = (bits >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    C = np.floor(u[:, :nr * nc] * float(rng)).reshape(count, nr, nc)
    S = 1.0 + np.floor(u[:, nr * nc:nr * nc + nr] * float(qmax))
    D = 1.0 + np.floor(u[:, nr * nc + nr:] * float(qmax))
    diff = S.sum(axis=1) - D.sum(axis=1)
    D[:, -1] += np.maximum(diff, 0.0)
    S[:, -1] += np.maximum(-diff, 0.0)
    return C, S, D


def stats(ts):
    return {"median_ms": round(1e3 * statistics.median(ts), 4), "min_ms": round(1e3 * min(ts), 4),
            "max_ms": round(1e3 * max(ts), 4)}


class TransportLeg:
    def __init__(self, count, nr, nc, start="least_cost", env=None):
        env = env or {}
        old = {k: os.environ.pop(k, None) for k in ("LPG_TRANSPORT_FORM", "LPG_TRANSPORT_CHUNK", "LPG_TRANSPORT_TIER")}
        os.environ.update(env)                            # read by lpg_transport_create
        try:
            self.t = lpg.TransportBatch(count, nr, nc, start=start)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        self.kernel, self.launches = [], 0

    def run(self):
        self.t.generate(SEED, RANGE, QMAX)
        t0 = time.perf_counter()
        res = self.t.solve()
        dt = time.perf_counter() - t0
        info = self.t.info
        self.kernel.append(1e-3 * info.kernel_ms)
        self.launches = int(info.launches)
        return dt, res

    def results(self):
        _, res = self.run()
        return (res,) + self.t.get()


class LpLeg:
    """The first `count` problems as LPs in one BatchEngine; reloaded before every timed solve."""

    def __init__(self, C, S, D):
        count, nr, nc = C.shape
        self.m, nx = nr + nc, nr * nc
        self.ncols = 1 + nx + self.m
        T = np.zeros((count, self.m + 1, self.ncols))
        T[:, :nr, 0], T[:, nr:self.m, 0] = S, D
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


def scipy_leg(C, S, D):
    try:
        from scipy.optimize import linprog
        from scipy.sparse import csr_matrix
    except Exception:
        return None
    count, nr, nc = C.shape
    rows = np.concatenate([np.repeat(np.arange(nr), nc), nr + np.tile(np.arange(nc), nr)])
    cols = np.concatenate([np.arange(nr * nc), np.arange(nr * nc)])
    A = csr_matrix((np.ones(2 * nr * nc), (rows, cols)), shape=(nr + nc, nr * nc))

    def run():
        t0 = time.perf_counter()
        obj = [linprog(C[q].ravel(), A_eq=A, b_eq=np.concatenate([S[q], D[q]]), method="highs").fun for q in range(count)]
        return time.perf_counter() - t0, obj
    return run


def same_bits(x, y):
    return all((np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)).all()
               if a.dtype == np.float64 else (a == b).all() for a, b in zip(x, y))


def bench_shape(nr, nc, count, repeats):
    C, S, D = generated(count, nr, nc)
    a = TransportLeg(count, nr, nc)
    info = a.t.info
    res, x, u, v, basis = a.results()
    obj = np.array([r.objective for r in res])
    line = {"nr": nr, "nc": nc, "batch": count, "tier": "lds" if info.tier == 0 else "global",
            "form": "wave" if info.form == 0 else "workgroup", "lds_bytes": int(info.lds_bytes), "chunk": int(info.chunk),
            "launches": a.launches, "iterations": int(sum(r.iterations for r in res)),
            "max_iterations": int(max(r.iterations for r in res)), "optimal": int(sum(r.status == lpg.OPTIMAL for r in res))}
    assert line["optimal"] == count
    assert ((C * x).sum(axis=(1, 2)) == obj).all() and (x.sum(axis=2) == S).all() and (x.sum(axis=1) == D).all(), \
        "generator restatement"
    legs = {"a": a.run}
    d = None
    if info.form == 0:
        d = TransportLeg(count, nr, nc, env={"LPG_TRANSPORT_FORM": "workgroup"})
        assert d.t.info.form == 1
        rd, xd, ud, vd, bd = d.results()
        assert [(r.status, r.iterations, r.objective) for r in rd] == [(r.status, r.iterations, r.objective) for r in res]
        assert same_bits((xd, ud, vd, bd), (x, u, v, basis)), "wave and workgroup forms differ"
        legs["d"] = d.run
    n = TransportLeg(count, nr, nc, start="northwest")
    rn = n.results()[0]
    assert all(r.status == lpg.OPTIMAL for r in rn) and (np.array([r.objective for r in rn]) == obj).all(), \
        "the northwest start's objective differs"
    line["n_iterations"] = int(sum(r.iterations for r in rn))
    legs["n"] = n.run
    b = None
    if 1 + nr * nc + nr + nc <= 8192:
        per = 8 * (nr + nc + 1) * (1 + nr * nc + nr + nc)
        nb = max(1, min(count, (1 << 30) // per))
        b = LpLeg(C[:nb], S[:nb], D[:nb])
        _, rb = b.run()
        assert all(r.status == lpg.OPTIMAL for r in rb), "a transportation LP did not end OPTIMAL"
        assert (np.array([-r.objective for r in rb]) == obj[:nb]).all(), "the LP route's objective differs"
        line["b_problems"], line["b_pivots"], line["b_tier"] = nb, int(sum(r.pivots for r in rb)), \
            "lds" if b.e.info.tier == 0 else "global"
        legs["b"] = b.run
    nc_models = min(count, 128)
    c = scipy_leg(C[:nc_models], S[:nc_models], D[:nc_models])
    c_first = None
    if c is not None:
        c_first, oc = c()
        assert np.allclose(np.array(oc), obj[:nc_models], rtol=1e-9, atol=1e-6), "HiGHS' objective differs"
        line["c_models"] = nc_models
        legs["c"] = c
    for run in legs.values():                               # warm-up
        run()
    for leg in (a, d, n):
        if leg:
            leg.kernel.clear()
    times = {k: [] for k in legs}
    for r in range(repeats):                                # alternating
        for k, run in legs.items():
            if k == "c" and c_first > 3.0 and r >= 3:
                continue
            times[k].append(run()[0])
    line["a_call"], line["a_kernel"] = stats(times["a"]), stats(a.kernel)
    line["n_call"], line["n_kernel"] = stats(times["n"]), stats(n.kernel)
    line["northwest_over_least_cost_call"] = round(statistics.median(times["n"]) / statistics.median(times["a"]), 3)
    if d:
        line["d_call"], line["d_kernel"] = stats(times["d"]), stats(d.kernel)
        line["wave_over_workgroup_kernel"] = round(statistics.median(a.kernel) / statistics.median(d.kernel), 3)
    per_a = statistics.median(times["a"]) / count
    if b:
        line["b_call"] = stats(times["b"])
        line["b_over_a_per_problem"] = round(statistics.median(times["b"]) / line["b_problems"] / per_a, 1)
    if c is not None:
        line["c_call"], line["c_repeats"] = stats(times["c"]), len(times["c"])
        line["c_over_a_per_problem"] = round(statistics.median(times["c"]) / nc_models / per_a, 1)
    line["a_us_per_problem"] = round(1e6 * per_a, 3)
    for leg in (a, d, n):
        if leg:
            leg.t.close()
    if b:
        b.e.close()
    return line


def sweep_shape(nr, nc, count, chunks, repeats):
    legs = {ch: TransportLeg(count, nr, nc, env={"LPG_TRANSPORT_CHUNK": str(ch)}) for ch in chunks}
    first = None
    for ch, leg in legs.items():
        assert leg.t.info.chunk == ch
        got = leg.results()
        key = [(r.status, r.iterations, r.objective) for r in got[0]]
        first = first or (key, got[1:])
        assert key == first[0] and same_bits(got[1:], first[1]), f"chunk {ch} differs"
        leg.kernel.clear()
    times = {ch: [] for ch in chunks}
    for _ in range(repeats):
        for ch, leg in legs.items():
            times[ch].append(leg.run()[0])
    line = {"sweep": "chunk", "nr": nr, "nc": nc, "batch": count, "max_iterations": max(k[1] for k in first[0]),
            "chunks": {str(ch): {"launches": legs[ch].launches, "call": stats(times[ch]), "kernel": stats(legs[ch].kernel)}
                       for ch in chunks}}
    for leg in legs.values():
        leg.t.close()
    return line


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="4x5x4096,8x8x4096,16x16x4096,32x32x1024,64x64x1024,128x128x256,8x8x64")
    ap.add_argument("--chunks", default=None, help="comma-separated LPG_TRANSPORT_CHUNK values: the chunk sweep")
    args = ap.parse_args(argv)
    out = open(args.out, "w") if args.out else None
    for spec in args.shapes.split(","):
        nr, nc, count = (int(x) for x in spec.split("x"))
        if args.chunks:
            rec = sweep_shape(nr, nc, count, [int(c) for c in args.chunks.split(",")], args.repeats)
        else:
            rec = bench_shape(nr, nc, count, args.repeats)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
