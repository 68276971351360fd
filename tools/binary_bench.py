#!/usr/bin/env python3
"""Batches of 0-1 programs on the MI355X: lpg_binary_solve against the routes a
caller had without it.

    python tools/binary_bench.py [--out FILE.jsonl] [--repeats 5] [--shapes 8x8x4096,...] [--sweep MxNxSEED]

Per shape M x N x count (the banded planted problems of lpg_binary_generate,
restated by tests/binary_cases.py so that the other legs see the same models):
  a  lpg_binary_solve on the whole batch: the call (host clock around it; it
     ends in a device synchronise and the copy of the records) and the kernels
     alone (device events around every launch, lpg_binary_info.kernel_ms)
  b  frontend.solve_ilp, one model at a time, the x_j <= 1 bounds as rows:
     what a caller had before. On the first few models whose text the front
     end takes (every cost non-zero, no empty row) and only up to --b-max-n
     columns (a tree level is a launch and a host round trip); left out, with
     the reason, where a model does not end OPTIMAL within the node limit
  c  scipy.optimize.milp in a loop on the CPU (left out where scipy has none)
  d  the numpy statement (tests/binary_cases.py enumerate01) on the CPU
The legs are first checked against each other (a against d bit for bit on
status, objective, x and nodes; the objectives of b and c against a's), then
warmed up and timed in `repeats` alternating rounds; the figures are median,
min and max, and per problem where a leg runs fewer problems than the batch.
Then a split sweep of one large problem: split 0..10, the call's time, the
nodes, and objective and x the same for every split. One JSON line per shape
and one for the sweep.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linearprogramming_amd as lpg  # noqa: E402
from linearprogramming_amd import frontend  # noqa: E402
import binary_cases as bc  # noqa: E402

SEED = 20220518
B_MODELS, C_MODELS, D_MODELS = 4, 128, 16


def stats(ts, per=1):
    return {"median_ms": round(1e3 * statistics.median(ts), 4), "min_ms": round(1e3 * min(ts), 4),
            "max_ms": round(1e3 * max(ts), 4), "problems": per}


def model_text(A, sense, rhs, c):
    """The model as the reference's text, every variable 0 <= x <= 1; None where the front end would not take it."""
    m, n = A.shape
    if (c == 0).any() or (np.count_nonzero(A, axis=1) == 0).any():
        return None
    def terms(v):
        return "".join(f"{int(a):+d}x{j + 1}" for j, a in enumerate(v) if a).lstrip("+")
    rows = [terms(A[i]) + {-1: "<=", 0: "=", 1: ">="}[int(sense[i])] + str(int(rhs[i])) for i in range(m)]
    rows += [f"x{j + 1}<=1" for j in range(n)] + [f"x{j + 1}>=0" for j in range(n)]
    return "OF {\n\tmin:z=%s\n}\nST {\n\t%s\n}\n" % (terms(c), ";\n\t".join(rows))


def ilp_leg(models):
    sms = []
    for mod in models:
        text = model_text(*mod)
        if text is not None:
            sms.append((frontend.build_smatrix(text), [f"x{j + 1}" for j in range(mod[0].shape[1])]))
        if len(sms) == B_MODELS:
            break

    def run():
        t0 = time.perf_counter()
        sols = [frontend.solve_ilp(sm, names, node_limit=20000) for sm, names in sms]
        return time.perf_counter() - t0, sols
    return run, len(sms)


def milp_leg(models):
    try:
        from scipy.optimize import Bounds, LinearConstraint, milp
    except Exception:
        return None
    cons = [(c, LinearConstraint(A, *bc.bounds(sense, rhs))) for A, sense, rhs, c in models]

    def run():
        t0 = time.perf_counter()
        res = [milp(c, constraints=k, integrality=np.ones(len(c)), bounds=Bounds(0, 1)) for c, k in cons]
        return time.perf_counter() - t0, res
    return run


def bench_shape(m, n, count, repeats, max_nodes=20000000, b_max_n=33):
    models = [bc.generate(m, n, SEED + q)[:4] for q in range(min(count, max(C_MODELS, 64)))]
    with lpg.BinaryBatch(count, m, n) as a:
        a.generate(SEED)
        kernel = []

        def run_a():
            a.generate(SEED)                                   # a load or generate resets the searches
            t0 = time.perf_counter()
            res = a.solve(max_nodes)                           # a cap, so that a runaway search fails the check below
            dt = time.perf_counter() - t0
            kernel.append(1e-3 * a.info.kernel_ms)
            return dt, res

        _, res = run_a()
        x = a.get()
        info = a.info
        line = {"m": m, "n": n, "batch": count, "tier": "lds" if info.tier == 0 else "global",
                "rows_per_lane": int(info.rows_per_lane), "lds_bytes": int(info.lds_bytes), "chunk": int(info.chunk),
                "launches": int(info.launches), "resident_waves": a.resident_waves,
                "nodes": int(sum(r.nodes for r in res)), "max_nodes": int(max(r.nodes for r in res)),
                "optimal": int(sum(r.status == lpg.OPTIMAL for r in res))}
        assert line["optimal"] == count, "a generated problem did not end OPTIMAL"
        legs = {"a": run_a}
        nd = min(D_MODELS, len(models))

        def run_d():
            t0 = time.perf_counter()
            refs = [bc.enumerate01(*mod) for mod in models[:nd]]
            return time.perf_counter() - t0, refs

        _, refs = run_d()
        bc.assert_same(bc.results_of(res[:nd], x[:nd]), bc.stacked(refs), "the batch against the statement")
        legs["d"] = run_d
        obj = np.array([r.objective for r in res])
        nc = min(C_MODELS, len(models))
        run_c = milp_leg(models[:nc])
        if run_c is not None:
            _, rc = run_c()
            assert all(r.status == 0 for r in rc) and (np.round([r.fun for r in rc]) == obj[:nc]).all(), "scipy differs"
            legs["c"] = run_c
        run_b, nb = ilp_leg(models) if n <= b_max_n else (None, 0)
        if n > b_max_n:
            line["b_status"] = f"left out: n > {b_max_n}"
        elif nb:
            try:
                _, sols = run_b()
                ok = all(s.status == "OPTIMAL" for s in sols)
                line["b_status"] = "ok" if ok else "left out: " + ",".join(sorted({s.status for s in sols}))
                if ok:
                    eligible = [q for q, mod in enumerate(models) if model_text(*mod) is not None][:nb]
                    assert all(round(s.z) == obj[q] for s, q in zip(sols, eligible)), \
                        "solve_ilp's objective differs"
                    line["b_nodes"], line["b_pivots"] = int(sum(s.nodes for s in sols)), int(sum(s.pivots for s in sols))
                    legs["b"] = run_b
            except Exception as e:                            # the route a caller had may not take the model at all
                line["b_status"] = f"left out: {type(e).__name__}: {str(e)[:80]}"
        else:
            line["b_status"] = "left out: no model the text front end takes (a zero cost or an empty row)"
        for run in legs.values():                             # warm-up
            run()
        kernel.clear()
        times = {k: [] for k in legs}
        for _ in range(repeats):                              # alternating
            for k, run in legs.items():
                times[k].append(run()[0])
    per = {"a": count, "b": nb, "c": nc, "d": nd}
    for k in legs:
        line[f"{k}_call"] = stats(times[k], per[k])
        line[f"{k}_us_per_problem"] = round(1e6 * statistics.median(times[k]) / per[k], 3)
    line["a_kernel"] = stats(kernel, count)
    line["a_nodes_per_s"] = round(line["nodes"] / statistics.median(times["a"]), 1)
    line["a_kernel_nodes_per_s"] = round(line["nodes"] / statistics.median(kernel), 1)
    line["a_ms_per_launch"] = round(1e3 * statistics.median(kernel) / max(1, line["launches"]), 4)
    for k in legs:
        if k != "a":
            line[f"{k}_over_a_per_problem"] = round(line[f"{k}_us_per_problem"] / line["a_us_per_problem"], 2)
    return line


def sweep(m, n, seed, repeats, max_nodes):
    """One large problem at split 0..min(n, 10): objective and x the same, nodes and time per split."""
    line = {"sweep": [m, n, seed], "splits": []}
    first = None
    for split in range(min(n, 10) + 1):
        with lpg.BinaryBatch(1, m, n, split=split) as b:
            ts = []
            for _ in range(repeats + 1):
                b.generate(seed)
                t0 = time.perf_counter()
                res = b.solve(max_nodes)
                ts.append(time.perf_counter() - t0)
            got = (res[0].status, res[0].objective, b.get().tobytes())
            if res[0].status == lpg.OPTIMAL:
                first = first or got
                assert got == first, "objective or x changes with the split"
            info = b.info
            line["splits"].append({"split": split, "status": lpg.STATUS_NAMES[res[0].status], "nodes": int(res[0].nodes),
                                   "launches": int(info.launches), "tier": "lds" if info.tier == 0 else "global",
                                   "call": stats(ts[1:]), "kernel_ms": round(info.kernel_ms, 4),
                                   "nodes_per_s": round(res[0].nodes / statistics.median(ts[1:]), 1)})
    line["auto_split"] = frontend.binary_split(1, m, n)
    return line


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="8x8x4096,16x16x4096,32x33x4096,64x64x1024,128x64x1024,256x64x256,8x8x64,64x64x64")
    ap.add_argument("--sweep", default="28x56x104")
    ap.add_argument("--sweep-max-nodes", type=int, default=4000000)
    ap.add_argument("--b-max-n", type=int, default=33)
    args = ap.parse_args(argv)
    out = open(args.out, "w") if args.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
    for spec in args.shapes.split(","):
        m, n, count = (int(v) for v in spec.split("x"))
        emit(bench_shape(m, n, count, args.repeats, b_max_n=args.b_max_n))
    if args.sweep:
        m, n, seed = (int(v) for v in args.sweep.split("x"))
        emit(sweep(m, n, seed, args.repeats, args.sweep_max_nodes))
    return 0


if __name__ == "__main__":
    sys.exit(main())
