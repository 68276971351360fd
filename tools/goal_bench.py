#!/usr/bin/env python3
"""Goal batches measured: medians of 5 alternating repeats, every leg checked against the others first.

    python tools/goal_bench.py [--out FILE.jsonl] [--parent-lib LIB --parent-src ROOT] [--scipy-lps N]

Shapes (hard, goals, n, K) x count of tests/goal_cases.py's graded generator: 4096 x (4, 8, 8, 4),
1024 x (20, 40, 80, 5), 256 x (30, 70, 60, 4) (global tier). Legs, seconds per whole batch:
  (a) BatchEngine.solve_goal: one goal batch, load + solve + read-back of attain.
  (b) what a caller had before, on the device: the sequential method, K batch solves, level k with the earlier
      levels' optima added on the host as equality rows (an artificial each, so two-phase from level 1 on). The
      solves are BatchEngine's own (set_objective + solve, then solve_two_phase), which is what
      frontend.solve_batch runs underneath; solve_batch itself takes parsed model text, which generated
      tableaus do not have, and its parsing would only add host time to this leg.
  (c) the same sequential method with scipy.optimize.linprog, on the first --scipy-lps LPs only (a whole batch
      would take minutes), its time scaled by count / --scipy-lps; it alternates with (a) and (b) in the repeats.
  (d) a K = 2 goal batch beside the Big-M batch on the same generated artificial LPs, (64, 64) x 1024.
  (e) with --parent-lib: the parent commit's library beside this one on the plain (64, 128) and the two-phase
      (64, 64) batch of 1024 (batch leg only), for no regression in the existing modes.
(a), (b) and (c) must agree on every attained level (relative 1e-9) before anything is timed. An LP that (b)
loses (phase I ends INFEASIBLE because an earlier level's optimum, pinned as an equality, carries its rounding) is
counted in the output and left out of that comparison.
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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import goal_cases as gc  # noqa: E402
import linearprogramming_amd as lpg  # noqa: E402

SHAPES = [((4, 8, 8, 4), 4096), ((20, 40, 80, 5), 1024), ((30, 70, 60, 4), 256)]
REPEATS = 5


def build(shape, count, seed=1000):
    lps = [gc.graded(*shape, seed + b) for b in range(count)]
    return tuple(np.array([lp[i] for lp in lps]) for i in range(3))


def leg_goal(A, basis, costs):
    B, m, nc = A.shape
    K = costs.shape[1]
    T = np.zeros((B, m + K, nc))
    T[:, :m] = A
    t0 = time.perf_counter()
    with lpg.BatchEngine(B, m, nc, levels=K) as e:
        e.load(T, basis)
        res, attain = e.solve_goal(costs, 50 * (m + nc))
        tier = int(e.info.tier)
    dt = time.perf_counter() - t0
    assert all(r.status == lpg.OPTIMAL for r in res)
    return dt, attain, sum(r.pivots for r in res), tier


def leg_sequential_device(A, basis, costs):
    """Level k: the LP with the k rows  cost_j . x = attained_j  (j < k) behind its own, an artificial column each."""
    B, m, nc = A.shape
    K = costs.shape[1]
    attain = np.zeros((B, K))
    failed = np.zeros(B, dtype=bool)
    pivots = 0
    t0 = time.perf_counter()
    for k in range(K):
        T = np.zeros((B, m + k + 1, nc + k))
        T[:, :m, :nc] = A
        bas = np.zeros((B, m + k), dtype=np.int64)
        bas[:, :m] = basis
        for j in range(k):
            row = np.zeros((B, nc))
            row[:, 1:] = -costs[:, j]                           # the weighted deviation of level j ...
            row[:, 0] = -attain[:, j]                           # ... stays what level j reached
            # canonical form: zeros in the columns of the starting basis, a right-hand side >= 0
            g = np.take_along_axis(row, basis, axis=1)
            row -= np.einsum("bi,bij->bj", g, A)
            row *= np.where(row[:, 0] < 0, -1.0, 1.0)[:, None]
            T[:, m + j, :nc] = row
            T[:, m + j, nc + j] = 1.0
            bas[:, m + j] = nc + j
        c = np.zeros((B, nc + k - 1))
        c[:, :nc - 1] = costs[:, k]
        with lpg.BatchEngine(B, m + k, nc + k) as e:
            e.load(T, bas)
            if k == 0:
                e.set_objective(c)
                res = e.solve(50 * (m + nc))
            else:
                res = e.solve_two_phase(nc, c, 50 * (m + nc))
        # the method's own weakness: an earlier optimum pinned as an equality, rounded as it is, can leave phase I
        # above Big-M's feasibility threshold. Such an LP is counted, left out of the comparison, and goes on with 0
        status = np.array([r.status for r in res])
        assert set(status[~failed].tolist()) <= {lpg.OPTIMAL, lpg.INFEASIBLE}, (k, sorted(set(status.tolist())))
        failed |= status != lpg.OPTIMAL
        attain[:, k] = np.where(failed, 0.0, [r.objective for r in res])
        pivots += sum(r.pivots for r in res)
    return time.perf_counter() - t0, attain, pivots, failed


def leg_scipy(A, basis, costs, nlps):
    from scipy.optimize import linprog
    nlps = min(nlps, A.shape[0])
    attain = np.zeros((nlps, costs.shape[1]))
    t0 = time.perf_counter()
    for q in range(nlps):
        Aeq, beq = [A[q, :, 1:]], [A[q, :, 0]]
        for k, c in enumerate(costs[q]):
            r = linprog(-c, A_eq=np.vstack(Aeq), b_eq=np.concatenate(beq), bounds=(0, None), method="highs")
            assert r.status == 0, r.message
            attain[q, k] = -r.fun
            Aeq.append(-c[None, :])
            beq.append(np.array([r.fun]))
    return (time.perf_counter() - t0) * A.shape[0] / nlps, attain


def close(x, y):
    return float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y))))


def medians(legs):
    """{name: [seconds]} from REPEATS rounds in which the legs alternate."""
    times = {name: [] for name, _ in legs}
    for _ in range(REPEATS):
        for name, fn in legs:
            times[name].append(fn())
    return {name: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v)} for name, v in times.items()}


def bench_shape(shape, count, scipy_lps):
    A, basis, costs = build(shape, count)
    _, at_a, piv_a, tier = leg_goal(A, basis, costs)             # warm-up and check
    _, at_b, piv_b, failed = leg_sequential_device(A, basis, costs)
    _, at_c = leg_scipy(A, basis, costs, scipy_lps)
    diff_b, diff_c = close(at_a[~failed], at_b[~failed]), close(at_a[:at_c.shape[0]], at_c)
    assert diff_b <= 1e-9 and diff_c <= 1e-9, (diff_b, diff_c)
    out = medians([("goal_batch", lambda: leg_goal(A, basis, costs)[0]),
                   ("sequential_device", lambda: leg_sequential_device(A, basis, costs)[0]),
                   ("scipy_sequential_scaled", lambda: leg_scipy(A, basis, costs, scipy_lps)[0])])
    return {"bench": "goal", "shape": list(shape), "count": count, "m": int(A.shape[1]), "ncols": int(A.shape[2]),
            "tier": "global" if tier else "lds", "pivots_goal": int(piv_a), "pivots_sequential": int(piv_b),
            "sequential_lps_lost_to_rounding": int(failed.sum()),
            "max_rel_diff_sequential": diff_b, "max_rel_diff_scipy": diff_c, "scipy_lps_timed": int(at_c.shape[0]), **out}


def bench_big_m(m=64, n=64, B=1024):
    A, basis, costs, af = gc.artificial(m, n, 2, B, 20220518)
    nc = n + m + 1
    T2 = np.zeros((B, m + 2, nc))
    T2[:, :m] = A

    def goal():
        t0 = time.perf_counter()
        with lpg.BatchEngine(B, m, nc, levels=2) as e:
            e.load(T2, basis)
            res, _ = e.solve_goal(costs, 50 * (m + n))
            rows = e.get_rows()
        return time.perf_counter() - t0, res, rows

    def big_m():
        t0 = time.perf_counter()
        with lpg.BatchEngine(B, m, nc, big_m=True) as e:
            e.load(T2, basis)
            res = e.solve_big_m(af, np.hstack([costs[:, 1], np.zeros((B, 1))]), 50 * (m + n))
            rows = e.get_rows()
        return time.perf_counter() - t0, res, rows

    (_, rg, Tg), (_, rb, Tb) = goal(), big_m()
    assert np.array_equal(Tg.view(np.int64), Tb.view(np.int64)) and [r.pivots for r in rg] == [r.pivots for r in rb]
    out = medians([("goal_K2", lambda: goal()[0]), ("big_m", lambda: big_m()[0])])
    return {"bench": "goal_vs_big_m", "m": m, "n": n, "count": B, "pivots": int(sum(r.pivots for r in rg)), **out}


def bench_parent(parent_lib, parent_src):
    from linearprogramming_amd import _lib
    libs = {"parent": _lib.load(parent_lib, parent_src), "this": _lib.load()}
    out = []
    for name, m, n, two_phase in (("plain", 64, 128, False), ("two_phase", 64, 64, True)):
        def run(lib):
            with lpg.BatchEngine(1024, m, n + m + 1, lib=lib) as e:
                if two_phase:
                    af = e.generate_artificial(n)
                    t0 = time.perf_counter()
                    res = e.solve_two_phase(af, None, 50 * (m + n))
                else:
                    e.generate(n)
                    t0 = time.perf_counter()
                    res = e.solve(50 * (m + n))
                return time.perf_counter() - t0, sum(r.pivots for r in res)
        assert run(libs["parent"])[1] == run(libs["this"])[1]
        out.append({"bench": "goal_parent", "mode": name, "m": m, "n": n, "count": 1024,
                    **medians([(k, (lambda lib=lib: run(lib)[0])) for k, lib in libs.items()])})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-src")
    ap.add_argument("--scipy-lps", type=int, default=32)
    args = ap.parse_args(argv)
    lines = [bench_shape(shape, count, args.scipy_lps) for shape, count in SHAPES]
    lines.append(bench_big_m())
    if args.parent_lib:
        lines += bench_parent(args.parent_lib, args.parent_src or os.path.dirname(os.path.dirname(args.parent_lib)))
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
