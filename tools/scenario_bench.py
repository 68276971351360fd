#!/usr/bin/env python3
"""Right-hand-side scenarios: warm-started on the device vs loaded and solved cold.

    python tools/scenario_bench.py [--m 64 --n 128] [--art-m 16 --art-n 16] [--scenarios 1024] [--repeats 5]
                                   [--out profiles/scenario_bench.jsonl] [--kernel-trace]

Two LPs, one generated dense LP of m rows and n structural columns and one
generated artificial LP (GEN_ARTIFICIAL, solved two-phase), each under
`scenarios` right-hand sides: scenario 0 is the LP's own b, scenario c is
b * (0.2 + 2.5 * rng.random(m)), rng = numpy.random.default_rng(11). The
scenarios are solved in two ways:

(a) warm: a batch of one is created, loaded and solved; BatchEngine.scenario
    (lpg_batch_scenario) makes the batch of the scenarios from the solved
    tableau on the device; one solve_dual re-optimises them;
(b) cold, what a caller had before lpg_batch_scenario: the same LPs, their
    tableaus prepared on the host before the clock starts, loaded into one
    batch and solved from the slack basis (the artificial LP: two-phase).

Both are timed from the creation of their first batch to the last result,
closing the batches not included. One warm-up of each, then `repeats` timed
runs, the legs alternating. Prints one JSON line per LP (and appends it to
--out): the seconds of both legs (median, min, max), their pivots, how many
scenarios end in a different status, and

(d) a sweep in steps on batches that stay, `2 * repeats` timed steps whose
    right-hand sides alternate between two sets: set_rhs + solve_dual on the
    solved children (step_warm_s) against load + a cold solve on a batch kept
    for it (step_cold_s); neither allocates;
(c) the scenario() call alone for each walk of column 0 (the default, a
    lane per row, and LPG_SCENARIO_WALK=tile): its seconds and the bytes the kernel moves (the parent's rows
    read once per child, the children's rows written, the ident columns read
    once more) over that time in GB/s. The call includes the allocation and
    zero fill of the child batch, the uploads and a synchronisation.

--kernel-trace: the kernels alone. Per walk a child process runs leg (a) and
one set_rhs on its children under `rocprofv3 --kernel-trace`; the median
durations of the k_batch_scenario and k_batch_set_rhs dispatches give
scenario_kernel_us / scenario_kernel_gbs and set_rhs_kernel_us (the column
walk without the copy).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WALKS = ("rows", "tile")                                  # the default first


def kernel_seconds(argv, walk):
    """{kernel: durations} of the k_batch_scenario and k_batch_set_rhs dispatches of a child process's device leg."""
    import csv
    import glob
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--device-leg-only"] + argv
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env={**os.environ, "LPG_SCENARIO_WALK": walk})
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 failed rc={p.returncode}: {p.stderr[-1000:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel trace")
        out = {"k_batch_scenario": [], "k_batch_set_rhs": []}
        with open(files[0], newline="") as f:
            for r in csv.DictReader(f):
                for k in out:
                    if k in r["Kernel_Name"]:
                        out[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
    if not out["k_batch_scenario"] or not out["k_batch_set_rhs"]:
        raise RuntimeError("no k_batch_scenario / k_batch_set_rhs dispatch in the kernel trace")
    return out


def run(kind, m, n, S, repeats, seed, device_only=False):
    import numpy as np

    import linearprogramming_amd as lpg
    nc = n + m + 1
    art = kind == "artificial"
    g = lpg.BatchEngine(1, m, nc)
    af = g.generate_artificial(n, seed) if art else g.generate(n, seed, lpg.GEN_DENSE)
    T0, basis = g.get_rows(), g.get_basis()
    ident = basis[0]
    g.close()
    rng = np.random.default_rng(11)
    b = T0[0, :m, 0]
    rhs = np.array([b] + [b * (0.2 + 2.5 * rng.random(m)) for _ in range(S - 1)])
    src = np.zeros(S, dtype=np.int64)
    cold_T = np.tile(T0, (S, 1, 1))
    cold_T[:, :m, 0] = rhs
    cold_basis = np.tile(basis, (S, 1))

    def solve(e):
        return e.solve_two_phase(af, None) if art else e.solve()

    def warm(extra=False):
        t0 = time.perf_counter()
        base = lpg.BatchEngine(1, m, nc)
        base.load(T0, basis)
        r0 = solve(base)
        t1 = time.perf_counter()
        ch = base.scenario(src, rhs, ident)
        t2 = time.perf_counter()
        r = ch.solve_dual()
        t3 = time.perf_counter()
        if extra:
            ch.set_rhs(rhs, ident)
        ch.close()
        base.close()
        assert r0[0].status == lpg.OPTIMAL
        return t3 - t0, t2 - t1, [x.status for x in r], sum(x.pivots for x in r) + r0[0].pivots

    def cold():
        t0 = time.perf_counter()
        e = lpg.BatchEngine(S, m, nc)
        e.load(cold_T, cold_basis)
        r = solve(e)
        t3 = time.perf_counter()
        e.close()
        return t3 - t0, 0.0, [x.status for x in r], sum(x.pivots for x in r)

    if device_only:
        for _ in range(repeats + 1):
            warm(extra=True)
        return None
    walk0 = os.environ.get("LPG_SCENARIO_WALK")
    os.environ["LPG_SCENARIO_WALK"] = WALKS[0]
    legs = {"warm": warm, "cold": cold}
    first = {k: fn() for k, fn in legs.items()}                  # warm-up
    t = {k: [] for k in legs}
    call = {w: [] for w in WALKS}
    for _ in range(repeats):
        for k, fn in legs.items():
            sec, sec_call, st, _ = fn()
            assert st == first[k][2], f"{k}: statuses changed between repeats"
            t[k].append(sec)
            if k == "warm":
                call[WALKS[0]].append(sec_call)
    for w in WALKS[1:]:
        os.environ["LPG_SCENARIO_WALK"] = w
        sec, sec_call, st, _ = warm()
        assert st == first["warm"][2], f"walk {w}: statuses differ"
        call[w] = [warm()[1] for _ in range(repeats)]
    if walk0 is None:
        del os.environ["LPG_SCENARIO_WALK"]
    else:
        os.environ["LPG_SCENARIO_WALK"] = walk0
    # (d) a sweep in steps on batches that stay: the right-hand sides alternate between two sets
    rhs2 = np.array([b * (0.2 + 2.5 * rng.random(m)) for _ in range(S)])
    cold_T2 = cold_T.copy()
    cold_T2[:, :m, 0] = rhs2
    base = lpg.BatchEngine(1, m, nc)
    base.load(T0, basis)
    solve(base)
    ch = base.scenario(src, rhs, ident)
    ch.solve_dual()
    e = lpg.BatchEngine(S, m, nc)

    def warm_step(r, _):
        t0 = time.perf_counter()
        ch.set_rhs(r, ident)
        res = ch.solve_dual()
        return time.perf_counter() - t0, [x.status for x in res], sum(x.pivots for x in res)

    def cold_step(_, Tx):
        t0 = time.perf_counter()
        e.load(Tx, cold_basis)
        res = solve(e)
        return time.perf_counter() - t0, [x.status for x in res], sum(x.pivots for x in res)

    steps = {"warm": warm_step, "cold": cold_step}
    ts, piv, mism = {k: [] for k in steps}, {k: 0 for k in steps}, 0
    for it in range(2 + 2 * repeats):                            # one warm-up step per set, then the timed ones
        args = (rhs2, cold_T2) if it % 2 == 0 else (rhs, cold_T)
        got = {k: fn(*args) for k, fn in steps.items()}
        mism += sum(1 for x, y in zip(got["warm"][1], got["cold"][1]) if x != y)
        if it >= 2:
            for k in steps:
                ts[k].append(got[k][0])
                piv[k] += got[k][2]
    for x in (ch, base, e):
        x.close()
    moved = S * 8 * (2 * (m + 1) * nc + (m + 1) * m)
    stat = lambda x: {"median": statistics.median(x), "min": min(x), "max": max(x)}
    return {"bench": "scenarios", "kind": kind, "m": m, "n": n, "scenarios": S, "repeats": repeats,
            "warm_s": stat(t["warm"]), "cold_s": stat(t["cold"]),
            "cold_over_warm": statistics.median(t["cold"]) / statistics.median(t["warm"]),
            "slowest_warm_below_fastest_cold": max(t["warm"]) < min(t["cold"]),
            "warm_pivots": int(first["warm"][3]), "cold_pivots": int(first["cold"][3]),
            "status_mismatches": sum(1 for x, y in zip(first["warm"][2], first["cold"][2]) if x != y),
            "not_optimal": sum(1 for x in first["cold"][2] if x != lpg.OPTIMAL),
            "step_warm_s": stat(ts["warm"]), "step_cold_s": stat(ts["cold"]),
            "step_cold_over_warm": statistics.median(ts["cold"]) / statistics.median(ts["warm"]),
            "slowest_warm_step_below_fastest_cold_step": max(ts["warm"]) < min(ts["cold"]),
            "step_warm_pivots": int(piv["warm"]), "step_cold_pivots": int(piv["cold"]), "step_status_mismatches": mism,
            "scenario_bytes": moved,
            "scenario_call_s": {w: stat(call[w]) for w in WALKS},
            "scenario_call_gbs": {w: moved / statistics.median(call[w]) / 1e9 for w in WALKS}}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--art-m", type=int, default=16)
    ap.add_argument("--art-n", type=int, default=16)
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20220518)
    ap.add_argument("--out")
    ap.add_argument("--kernel-trace", action="store_true",
                    help="k_batch_scenario and k_batch_set_rhs alone, per walk, from a rocprofv3 kernel trace")
    ap.add_argument("--kind", choices=["dense", "artificial"], help=argparse.SUPPRESS)
    ap.add_argument("--device-leg-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    cases = [("dense", a.m, a.n), ("artificial", a.art_m, a.art_n)]
    for kind, m, n in cases:
        if a.kind and kind != a.kind:
            continue
        if a.device_leg_only:
            run(kind, m, n, a.scenarios, a.repeats, a.seed, device_only=True)
            continue
        res = run(kind, m, n, a.scenarios, a.repeats, a.seed)
        if a.kernel_trace:
            sub = ["--kind", kind, "--m", str(a.m), "--n", str(a.n), "--art-m", str(a.art_m), "--art-n", str(a.art_n),
                   "--scenarios", str(a.scenarios), "--repeats", str(a.repeats), "--seed", str(a.seed)]
            res["scenario_kernel_us"], res["scenario_kernel_gbs"], res["set_rhs_kernel_us"] = {}, {}, {}
            for w in WALKS:
                ks = kernel_seconds(sub, w)
                sk, rk = statistics.median(ks["k_batch_scenario"]), statistics.median(ks["k_batch_set_rhs"])
                res["scenario_kernel_us"][w] = sk * 1e6
                res["scenario_kernel_gbs"][w] = res["scenario_bytes"] / sk / 1e9
                res["set_rhs_kernel_us"][w] = rk * 1e6
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
