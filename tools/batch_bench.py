#!/usr/bin/env python3
"""Batch solver vs a loop of single-LP engines: B generated LPs of one shape.

    python tools/batch_bench.py --m 64 --n 128 --batch 1024 [--repeats 5] [--kind dense] [--out FILE]

--kind artificial: the generator's artificial LPs (equality rows with
artificial unit columns) by the two-phase method, (a) generate_artificial +
BatchEngine.solve_two_phase, (b) generate(kind=GEN_ARTIFICIAL) +
Engine.solve_two_phase per LP. With --method big_m (valid with --kind
artificial): (a) a Big-M BatchEngine, generate_artificial + solve_big_m, (b)
Engine(flags=FLAG_BIG_M), generate(kind=GEN_ARTIFICIAL), solve_big_m, close
per LP.

(a) one BatchEngine.solve over B LPs (seeds S, S + 1, ...): generate (not
    timed), then the wall time of solve(), which returns after a device
    synchronise and the read-back of every LP's result;
(b) what a caller had before lpg_batch: for each seed, Engine(m, ncols),
    generate, solve, close -- the whole loop timed (allocation and launch
    cost are the price of that path), on the same GPU in the same process.

One warm-up of each, then `repeats` timed runs, (a) and (b) alternating. The
two must agree on every status and pivot count, else the run fails. Prints one
JSON line (and appends it to --out): LPs/s and pivots/s of both (median, min,
max), their ratio, whether (a) beats (b) by more than (b)'s spread, the
per-pivot time of one LP (workgroup) in (a), and for the LDS tier the LDS
traffic model of the rank-1 update: (m+1) * ncols * 8 bytes read and the same
written per pivot, at one CU's ds_read_b64 (256 B/clk) and ds_write_b64
(~85 B/clk) rates at 2.4 GHz.
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

CLK_HZ = 2.4e9
DS_READ_B64_BPC, DS_WRITE_B64_BPC = 256.0, 85.0      # bytes per clock and CU
KINDS = {"dense": 0, "degenerate": 1, "artificial": 2}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, required=True)
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20220518)
    ap.add_argument("--kind", choices=sorted(KINDS), default="dense")
    ap.add_argument("--method", choices=["two_phase", "big_m"], default="two_phase",
                    help="how --kind artificial is solved (big_m: Big-M batch vs a loop of FLAG_BIG_M engines)")
    ap.add_argument("--rule", choices=["dantzig", "bland"], default="dantzig")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-loop", action="store_true", help="time (a) only (e.g. to compare the tiers: LPG_BATCH_TIER=global)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import linearprogramming_amd as lpg
    m, n, B, nc = a.m, a.n, a.batch, a.n + a.m + 1
    kind, rule = KINDS[a.kind], 1 if a.rule == "bland" else 0
    budget = 50 * (m + n)
    two = a.kind == "artificial"
    bigm = a.method == "big_m"
    if bigm and not two:
        ap.error("--method big_m needs --kind artificial")
    cus = 256

    be = lpg.BatchEngine(B, m, nc, device=a.device, flags=lpg._lib.FLAG_NO_LOG, big_m=bigm)
    info = be.info

    def run_batch():
        if two:
            af = be.generate_artificial(n, a.seed)
            t0 = time.perf_counter()
            res = be.solve_big_m(af, None, budget, rule) if bigm else be.solve_two_phase(af, None, budget, rule)
        else:
            be.generate(n, a.seed, kind)
            t0 = time.perf_counter()
            res = be.solve(budget, rule)        # ends in a device synchronise + result read-back
        return time.perf_counter() - t0, [(r.status, r.pivots) for r in res]

    def run_loop():
        out = []
        t0 = time.perf_counter()
        for b in range(B):
            e = lpg.Engine(m, nc, device=a.device, flags=lpg._lib.FLAG_NO_LOG | (lpg._lib.FLAG_BIG_M if bigm else 0))
            e.generate(n, a.seed + b, kind)
            if bigm:
                r = e.solve_big_m(1 + n + (m + 1) // 2, None, budget, rule)
            else:
                r = e.solve_two_phase(1 + n + (m + 1) // 2, None, budget, rule) if two else e.solve(budget, rule)   # synchronises
            out.append((r.status, r.pivots))
            e.close()
        return time.perf_counter() - t0, out

    _, got_a = run_batch()                      # warm-up: code objects, first launches
    _, got_b = (0.0, got_a) if a.no_loop else run_loop()
    if got_a != got_b:
        bad = [i for i, (x, y) in enumerate(zip(got_a, got_b)) if x != y]
        print(json.dumps({"error": "batch and loop disagree", "first": bad[0], "batch": got_a[bad[0]],
                          "loop": got_b[bad[0]], "count": len(bad)}))
        return 1
    ta, tb = [], []
    for _ in range(a.repeats):
        t, g = run_batch()
        assert g == got_a
        ta.append(t)
        if a.no_loop:
            continue
        t, g = run_loop()
        assert g == got_a
        tb.append(t)
    be.close()

    pivots = sum(p for _, p in got_a)
    statuses = {}
    for s, _ in got_a:
        statuses[lpg.STATUS_NAMES[s]] = statuses.get(lpg.STATUS_NAMES[s], 0) + 1

    def rates(ts):
        med = statistics.median(ts)
        return {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts),
                "lps_per_s": B / med, "pivots_per_s": pivots / med}

    ra = rates(ta)
    # B workgroups share the CUs; a workgroup's pivot time is the solve time over the pivots of
    # the LPs that ran one after another on its CU slot (a lower bound on residency is 1 per CU
    # when the LDS footprint exceeds half a CU's LDS, as at 64 x 128)
    resident = max(1, min(B, cus * min(8, max(1, (160 * 1024) // (int(info.lds_bytes) + 512)))))
    line = {
        "bench": "batch_vs_loop", "m": m, "n": n, "ncols": nc, "batch": B, "kind": a.kind, "rule": a.rule,
        "method": ("big_m" if bigm else "two_phase") if two else "primal",
        "tier": "lds" if info.tier == lpg.BATCH_TIER_LDS else "global", "lds_bytes": int(info.lds_bytes),
        "chunk": int(info.chunk), "repeats": a.repeats, "statuses": statuses, "pivots": pivots,
        "batch_solve": ra,
        "us_per_pivot_per_lp_slot": ra["seconds_median"] * 1e6 * resident / pivots,
        "resident_lps_assumed": resident,
        "us_per_pivot_chip_batch": ra["seconds_median"] * 1e6 / pivots,
        "build_stamp": lpg._lib.build_stamp,
    }
    if not a.no_loop:
        rb = rates(tb)
        line.update({
            "engine_loop": rb, "ratio_lps": ra["lps_per_s"] / rb["lps_per_s"], "loop_spread_s": max(tb) - min(tb),
            "batch_beats_loop_beyond_spread": max(ta) < min(tb) and (min(tb) - max(ta)) > (max(tb) - min(tb)),
            "us_per_pivot_chip_loop": rb["seconds_median"] * 1e6 / pivots,
        })
    if info.tier == lpg.BATCH_TIER_LDS:
        bytes_each_way = (m + int(info.nobj)) * nc * 8
        line["lds_model_us_per_pivot"] = (bytes_each_way / DS_READ_B64_BPC + bytes_each_way / DS_WRITE_B64_BPC) / CLK_HZ * 1e6
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
