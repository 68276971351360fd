#!/usr/bin/env python3
"""Batch solver vs a loop of single-LP engines: B generated LPs of one shape.

    python tools/batch_bench.py --m 64 --n 128 --batch 1024 [--repeats 5] [--kind dense] [--out FILE]
    python tools/batch_bench.py --ragged --batch 1024 --shapes 64 [--dims 4 64] [--extra 130x130] [--out FILE]

--ragged: B dense LPs over K distinct seeded shapes (m and n drawn from
--dims; --extra MxN adds one LP of that shape), their tableaus made by a
uniform BatchEngine.generate per shape and read back (not timed). Then three
ways to solve them, each timed from the creation of its batches to the last
result (and, as a second figure, its solve calls alone): (i) one ragged batch;
(ii) one uniform batch per shape, created, loaded and solved in turn, which is
frontend.solve_batch(ragged=False); (iii) every LP zero-padded to the largest
shape in one uniform batch. One warm-up of each, then `repeats` timed runs,
the legs alternating; they must agree on every status and pivot count, else
the run fails.

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


def ragged_main(a) -> int:
    import random

    import numpy as np

    import linearprogramming_amd as lpg
    rnd = random.Random(a.seed)
    lo, hi = a.dims
    shapes = set()
    while len(shapes) < a.shapes:
        shapes.add((rnd.randint(lo, hi), rnd.randint(lo, hi)))
    shapes = sorted(shapes)
    of_lp = shapes + [shapes[rnd.randrange(len(shapes))] for _ in range(a.batch - len(shapes))]
    rnd.shuffle(of_lp)
    if a.extra:
        em, en = (int(x) for x in a.extra.lower().split("x"))
        of_lp.insert(len(of_lp) // 2, (em, en))
    B = len(of_lp)
    rule, flags = 1 if a.rule == "bland" else 0, lpg._lib.FLAG_NO_LOG
    members = {}
    for q, sh in enumerate(of_lp):
        members.setdefault(sh, []).append(q)
    tabs, bases = [None] * B, [None] * B
    for si, ((m, n), idx) in enumerate(members.items()):                 # set-up, not timed
        with lpg.BatchEngine(len(idx), m, n + m + 1, device=a.device, flags=flags) as e:
            e.generate(n, a.seed + 4096 * si, 0)
            T, bs = e.get_rows(), e.get_basis()
        for k, q in enumerate(idx):
            tabs[q], bases[q] = T[k], bs[k]
    M, NC = max(m for m, _ in of_lp), max(n + m + 1 for m, n in of_lp)
    budget = 50 * (M + NC)
    Tpad, bpad = np.zeros((B, M + 1, NC)), np.ones((B, M), dtype=np.int64)
    for q, (m, n) in enumerate(of_lp):                                    # zero rows and columns never pivot
        nc = n + m + 1
        Tpad[q, :m, :nc], Tpad[q, M, :nc], bpad[q, :m] = tabs[q][:m], tabs[q][m], bases[q]
    group_T = {sh: np.array([tabs[q] for q in idx]) for sh, idx in members.items()}
    group_b = {sh: np.array([bases[q] for q in idx]) for sh, idx in members.items()}

    def leg_ragged():
        t0 = time.perf_counter()
        with lpg.BatchEngine.ragged([(m, n + m + 1) for m, n in of_lp], device=a.device, flags=flags) as e:
            e.load(tabs, bases)
            t1 = time.perf_counter()
            res = e.solve(budget, rule)
            t2 = time.perf_counter()
            groups = len({e.shape(q).group for q in range(B)}) if not leg_ragged.groups else leg_ragged.groups
        leg_ragged.groups = groups
        return time.perf_counter() - t0, t2 - t1, [(r.status, r.pivots) for r in res]
    leg_ragged.groups = 0

    def leg_per_shape():
        out, ts = [None] * B, 0.0
        t0 = time.perf_counter()
        for (m, n), idx in members.items():
            with lpg.BatchEngine(len(idx), m, n + m + 1, device=a.device, flags=flags) as e:
                e.load(group_T[(m, n)], group_b[(m, n)])
                t1 = time.perf_counter()
                res = e.solve(budget, rule)
                ts += time.perf_counter() - t1
            for k, q in enumerate(idx):
                out[q] = (res[k].status, res[k].pivots)
        return time.perf_counter() - t0, ts, out

    def leg_padded():
        t0 = time.perf_counter()
        with lpg.BatchEngine(B, M, NC, device=a.device, flags=flags) as e:
            e.load(Tpad, bpad)
            t1 = time.perf_counter()
            res = e.solve(budget, rule)
            t2 = time.perf_counter()
            tier = "lds" if e.info.tier == lpg.BATCH_TIER_LDS else "global"
        leg_padded.tier = tier
        return time.perf_counter() - t0, t2 - t1, [(r.status, r.pivots) for r in res]

    legs = {"ragged": leg_ragged, "per_shape": leg_per_shape, "padded": leg_padded}
    want = None
    for name, leg in legs.items():                                        # warm-up, and the agreement check
        _, _, got = leg()
        want = got if want is None else want
        if got != want:
            bad = [q for q, (x, y) in enumerate(zip(got, want)) if x != y]
            print(json.dumps({"error": f"{name} and ragged disagree", "first": bad[0], "shape": of_lp[bad[0]],
                              name: got[bad[0]], "ragged": want[bad[0]], "count": len(bad)}))
            return 1
    total, solve = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(a.repeats):
        for name, leg in legs.items():
            t, ts, got = leg()
            assert got == want, name
            total[name].append(t)
            solve[name].append(ts)
    pivots = sum(p for _, p in want)

    def rates(ts):
        med = statistics.median(ts)
        return {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts), "lps_per_s": B / med}

    line = {"bench": "ragged", "batch": B, "shapes": len(members), "dims": [lo, hi], "extra": a.extra, "rule": a.rule,
            "max_m": M, "max_ncols": NC, "pivots": pivots, "repeats": a.repeats,
            "launch_groups": leg_ragged.groups,
            "padded_tier": leg_padded.tier, "build_stamp": lpg._lib.build_stamp}
    for name in legs:
        line[name] = {"create_load_solve": rates(total[name]), "solve_only": rates(solve[name])}
    for other in ("per_shape", "padded"):
        line[f"ragged_slowest_below_fastest_{other}"] = max(total["ragged"]) < min(total[other])
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int)
    ap.add_argument("--n", type=int)
    ap.add_argument("--ragged", action="store_true", help="B LPs over --shapes distinct shapes: ragged vs per-shape vs padded")
    ap.add_argument("--shapes", type=int, default=64)
    ap.add_argument("--dims", type=int, nargs=2, default=[4, 64], metavar=("LO", "HI"))
    ap.add_argument("--extra", default=None, metavar="MxN", help="--ragged: one more LP of this shape")
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
    if a.ragged:
        if a.shapes < 1 or a.batch < a.shapes or (a.dims[1] - a.dims[0] + 1) ** 2 < a.shapes:
            ap.error("--ragged needs 1 <= --shapes <= --batch and that many shapes within --dims")
        return ragged_main(a)
    if a.m is None or a.n is None:
        ap.error("--m and --n are required without --ragged")

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
