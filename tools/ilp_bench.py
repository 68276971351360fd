#!/usr/bin/env python3
"""One level of a branch-and-bound tree: children on the device vs the host round trip.

    python tools/ilp_bench.py [--shapes 8x8x4096 64x128x1024 96x160x1024] [--repeats 5] [--out FILE] [--kernel-trace]
                               [--cuts K]

For each MxNxB: B generated dense LPs of m rows and n structural columns are
solved (not timed) and branch_select picks every LP's branching row (not
timed; both legs use it). Every LP gets its two children, down before up,
2 B children in all, and the level is made and re-optimised in two ways:

(a) device: BatchEngine.branch (lpg_batch_branch: the child batch is allocated
    and filled on the device) + solve_dual;
(b) host route, what a caller had before lpg_batch_branch: get_rows /
    get_basis of the parents, the child tableaus built in numpy (vectorised),
    a new BatchEngine, load, solve_dual.

Both are timed from their first call to the last result, closing the child
batch not included. One warm-up of each, then `repeats` timed runs, the legs
alternating; they must agree on every status and pivot count, else the run
fails. Prints one JSON line per shape (and appends it to --out): the seconds
of both legs (median, min, max), whether the slowest device repeat is below
the fastest host-route repeat, and the branch() call alone: its seconds and
the bytes lpg_batch_branch reads and writes (the parents' rows once per child,
the children's rows) over that time in GB/s, next to the 5590 GB/s copy
ceiling of tools/hbm_ceiling.hip. The call includes the allocation and the
zero fill of the child batch and a synchronisation, so that figure is a lower
bound of the kernel's own rate.

--cuts K: the same protocol for one round of Gomory mixed-integer cuts instead
of a level: every parent with at least K candidate rows (all-ones mask) gets
one child with its K most fractional rows cut, (a) by BatchEngine.cut
(lpg_batch_cut) + solve_dual, (b) by get_rows / get_basis, the cut rows in
numpy (vectorised), a new BatchEngine, load, solve_dual. The line reports
bench "ilp_cuts", cut_call_s / cut_bytes / cut_call_gbs, and with
--kernel-trace cut_kernel_us / cut_kernel_gbs from the k_batch_cut dispatches.

--kernel-trace: k_batch_branch alone. Before the timed runs of a shape, a
child process runs the device leg of that shape (warm-up and `repeats`
launches) under `rocprofv3 --kernel-trace`, and the median duration of the
k_batch_branch dispatches in its trace gives branch_kernel_us and
branch_kernel_gbs (the same bytes over that time).
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

COPY_CEILING_GBS = 5590.0


def host_children(T, basis, src, row, d):
    """The children of lpg_batch_branch in numpy, for parents whose columns are all active."""
    import numpy as np
    n, m, nc = len(src), T.shape[1] - 1, T.shape[2]
    C = np.zeros((n, m + 2, nc + 1))
    C[:, :m, :nc] = T[src, :m]
    C[:, m + 1, :nc] = T[src, m]
    idx = np.arange(n)
    v = T[src, row, 0]
    new = T[src, row] * d[:, None].astype(np.float64)
    new[:, 0] = np.where(d < 0, np.floor(v) - v, v - np.ceil(v))
    new[idx, basis[src, row]] = 0.0
    C[:, m, :nc] = new
    C[:, m, nc] = 1.0
    cb = np.concatenate([basis[src], np.full((n, 1), nc, dtype=np.int64)], axis=1)
    return C, cb


def host_cut_children(T, basis, src, rows):
    """The children of lpg_batch_cut in numpy, for parents whose columns are all active and all integer-constrained
    (include/lpg.h, "cuts"); rows: [n, K]."""
    import numpy as np
    n, K, m, nc = len(src), rows.shape[1], T.shape[1] - 1, T.shape[2]

    def frac(x):
        f = x - np.floor(x)
        return np.where(f >= 1.0, 0.0, f)

    a = T[src[:, None], rows]                              # [n, K, nc]
    f0 = frac(a[:, :, 0])
    rho = f0 / (1.0 - f0)
    f = frac(a)
    g = np.where(f <= f0[:, :, None], f, rho[:, :, None] * (1.0 - f))
    basic = np.zeros((n, nc), dtype=bool)
    np.put_along_axis(basic, basis[src], True, axis=1)
    g[np.broadcast_to(basic[:, None, :], g.shape)] = 0.0
    new = -g
    new[:, :, 0] = -f0
    C = np.zeros((n, m + K + 1, nc + K))
    C[:, :m, :nc] = T[src, :m]
    C[:, m:m + K, :nc] = new
    C[:, m + K, :nc] = T[src, m]
    C[:, m + np.arange(K), nc + np.arange(K)] = 1.0
    cb = np.concatenate([basis[src], np.broadcast_to(nc + np.arange(K), (n, K))], axis=1)
    return C, cb


def kernel_seconds(shape, repeats, seed, cuts=0):
    """Durations of the k_batch_branch dispatches of one shape's device leg, from a kernel trace of a child process."""
    import csv
    import glob
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--device-leg-only", "--shapes", shape, "--repeats", str(repeats), "--seed", str(seed),
               "--cuts", str(cuts)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 failed rc={p.returncode}: {p.stderr[-1000:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel trace")
        out = []
        with open(files[0], newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                if ("k_batch_cut<" if cuts else "k_batch_branch<") in name and "select" not in name:
                    out.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
    if not out:
        raise RuntimeError("no %s dispatch in the kernel trace" % ("k_batch_cut" if cuts else "k_batch_branch"))
    return out


def run(m, n, B, repeats, seed, device_only=False, cuts=0):
    import numpy as np

    import linearprogramming_amd as lpg
    nc = n + m + 1
    e = lpg.BatchEngine(B, m, nc)
    e.generate(n, seed, lpg.GEN_DENSE)
    res = e.solve()
    assert all(r.status == lpg.OPTIMAL for r in res)
    ones = np.ones(nc - 1, dtype=np.uint8)
    if cuts:
        cand = e.cut_select(ones, 1e-6, cuts)
        src = np.array([q for q in range(B) if len(cand[q]) == cuts], dtype=np.int64)
        assert len(src), f"no LP of {m}x{n} has {cuts} candidate rows"
        row = np.array([cand[q] for q in src], dtype=np.int64)          # [n, K]
    else:
        pick, _, _ = e.branch_select(ones)
        parents = np.flatnonzero(pick >= 0)
        src = np.repeat(parents, 2)
        row = pick[src]
        d = np.tile(np.array([-1, 1], dtype=np.int8), len(parents))

    def device():
        t0 = time.perf_counter()
        ch = e.cut(src, row, ones) if cuts else e.branch(src, row, d)
        t1 = time.perf_counter()
        r = ch.solve_dual()
        t2 = time.perf_counter()
        ch.close()
        return t2 - t0, t1 - t0, [(x.status, x.pivots) for x in r]

    def host():
        t0 = time.perf_counter()
        if cuts:
            C, cb = host_cut_children(e.get_rows(), e.get_basis(), src, row)
        else:
            C, cb = host_children(e.get_rows(), e.get_basis(), src, row, d)
        ch = lpg.BatchEngine(len(src), C.shape[1] - 1, C.shape[2])
        ch.load(C, cb)
        r = ch.solve_dual()
        t2 = time.perf_counter()
        ch.close()
        return t2 - t0, 0.0, [(x.status, x.pivots) for x in r]

    legs = {"device": device} if device_only else {"device": device, "host": host}
    want = None
    for fn in legs.values():                               # warm-up, and the two legs agree
        got = fn()[2]
        assert want is None or got == want, "the legs disagree on a status or a pivot count"
        want = got
    t = {k: [] for k in legs}
    tb = []
    for _ in range(repeats):
        for k, fn in legs.items():
            sec, sec_branch, got = fn()
            assert got == want, f"{k}: statuses or pivots changed between repeats"
            t[k].append(sec)
            if k == "device":
                tb.append(sec_branch)
    e.close()
    if device_only:
        return {"children": int(len(src))}
    K = cuts if cuts else 1
    ld_p, ld_c = (nc + 63) & ~63, (nc + K + 63) & ~63
    moved = len(src) * 8 * ((m + K + 1) * nc + (m + K + 1) * (nc + K))
    stat = lambda x: {"median": statistics.median(x), "min": min(x), "max": max(x)}
    call = "cut" if cuts else "branch"
    out = {"bench": "ilp_cuts" if cuts else "ilp_level", "m": m, "n": n, "parents": int(B), "children": int(len(src)),
           "repeats": repeats, "ld_parent": ld_p, "ld_child": ld_c, "pivots": int(sum(p for _, p in want)),
           "device_s": stat(t["device"]), "host_s": stat(t["host"]),
           "host_over_device": statistics.median(t["host"]) / statistics.median(t["device"]),
           "slowest_device_below_fastest_host": max(t["device"]) < min(t["host"]),
           call + "_call_s": stat(tb), call + "_bytes": moved,
           call + "_call_gbs": moved / statistics.median(tb) / 1e9, "copy_ceiling_gbs": COPY_CEILING_GBS}
    if cuts:
        out["cuts"] = cuts
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["8x8x4096", "64x128x1024", "96x160x1024"], help="MxNxB")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20220518)
    ap.add_argument("--out")
    ap.add_argument("--kernel-trace", action="store_true",
                    help="k_batch_branch (--cuts: k_batch_cut) alone, from a rocprofv3 kernel trace")
    ap.add_argument("--cuts", type=int, default=0, help="K: one round of K cuts per LP instead of a level of the tree")
    ap.add_argument("--device-leg-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    for shape in a.shapes:
        m, n, B = (int(x) for x in shape.split("x"))
        if a.device_leg_only:
            run(m, n, B, a.repeats, a.seed, device_only=True, cuts=a.cuts)
            continue
        ks = kernel_seconds(shape, a.repeats, a.seed, a.cuts) if a.kernel_trace else None
        res = run(m, n, B, a.repeats, a.seed, cuts=a.cuts)
        if ks:
            call = "cut" if a.cuts else "branch"
            res[call + "_kernel_us"] = {"median": statistics.median(ks) * 1e6, "min": min(ks) * 1e6, "max": max(ks) * 1e6,
                                        "dispatches": len(ks)}
            res[call + "_kernel_gbs"] = res[call + "_bytes"] / statistics.median(ks) / 1e9
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
