#!/usr/bin/env python3
"""Ranging: on the device vs read back and walked in numpy.

    python tools/ranging_bench.py [--repeats 5] [--out profiles/ranging_bench.jsonl] [--kernel-trace]
                                  [--shape KIND M N COUNT]

Per shape (default: dense 64 x 128 x 1024, artificial 16 x 16 x 1024,
artificial 96 x 96 x 512, dense 256 x 256 x 512) one generated batch is solved
(the artificial kind two-phase) and then ranged in two ways:

(a) BatchEngine.ranging (lpg_batch_ranging, k_batch_ranging) on the solved
    batch: wall time of the call, which ends with the nine arrays on the host;
(b) what a caller had before: get_rows + get_basis, then the ranging of the
    whole batch in vectorised numpy (ranging_numpy below, a few LPs at a time
    so that its temporaries stay near 64 MB).

The tool fails unless the two agree bit for bit. One warm-up of each, then
`repeats` timed runs, the legs alternating. Prints one JSON line per shape (and
appends it to --out): the seconds of both legs (median, min, max), the seconds
of leg (b)'s read-back alone, and the LPs ranged.

--kernel-trace: the kernel alone. A child process runs leg (a) under
`rocprofv3 --kernel-trace`, three times with all groups, three times with the
cost group alone and three times with the right-hand-side group alone; the
median durations of those k_batch_ranging dispatches give kernel_us,
kernel_cost_us and kernel_rhs_us (which phase the kernel's time is in).
kernel_us is set against the bytes the definition reads, about
(m * nact + m * m + ncols) * 8 per LP, as kernel_gbs and as a fraction of the
5.59 TB/s copy ceiling of DESIGN.md §3.4.
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

SHAPES = [("dense", 64, 128, 1024), ("artificial", 16, 16, 1024), ("artificial", 96, 96, 512), ("dense", 256, 256, 512)]
FIELDS = ("dual", "cost_lo", "cost_hi", "cost_lo_at", "cost_hi_at", "rhs_lo", "rhs_hi", "rhs_lo_at", "rhs_hi_at")
COPY_CEILING = 5.59e12
OPTIMAL = 1


def _bound(x, a, cand, upper, none, index0):
    """One bound per leading entry over the last axis: x, a, cand [..., K] -> (q [...], index [...]); the index
    is the position along the axis plus index0."""
    import numpy as np
    with np.errstate(all="ignore"):
        q = (-x) / a
    cand = cand & ((a < -1e-9) if upper else (a > 1e-9)) & ~np.isnan(q)
    key = np.where(cand, q, np.inf if upper else -np.inf)
    best = key.min(-1) if upper else key.max(-1)
    first = np.argmax(cand & (q == best[..., None]), -1)          # equal ratios: the smallest index
    some = cand.any(-1)
    return np.where(some, np.take_along_axis(q, first[..., None], -1)[..., 0], np.inf if upper else -np.inf), \
        np.where(some, first + index0, none)


def ranging_numpy(T, basis, nact, ident, status):
    """include/lpg.h's "ranging" for a batch of one shape in numpy: T [B, m+1, ncols], basis and ident [B, m],
    status [B]; eps_piv = 1e-9. Returns {field: [B, m] or [B, ncols - 1]}."""
    import numpy as np
    B, m, N = T.shape[0], T.shape[1] - 1, T.shape[2] - 1
    out = {f: (np.zeros if f.endswith("_at") else np.empty)((B, N if f.startswith("cost") else m),
                                                           dtype=np.int64 if f.endswith("_at") else np.float64) for f in FIELDS}
    step = max(1, (64 << 20) // (8 * m * max(m, nact)))
    cols = np.arange(1, N + 1)
    for q0 in range(0, B, step):
        s = slice(q0, min(B, q0 + step))
        Ts, bs, ids = T[s], basis[s], ident[s]
        n = Ts.shape[0]
        obj = Ts[:, m, :]
        out["dual"][s] = np.take_along_axis(obj, ids, 1)
        # right-hand sides: frame row i along axis 1, candidate row r along the last axis
        a = np.take_along_axis(Ts[:, :m, :], ids[:, None, :], 2).transpose(0, 2, 1)
        x = np.broadcast_to(Ts[:, None, :m, 0], a.shape)
        every = np.ones(a.shape, dtype=bool)
        out["rhs_lo"][s], out["rhs_lo_at"][s] = _bound(x, a, every, False, -1, 0)
        out["rhs_hi"][s], out["rhs_hi_at"][s] = _bound(x, a, every, True, -1, 0)
        # costs: nonbasic and inert columns first, then the basic ones from their rows
        member = np.zeros((n, N + 1), dtype=bool)
        np.put_along_axis(member, bs, True, 1)
        inert = cols[None, :] > nact
        out["cost_lo"][s], out["cost_lo_at"][s] = -np.inf, 0
        out["cost_hi"][s] = np.where(inert, np.inf, obj[:, 1:])
        out["cost_hi_at"][s] = np.where(inert, 0, cols[None, :])
        a = Ts[:, :m, 1:nact + 1]
        x = np.broadcast_to(obj[:, None, 1:nact + 1], a.shape)
        cand = np.broadcast_to(~member[:, None, 1:nact + 1], a.shape)
        ranged = bs <= nact                                       # a kept artificial ranges nothing
        qq, rr = np.nonzero(ranged)
        for up, (fq, fat) in ((False, ("cost_lo", "cost_lo_at")), (True, ("cost_hi", "cost_hi_at"))):
            v, at = _bound(x, a, cand, up, 0, 1)
            out[fq][q0 + qq, bs[qq, rr] - 1] = v[qq, rr]
            out[fat][q0 + qq, bs[qq, rr] - 1] = at[qq, rr]
    bad = np.asarray(status) != OPTIMAL
    for f in FIELDS:
        out[f][bad] = (0 if f.startswith("cost") else -1) if f.endswith("_at") else np.nan
    return out


def solved(kind, m, n, count, seed):
    """(engine, results, ident [count, m]) of the generated batch, solved."""
    import numpy as np

    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(count, m, n + m + 1)
    if kind == "artificial":
        af = e.generate_artificial(n, seed)
        ident = e.get_basis()
        res = e.solve_two_phase(af, None)
    else:
        e.generate(n, seed, lpg.GEN_DENSE)
        ident = e.get_basis()
        res = e.solve()
    return e, res, np.ascontiguousarray(ident)


def kernel_seconds(shape, seed):
    """The durations of the k_batch_ranging dispatches of a child process's leg (a), in the order of their start:
    three with all groups, three with the cost group, three with the right-hand-side group."""
    import csv
    import glob
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--device-leg-only", "--seed", str(seed), "--shape"] + [str(x) for x in shape]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 failed rc={p.returncode}: {p.stderr[-1000:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel trace")
        with open(files[0], newline="") as f:
            out = sorted((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
                         for r in csv.DictReader(f) if "k_batch_ranging" in r["Kernel_Name"])
    if len(out) != 9:
        raise RuntimeError(f"{len(out)} k_batch_ranging dispatches in the kernel trace, expected 9")
    return [d for _, d in out]


def run(kind, m, n, count, repeats, seed, device_only=False):
    import numpy as np
    e, res, ident = solved(kind, m, n, count, seed)
    try:
        status = [r.status for r in res]
        nact = e.active_columns(0)[0]

        def device():
            t0 = time.perf_counter()
            r = e.ranging(ident)
            return time.perf_counter() - t0, 0.0, {f: getattr(r, f) for f in FIELDS}

        def host():
            t0 = time.perf_counter()
            T, basis = e.get_rows(), e.get_basis()
            t1 = time.perf_counter()
            out = ranging_numpy(T, basis, nact, ident, status)
            return time.perf_counter() - t0, t1 - t0, out

        if device_only:
            for groups in ({}, {"dual": False, "rhs": False}, {"dual": False, "cost": False}):
                for _ in range(3):
                    e.ranging(ident, **groups)
            return None
        a, b = device()[2], host()[2]                                # the warm-up, and the agreement
        for f in FIELDS:
            x, y = (np.ascontiguousarray(v).view(np.uint64 if v.dtype == np.float64 else np.int64) for v in (a[f], b[f]))
            if not np.array_equal(x, y):
                raise SystemExit(f"ranging_bench: {kind} {m} x {n}: {f} differs between the device and numpy in "
                                 f"{int((x != y).sum())} of {x.size} entries")
        ta, tb, tr = [], [], []
        for _ in range(repeats):
            ta.append(device()[0])
            t, r, _ = host()
            tb.append(t)
            tr.append(r)
    finally:
        e.close()
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return {"bench": "ranging", "kind": kind, "m": m, "n": n, "count": count, "repeats": repeats, "nact": nact,
            "ranged": int(sum(s == OPTIMAL for s in status)), "device_s": stat(ta), "host_s": stat(tb), "host_readback_s": stat(tr),
            "host_over_device": statistics.median(tb) / statistics.median(ta),
            "slowest_device_below_fastest_host": max(ta) < min(tb), "bit_for_bit": True}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", nargs=4, metavar=("KIND", "M", "N", "COUNT"), action="append")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20220518)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranging_bench.jsonl"))
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--device-leg-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    shapes = [(k, int(m), int(n), int(c)) for k, m, n, c in a.shape] if a.shape else SHAPES
    for kind, m, n, count in shapes:
        if a.device_leg_only:
            run(kind, m, n, count, a.repeats, a.seed, device_only=True)
            continue
        line = run(kind, m, n, count, a.repeats, a.seed)
        if a.kernel_trace:
            ks = kernel_seconds((kind, m, n, count), a.seed)
            k = statistics.median(ks[:3])
            line.update(kernel_cost_us=statistics.median(ks[3:6]) * 1e6, kernel_rhs_us=statistics.median(ks[6:]) * 1e6)
            nbytes = count * (m * line["nact"] + m * m + (n + m + 1)) * 8
            line.update(kernel_us=k * 1e6, kernel_bytes=nbytes, kernel_gbs=nbytes / k / 1e9,
                        kernel_fraction_of_copy_ceiling=nbytes / k / COPY_CEILING)
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
