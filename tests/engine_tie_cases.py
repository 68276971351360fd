"""The tie, tolerance-boundary and non-finite cases of tests/tie_cases.py on the
single-LP engine (tests/test_engine_tie_cases.py on the CPU,
tests/test_gpu_engine_ties.py on the device).

tests/tie_cases.py builds interval LPs on which every operation is exact and
most pivots tie; here they run through lpg.Engine on every pivot path it has,
so that the tie-breaking arms of the engine's decision code (rec_min /
key_less and the tied-key fetch of k_pivot_block, the second stage of
k_prep_d / k_select_d, of the generic pair and of the eager kernels,
dual_cand / ratio_cand of the dual, the exchange of the ranks' candidates)
decide pivots under test. A case is a tie_cases spec of two LPs (B = 2, seeds
seed and seed + 1); a path is an environment around lpg.Engine(...) plus what
e.info must then report, so a path that silently falls back fails.

The geometry the census needs is restated here, not read from the engine:

- the deferred pair (k_prep_d / k_select_d, lpg_kernels.hip): one row per
  thread and two physical columns per thread of a 256-thread workgroup, i.e.
  row blocks of 256 and column blocks of 512 (column 0 included);
- a forced split of k_pivot_block (LPG_PERSIST_WG=w, block_geometry of
  lpg_block.hip): ceil(m / w) rows and ceil(ncp / w) columns per slice, ncp the
  column count rounded up to even; region mode slices the nonbasic columns of
  the block start instead (block_geometry_region), which move with the column
  trade, so the census counts the all-column slices only;
- rank r of a row partition holds rows m * r // world .. m * (r + 1) // world - 1
  (lpg_create_dist).

info_checks() cross-checks these against e.info.
"""
from __future__ import annotations

import contextlib
import json
import os
import pickle
import tempfile
import threading

import numpy as np

import batch_cases as bc
import tie_cases as tc

SEED = tc.SEED
LARGE, SMALL = (300, 600), (70, 150)
D_ROWS, D_COLS = 256, 512                # k_select_d: a row per thread; k_prep_d: two columns per thread; 256 threads
SPLIT_WG = 7
BLOCK = {LARGE: 32, SMALL: 8}
TWO_BANK_BLOCK = 80                      # 65 .. 96 pending pivots: the second lane bank
DUAL_BLOCK = {LARGE: 8, SMALL: 4}        # the dual's logs are short: 17 and 30 pivots at LARGE, 9 and 14 at SMALL
DUAL_WIDE_BLOCK = 128
WORLDS = (2, 3)
LDS_CAP = 150 * 1024

# seeds other than SEED, where a case misses a floor or a log is too short under SEED
CASE_SEED = {}


def case(m, n, method, rule):
    return tc.spec(m, n, method, rule, B=2, seed=CASE_SEED.get((m, n, method, rule), SEED))


def cases(shape=None):
    return [case(m, n, method, rule) for m, n in (LARGE, SMALL) if shape in (None, (m, n)) for method, rule in tc.METHODS]


def case_id(s):
    return tc.case_id(s)


# ---------------------------------------------------------------------------
# geometry, restated
# ---------------------------------------------------------------------------
def ncols_of(s):
    return s["n"] + s["m"] + 1


def slot_stride(block):
    return ((block + 15) & ~15) + 2


def slice_widths(m, ncols, wg):
    """(rows, columns) per slice of the all-column form: block_geometry (lpg_block.hip)."""
    ncp = (ncols + 1) & ~1
    return -(-m // wg), -(-ncp // wg)


def fits_all_column(m, ncols, block, wg):
    """block_geometry's rule, as tests/test_gpu_block.py::_fits."""
    rw, cw = slice_widths(m, ncols, wg)
    return cw <= 256 and rw <= 256 and slot_stride(block) * (cw + rw) * 8 <= LDS_CAP


def fits_region(m, n, block, wg):
    """block_geometry_region's rule, as tests/test_gpu_region.py::_fits."""
    cw, rw, nsp = -(-n // wg), -(-m // wg), -(-block // wg)
    x = cw + nsp + 1
    return x <= 256 and rw <= 256 and (x + rw) * slot_stride(block) * 8 <= LDS_CAP


def rank_rows(m, world):
    return [m * r // world for r in range(world + 1)]


def bounds_of(s):
    """The boundaries that matter for case s, per class of tie_cases.census: rows for the ratio test (the dual: the
    leaving row, "price"), physical columns for pricing (the dual: the entering column, "ratio")."""
    m, nc = s["m"], ncols_of(s)
    rw, cw = slice_widths(m, nc, SPLIT_WG)
    rows, cols = {"slice": rw}, {"slice": cw}
    if m > D_ROWS:
        rows["d"] = D_ROWS
    if nc > D_COLS:
        cols["d"] = D_COLS
    if (m, s["n"]) == SMALL:
        for w in WORLDS:
            rows[f"rank{w}"] = rank_rows(m, w)[1:-1]
    r, c = ("price", "ratio") if s["method"] == "dual" else ("ratio", "price")
    return {r: rows, c: cols}


def floors_of(s):
    """The census keys of bounds_of(s) that must reach 3, summed over the case's LPs. Pricing under Bland takes the
    first eligible column and has no ties (tie_cases.floors_of's rule)."""
    b = bounds_of(s)
    return [k for k in tc.bounds_keys(b) if not (s["rule"] == tc.RULE_BLAND and k.startswith("price") and s["method"] != "dual")]


# ---------------------------------------------------------------------------
# paths: an environment around lpg.Engine(...), and what e.info must report
# ---------------------------------------------------------------------------
PRIMAL_PATHS = {
    "persistent": {"LPG_NO_REORDER": "1"},
    "region": {"LPG_NO_REORDER": "0"},
    "split": {"LPG_NO_REORDER": "1", "LPG_PERSIST_WG": str(SPLIT_WG)},
    "split-region": {"LPG_NO_REORDER": "0", "LPG_PERSIST_WG": str(SPLIT_WG)},
    "pair": {"LPG_PERSIST": "0"},
    "generic": {"LPG_SLOW_PIVOT": "1"},
    "eager": {"LPG_DEFER": "0"},
}
DUAL_PATHS = {"dual-eager": {"LPG_DEFER": "0"}, "dual-deferred": {}, "dual-wide": {}}


def paths_of(s):
    return list(DUAL_PATHS if s["method"] == "dual" else PRIMAL_PATHS)


def block_of(s, path):
    """The block size (LPG_DEFER) of case s on a path; 0: eager."""
    if path in ("eager", "dual-eager"):
        return 0
    if path == "dual-wide":
        return DUAL_WIDE_BLOCK
    return (DUAL_BLOCK if s["method"] == "dual" else BLOCK)[(s["m"], s["n"])]


def two_bank_cases():
    """The cases whose logs cover two blocks of TWO_BANK_BLOCK pivots (tests/test_engine_tie_cases.py checks)."""
    return [case(*LARGE, method, tc.RULE_BLAND) for method in ("two_phase", "big_m")]


def env_of(s, path, block=None):
    env = dict({**PRIMAL_PATHS, **DUAL_PATHS}[path])
    block = block_of(s, path) if block is None else block
    env.setdefault("LPG_DEFER", str(block))
    return env


@contextlib.contextmanager
def environment(env):
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def info_checks(s, path, block, info):
    """What e.info must show on a path (a fallback to another path fails here), and the restated geometry."""
    m, nc, big = s["m"], ncols_of(s), s["method"] == "big_m"
    assert info.defer_k == block, (path, info.defer_k, block)
    assert info.nobj == tc.nobj_of(s) and (info.row0, info.nrows) == (0, m)
    if path in ("persistent", "split"):
        assert info.pivot_wg > 0 and info.region == 0, (path, info.pivot_wg, info.region)
    if path in ("region", "split-region"):
        assert info.pivot_wg > 0 and info.region == (0 if big else 1), (path, info.pivot_wg, info.region)
        assert info.column_trade == 1
    if path in ("split", "split-region"):
        assert fits_all_column(m, nc, block, SPLIT_WG) and (big or fits_region(m, s["n"], block, SPLIT_WG))
        assert info.pivot_wg == SPLIT_WG
    if path in ("pair", "generic", "eager", "dual-eager"):
        assert info.pivot_wg == 0, (path, info.pivot_wg)


# ---------------------------------------------------------------------------
# one LP on one engine; results in batch_cases' form, a batch of one
# ---------------------------------------------------------------------------
def _pack(e, res, calls, m, nobj, rows=None):
    k, r = e.get_log()
    return {
        "status": np.array([res.status], dtype=np.int64), "pivots": np.array([res.pivots], dtype=np.int64),
        "objective": np.array([res.objective]), "entering": np.array([res.entering], dtype=np.int64),
        "leaving": np.array([res.leaving], dtype=np.int64),
        "rows": (e.get_rows(0, m + nobj) if rows is None else rows)[None], "basis": e.get_basis()[None],
        "loglen": np.array([len(k)], dtype=np.int64), "logk": k, "logr": r,
        "calls": np.array([[c] for c in calls], dtype=np.int64),
    }


def lp_of(want, q):
    """LP q of a tie_cases.run_oracle result, as a batch of one."""
    lo = int(want["loglen"][:q].sum())
    n = int(want["loglen"][q])
    out = {k: np.asarray(want[k])[q:q + 1] for k in ("status", "pivots", "objective", "entering", "leaving", "rows", "basis",
                                                     "loglen")}
    out.update(logk=want["logk"][lo:lo + n], logr=want["logr"][lo:lo + n], calls=want["calls"][:, q:q + 1],
               logcap=want["logcap"])
    return out


NO_SKIP = {"LPG_NO_SKIP": "1"}            # update every column: no skipping of the columns whose P entry is zero


def assert_same(got, want, nonfinite=False, rows="bits"):
    """One LP against the oracle: the status after every call, status, pivot count, basis and the whole log, and the
    objective and all m + nobj rows by their bits. nonfinite: where the oracle's entry is a NaN the device's must be
    one, its sign and payload left out (tie_cases.assert_same_nonfinite's rule). rows "value": the rows by value
    (-0 == +0) instead of by bits; None: the rows not at all (neither is used by the tests: they show what differs)."""
    for key in ("calls", "status", "pivots", "basis", "loglen", "logk", "logr"):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    for key in ("objective", "rows") if rows else ("objective",):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        nan = np.isnan(w) if nonfinite else np.zeros(w.shape, dtype=bool)
        assert np.array_equal(np.isnan(g), nan), (key, "NaN-ness differs first at", np.argwhere(np.isnan(g) != nan)[0].tolist())
        differs = (g != w) if key == "rows" and rows == "value" else (bc.bits(g) != bc.bits(w))
        diff = np.argwhere(differs & ~nan)
        assert diff.size == 0, (key, "differs first at", diff[0].tolist(), g[tuple(diff[0])], w[tuple(diff[0])],
                                f"{len(diff)} entries differ, {int((differs & ~nan & (g == w)).sum())} of them in the sign of a zero")


def method_call(x, s, art_first, cost=None):
    """budget -> one call of case s's method on x, an lpg.Engine or an Oracle (their signatures agree). cost: the
    costs of two-phase and Big-M; None takes -1 x the objective row as it stands, which is the LP's own only in
    front of the first pivot, so a run continued by further calls passes them."""
    if s["method"] == "primal":
        return lambda budget: x.solve(budget, s["rule"])
    if s["method"] == "dual":
        return lambda budget: x.solve_dual(budget)
    if s["method"] == "two_phase":
        return lambda budget: x.solve_two_phase(art_first, cost, budget, s["rule"])
    return lambda budget: x.solve_big_m(art_first, cost, budget, s["rule"])


def costs_of(T):
    return -T[-1, 1:].copy()


def solve_lp(T, basis, s, env, budgets, path=None, block=None, eps=None, pieces=None, cost=None):
    """LP (T, basis) of case s through one lpg.Engine made under `env`. budgets: one call of the method each.
    pieces: the primal in lpg_enqueue pieces (ints; "b": a get_column0 in between, which flushes inside a block)
    in front of the budgets. Returns (result as a batch of one, info after the solve)."""
    import linearprogramming_amd as lpg
    m = basis.shape[0]
    n = T.shape[1] - m - 1
    nobj = tc.nobj_of(s)
    with environment(env):
        e = lpg.Engine(m, T.shape[1], flags=lpg._lib.FLAG_BIG_M if nobj == 2 else 0)
    try:
        if path is not None:
            info_checks(s, path, block, e.info)
        e.load_rows(0, T)
        e.set_basis(basis)
        if eps is not None:
            e.set_tolerances(*eps)
        if pieces:
            e.reserve_log(4096)
            for p in pieces:
                if p == "b":
                    e.get_column0()
                else:
                    e.enqueue(p, s["rule"])
            e.sync()
        solve, calls = method_call(e, s, tc.art_first_of(m, n), cost), []
        for budget in budgets:
            res = solve(budget)
            calls.append(res.status)
        info = e.info
        assert info.residency_fallbacks == 0, "the persistent launch fell back to the pair"
        return _pack(e, res, calls, m, nobj), info
    finally:
        e.close()


def run_single(s, q, path, block=None, budgets=None, pieces=None, explicit_costs=False, extra_env=None):
    """LP q of interval case s on a single-rank path; the block size is block_of(s, path) unless given."""
    block = block_of(s, path) if block is None else block
    T, basis = tc.build_lp(s, q)
    return solve_lp(T, basis, s, {**env_of(s, path, block), **(extra_env or {})}, budgets or s["budgets"], path, block,
                    s["eps"], pieces,
                    costs_of(T) if explicit_costs else None)


# ---------------------------------------------------------------------------
# the row partition: ranks as threads over the host collectives
# ---------------------------------------------------------------------------
def _rank_result(e, res, m, nobj):
    info = e.info
    return dict(status=res.status, pivots=res.pivots, objective=res.objective, log=e.get_log(), basis=e.get_basis(),
                rows=e.get_rows(info.row0, info.nrows), obj=e.get_rows(m, nobj), row0=info.row0, nrows=info.nrows,
                wg=info.pivot_wg, region=info.region, defer_k=info.defer_k)


def run_threads(T, basis, s, world, block, budget=20000, extra_env=None):
    """Every rank a thread with the whole tableau and basis loaded, the exchange through an in-process transport
    (tests/test_gpu_dist.py's ThreadComm, which checks that every allreduce is a broadcast in disguise)."""
    import linearprogramming_amd as lpg
    from test_gpu_dist import ThreadComm
    m = basis.shape[0]
    n, nobj = T.shape[1] - m - 1, tc.nobj_of(s)
    comm, out, errs = ThreadComm(world), [None] * world, []

    def worker(rank):
        try:
            e = lpg.Engine(m, T.shape[1], world=world, rank=rank, flags=lpg._lib.FLAG_BIG_M if nobj == 2 else 0)
            e.comm_init_host(lambda b: comm.allgather(rank, b), lambda a: comm.allreduce(rank, a))
            e.load_rows(0, T)
            e.set_basis(basis)
            res = tc._solve_fn(e, s, tc.art_first_of(m, n))(budget)
            out[rank] = _rank_result(e, res, m, nobj)
            e.close()
        except Exception as ex:   # pragma: no cover
            errs.append(ex)
            comm.bar.abort()

    with environment({"LPG_DEFER": str(block), **(extra_env or {})}):
        th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(600)
    assert not comm.violations, comm.violations[:4]
    assert not errs, errs
    return out


def assert_ranks_same(parts, want, m, world, block, nonfinite=False, rows="bits"):
    """Every rank's status, pivot count, objective, log and basis, the replicated objective rows and the stacked row
    blocks against LP `want` (a batch of one), bit for bit; the row ranges against rank_rows. nonfinite and rows as
    assert_same's."""
    edges = rank_rows(m, world)
    W = want["rows"][0]

    def same(a, b, how="bits"):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        nan = np.isnan(b) if nonfinite else np.zeros(b.shape, dtype=bool)
        eq = (a == b) if how == "value" else (bc.bits(a) == bc.bits(b))
        bad = np.argwhere((np.isnan(a) != nan) | ~(eq | nan))
        if bad.size:
            print(f"differs first at {bad[0].tolist()}: {a[tuple(bad[0])]!r} for {b[tuple(bad[0])]!r}, {len(bad)} entries")
        return not bad.size

    for r, p in enumerate(parts):
        assert (p["row0"], p["nrows"]) == (edges[r], edges[r + 1] - edges[r]) and p["defer_k"] == block
        assert (p["status"], p["pivots"]) == (int(want["status"][0]), int(want["pivots"][0])), (r, p["status"], p["pivots"])
        assert same([p["objective"]], want["objective"])
        assert np.array_equal(p["log"][0], want["logk"]) and np.array_equal(p["log"][1], want["logr"]), f"rank {r}: log"
        assert np.array_equal(p["basis"], want["basis"][0]), f"rank {r}: basis"
        assert not rows or same(p["obj"], W[m:], rows), f"rank {r}: objective rows"
    assert not rows or same(np.vstack([p["rows"] for p in parts]), W[:m], rows), "stacked row blocks"


# ---------------------------------------------------------------------------
# the row partition: separate processes with the owner push
# ---------------------------------------------------------------------------
# (method, rule, world, LPG_PERSIST_MR)
PUSH_CASES = [("primal", 0, 2, None), ("primal", 0, 2, "0"), ("primal", 1, 2, None), ("primal", 1, 2, "0"),
              ("big_m", 0, 2, None), ("big_m", 0, 2, "0"), ("dual", 0, 3, None), ("two_phase", 1, 3, None)]


def push_worker(rank, world, init, spec_json, q, block, mr, outdir, extra_env=None):
    """One rank of an owner-push run (after tests/test_gpu_dist.py::_gloo_worker): gloo for the setup collectives,
    IPC-mapped exchange buffers for the pivots."""
    os.environ["LPG_DEFER"] = str(block)
    os.environ["LPG_PUSH_SHARED_QUEUES"] = os.environ["LPG_PUSH_SHARED_DEVICE"] = "1"   # the ranks share one GPU here
    if mr is not None:
        os.environ["LPG_PERSIST_MR"] = mr
    os.environ.update(extra_env or {})
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    import linearprogramming_amd as lpg

    def allgather(b: bytes) -> bytes:
        t = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        outs = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(outs, t)
        return b"".join(bytes(o.numpy()) for o in outs)

    def allreduce(a: np.ndarray) -> np.ndarray:
        t = torch.from_numpy(a)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.numpy()

    s = json.loads(spec_json)
    T, basis = tc.build_lp(s, q)
    m = basis.shape[0]
    n, nobj = T.shape[1] - m - 1, tc.nobj_of(s)
    e = lpg.Engine(m, T.shape[1], world=world, rank=rank, flags=lpg._lib.FLAG_BIG_M if nobj == 2 else 0)
    e.comm_init_host(allgather, allreduce)
    h = allgather(e.push_handle())
    e.comm_init_push([h[64 * r:64 * r + 64] for r in range(world)])
    e.load_rows(0, T)
    e.set_basis(basis)
    res = tc._solve_fn(e, s, tc.art_first_of(m, n))(s["budgets"][0])
    out = _rank_result(e, res, m, nobj)
    out["exchange"] = e.info.exchange
    with open(os.path.join(outdir, f"r{rank}.pkl"), "wb") as f:
        pickle.dump(out, f)
    e.close()
    dist.destroy_process_group()


def run_processes(s, q, world, block, mr, extra_env=None):
    from util import spawn_ranks
    with tempfile.TemporaryDirectory() as d:
        spawn_ranks(push_worker, lambda init: (world, init, json.dumps(s), q, block, mr, d, extra_env), world)
        return [pickle.load(open(os.path.join(d, f"r{r}.pkl"), "rb")) for r in range(world)]


# ---------------------------------------------------------------------------
# non-finite entries
# ---------------------------------------------------------------------------
def nan_ratio_across_ranks():
    """tie_cases.nan_ratio_lp at (70, 20) with the NaN row (1) in rank 0 and the best row (40) in rank 1 of a
    partition over two ranks (rows 0 .. 34 and 35 .. 69). Returns (T, basis, case spec)."""
    m, n = 70, 20
    T, basis = tc.nonfinite_batch("nan_ratio")
    assert rank_rows(m, 2) == [0, 35, 70]
    return tc.nan_ratio_lp(T[0], m, n, nan_row=1, best_row=40), basis[0], tc.spec(m, n, "primal", 0, B=1, budgets=[1000])


def dual_nan_ratio_across_column_blocks():
    """tie_cases' dual_nan_ratio_stride widened to n = 700: row 0 leaves, column 2's ratio +inf / +inf is NaN and
    column 600, in the second column block of D_COLS, holds the least. Returns (T, basis, case spec)."""
    from oracle.lpo import GEN_DUAL, Oracle
    m, n = 12, 700
    o = Oracle(m, n + m + 1)
    o.generate(n, bc.SEED, GEN_DUAL)
    T, basis = o.get_rows(), o.get_basis()
    o.close()
    T[:m, 0] = -1.0
    T[0, 0] = -2.0
    T[0, 1:n + 1] = -1.0
    T[m, 1:n + 1] = 2.0 + np.arange(n)
    T[m, 600] = 0.5
    T[0, 2], T[m, 2] = -np.inf, np.inf
    assert 2 // D_COLS != 600 // D_COLS
    return T, basis, tc.spec(m, n, "dual", 0, B=1, budgets=[5])


def oracle_lp(T, basis, s, eps=None, cost=None):
    """One loaded LP through the oracle, one call per budget of s, as a batch of one."""
    m = basis.shape[0]

    def prepare(o):
        if eps is not None:
            o.set_tolerances(*eps)
    return bc.oracle_loop(T[None], basis[None], s["budgets"],
                          lambda o, b, budget: method_call(o, s, tc.art_first_of(m, T.shape[1] - m - 1), cost)(budget), 4096,
                          prepare, nobj=tc.nobj_of(s))


RESUME_BUDGETS = [5, 14, 31, 64, 20000]
_RESUMED = {}


def oracle_resumed(s, q):
    """LP q of case s through the oracle in calls of RESUME_BUDGETS, the costs passed to every call (computed once)."""
    key = json.dumps([s, q], sort_keys=True)
    if key not in _RESUMED:
        T, basis = tc.build_lp(s, q)
        _RESUMED[key] = oracle_lp(T, basis, dict(s, budgets=RESUME_BUDGETS), cost=costs_of(T))
    return _RESUMED[key]
