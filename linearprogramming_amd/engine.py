"""Python handle on one lpg context (include/lpg.h) — test and bench plumbing.

The product is the C-ABI library; this class only marshals numpy arrays and
turns negative return codes into exceptions carrying lpg_last_error(), the way
the reference turns ``valid == 0`` into an ``ERROR: ...`` line.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import _lib as L


class LPGError(RuntimeError):
    pass


class _HasStatus:
    @property
    def status_name(self) -> str:
        return L.STATUS_NAMES.get(self.status, str(self.status))


@dataclass
class SolveResult(_HasStatus):
    status: int
    pivots: int
    objective: float
    entering: int
    leaving: int
    rule: int


@dataclass
class Ranging:
    """What BatchEngine.ranging returns (include/lpg.h, "ranging"): per LP the dual values [m], the cost ranges
    [ncols - 1] and the right-hand-side ranges [m], each range as its two ends and the index that limits each (a
    column, 0 = none; a row, -1 = none). A batch of one shape gives 2-D arrays, a ragged one a list of arrays per
    LP; a group that was not asked for is None. An LP that is not OPTIMAL has NaN and none everywhere."""
    dual: object = None
    cost_lo: object = None
    cost_hi: object = None
    cost_lo_at: object = None
    cost_hi_at: object = None
    rhs_lo: object = None
    rhs_hi: object = None
    rhs_lo_at: object = None
    rhs_hi_at: object = None


RANGING_FIELDS = ("dual", "cost_lo", "cost_hi", "cost_lo_at", "cost_hi_at", "rhs_lo", "rhs_hi", "rhs_lo_at", "rhs_hi_at")


def _res(r: L.Result) -> SolveResult:
    return SolveResult(r.status, r.pivots, r.objective, r.entering, r.leaving, r.rule)


@contextlib.contextmanager
def _stdout_to_stderr():
    """RCCL prints a version banner on the process's stdout at init; keep
    stdout for results (bench.py's one JSON line) by pointing fd 1 at fd 2."""
    sys.stdout.flush()
    saved = os.dup(1)
    try:
        os.dup2(2, 1)
        yield
    finally:
        ctypes.CDLL(None).fflush(None)      # C stdio buffers go out through the redirected fd
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


def flush_kernel_for(pending: int) -> str:
    """Which block-pass kernel the default configuration launches for `pending`
    pivots (lpg_kernels.hip launch_flush_main): k_flushw at every block size
    ("m" = k_flushm only when LPG_FLUSH_KERNEL=m asks for it, <= 32 slots)."""
    return "w"


def device_count() -> int:
    lib = L.load()
    n = ctypes.c_int(0)
    lib.lpg_device_count(ctypes.byref(n))
    return n.value


class _Handle:
    """What every handle on a library object shares. A subclass names the C prefix of its calls (``lpg_assign``:
    lpg_assign_destroy, lpg_assign_last_error, lpg_assign_info) and its info struct; the handle itself is ``_h``."""

    _prefix = None
    _info_type = None
    _h = None

    def _open(self, lib, handle=None):
        """The library, and the handle: null until _create fills it, or one the library already made."""
        self.lib = lib if lib is not None else L.load()
        self._h = ctypes.c_void_p() if handle is None else handle

    def _call(self, suffix):
        return getattr(self.lib, f"{self._prefix}_{suffix}")

    def _create(self, name, *args):
        rc = getattr(self.lib, name)(ctypes.byref(self._h), *args)
        if rc != 0:
            raise LPGError(f"{name} rc={rc}: {self._call('last_error')(None).decode()}")

    def close(self):
        if self._h:
            self._call("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise LPGError(f"{what} rc={rc}: {self._call('last_error')(self._h).decode()}")
        return rc

    @property
    def info(self):
        i = self._info_type()
        self._check(self._call("info")(self._h, ctypes.byref(i)), f"{self._prefix}_info")
        return i


class Engine(_Handle):
    """One rank's engine for an m x ncols (= N+1) tableau."""

    _prefix, _info_type = "lpg", L.Info

    def __init__(self, m: int, ncols: int, device: int = 0, world: int = 1, rank: int = 0, flags: int = 0,
                 lib=None):
        self._open(lib)
        self._create("lpg_create_dist", device, world, rank, m, ncols, flags)
        self.m, self.ncols, self.world, self.rank = m, ncols, world, rank
        self.nobj = 2 if flags & L.FLAG_BIG_M else 1
        self._keep = []   # ctypes callbacks kept alive

    # -- communication ---------------------------------------------------
    def comm_init_rccl(self, uid: bytes):
        buf = ctypes.create_string_buffer(bytes(uid), len(uid))
        with _stdout_to_stderr():
            rc = self.lib.lpg_comm_init_rccl(self._h, buf, len(uid))
        self._check(rc, "lpg_comm_init_rccl")

    @staticmethod
    def rccl_unique_id() -> bytes:
        lib = L.load()
        buf = ctypes.create_string_buffer(128)
        with _stdout_to_stderr():
            rc = lib.lpg_comm_unique_id(buf, 128)
        if rc != 0:
            raise LPGError(f"lpg_comm_unique_id rc={rc}: {lib.lpg_last_error(None).decode()}")
        return buf.raw

    def comm_init_host(self, allgather, allreduce_sum):
        """allgather(send: bytes) -> bytes (world * len); allreduce_sum(np.ndarray f64) -> np.ndarray."""
        world = self.world

        def _ag(user, send, recv, nbytes):
            try:
                data = ctypes.string_at(send, nbytes)
                out = allgather(data)
                assert len(out) == nbytes * world
                ctypes.memmove(recv, out, len(out))
                return 0
            except Exception:   # pragma: no cover - reported as LPG_ERR_COMM
                return -1

        def _ar(user, buf, count):
            try:
                arr = np.ctypeslib.as_array(buf, shape=(count,))
                arr[:] = allreduce_sum(arr.copy())
                return 0
            except Exception:   # pragma: no cover
                return -1

        ops = L.HostCommOps(None, L.ALLGATHER_FN(_ag), L.ALLREDUCE_FN(_ar))
        self._keep += [ops, _ag, _ar]
        self._check(self.lib.lpg_comm_init_host(self._h, ctypes.byref(ops)), "lpg_comm_init_host")

    # owner-push exchange (include/lpg.h): after a communicator
    def push_handle(self) -> bytes:
        buf = ctypes.create_string_buffer(64)
        self._check(self.lib.lpg_comm_push_handle(self._h, buf, 64), "lpg_comm_push_handle")
        return buf.raw

    def push_base(self) -> int:
        p = ctypes.c_void_p()
        self._check(self.lib.lpg_comm_push_base(self._h, ctypes.byref(p)), "lpg_comm_push_base")
        return p.value

    def comm_init_push(self, handles):
        """handles: every rank's push_handle(), in rank order."""
        blob = b"".join(bytes(h) for h in handles)
        buf = ctypes.create_string_buffer(blob, len(blob))
        self._check(self.lib.lpg_comm_init_push(self._h, buf, len(blob)), "lpg_comm_init_push")

    def comm_init_push_local(self, bases):
        """bases: every rank's push_base() (ranks of one process), in rank order."""
        arr = (ctypes.c_void_p * len(bases))(*bases)
        self._check(self.lib.lpg_comm_init_push_local(self._h, arr, len(bases)), "lpg_comm_init_push_local")

    # -- loading ---------------------------------------------------------
    def load_rows(self, row0: int, rows: np.ndarray):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        self._check(self.lib.lpg_load_rows(self._h, row0, rows.shape[0],
                                           rows.ctypes.data_as(L.c_double_p), rows.shape[1]), "lpg_load_rows")

    def load_tableau(self, T: np.ndarray, basis=None):
        """T: (m+1) x ncols full tableau (objective row last)."""
        self.load_rows(0, T)
        if basis is not None:
            self.set_basis(basis)

    def set_basis(self, basis):
        b = np.ascontiguousarray(basis, dtype=np.int64)
        self._check(self.lib.lpg_set_basis(self._h, b.ctypes.data_as(L.c_int64_p)), "lpg_set_basis")

    def set_objective(self, c):
        c = np.ascontiguousarray(c, dtype=np.float64)
        self._check(self.lib.lpg_set_objective(self._h, c.ctypes.data_as(L.c_double_p)), "lpg_set_objective")

    def set_tolerances(self, eps_piv=1e-9, eps_opt=1e-9):
        self._check(self.lib.lpg_set_tolerances(self._h, eps_piv, eps_opt), "lpg_set_tolerances")

    def set_active_columns(self, nact: int):
        self._check(self.lib.lpg_set_active_columns(self._h, nact), "lpg_set_active_columns")

    def generate(self, n: int, seed: int = 20220518, kind: int = L.GEN_DENSE):
        self._check(self.lib.lpg_generate(self._h, n, seed, kind), "lpg_generate")

    # -- pivoting --------------------------------------------------------
    def solve(self, max_pivots: int = 1 << 40, rule: int = L.RULE_DANTZIG) -> SolveResult:
        r = L.Result()
        self._check(self.lib.lpg_solve(self._h, max_pivots, rule, ctypes.byref(r)), "lpg_solve")
        return _res(r)

    def enqueue(self, npivots: int, rule: int = L.RULE_DANTZIG):
        self._check(self.lib.lpg_enqueue(self._h, npivots, rule), "lpg_enqueue")

    def sync(self) -> SolveResult:
        r = L.Result()
        self._check(self.lib.lpg_sync(self._h, ctypes.byref(r)), "lpg_sync")
        return _res(r)

    def pivot(self, k: int, r: int):
        self._check(self.lib.lpg_pivot(self._h, k, r), "lpg_pivot")

    def solve_two_phase(self, art_first: int, cost=None, max_pivots: int = 1 << 40, rule: int = L.RULE_DANTZIG):
        cp = None if cost is None else np.ascontiguousarray(cost, dtype=np.float64).ctypes.data_as(L.c_double_p)
        r = L.Result()
        self._check(self.lib.lpg_solve_two_phase(self._h, art_first, cp, max_pivots, rule, ctypes.byref(r)),
                    "lpg_solve_two_phase")
        return _res(r)

    def set_objective_m(self, cM):
        c = np.ascontiguousarray(cM, dtype=np.float64)
        self._check(self.lib.lpg_set_objective_m(self._h, c.ctypes.data_as(L.c_double_p)), "lpg_set_objective_m")

    def solve_big_m(self, art_first: int, cost=None, max_pivots: int = 1 << 40, rule: int = L.RULE_DANTZIG):
        cp = None if cost is None else np.ascontiguousarray(cost, dtype=np.float64).ctypes.data_as(L.c_double_p)
        r = L.Result()
        self._check(self.lib.lpg_solve_big_m(self._h, art_first, cp, max_pivots, rule, ctypes.byref(r)),
                    "lpg_solve_big_m")
        return _res(r)

    def solve_dual(self, max_pivots: int = 1 << 40) -> SolveResult:
        r = L.Result()
        self._check(self.lib.lpg_solve_dual(self._h, max_pivots, ctypes.byref(r)), "lpg_solve_dual")
        return _res(r)

    def reserve_log(self, n: int):
        self._check(self.lib.lpg_reserve_log(self._h, n), "lpg_reserve_log")

    def prepare(self, rule: int = L.RULE_DANTZIG):
        """Build the replayed pivot graph now (no pivots run; include/lpg.h lpg_prepare)."""
        self._check(self.lib.lpg_prepare(self._h, rule), "lpg_prepare")

    def device_sync(self):
        self._check(self.lib.lpg_device_sync(self._h), "lpg_device_sync")

    # -- readout ---------------------------------------------------------
    def get_rows(self, row0: int, nrows: int) -> np.ndarray:
        out = np.zeros((nrows, self.ncols), dtype=np.float64)
        self._check(self.lib.lpg_get_rows(self._h, row0, nrows, out.ctypes.data_as(L.c_double_p), self.ncols),
                    "lpg_get_rows")
        return out

    def get_basis(self) -> np.ndarray:
        out = np.zeros(self.m, dtype=np.int64)
        self._check(self.lib.lpg_get_basis(self._h, out.ctypes.data_as(L.c_int64_p)), "lpg_get_basis")
        return out

    def get_column0(self) -> np.ndarray:
        out = np.zeros(self.info.nrows, dtype=np.float64)
        self._check(self.lib.lpg_get_column0(self._h, out.ctypes.data_as(L.c_double_p)), "lpg_get_column0")
        return out

    def get_log(self):
        n = self._check(self.lib.lpg_get_log(self._h, None, None, 0), "lpg_get_log")
        k = np.zeros(max(n, 1), dtype=np.int64)
        r = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self.lib.lpg_get_log(self._h, k.ctypes.data_as(L.c_int64_p), r.ctypes.data_as(L.c_int64_p), n),
                    "lpg_get_log")
        return k[:n], r[:n]

    # -- timing ----------------------------------------------------------
    def set_timing(self, enable: bool):
        self._check(self.lib.lpg_set_timing(self._h, int(enable)), "lpg_set_timing")

    def get_timing(self) -> L.Timing:
        t = L.Timing()
        self._check(self.lib.lpg_get_timing(self._h, ctypes.byref(t)), "lpg_get_timing")
        return t


class BatchEngine(_Handle):
    """`count` LPs of one shape, each an (m+1) x ncols tableau, solved in one
    launch with one workgroup per LP (include/lpg.h, "batches"). ``big_m=True``:
    a Big-M batch, (m+2) x ncols tableaus (row m the M part, row m + 1 the real
    part of the objective), solved by solve_big_m only. ``levels=K``: a goal
    batch, (m+K) x ncols tableaus (row m + k the objective row of priority level
    k, level 0 the highest), solved by solve_goal only.

    ``BatchEngine.ragged(shapes)`` makes a ragged batch instead: LP q has its own
    (m, ncols) = shapes[q], and the solve calls still run all of them in one
    round of launches, every LP bit for bit what it computes alone. Its methods
    take and return one array per LP (RaggedBatchEngine)."""

    _prefix, _info_type = "lpg_batch", L.BatchInfo
    _b = property(lambda self: self._h)      # the tests call the library on the handle directly

    @staticmethod
    def ragged(shapes, device: int = 0, big_m: bool = False, flags: int = 0, lib=None) -> "RaggedBatchEngine":
        """A batch of len(shapes) LPs, LP q of shapes[q] = (m, ncols)."""
        return RaggedBatchEngine(shapes, device=device, big_m=big_m, flags=flags, lib=lib)

    def __init__(self, count: int, m: int, ncols: int, device: int = 0, flags: int = 0, lib=None, big_m: bool = False,
                 _handle=None, levels: int = None):
        """``_handle``: an lpg_batch of this shape that the library already made (branch()); the engine owns it."""
        self._open(lib, _handle)
        if levels is not None and big_m:
            raise LPGError("BatchEngine: big_m and levels exclude each other (a goal batch of 2 levels is no Big-M batch)")
        if _handle is None:
            if levels is not None:
                self._create("lpg_batch_create_goal", device, count, m, ncols, levels, flags)
            else:
                self._create("lpg_batch_create_big_m" if big_m else "lpg_batch_create", device, count, m, ncols, flags)
        self.count, self.m, self.ncols = count, m, ncols
        self.nobj = levels if levels is not None else (2 if big_m else 1)
        self.levels = levels

    # -- loading ---------------------------------------------------------
    def load(self, T: np.ndarray, basis=None, first: int = 0):
        """T: [n, m+1, ncols] tableaus (objective row last; Big-M batch: [n, m+2, ncols], M part then real part),
        basis: [n, m]; LPs first .. first + n - 1."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        if T.ndim != 3 or T.shape[1] != self.m + self.nobj or T.shape[2] != self.ncols:
            raise LPGError(f"load: tableaus of shape {T.shape}, want [n, {self.m + self.nobj}, {self.ncols}]")
        bp = None
        if basis is not None:
            basis = np.ascontiguousarray(basis, dtype=np.int64)
            if basis.shape != (T.shape[0], self.m):
                raise LPGError(f"load: basis of shape {basis.shape}, want [{T.shape[0]}, {self.m}]")
            bp = basis.ctypes.data_as(L.c_int64_p)
        self._check(self.lib.lpg_batch_load(self._h, first, T.shape[0], T.ctypes.data_as(L.c_double_p), self.ncols, bp),
                    "lpg_batch_load")

    def generate(self, n: int, seed: int = 20220518, kind: int = L.GEN_DENSE):
        """LP b = Engine.generate(n, seed + b, kind)."""
        self._check(self.lib.lpg_batch_generate(self._h, n, seed, kind), "lpg_batch_generate")

    def set_tolerances(self, eps_piv=1e-9, eps_opt=1e-9):
        self._check(self.lib.lpg_batch_set_tolerances(self._h, eps_piv, eps_opt), "lpg_batch_set_tolerances")

    def set_active_columns(self, nact: int):
        self._check(self.lib.lpg_batch_set_active_columns(self._h, nact), "lpg_batch_set_active_columns")

    def reserve_log(self, n: int):
        self._check(self.lib.lpg_batch_reserve_log(self._h, n), "lpg_batch_reserve_log")

    # -- pivoting --------------------------------------------------------
    def solve(self, max_pivots: int = 1 << 40, rule: int = L.RULE_DANTZIG) -> list:
        r = (L.Result * self.count)()
        self._check(self.lib.lpg_batch_solve(self._h, max_pivots, rule, r), "lpg_batch_solve")
        return [_res(x) for x in r]

    def solve_dual(self, max_pivots: int = 1 << 40) -> list:
        r = (L.Result * self.count)()
        self._check(self.lib.lpg_batch_solve_dual(self._h, max_pivots, r), "lpg_batch_solve_dual")
        return [_res(x) for x in r]

    def _costs(self, cost, what):
        """cost: [N] (the same for every LP) or [count, >= N] -> a C-contiguous array, its pointer and pitch."""
        c = np.asarray(cost, dtype=np.float64)
        if c.ndim == 1:
            c = np.tile(c, (self.count, 1))
        c = np.ascontiguousarray(c)
        if c.ndim != 2 or c.shape[0] != self.count:
            raise LPGError(f"{what}: costs of shape {c.shape}, want [{self.count}, >= {self.ncols - 1}]")
        return c, c.ctypes.data_as(L.c_double_p), c.shape[1]

    def solve_two_phase(self, art_first: int, cost=None, max_pivots: int = 1 << 40, rule: int = L.RULE_DANTZIG) -> list:
        """Engine.solve_two_phase on every LP in one launch; cost: None, [N] or [count, >= N]
        (the row pitch is the array's width). Afterwards columns 1..art_first-1 are active."""
        keep, cp, ld = (None, None, 0) if cost is None else self._costs(cost, "solve_two_phase")
        r = (L.Result * self.count)()
        self._check(self.lib.lpg_batch_solve_two_phase(self._h, art_first, cp, ld, max_pivots, rule, r),
                    "lpg_batch_solve_two_phase")
        del keep
        return [_res(x) for x in r]

    def solve_big_m(self, art_first: int, cost=None, max_pivots: int = 1 << 40, rule: int = L.RULE_DANTZIG) -> list:
        """Engine.solve_big_m on every LP of a Big-M batch in one launch; cost as solve_two_phase's.
        Another call goes on where a budget-limited one stopped."""
        keep, cp, ld = (None, None, 0) if cost is None else self._costs(cost, "solve_big_m")
        r = (L.Result * self.count)()
        self._check(self.lib.lpg_batch_solve_big_m(self._h, art_first, cp, ld, max_pivots, rule, r),
                    "lpg_batch_solve_big_m")
        del keep
        return [_res(x) for x in r]

    def solve_goal(self, costs, max_pivots: int = 1 << 40, rule: int = L.RULE_DANTZIG):
        """The preemptive goal programme of every LP of a goal batch in one launch (include/lpg.h, "goal
        programmes"). costs: [count, K, >= N] (or [K, >= N], the same for every LP), row k the costs of priority
        level k. Returns (results, attain[count, K]): attain[q, k] is column 0 of LP q's objective row of level k.
        Every call sets the K objective rows anew from the current basis and has a budget of its own."""
        K = self.nobj
        c = np.asarray(costs, dtype=np.float64)
        if c.ndim == 2:
            c = np.tile(c, (self.count, 1, 1))
        c = np.ascontiguousarray(c)
        if c.ndim != 3 or c.shape[0] != self.count or c.shape[1] != K:
            raise LPGError(f"solve_goal: costs of shape {c.shape}, want [{self.count}, {K}, >= {self.ncols - 1}]")
        r = (L.Result * self.count)()
        attain = np.zeros((self.count, K), dtype=np.float64)
        self._check(self.lib.lpg_batch_solve_goal(self._h, c.ctypes.data_as(L.c_double_p), K * c.shape[2], c.shape[2],
                                                  max_pivots, rule, r, attain.ctypes.data_as(L.c_double_p)),
                    "lpg_batch_solve_goal")
        return [_res(x) for x in r], attain

    def set_objective(self, cost):
        """Engine.set_objective on every LP; cost: [N] or [count, >= N]."""
        keep, cp, ld = self._costs(cost, "set_objective")
        self._check(self.lib.lpg_batch_set_objective(self._h, cp, ld), "lpg_batch_set_objective")
        del keep

    def generate_artificial(self, n: int, seed: int = 20220518) -> int:
        """LP b = Engine.generate(n, seed + b, GEN_ARTIFICIAL); returns art_first."""
        af = ctypes.c_int64(0)
        self._check(self.lib.lpg_batch_generate_artificial(self._h, n, seed, ctypes.byref(af)),
                    "lpg_batch_generate_artificial")
        return int(af.value)

    # -- readout ---------------------------------------------------------
    def get_rows(self, first: int = 0, n: int = None) -> np.ndarray:
        n = self.count - first if n is None else n
        out = np.zeros((n, self.m + self.nobj, self.ncols), dtype=np.float64)
        self._check(self.lib.lpg_batch_get_rows(self._h, first, n, out.ctypes.data_as(L.c_double_p), self.ncols),
                    "lpg_batch_get_rows")
        return out

    def get_basis(self, first: int = 0, n: int = None) -> np.ndarray:
        n = self.count - first if n is None else n
        out = np.zeros((n, self.m), dtype=np.int64)
        self._check(self.lib.lpg_batch_get_basis(self._h, first, n, out.ctypes.data_as(L.c_int64_p)),
                    "lpg_batch_get_basis")
        return out

    def get_log(self, lp: int):
        n = self._check(self.lib.lpg_batch_get_log(self._h, lp, None, None, 0), "lpg_batch_get_log")
        k = np.zeros(max(n, 1), dtype=np.int64)
        r = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self.lib.lpg_batch_get_log(self._h, lp, k.ctypes.data_as(L.c_int64_p),
                                               r.ctypes.data_as(L.c_int64_p), n), "lpg_batch_get_log")
        return k[:n], r[:n]

    # -- branching -------------------------------------------------------
    def active_columns(self, lp: int = 0):
        """(nact, art_first) of LP lp: its priced columns 1..nact, and a ragged batch's recorded art_first."""
        nact, af = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.lpg_batch_active_columns(self._h, lp, ctypes.byref(nact), ctypes.byref(af)),
                    "lpg_batch_active_columns")
        return int(nact.value), int(af.value)

    def branch_select(self, mask, int_tol: float = 1e-6, rule: int = L.BRANCH_MOST_FRACTIONAL):
        """The branching row of every LP (include/lpg.h lpg_batch_branch_select). mask: [nmask] (the same for
        every LP) or [count, nmask], non-zero where tableau column 1 + index is integer-constrained. Returns
        (row, col, value), one entry per LP; row = col = -1 where every integer column is integral."""
        mk, mp, nmask, ld = self._mask(mask, "branch_select")
        out = (L.Branch * self.count)()
        self._check(self.lib.lpg_batch_branch_select(self._h, mp, nmask, ld, int_tol, rule, out), "lpg_batch_branch_select")
        a = np.frombuffer(out, dtype=np.dtype([("row", np.int64), ("col", np.int64), ("value", np.float64)]))
        return a["row"].copy(), a["col"].copy(), a["value"].copy()

    def branch(self, src, row, dir):
        """A new batch of len(src) children made on the device (include/lpg.h lpg_batch_branch): child c is LP
        src[c] plus the bound x <= floor(v) (dir[c] = -1) or x >= ceil(v) (dir[c] = +1) on the variable basic in
        row[c]; solve_dual() re-optimises it. The engine returned is of this engine's class."""
        src = np.ascontiguousarray(src, dtype=np.int64)
        row = np.ascontiguousarray(row, dtype=np.int64)
        d = np.ascontiguousarray(dir, dtype=np.int8)
        if src.ndim != 1 or row.shape != src.shape or d.shape != src.shape:
            raise LPGError(f"branch: src, row, dir of shapes {src.shape}, {row.shape}, {d.shape}, want three [n]")
        child = ctypes.c_void_p()
        self._check(self.lib.lpg_batch_branch(ctypes.byref(child), self._h, src.shape[0], src.ctypes.data_as(L.c_int64_p),
                                              row.ctypes.data_as(L.c_int64_p), d.ctypes.data_as(L.c_int8_p)),
                    "lpg_batch_branch")
        return self._wrap_child(child, src, [1] * len(src))

    def _wrap_child(self, handle, src, grow):
        """The engine that owns the child batch `handle` of branch() or cut(): child c is LP src[c] with grow[c]
        more rows and columns; a RaggedBatchEngine where the library made a ragged batch (lpg_batch_info)."""
        info = L.BatchInfo()
        self.lib.lpg_batch_info(handle, ctypes.byref(info))
        if info.pad:
            shapes = [(self._shape_of(q)[0] + k, self._shape_of(q)[1] + k) for q, k in zip(src, grow)]
            return RaggedBatchEngine(shapes, lib=self.lib, _handle=handle)
        (m, ncols), k = self._shape_of(src[0]), grow[0]   # one shape: every child's
        return BatchEngine(len(src), m + k, ncols + k, lib=self.lib, _handle=handle)

    # -- cuts ------------------------------------------------------------
    def _mask(self, mask, what):
        """mask: [nmask] or [count, nmask] -> the uint8 array, its pointer, nmask and pitch (0: one for every LP)."""
        mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mk.ndim not in (1, 2) or (mk.ndim == 2 and mk.shape[0] != self.count):
            raise LPGError(f"{what}: mask of shape {mk.shape}, want [nmask] or [{self.count}, nmask]")
        return mk, mk.ctypes.data_as(L.c_uint8_p), mk.shape[-1], mk.shape[1] if mk.ndim == 2 else 0

    def cut_select(self, mask, int_tol: float = 1e-6, max_cuts: int = 8) -> list:
        """The cut rows of every LP (include/lpg.h lpg_batch_cut_select): branch_select's candidates, at most
        max_cuts of them, most fractional first, ties to the smallest column. mask as branch_select's. Returns one
        int64 array of rows per LP (empty where every integer column is integral)."""
        mk, mp, nmask, ld = self._mask(mask, "cut_select")
        ncut = np.zeros(self.count, dtype=np.int64)
        rows = np.zeros((self.count, max(int(max_cuts), 1)), dtype=np.int64)
        self._check(self.lib.lpg_batch_cut_select(self._h, mp, nmask, ld, int_tol, max_cuts, ncut.ctypes.data_as(L.c_int64_p),
                                                  rows.ctypes.data_as(L.c_int64_p)), "lpg_batch_cut_select")
        return [rows[q, :ncut[q]].copy() for q in range(self.count)]

    def cut(self, src, rows_per_child, mask):
        """A new batch of len(src) children made on the device (include/lpg.h lpg_batch_cut): child c is LP src[c]
        plus one Gomory mixed-integer cut per row in rows_per_child[c] (at least one; distinct rows); mask as
        cut_select's, indexed by this batch's LPs; solve_dual() re-optimises the child. Returns a BatchEngine, or a
        RaggedBatchEngine where this batch is ragged or the children's cut counts differ, as the library made it."""
        src = np.ascontiguousarray(src, dtype=np.int64)
        per = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows_per_child]
        if src.ndim != 1 or len(per) != src.shape[0]:
            raise LPGError(f"cut: src of shape {src.shape} and {len(per)} row lists, want [n] and n lists")
        first = np.zeros(len(per) + 1, dtype=np.int64)
        first[1:] = np.cumsum([len(r) for r in per])
        rows = np.ascontiguousarray(np.concatenate(per + [np.zeros(0, dtype=np.int64)]))
        if rows.size == 0:
            rows = np.zeros(1, dtype=np.int64)           # a pointer to pass; the library refuses the empty interval
        mk, mp, nmask, ld = self._mask(mask, "cut")
        child = ctypes.c_void_p()
        self._check(self.lib.lpg_batch_cut(ctypes.byref(child), self._h, src.shape[0], src.ctypes.data_as(L.c_int64_p),
                                           first.ctypes.data_as(L.c_int64_p), rows.ctypes.data_as(L.c_int64_p), mp, nmask, ld),
                    "lpg_batch_cut")
        return self._wrap_child(child, src, [len(r) for r in per])

    # -- scenarios -------------------------------------------------------
    def _ident(self, ident, what):
        """ident: [m] (the same for every LP) or [count, m] -> the flat int64 array of the C ABI."""
        a = np.asarray(ident, dtype=np.int64)
        if a.ndim == 1:
            a = np.tile(a, (self.count, 1))
        if a.shape != (self.count, self.m):
            raise LPGError(f"{what}: ident of shape {a.shape}, want [{self.m}] or [{self.count}, {self.m}]")
        return np.ascontiguousarray(a).ravel()

    def _rhs(self, rhs, lps, what):
        """rhs: [len(lps), m], row c the right-hand side for LP lps[c] -> the packed float64 array of the C ABI."""
        a = np.ascontiguousarray(rhs, dtype=np.float64)
        if a.shape != (len(lps), self.m):
            raise LPGError(f"{what}: rhs of shape {a.shape}, want [{len(lps)}, {self.m}]")
        return a.ravel()

    def scenario(self, src, rhs, ident):
        """A new batch of len(src) children made on the device (include/lpg.h lpg_batch_scenario): child c is LP
        src[c] as it stands, its column 0 restated for the right-hand side rhs[c]; ident[q][i] is the column of LP
        q that was the unit vector e_i in the frame rhs is given in (the basis the LP was loaded with).
        solve_dual() re-optimises the children. The engine returned is of this engine's class."""
        src = np.ascontiguousarray(src, dtype=np.int64)
        if src.ndim != 1:
            raise LPGError(f"scenario: src of shape {src.shape}, want [n]")
        idt, r = self._ident(ident, "scenario"), self._rhs(rhs, src, "scenario")
        child = ctypes.c_void_p()
        self._check(self.lib.lpg_batch_scenario(ctypes.byref(child), self._h, src.shape[0], src.ctypes.data_as(L.c_int64_p),
                                                idt.ctypes.data_as(L.c_int64_p), r.ctypes.data_as(L.c_double_p)),
                    "lpg_batch_scenario")
        return self._wrap_child(child, src, [0] * len(src))

    def set_rhs(self, rhs, ident):
        """Every LP's column 0 restated in place for its new right-hand side rhs[q] (include/lpg.h
        lpg_batch_set_rhs); ident as scenario's, of this batch. The LPs start again as after load()."""
        idt, r = self._ident(ident, "set_rhs"), self._rhs(rhs, range(self.count), "set_rhs")
        self._check(self.lib.lpg_batch_set_rhs(self._h, idt.ctypes.data_as(L.c_int64_p), r.ctypes.data_as(L.c_double_p)),
                    "lpg_batch_set_rhs")

    # -- ranging ---------------------------------------------------------
    def _ranging_flat(self, ident, dual, cost, rhs) -> dict:
        """lpg_batch_ranging into flat arrays: {field: array} for the fields of the wanted groups."""
        idt = self._ident(ident, "ranging")
        nb = sum(self._shape_of(q)[0] for q in range(self.count))
        nc = sum(self._shape_of(q)[1] - 1 for q in range(self.count))
        want = {"dual": dual, "cost": cost, "rhs": rhs}
        out, flat = L.RangingOut(), {}
        for f in RANGING_FIELDS:
            if not want[f.split("_")[0]]:
                continue
            ints = f.endswith("_at")
            flat[f] = np.zeros(nc if f.startswith("cost") else nb, dtype=np.int64 if ints else np.float64)
            setattr(out, f, flat[f].ctypes.data_as(L.c_int64_p if ints else L.c_double_p))
        self._check(self.lib.lpg_batch_ranging(self._h, idt.ctypes.data_as(L.c_int64_p), ctypes.byref(out)),
                    "lpg_batch_ranging")
        return flat

    def ranging(self, ident, *, dual: bool = True, cost: bool = True, rhs: bool = True) -> Ranging:
        """Shadow prices and cost / right-hand-side ranges of every LP, computed on the device from the solved
        tableaus (include/lpg.h lpg_batch_ranging); ident as scenario's. Each of the three groups can be left
        out (then its fields are None and it is not computed). The batch is not changed."""
        flat = self._ranging_flat(ident, dual, cost, rhs)
        return Ranging(**{f: a.reshape(self.count, -1) for f, a in flat.items()})

    def _shape_of(self, q):
        return self.m, self.ncols


class RaggedBatchEngine(BatchEngine):
    """BatchEngine.ragged(shapes): LPs of different shapes in one batch
    (include/lpg.h, "ragged batches"). LP q is an (m_q + nobj) x ncols_q tableau;
    load, set_objective and the artificial solves take one array per LP, get_rows
    and get_basis return one per LP, scenario and set_rhs take one rhs per child or LP and
    one ident per LP, ranging takes one ident per LP and returns one array per LP in every field; solve, solve_dual, reserve_log, set_tolerances,
    get_log and info are BatchEngine's (info reports the largest m, ncols, ld and
    lds_bytes). The packing to and from the C ABI's flat arrays happens here."""

    def __init__(self, shapes, device: int = 0, big_m: bool = False, flags: int = 0, lib=None, _handle=None):
        self._open(lib, _handle)
        try:
            self.shapes = [(int(m), int(nc)) for m, nc in shapes]
        except (TypeError, ValueError) as e:
            raise LPGError(f"BatchEngine.ragged: shapes must be a list of (m, ncols): {e}") from None
        self.count, self.nobj = len(self.shapes), 2 if big_m else 1
        ms = np.array([m for m, _ in self.shapes], dtype=np.int64)
        ncs = np.array([nc for _, nc in self.shapes], dtype=np.int64)
        if _handle is None:
            self._create("lpg_batch_create_ragged", device, self.count, ms.ctypes.data_as(L.c_int64_p),
                         ncs.ctypes.data_as(L.c_int64_p), self.nobj, flags)
        self.m, self.ncols = int(ms.max()), int(ncs.max())

    def _shape_of(self, q):
        return self.shapes[q]

    def shape(self, lp: int) -> L.BatchShape:
        s = L.BatchShape()
        self._check(self.lib.lpg_batch_shape(self._h, lp, ctypes.byref(s)), "lpg_batch_shape")
        return s

    def _flat(self, arrays, what, shape_of, dtype):
        """One array per LP, each of shape_of(m, ncols), flattened LP after LP."""
        arrays = list(arrays)
        if len(arrays) != self.count:
            raise LPGError(f"{what}: {len(arrays)} arrays for {self.count} LPs")
        parts = []
        for q, (a, (m, nc)) in enumerate(zip(arrays, self.shapes)):
            a = np.asarray(a, dtype=dtype)
            if a.shape != shape_of(m, nc):
                raise LPGError(f"{what}: LP {q} has shape {a.shape}, want {shape_of(m, nc)}")
            parts.append(a.ravel())
        return np.ascontiguousarray(np.concatenate(parts))

    def _split(self, flat, shape_of):
        out, at = [], 0
        for m, nc in self.shapes:
            shp = shape_of(m, nc)
            n = int(np.prod(shp))
            out.append(flat[at:at + n].reshape(shp).copy())
            at += n
        return out

    def load(self, tableaus, bases=None):
        """tableaus[q]: [m_q + nobj, ncols_q] (objective row(s) last), bases[q]: [m_q]; the whole batch."""
        T = self._flat(tableaus, "load", lambda m, nc: (m + self.nobj, nc), np.float64)
        bp = None
        if bases is not None:
            bas = self._flat(bases, "load (bases)", lambda m, nc: (m,), np.int64)
            bp = bas.ctypes.data_as(L.c_int64_p)
        self._check(self.lib.lpg_batch_load_packed(self._h, 0, self.count, T.ctypes.data_as(L.c_double_p), bp),
                    "lpg_batch_load_packed")

    def _packed_costs(self, costs, what):
        if costs is None:
            return None, None
        c = self._flat(costs, what, lambda m, nc: (nc - 1,), np.float64)
        return c, c.ctypes.data_as(L.c_double_p)

    def _art(self, art_first, what):
        af = np.ascontiguousarray(art_first, dtype=np.int64)
        if af.shape != (self.count,):
            raise LPGError(f"{what}: art_first of shape {af.shape}, want [{self.count}]")
        return af

    def solve_two_phase(self, art_first, costs=None, max_pivots: int = 1 << 40, rule: int = L.RULE_DANTZIG) -> list:
        """BatchEngine.solve_two_phase with art_first[q] and costs[q] ([ncols_q - 1]) per LP; costs None: -1 x each
        LP's objective row. Afterwards LP q's active columns are 1..art_first[q]-1."""
        af = self._art(art_first, "solve_two_phase")
        keep, cp = self._packed_costs(costs, "solve_two_phase")
        r = (L.Result * self.count)()
        self._check(self.lib.lpg_batch_solve_two_phase_ragged(self._h, af.ctypes.data_as(L.c_int64_p), cp, max_pivots, rule,
                                                              r), "lpg_batch_solve_two_phase_ragged")
        del keep
        return [_res(x) for x in r]

    def solve_big_m(self, art_first, costs=None, max_pivots: int = 1 << 40, rule: int = L.RULE_DANTZIG) -> list:
        """BatchEngine.solve_big_m with art_first[q] and costs[q] per LP."""
        af = self._art(art_first, "solve_big_m")
        keep, cp = self._packed_costs(costs, "solve_big_m")
        r = (L.Result * self.count)()
        self._check(self.lib.lpg_batch_solve_big_m_ragged(self._h, af.ctypes.data_as(L.c_int64_p), cp, max_pivots, rule, r),
                    "lpg_batch_solve_big_m_ragged")
        del keep
        return [_res(x) for x in r]

    def set_objective(self, costs):
        """Engine.set_objective on every LP; costs[q]: [ncols_q - 1]."""
        keep, cp = self._packed_costs(costs, "set_objective")
        self._check(self.lib.lpg_batch_set_objective_packed(self._h, cp), "lpg_batch_set_objective_packed")
        del keep

    def _ident(self, ident, what):
        """ident[q]: [m_q], one array per LP."""
        return self._flat(ident, f"{what} (ident)", lambda m, nc: (m,), np.int64)

    def _rhs(self, rhs, lps, what):
        """rhs[c]: [m of LP lps[c]], one array per entry of lps (an LP outside the batch is the library's to refuse)."""
        rhs = list(rhs)
        if len(rhs) != len(lps):
            raise LPGError(f"{what}: {len(rhs)} right-hand sides for {len(lps)} LPs")
        parts = [np.asarray(a, dtype=np.float64) for a in rhs]
        for c, (a, q) in enumerate(zip(parts, lps)):
            if a.ndim != 1 or (0 <= q < self.count and a.shape != (self.shapes[q][0],)):
                raise LPGError(f"{what}: rhs[{c}] has shape {a.shape}, want ({self.shapes[q][0] if 0 <= q < self.count else 'm'},)")
        return np.ascontiguousarray(np.concatenate(parts + [np.zeros(0)]))

    def ranging(self, ident, *, dual: bool = True, cost: bool = True, rhs: bool = True) -> Ranging:
        """BatchEngine.ranging with one ident array per LP; every field is a list of one array per LP."""
        flat = self._ranging_flat(ident, dual, cost, rhs)
        return Ranging(**{f: self._split(a, (lambda m, nc: (nc - 1,)) if f.startswith("cost") else (lambda m, nc: (m,)))
                          for f, a in flat.items()})

    def get_rows(self) -> list:
        flat = np.zeros(sum((m + self.nobj) * nc for m, nc in self.shapes), dtype=np.float64)
        self._check(self.lib.lpg_batch_get_rows_packed(self._h, 0, self.count, flat.ctypes.data_as(L.c_double_p)),
                    "lpg_batch_get_rows_packed")
        return self._split(flat, lambda m, nc: (m + self.nobj, nc))

    def get_basis(self) -> list:
        flat = np.zeros(sum(m for m, _ in self.shapes), dtype=np.int64)
        self._check(self.lib.lpg_batch_get_basis_packed(self._h, 0, self.count, flat.ctypes.data_as(L.c_int64_p)),
                    "lpg_batch_get_basis_packed")
        return self._split(flat, lambda m, nc: (m,))


@dataclass
class AssignResult(_HasStatus):
    status: int
    steps: int
    objective: float


class AssignmentBatch(_Handle):
    """`count` assignment problems of one shape, nr x nc cost matrices with
    nr <= nc, solved in one launch by the Hungarian method (include/lpg.h,
    "assignment"): every row gets a distinct column, the chosen costs sum to the
    minimum (``maximize=True``: the maximum); +inf forbids a pair."""

    _prefix, _info_type = "lpg_assign", L.AssignInfo

    def __init__(self, count: int, nr: int, nc: int, device: int = 0, maximize: bool = False, lib=None):
        self._open(lib)
        self._create("lpg_assign_create", device, count, nr, nc, L.ASSIGN_MAXIMIZE if maximize else 0)
        self.count, self.nr, self.nc, self.maximize = count, nr, nc, bool(maximize)

    def load(self, costs: np.ndarray, first: int = 0):
        """costs: [n, nr, nc]; problems first .. first + n - 1."""
        c = np.ascontiguousarray(costs, dtype=np.float64)
        if c.ndim != 3 or c.shape[1] != self.nr or c.shape[2] != self.nc:
            raise LPGError(f"load: costs of shape {c.shape}, want [n, {self.nr}, {self.nc}]")
        self._check(self.lib.lpg_assign_load(self._h, first, c.shape[0], c.ctypes.data_as(L.c_double_p), self.nc),
                    "lpg_assign_load")

    def generate(self, seed: int = 20220518, range: int = 100):
        """Problem q, entry (i, j) = floor(uniform01(seed + q, i * nc + j) * range)."""
        self._check(self.lib.lpg_assign_generate(self._h, seed, range), "lpg_assign_generate")

    def solve(self) -> list:
        r = (L.AssignResult * self.count)()
        self._check(self.lib.lpg_assign_solve(self._h, r), "lpg_assign_solve")
        return [AssignResult(x.status, x.steps, x.objective) for x in r]

    def get(self, first: int = 0, n: int = None):
        """(col [n, nr] int64, u [n, nr], v [n, nc]) of problems first .. first + n - 1 after a solve."""
        n = self.count - first if n is None else n
        col = np.empty((n, self.nr), dtype=np.int64)
        u = np.empty((n, self.nr), dtype=np.float64)
        v = np.empty((n, self.nc), dtype=np.float64)
        self._check(self.lib.lpg_assign_get(self._h, first, n, col.ctypes.data_as(L.c_int64_p),
                                            u.ctypes.data_as(L.c_double_p), v.ctypes.data_as(L.c_double_p)),
                    "lpg_assign_get")
        return col, u, v


@dataclass
class BinaryResult(_HasStatus):
    status: int
    found: int
    nodes: int
    objective: float


class BinaryBatch(_Handle):
    """`count` 0-1 programs of one shape, m rows and n <= 64 binary variables,
    solved by implicit enumeration on the device (include/lpg.h, "0-1
    programs"): minimise (``maximize=True``: maximise) c.x subject to a_i.x
    {<=, =, >=} b_i on integer data; 2^split independent sub-searches per problem."""

    _prefix, _info_type = "lpg_binary", L.BinaryInfo

    def __init__(self, count: int, m: int, n: int, split: int = 0, maximize: bool = False, device: int = 0, lib=None):
        self._open(lib)
        self._create("lpg_binary_create", device, count, m, n, split, L.BINARY_MAXIMIZE if maximize else 0)
        self.count, self.m, self.n, self.split, self.maximize = count, m, n, split, bool(maximize)

    @property
    def resident_waves(self) -> int:
        """The waves of this batch's kernel that the device holds at once (the occupancy query)."""
        w = ctypes.c_int64()
        self._check(self.lib.lpg_binary_occupancy(self._h, ctypes.byref(w)), "lpg_binary_occupancy")
        return int(w.value)

    def load(self, A, sense, rhs, c, first: int = 0):
        """A [k, m, n], sense [k, m] of -1 / 0 / +1, rhs [k, m], c [k, n]: problems first .. first + k - 1."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        sense = np.ascontiguousarray(sense, dtype=np.int32)
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64)
        k = A.shape[0] if A.ndim == 3 else -1
        if A.shape != (k, self.m, self.n) or sense.shape != (k, self.m) or rhs.shape != (k, self.m) or c.shape != (k, self.n):
            raise LPGError(f"load: shapes {A.shape}, {sense.shape}, {rhs.shape}, {c.shape}, want [k, {self.m}, {self.n}], "
                           f"[k, {self.m}], [k, {self.m}], [k, {self.n}]")
        self._check(self.lib.lpg_binary_load(self._h, first, k, A.ctypes.data_as(L.c_double_p), self.n,
                                             sense.ctypes.data_as(L.c_int32_p), rhs.ctypes.data_as(L.c_double_p),
                                             c.ctypes.data_as(L.c_double_p)), "lpg_binary_load")

    def generate(self, seed: int = 20220518, kind: int = L.BINARY_GEN_BANDED):
        """The banded planted problems of include/lpg.h ("Generator"), problem q from seed + q."""
        self._check(self.lib.lpg_binary_generate(self._h, seed, kind), "lpg_binary_generate")

    def solve(self, max_nodes: int = 0) -> list:
        """Continues every search, by at most max_nodes nodes per sub-search (0: to the end)."""
        r = (L.BinaryResult * self.count)()
        self._check(self.lib.lpg_binary_solve(self._h, max_nodes, r), "lpg_binary_solve")
        return [BinaryResult(x.status, x.found, x.nodes, x.objective) for x in r]

    def get(self, first: int = 0, n: int = None) -> np.ndarray:
        """x [n, self.n] int8 of problems first .. first + n - 1 after a solve; -1 throughout where nothing was found."""
        n = self.count - first if n is None else n
        x = np.empty((n, self.n), dtype=np.int8)
        self._check(self.lib.lpg_binary_get(self._h, first, n, x.ctypes.data_as(L.c_int8_p)), "lpg_binary_get")
        return x


@dataclass
class TransportResult(_HasStatus):
    status: int
    iterations: int
    objective: float


class TransportBatch(_Handle):
    """`count` balanced transportation problems of one shape, nr sources by nc
    sinks, solved on the device by the tableau method (include/lpg.h,
    "transportation"): a least-cost or northwest-corner start, potentials,
    pricing and the closed loop. Costs, supplies and demands are integers."""

    _prefix, _info_type = "lpg_transport", L.TransportInfo

    STARTS = {"least_cost": L.TRANSPORT_START_LEAST_COST, "northwest": L.TRANSPORT_START_NORTHWEST}

    def __init__(self, count: int, nr: int, nc: int, maximize: bool = False, start: str = "least_cost", device: int = 0,
                 lib=None):
        if start not in self.STARTS:
            raise LPGError(f"TransportBatch: start {start!r}, want 'least_cost' or 'northwest'")
        self._open(lib)
        self._create("lpg_transport_create", device, count, nr, nc, (L.TRANSPORT_MAXIMIZE if maximize else 0) | self.STARTS[start])
        self.count, self.nr, self.nc, self.maximize, self.start = count, nr, nc, bool(maximize), start

    def load(self, costs, supply, demand, first: int = 0):
        """costs [n, nr, nc], supply [n, nr], demand [n, nc]: problems first .. first + n - 1."""
        c = np.ascontiguousarray(costs, dtype=np.float64)
        s = np.ascontiguousarray(supply, dtype=np.float64)
        d = np.ascontiguousarray(demand, dtype=np.float64)
        n = c.shape[0] if c.ndim == 3 else -1
        if c.shape != (n, self.nr, self.nc) or s.shape != (n, self.nr) or d.shape != (n, self.nc):
            raise LPGError(f"load: shapes {c.shape}, {s.shape}, {d.shape}, want [n, {self.nr}, {self.nc}], "
                           f"[n, {self.nr}], [n, {self.nc}]")
        self._check(self.lib.lpg_transport_load(self._h, first, n, c.ctypes.data_as(L.c_double_p), self.nc,
                                                s.ctypes.data_as(L.c_double_p), d.ctypes.data_as(L.c_double_p)),
                    "lpg_transport_load")

    def generate(self, seed: int = 20220518, range: int = 100, qmax: int = 9):
        """The generated problems of include/lpg.h ("Generator"), problem q from seed + q."""
        self._check(self.lib.lpg_transport_generate(self._h, seed, range, qmax), "lpg_transport_generate")

    def solve(self, max_iters: int = None, rule: int = L.RULE_DANTZIG) -> list:
        """Continues every problem by at most max_iters iterations (default 50 (nr + nc))."""
        if max_iters is None:
            max_iters = 50 * (self.nr + self.nc)
        r = (L.TransportResult * self.count)()
        self._check(self.lib.lpg_transport_solve(self._h, max_iters, rule, r), "lpg_transport_solve")
        return [TransportResult(x.status, x.iterations, x.objective) for x in r]

    def get(self, first: int = 0, n: int = None):
        """(x [n, nr, nc], u [n, nr], v [n, nc], basis [n, nr + nc - 1] int64) of problems first .. first + n - 1."""
        n = self.count - first if n is None else n
        x = np.empty((n, self.nr, self.nc), dtype=np.float64)
        u = np.empty((n, self.nr), dtype=np.float64)
        v = np.empty((n, self.nc), dtype=np.float64)
        basis = np.empty((n, self.nr + self.nc - 1), dtype=np.int64)
        self._check(self.lib.lpg_transport_get(self._h, first, n, x.ctypes.data_as(L.c_double_p),
                                               u.ctypes.data_as(L.c_double_p), v.ctypes.data_as(L.c_double_p),
                                               basis.ctypes.data_as(L.c_int64_p)), "lpg_transport_get")
        return x, u, v, basis
