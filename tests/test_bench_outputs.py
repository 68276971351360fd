"""bench.py's plain and --full forms and --dump-outputs.

A plain run prints the headline line only (no CPU baseline, no parity legs);
--full adds them. --dump-outputs writes the engine's state after the last
timed step as float64 .npy files, under 64 MB for every BASELINE config, the
sampled rows depending on the shape alone. CPU tests drive dump_outputs with a
stand-in engine; the GPU tests run the benchmark itself at config 2 (that is
what they are about) and compare the dump bitwise with the CPU oracle at the
same pivot count.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 64 * 1000 * 1000


class _FakeEngine:
    """Readouts of a made-up m x ncols state (row i holds i + column / ncols)."""

    def __init__(self, m, ncols, npiv):
        self.m, self.ncols, self.npiv = m, ncols, npiv

    def get_log(self):
        return np.arange(1, self.npiv + 1, dtype=np.int64), np.arange(self.npiv, dtype=np.int64) % self.m

    def get_basis(self):
        return np.arange(self.m, dtype=np.int64) + 7

    def get_column0(self):
        return np.arange(self.m, dtype=np.float64)

    def get_rows(self, row0, nrows):
        return row0 + np.arange(nrows)[:, None] + np.arange(self.ncols)[None, :] / self.ncols


def _res(pivots):
    return types.SimpleNamespace(status=2, pivots=pivots, objective=0.1 + 0.2)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_float64_arrays_of_the_state(tmp_path):
    m, ncols = 37, 101
    bench.dump_outputs(str(tmp_path / "o"), _FakeEngine(m, ncols, 50), _res(50), m, 1, 0)
    out = _load(tmp_path / "o")
    assert sorted(out) == ["basis", "column0", "log_entering", "log_leaving", "objective_row", "result",
                           "tableau_row_index", "tableau_rows"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert out["result"].tolist() == [2.0, 50.0, 0.1 + 0.2]
    assert out["log_entering"].tolist() == list(range(1, 51)) and out["basis"].tolist() == list(range(7, 7 + m))
    assert out["tableau_row_index"].tolist() == list(range(m))          # small: every constraint row
    assert out["tableau_rows"].shape == (m, ncols) and out["tableau_rows"][5, 0] == 5.0
    assert out["objective_row"][0] == float(m) and out["column0"].shape == (m,)


def test_dump_is_the_same_from_run_to_run_and_other_ranks_write_nothing(tmp_path):
    m, ncols = 600, 20000                                              # 600 rows x 160 kB: a sample
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _FakeEngine(m, ncols, 9), _res(9), m, 1, 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["tableau_row_index"].astype(int)
    assert 1 < len(idx) < m and np.all(np.diff(idx) > 0) and idx.max() < m
    assert np.array_equal(a["tableau_rows"][:, 0], idx.astype(np.float64))
    bench.dump_outputs(str(tmp_path / "r1"), _FakeEngine(m, ncols, 9), _res(9), m, 2, 1)
    assert not (tmp_path / "r1").exists()
    bench.dump_outputs(str(tmp_path / "r0"), _FakeEngine(m, ncols, 9), _res(9), m, 2, 0)
    assert sorted(_load(tmp_path / "r0")) == ["basis", "log_entering", "log_leaving", "result"]


@pytest.mark.parametrize("config", sorted(bench.CONFIGS))
def test_dump_stays_under_64_mb_at_every_config(config):
    """Bytes of every array for the config's shape with the longest log kept."""
    m, n = bench.CONFIGS[config]["m"], bench.CONFIGS[config]["n"]
    ncols = n + m + 1
    rows = len(bench.dump_row_sample(m, ncols))
    assert rows >= 1 and np.array_equal(bench.dump_row_sample(m, ncols), bench.dump_row_sample(m, ncols))
    total = 8 * (3 + 2 * bench.DUMP_LOG_ENTRIES + m + (m + 1) + ncols + rows + rows * ncols) + 8 * 128
    assert total <= LIMIT, total


def test_log_keeps_the_last_entries(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LOG_ENTRIES", 16)
    bench.dump_outputs(str(tmp_path), _FakeEngine(8, 12, 40), _res(40), 8, 1, 0)
    assert np.load(tmp_path / "log_entering.npy").tolist() == list(range(25, 41))


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LPG_DEFER")}
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", "2", "--steps", "3", "--warmup", "1",
                        *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_dump_is_the_oracles_state(tmp_path):
    from oracle.lpo import GEN_DENSE, RULE_DANTZIG, Oracle
    d = _bench("--dump-outputs", str(tmp_path / "out"))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "f64"
    K = d["roofline"]["pending_pivots_per_launch"]
    assert d["config"]["pivots_timed"] == 3 * K                        # --steps sets the timed blocks
    assert abs(d["value"] - K / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    assert d["cpu_baseline"] is None and "parity" not in d and "parity_trajectory" not in d
    assert d["roofline"]["launches_timed"] == 0 and "--full" in d["roofline"]["note"]
    out = _load(tmp_path / "out")
    assert all(a.dtype == np.float64 for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= LIMIT
    m, n = bench.CONFIGS[2]["m"], bench.CONFIGS[2]["n"]
    npiv = d["pivots_total"]
    assert out["result"][1] == npiv and out["result"][2] == d["objective"]
    o = Oracle(m, n + m + 1)
    try:
        o.generate(n, bench.SEED, GEN_DENSE)
        ores = o.solve(npiv, RULE_DANTZIG)
        k, r = o.get_log()
        rows = o.get_rows()
        basis = o.get_basis()
    finally:
        o.close()
    assert ores.pivots == npiv and out["result"][2] == ores.objective
    assert np.array_equal(out["log_entering"], k.astype(np.float64))
    assert np.array_equal(out["log_leaving"], r.astype(np.float64))
    assert np.array_equal(out["basis"], basis.astype(np.float64))
    assert np.array_equal(out["column0"], rows[:m, 0]) and np.array_equal(out["objective_row"], rows[m])
    idx = out["tableau_row_index"].astype(int)
    assert idx.tolist() == list(range(m)) and np.array_equal(out["tableau_rows"], rows[idx])


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline_and_the_event_timed_pass():
    d = _bench("--full", "--cpu-seconds", "0.5", "--cpu-1core-seconds", "0")
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["parity"]["identical_pivot_sequence"] is True
    assert d["parity"]["pivots_compared"] > 0
    assert d["roofline"]["launches_timed"] > 0 and d["roofline"]["update_ms_mean"] > 0 and "note" not in d["roofline"]
