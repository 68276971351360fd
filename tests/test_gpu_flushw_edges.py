"""k_flushw's band addressing at its edges, bitwise against the oracle.

The block pass (linearprogramming_amd/csrc/lpg_flushw.h) reads and writes a
16-row band of a column tile as a buffer whose size is the band's rows inside
the item: the range check is the row predicate of a ragged last band, an empty
buffer stands for the look-ahead past the item's end, and a lane whose column
pair is dead or beyond the tableau sits outside every buffer. The shapes here
are the smallest at which that can go wrong: a ragged band only, one full
band, a full band plus one row, 3 - 4 bands around the NB = 2 ring prologue;
an odd last column pair, an exact tile, one pair into the next tile; whole and
partial blocks at every compiled slot count; both item queues with a ragged
band and a partial last tile. Every case compares the pivot log, the basis
and the whole tableau bit for bit.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle.lpo import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lpg():
    import linearprogramming_amd as lpg
    lpg.load()
    assert lpg.device_count() >= 1, "no GPU visible"
    return lpg


_SOLVED: dict = {}


def _oracle(m, n, seed, rule, cap):
    """The oracle's solve of the generated LP, computed once and only read afterwards."""
    key = (m, n, seed, rule, cap)
    if key not in _SOLVED:
        o = Oracle(m, n + m + 1, nthreads=8 if m > 1000 else 1)
        o.generate(n, seed, 0)
        _SOLVED[key] = (o, o.solve(cap, rule))
    return _SOLVED[key]


def _log(x):
    k, r = x.get_log()
    return list(zip(k.tolist(), r.tolist()))


def _run(lpg, monkeypatch, k, m, n, seed, rule, cap, min_pivots, **env):
    monkeypatch.setenv("LPG_FLUSH_KERNEL", "w")
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    monkeypatch.setenv("LPG_DEFER", str(k))
    e = lpg.Engine(m, n + m + 1)
    monkeypatch.delenv("LPG_DEFER")
    o, ores = _oracle(m, n, seed, rule, cap)
    e.generate(n, seed, 0)
    res = e.solve(cap, rule)
    assert res.status == ores.status
    assert res.pivots == ores.pivots and res.pivots >= min_pivots
    assert _log(e) == _log(o)
    assert np.array_equal(e.get_basis(), o.get_basis())
    assert np.array_equal(e.get_rows(0, m + 1), o.get_rows())
    return res


@pytest.mark.parametrize("k,noskip", [(8, "0"), (32, "0"), (64, "0"), (96, "0"), (128, "0"), (32, "1"), (96, "1")])
@pytest.mark.parametrize("ncols", [255, 256, 257])
@pytest.mark.parametrize("m", [15, 16, 17, 47, 48, 49])
def test_row_edges_and_column_tile_edges(lpg, monkeypatch, m, ncols, k, noskip):
    """Ragged band only / one full band / full + 1 row / 3 - 4 bands, times an
    odd last pair / an exact tile / one pair into the next tile; whole blocks
    (K = 8, and K = 32 from m = 47), partial ones above; with and without
    column skipping. The oracle takes 22 - 70 pivots to optimality."""
    res = _run(lpg, monkeypatch, k, m, ncols - m - 1, 31, 0, 200_000, 1, LPG_NO_SKIP=noskip)
    assert res.status == 1


@pytest.mark.parametrize("k", [32, 64, 96, 128])
def test_whole_and_partial_blocks_ragged_rows(lpg, monkeypatch, k):
    """209 = 13 x 16 + 1 rows, 158 pivots to optimality: at least one whole
    block and a partial one in every instantiation."""
    res = _run(lpg, monkeypatch, k, 209, 303, 16, 0, 200_000, k + 1)
    assert res.status == 1


@pytest.mark.parametrize("xcd", ["0", "1"])
@pytest.mark.parametrize("k", [96, 128])
def test_item_queues_ragged_band_partial_last_tile(lpg, monkeypatch, k, xcd):
    """1037 rows (a 13-row ragged band) x 16,439 columns (odd, 65 tiles of 256):
    the global queue and the XCD-grouped queues, one whole block and a partial
    one, stopped at the iteration limit."""
    _run(lpg, monkeypatch, k, 1037, 15401, 17, 0, k + 17, k + 1, LPG_FLUSH_XCD=xcd)
