"""Cuts on the device (include/lpg.h, "cuts") against their numpy statement and
the CPU oracle (tests/cut_cases.py), bit for bit: the children lpg_batch_cut
makes, what lpg_batch_cut_select lists, the re-solve of the children by
solve_dual, a second round, cuts on branched children, the host refusals that
need a parent batch, and frontend.solve_ilp_text with cut rounds against the
reference walk.

Two notes on the shapes. (1, 1) has one row, so its k = 2 case has one cut per
child. At (37, 92), ncols 130, no k reaches the next pitch: there are 37 rows,
and 130 + 37 < 192; the pitch that small k keep and every candidate crosses is
covered by (40, 79) instead: ncols 120, pitch 128, more than 8 candidates per
LP."""
from __future__ import annotations

import numpy as np
import pytest

import batch_cases as bc
import branch_cases as br
import cut_cases as cc

pytestmark = pytest.mark.gpu

# (m, n): ncols = n + m + 1
# (96, 160) is the global-tier shape: ncols 257, its tableau does not fit in LDS
SHAPES = [(1, 1), (5, 6), (8, 8), (33, 33), (20, 43), (37, 92), (40, 79), (96, 160)]
LDS_SHAPES = SHAPES[:-1]                                   # every LDS-tier shape also runs forced to the global tier


def _pitch(nc):
    return (nc + 63) & ~63


def _check(s, got):
    cc.check_selection(s, got)
    want = cc.expected(s, got)
    for level in range(1, s["levels"] + 1):
        assert got[f"{level}/built/src"].size > 0
        br.assert_level(got, want, level)
    return want


def _ks(got, level=1):
    return np.diff(got[f"{level}/built/first"])


@pytest.mark.parametrize("k", ["1", "2", "all"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_children_and_their_resolve_equal_numpy_and_the_oracle(m, n, k):
    """A dense batch, one child per LP with k cuts: the children as built equal numpy's, and after solve_dual the
    oracle's, bit for bit."""
    s = cc.spec("dense", m, n, B=4, k=k)
    got = cc.run_batch(s)
    assert (got["parent/status"] == br.OPTIMAL).all()
    assert got["1/built/src"].size == s["B"]                # every LP of these has a fractional masked basic variable
    _check(s, got)
    nc, ks, ncand = n + m + 1, _ks(got), got["1/built/ncand"]
    assert np.array_equal(ks, {"1": np.minimum(ncand, 1), "2": np.minimum(ncand, 2), "all": ncand}[k])
    if k == "2" and m > 1:
        first, rows = got["1/built/first"], got["1/built/cutrows"]
        assert (ks == 2).all() and all(rows[first[c]] > rows[first[c] + 1] for c in range(s["B"]))
    assert np.array_equal(got["1/built/ncols"], nc + ks) and np.array_equal(got["1/built/m"], m + ks)
    assert np.array_equal(got["1/built/nact"], nc - 1 + ks)
    assert np.array_equal(got["1/built/art_first"], nc + ks)        # no artificials: what a batch of one shape reports
    assert np.array_equal(got["1/built/ld"], _pitch(nc + ks))
    assert int(got["1/ragged"]) == int(len(set(ks.tolist())) > 1)   # one shape unless the cut counts differ
    if (m, n) == (20, 43):
        assert got["parent/ld"][0] == 64 and (got["1/built/ld"] == 128).all()       # one cut crosses the pitch
    if (m, n) == (37, 92):
        assert got["parent/ld"][0] == 192 and (got["1/built/ld"] == 192).all()
    if (m, n) == (40, 79):
        assert got["parent/ld"][0] == 128 and (got["1/built/ld"] == (192 if k == "all" else 128)).all()
    if (m, n) == (96, 160):
        assert (got["1/built/tier"] == 1).all()


def test_lds_tier_shapes_forced_to_the_global_tier(tmp_path):
    specs = [cc.spec("dense", m, n, B=4, k=k) for m, n in LDS_SHAPES for k in ("1", "all")]
    for s, got in zip(specs, cc.in_subprocess(specs, {"LPG_BATCH_TIER": "global"}, tmp_path)):
        assert (got["parent/tier"] == 1).all() and (got["1/built/tier"] == 1).all()
        _check(s, got)


@pytest.mark.parametrize("k", ["1", "2"])
@pytest.mark.parametrize("m,n", [(8, 8), (33, 33)])
def test_two_phase_parent_moves_the_artificials_right_by_k(m, n, k):
    """The odd and the even shift of the inert artificial columns behind nact."""
    s = cc.spec("art", m, n, B=4, k=k)
    got = cc.run_batch(s)
    af, kk = br.art_first_of(m, n), int(k)
    assert (got["parent/nact"] == af - 1).all() and (got["1/built/nact"] == af - 1 + kk).all()
    assert (got["1/built/ncols"] == n + m + 1 + kk).all() and (got["1/built/art_first"] == n + m + 1 + kk).all()
    assert (got["1/built/ncols"] > got["1/built/nact"] + 1).all()      # artificial columns behind the new slacks
    assert got["1/built/src"].size == s["B"] and int(got["1/ragged"]) == 0
    _check(s, got)


def test_src_repeating_and_descending_with_different_row_sets_and_a_mask_per_lp():
    s = cc.spec("dense", 8, 8, B=4, pattern="repeat", mask="per_lp")
    got = cc.run_batch(s)
    src, first, rows = got["1/built/src"], got["1/built/first"], got["1/built/cutrows"]
    assert got["mask"].shape == (4, 16) and len({r.tobytes() for r in got["mask"]}) > 1
    assert src.size != s["B"] and (np.diff(src[:4]) < 0).all() and len(set(src.tolist())) < src.size
    sets = {}
    for c, q in enumerate(src):
        sets.setdefault(int(q), set()).add(tuple(rows[first[c]:first[c + 1]]))
    assert any(len(v) > 1 for v in sets.values())           # one source, different row sets
    _check(s, got)


def test_unequal_cut_counts_on_a_uniform_parent_give_a_ragged_child():
    s = cc.spec("dense", 33, 33, B=4, k="uneven")
    got = cc.run_batch(s)
    ks = _ks(got)
    assert ks.tolist() == [1, 2, 3, 1] and int(got["1/ragged"]) == 1
    assert np.array_equal(got["1/built/ncols"], 67 + ks) and np.array_equal(got["1/built/nact"], 66 + ks)
    assert np.array_equal(got["1/built/art_first"], got["1/built/ncols"])
    _check(s, got)


@pytest.mark.parametrize("k", ["1", "all"])
def test_ragged_parent_gives_a_ragged_child_on_both_tiers(k):
    s = cc.spec("ragged", lps=[[2, 2], [8, 8], [33, 33], [96, 160]], k=k)
    got = cc.run_batch(s)
    src, ks = got["1/built/src"], _ks(got)
    assert src.size == 4 and int(got["1/ragged"]) == 1
    assert np.array_equal(got["1/built/m"], got["parent/m"][src] + ks)
    assert np.array_equal(got["1/built/ncols"], got["parent/ncols"][src] + ks)
    assert np.array_equal(got["1/built/art_first"], got["parent/art_first"][src] + ks)
    assert set(got["1/built/tier"].tolist()) == {0, 1}
    _check(s, got)


@pytest.mark.parametrize("kind,m,n,k", [("dense", 8, 8, "2"), ("dense", 33, 33, "all")])
def test_a_second_round_on_a_child_that_holds_cut_slacks(kind, m, n, k):
    s = cc.spec(kind, m, n, B=4, k=k, levels=2)
    got = cc.run_batch(s)
    _check(s, got)
    src = got["2/built/src"]
    assert np.array_equal(got["2/built/ncols"], got["1/built/ncols"][src] + _ks(got, 2))
    assert (got["2/built/nact"] > got["1/built/nact"][src]).all()


@pytest.mark.parametrize("kind,m,n", [("dense", 8, 8), ("art", 8, 8), ("ragged", None, None)])
def test_a_cut_on_a_branched_child_counts_the_branch_slack_as_continuous(kind, m, n):
    s = cc.spec(kind, m, n, B=4, lps=[[2, 2], [8, 8], [33, 33]] if kind == "ragged" else None, k="2", pre="branch")
    got = cc.run_batch(s)
    assert got["parent/status"].size > 4 or kind == "ragged"        # the branched level: two children per parent
    nmask = got["mask"].shape[-1]
    assert (got["parent/nact"] > nmask).any() or kind == "art"      # the branch slack lies behind the mask
    _check(s, got)


# ---------------------------------------------------------------------------
# one cut against one bound: the two calls share the copy that makes a child
# ---------------------------------------------------------------------------
def _solved(m, n, B=3):
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(B, m, n + m + 1)
    e.generate(n, bc.SEED, 0)
    assert all(r.status == br.OPTIMAL for r in e.solve(br.BUDGET))
    return e


def _same_outside_the_new_row(parent, shapes, nacts):
    """A child by cut() with one cut and the two children by branch() on the same row of every LP of `parent`
    (LP q of shape shapes[q] = (m, ncols) with nacts[q] active columns): bit for bit the same in rows 0..m-1, the
    objective row and the basis, and in the new row the same 1 in the new slack column nact + 1."""
    B = len(shapes)
    ones = np.ones(max(nc for _, nc in shapes) - 1, dtype=np.uint8)
    row = parent.branch_select(ones)[0]
    assert (row >= 0).all()                                 # every LP of these has a fractional basic variable
    src = np.arange(B)
    cut = parent.cut(src, [[r] for r in row], ones)
    bound = parent.branch(np.repeat(src, 2), np.repeat(row, 2), np.tile([-1, 1], B))
    try:
        assert type(cut) is type(bound) is type(parent)
        cT, cB, bT, bB = list(cut.get_rows()), list(cut.get_basis()), list(bound.get_rows()), list(bound.get_basis())
        for q, ((m, nc), nact) in enumerate(zip(shapes, nacts)):
            assert cT[q].shape == (m + 2, nc + 1) and cut.active_columns(q)[0] == nact + 1
            keep = np.arange(m + 2) != m
            assert (cT[q][keep, nact + 1] == 0.0).all() and cT[q][m, nact + 1] == 1.0 and cB[q][m] == nact + 1
            for child in (2 * q, 2 * q + 1):
                assert bT[child].shape == cT[q].shape and bound.active_columns(child) == cut.active_columns(q)
                assert np.array_equal(bc.bits(bT[child][keep]), bc.bits(cT[q][keep])), (q, child)
                assert bT[child][m, nact + 1] == 1.0
                assert np.array_equal(bB[child], cB[q]), (q, child)
    finally:
        cut.close()
        bound.close()


@pytest.mark.parametrize("inert", [0, 1])
@pytest.mark.parametrize("m,n", [(5, 6), (8, 8)])
def test_one_cut_and_a_bound_on_the_same_row_differ_in_the_new_row_only(m, n, inert):
    """nact + 1 is even at (5, 6) and odd at (8, 8) (all of columns 0..nact as pairs, or one of them in the tail);
    `inert` columns behind nact are the shifted part, which turns that parity round, and some of them are basic."""
    nc = n + m + 1
    e = _solved(m, n)
    try:
        if inert:
            e.set_active_columns(nc - 1 - inert)
            assert (e.get_basis() > nc - 1 - inert).any()   # the basis shift
        _same_outside_the_new_row(e, [(m, nc)] * e.count, [nc - 1 - inert] * e.count)
    finally:
        e.close()


def test_one_cut_and_a_bound_on_the_same_row_of_a_ragged_parent():
    import linearprogramming_amd as lpg
    shapes = [(5, 12), (8, 17), (5, 12)]
    g = lpg.BatchEngine.ragged(shapes)
    a, b = _solved(5, 6), _solved(8, 8)
    try:
        Ta, Ba, Tb, Bb = a.get_rows(), a.get_basis(), b.get_rows(), b.get_basis()
        g.load([Ta[0], Tb[0], Ta[1]], [Ba[0], Bb[0], Ba[1]])
        assert all(r.status == br.OPTIMAL and r.pivots == 0 for r in g.solve(br.BUDGET))
        _same_outside_the_new_row(g, shapes, [nc - 1 for _, nc in shapes])
    finally:
        for x in (g, a, b):
            x.close()


# ---------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------
def test_cut_select_equals_numpy_for_every_max_cuts_and_a_mask_per_lp():
    m, n, B = 33, 33, 6
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(B, m, n + m + 1)
    try:
        e.generate(n, bc.SEED, 0)
        e.solve(br.BUDGET)
        T, basis = e.get_rows(), e.get_basis()
        rng = np.random.default_rng(11)
        nmask = n + m - 5                                   # nmask < ncols - 1
        holes = (rng.random(nmask) < 0.6).astype(np.uint8)
        per_lp = (rng.random((B, nmask)) < 0.5).astype(np.uint8)
        per_lp[B - 1] = 0                                   # an LP without integer columns
        for mask in (holes, per_lp):
            full = [cc.select_rows(T[q], basis[q], m, mask if mask.ndim == 1 else mask[q], 1e-6, cc.MAX_CUTS) for q in range(B)]
            counts = sorted({len(x) for x in full})
            assert counts[-1] > 3
            # smaller than, equal to and larger than the candidate counts of the batch
            for max_cuts in (1, 3, counts[0] or 1, counts[-1], counts[-1] + 5, cc.MAX_CUTS):
                got = e.cut_select(mask, 1e-6, max_cuts)
                for q in range(B):
                    assert np.array_equal(got[q], full[q][:max_cuts]), (max_cuts, q, got[q], full[q])
        assert len(e.cut_select(per_lp, 1e-6, 8)[B - 1]) == 0
    finally:
        e.close()


def test_cut_select_ties_the_fill_and_the_raw_arrays():
    import ctypes
    from linearprogramming_amd import _lib as L
    m, nc = 5, 9
    T = np.zeros((2, m + 1, nc))
    basis = np.tile(np.array([5, 2, 3, 7, 1]), (2, 1))
    for q in range(2):
        for i in range(m):
            T[q, i, basis[q, i]] = 1.0
    T[0, :m, 0] = [2.5, 7.25, 4.5, 3.0, 1.75]      # 0.5 twice: column 3 (row 2) before column 5 (row 0); 0.25 twice
    T[1, :m, 0] = [3.0, 4.0 + 1e-7, 6.0 - 1e-7, 0.0, 11.0]    # integral or within int_tol
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(2, m, nc)
    try:
        e.load(T, basis)
        ones = np.ones(nc - 1, dtype=np.uint8)
        got = e.cut_select(ones, 1e-6, 8)
        assert got[0].tolist() == [2, 0, 4, 1] and got[1].size == 0
        assert e.cut_select(ones, 1e-6, 3)[0].tolist() == [2, 0, 4]
        assert e.cut_select(np.array([1, 1, 0, 1, 1, 1, 1, 1], dtype=np.uint8))[0].tolist() == [0, 4, 1]
        ncut, rows = np.full(2, 99, dtype=np.int64), np.full((2, 6), 99, dtype=np.int64)
        rc = e.lib.lpg_batch_cut_select(e._b, ones.ctypes.data_as(L.c_uint8_p), nc - 1, 0, 1e-6, 6,
                                        ncut.ctypes.data_as(L.c_int64_p), rows.ctypes.data_as(L.c_int64_p))
        assert rc == 0 and ncut.tolist() == [4, 0]
        assert rows.tolist() == [[2, 0, 4, 1, -1, -1], [-1] * 6]             # unused slots are -1
        del ctypes
    finally:
        e.close()


# ---------------------------------------------------------------------------
# the host refusals that need a parent batch (tests/test_batch_cut_abi.py has the others)
# ---------------------------------------------------------------------------
def test_refusals_name_the_index_and_leave_the_parent_alone():
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(3, 4, 9)
    g = lpg.BatchEngine.ragged([(4, 9), (2, 5)])
    bm = lpg.BatchEngine(2, 4, 9, big_m=True)
    ones = np.ones(8, dtype=np.uint8)
    try:
        e.generate(4, bc.SEED, 0)
        before = bc.bits(e.get_rows()).copy()
        with pytest.raises(lpg.LPGError, match=r"lpg_batch_cut rc=-1.*src\[1\] = 3 outside"):
            e.cut([0, 3], [[0], [0]], ones)
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*rows\[2\] = 4 \(child 1\) outside the rows 0\.\.3 of LP 1"):
            e.cut([0, 1], [[0, 3], [4]], ones)
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*rows\[1\] = -1 \(child 0\) outside"):
            e.cut([0], [[0, -1]], ones)
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*rows\[1\] = 2 \(child 1\) outside the rows 0\.\.1 of LP 1"):
            g.cut([0, 1], [[3], [2]], np.ones(4, dtype=np.uint8))
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*rows\[3\] = 1 appears twice in child 1"):
            e.cut([0, 2], [[1], [1, 2, 1]], ones)
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*child 1 has 1025 cuts, more than LPG_BATCH_MAX_CUTS = 1024"):
            e.cut([0, 0], [[0], [0] * 1025], ones)
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*first\[1\] = 0 is not above first\[0\] = 0"):
            e.cut([0], [[]], ones)
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*n = 0"):
            e.cut([], [], ones)
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*nmask 9 outside 1\.\.8"):
            e.cut([0], [[0]], np.ones(9, dtype=np.uint8))
        with pytest.raises(lpg.LPGError, match=r"lpg_batch_cut rc=-4.*Big-M"):
            bm.cut([0], [[0]], ones)
        with pytest.raises(lpg.LPGError, match=r"lpg_batch_cut_select rc=-4.*Big-M"):
            bm.cut_select(ones)
        for mask, tol, mc, word in ((np.ones(9), 1e-6, 8, "nmask 9 outside 1..8"), (ones, 0.5, 8, "int_tol"),
                                    (ones, 1e-6, 0, "max_cuts = 0"), (ones, 1e-6, 1025, "max_cuts = 1025")):
            with pytest.raises(lpg.LPGError, match="rc=-1.*" + word):
                e.cut_select(mask, tol, mc)
        assert np.array_equal(bc.bits(e.get_rows()), before)
    finally:
        for x in (e, g, bm):
            x.close()


def test_child_dimension_over_the_limit_is_refused():
    import linearprogramming_amd as lpg
    e = lpg.BatchEngine(1, 2, 8191)
    try:
        with pytest.raises(lpg.LPGError, match=r"rc=-1.*child 0 of LP 0.*ncols \+ 2 = 8193 exceed 8192"):
            e.cut([0], [[0, 1]], np.ones(4, dtype=np.uint8))
    finally:
        e.close()


# ---------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------
def _models():
    return {name: v[0] for name, v in cc.MODELS.items()}


@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("name", ["a3_min_eq_neg", "three_var", "two_phase", "two_var"])
def test_solve_ilp_text_with_cut_rounds_equals_the_reference_walk(name, rounds):
    from linearprogramming_amd import frontend as F
    text = _models()[name]
    ref = cc.reference_walk(text, cut_rounds=rounds, node_limit=200)
    assert ref["status"] == "OPTIMAL" and ref["nodes"] < 200
    sol = F.solve_ilp_text(text, cut_rounds=rounds)
    cc.same_as_walk(sol, ref)


@pytest.mark.parametrize("name", ["a3_min_eq_neg", "three_var", "two_phase", "two_var"])
def test_cut_rounds_zero_is_todays_solve_ilp_text(name):
    from linearprogramming_amd import frontend as F
    text = _models()[name]
    plain, zero = F.solve_ilp_text(text), F.solve_ilp_text(text, cut_rounds=0, max_cuts=3)
    assert (plain.status, plain.nodes, plain.depth, plain.pivots, plain.method) == \
        (zero.status, zero.nodes, zero.depth, zero.pivots, zero.method)
    assert bc.bits(plain.z) == bc.bits(zero.z)
    assert plain.variables.keys() == zero.variables.keys()
    for key in plain.variables:
        assert bc.bits(plain.variables[key]) == bc.bits(zero.variables[key]), key
    cc.same_as_walk(zero, br.reference_walk(text, node_limit=200))


def test_max_cuts_one_and_a_mixed_model():
    from linearprogramming_amd import frontend as F
    text = _models()["three_var"]
    for kw in ({"cut_rounds": 2, "max_cuts": 1}, {"cut_rounds": 1, "integer": ["x1"]}):
        ref = cc.reference_walk(text, node_limit=200, **kw)
        sol = F.solve_ilp_text(text, **kw)
        cc.same_as_walk(sol, ref)
        assert sol.status == "OPTIMAL"
