"""Ragged batches on the device (include/lpg.h, "ragged batches"): LPs of
different shapes in one batch, every LP compared bit for bit with an
oracle.lpo.Oracle of its own (tests/batch_ragged_cases.py): status, pivot
count, objective bits, last (entering, leaving), basis, the log and the whole
tableau.

Bit parity does not depend on the update tile (every element's update is an
independent fma), so the shapes are chosen so that a wrong per-LP geometry
corrupts or misses elements: ncols below, at and between powers of two and
above 256 (where the tile's width is capped and a thread walks several
columns), row counts below the tile's height and off multiples of four times
it, both tiers and every launch group in one batch.
"""
from __future__ import annotations

import ctypes
import os
import random

import numpy as np
import pytest

import batch_cases as bc
import batch_ragged_cases as rc
from conftest import ROOT
from oracle.lpo import RULE_BLAND, RULE_DANTZIG

pytestmark = pytest.mark.gpu

RULES = [RULE_DANTZIG, RULE_BLAND]
OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT = 1, 2, 3, 4
LDS, GLOBAL = 0, 1

# 1: the LDS-tier mix, two LPs of every shape
MIX = [(1, 1), (2, 2), (5, 6), (8, 8), (12, 20), (16, 16), (33, 33), (40, 24), (37, 70), (8, 300)]
MIX2 = [s for s in MIX for _ in range(2)]
# 2: both tiers; (96, 160) takes 202648 bytes of LDS: global
TIERS = [(8, 8), (96, 160), (33, 33)]
# 8, 9: artificial LPs, the constructions of batch2_cases in two or three shapes each
ART = [(8, 8), (33, 33), (37, 70), (8, 8), (33, 33), (37, 70), (33, 33), (37, 70), (8, 8), (37, 70)]
ART_CONSTRUCTS = {1: "inconsistent", 2: "redundant", 3: "driveout", 4: "driveout", 5: "inconsistent", 6: "redundant",
                  8: "inconsistent"}


def mix_spec(rule, reverse=False, **kw):
    lps = rc.lps_of(MIX2)
    return rc.spec(lps[::-1] if reverse else lps, rule=rule, **kw)


def tiers_spec(rule=RULE_DANTZIG, **kw):
    return rc.spec(rc.lps_of(TIERS), rule=rule, **kw)


def art_spec(rule=RULE_DANTZIG, kind="art", shapes=ART, constructs=ART_CONSTRUCTS, **kw):
    return rc.spec(rc.lps_of(shapes, constructs), kind=kind, rule=rule, **kw)


def check(s, got=None):
    got = rc.run_batch(s) if got is None else got
    bc.assert_same(got, rc.run_oracle(s))
    return got


# ---- 1 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
def test_lds_tier_mix(rule):
    got = check(mix_spec(rule))
    assert (got["tier"] == LDS).all() and (got["status"] == OPTIMAL).all() and got["pivots"].min() >= 1
    assert (got["group"] == 1).all()
    assert len({rc.fit_on_a_cu(l) for l in got["lds"].tolist()}) >= 3     # one launch, LPs of several occupancies


def test_lds_tier_mix_in_reverse_order():
    """The same LPs at other places of the batch, beside other neighbours: each still equals its oracle, so LP for LP
    the bits are those of test_lds_tier_mix."""
    fwd, rev = rc.run_oracle(mix_spec(RULE_DANTZIG)), check(mix_spec(RULE_DANTZIG, reverse=True))
    assert np.array_equal(rev["pivots"], fwd["pivots"][::-1])
    assert np.array_equal(bc.bits(rev["objective"]), bc.bits(fwd["objective"])[::-1])


# ---- 2 --------------------------------------------------------------------------------------

def test_both_tiers_in_one_batch(tmp_path):
    s = tiers_spec()
    got = check(s)
    assert got["tier"].tolist() == [LDS, GLOBAL, LDS] and got["group"][1] == 0
    assert got["lds"].tolist() == [rc.lds_bytes(8, 17), 8 * (257 + 97), rc.lds_bytes(33, 67)]
    forced = rc.in_subprocess([s], {"LPG_BATCH_TIER": "global"}, tmp_path)[0]
    assert forced["tier"].tolist() == [GLOBAL] * 3 and (forced["group"] == 0).all()
    bc.assert_same(forced, rc.run_oracle(s))


# ---- 3 --------------------------------------------------------------------------------------

# One launch per tier: the LDS-tier LPs share a launch whose dynamic LDS is that of the largest of them, whatever
# their own size. lds_bytes just below / just above 160 KiB / k, the sizes at which another workgroup fits on a CU:
# k = 1 (163824, 164032: over the 150 KiB cap, so global; and 153544, the largest under the cap), k = 2 (81888, 81952),
# k = 4 (40960, 40976), k = 8 (20480, 20488)
GROUPS = [(109, 73), (91, 126), (108, 64), (61, 99), (67, 78), (50, 46), (48, 51), (39, 20), (39, 21), (8, 8)]
GROUP_LDS = [163824, 164032, 153544, 81888, 81952, 40960, 40976, 20480, 20488]


def test_launch_groups():
    assert [rc.lds_bytes(m, n + m + 1) for m, n in GROUPS[:-1]] == GROUP_LDS
    s = rc.spec(rc.lps_of(GROUPS))
    got = check(s)
    want_tier = [GLOBAL if rc.lds_bytes(m, n + m + 1) > rc.LDS_CAP else LDS for m, n in GROUPS]
    assert got["tier"].tolist() == want_tier == [GLOBAL, GLOBAL] + [LDS] * 8
    assert got["lds"][2:].tolist() == [rc.lds_bytes(m, n + m + 1) for m, n in GROUPS[2:]]
    assert got["group"].tolist() == [rc.group_of(l, t) for l, t in zip(got["lds"].tolist(), want_tier)]
    assert got["group"].tolist() == [0, 0] + [1] * 8
    assert [rc.fit_on_a_cu(l) for l in got["lds"][2:].tolist()] == [1, 2, 1, 4, 3, 8, 7, 8]


# ---- 4 --------------------------------------------------------------------------------------

def test_600_lps_of_random_shapes():
    rnd = random.Random(20220518)
    shapes = [(rnd.randint(1, 40), rnd.randint(1, 40)) for _ in range(600)]
    got = check(rc.spec(rc.lps_of(shapes)))
    assert len(set(shapes)) > 200 and len({rc.fit_on_a_cu(l) for l in got["lds"].tolist()}) >= 3


# ---- 5 --------------------------------------------------------------------------------------

OUTCOMES = {0: "ray", 3: "optimal", 7: "ray", 10: "optimal", 13: "ray", 18: "optimal"}


def test_mixed_outcomes_and_two_calls_equal_one():
    lps = rc.lps_of(MIX2, OUTCOMES)
    short = check(rc.spec(lps, budgets=[7]))
    assert {UNBOUNDED, OPTIMAL, ITER_LIMIT} == set(short["status"].tolist())
    assert all(short["status"][q] == (UNBOUNDED if c == "ray" else OPTIMAL) for q, c in OUTCOMES.items())
    assert (short["pivots"][[3, 10, 18]] == 0).all() and short["pivots"].max() == 7
    two, one = check(rc.spec(lps, budgets=[7, 20000])), check(rc.spec(lps, budgets=[20007]))
    assert ITER_LIMIT in two["calls"][0] and ITER_LIMIT not in two["calls"][1]
    for key in ("status", "pivots", "entering", "leaving", "basis", "loglen", "logk", "logr"):
        assert np.array_equal(two[key], one[key]), key
    assert np.array_equal(bc.bits(two["rows"]), bc.bits(one["rows"]))
    # only the default capacity, 2 * (max m + max ncols), was used, and some LP filled more than its own shape's
    assert two["logcap"] == 2 * (40 + 309) and two["loglen"].max() <= two["logcap"]


# ---- 6 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [1, 3])
def test_small_chunks(chunk, tmp_path):
    specs = [mix_spec(RULE_DANTZIG), tiers_spec(), art_spec(cost="explicit"), art_spec(RULE_BLAND, budgets=[9, 20000])]
    for s, got in zip(specs, rc.in_subprocess(specs, {"LPG_BATCH_CHUNK": str(chunk)}, tmp_path)):
        assert got["chunk"] == chunk
        bc.assert_same(got, rc.run_oracle(s))


# ---- 7 --------------------------------------------------------------------------------------

DUAL = [(5, 6), (12, 20), (40, 24), (96, 160)]


def test_dual():
    got = check(rc.spec(rc.lps_of(DUAL), kind="dual"))
    assert got["tier"].tolist() == [LDS, LDS, LDS, GLOBAL] and got["pivots"].min() >= 1


def test_dual_refusal_names_the_batch_index():
    """LP 0 is not dual feasible. The global-tier LP 3 is launched first and the LDS-tier LPs by descending size, the
    smallest of them, LP 0, last: its place in the launches is 2 of group 1, its index 0."""
    import linearprogramming_amd as lpg
    s = rc.spec(rc.lps_of(DUAL, {0: "dual_infeasible"}), kind="dual")
    e = rc.engine_for(s)
    try:
        before = e.get_rows()
        assert [e.shape(q).group for q in range(4)] == [1, 1, 1, 0]
        with pytest.raises(lpg.LPGError, match=r"lpg_batch_solve_dual rc=-4: .*LP 0 is not dual feasible.*nothing has pivoted"):
            e.solve_dual()
        assert all(np.array_equal(bc.bits(a), bc.bits(b)) for a, b in zip(before, e.get_rows()))
        assert all(len(e.get_log(q)[0]) == 0 for q in range(4))
    finally:
        e.close()
    s = rc.spec(rc.lps_of(DUAL, {2: "dual_infeasible"}), kind="dual")
    e = rc.engine_for(s)
    try:
        with pytest.raises(lpg.LPGError, match=r"rc=-4: .*LP 2 is not dual feasible"):
            e.solve_dual()
    finally:
        e.close()


# ---- 8 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("cost", ["none", "explicit"])
def test_two_phase(rule, cost):
    got = check(art_spec(rule, cost=cost))
    st = got["status"].tolist()
    assert all(st[q] == INFEASIBLE for q, c in ART_CONSTRUCTS.items() if c == "inconsistent")
    assert st.count(OPTIMAL) >= 3 and st[3] == OPTIMAL       # the (8, 8) LP whose artificials are driven out
    # a redundant row keeps its artificial basic: LPs 2 (37, 70) and 6 (33, 33)
    bas = np.split(got["basis"], np.cumsum([m for m, _ in ART])[:-1])
    for q in (2, 6):
        m, n = ART[q]
        assert (bas[q] >= rc.art_first_of(m, n)).sum() == 1


def test_two_phase_budget_limited_call_is_continued():
    got = check(art_spec(budgets=[9, 20000]))
    assert ITER_LIMIT in got["calls"][0] and ITER_LIMIT not in got["calls"][1]


def test_two_phase_then_primal_prices_each_lps_own_real_columns():
    """After the two-phase call LP q's active columns are 1..art_first[q]-1: new costs and a plain solve then do what
    the oracle does after its own two-phase call, which leaves the same columns active."""
    from oracle.lpo import Oracle
    shapes = ART[:3]
    s = art_spec(shapes=shapes, constructs={})
    costs = [np.array([((5 * q + 2 * j) % 7) - 3.0 if j < n else 0.0 for j in range(n + m)])   # of both signs
             for q, (m, n) in enumerate(shapes)]
    e = rc.engine_for(s)
    try:
        rc.solve_fn(e, s)(20000)
        e.set_objective(costs)
        got, rows, bas = e.solve(20000, RULE_DANTZIG), e.get_rows(), e.get_basis()
    finally:
        e.close()
    more = 0
    for q, (m, n) in enumerate(shapes):
        T, basis = rc.build_lp(s, q)
        o = Oracle(m, n + m + 1)
        o.load_tableau(T, basis)
        first = o.solve_two_phase(rc.art_first_of(m, n), None, 20000, RULE_DANTZIG)
        o.set_objective(costs[q].copy())
        want = o.solve(20000, RULE_DANTZIG)
        more += want.pivots - first.pivots
        assert (got[q].status, got[q].pivots) == (want.status, want.pivots), q
        assert np.array_equal(bc.bits(rows[q]), bc.bits(o.get_rows())) and np.array_equal(bas[q], o.get_basis()), q
        o.close()
    assert more >= 3                                           # the new costs made the LPs pivot again


# ---- 9 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
def test_big_m(rule):
    check(art_spec(rule, kind="bigm", cost="explicit"))
    check(art_spec(rule, kind="bigm", budgets=[9, 20000]))


def test_big_m_tier_boundary_per_lp():
    """(95, 95) with its two objective rows takes 150904 bytes: LDS; (96, 96) takes 154024: global."""
    got = check(art_spec(kind="bigm", shapes=[(8, 8), (95, 95), (96, 96)], constructs={}))
    assert got["lds"][1] == rc.lds_bytes(95, 191, 2) == 150904 and rc.lds_bytes(96, 193, 2) == 154024
    assert got["tier"].tolist() == [LDS, LDS, GLOBAL] and got["group"].tolist() == [1, 1, 0]


# ---- 10 -------------------------------------------------------------------------------------

def test_one_shape_equals_the_uniform_batch():
    u = bc.spec(12, 20, B=6)
    uni = bc.run_batch(u)
    s = rc.spec([[12, 20, bc.SEED + b, None] for b in range(6)], budgets=u["budgets"])
    got = rc.run_batch(s)
    for key in ("status", "pivots", "entering", "leaving", "loglen", "logk", "logr", "logcap", "calls"):
        assert np.array_equal(got[key], uni[key]), key
    assert np.array_equal(bc.bits(got["objective"]), bc.bits(uni["objective"]))
    assert np.array_equal(bc.bits(got["rows"]), bc.bits(uni["rows"]).ravel())
    assert np.array_equal(got["basis"], uni["basis"].ravel())


def test_layout_refusals_in_both_directions():
    import linearprogramming_amd as lpg
    from linearprogramming_amd import _lib as L
    lib = L.load()
    res = (L.Result * 2)()
    d = np.zeros(4096)
    i64 = np.full(64, 2, dtype=np.int64)
    dp, ip = d.ctypes.data_as(L.c_double_p), i64.ctypes.data_as(L.c_int64_p)
    shp = L.BatchShape()

    def refused(b, rc_, *words):
        msg = lib.lpg_batch_last_error(b).decode()
        assert rc_ == L.ERR_STATE and all(w in msg for w in words), (rc_, msg)

    s = rc.spec(rc.lps_of([(5, 6), (8, 8)]), kind="art")
    for big_m in (False, True):
        s["kind"] = "bigm" if big_m else "art"
        e = rc.engine_for(s)
        try:
            before = e.get_rows()
            b = e._b
            refused(b, lib.lpg_batch_load(b, 0, 1, dp, 64, None), "ragged", "lpg_batch_load_packed")
            refused(b, lib.lpg_batch_get_rows(b, 0, 1, dp, 64), "ragged", "lpg_batch_get_rows_packed")
            refused(b, lib.lpg_batch_get_basis(b, 0, 1, ip), "ragged", "lpg_batch_get_basis_packed")
            refused(b, lib.lpg_batch_generate_artificial(b, 6, 1, None), "ragged", "no generator")
            if big_m:
                refused(b, lib.lpg_batch_solve_big_m(b, 9, None, 0, 10, 0, res), "ragged", "lpg_batch_solve_big_m_ragged")
            else:
                refused(b, lib.lpg_batch_set_objective(b, dp, 64), "ragged", "lpg_batch_set_objective_packed")
                refused(b, lib.lpg_batch_set_active_columns(b, 3), "ragged", "per LP")
                refused(b, lib.lpg_batch_generate(b, 6, 1, 0), "ragged", "no generator")
                refused(b, lib.lpg_batch_solve_two_phase(b, 9, None, 0, 10, 0, res), "ragged",
                        "lpg_batch_solve_two_phase_ragged")
            assert all(np.array_equal(bc.bits(x), bc.bits(y)) for x, y in zip(before, e.get_rows()))
            assert all(len(e.get_log(q)[0]) == 0 for q in range(2))
            assert e.info.pad == 1 and (e.info.m, e.info.ncols, e.info.ld) == (8, 17, 64)
            assert e.info.lds_bytes == max(e.shape(q).lds_bytes for q in range(2))
        finally:
            e.close()
        with lpg.BatchEngine(2, 5, 12, big_m=big_m) as u:
            u.generate_artificial(6)
            before = u.get_rows()
            b = u._b
            refused(b, lib.lpg_batch_shape(b, 0, ctypes.byref(shp)), "one shape", "lpg_batch_info")
            refused(b, lib.lpg_batch_load_packed(b, 0, 1, dp, None), "one shape", "lpg_batch_load")
            refused(b, lib.lpg_batch_get_rows_packed(b, 0, 1, dp), "one shape", "lpg_batch_get_rows")
            refused(b, lib.lpg_batch_get_basis_packed(b, 0, 1, ip), "one shape", "lpg_batch_get_basis")
            if big_m:
                refused(b, lib.lpg_batch_solve_big_m_ragged(b, ip, None, 10, 0, res), "one shape", "lpg_batch_solve_big_m")
            else:
                refused(b, lib.lpg_batch_set_objective_packed(b, dp), "one shape", "lpg_batch_set_objective")
                refused(b, lib.lpg_batch_solve_two_phase_ragged(b, ip, None, 10, 0, res), "one shape",
                        "lpg_batch_solve_two_phase")
            assert np.array_equal(bc.bits(before), bc.bits(u.get_rows()))
            assert u.info.pad == 0


def test_host_side_validation_on_a_live_ragged_batch():
    import linearprogramming_amd as lpg
    s = art_spec(shapes=ART[:3], constructs={})
    e = rc.engine_for(s)
    try:
        before = e.get_rows()
        with pytest.raises(lpg.LPGError, match=r"art_first 17 of LP 0 outside 2\.\.16"):
            e.solve_two_phase([17, 40, 60])
        with pytest.raises(lpg.LPGError, match=r"art_first 1 of LP 2 outside 2\.\.107"):
            e.solve_two_phase([16, 40, 1])
        with pytest.raises(lpg.LPGError, match="this is a ragged batch|one objective row"):
            e.solve_big_m([16, 40, 60])
        bad = [b.copy() for b in e.get_basis()]
        bad[1][4] = 67
        with pytest.raises(lpg.LPGError, match=r"basis\[4\] of LP 1 out of range 1\.\.66"):
            e.load(before, bad)
        with pytest.raises(lpg.LPGError, match="LP 1 has shape"):
            e.load([before[0], before[0], before[2]])
        with pytest.raises(lpg.LPGError, match="outside the batch"):
            e.shape(3)
        assert all(np.array_equal(bc.bits(x), bc.bits(y)) for x, y in zip(before, e.get_rows()))
    finally:
        e.close()


# ---- 11 -------------------------------------------------------------------------------------

LP_DIRS = [os.path.join(ROOT, "tests", "golden", d) for d in ("lp", "lp_extra")]
DUAL_LP = "OF {\n\tmin:z=2x1+3x2\n}\nST {\n\tx1+x2>=4;\n\tx1+3x2>=6;\n\tx1>=0;\n\tx2>=0\n}\n"
DUAL_LP3 = "OF {\n\tmin:z=x1+2x2+3x3\n}\nST {\n\tx1+x2+x3>=3;\n\tx1+2x3>=2;\n\tx2+x3<=5;\n\tx1>=0;\n\tx2>=0;\n\tx3>=0\n}\n"


def _same_solution(a, b):
    def fbits(d):
        return {k: np.float64(v).view(np.int64) for k, v in d.items()}
    return (a.status == b.status and a.pivots == b.pivots and a.method == b.method and
            np.float64(a.z).view(np.int64) == np.float64(b.z).view(np.int64) and
            list(a.columns) == list(b.columns) and fbits(a.columns) == fbits(b.columns) and
            list(a.variables) == list(b.variables) and fbits(a.variables) == fbits(b.variables))


def _models(rule, dual):
    """Every golden model build_smatrix accepts (Beale's LP cycles for good under Dantzig's rule: Bland only); dual: the
    dual-form build, where it passes solve_batch's two checks, and two small covering LPs."""
    from linearprogramming_amd import frontend as F
    texts = []
    for d in LP_DIRS:
        for name in sorted(os.listdir(d)):
            if name == "kat_beale_cycling.txt" and rule == RULE_DANTZIG:
                continue
            texts.append(open(os.path.join(d, name), "rb").read())
    if dual:
        texts += [DUAL_LP, DUAL_LP3]
    sms = []
    for text in texts:
        try:
            sm = F.build_smatrix(text, dual=dual)
        except F.FrontendError:
            continue                                           # not a model (testdata_shipped.txt)
        if dual and (F.engine_arrays(sm)[4] or any(F._dec(c) > 0 for c in sm.costs)):
            continue
        sms.append(sm)
    return sms


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("method", ["two_phase", "big_m", "dual"])
def test_solve_batch_ragged_equals_solve_batch(method, rule, monkeypatch):
    import linearprogramming_amd.engine as E
    from linearprogramming_amd import frontend as F
    sms = _models(rule, method == "dual")
    assert len(sms) >= (2 if method == "dual" else 12) and len(F.batch_groups(sms)) >= 2
    want = F.solve_batch(sms, rule, method=method)
    created = []
    real = E.RaggedBatchEngine.__init__
    monkeypatch.setattr(E.RaggedBatchEngine, "__init__", lambda self, *a, **kw: (created.append(1), real(self, *a, **kw))[1])
    got = F.solve_batch(sms, rule, method=method, ragged=True)
    assert len(created) == (1 if method == "dual" else 2)      # not one batch per shape
    assert len(got) == len(sms)
    for q, (g, w) in enumerate(zip(got, want)):
        assert _same_solution(g, w), (q, g, w)
    assert {g.method for g in got} == ({"dual"} if method == "dual" else {"primal", method})
