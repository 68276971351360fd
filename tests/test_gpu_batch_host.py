"""The host scaffold the batch families share (csrc/lpg_host.h) on the device:
one handle of each family alive at the same time, their calls interleaved, a
partial load, a reload that withdraws the results until the next solve, and
handles destroyed in another order than they were made. Every value is held
to the families' numpy statements (assign_cases, transport_cases, binary_cases)
bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

import assign_cases as ac
import binary_cases as bc
import transport_cases as tc

pytestmark = pytest.mark.gpu

# two problems each; problem 1 is later replaced by problem 0 of the *_B spec
ASSIGN_A, ASSIGN_B = ac.spec(2, 3, kinds=("int3", "int49")), ac.spec(2, 3, seed=1, kinds=("frac",))
# from the northwest corner, so that these small problems take iterations
TRANSPORT_A = tc.spec(2, 3, start=tc.NORTHWEST, kinds=("c2", "c99"))
TRANSPORT_B = tc.spec(2, 3, start=tc.NORTHWEST, seed=3, kinds=("big",))
BINARY_A, BINARY_B = bc.spec(2, 3, split=1, kinds=("mixed", "knapsack")), bc.spec(2, 3, seed=1, split=1, kinds=("cover",))


def assign_got(a):
    res = a.solve()
    col, u, v = a.get()
    return {"status": np.array([r.status for r in res]), "steps": np.array([r.steps for r in res]),
            "objective": np.array([r.objective for r in res]), "col": col, "u": u, "v": v}


def transport_got(t):
    res = t.solve()
    x, u, v, basis = t.get()
    return {"status": np.array([r.status for r in res]), "iterations": np.array([r.iterations for r in res]),
            "objective": np.array([r.objective for r in res]), "x": x, "u": u, "v": v, "basis": basis}


def binary_got(b):
    return bc.results_of(b.solve(), b.get())


def replaced(first, second):
    """The references of `first` with problem 1 replaced by problem 0 of `second`."""
    return [first[0], second[0]]


def test_three_families_side_by_side_partial_loads_reloads_and_teardown_in_any_order():
    import linearprogramming_amd as lpg
    L = lpg._lib
    a, t, b = lpg.AssignmentBatch(2, 2, 3), lpg.TransportBatch(2, 2, 3, start=tc.NORTHWEST), lpg.BinaryBatch(2, 2, 3, split=1)
    try:
        aC, (tC, tS, tD), bD = ac.costs_of(ASSIGN_A), tc.data_of(TRANSPORT_A), bc.data_of(BINARY_A)
        # problem 1 alone: the batch is not loaded, and solve names the problem that is missing
        a.load(aC[1:], first=1)
        t.load(tC[1:], tS[1:], tD[1:], first=1)
        b.load(*(x[1:] for x in bD), first=1)
        for h, call, what in ((a, "lpg_assign_solve", "costs"), (t, "lpg_transport_solve", "data"),
                              (b, "lpg_binary_solve", "data")):
            with pytest.raises(lpg.LPGError, match=rf"{call} rc={L.ERR_STATE}: {call}: problem 0 has no {what} yet"):
                h.solve()
        b.load(*(x[:1] for x in bD))
        a.load(aC[:1])
        t.load(tC[:1], tS[:1], tD[:1])
        # solve and get, interleaved
        ares = a.solve()
        got_t = transport_got(t)
        bres = b.solve()
        col, u, v = a.get()
        got_b = bc.results_of(bres, b.get())
        got_a = {"status": np.array([r.status for r in ares]), "steps": np.array([r.steps for r in ares]),
                 "objective": np.array([r.objective for r in ares]), "col": col, "u": u, "v": v}
        ac.assert_same(got_a, ac.stacked(ac.reference(ASSIGN_A)), "assign")
        tc.assert_same(got_t, tc.stacked(tc.reference(TRANSPORT_A)), "transport")
        bc.assert_same(got_b, bc.stacked(bc.reference(BINARY_A)), "binary")
        assert a.info.kernel_ms > 0.0 and t.info.kernel_ms > 0.0 and b.info.kernel_ms > 0.0
        assert t.info.launches >= 1 and b.info.launches >= 1

        # one problem of each reloaded: no results until the next solve
        a.load(ac.costs_of(ASSIGN_B), first=1)
        t.load(*tc.data_of(TRANSPORT_B), first=1)
        b.load(*bc.data_of(BINARY_B), first=1)
        for h, call in ((a, "lpg_assign_get"), (t, "lpg_transport_get"), (b, "lpg_binary_get")):
            with pytest.raises(lpg.LPGError, match=rf"{call} rc={L.ERR_STATE}: {call}: no solve since the last load or generate"):
                h.get()
        tc.assert_same(transport_got(t), tc.stacked(replaced(tc.reference(TRANSPORT_A), tc.reference(TRANSPORT_B))),
                       "transport, reloaded")
        bc.assert_same(binary_got(b), bc.stacked(replaced(bc.reference(BINARY_A), bc.reference(BINARY_B))), "binary, reloaded")
        ac.assert_same(assign_got(a), ac.stacked(replaced(ac.reference(ASSIGN_A), ac.reference(ASSIGN_B))), "assign, reloaded")
    finally:
        t.close()                                    # not the order they were made in
        a.close()
        b.close()
    # and a batch made after the others are gone
    with lpg.AssignmentBatch(2, 2, 3) as again:
        again.load(ac.costs_of(ASSIGN_A))
        ac.assert_same(assign_got(again), ac.stacked(ac.reference(ASSIGN_A)), "assign, after the teardown")
