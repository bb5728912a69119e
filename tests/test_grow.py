"""CPU tests of grow placement (DESIGN.md §2 "Grow placement"): hand cases of the plan, the host's budgeted walk
(jsp_walk.cc walk_grow) on the reference's lists against the reference's O(J D) walk, and the two reductions."""
import ctypes
import dataclasses

import numpy as np
import pytest

from jobset_amd import native
from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from grow_ref import CASES, NO_LIMIT, domain_table, grow_ref, plan, table_ref


@pytest.mark.parametrize("tc,ma,rem,want", [
    ([3, 5, 5, 2], [2, 1, 2, 9], 14, (True, [(1, 1), (2, 2)])),           # ties: the finishing leaf partial
    ([3, 5, 5, 2], [2, 1, 1, 9], 14, (True, [(1, 1), (2, 1), (0, 2)])),   # falls through to a smaller template
    ([2, 2], [1, 1], 4, (True, [(0, 1), (1, 1)])),                         # covered exactly
    ([2, 2], [1, 1], 5, (False, [(0, 1), (1, 1)])),                        # one short
    ([0, 4], [9, 0], 1, (False, [])),                                      # tcap 0, max_add 0
    ([65536], [65536], (1 << 32) - 1, (True, [(0, 65536)])),               # the product is 2^32
    ([7], [3], 0, (True, [])),
])
def test_plan_by_hand(tc, ma, rem, want):
    assert plan(tc, ma, rem) == want


def walk(p, tab, budget):
    """jspi_grow_walk_test on the reference's lists: (assign, need, totals)."""
    order, nf, need, _ = table_ref(p, None, tab)
    fn = native.lib().jspi_grow_walk_test
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    fn.restype, fn.argtypes = ctypes.c_int, [u32, vp, vp, u32, vp, vp, vp, vp, vp, ctypes.c_uint64, vp, vp, u32, vp, vp, vp]
    topo = p.topology
    K = topo.n_levels
    D = (u32 * 4)(*([topo.n_domains[k] for k in range(K)] + [0] * (4 - K)))
    fls = [np.ascontiguousarray(topo.first_leaf[k], dtype=np.uint32) for k in range(K)]
    flp = (vp * 4)(*([f.ctypes.data for f in fls] + [None] * (4 - K)))
    lv = np.array([c.level for c in p.classes], dtype=np.uint32)
    pods = np.array([c.pods for c in p.classes], dtype=np.uint32)
    rc, rl = (np.ascontiguousarray(x, dtype=np.uint32) for x in job_runs(p.job_class))
    out, nd, tot = np.full(p.n_jobs + 1, -7, dtype=np.int32), np.full(p.n_jobs + 1, 7, dtype=np.uint32), np.zeros(5, np.uint32)
    fn(K, D, flp, len(p.classes), lv.ctypes.data, pods.ctypes.data, order.ctypes.data, nf.ctypes.data, need.ctypes.data,
       (1 << 64) - 1 if budget == NO_LIMIT else budget, rc.ctypes.data, rl.ctypes.data, len(rc), out.ctypes.data,
       nd.ctypes.data, tot.ctypes.data)
    assert out[p.n_jobs] == -7 and nd[p.n_jobs] == 7, "the walk wrote behind its outputs"
    return out[:-1], nd[:-1], dict(placed=int(tot[0]), grown=int(tot[1]), over_budget=int(tot[2]),
                                   nodes=int(tot[3]) | int(tot[4]) << 32)


@pytest.mark.parametrize("case", list(CASES))
def test_host_walk_and_reductions(case):
    p, t = CASES[case]()
    tab = domain_table(p, t)
    free = grow_ref(p, t, tab=tab)
    assert free[5]["grown"] > 0 and free[5]["placed"] < p.n_jobs
    budgets = [NO_LIMIT, free[5]["nodes"] // 2, 0]
    for budget in budgets:
        a, n, off, leaf, nodes, st = grow_ref(p, t, budget, tab)
        got_a, got_n, tot = walk(p, tab, budget)
        np.testing.assert_array_equal(got_a, a)
        np.testing.assert_array_equal(got_n, n)
        assert tot == {k: st[k] for k in tot}
        assert st["nodes"] == int(nodes.astype(np.int64).sum()) == int(n.astype(np.int64).sum()) and off[-1] == leaf.shape[0]
        assert budget == NO_LIMIT or st["nodes"] <= budget
    assert grow_ref(p, t, budgets[1], tab)[5]["over_budget"] > 0
    # the reductions: no budget, or no group that can grow, is jsp_place
    place = O.place_c(p)[0]
    np.testing.assert_array_equal(grow_ref(p, t, 0, tab)[0], place)
    fixed = dataclasses.replace(t, max_add=np.zeros_like(t.max_add))
    np.testing.assert_array_equal(grow_ref(p, fixed)[0], place)
