"""jsp_place_sticky on the GPU against the rule restated over the CPU oracle
(tests/sticky_ref.py; it never calls the engine). Every comparison is exact.
Cases with at most 1,024 jobs run in both keep forms (the one-workgroup form
and, forced by the sticky_grid hook, the grid form; above 1,024 jobs only the
grid form exists). The multi-level cases also run with set_fused(False), so
that the GPU walkers and, from 256 jobs on, the host walk fill."""
import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import JobClass, Nodes, Problem, Topology, shard_problem
from oracle import oracle as O
from sticky_ref import (check_sticky, greedy_keep, scenario_cfg2, scenario_cfg4, scenario_cfg5, sticky_ref,
                        taint_rows)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["one", "grid"])
def form(request, monkeypatch):
    """The keep form: the hook string is read again at every snapshot upload."""
    if request.param == "grid":
        monkeypatch.setenv("JSP_TEST_HOOKS", "sticky_grid=1")
    else:
        monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    return request.param


@pytest.fixture(params=[True, False], ids=["auto", "gpu-walk"])
def fused(request, engine):
    engine.set_fused(request.param)
    yield request.param
    engine.set_fused(True)


def run(engine, p, prev):
    """Load p, place sticky, compare with the yardstick. Returns (assign, kept, stats)."""
    engine.load(p)
    tl = O.place_c(p)[1:]
    want, kept = sticky_ref(p, prev, tl)
    got, st = engine.place_sticky(p.job_class, prev)
    np.testing.assert_array_equal(got, want)
    check_sticky(p, prev, got, tl)
    assert st.jobs == p.n_jobs
    assert st.kept == int(kept.sum())
    assert st.placed == int((want >= 0).sum())
    assert st.hinted == (0 if prev is None else int((np.asarray(prev) >= 0).sum()))
    assert np.all(got[kept] == np.asarray(prev)[kept]) if prev is not None else not kept.any()
    return got, kept, st


def flat(rows_per_leaf, classes, job_class, taints=None, excl=None):
    """A one-level problem: leaf l has rows_per_leaf[l] rows with one free unit each."""
    return nested([np.arange(len(rows_per_leaf) + 1)], rows_per_leaf, classes, job_class, taints, excl)


def nested(first_leaf, rows_per_leaf, classes, job_class, taints=None, excl=None):
    sizes = np.asarray(rows_per_leaf, dtype=np.int64)
    L, N = sizes.shape[0], int(sizes.sum())
    fl = [np.asarray(f, dtype=np.uint32) for f in first_leaf]
    topo = Topology(level_keys=[f"example.com/l{k}" for k in range(len(fl))], n_domains=[f.shape[0] - 1 for f in fl],
                    first_leaf=fl)
    topo.validate()
    ls = np.zeros(L + 1, dtype=np.uint32)
    np.cumsum(sizes, out=ls[1:])
    nodes = Nodes(leaf_start=ls, labels=np.ones((1, N), dtype=np.uint64),
                  taints=np.zeros(N, dtype=np.uint32) if taints is None else np.asarray(taints, dtype=np.uint32),
                  free=np.ones((1, N), dtype=np.uint32),
                  excl=np.full(N, -1, dtype=np.int32) if excl is None else np.asarray(excl, dtype=np.int32))
    return Problem(topology=topo, nodes=nodes, classes=classes, job_class=np.asarray(job_class, dtype=np.uint32))


def cls(level, pods, tol=0):
    return JobClass(req_labels=(1,), tolerated_taints=tol, level=level, pods=pods, req_res=(1,))


# ------------------------------------------------------------------ 1. one level, L = 3, J = 5
def test_two_jobs_hint_one_domain(engine, form):
    p = flat([2, 2, 2], [cls(0, 2)], [0] * 5)
    got, kept, _ = run(engine, p, [1, 1, -1, -1, -1])
    np.testing.assert_array_equal(kept, [True, False, False, False, False])
    np.testing.assert_array_equal(got, [1, 0, 2, -1, -1])  # the lower index keeps; the loser is an ordinary job


def test_occupied_or_short_hint_is_no_claim(engine, form):
    taints = [0, 0, 0, 0, 0, 1]         # leaf 2 is one row short for a class that tolerates nothing
    excl = [77, 77, -1, -1, -1, -1]     # leaf 0 is held by another exclusive job
    p = flat([2, 2, 2], [cls(0, 2)], [0] * 5, taints, excl)
    got, kept, st = run(engine, p, [0, 2, -1, 1, -1])
    np.testing.assert_array_equal(kept, [False, False, False, True, False])
    np.testing.assert_array_equal(got, [-1, -1, -1, 1, -1])
    assert (st.hinted, st.kept, st.placed) == (3, 1, 1)


def test_infeasible_hint_of_one_class_leaves_the_domain_to_another(engine, form):
    taints = [0, 0, 1, 1, 0, 0]         # leaf 1 is feasible only for the tolerant class 1
    p = flat([2, 2, 2], [cls(0, 2), cls(0, 2, tol=1)], [0, 1, 0, 1, 0], taints)
    got, kept, _ = run(engine, p, [1, 1, -1, -1, -1])
    np.testing.assert_array_equal(kept, [False, True, False, False, False])
    np.testing.assert_array_equal(got, [0, 1, 2, -1, -1])


# ------------------------------------------------------------------ 2. word edges
@pytest.mark.parametrize("D", [64, 65, 129])
def test_word_edges(engine, form, D):
    hints = [d for d in (128, 64, 63, 0) if d < D]
    p = flat([1] * D, [cls(0, 1)], [0] * (D + 2))
    taint_rows(p, [1, 5], 1)
    prev = np.full(D + 2, -1, dtype=np.int32)
    prev[2:2 + len(hints)] = hints
    got, kept, _ = run(engine, p, prev)
    assert int(kept.sum()) == len(hints)
    assert sorted(got[got >= 0].tolist()) == [d for d in range(D) if d not in (1, 5)]


# ------------------------------------------------------------------ 3. nested hierarchies
def tree8():
    """2 zones x 2 racks x 2 leaves, one row per leaf; a zone job needs its 4 rows, a rack job 2, a leaf job 1."""
    return [np.array([0, 4, 8]), np.array([0, 2, 4, 6, 8]), np.arange(9)], [cls(0, 4), cls(1, 2), cls(2, 1)]


def test_ancestor_hint_before_descendant(engine, form, fused):
    fl, classes = tree8()
    p = nested(fl, [1] * 8, classes, [0, 1, 2, 1, 2])
    got, kept, _ = run(engine, p, [0, 0, 1, -1, -1])   # zone 0, then rack 0 and leaf 1 inside it
    np.testing.assert_array_equal(kept, [True, False, False, False, False])
    np.testing.assert_array_equal(got, [0, 2, 6, -1, 7])


def test_descendant_hint_before_ancestor(engine, form, fused):
    fl, classes = tree8()
    p = nested(fl, [1] * 8, classes, [2, 1, 0, 0, 2])
    got, kept, _ = run(engine, p, [5, 3, 1, -1, -1])   # leaf 5, then rack 3, then zone 1 above both
    np.testing.assert_array_equal(kept, [True, True, False, False, False])
    np.testing.assert_array_equal(got, [5, 3, 0, -1, 4])


def test_chain_pins_the_order_free_rule(engine, form, fused):
    """j0 hints rack 2 in zone 1, j1 hints zone 1, j2 hints rack 3 in zone 1: only j0 keeps. j2 is blocked
    by the claimant j1 although j1 loses -- the sequential greedy would keep j2."""
    fl, classes = tree8()
    p = nested(fl, [1] * 8, classes, [1, 0, 1, 2])
    prev = [2, 1, 3, -1]
    got, kept, _ = run(engine, p, prev)
    np.testing.assert_array_equal(kept, [True, False, False, False])
    np.testing.assert_array_equal(greedy_keep(p, prev), [True, False, True, False])
    np.testing.assert_array_equal(got, [2, 0, 3, -1])  # the fill hands j2 the free rack 3 anyway


@pytest.mark.parametrize("zone_first", [True, False])
def test_zone_keeper_spans_words(engine, form, fused, zone_first):
    """3 zones x 100 racks: zone 1 is racks 100..199, bits in three 64-bit words of every rack class.
    300 jobs, so AUTO fills on the host and OFF on the GPU."""
    Z, RZ = 3, 100
    fl = [np.arange(Z + 1) * RZ, np.arange(Z * RZ + 1)]
    classes = [cls(0, RZ), cls(1, 1), cls(1, 1, tol=1)]
    jc = np.array([1, 2] * 150, dtype=np.uint32)
    jc[7] = 0
    p = nested(fl, [1] * (Z * RZ), classes, jc)
    taint_rows(p, [3, 64, 250], 1)
    prev = np.full(300, -1, dtype=np.int32)
    prev[7] = 1
    prev[[20, 21, 40]] = [150, 99, 200]
    if not zone_first:
        prev[2] = 163                       # a rack claim in zone 1 below the zone job's index
    got, kept, _ = run(engine, p, prev)
    assert bool(kept[7]) == zone_first
    if zone_first:
        assert not ((got[jc != 0] >= 100) & (got[jc != 0] < 200)).any()
        assert not kept[20] and kept[21] and kept[40]


# ------------------------------------------------------------------ 4. runs
def test_runs_all_kept_and_keepers_in_the_middle(engine, form):
    p = flat([1] * 12, [cls(0, 1), cls(0, 1, tol=1)], [0, 0, 0, 1, 1, 0, 0, 0, 0, 1])
    prev = [-1, -1, -1, 7, 3, -1, 9, 2, -1, -1]   # run 1 (jobs 3, 4) is all kept; run 2 keeps in its middle
    got, kept, st = run(engine, p, prev)
    np.testing.assert_array_equal(kept, np.asarray(prev) >= 0)
    np.testing.assert_array_equal(got, [0, 1, 4, 7, 3, 5, 9, 2, 6, 8])
    assert st.runs == 4


def test_empty_batch_null_prev_and_bad_hint(engine, form):
    p = flat([1] * 6, [cls(0, 1)], [0] * 4)
    run(engine, p, None)
    got, st = engine.place_sticky(np.zeros(0, dtype=np.uint32), None)
    assert got.shape == (0,) and (st.jobs, st.placed, st.kept) == (0, 0, 0)
    got, st = engine.place_sticky_runs(np.array([0, 0], dtype=np.uint32), np.array([0, 2], dtype=np.uint32), [4, -1])
    np.testing.assert_array_equal(got, [4, 0])   # an empty run in the call's list
    for bad in (6, -2):
        with pytest.raises(native.JspError) as ei:
            engine.place_sticky(p.job_class, [-1, -1, bad, -1])
        assert ei.value.code == native.JSP_EINVAL and "job 2" in str(ei.value)
    np.testing.assert_array_equal(engine.place_sticky(p.job_class, [5, -1, -1, -1])[0], [5, 0, 1, 2])


def test_device_set_sharded_and_unloaded_engines_are_estate():
    p = synth.config5()

    def refused(e, word):
        with pytest.raises(native.JspError) as ei:
            e.place_sticky(p.job_class, None)
        assert ei.value.code == native.JSP_ESTATE, str(ei.value)
        assert word in str(ei.value), str(ei.value)

    with Engine(devices=[0, 0]) as multi:
        multi.load(p)
        refused(multi, "device-set")
    with Engine(0) as e:
        e.upload_topology(p.topology)
        e.upload_snapshot(shard_problem(p, 0, 2))
        e.upload_classes(p.classes)
        refused(e, "sharded")
    lib = native.lib()
    with Engine(0) as e:
        a = np.zeros(1, dtype=np.int32)
        one, zero = np.ones(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        call = lambda: lib.jsp_place_sticky(e._h, zero.ctypes.data, one.ctypes.data, 1, None,  # noqa: E731
                                            a.ctypes.data, None)
        assert call() == native.JSP_ESTATE               # no topology yet
        e.upload_topology(p.topology)
        assert call() == native.JSP_ESTATE               # no snapshot yet
        e.upload_snapshot(p.nodes)
        assert call() == native.JSP_ESTATE               # no classes yet
        e.upload_classes(p.classes)
        assert call() == native.JSP_OK


def test_sticky_loop_leaves_the_last_answer(engine):
    p = flat([1] * 6, [cls(0, 1)], [0] * 4)
    engine.load(p)
    rc, rl = np.zeros(1, dtype=np.uint32), np.full(1, 4, dtype=np.uint32)
    prev = [-1, 4, -1, -1]
    total, median, p99 = engine.place_sticky_loop(rc, rl, prev, iters=5)
    assert 0 < median <= p99 <= total
    want, kept = sticky_ref(p, prev)
    np.testing.assert_array_equal(kept, [False, True, False, False])
    got, st = engine.place_sticky_runs(rc, rl, prev)   # the engine stays usable, and answers as before
    np.testing.assert_array_equal(got, want)
    assert (st.jobs, st.kept, st.placed) == (4, 1, 4)


# ------------------------------------------------------------------ 5. the scan across workgroups
@pytest.mark.parametrize("n_classes", [1, 2])
def test_scan_across_workgroups(engine, fused, n_classes):
    """5,000 jobs over 300 leaves; 250 hinted jobs at indices 0, 20, 40, ... keep while the unhinted jobs
    before them fill the other 50 leaves. One class: the level walker; two (100 runs): the generic
    GPU walker or the host walk."""
    J, L = 5000, 300
    classes = [cls(0, 1), cls(0, 1, tol=1)][:n_classes]
    jc = (np.arange(J) // 50 % n_classes).astype(np.uint32)
    p = flat([1] * L, classes, jc)
    prev = np.full(J, -1, dtype=np.int32)
    prev[np.arange(250) * 20] = L - 1 - np.arange(250)
    got, kept, st = run(engine, p, prev)
    assert st.kept == 250 and st.placed == 300
    assert got[0] == 299 and got[4980] == 50     # the first and the last hinted job keep
    assert got[1] == 0                            # the unhinted jobs before them fill the low leaves


# ------------------------------------------------------------------ 6. random sweep
@pytest.mark.parametrize("seed", range(24))
def test_random_sweep(engine, form, fused, seed):
    p = synth.random_problem(seed, max_nodes=600, max_leaves=40)
    before = O.place_c(p)[0].copy()
    N = p.nodes.n_nodes
    taint_rows(p, np.nonzero(synth.bernoulli(seed, 7002, N, 0.10))[0], 1 << 20)   # a taint no class tolerates
    run(engine, p, before)
    lvl = np.array([p.classes[int(c)].level for c in p.job_class], dtype=np.int64)
    nd = np.array(p.topology.n_domains, dtype=np.int64)[lvl] if p.n_jobs else np.zeros(0, dtype=np.int64)
    run(engine, p, (synth.uniform_int(seed, 7001, p.n_jobs, 0, 1 << 30) % np.maximum(nd, 1)).astype(np.int32))


# ------------------------------------------------------------------ 7. the scenarios of DESIGN.md §4
def differs(prev, got):
    return int(((prev >= 0) & (got != prev)).sum())


def test_scenario_cfg2(engine, form):
    p, prev = scenario_cfg2()
    got, kept, st = run(engine, p, prev)
    assert differs(prev, got) == 1 and st.kept == 989
    assert differs(prev, O.place_c(p)[0]) == 985   # what the lowest-index rule alone moves


def test_scenario_cfg5(engine, form, fused):
    p, prev = scenario_cfg5()
    got, kept, st = run(engine, p, prev)
    assert differs(prev, got) == 1
    assert st.fused == (7 if fused else 0)


def test_scenario_cfg4_reduced(engine):
    p, prev = scenario_cfg4()
    got, kept, st = run(engine, p, prev)
    assert differs(prev, got) == 3


def test_scenario_cfg4_wide_level_walker(engine):
    """20,000 domains: 313 words per class, the 1,024-thread level walker fills."""
    p, prev = scenario_cfg4(262_144, 20_000)
    got, kept, st = run(engine, p, prev)
    assert differs(prev, got) == 3 and st.fused == 0


# ------------------------------------------------------------------ 8. service and patches
def test_service_patch_then_sticky(engine, form):
    engine.set_service(True)
    engine.set_fused(True)
    try:
        p = synth.config2()
        engine.load(p)
        prev = O.place_c(p)[0].copy()
        for _ in range(4):
            if engine.place(p.job_class).fused == 3:
                break
        assert engine.place(p.job_class).fused == 3
        m0 = engine.metrics()
        r = int(prev[5])
        row = next(n for n in range(r * 15, r * 15 + 15) if p.nodes.taints[n] == 0)
        engine.patch_rows(np.array([row], dtype=np.uint32), taints=np.array([1], dtype=np.uint32))
        got, st = engine.place_sticky(p.job_class, prev)        # at once: ordered after the patch
        p.nodes.taints[row] = 1
        want, kept = sticky_ref(p, prev)
        np.testing.assert_array_equal(got, want)
        assert got[5] != prev[5] and st.kept == 989
        m1 = engine.metrics()
        assert m1.place_us.count == m0.place_us.count + 1 and m1.batch_jobs.count == m0.batch_jobs.count + 1
        assert m1.placed == m0.placed + st.placed and m1.unplaceable == m0.unplaceable + (st.jobs - st.placed)
        after = engine.place(p.job_class)                       # the service kept its tiles
        assert after.fused == 3
        np.testing.assert_array_equal(after.assign, O.place_c(p)[0])
        with pytest.raises(native.JspError):
            engine.place_sticky(p.job_class, np.full(p.n_jobs, 1000, dtype=np.int32))
        assert engine.metrics().place_errors == m1.place_errors + 1
    finally:
        engine.service_stop()
