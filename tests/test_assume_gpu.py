"""jsp_assume / jsp_forget on the GPU against the rules restated in plain numpy
(tests/assume_ref.py; it never calls the engine). The excl column is not read
back: it is observed through jsp_place with occ_out / tally_out, jsp_explain's
rows_occupied, committed_out, both calls' counts, and forgets of chosen subsets,
which pin the owner ids themselves. Every comparison is exact. Cases run in
both forms of the bind front end: the default (one wave per job for domains of
up to 256 rows, one workgroup per job above) and, forced by the bind_wg hook,
the workgroup form for every job."""
import ctypes
import dataclasses

import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import job_runs, shard_problem
from oracle import oracle as O
from assume_ref import BindConflict, assume_ref, domains_intersect, forget_ref, stats_dict
from bind_ref import bind_ref, cls, domain_rows, flat, nested
from sticky_ref import sticky_ref

pytestmark = pytest.mark.gpu

INT32_MIN = -(1 << 31)
BASE = 0x40000000


@pytest.fixture(params=["auto", "wg"])
def form(request, monkeypatch):
    """The bind form: the hook string is read again at every snapshot upload."""
    if request.param == "wg":
        monkeypatch.setenv("JSP_TEST_HOOKS", "bind_wg=1")
    else:
        monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    return request.param


def batch(p, job_class):
    return dataclasses.replace(p, job_class=np.asarray(job_class, dtype=np.uint32))


def observe(engine, p):
    """(assign, cap, occ, rows_occupied) of the engine's snapshot for p's jobs."""
    got = engine.place(p.job_class, want_tally=True)
    return got.assign.copy(), got.cap.copy(), got.occ.copy(), int(engine.explain()[0].rows_occupied)


def verify(engine, p):
    """The engine's snapshot is p's: placement, tallies and occupancy equal the oracle's on p."""
    assign, cap, occ, rows_occ = observe(engine, p)
    a, cap_c, occ_c = O.place_c(p)
    np.testing.assert_array_equal(occ, occ_c)
    np.testing.assert_array_equal(cap, cap_c)
    np.testing.assert_array_equal(assign, a)
    assert rows_occ == int((p.nodes.excl != -1).sum())
    return assign, occ


def assume_checked(engine, p, job_class, assign, owner):
    """engine.assume against the yardstick on p's columns; p.nodes.excl then
    follows, and the engine's snapshot is checked against it."""
    q = batch(p, job_class)
    new, committed, want = assume_ref(q, assign, owner)
    got, st = engine.assume(q.job_class, np.asarray(assign, dtype=np.int32), np.asarray(owner, dtype=np.int32))
    np.testing.assert_array_equal(got, committed)
    assert stats_dict(st) == want
    p.nodes.excl[:] = new
    verify(engine, p)
    return committed, st


def forget_checked(engine, p, owners):
    new, want = forget_ref(p.nodes.excl, owners)
    assert engine.forget(owners) == want
    p.nodes.excl[:] = new
    verify(engine, p)
    return want


# ------------------------------------------------------------------ 1. the hand case
def test_hand_case(engine, form):
    p = flat([2, 2, 2], [cls(0, 2)], [0, 0, 0])
    engine.load(p)
    committed, st = assume_checked(engine, p, [0, 0, 0], [1, 0, -1], [7, 9, 5])
    np.testing.assert_array_equal(committed, [True, True, False])
    assert (st.jobs, st.committed, st.stale, st.reserved, st.rows_marked) == (3, 2, 0, 0, 4)
    np.testing.assert_array_equal(observe(engine, p)[2], [2, 2, 0])
    assert forget_checked(engine, p, [9]) == 2                        # leaf 0's two rows, and only they
    np.testing.assert_array_equal(observe(engine, p)[2], [0, 2, 0])
    assert forget_checked(engine, p, [5]) == 0                        # the unplaced job's owner marked nothing
    assert forget_checked(engine, p, [7]) == 2


# ------------------------------------------------------------------ 2. place, assume, place
def test_place_assume_place(engine, form):
    p = flat([3] * 8 + [2], [cls(0, 3)], [0, 0, 0])
    engine.load(p)
    first = engine.place(p.job_class).assign.copy()
    np.testing.assert_array_equal(first, [0, 1, 2])
    np.testing.assert_array_equal(engine.place(p.job_class).assign, first)      # without the assume: the same domains
    assume_checked(engine, p, p.job_class, first, BASE + np.arange(3))
    second = engine.place(p.job_class).assign.copy()
    np.testing.assert_array_equal(second, O.place_c(p)[0])                       # p.nodes.excl is assume_ref's column
    np.testing.assert_array_equal(second, [3, 4, 5])
    assert domains_intersect(p, p.job_class, first, p.job_class, second) == []


def test_random_place_assume_place(engine, form):
    """Random nested snapshots: the first half of the batch is placed and
    assumed, then the second half equals the oracle on the yardstick's column
    and meets no committed domain."""
    done = 0
    for seed in range(12):
        p = synth.random_problem(seed, max_nodes=2500, max_leaves=120, max_jobs=80)
        J = p.n_jobs
        engine.load(p)
        jc1, jc2 = p.job_class[:J // 2], p.job_class[J // 2:]
        a1 = engine.place(jc1).assign.copy()
        np.testing.assert_array_equal(a1, O.place_c(batch(p, jc1))[0])
        committed, st = assume_checked(engine, p, jc1, a1, BASE + np.arange(jc1.shape[0]))
        np.testing.assert_array_equal(committed, a1 >= 0)
        a2 = engine.place(jc2).assign.copy()
        np.testing.assert_array_equal(a2, O.place_c(batch(p, jc2))[0])
        assert domains_intersect(p, jc1, a1, jc2, a2) == []
        done += int(st.committed)
    assert done > 50


# ------------------------------------------------------------------ 3. nested
def tree8():
    """2 zones x 2 racks x 2 leaves, one row per leaf; a zone job needs its 4 rows, a rack job 2, a leaf job 1."""
    return [np.array([0, 4, 8]), np.array([0, 2, 4, 6, 8]), np.arange(9)], [cls(0, 4), cls(1, 2), cls(2, 1)]


def test_nested(engine, form):
    fl, classes = tree8()
    p = nested(fl, [1] * 8, classes, [0])                             # one zone job
    engine.load(p)
    assume_checked(engine, p, [1], [0], [BASE])                       # rack 0, in zone 0
    np.testing.assert_array_equal(engine.place(np.array([0, 0], dtype=np.uint32)).assign, [1, -1])   # zone 0 is closed
    np.testing.assert_array_equal(engine.place(np.array([1, 1, 1, 1], dtype=np.uint32)).assign, [1, 2, 3, -1])
    assume_checked(engine, p, [0, 0], [0, 1], [BASE + 1, BASE + 2])   # zone 0 is stale now, zone 1 commits
    np.testing.assert_array_equal(engine.place(np.array([1, 1], dtype=np.uint32)).assign, [1, -1])   # racks 2, 3 closed
    np.testing.assert_array_equal(engine.place(np.array([2] * 4, dtype=np.uint32)).assign, [2, 3, -1, -1])
    assert forget_checked(engine, p, [BASE + 2]) == 4
    np.testing.assert_array_equal(engine.place(np.array([1, 1, 1, 1], dtype=np.uint32)).assign, [1, 2, 3, -1])


# ------------------------------------------------------------------ 4. stale
def test_stale_occupied_and_short(engine, form):
    excl = [-1, -1, -1, 7, -1, -1]     # leaf 1 holds a row of another exclusive job
    taints = [0, 0, 0, 0, 0, 1]        # leaf 2 is one pod short
    p = flat([2, 2, 2], [cls(0, 2)], [0, 0, 0], taints=taints, excl=excl)
    engine.load(p)
    before = observe(engine, p)[2]
    committed, st = assume_checked(engine, p, p.job_class, [1, 0, 2], [11, 12, 13])
    np.testing.assert_array_equal(committed, [False, True, False])
    assert (st.committed, st.stale, st.rows_marked) == (1, 2, 2)
    after = observe(engine, p)[2]
    np.testing.assert_array_equal(after[1:], before[1:])              # nothing written for the stale jobs
    np.testing.assert_array_equal(after, [2, 1, 0])
    assert forget_checked(engine, p, [11, 13]) == 0                   # their owners hold no row
    assert forget_checked(engine, p, [7]) == 1                        # (any id can be forgotten)


# ------------------------------------------------------------------ 5. domain sizes at the edges of both forms
@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_domain_size_edges(engine, form, rows, lead):
    """`lead` rows of another leaf in front (the domain starts on and off a
    4-row boundary, and the rows are loaded from the boundary below it), a
    2-row leaf behind: the fill covers the domain's rows and no other."""
    sizes = ([lead] if lead else []) + [rows, 2]
    d = 1 if lead else 0
    p = flat(sizes, [cls(0, rows)], [0])
    engine.load(p)
    _, st = assume_checked(engine, p, [0], [d], [BASE + rows])
    assert (st.committed, st.rows_marked) == (1, rows)
    occ = observe(engine, p)[2]
    assert occ[d] == rows and occ[d + 1] == 0 and (lead == 0 or occ[0] == 0)
    assert forget_checked(engine, p, [BASE + rows]) == rows


# ------------------------------------------------------------------ 6. snapshot sizes
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1025])
def test_snapshot_size_edges(engine, form, N):
    """One domain of N rows: the padding behind row N is neither written nor counted."""
    p = flat([N], [cls(0, 1)], [0])
    engine.load(p)
    _, st = assume_checked(engine, p, [0], [0], [INT32_MIN + 1])
    assert st.rows_marked == N
    assert forget_checked(engine, p, [INT32_MIN + 1]) == N
    assert forget_checked(engine, p, [INT32_MIN + 1]) == 0


# ------------------------------------------------------------------ 7. job counts at the in-place limit
@pytest.mark.parametrize("J", [1024, 1025])
def test_job_count_edges(engine, form, J):
    """One-row domains, every second one tainted (stale): up to 1,024 jobs the
    kernels read the input in place, above it its device copy."""
    taints = (np.arange(J) & 1).astype(np.uint32)
    p = flat([1] * J, [cls(0, 1)], np.zeros(J, dtype=np.uint32), taints=taints)
    engine.load(p)
    committed, st = assume_checked(engine, p, p.job_class, np.arange(J)[::-1], BASE + np.arange(J))
    assert (st.committed, st.stale, st.rows_marked) == ((J + 1) // 2, J // 2, (J + 1) // 2)
    np.testing.assert_array_equal(committed, taints[::-1] == 0)
    assert forget_checked(engine, p, BASE + np.arange(0, J, 3)) == int(committed[::3].sum())


# ------------------------------------------------------------------ 8. refusals
def refused(engine, job_class, assign, owner, code, text=None, **kw):
    rc, rl = job_runs(np.asarray(job_class, dtype=np.uint32))
    with pytest.raises(native.JspError) as ei:
        engine.assume_runs(rc, rl, np.asarray(assign, dtype=np.int32), np.asarray(owner, dtype=np.int32), **kw)
    assert ei.value.code == code, str(ei.value)
    if text is not None:
        assert text in str(ei.value), str(ei.value)


def test_refusals_write_nothing(engine, form):
    fl, classes = tree8()
    jc = [1, 2, 1, 0, 1, 2, 2]
    p = nested(fl, [1] * 8, classes, jc)
    p.nodes.excl[7] = 3                                               # leaf 7 is another job's
    engine.load(p)
    own = BASE + np.arange(7)
    good = [1, 0, -1, -1, 2, 1, 6]                                    # rack 1, leaf 0, rack 2, leaves 1 and 6
    before = observe(engine, p)
    lib = native.lib()
    rc, rl = job_runs(np.asarray(jc, dtype=np.uint32))
    a32, o32 = np.asarray(good, dtype=np.int32), own.astype(np.int32)

    def unchanged_then_usable():
        now = observe(engine, p)
        for x, y in zip(now[:3], before[:3]):
            np.testing.assert_array_equal(x, y)
        assert now[3] == before[3]
        committed, _ = assume_checked(engine, p, jc, good, own)       # the next valid call succeeds
        np.testing.assert_array_equal(committed, [True, True, False, False, True, True, True])
        assert forget_checked(engine, p, own) == 7                    # and is taken back

    for args in ((rc.ctypes.data, rl.ctypes.data, rc.shape[0], None, o32.ctypes.data, 0),          # NULL assign
                 (rc.ctypes.data, rl.ctypes.data, rc.shape[0], a32.ctypes.data, None, 0)):        # NULL owner
        assert lib.jsp_assume(engine._h, *args, None, None) == native.JSP_EINVAL
        unchanged_then_usable()
    bad_rc = rc.copy()
    bad_rc[-1] = 3                                                    # classes are 0..2
    assert lib.jsp_assume(engine._h, bad_rc.ctypes.data, rl.ctypes.data, rc.shape[0], a32.ctypes.data,
                          o32.ctypes.data, 0, None, None) == native.JSP_EINVAL
    unchanged_then_usable()
    refused(engine, jc, good, own, native.JSP_EINVAL, "flags", flags=1)
    unchanged_then_usable()
    minus = own.copy()
    minus[4] = -1
    refused(engine, jc, good, minus, native.JSP_EINVAL, "job 4:")      # owner -1 for a placed job
    unchanged_then_usable()
    minus[4], minus[2] = own[4], -1
    assume_checked(engine, p, jc, good, minus)                        # ... but ignored for an unplaced one
    forget_checked(engine, p, own)
    refused(engine, jc, [1, 0, -2, -1, 2, 1, 6], own, native.JSP_EINVAL, "job 2:")
    unchanged_then_usable()
    refused(engine, jc, [1, 8, -1, -1, 2, 1, 6], own, native.JSP_EINVAL, "job 1:")      # leaves are 0..7
    unchanged_then_usable()
    refused(engine, jc, [1, 0, -1, 2, 2, 1, 6], own, native.JSP_EINVAL, "job 3:")       # zones are 0..1
    unchanged_then_usable()
    # the conflicting pair last in a batch of otherwise valid jobs: leaf 4 after rack 2, which holds it
    conflict = [1, 0, -1, -1, 2, 1, 4]
    with pytest.raises(BindConflict) as ei:
        assume_ref(p, conflict, own)
    assert ei.value.job == 6
    refused(engine, jc, conflict, own, native.JSP_EINVAL, "job 6:")
    unchanged_then_usable()
    refused(engine, jc, [1, 0, -1, 0, 2, 1, 6], own, native.JSP_EINVAL, "job 3:")       # zone 0 after rack 1 and leaf 0
    unchanged_then_usable()


def test_forget_refusals(engine, form):
    p = flat([2, 2], [cls(0, 2)], [0])
    engine.load(p)
    assume_checked(engine, p, [0], [1], [BASE])
    lib = native.lib()
    n = ctypes.c_uint64(99)
    assert lib.jsp_forget(engine._h, None, 1, ctypes.byref(n)) == native.JSP_EINVAL
    with pytest.raises(native.JspError) as ei:
        engine.forget([BASE, -1])
    assert ei.value.code == native.JSP_EINVAL
    with pytest.raises(native.JspError) as ei:
        engine.forget(np.full(native.JSP_FORGET_MAX_OWNERS + 1, BASE, dtype=np.int32))
    assert ei.value.code == native.JSP_ERANGE
    verify(engine, p)                                                 # nothing was cleared
    assert engine.forget([]) == 0
    assert lib.jsp_forget(engine._h, None, 0, None) == native.JSP_OK
    assert forget_checked(engine, p, [BASE]) == 2


def test_device_set_sharded_and_unloaded_engines_are_estate():
    p = synth.config5()
    assign = O.place_c(p)[0]
    own = BASE + np.arange(p.n_jobs)
    with Engine(devices=[0, 0]) as multi:
        multi.load(p)
        refused(multi, p.job_class, assign, own, native.JSP_ESTATE, "device-set")
        with pytest.raises(native.JspError) as ei:
            multi.forget([BASE])
        assert ei.value.code == native.JSP_ESTATE and "device-set" in str(ei.value)
    with Engine(0) as e:
        e.upload_topology(p.topology)
        e.upload_snapshot(shard_problem(p, 0, 2))
        e.upload_classes(p.classes)
        refused(e, p.job_class, assign, own, native.JSP_ESTATE, "sharded")
        with pytest.raises(native.JspError) as ei:
            e.forget([BASE])
        assert ei.value.code == native.JSP_ESTATE and "sharded" in str(ei.value)
    lib = native.lib()
    with Engine(0) as e:
        a = np.zeros(1, dtype=np.int32)
        one, zero = np.ones(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        assert lib.jsp_assume(e._h, zero.ctypes.data, one.ctypes.data, 1, a.ctypes.data, a.ctypes.data, 0, None,
                              None) == native.JSP_ESTATE               # no topology yet
        assert lib.jsp_forget(e._h, a.ctypes.data, 1, None) == native.JSP_ESTATE
        e.upload_topology(p.topology)
        assert lib.jsp_assume(e._h, zero.ctypes.data, one.ctypes.data, 1, a.ctypes.data, a.ctypes.data, 0, None,
                              None) == native.JSP_ESTATE               # no snapshot yet
        e.upload_snapshot(p.nodes)
        assert lib.jsp_assume(e._h, zero.ctypes.data, one.ctypes.data, 1, a.ctypes.data, a.ctypes.data, 0, None,
                              None) == native.JSP_ESTATE               # no classes yet
        assert lib.jsp_forget(e._h, a.ctypes.data, 1, None) == native.JSP_ESTATE


# ------------------------------------------------------------------ 9. empty leaves, a domain without leaves
def test_empty_leaves_and_empty_domain(engine, form):
    """Zone 0 = two empty leaves, a full one and another empty one; zone 1 has no rows at all."""
    p = nested([[0, 4, 6, 7], np.arange(8)], [0, 0, 5, 0, 0, 0, 3], [cls(0, 5), cls(0, 3)], [0, 1, 1])
    engine.load(p)
    committed, st = assume_checked(engine, p, p.job_class, [0, 1, 2], [BASE, BASE + 1, BASE + 2])
    np.testing.assert_array_equal(committed, [True, False, True])
    assert (st.committed, st.stale, st.rows_marked) == (2, 1, 8)
    assert forget_checked(engine, p, [BASE + 1]) == 0
    assert forget_checked(engine, p, [BASE + 2, BASE]) == 8


def test_domains_without_leaves_claim_nothing(engine, form):
    """Rack 2 has no leaves (it sits at leaf 4, where zone 1 begins): assumed
    twice and beside zone 1 it conflicts with nothing, is stale and marks nothing."""
    fl = [np.array([0, 4, 8]), np.array([0, 2, 4, 4, 6, 8]), np.arange(9)]
    classes = [cls(0, 4), cls(1, 2), cls(2, 1)]
    p = nested(fl, [1] * 8, classes, [0, 1, 1, 1])
    engine.load(p)
    committed, st = assume_checked(engine, p, p.job_class, [1, 2, 2, 0], BASE + np.arange(4))
    np.testing.assert_array_equal(committed, [True, False, False, True])
    assert (st.committed, st.stale, st.rows_marked) == (2, 2, 6)
    assert forget_checked(engine, p, [BASE + 1, BASE + 2]) == 0
    refused(engine, p.job_class, [1, 2, 2, 3], BASE + np.arange(4), native.JSP_EINVAL, "job 3:")  # rack 3 is in zone 1
    verify(engine, p)


# ------------------------------------------------------------------ 10. the resident service
def warm(engine, job_class):
    for _ in range(4):
        got = engine.place(job_class)
        if got.fused in (3, 4, 5):
            return got
    return got


def short_by_one(p, c, d):
    """(row, taints) that leaves domain d one pod short for class c: a row the class passes gets a bit it does not tolerate."""
    jc = p.classes[c]
    r0, r1 = domain_rows(p, jc.level, d)
    bit = next(b for b in range(32) if not (jc.tolerated_taints >> b) & 1)
    row = next(n for n in range(r0, r1) if (int(p.nodes.taints[n]) & ~jc.tolerated_taints & 0xFFFFFFFF) == 0)
    return row, int(p.nodes.taints[row]) | (1 << bit)


@pytest.mark.parametrize("cfg,fused", [(2, 3), (5, 5)])
def test_service_stays_up(engine, form, cfg, fused):
    """Place, assume, place with the resident service answering: the tiles
    reload their rows, the service is neither stopped nor restarted, and both
    calls are ordered after a pending patch. Every reference is computed
    before its engine calls, which then run back to back: the service leaves
    after an idle gap, and that restart is not what is counted here."""
    engine.set_service(True)
    engine.set_fused(True)

    def back_to_back(middle):
        """place (the service is up after it), middle(), place: fused and svc_starts around the last two."""
        assert warm(engine, p.job_class).fused == fused
        starts = engine.metrics().svc_starts
        out = middle()
        got = engine.place(p.job_class)
        assert got.fused == fused
        assert engine.metrics().svc_starts == starts
        return out, got.assign.copy()

    try:
        p = synth.CONFIGS[cfg]()
        engine.load(p)
        a1 = O.place_c(p)[0]
        np.testing.assert_array_equal(warm(engine, p.job_class).assign, a1)
        # place, assume, place
        jc1, own = p.job_class[:100], BASE + np.arange(100)
        new, committed, want = assume_ref(batch(p, jc1), a1[:100], own)
        assert want["committed"] == int((a1[:100] >= 0).sum()) > 0
        p.nodes.excl[:] = new
        a2 = O.place_c(p)[0]
        assert domains_intersect(p, jc1, a1[:100], p.job_class, a2) == []
        (got, st), second = back_to_back(lambda: engine.assume(jc1, a1[:100], own))
        np.testing.assert_array_equal(got, committed)
        assert stats_dict(st) == want
        np.testing.assert_array_equal(second, a2)                    # at once: the tiles reloaded the rows
        # a patch that leaves a domain one pod short, then at once the assume of its job
        jc2, d2, own2 = p.job_class[100:200], a2[100:200].copy(), BASE + np.arange(100, 200)
        k = next(j for j in range(100) if d2[j] >= 0)
        row, tn = short_by_one(p, int(jc2[k]), int(d2[k]))
        p.nodes.taints[row] = tn
        new, committed, want = assume_ref(batch(p, jc2), d2, own2)
        assert not committed[k] and want["stale"] >= 1 and want["committed"] > 0
        p.nodes.excl[:] = new
        a3 = O.place_c(p)[0]

        def patch_then_assume():
            engine.patch_rows(np.array([row], dtype=np.uint32), taints=np.array([tn], dtype=np.uint32))
            return engine.assume(jc2, d2, own2)
        (got, st), third = back_to_back(patch_then_assume)
        np.testing.assert_array_equal(got, committed)
        assert stats_dict(st) == want
        np.testing.assert_array_equal(third, a3)
        # forget in the middle position, behind a patch that hands a free row to one of its owners
        free_row = int(np.flatnonzero(p.nodes.excl == -1)[0])
        p.nodes.excl[free_row] = BASE + 7
        new, want = forget_ref(p.nodes.excl, own[:50])
        assert new[free_row] == -1 and want > 1
        p.nodes.excl[:] = new
        a4 = O.place_c(p)[0]

        def patch_then_forget():
            engine.patch_rows(np.array([free_row], dtype=np.uint32), excl=np.array([BASE + 7], dtype=np.int32))
            return engine.forget(own[:50])
        cleared, fourth = back_to_back(patch_then_forget)
        assert cleared == want
        np.testing.assert_array_equal(fourth, a4)
        verify(engine, p)                                            # (tallies requested: the launch path)
    finally:
        engine.service_stop()


# ------------------------------------------------------------------ 11. forget
def test_forget_subsets_and_list_sizes(engine, form):
    """30 leaves of 10 rows: three belong to informer-style ids (0, 3,
    INT32_MIN), the others are assumed. Lists on both sides of the kernel's
    LDS limit (4,096 owners) and the call's limit, unsorted and with
    duplicates, whose absent ids neighbour the present ones."""
    L = 30
    excl = np.full(10 * L, -1, dtype=np.int32)
    excl[0:10], excl[10:20], excl[20:30] = 0, 3, INT32_MIN
    p = flat([10] * L, [cls(0, 10)], [0])
    p.nodes.excl[:] = excl
    engine.load(p)
    jobs = np.zeros(L - 3, dtype=np.uint32)
    own = BASE + 5 * np.arange(L - 3)
    committed, st = assume_checked(engine, p, jobs, np.arange(3, L), own)
    assert committed.all() and st.rows_marked == 10 * (L - 3)
    assert forget_checked(engine, p, [own[5], own[2], own[5], own[9]]) == 30          # unsorted, a duplicate
    assert forget_checked(engine, p, [own[5], BASE + 1, 1, 2, 4, INT32_MIN + 1, 0x7FFFFFFF]) == 0    # all absent
    rng = np.random.default_rng(11)
    held = [j for j in range(L - 3) if j not in (2, 5, 9)]
    assert native.JSP_FORGET_MAX_OWNERS == 65536
    for n in (4095, 4096, 4097, 65536):
        take, held = held[:4], held[4:]
        near = np.concatenate([own[take] + 1, own[take] - 1])                          # neighbours of the present ids
        low = np.arange(5, 5 + (n - 12) // 2, dtype=np.int64)                          # absent, below every owner
        high = BASE + 1000 + np.arange(n - 12 - low.shape[0], dtype=np.int64)          # absent, above
        owners = np.concatenate([own[take], near, low, high]).astype(np.int32)
        assert owners.shape[0] == n and np.unique(owners).shape[0] == n
        assert forget_checked(engine, p, rng.permutation(owners)) == 40
    assert (p.nodes.excl[:30] == excl[:30]).all()                                      # the informer's rows stayed
    with pytest.raises(native.JspError) as ei:
        engine.forget(np.arange(5, 5 + 65537, dtype=np.int32))
    assert ei.value.code == native.JSP_ERANGE
    verify(engine, p)
    assert forget_checked(engine, p, [0, INT32_MIN]) == 20                             # any id but -1 can be forgotten


# ------------------------------------------------------------------ 12. bind and sticky beside assume
def test_bind_and_sticky(engine, form):
    p = flat([4] * 6, [cls(0, 3)], [0, 0, 0, 0])
    engine.load(p)
    a = engine.place(p.job_class).assign.copy()
    np.testing.assert_array_equal(a, [0, 1, 2, 3])
    want_rows = bind_ref(p, a)[0]
    rows, _, st = engine.bind_pods(p.job_class, a)                    # bind first ...
    np.testing.assert_array_equal(rows, want_rows)
    assert st.bound == 4
    own = BASE + np.arange(4)
    committed, _ = assume_checked(engine, p, p.job_class, a, own)     # ... then assume
    assert committed.all()
    rows, _, st = engine.bind_pods(p.job_class, a)                    # bind after assume is stale
    np.testing.assert_array_equal(rows, bind_ref(p, a)[0])
    assert (rows == -1).all() and (st.bound, st.stale) == (0, 4)
    committed, st2 = assume_checked(engine, p, p.job_class, a, own)   # and so is a repeated assume
    assert not committed.any() and st2.stale == 4
    got, sst = engine.place_sticky(p.job_class, a)                    # the assumed domains are closed to their own jobs
    (want, kept) = sticky_ref(p, a)
    np.testing.assert_array_equal(got, want)
    assert sst.kept == 0 and not kept.any() and sst.hinted == 4
    np.testing.assert_array_equal(got, [4, 5, -1, -1])
    assert forget_checked(engine, p, own) == 16
    got, sst = engine.place_sticky(p.job_class, a)                    # forgotten: every job keeps its domain
    np.testing.assert_array_equal(got, a)
    assert sst.kept == 4


# ------------------------------------------------------------------ 13. round trip
def test_round_trip_is_exact_and_repeatable(engine, form):
    p = synth.random_problem(3, max_nodes=3000, max_leaves=150, max_jobs=100)
    engine.load(p)
    before = observe(engine, p)
    a = before[0]
    own = BASE + np.arange(p.n_jobs)
    outs = []
    for _ in range(2):
        committed, st = engine.assume(p.job_class, a, own)
        cleared = engine.forget(own[::-1])
        outs.append((committed.tolist(), stats_dict(st), cleared))
        after = observe(engine, p)
        for x, y in zip(after[:3], before[:3]):
            np.testing.assert_array_equal(x, y)
        assert after[3] == before[3]
    assert outs[0] == outs[1]
    assert outs[0][2] == outs[0][1]["rows_marked"] > 0 and outs[0][0] == (a >= 0).tolist()


def test_assume_forget_loop_leaves_the_snapshot(engine, form):
    p = flat([5] * 40, [cls(0, 5)], np.zeros(30, dtype=np.uint32))
    engine.load(p)
    a = engine.place(p.job_class).assign.copy()
    rc, rl = job_runs(p.job_class)
    (am, a99, fm, f99), st, cleared = engine.assume_forget_loop(rc, rl, a, BASE + np.arange(30), iters=5)
    assert 0 < am <= a99 and 0 < fm <= f99
    assert (st.committed, st.stale, st.rows_marked, cleared) == (30, 0, 150, 150)
    verify(engine, p)
