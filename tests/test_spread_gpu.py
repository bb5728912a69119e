"""jsp_place_spread on the GPU against the rule taken literally in numpy
(tests/spread_ref.py; it never calls the engine). Every comparison is exact:
assign[], spread_out[] and count_out[] entry for entry, the stats field by
field, and the tables behind the walk -- the fits words, the feasibility words
beside them, peers[] and the two span-count tables -- word for word, in both
span-count forms and at every lane count of the leaf pass (tests/test_spread.py
asserts the sweep's coverage floors on the reference's own output)."""
import dataclasses

import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from bind_ref import cls, nested
from gang_ref import feas_words
from spread_ref import (INT32_MIN, SOFT, SWEEP_SEEDS, check_spread, count_tables, fits_words, hand_cases, one_class,
                        owners_of, peers_ref, reduction_problem, rooted, spread_ref, stats_dict, sweep)

pytestmark = pytest.mark.gpu

BIG = 0x40000000


def run(engine, p, s, k, peers, load=True, tallies=None):
    """Load p, spread its jobs, compare everything with the yardstick."""
    if load:
        engine.load(p)
    want = spread_ref(p, s, k, peers, tallies)
    a, sp, cnt, st = engine.place_spread(p.job_class, s, k, peers)
    np.testing.assert_array_equal(a, want[0], err_msg=f"{p.name} s {s} skew {k}")
    np.testing.assert_array_equal(sp, want[1], err_msg=f"{p.name} s {s} skew {k}")
    np.testing.assert_array_equal(cnt, want[2], err_msg=f"{p.name} s {s} skew {k}")
    assert stats_dict(st) == want[3], (p.name, s, k)
    return a, sp, cnt, st


# ------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("seed", list(SWEEP_SEEDS))
def test_sweep(engine, seed):
    p, s, k, peers = sweep(seed)
    engine.load(p)
    tallies = O.place_c(p)[1:]
    a, sp, cnt, st = run(engine, p, s, k, peers, load=False, tallies=tallies)
    check_spread(p, s, k, peers, a, sp, cnt, tallies)
    # the same jobs as raw runs
    rc, rl = job_runs(p.job_class)
    a2, sp2, cnt2, st2 = engine.place_spread_runs(rc, rl, s, k, peers)
    np.testing.assert_array_equal(a2, a)
    np.testing.assert_array_equal(sp2, sp)
    np.testing.assert_array_equal(cnt2, cnt)
    assert st2.runs == len(rc) and st2.fused == 7 and stats_dict(st2) == stats_dict(st)
    # the other settings, and no peers
    for k2 in (SOFT, 1, 3):
        if k2 != k:
            run(engine, p, s, k2, peers, load=False, tallies=tallies)
    run(engine, p, s, k, [], load=False, tallies=tallies)


# ------------------------------------------------------------------ 2. the reductions, on the engine's own jsp_place
@pytest.mark.parametrize("i", range(0, 60, 2))
def test_reductions_are_jsp_place(engine, i):
    q = reduction_problem(i)
    p = rooted(q)
    if p is not None:      # one level-s domain: bit for bit, every max_skew and peer list
        engine.load(p)
        plain = engine.place(p.job_class).assign.copy()
        own = owners_of(p)
        for k in (SOFT, 1, 3):
            for peers in ([], own):
                a, sp, cnt, st = engine.place_spread(p.job_class, 0, k, peers)
                np.testing.assert_array_equal(a, plain)
                assert (st.jobs, st.placed, st.refused, st.skew) == (p.n_jobs, int((plain >= 0).sum()), 0, 0)
    p = one_class(q)
    if p.n_jobs:
        engine.load(p)
        got = engine.place(p.job_class)
        lvl = p.classes[int(p.job_class[0])].level
        for k in (SOFT, 1, 3):     # s == level[c], no peers
            a, sp, cnt, st = engine.place_spread(p.job_class, lvl, k, [])
            np.testing.assert_array_equal(a, got.assign)
            np.testing.assert_array_equal(sp, got.assign)
        for s in range(lvl + 1):   # SOFT places as many
            assert engine.place_spread(p.job_class, s, SOFT, owners_of(p))[3].placed == got.placed


# ------------------------------------------------------------------ 3. the hand cases
@pytest.mark.parametrize("name", list(hand_cases()))
def test_hand_cases(engine, name):
    p, s, k, peers, want, want_s, want_n, want_refused = hand_cases()[name]
    a, sp, cnt, st = run(engine, p, s, k, peers)
    np.testing.assert_array_equal(a, want)
    np.testing.assert_array_equal(sp, want_s)
    np.testing.assert_array_equal(cnt, want_n)
    assert st.refused == want_refused


# ------------------------------------------------------------------ 4. the tables against numpy
OWNERS = (-1, -1, -1, 0, INT32_MIN, BIG, 900)       # 900 is in no peer table
TABLES = ([], [0], [INT32_MIN, 0], [BIG, 0, INT32_MIN])


def table_case(first_leaf, levels, rows=None, seed=1, pods=(1, 3), taint_p=0.3, jobs=(), seg_max=5, excl=None):
    """rows[l] rows per leaf (default 1 to 4 by the seed), a share of them
    tainted with bit 0; per level in `levels` one class per pods value,
    alternately tolerating nothing and bit 0; owners laid over the rows in
    seeded segments of 1..seg_max rows whatever the leaves, so that segments
    cross leaf and domain boundaries and an owner comes back in several
    (excl: the owners given row by row instead)."""
    L = len(first_leaf[-1]) - 1
    rows = synth.uniform_int(seed, 5, L, 1, 4) if rows is None else np.asarray(rows, dtype=np.int64)
    N = int(rows.sum())
    taints = synth.bernoulli(seed, 11, N, taint_p).astype(np.uint32)
    lens = synth.uniform_int(seed, 12, max(N, 1), 1, seg_max)
    who = synth.uniform_int(seed, 13, max(N, 1), 0, len(OWNERS) - 1)
    if excl is None:
        excl = np.repeat(np.array(OWNERS, dtype=np.int64)[who], lens)[:N].astype(np.int32)
    classes = [cls(k, n, tol=i % 2) for k in levels for i, n in enumerate(pods)]
    p = nested(first_leaf, rows, classes, list(jobs), taints=taints, excl=excl)
    p.topology.validate()
    return p


def ident(n):
    return np.arange(n + 1)


TABLE_CASES = {
    # segments of 63, 64 and 65 domains per S: the word-boundary masks
    "K2-63-64-65": lambda: table_case([[0, 63, 127, 192], ident(192)], [1, 0], jobs=[0, 2, 1, 3] * 5),
    # more than 256 level-s domains: more than one block in every launch over S
    "K2-300-zones": lambda: table_case([np.arange(0, 601, 2), ident(600)], [1, 0], jobs=[0, 2] * 8),
    # an S without leaves (0, 2, 4), leaves without rows, an S whose first leaf is empty (1, 3)
    # (owner 0's segment runs from S 1 into S 3: rows 0-1 are leaf 1, rows 2-4 leaf 5)
    "K2-empty": lambda: table_case([[0, 0, 3, 3, 10, 10], ident(10)], [1, 0], rows=[0, 2, 0, 0, 0, 3, 1, 0, 2, 1],
                                   jobs=[0, 2, 1], excl=[0, 0, 0, 900, INT32_MIN, INT32_MIN, -1, -1, BIG]),
    # leaves of 0, 1 and about 300 rows: every lane count of the leaf pass
    "K1-long-leaves": lambda: table_case([ident(9)], [0], rows=[200, 1, 0, 130, 64, 65, 300, 2, 90], jobs=[0, 1] * 3,
                                         seg_max=40),
    "K1-D257": lambda: table_case([ident(257)], [0], jobs=[0, 1] * 10),
    "K3": lambda: table_case([[0, 50, 50, 192, 200],
                              sorted(set(range(0, 50, 2)) | set(range(50, 192, 7)) | {192, 200}), ident(200)], [2, 0, 1],
                             jobs=[0, 4, 2, 5] * 4),
    "K4": lambda: table_case([[0, 75, 75, 200], np.arange(0, 201, 25), np.arange(0, 201, 5), ident(200)], [3, 1, 0, 2],
                             jobs=[6, 2, 0, 4] * 3),
    # long upper domains: several lanes sum one S's leaves (2 zones x 700 racks)
    "K3-long": lambda: table_case([[0, 700, 1400], np.r_[np.arange(0, 700, 7), np.arange(700, 1401, 350)], ident(1400)],
                                  [2, 1, 0], rows=[1] * 1400, jobs=[0, 2, 4] * 4),
}


def tables_ref(p, s, peers):
    cap, occ = O.place_c(p)[1:]
    cf, ce = count_tables(p, s, cap, occ)
    return fits_words(p, cap), feas_words(p, cap, occ), peers_ref(p, s, peers).astype(np.uint32), cf, ce


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_tables_match_numpy(engine, name):
    p = TABLE_CASES[name]()
    engine.load(p)
    some = 0
    assert 900 in p.nodes.excl            # an owner that is in no table
    for s in range(p.topology.n_levels):
        for peers in TABLES:
            want = tables_ref(p, s, peers)
            some += int(want[2].sum())
            first = s == 0 and len(peers) == 3
            for form in ((0, 1, 2) if len(peers) == 3 else (0,)):
                for shift in ((-1, 0, 1, 2, 3, 4, 5, 6) if first and form == 0 else (-1,)):
                    got = engine.spread_tables(s, peers, form=form, shift=shift)
                    for g, w, what in zip(got, want, ("fits", "feas", "peers", "cnt_feas", "cnt_fits")):
                        np.testing.assert_array_equal(
                            g, w, err_msg=f"{name} s {s} peers {len(peers)} form {form} shift {shift}: {what}")
    assert some > 0  # the case is not empty
    # and the walk over them, at every level no class of the jobs is coarser than
    lv = min(p.classes[int(c)].level for c in p.job_class)
    for s in range(lv + 1):
        for k in (SOFT, 1, 3):
            run(engine, p, s, k, TABLES[3], load=False)


def test_peer_segments_across_boundaries(engine):
    """One S of two leaves with a segment over the leaf boundary: counted
    once; a segment over the boundary between two S: counted in both; the same
    owner back after a gap: counted again; an owner that is no peer between."""
    A, B = 7, 9
    #        zone 0: racks 0, 1            zone 1: racks 2, 3
    excl = [-1, A, A, A, A, B, A, A,      A, A, B, B, B, A, -1, -1]
    p = nested([[0, 2, 4], ident(4)], [4, 4, 4, 4], [cls(1, 1)], [0], excl=excl)
    engine.load(p)
    for peers, zones, racks in (([A], [2, 2], [1, 2, 1, 1]), ([A, B], [3, 3], [1, 3, 2, 2]), ([B], [1, 1], [0, 1, 1, 1])):
        assert peers_ref(p, 0, peers).tolist() == zones and peers_ref(p, 1, peers).tolist() == racks
        for shift in (-1, 0, 2):
            np.testing.assert_array_equal(engine.spread_tables(0, peers, shift=shift)[2], zones)
            np.testing.assert_array_equal(engine.spread_tables(1, peers, shift=shift)[2], racks)


def test_spread_tables_refusals_and_timing(engine):
    p = TABLE_CASES["K3-long"]()
    engine.load(p)
    lib = native.lib()
    nw = sum((p.topology.n_domains[jc.level] + 63) // 64 for jc in p.classes)
    fits = np.zeros(nw + 1, dtype=np.uint64)
    pr = np.zeros(p.topology.n_domains[0] + 1, dtype=np.uint32)
    ids = np.array([5, 5], dtype=np.int32)
    f, q = fits.ctypes.data, pr.ctypes.data
    for args in ((0, None, 0, 3, -1, f, None, nw, q),          # form
                 (0, None, 0, 0, 7, f, None, nw, q),           # shift
                 (3, None, 0, 0, -1, f, None, nw, q),          # the level
                 (0, None, 0, 0, -1, f, None, nw + 1, q),      # n_words
                 (0, None, 0, 0, -1, None, None, nw, q),       # fits_out
                 (0, None, 0, 0, -1, f, None, nw, None),       # peers_out
                 (0, None, 1, 0, -1, f, None, nw, q),          # peer_ids
                 (0, ids.ctypes.data, 2, 0, -1, f, None, nw, q)):   # the same id twice
        assert lib.jspb_spread_tables(engine._h, *args, None, None, 0, None) == native.JSP_EINVAL
    *_, (med, mean) = engine.spread_tables(0, TABLES[3], iters=20)
    assert 0 < med < 1e4 and 0 < mean < 1e4


# ------------------------------------------------------------------ 5. behind the service and a patch
def rows_of(p, level, d):
    fl = p.topology.first_leaf[level]
    ls = p.nodes.leaf_start
    return np.arange(int(ls[int(fl[d])]), int(ls[int(fl[d + 1])]))


def same(got, want, what):
    a, sp, cnt, st = got
    np.testing.assert_array_equal(a, want[0], err_msg=what)
    np.testing.assert_array_equal(sp, want[1], err_msg=what)
    np.testing.assert_array_equal(cnt, want[2], err_msg=what)
    assert stats_dict(st) == want[3], what


def test_behind_the_service_and_a_patch(engine):
    """With the resident service up: a jsp_place before and after the call
    answers identically and the service is not restarted; a patch that gives a
    domain to a peer, and one that frees it again, are each seen by the call
    that follows at once. Every reference is computed first and the engine
    calls run back to back: the service leaves after an idle gap, and that
    restart is not what is counted here."""
    engine.set_service(True)
    engine.set_fused(True)
    try:
        p = synth.config2()
        engine.load(p)
        plain = O.place_c(p)[0]
        few = dataclasses.replace(p, job_class=p.job_class[:24], job_names=None)
        lvl = p.classes[int(few.job_class[0])].level
        want1 = spread_ref(few, lvl, 1, [])
        d = int(want1[0][0])
        rows = rows_of(p, lvl, d)
        held = p.nodes.excl.copy()
        held[rows] = 777
        few2 = dataclasses.replace(few, nodes=dataclasses.replace(p.nodes, excl=held))
        want2 = spread_ref(few2, lvl, 1, [777])
        want3 = spread_ref(few, lvl, 1, [777])
        assert d not in want2[0].tolist() and want2[2].sum() == want1[2].sum() + 1
        for _ in range(4):
            if engine.place(p.job_class).fused == 3:
                break
        before = engine.place(p.job_class)
        m0 = engine.metrics()
        got1 = engine.place_spread(few.job_class, lvl, 1, [])
        after = engine.place(p.job_class)
        m1 = engine.metrics()
        engine.patch_rows(rows.astype(np.uint32), excl=np.full(rows.shape[0], 777, dtype=np.int32))
        got2 = engine.place_spread(few.job_class, lvl, 1, [777])     # at once: behind the patch the dispatcher holds
        engine.patch_rows(rows.astype(np.uint32), excl=np.full(rows.shape[0], -1, dtype=np.int32))
        got3 = engine.place_spread(few.job_class, lvl, 1, [777])     # the patch frees a domain the call sees
        again = engine.place(p.job_class)
        m2 = engine.metrics()
        assert before.fused == 3 and after.fused == 3 and again.fused == 3
        assert m1.svc_starts == m0.svc_starts == m2.svc_starts      # the service kept its tiles
        for r in (before, after, again):
            np.testing.assert_array_equal(r.assign, plain)
        same(got1, want1, "behind the service")
        same(got2, want2, "behind the patch that holds the domain")
        same(got3, want3, "behind the patch that frees it")
        # counted as jsp_place_fit's calls are: one spread call and one jsp_place between m0 and m1
        assert m1.place_us.count == m0.place_us.count + 2 and m1.batch_jobs.count == m0.batch_jobs.count + 2
        assert m1.placed == m0.placed + got1[3].placed + after.placed and m1.place_errors == m0.place_errors
        with pytest.raises(native.JspError):
            engine.place_spread_runs([0], [4], lvl, 1, [], flags=1)
        assert engine.metrics().place_errors == m2.place_errors + 1
    finally:
        engine.service_stop()


# ------------------------------------------------------------------ 6. refusals, each followed by a correct call
def refused(engine, code, word, *args, **kw):
    with pytest.raises(native.JspError) as ei:
        engine.place_spread_runs(*args, **kw)
    assert ei.value.code == code, str(ei.value)
    assert word in str(ei.value), str(ei.value)


def test_refusals_leave_the_engine_usable(engine):
    p, s, k, peers, want, want_s, want_n, _ = hand_cases()["mixed-levels"]    # a zone class and a rack class
    engine.load(p)
    rc, rl = job_runs(p.job_class)
    lib = native.lib()
    one, zero = np.ones(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    out = np.zeros(4, dtype=np.int32)
    own = np.array([7], dtype=np.int32)

    def ok():
        np.testing.assert_array_equal(run(engine, p, s, k, peers, load=False)[0], want)

    def raw(*args):
        return lib.jsp_place_spread(engine._h, *args)

    refused(engine, native.JSP_EINVAL, "flags 1", rc, rl, s, k, peers, flags=1)
    ok()
    refused(engine, native.JSP_EINVAL, "run 1", [0, 2, 0], [1, 1, 1], s, k, peers)               # a class that does not exist
    ok()
    refused(engine, native.JSP_EINVAL, "spread level 2", rc, rl, 2, k, peers)                    # no such level
    ok()
    refused(engine, native.JSP_EINVAL, "run 0", [0, 1], [1, 1], 1, k, peers)                     # finer than the zone class
    ok()
    a, sp, cnt, st = engine.place_spread_runs([0, 1], [0, 2], 1, k, peers)                       # ... whose run is empty
    np.testing.assert_array_equal(a, [0, 1])
    assert (st.jobs, st.placed, st.runs) == (2, 2, 1)
    refused(engine, native.JSP_EINVAL, "table index 1", rc, rl, s, k, [7, -1])                   # -1 names no owner
    ok()
    refused(engine, native.JSP_EINVAL, "table index 2", rc, rl, s, k, [7, 9, 7])                 # the same id twice
    ok()
    refused(engine, native.JSP_ERANGE, "limit of 65536", [0], [native.JSP_SPREAD_MAX_JOBS + 1], s, k, peers)
    ok()
    big = np.arange(100, 100 + native.JSP_SPREAD_MAX_PEERS + 1, dtype=np.int32)                  # ids nobody holds
    refused(engine, native.JSP_ERANGE, "limit of 65536", rc, rl, s, k, big)
    ok()
    a, sp, cnt, st = engine.place_spread_runs(rc, rl, s, k, big[:-1])                            # 65536 peers, none held
    np.testing.assert_array_equal(a, want)
    assert raw(zero.ctypes.data, one.ctypes.data, 1, 0, 1, None, 0, 0, None, None, None, None) == \
        native.JSP_EINVAL and b"NULL" in lib.jsp_last_error()                                    # assign_out
    ok()
    assert raw(None, one.ctypes.data, 1, 0, 1, None, 0, 0, out.ctypes.data, None, None, None) == \
        native.JSP_EINVAL and b"NULL" in lib.jsp_last_error()                                    # run_class
    ok()
    assert raw(zero.ctypes.data, one.ctypes.data, 1, 0, 1, None, 1, 0, out.ctypes.data, None, None, None) == \
        native.JSP_EINVAL and b"NULL" in lib.jsp_last_error()                                    # peer_ids
    ok()
    assert raw(zero.ctypes.data, one.ctypes.data, 1, 0, 1, own.ctypes.data, 1, 0, out.ctypes.data, None, None,
               None) == native.JSP_OK                                                            # every nullable NULL
    assert out[0] == 0
    a, sp, cnt, st = engine.place_spread_runs([], [], s, k, peers)                               # J == 0: the peers still
    assert a.shape == (0,) and sp.shape == (0,)
    np.testing.assert_array_equal(cnt, peers_ref(p, s, peers))
    assert (st.jobs, st.placed, st.refused, st.skew, st.runs, st.fused) == (0, 0, 0, 0, 0, 7)
    q, s2, k2, peers2 = hand_cases()["peer-crosses"][:4]
    engine.load(q)
    np.testing.assert_array_equal(engine.place_spread_runs([], [], s2, k2, peers2)[2], [1, 1])
    np.testing.assert_array_equal(engine.place_spread_runs([0], [0], s2, k2, peers2)[2], [1, 1])  # an empty run


def test_device_set_sharded_and_unloaded_engines_are_estate():
    from jobset_amd.snapshot import shard_problem
    p = synth.config5()
    rc, rl = job_runs(p.job_class)
    lvl = min(jc.level for jc in p.classes)
    with Engine(devices=[0, 0]) as multi:
        multi.load(p)
        refused(multi, native.JSP_ESTATE, "device-set", rc, rl, lvl, 1, [5])
        with pytest.raises(native.JspError) as ei:
            multi.spread_tables(lvl, [5])
        assert ei.value.code == native.JSP_ESTATE
    with Engine(0) as e:
        e.upload_topology(p.topology)
        e.upload_snapshot(shard_problem(p, 0, 2))
        e.upload_classes(p.classes)
        refused(e, native.JSP_ESTATE, "sharded", rc, rl, lvl, 1, [5])
        with pytest.raises(native.JspError) as ei:
            e.spread_tables(lvl, [5])
        assert ei.value.code == native.JSP_ESTATE
    lib = native.lib()
    with Engine(0) as e:
        a = np.zeros(1, dtype=np.int32)
        one, zero = np.ones(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        call = lambda: lib.jsp_place_spread(e._h, zero.ctypes.data, one.ctypes.data, 1, 0, 0, None, 0, 0,  # noqa: E731
                                            a.ctypes.data, None, None, None)
        assert call() == native.JSP_ESTATE               # no topology yet
        e.upload_topology(p.topology)
        assert call() == native.JSP_ESTATE               # no snapshot yet
        e.upload_snapshot(p.nodes)
        assert call() == native.JSP_ESTATE               # no classes yet
        e.upload_classes(p.classes)
        assert call() == native.JSP_OK                   # level 0 is finer than no class


def test_class_reupload_with_the_same_geometry(engine):
    """The tables follow the classes: a second upload with the same class
    count and levels but other pods is counted afresh."""
    p = TABLE_CASES["K2-63-64-65"]()
    run(engine, p, 0, 1, TABLES[3])
    q = dataclasses.replace(p, classes=[dataclasses.replace(jc, pods=jc.pods + 1) for jc in p.classes])
    engine.upload_classes(q.classes)
    run(engine, q, 0, 1, TABLES[3], load=False)


# ------------------------------------------------------------------ 7. a real shape, and the timed loop
def test_config5_once(engine):
    p = synth.config5()
    lvl = min(jc.level for jc in p.classes)
    few = dataclasses.replace(p, job_class=p.job_class[:32], job_names=None)
    engine.load(p)
    run(engine, few, lvl, 1, owners_of(p)[:3], load=False)
    rc, rl = job_runs(p.job_class)
    a, sp, cnt, st = engine.place_spread_runs(rc, rl, lvl, SOFT, [])
    assert st.placed > 0 and st.jobs == p.n_jobs and int(cnt.sum()) == st.placed
    total, med, p99, walk = engine.place_spread_loop(rc, rl, lvl, SOFT, [], iters=20)
    assert 0 < walk < med <= p99 and total > 0
