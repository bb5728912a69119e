"""jsp_place_gangs on the GPU against the rule restated over the CPU oracle
(tests/gang_ref.py; it never calls the engine). Every comparison is exact:
assign[] and gang_span_out[] bit for bit, the span counts word for word with
numpy (tests/test_gang.py asserts the sweep's coverage floors on the
reference's own output)."""
import dataclasses

import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import shard_problem
from oracle import oracle as O
from bind_ref import cls, nested
from gang_ref import (ANY, SWEEP_SEEDS, check_gangs, gang_ref, gang_runs_of, reduction_problem, span_counts_ref,
                      sweep_case)

pytestmark = pytest.mark.gpu


def run(engine, p, gang_jobs, gang_span, load=True):
    """Load p, place its gangs, compare with the yardstick. Returns (assign, span_out, stats)."""
    if load:
        engine.load(p)
    tl = O.place_c(p)[1:]
    want, want_span = gang_ref(p, gang_jobs, gang_span, tl)
    rc, rl, gr = gang_runs_of(p.job_class, gang_jobs)
    got, span, st = engine.place_gangs_runs(rc, rl, gr, gang_span)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(span, want_span)
    check_gangs(p, gang_jobs, gang_span, got, span, tl)
    assert (st.jobs, st.placed) == (p.n_jobs, int((want >= 0).sum()))
    assert (st.gangs, st.gangs_placed) == (len(gang_jobs), int((want_span >= 0).sum()))
    assert st.runs == len(rc) and st.fused == 7
    return got, span, st


# ------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_sweep(engine, seed):
    p, gj, gs = sweep_case(seed)
    run(engine, p, gj, gs)
    # the same gangs through one class id and one gang id per job
    got, span, _ = engine.place_gangs(p.job_class, np.repeat(np.arange(len(gj)), gj), gs)
    want, want_span = gang_ref(p, gj, gs)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(span, want_span)


# ------------------------------------------------------------------ 2. the two reductions, on the engine's own jsp_place
@pytest.mark.parametrize("i", range(0, 60, 2))
def test_reductions(engine, i):
    p = reduction_problem(i)
    engine.load(p)
    plain = engine.place(p.job_class).assign.copy()
    J = p.n_jobs
    got, span, st = engine.place_gangs(p.job_class, np.arange(J), np.full(J, ANY))
    np.testing.assert_array_equal(got, plain)
    np.testing.assert_array_equal(span, np.where(plain >= 0, 0, -1))
    got, span, st = engine.place_gangs(p.job_class, np.zeros(J, dtype=np.int64), [ANY])
    if J > 0 and np.all(plain >= 0):
        np.testing.assert_array_equal(got, plain)
        assert span[0] == 0 and st.gangs_placed == 1
    else:
        assert np.all(got == -1) and span[0] == -1 and st.placed == 0


# ------------------------------------------------------------------ 3. the span counts against numpy
def count_case(first_leaf, levels, rows=None, seed=1):
    """One row per leaf (or rows[l]), 40 % of the rows tainted with bit 0; per
    level in `levels` one class that tolerates nothing and one that tolerates
    bit 0, one pod each; every 37th leaf's rows held by another job."""
    L = len(first_leaf[-1]) - 1
    rows = np.ones(L, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    N = int(rows.sum())
    taints = synth.bernoulli(seed, 11, N, 0.4).astype(np.uint32)
    leaf_of = np.repeat(np.arange(L), rows)
    excl = np.where(leaf_of % 37 == 36, 900, -1)
    classes = [cls(k, 1, tol=t) for k in levels for t in (0, 1)]
    return nested(first_leaf, rows, classes, [], taints=taints, excl=excl)


def ident(n):
    return np.arange(n + 1)


def edges(n):
    """level-0 boundaries at and one off the 64-bit word boundaries below n"""
    return np.array(sorted({0, n} | {b for b in (1, 63, 64, 65, 127, 128, 129) if b < n}))


COUNT_CASES = {
    # K = 1: only s == level (and ANY, the host's sum)
    **{f"K1-D{n}": lambda n=n: count_case([ident(n)], [0]) for n in (1, 63, 64, 65, 128, 129)},
    # K = 2: span boundaries exactly at and one off a word boundary; classes at both levels in one upload
    **{f"K2-D{n}": lambda n=n: count_case([edges(n), ident(n)], [1, 0]) for n in (1, 63, 64, 65, 128, 129)},
    # span domains without children (empty level-0 domains, in front, in the middle, at the end)
    "K2-empty-spans": lambda: count_case([[0, 0, 64, 64, 64, 130, 130], ident(130)], [1, 0]),
    # span domains whose leaves have no rows
    "K2-rowless": lambda: count_case([[0, 3, 70, 140], ident(140)], [1, 0],
                                     rows=[0, 0, 0] + [1] * 61 + [0] * 6 + [2] * 70),
    "K3": lambda: count_case([[0, 50, 50, 192, 200],
                              sorted(set(range(0, 50, 2)) | set(range(50, 192, 7)) | {192, 200}), ident(200)], [2, 0, 1]),
    "K4": lambda: count_case([[0, 75, 75, 200], np.arange(0, 201, 25), np.arange(0, 201, 5), ident(200)],
                             [3, 1, 0, 2]),
    # long segments: the wave form by the engine's own choice (2 zones x 700 racks) beside short ones
    "K3-long": lambda: count_case([[0, 700, 1400], np.r_[np.arange(0, 700, 7), np.arange(700, 1401, 350)],
                                   ident(1400)], [2, 1, 0]),
}


@pytest.mark.parametrize("name", list(COUNT_CASES))
def test_span_counts_match_numpy(engine, name):
    p = COUNT_CASES[name]()
    p.topology.validate()
    engine.load(p)
    cap, occ = O.place_c(p)[1:]
    want = span_counts_ref(p, cap, occ)
    assert want.shape[0] == sum(sum(p.topology.n_domains[:jc.level + 1]) for jc in p.classes)
    assert 0 < int(want.sum())  # the case is not empty
    for form in (0, 1, 2):
        got, _ = engine.span_counts(want.shape[0], form=form)
        np.testing.assert_array_equal(got, want, err_msg=f"{name} form {form}")
    with pytest.raises(native.JspError) as ei:
        engine.span_counts(want.shape[0] + 1)
    assert ei.value.code == native.JSP_EINVAL


def test_span_counts_time_their_launches(engine):
    p = COUNT_CASES["K3-long"]()
    engine.load(p)
    n = sum(sum(p.topology.n_domains[:jc.level + 1]) for jc in p.classes)
    _, (med, mean) = engine.span_counts(n, iters=20)
    assert 0 < med < 1e4 and 0 < mean < 1e4


# ------------------------------------------------------------------ 4. rollback
def rollback_case():
    """3 zones x 4 racks, one row per rack. Zone 0: rack 0 clean, rack 1 tainted
    with bit 0, racks 2-3 with bit 1 (nobody tolerates it); zones 1-2 clean.
    Classes: 0 rack / tolerates bit 0, 1 rack / tolerates nothing, 2 zone /
    tolerates bit 0."""
    taints = [0, 1, 2, 2] + [0] * 8
    return nested([[0, 4, 8, 12], ident(12)], [1] * 12, [cls(1, 1, tol=1), cls(1, 1), cls(0, 1, tol=1)],
                  [0, 1, 2, 1], taints=taints)


def test_failed_trial_leaves_no_mark(engine):
    """Gang 0 (a tolerant and a strict rack job, span 0): zone 0's counts pass
    (2 and 1), its trial fails after the tolerant job took rack 0 and marked
    zone 0; zone 1 succeeds. Gang 1 (a zone job) then still gets zone 0, which
    the failed trial touched, and gang 2's rack job goes on behind zone 1's."""
    p = rollback_case()
    got, span, _ = run(engine, p, [2, 1, 1], [0, 0, ANY])
    np.testing.assert_array_equal(got, [4, 5, 0, 6])
    np.testing.assert_array_equal(span, [1, 0, 0])
    # the same jobs as one gang over the whole cluster: whole; with a span it cannot have: refused whole
    got, span, _ = run(engine, p, [4], [ANY], load=False)
    np.testing.assert_array_equal(got, [0, 4, 2, 5])
    p2 = dataclasses.replace(p, job_class=np.array([0, 1, 1, 1, 1, 1], dtype=np.uint32))
    got, span, st = run(engine, p2, [6], [1], load=False)   # span == the class level: six jobs in one rack
    assert np.all(got == -1) and span[0] == -1 and st.gangs_placed == 0


def test_empty_gangs_and_empty_runs(engine):
    p = rollback_case()
    engine.load(p)
    rc = np.array([0, 1, 1, 2], dtype=np.uint32)
    rl = np.array([1, 0, 1, 0], dtype=np.uint32)
    got, span, st = engine.place_gangs_runs(rc, rl, [0, 2, 0, 2, 0], [0, 0, 1, ANY, ANY])
    np.testing.assert_array_equal(got, [0, 4])          # gang 1: rack 0 alone in zone 0; gang 3: the next clean rack
    np.testing.assert_array_equal(span, [-1, 0, -1, 0, -1])
    assert (st.gangs, st.gangs_placed, st.jobs, st.placed, st.runs) == (5, 2, 2, 2, 2)
    got, span, st = engine.place_gangs_runs([], [], [], [])
    assert got.shape == (0,) and span.shape == (0,) and st.jobs == 0


# ------------------------------------------------------------------ 5. snapshot changes are seen
def rows_of(p, level, d):
    fl = p.topology.first_leaf[level]
    ls = p.nodes.leaf_start
    return np.arange(int(ls[int(fl[d])]), int(ls[int(fl[d + 1])]))


def test_patch_and_assume_between_calls(engine):
    p, gj, gs = sweep_case(3)
    got0, span0, _ = run(engine, p, gj, gs)
    assert (span0 >= 0).any()
    # a patch: every row of the first placed job's domain gets a taint nobody tolerates
    j = int(np.nonzero(got0 >= 0)[0][0])
    rows = rows_of(p, p.classes[int(p.job_class[j])].level, int(got0[j]))
    p.nodes.taints[rows] |= np.uint32(1 << 20)
    engine.patch_rows(rows.astype(np.uint32), taints=p.nodes.taints[rows])
    got1, span1, _ = run(engine, p, gj, gs, load=False)   # at once: ordered after the patch
    assert got1[j] != got0[j]
    # an assume of that answer: its domains are closed to the next call
    own = 0x40000000 + np.arange(p.n_jobs)
    committed, _ = engine.assume(p.job_class, got1, own)
    assert committed.sum() == (got1 >= 0).sum() > 0
    for jj in np.nonzero(got1 >= 0)[0]:
        p.nodes.excl[rows_of(p, p.classes[int(p.job_class[jj])].level, int(got1[jj]))] = own[jj]
    got2, _, _ = run(engine, p, gj, gs, load=False)
    held = {(p.classes[int(p.job_class[jj])].level, int(got1[jj])) for jj in np.nonzero(got1 >= 0)[0]}
    assert not held & {(p.classes[int(p.job_class[jj])].level, int(got2[jj])) for jj in np.nonzero(got2 >= 0)[0]}
    engine.forget(own)


# ------------------------------------------------------------------ 6. the resident service stays up
def test_service_stays_up_across_the_call(engine):
    engine.set_service(True)
    engine.set_fused(True)
    try:
        p = synth.config2()
        engine.load(p)
        for _ in range(4):
            if engine.place(p.job_class).fused == 3:
                break
        assert engine.place(p.job_class).fused == 3
        m0 = engine.metrics()
        r = int(O.place_c(p)[0][5])
        row = next(n for n in range(r * 15, r * 15 + 15) if p.nodes.taints[n] == 0)
        engine.patch_rows(np.array([row], dtype=np.uint32), taints=np.array([1], dtype=np.uint32))
        p.nodes.taints[row] = 1
        gj = np.full(99, 10)
        got, span, st = run(engine, p, gj, np.full(99, ANY), load=False)   # behind the patch the dispatcher holds
        assert st.gangs_placed >= 90
        m1 = engine.metrics()
        assert m1.place_us.count == m0.place_us.count + 1 and m1.batch_jobs.count == m0.batch_jobs.count + 1
        assert m1.placed == m0.placed + st.placed and m1.unplaceable == m0.unplaceable + (st.jobs - st.placed)
        after = engine.place(p.job_class)                                   # the service kept its tiles
        assert after.fused == 3
        np.testing.assert_array_equal(after.assign, O.place_c(p)[0])
        with pytest.raises(native.JspError):
            engine.place_gangs_runs([0], [990], [1], [0], flags=1)
        assert engine.metrics().place_errors == m1.place_errors + 1
    finally:
        engine.service_stop()


# ------------------------------------------------------------------ 7. refusals
def refused(engine, code, word, *args, **kw):
    with pytest.raises(native.JspError) as ei:
        engine.place_gangs_runs(*args, **kw)
    assert ei.value.code == code, str(ei.value)
    assert word in str(ei.value), str(ei.value)


def test_refusals_name_the_gang_and_leave_the_engine_usable(engine):
    p = rollback_case()                       # K = 2; classes 0, 1 at level 1, class 2 at level 0
    engine.load(p)
    rc, rl = [0, 1, 2], [1, 1, 1]
    refused(engine, native.JSP_EINVAL, "gang", rc, rl, [2, 1], [0, 0], flags=2)
    refused(engine, native.JSP_EINVAL, "gang 1", rc, rl, [2, 2], [0, 0])          # the gangs' runs pass n_runs
    refused(engine, native.JSP_EINVAL, "gang 1", rc, rl, [1, 1], [0, 0])          # ... or fall short of it
    refused(engine, native.JSP_EINVAL, "gang 1", rc, rl, [2, 1], [0, 2])          # a level that does not exist
    refused(engine, native.JSP_EINVAL, "gang 1", rc, rl, [2, 1], [0, 1])          # finer than the zone class
    refused(engine, native.JSP_EINVAL, "gang 0", [0, 3, 2], rl, [2, 1], [0, 0])   # a class that does not exist
    refused(engine, native.JSP_EINVAL, "gang", rc, rl, [], [])                    # runs without gangs
    refused(engine, native.JSP_ERANGE, "limit of 65536", [0], [native.JSP_GANG_MAX_JOBS + 1], [1], [ANY])
    lib = native.lib()
    one = np.ones(1, dtype=np.uint32)
    out = np.zeros(4, dtype=np.int32)
    for args in ((None, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, 1, 0, out.ctypes.data),     # run_class
                 (one.ctypes.data, one.ctypes.data, 1, None, one.ctypes.data, 1, 0, out.ctypes.data),     # gang_runs
                 (one.ctypes.data, one.ctypes.data, 1, one.ctypes.data, None, 1, 0, out.ctypes.data),     # gang_span
                 (one.ctypes.data, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, 1, 0, None)):    # assign_out
        assert lib.jsp_place_gangs(engine._h, *args, None, None) == native.JSP_EINVAL
        assert b"NULL" in lib.jsp_last_error() and b"gang" in lib.jsp_last_error()
    # a span equal to the class level is allowed, an empty run of a coarser class under a finer span too
    got, span, _ = engine.place_gangs_runs([0, 2, 1], [1, 0, 1], [3], [1])
    assert np.all(got == -1) and span[0] == -1     # two jobs, one rack
    got, span, _ = engine.place_gangs_runs([0, 2], [1, 0], [2], [1])
    np.testing.assert_array_equal(got, [0])
    np.testing.assert_array_equal(span, [0])
    run(engine, p, [2, 1, 1], [0, 0, ANY], load=False)


def test_device_set_sharded_and_unloaded_engines_are_estate():
    p = synth.config5()
    J = p.n_jobs
    rc, rl, gr = gang_runs_of(p.job_class, np.ones(J, dtype=np.int64))
    with Engine(devices=[0, 0]) as multi:
        multi.load(p)
        refused(multi, native.JSP_ESTATE, "device-set", rc, rl, gr, np.full(J, ANY))
    with Engine(0) as e:
        e.upload_topology(p.topology)
        e.upload_snapshot(shard_problem(p, 0, 2))
        e.upload_classes(p.classes)
        refused(e, native.JSP_ESTATE, "sharded", rc, rl, gr, np.full(J, ANY))
        with pytest.raises(native.JspError) as ei:
            e.span_counts(1)
        assert ei.value.code == native.JSP_ESTATE
    lib = native.lib()
    with Engine(0) as e:
        a = np.zeros(1, dtype=np.int32)
        one, zero = np.ones(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        call = lambda: lib.jsp_place_gangs(e._h, zero.ctypes.data, one.ctypes.data, 1, one.ctypes.data,  # noqa: E731
                                           zero.ctypes.data, 1, 0, a.ctypes.data, None, None)
        assert call() == native.JSP_ESTATE               # no topology yet
        e.upload_topology(p.topology)
        assert call() == native.JSP_ESTATE               # no snapshot yet
        e.upload_snapshot(p.nodes)
        assert call() == native.JSP_ESTATE               # no classes yet
        e.upload_classes(p.classes)
        assert call() == native.JSP_OK


# ------------------------------------------------------------------ 8. one real shape
def cfg5_gangs():
    """config5's 496 rack JobSets regrouped into 124 gangs of 4, each inside one zone."""
    p = synth.config5()
    rack = np.array([p.classes[int(c)].level == 1 for c in p.job_class])
    q = dataclasses.replace(p, job_class=np.ascontiguousarray(p.job_class[rack]), job_names=None)
    assert q.n_jobs == 496
    return q, np.full(124, 4), np.zeros(124, dtype=np.int64)


def test_config5_rack_jobsets_in_gangs_of_four(engine):
    p, gj, gs = cfg5_gangs()
    got, span, st = run(engine, p, gj, gs)
    assert st.gangs_placed == 124 and len(set(span.tolist())) > 1      # several zones fill in turn
    zone = got // 128
    assert np.all(zone.reshape(124, 4) == span[:, None])
    rc, rl, gr = gang_runs_of(p.job_class, gj)
    total, med, p99 = engine.place_gangs_loop(rc, rl, gr, gs, iters=5)
    assert 0 < med <= p99 and total > 0
