"""The host lease of the resident compaction service: while
nothing has changed the rows, the class, the topology or the service since the
last request that crossed the link, jsp_place expands the lines of that
request's answer on the host and posts nothing (test hook svc_standing=3, the
default). Every placement is compared with the oracle, and the lease's
counters (jspb_lease_counters) and the dispatcher's (jspb_service_counters)
say who answered, so no case passes on the fallback alone.

The snapshots are the standing tests' (cfg2-shaped: 60 / 120 / 540 / 560 /
1000 racks give 1 / 2 / 8 / 9 / 15 tiles). Oracles are computed before the
placements they check: a lease holds for a quarter of the idle limit only."""
import dataclasses
import threading
import time

import numpy as np
import pytest

from jobset_amd import synth
from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from assume_ref import assume_ref, forget_ref
from test_service_standing_gpu import BAD, IDLE_S, PER, TILE_ROWS, TILES, set_taint, snapshot, warm

pytestmark = pytest.mark.gpu


@pytest.fixture
def svc_engine(engine):
    engine.set_service(True)
    engine.set_fused(True)
    yield engine
    engine.set_timing(False)
    engine.service_stop()


def start(engine, monkeypatch, racks, hooks="", trial=0):
    """The snapshot loaded under the hooks (read at upload; none: the
    default, the lease on) and a resident service that has answered one
    request -- the one that crossed the link; the lease's counters at zero."""
    monkeypatch.setenv("JSP_TEST_HOOKS", hooks)
    p = snapshot(racks, trial)
    engine.load(p)
    engine.lease_counters(reset=True)
    warm(engine, p)
    assert engine.lease_counters()["answered"] == 0  # the first request after an upload crosses the link
    engine.metrics(reset=True)
    return p


CROSSED = [0.0]  # when the last placement that crossed the link returned (perf_counter)


def renew(engine, p):
    """A placement without jobs: it always crosses the link, so the lease is
    fresh whatever the host did since the last request (oracles, a slow box)."""
    got = engine.place(p.job_class[:0])
    assert got.fused == 3
    CROSSED[0] = time.perf_counter()


def place(engine, p, want, host, J=None, what=""):
    """One placement of the first J jobs: answered by the service, equal to
    `want`, and answered on the host or not as `host` says (None: either)."""
    before = engine.lease_counters()["answered"]
    got = engine.place(p.job_class if J is None else p.job_class[:J])
    n = engine.lease_counters()["answered"] - before
    since_ms = (time.perf_counter() - CROSSED[0]) * 1e3
    if n == 0:
        CROSSED[0] = time.perf_counter()
    assert got.fused == 3, (what, got.fused)
    np.testing.assert_array_equal(got.assign, want, err_msg=what)
    assert got.placed == int((want >= 0).sum()), what
    if host is not None:
        assert n == (1 if host else 0), (what, "host-answered" if n else "crossed the link",
                                         f"{since_ms:.2f} ms after the last crossing")
    return n


def crossed_then_leased(engine, p, what):
    """After a change: the first placement sees it and is not answered on
    the host; the two after it are, and equal the oracle as well."""
    want = O.place_c(p)[0]
    place(engine, p, want, False, what=f"{what}: first placement after the change")
    for i in range(2):
        place(engine, p, want, True, what=f"{what}: clean placement {i} after it")
    return want


def dispatcher(engine):
    engine.service_stop()
    return engine.service_counters()


@pytest.mark.parametrize("racks", sorted(TILES))
def test_clean_run(svc_engine, monkeypatch, racks):
    """J = all, 1, 0, all, 1, all without a change, after a call that crossed
    the link (the start's was the service's first ring; renew's, without jobs,
    follows the oracles). Of the six, the one without jobs crosses (no lease
    without jobs); every call with jobs is answered on the host, and the
    dispatcher saw exactly the others."""
    p = start(svc_engine, monkeypatch, racks)
    n_all = p.job_class.size
    wants = {J: O.place_c(dataclasses.replace(p, job_class=p.job_class[:J]))[0] for J in (n_all, 1, 0)}
    svc_engine.metrics(reset=True)
    svc_engine.timing(reset=True)
    renew(svc_engine, p)
    host, crossed = 0, 1
    for J in (n_all, 1, 0, n_all, 1, n_all):
        host += place(svc_engine, p, wants[J], J > 0, J=J, what=f"J={J}")
        crossed += 0 if J > 0 else 1
    lc = svc_engine.lease_counters()
    assert lc["answered"] == host == 5 and lc["taken"] == 2 and lc["dropped"] == 0, lc
    t = svc_engine.timing(reset=True)
    assert t.svc_calls == 7 and t.svc_starts == 0 and t.svc_fallbacks == 0
    assert svc_engine.metrics().svc_calls == 7
    c = dispatcher(svc_engine)
    assert c["tiles"] == TILES[racks] and c["evals"] == 1, c  # the start's request: the first ring
    assert c["answered"] + c["handed"] == crossed == 2, c
    assert svc_engine.lease_counters()["dropped"] == 1  # the stop ends the lease


def test_early_answer_then_lease(svc_engine, monkeypatch):
    """A request that crossed the link with one job returns before the last
    tiles' lines (the early answer); the next placement settles it first and
    is then answered on the host from lines that are whole."""
    p = start(svc_engine, monkeypatch, 1000)
    for row in (3 * TILE_ROWS, 14 * TILE_ROWS + 5):
        set_taint(svc_engine, p, [row], [BAD])
        want = O.place_c(p)[0]
        place(svc_engine, p, want[:1], False, J=1, what="one job after the patch")
        place(svc_engine, p, want, True, what="all jobs after the early answer")
        place(svc_engine, p, want[:1], True, J=1)


CHANGES = ["micro_one_row", "micro_two_tiles", "inline_300", "descriptor_5000", "after_idle_exit", "assume_forget",
           "reupload", "class_pods"]


@pytest.mark.parametrize("change", CHANGES)
def test_change_then_crossing_then_two_host_answers(svc_engine, monkeypatch, change):
    """Every way the rows (or the class) change under a held lease: the first
    placement after it crosses the link and sees the change, the two after it
    are answered on the host. (After an idle exit the patch wakes the service
    and its warm-up request carries the patch: that request's lines may answer
    the first placement on the host -- the recovery's case -- so who answers
    that one is not asserted; what it answers is.)"""
    p = start(svc_engine, monkeypatch, 1000)
    N = p.nodes.n_nodes
    before = O.place_c(p)[0]
    renew(svc_engine, p)
    place(svc_engine, p, before, True, what="a lease held before the change")
    if change == "micro_one_row":
        for row in (7 * TILE_ROWS, 8 * TILE_ROWS - 1, N - 1):
            for v in (BAD, 0):
                set_taint(svc_engine, p, [row], [v])
                crossed_then_leased(svc_engine, p, f"row {row} := {int(v)}")
    elif change == "micro_two_tiles":
        a, b = 4 * TILE_ROWS - 1, 4 * TILE_ROWS
        set_taint(svc_engine, p, [a, b], [BAD, BAD])
        assert not np.array_equal(crossed_then_leased(svc_engine, p, "two tiles"), before)
        set_taint(svc_engine, p, [a, 9 * TILE_ROWS + 7], [0, p.nodes.taints[9 * TILE_ROWS + 7]])
        crossed_then_leased(svc_engine, p, "one back")
        set_taint(svc_engine, p, [b], [0])
        np.testing.assert_array_equal(crossed_then_leased(svc_engine, p, "both back"), before)
    elif change == "inline_300":
        rows = np.arange(2 * TILE_ROWS - 150, 2 * TILE_ROWS + 150)
        set_taint(svc_engine, p, rows, synth.bernoulli(7, 1, rows.size, 0.1).astype(np.uint32))
        assert not np.array_equal(crossed_then_leased(svc_engine, p, change), before)
    elif change == "descriptor_5000":
        rows = np.sort(synth.permutation(7, 2, N)[:5000])
        set_taint(svc_engine, p, rows, synth.bernoulli(7, 3, rows.size, 0.02).astype(np.uint32))
        assert not np.array_equal(crossed_then_leased(svc_engine, p, change), before)
    elif change == "after_idle_exit":
        p.nodes.taints[5 * TILE_ROWS] = BAD
        want = O.place_c(p)[0]
        p.nodes.taints[5 * TILE_ROWS] = 0
        time.sleep(IDLE_S * 1.6)  # the service has left; the patch wakes it, its warm-up evaluates
        set_taint(svc_engine, p, [5 * TILE_ROWS], [BAD])
        place(svc_engine, p, want, None, what="first placement after the wake")
        for i in range(2):
            place(svc_engine, p, want, True, what=f"clean placement {i} after the wake")
        assert not np.array_equal(want, before)
    elif change == "assume_forget":
        own = (0x40000000 + np.arange(60)).astype(np.int32)
        new, committed, _ = assume_ref(dataclasses.replace(p, job_class=p.job_class[:60]), before[:60], own)
        got, _ = svc_engine.assume(p.job_class[:60], before[:60], own)
        np.testing.assert_array_equal(got, committed)
        p.nodes.excl[:] = new
        assert not np.array_equal(crossed_then_leased(svc_engine, p, "assume"), before)
        p.nodes.excl[:] = forget_ref(p.nodes.excl, own[::2])[0]
        svc_engine.forget(own[::2])
        crossed_then_leased(svc_engine, p, "forget")
    elif change == "reupload":
        p = snapshot(1000, trial=1)
        svc_engine.upload_snapshot(p.nodes)
        assert not np.array_equal(crossed_then_leased(svc_engine, p, change), before)
    elif change == "class_pods":
        p.classes = [dataclasses.replace(p.classes[0], pods=PER - 1)]
        svc_engine.upload_classes(p.classes)
        assert not np.array_equal(crossed_then_leased(svc_engine, p, change), before)
    assert svc_engine.metrics().svc_fallbacks == 0


def test_lease_ends_before_the_idle_limit(svc_engine, monkeypatch):
    """A host answer does not keep the service alive. Past a quarter of the
    idle limit the next call crosses the link (and restarts nothing); past
    half of it the next call crosses as well (a restart, as ever); the call
    after either is answered on the host again."""
    p = start(svc_engine, monkeypatch, 560)
    want = O.place_c(p)[0]
    renew(svc_engine, p)
    place(svc_engine, p, want, True)
    for frac, restarts in ((0.3, 0), (0.6, 1)):
        svc_engine.timing(reset=True)
        time.sleep(frac * IDLE_S)
        place(svc_engine, p, want, False, what=f"after {frac} of the idle limit")
        place(svc_engine, p, want, True, what="the call after it")
        place(svc_engine, p, want, True)
        assert svc_engine.timing(reset=True).svc_starts == restarts


@pytest.mark.parametrize("how", ["svc_standing=0", "svc_standing=1", "svc_standing=2", "timing", "svc_entries=1",
                                 "cfg3", "cfg5"])
def test_paths_the_lease_leaves_alone(svc_engine, monkeypatch, how):
    """The older modes of the hook, the device stamps on, the per-job entries
    answer and the split shapes: exact, and not one host answer."""
    if how == "timing":
        svc_engine.set_timing(True)
    if how.startswith("cfg"):
        monkeypatch.setenv("JSP_TEST_HOOKS", "")
        p = synth.CONFIGS[int(how[3:])]()
        svc_engine.load(p)
        svc_engine.lease_counters(reset=True)
        want = O.place_c(p)[0]
        for i in range(6):
            got = svc_engine.place(p.job_class)
            assert got.fused == 5 or i == 0, (i, got.fused)  # (the first may find the service still starting)
            np.testing.assert_array_equal(got.assign, want)
    else:
        p = start(svc_engine, monkeypatch, 560, "" if how == "timing" else how)
        want = O.place_c(p)[0]
        for i in range(4):
            place(svc_engine, p, want, False, what=f"{how}: placement {i}")
        set_taint(svc_engine, p, [TILE_ROWS], [BAD])
        want = O.place_c(p)[0]
        for i in range(3):
            place(svc_engine, p, want, False, what=f"{how}: placement {i} after a patch")
    lc = svc_engine.lease_counters()
    assert lc["answered"] == 0 and lc["taken"] == 0, lc
    svc_engine.set_timing(False)


def test_no_lease_from_a_request_that_failed(svc_engine, monkeypatch):
    """micro_spins=0: the request that carries a micro-patch fails (a tile
    gives up its microbox wait and writes no line) and is answered on the
    launch path. Nothing is answered on the host until a request has crossed
    the link again and left whole lines."""
    p = start(svc_engine, monkeypatch, 1000, "micro_spins=0")
    a0 = O.place_c(p)[0]
    renew(svc_engine, p)
    place(svc_engine, p, a0, True)
    r = int(p.nodes.leaf_start[int(a0[3])])
    svc_engine.metrics(reset=True)
    set_taint(svc_engine, p, [r], [p.nodes.taints[r] | BAD])
    want = O.place_c(p)[0]
    assert not np.array_equal(want, a0)
    before = svc_engine.lease_counters()["answered"]
    got = svc_engine.place(p.job_class)
    np.testing.assert_array_equal(got.assign, want)
    assert got.fused != 3 and svc_engine.metrics().svc_fallbacks == 1
    assert svc_engine.lease_counters()["answered"] == before
    place(svc_engine, p, want, False, what="the fresh service's first request")
    place(svc_engine, p, want, True)


def test_recovery_loop(svc_engine, monkeypatch):
    """The cold recovery, 20 trials timed in C: the idle exit, a one-row patch
    that changes the answer, a 1 ms gap, jsp_place. The patch wakes the
    service, whose warm-up request carries it; the placement may be answered
    from that request's lines. Every trial is exact; how many were answered
    on the host is reported."""
    p = start(svc_engine, monkeypatch, 1000)
    a0 = O.place_c(p)[0]
    r = int(p.nodes.leaf_start[int(a0[500])])
    call = svc_engine.host_placer(*job_runs(p.job_class))
    wants = {}
    for v in (BAD, 0):
        p.nodes.taints[r] = v
        wants[int(v)] = O.place_c(p)[0]
    assert not np.array_equal(wants[int(BAD)], wants[0])
    host = 0
    us = []
    for t in range(20):
        v = BAD if t % 2 == 0 else 0
        before = svc_engine.lease_counters()["answered"]
        out = call.recovery(1, IDLE_S * 1.6e6, 1000.0, np.array([r]), np.array([v]))
        host += svc_engine.lease_counters()["answered"] - before
        us.append(float(out[0, 1]))
        np.testing.assert_array_equal(call.assign, wants[int(v)], err_msg=f"trial {t}")
    print(f"recovery: {host}/20 placements answered on the host; place p50 {np.median(us):.2f} us")
    assert svc_engine.metrics().svc_fallbacks == 0


def test_four_threads_on_one_engine(svc_engine, monkeypatch):
    """One thread toggles a row's taint between two values, three threads
    place. Every answer is one of the two states' answers, and the placement
    after the join is the final state's."""
    p = start(svc_engine, monkeypatch, 1000)
    a0 = O.place_c(p)[0]
    r = int(p.nodes.leaf_start[int(a0[400])])
    wants = {}
    for v in (BAD, 0):
        p.nodes.taints[r] = v
        wants[int(v)] = O.place_c(p)[0]
    assert not np.array_equal(wants[int(BAD)], wants[0])
    errors = []
    stop = threading.Event()

    def toggler():
        try:
            for i in range(300):
                svc_engine.patch_rows(np.array([r], dtype=np.uint32), taints=np.array([BAD if i % 2 == 0 else 0],
                                                                                   dtype=np.uint32))
        except Exception as ex:  # noqa: BLE001
            errors.append(repr(ex))
        finally:
            stop.set()

    def placer(k):
        try:
            call = svc_engine.host_placer(*job_runs(p.job_class))
            n = 0
            while not stop.is_set() or n < 50:
                st = call()
                n += 1
                if not (np.array_equal(call.assign, wants[0]) or np.array_equal(call.assign, wants[int(BAD)])):
                    errors.append(f"thread {k} call {n}: neither state's answer (fused {st.fused})")
                    return
        except Exception as ex:  # noqa: BLE001
            errors.append(repr(ex))

    threads = [threading.Thread(target=toggler)] + [threading.Thread(target=placer, args=(k,)) for k in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    final = wants[0]  # the 300th patch (i = 299) wrote 0
    place(svc_engine, p, final, None, what="after the join")
    place(svc_engine, p, final, True)
    lc = svc_engine.lease_counters()
    print(f"four threads: {lc}")
