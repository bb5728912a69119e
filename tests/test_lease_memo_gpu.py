"""The lease's kept list ("the kept list"): under the host
lease the first host answer expands the lines as ever, the second builds the
list of feasible leaves the lines expand to, and every later one copies its
answer from that list after checking the lines' tags. Every placement is
compared with the oracle, and jspb_lease_memo_counters (answers copied from a
list -- the call that built it included -- and lists built) say which path
answered, beside jspb_lease_counters.

The build rule in numbers, for host answers H1 H2 H3 .. of one lease: H1
expands (0 copied, 0 built); H2 builds with its own J (1, 1); H3.. copy
(+1, +0) unless one asks for more jobs than an incomplete list holds, which
builds again with that J (+1, +1). A list is complete when the lines ran out
before the jobs did.

The snapshots, helpers and the pacing (oracles before the placements they
check: a lease holds for a quarter of the idle limit) are the lease tests'."""
import dataclasses
import threading
import time

import numpy as np
import pytest

from jobset_amd.snapshot import JobClass, job_runs
from oracle import oracle as O
from assume_ref import assume_ref, forget_ref
from test_service_standing_gpu import BAD, IDLE_S, PER, TILES, set_taint
from test_service_lease_gpu import renew, start

pytestmark = pytest.mark.gpu


@pytest.fixture
def svc_engine(engine):
    engine.set_service(True)
    engine.set_fused(True)
    yield engine
    engine.set_timing(False)
    engine.service_stop()


def oracle_for(p, J):
    """The oracle's answer for J jobs of the one class (J may exceed p's)."""
    return O.place_c(dataclasses.replace(p, job_class=np.zeros(J, dtype=np.uint32)))[0]


def place_j(engine, p, J, want, host, memo, what=""):
    """One placement of J jobs (J may exceed p's job count): equal to `want`,
    answered on the host or not as `host` says, and from a kept list or not as
    `memo` says (None: either). Returns the lists built by it."""
    lc, mc = engine.lease_counters(), engine.lease_memo_counters()
    got = engine.place(np.zeros(J, dtype=np.uint32))
    n_host = engine.lease_counters()["answered"] - lc["answered"]
    after = engine.lease_memo_counters()
    n_memo, n_built = after["answered"] - mc["answered"], after["built"] - mc["built"]
    assert got.fused == 3, (what, got.fused)
    np.testing.assert_array_equal(got.assign, want, err_msg=what)
    assert got.placed == int((want >= 0).sum()), what
    assert n_host == (1 if host else 0), (what, "host-answered" if n_host else "crossed the link")
    if memo is not None:
        assert n_memo == (1 if memo else 0), (what, "from a list" if n_memo else "not from a list")
    assert n_built <= n_memo, what
    return n_built


@pytest.mark.parametrize("racks", [60, 560, 1000])
def test_clean_run(svc_engine, monkeypatch, racks):
    """After a crossing: J = all, all, 1, all, J_over, all. All six are host
    answers; the first expands, the second builds the list (J = all), the
    third and fourth copy, the fifth asks for more than the list holds --
    more jobs than there are feasible leaves, a -1 tail -- and builds it
    again unless the first list was complete already (all > nF), the sixth
    copies: copied 5, built 2 (or 1)."""
    p = start(svc_engine, monkeypatch, racks)
    n_all = p.job_class.size
    J_over = racks + 5
    wants = {J: oracle_for(p, J) for J in (n_all, 1, J_over)}
    nF = int((wants[J_over] >= 0).sum())
    assert 0 < nF < J_over and (wants[J_over][nF:] == -1).all() and (wants[J_over][:nF] >= 0).all()
    svc_engine.lease_memo_counters(reset=True)
    renew(svc_engine, p)
    built = []
    for i, J in enumerate((n_all, n_all, 1, n_all, J_over, n_all)):
        built.append(place_j(svc_engine, p, J, wants[J], True, i > 0, what=f"call {i}, J={J}"))
    first_complete = n_all > nF
    assert built == [0, 1, 0, 0, 0 if first_complete else 1, 0], built
    mc, lc = svc_engine.lease_memo_counters(), svc_engine.lease_counters()
    assert mc == {"answered": 5, "built": 1 if first_complete else 2}, mc
    assert lc["answered"] == 6 and lc["taken"] == 1 and lc["dropped"] == 0, lc
    svc_engine.service_stop()
    c = svc_engine.service_counters()
    assert c["tiles"] == TILES[racks] and c["answered"] + c["handed"] == 1, c  # renew's: nothing else crossed


CHANGES = ["taint_one_row", "micro_two_rows", "assume_forget", "classes", "service_stop", "timing_on_off"]


@pytest.mark.parametrize("racks", [60, 1000])
@pytest.mark.parametrize("change", CHANGES)
def test_stale_list(svc_engine, monkeypatch, change, racks):
    """Crossing, host answer, answer from a list, a change, three placements:
    the first crosses, the second is a host answer not from a list, the third
    is from a list, and all three equal the oracle of the changed snapshot.
    The change flips the feasibility of one of the first ten racks, so the
    kept list is wrong for most jobs from there on. (service_stop and timing
    on / off change no row themselves: the row's patch goes with them, while
    the service is stopped / the stamps are on.)"""
    p = start(svc_engine, monkeypatch, racks)
    n_all = p.job_class.size
    before = oracle_for(p, n_all)
    rack = int(before[2])
    assert rack < 10
    row = int(p.nodes.leaf_start[rack])
    renew(svc_engine, p)
    place_j(svc_engine, p, n_all, before, True, False, what="host answer before the change")
    assert place_j(svc_engine, p, n_all, before, True, True, what="from a list before the change") == 1
    if change == "taint_one_row":
        set_taint(svc_engine, p, [row], [BAD])
    elif change == "micro_two_rows":
        last = p.nodes.n_nodes - 1
        set_taint(svc_engine, p, [row + 3, last], [BAD, BAD])
    elif change == "assume_forget":
        k = 10
        own = (0x40000000 + np.arange(k)).astype(np.int32)
        new, committed, _ = assume_ref(dataclasses.replace(p, job_class=p.job_class[:k]), before[:k], own)
        got, _ = svc_engine.assume(p.job_class[:k], before[:k], own)
        np.testing.assert_array_equal(got, committed)
        p.nodes.excl[:] = forget_ref(new, own[::2])[0]
        svc_engine.forget(own[::2])
    elif change == "classes":
        # one more required label bit, which a node of nearly every rack lacks
        p.classes = [JobClass(req_labels=(3,), level=0, pods=PER, req_res=p.classes[0].req_res)]
        svc_engine.upload_classes(p.classes)
    elif change == "service_stop":
        svc_engine.service_stop()
        set_taint(svc_engine, p, [row], [BAD])
    elif change == "timing_on_off":
        svc_engine.set_timing(True)
        set_taint(svc_engine, p, [row], [BAD])
        svc_engine.set_timing(False)
    want = oracle_for(p, n_all)
    feas = lambda a: set(int(x) for x in a[a >= 0] if x < 10)  # noqa: E731
    assert feas(want) != feas(before), "the change flips no rack of the first ten"
    assert (want != before).mean() > 0.5, "the changed answer differs from the kept list in most entries"
    place_j(svc_engine, p, n_all, want, False, False, what=f"{change}: the first placement crosses")
    place_j(svc_engine, p, n_all, want, True, False, what=f"{change}: a host answer, not from a list")
    assert place_j(svc_engine, p, n_all, want, True, True, what=f"{change}: from a list built after it") == 1
    assert svc_engine.metrics().svc_fallbacks == 0


def test_renewal(svc_engine, monkeypatch):
    """Past a quarter of the idle limit the next call crosses under a new
    request number; the call after it expands, the one after that builds a
    list again."""
    p = start(svc_engine, monkeypatch, 1000)
    n_all = p.job_class.size
    want = oracle_for(p, n_all)
    renew(svc_engine, p)
    place_j(svc_engine, p, n_all, want, True, False)
    assert place_j(svc_engine, p, n_all, want, True, True) == 1
    assert place_j(svc_engine, p, n_all, want, True, True) == 0
    built = svc_engine.lease_memo_counters()["built"]
    time.sleep(0.3 * IDLE_S)
    place_j(svc_engine, p, n_all, want, False, False, what="after 0.3 of the idle limit")
    place_j(svc_engine, p, n_all, want, True, False, what="the call after it")
    assert place_j(svc_engine, p, n_all, want, True, True, what="the one after that") == 1
    assert place_j(svc_engine, p, n_all, want, True, True) == 0
    assert svc_engine.lease_memo_counters()["built"] == built + 1


@pytest.mark.parametrize("racks", [60, 1000])
def test_hook_off(svc_engine, monkeypatch, racks):
    """lease_memo=0: the same answers, the same host answers, and no list."""
    p = start(svc_engine, monkeypatch, racks, "lease_memo=0")
    n_all = p.job_class.size
    J_over = racks + 5
    wants = {J: oracle_for(p, J) for J in (n_all, 1, J_over)}
    svc_engine.lease_memo_counters(reset=True)
    renew(svc_engine, p)
    for i, J in enumerate((n_all, n_all, 1, n_all, J_over, n_all)):
        place_j(svc_engine, p, J, wants[J], True, False, what=f"call {i}, J={J}")
    lc = svc_engine.lease_counters()
    assert lc["answered"] == 6 and lc["taken"] == 1 and lc["dropped"] == 0, lc
    assert svc_engine.lease_memo_counters() == {"answered": 0, "built": 0}


def test_four_threads_each_its_own_j(svc_engine, monkeypatch):
    """Four threads on one engine, J = 1, nF - 1, all, J_over, 200 calls each:
    every answer is its J's oracle answer, whoever built the list it came
    from and with whichever J."""
    racks = 1000
    p = start(svc_engine, monkeypatch, racks)
    J_over = racks + 5
    nF = int((oracle_for(p, J_over) >= 0).sum())
    Js = [1, nF - 1, p.job_class.size, J_over]
    wants = {J: oracle_for(p, J) for J in Js}
    errors = []

    def placer(J):
        try:
            call = svc_engine.host_placer(*job_runs(np.zeros(J, dtype=np.uint32)))
            for n in range(200):
                st = call()
                if st.fused != 3 or not np.array_equal(call.assign, wants[J]):
                    errors.append(f"J={J} call {n}: not the oracle's answer (fused {st.fused})")
                    return
        except Exception as ex:  # noqa: BLE001
            errors.append(repr(ex))

    svc_engine.lease_memo_counters(reset=True)
    threads = [threading.Thread(target=placer, args=(J,), daemon=True) for J in Js]
    for t in threads:
        t.start()
    deadline = time.monotonic() + 60.0
    for t in threads:
        t.join(max(deadline - time.monotonic(), 0.0))
        assert not t.is_alive(), "a placing thread did not finish within 60 s"
    assert not errors, errors
    mc = svc_engine.lease_memo_counters()
    print(f"four threads: lease {svc_engine.lease_counters()} list {mc}")
    assert mc["answered"] > 0 and mc["built"] > 0, mc


def test_accounting(svc_engine, monkeypatch):
    """50 answers from a list: the call histogram, the metrics' and the phase
    clocks' call counts each grow by 50, and the calls' wall is accounted."""
    p = start(svc_engine, monkeypatch, 1000)
    n_all = p.job_class.size
    want = oracle_for(p, n_all)
    call = svc_engine.host_placer(*job_runs(p.job_class))
    for attempt in range(3):  # (a slow box: the 50 must fit a quarter of the idle limit)
        renew(svc_engine, p)
        place_j(svc_engine, p, n_all, want, True, False)
        assert place_j(svc_engine, p, n_all, want, True, True) == 1
        m0, mc0, lc0 = svc_engine.metrics(), svc_engine.lease_memo_counters(), svc_engine.lease_counters()
        svc_engine.timing(reset=True)
        for _ in range(50):
            st = call()
        t = svc_engine.timing(reset=True)
        m1, mc1, lc1 = svc_engine.metrics(), svc_engine.lease_memo_counters(), svc_engine.lease_counters()
        if mc1["answered"] - mc0["answered"] == 50:
            break
    assert mc1["answered"] - mc0["answered"] == 50 and mc1["built"] == mc0["built"], (mc0, mc1)
    assert lc1["answered"] - lc0["answered"] == 50
    np.testing.assert_array_equal(call.assign, want)
    assert st.fused == 3 and st.placed == int((want >= 0).sum()) and st.wall_us > 0
    assert m1.place_us.count - m0.place_us.count == 50
    assert m1.svc_calls - m0.svc_calls == 50
    assert t.host_calls == 50 and t.svc_calls == 50
    assert t.host_prep_us + t.host_wait_us > 0
    assert t.host_prep_us == 0 and t.svc_pre_us == 0 and t.svc_answer_us == t.host_wait_us
