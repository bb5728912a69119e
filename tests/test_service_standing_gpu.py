"""Standing answers of the resident compaction service: a
resident tile evaluates when its rows change, not when somebody asks, and the
dispatcher answers a request without a patch from the lines the tiles
published at the last evaluate-ring. Every placement is compared with the
oracle, under the test hook svc_standing = 0 (every request evaluates), 1 (the
tiles' standing answers) and 2 (the dispatcher's too, the default); the
service's counters (jspb_service_counters) say which path answered, so no case
passes on the fallback alone.

Snapshots are cfg2-shaped (flat racks of 15 nodes, one leaf-level class, W = 1,
R = 3): 60, 120, 540, 560 and 1000 racks give 1, 2, 8, 9 and 15 tiles of at
most 68 racks (1,020 rows) -- 8 and 9 are the edges of the dispatcher's
eight-lines-per-store mapping, 15 the headline's."""
import dataclasses
import os
import time

import numpy as np
import pytest

from jobset_amd import synth
from jobset_amd.snapshot import JobClass, Nodes, Problem
from oracle import oracle as O
from assume_ref import assume_ref, forget_ref

pytestmark = pytest.mark.gpu

PER = 15              # nodes per rack
TILE_RACKS = 68       # racks of a full tile: 1,020 rows
TILE_ROWS = TILE_RACKS * PER
TILES = {60: 1, 120: 2, 540: 8, 560: 9, 1000: 15}
MODES = [0, 1, 2]
BAD = np.uint32(1 << 31)  # a taint bit the class does not tolerate
IDLE_S = float(os.environ.get("JSP_SERVICE_IDLE_MS", "50")) / 1e3


def snapshot(racks: int, trial: int = 0) -> Problem:
    """synth.config2 at another rack count, from the same generators."""
    if racks == 1000:
        return synth.config2(trial)
    seed = 2 * 1000 + trial
    N = racks * PER
    topo, leaf_start = synth._flat_topology(synth.RACK_KEY, np.full(racks, PER, dtype=np.int64))
    labels = np.zeros((1, N), dtype=np.uint64)
    labels[0] = synth.random_label_bits(seed, 10, N, 8, 63) | np.uint64(1)
    taints = np.zeros(N, dtype=np.uint32)
    n_bad = max(racks // 100, 2)
    bad_racks = synth.permutation(seed, 20, racks)[:n_bad]
    taints[bad_racks * PER + synth.uniform_int(seed, 21, n_bad, 0, PER - 1)] = 1
    nodes = Nodes(leaf_start=leaf_start, labels=labels, taints=taints, free=synth._full_free(N),
                  excl=np.full(N, -1, dtype=np.int32))
    cls = JobClass(req_labels=(1,), level=0, pods=PER, req_res=(96_000, 1_024_000, 8))
    return Problem(topology=topo, nodes=nodes, classes=[cls], job_class=np.zeros(racks - n_bad, dtype=np.uint32),
                   name=f"cfg2-shaped-{racks}-racks")


@pytest.fixture
def svc_engine(engine):
    engine.set_service(True)
    engine.set_fused(True)
    yield engine
    engine.set_timing(False)
    engine.service_stop()


def start(engine, monkeypatch, racks, mode, extra="", trial=0):
    """The snapshot loaded under the hooks (read at upload) and a resident
    service that has answered once."""
    monkeypatch.setenv("JSP_TEST_HOOKS", f"svc_standing={mode}" + ("," + extra if extra else ""))
    p = snapshot(racks, trial)
    engine.load(p)
    warm(engine, p)
    return p


def warm(engine, p):
    for _ in range(4):
        got = engine.place(p.job_class)
        np.testing.assert_array_equal(got.assign, O.place_c(p)[0])
        if got.fused == 3:
            return got
    raise AssertionError("the resident service did not answer")


def exact(engine, p, n=2):
    """n placements, each answered by the service and equal to the oracle's."""
    want = O.place_c(p)[0]
    for i in range(n):
        got = engine.place(p.job_class)
        assert got.fused == 3, (i, got.fused)
        np.testing.assert_array_equal(got.assign, want, err_msg=f"placement {i} after the change")
    return want


def tallies_exact(engine, p):
    got = engine.place(p.job_class, want_tally=True)
    a, cap, occ = O.place_c(p)
    np.testing.assert_array_equal(got.assign, a)
    np.testing.assert_array_equal(got.cap, cap)
    np.testing.assert_array_equal(got.occ, occ)


def counters(engine):
    engine.service_stop()
    return engine.service_counters()


def set_taint(engine, p, rows, values):
    rows = np.asarray(rows, dtype=np.uint32)
    values = np.asarray(values, dtype=np.uint32)
    engine.patch_rows(rows, taints=values)
    p.nodes.taints[rows] = values


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("racks", sorted(TILES))
def test_clean_run(svc_engine, monkeypatch, racks, mode):
    """Six placements without a patch, J = all jobs, 1, 0, twice over. Mode 2:
    the dispatcher answers every one of them and rings no evaluate-ring beyond
    the service's first; mode 1: the tiles get them all."""
    p = start(svc_engine, monkeypatch, racks, mode)
    want = O.place_c(p)[0]
    for J in (len(want), 1, 0, len(want), 1, 0):
        got = svc_engine.place(p.job_class[:J])
        assert got.fused == 3
        np.testing.assert_array_equal(got.assign, O.place_c(dataclasses.replace(p, job_class=p.job_class[:J]))[0])
    c = counters(svc_engine)
    assert c["tiles"] == TILES[racks]
    assert c["evals"] == 1, c
    if mode == 2:
        assert c["answered"] >= 6 and c["handed"] == 0, c
    else:
        assert c["answered"] == 0 and c["handed"] >= 6, c
    svc_engine.load(p)
    tallies_exact(svc_engine, p)


CHANGES = ["micro_one_row", "micro_two_tiles", "micro_spread", "inline_300", "descriptor_5000", "after_idle_exit",
           "assume_forget", "reupload", "class_pods"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("change", CHANGES)
def test_rows_change_then_two_clean_placements(svc_engine, monkeypatch, change, mode):
    """Every way the rows (or the class) change, then two placements without
    a patch: the first must not be stale, the second is answered from lines
    republished after the change. Patched rows sit at both ends of a tile,
    beside tiles that keep their standing answer."""
    p = start(svc_engine, monkeypatch, 1000, mode, "svc_xcd=0" if change == "micro_spread" else "")
    N = p.nodes.n_nodes
    exact(svc_engine, p)
    if change in ("micro_one_row", "micro_spread"):
        # the first and the last row of tile 7, and the last row of the last
        # (short) tile: a leaf goes infeasible, then comes back
        for row in (7 * TILE_ROWS, 8 * TILE_ROWS - 1, N - 1):
            for v in (BAD, 0):
                set_taint(svc_engine, p, [row], [v])
                exact(svc_engine, p)
    elif change == "micro_two_tiles":
        # both rows flip their leaves (tiles 3 and 4); then one flips back in
        # tile 3 while tile 9's row is rewritten with its own value
        a, b = 4 * TILE_ROWS - 1, 4 * TILE_ROWS
        set_taint(svc_engine, p, [a, b], [BAD, BAD])
        exact(svc_engine, p)
        set_taint(svc_engine, p, [a, 9 * TILE_ROWS + 7], [0, p.nodes.taints[9 * TILE_ROWS + 7]])
        exact(svc_engine, p)
        set_taint(svc_engine, p, [b], [0])
        exact(svc_engine, p)
    elif change == "inline_300":
        rows = np.arange(2 * TILE_ROWS - 150, 2 * TILE_ROWS + 150)
        set_taint(svc_engine, p, rows, synth.bernoulli(7, 1, rows.size, 0.1).astype(np.uint32))
        exact(svc_engine, p)
    elif change == "descriptor_5000":
        rows = np.sort(synth.permutation(7, 2, N)[:5000])
        set_taint(svc_engine, p, rows, synth.bernoulli(7, 3, rows.size, 0.02).astype(np.uint32))
        exact(svc_engine, p)
    elif change == "after_idle_exit":
        time.sleep(IDLE_S * 1.6)  # the service has left; the patch wakes it, its warm-up evaluates
        set_taint(svc_engine, p, [5 * TILE_ROWS], [BAD])
        want = O.place_c(p)[0]
        for i in range(2):
            np.testing.assert_array_equal(svc_engine.place(p.job_class).assign, want, err_msg=f"placement {i}")
        exact(svc_engine, p)
    elif change == "assume_forget":
        a = O.place_c(p)[0]
        own = (0x40000000 + np.arange(60)).astype(np.int32)
        new, committed, _ = assume_ref(dataclasses.replace(p, job_class=p.job_class[:60]), a[:60], own)
        got, _ = svc_engine.assume(p.job_class[:60], a[:60], own)
        np.testing.assert_array_equal(got, committed)
        p.nodes.excl[:] = new
        assert not np.array_equal(exact(svc_engine, p), a)
        p.nodes.excl[:] = forget_ref(p.nodes.excl, own[::2])[0]
        svc_engine.forget(own[::2])
        exact(svc_engine, p)
    elif change == "reupload":
        p = snapshot(1000, trial=1)
        svc_engine.upload_snapshot(p.nodes)
        warm(svc_engine, p)
        exact(svc_engine, p)
    elif change == "class_pods":
        before = O.place_c(p)[0]
        p.classes = [dataclasses.replace(p.classes[0], pods=PER - 1)]
        svc_engine.upload_classes(p.classes)
        warm(svc_engine, p)
        assert not np.array_equal(exact(svc_engine, p), before)
    tallies_exact(svc_engine, p)


@pytest.mark.parametrize("mode", MODES)
def test_microbox_give_up_leaves_no_standing_line(svc_engine, monkeypatch, mode):
    """micro_spins=0: every microbox wait gives up, the request is reported and
    answered on the launch path; the fresh service's first two placements are
    exact -- nothing comes from a standing line older than the failed request."""
    p = start(svc_engine, monkeypatch, 1000, mode, "micro_spins=0")
    a0 = exact(svc_engine, p)
    for k in range(2):
        r = int(p.nodes.leaf_start[int(a0[3 + 5 * k])])
        svc_engine.metrics(reset=True)
        set_taint(svc_engine, p, [r], [p.nodes.taints[r] | BAD])
        want = O.place_c(p)[0]
        got = svc_engine.place(p.job_class)
        np.testing.assert_array_equal(got.assign, want)
        assert got.fused != 3
        m = svc_engine.metrics()
        assert m.svc_fallbacks == 1 and m.place_errors == 0
        warm(svc_engine, p)
        a0 = exact(svc_engine, p)
    monkeypatch.setenv("JSP_TEST_HOOKS", "")
    svc_engine.load(p)
    tallies_exact(svc_engine, p)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("how", ["timing", "entries"])
def test_timing_on_and_entries_stay_with_the_tiles(svc_engine, monkeypatch, how, mode):
    """With the device stamps on, and with the per-job entries answer
    (svc_entries=1), the tiles answer every request: exact, and the
    dispatcher-answered counter stays 0."""
    if how == "timing":
        svc_engine.set_timing(True)
    p = start(svc_engine, monkeypatch, 560, mode, "svc_entries=1" if how == "entries" else "")
    exact(svc_engine, p, 3)
    set_taint(svc_engine, p, [TILE_ROWS], [BAD])
    exact(svc_engine, p, 3)
    if how == "timing":
        c, _ = svc_engine.service_clock_rows()
        assert c.shape[0] == TILES[560]
        if mode > 0:  # the standing path: tallied = broadcast
            np.testing.assert_array_equal(c[:, 2], c[:, 1])
    c = counters(svc_engine)
    assert c["tiles"] == TILES[560] and c["answered"] == 0, c
    svc_engine.set_timing(False)
    tallies_exact(svc_engine, p)


@pytest.mark.parametrize("mode", MODES)
def test_tiles_outlast_a_run_of_dispatcher_answers(svc_engine, monkeypatch, mode):
    """The noted bell: placements without a patch, back to back for more than
    twice the idle time (the tiles' own exit timer), then a micro-patched one
    and a clean one -- all exact and answered by the service, none on the
    fallback."""
    p = start(svc_engine, monkeypatch, 120, mode)
    want = O.place_c(p)[0]
    svc_engine.metrics(reset=True)
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < 2.5 * IDLE_S:
        got = svc_engine.place(p.job_class)
        assert got.fused == 3
        n += 1
        if n % 64 == 0:
            np.testing.assert_array_equal(got.assign, want)
    set_taint(svc_engine, p, [TILE_ROWS - 1], [BAD])
    exact(svc_engine, p)
    assert svc_engine.metrics().svc_fallbacks == 0
    c = counters(svc_engine)
    if mode == 2:
        assert c["answered"] >= n and c["handed"] == 0, (c, n)
    tallies_exact(svc_engine, p)
