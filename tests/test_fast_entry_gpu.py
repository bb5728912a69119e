"""The leased jsp_place's entry ("the entry stamps"): its two
stamps read off the TSC, its metrics recorded under the engine's lock into a
single-writer accumulator that jsp_engine_get_metrics adds up under the
metrics' lock alone. Checked here: the metrics are exact across crossing and
leased calls, across a reset under a held lease and beside placing threads;
the lease ends by the clock with either clock; a leased call's wall is sane;
and the answers are the oracle's.

The snapshots, helpers and the pacing are the lease tests' (60 racks: one
tile, cfg1-sized; 1000 racks: cfg2's 15 tiles), J = 1 and J = all."""
import dataclasses
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from test_service_standing_gpu import BAD, set_taint
from test_service_lease_gpu import renew, start

pytestmark = pytest.mark.gpu

RACKS = [60, 1000]


@pytest.fixture
def svc_engine(engine):
    engine.set_service(True)
    engine.set_fused(True)
    yield engine
    engine.set_timing(False)
    engine.service_stop()


def n_jobs(p, which):
    return 1 if which == "one" else p.job_class.size


def place(engine, J):
    """One placement of J jobs of the one class: (result, answered under the lease)."""
    before = engine.lease_counters()["answered"]
    got = engine.place(np.zeros(J, dtype=np.uint32))
    return got, engine.lease_counters()["answered"] - before == 1


def buckets(h):
    return sum(int(x) for x in h.bucket)


@pytest.mark.parametrize("which", ["one", "all"])
@pytest.mark.parametrize("racks", RACKS)
def test_metrics_exact(svc_engine, monkeypatch, racks, which):
    """Four rounds of: a one-row patch (the lease ends), a crossing call, two
    leased calls. The metrics hold every call once, whichever path recorded
    it."""
    p = start(svc_engine, monkeypatch, racks)
    J = n_jobs(p, which)
    renew(svc_engine, p)
    svc_engine.metrics(reset=True)
    calls, leased = [], []
    for i in range(4):
        set_taint(svc_engine, p, [7], [BAD if i % 2 == 0 else 0])
        for k in range(3):
            got, host = place(svc_engine, J)
            assert got.fused == 3
            assert host == (k > 0), (i, k, "leased" if host else "crossed")
            calls.append(got)
            leased.append(host)
    M, N = leased.count(False), leased.count(True)
    assert M == 4 and N == 8
    m = svc_engine.metrics()
    assert m.place_us.count == m.batch_jobs.count == M + N
    assert m.placed == sum(c.placed for c in calls)
    assert m.unplaceable == sum(c.jobs - c.placed for c in calls)
    assert m.svc_calls == M + N  # every one answered by the service (fused 3), as before
    assert m.place_errors == 0
    assert buckets(m.place_us) == m.place_us.count and buckets(m.batch_jobs) == m.batch_jobs.count
    walls = [c.wall_us for c in calls]
    assert m.place_us.sum == pytest.approx(sum(walls), rel=1e-6)
    assert m.place_us.max == max(walls)
    assert m.batch_jobs.sum == J * (M + N) and m.batch_jobs.max == J


@pytest.mark.parametrize("which", ["one", "all"])
@pytest.mark.parametrize("racks", RACKS)
def test_reset_under_a_held_lease(svc_engine, monkeypatch, racks, which):
    """A reset between leased calls: the next read holds exactly the calls
    behind it, and no maximum from before it."""
    p = start(svc_engine, monkeypatch, racks)
    J = n_jobs(p, which)
    renew(svc_engine, p)
    for _ in range(5):
        got, host = place(svc_engine, J)
        assert host
    before = svc_engine.metrics(reset=True)
    assert before.place_us.count == 6  # (renew's crossing and the five)
    walls = []
    K = 7
    for _ in range(K):
        got, host = place(svc_engine, J)
        assert host
        walls.append(got.wall_us)
    m = svc_engine.metrics()
    assert m.place_us.count == m.batch_jobs.count == m.svc_calls == K
    assert m.placed + m.unplaceable == K * J
    assert buckets(m.place_us) == K and buckets(m.batch_jobs) == K
    assert 0 < m.place_us.max <= max(walls)
    assert m.place_us.sum == pytest.approx(sum(walls), rel=1e-6)
    assert svc_engine.metrics().place_us.count == K  # a read without reset changes nothing


def test_concurrent_scrape(svc_engine, monkeypatch):
    """Four placing threads (one of them patching a row before each call, so
    that calls cross the link with the engine's lock held; the service is
    stopped first, so the first crossing is a cold start) and a scrape loop
    timed in C for 0.5 s: the scraped count never falls, no scrape waits for a
    placement, and the totals are exact at the end."""
    p = start(svc_engine, monkeypatch, 1000)
    n_all = p.job_class.size
    svc_engine.service_stop()
    svc_engine.metrics(reset=True)
    stop = threading.Event()
    made = [0, 0, 0, 0]
    placed = [0, 0, 0, 0]
    errors = []

    def placer(k):
        try:
            J = (1, n_all, n_all, 17)[k]
            call = svc_engine.host_placer(*job_runs(np.zeros(J, dtype=np.uint32)))
            patch = svc_engine.host_patcher(np.array([7], dtype=np.uint32), taints=np.array([0], dtype=np.uint32))
            while not stop.is_set():
                if k == 0:
                    patch()
                st = call()
                made[k] += 1
                placed[k] += int(st.placed)
        except Exception as ex:  # noqa: BLE001
            errors.append(repr(ex))

    threads = [threading.Thread(target=placer, args=(k,), daemon=True) for k in range(4)]
    for t in threads:
        t.start()
    out = np.zeros(4, dtype=np.uint64)
    rc = svc_engine._lib.jspb_scrape_loop(svc_engine._h, 0.5, out.ctypes.data)
    stop.set()
    for t in threads:
        t.join(30.0)
        assert not t.is_alive()
    assert rc == 0 and not errors, errors
    scrapes, worst_ns, fell, _ = (int(x) for x in out)
    m = svc_engine.metrics()
    print(f"{scrapes} scrapes beside {sum(made)} placements, the longest {worst_ns / 1e3:.1f} us")
    assert scrapes > 100 and min(made) > 0
    assert fell == 0
    assert worst_ns <= 1_000_000
    assert m.place_us.count == m.batch_jobs.count == sum(made)
    assert m.placed == sum(placed)
    assert buckets(m.place_us) == m.place_us.count


def test_lease_ends_by_the_clock_either_way():
    """JSP_SERVICE_IDLE_MS=40 (read once per process: a child), with
    fast_clock=1 and fast_clock=0: a leased call, 12 ms of sleep (past the
    quarter, short of the half), a call that must cross, 2 ms, a call that
    must be leased. The same counters either way."""
    env = dict(os.environ, JSP_SERVICE_IDLE_MS="40")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "fast_entry_child.py")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    for racks in ("60", "1000"):
        fast, steady = res[racks]["1"], res[racks]["0"]
        assert fast["tsc"] in (0, 1) and steady["tsc"] == 0
        for got in (fast, steady):
            assert got["leased"] == [True, False, True], got
            # behind the warm-up the service saw the request without jobs and the one behind the sleep
            assert got["service_requests"] == got["crossings"] == 2 and got["host_answered"] == 2, got
        assert {k: v for k, v in fast.items() if k != "tsc"} == {k: v for k, v in steady.items() if k != "tsc"}


@pytest.mark.parametrize("racks", RACKS)
def test_wall_is_sane(svc_engine, monkeypatch, racks):
    """A leased call's wall is positive and far below 50 us, and the mean wall
    of a loop's calls (from the metrics: the loop passes no stats) is no more
    than the loop's own total per call plus its p99."""
    p = start(svc_engine, monkeypatch, racks)
    call = svc_engine.host_placer(*job_runs(p.job_class))
    for attempt in range(3):  # (a slow box: the loop must fit a quarter of the idle limit)
        renew(svc_engine, p)
        for _ in range(3):
            st = call()
            assert 0 < st.wall_us < 50, st.wall_us
        lc0 = svc_engine.lease_counters()["answered"]
        svc_engine.metrics(reset=True)
        tot, p50, p99 = call.loop(2000)
        m = svc_engine.metrics()
        if svc_engine.lease_counters()["answered"] - lc0 == 2000:
            break
    assert svc_engine.lease_counters()["answered"] - lc0 == 2000
    assert m.place_us.count == 2000
    mean_wall = m.place_us.sum / 2000
    print(f"{racks} racks: wall per leased call {mean_wall:.4f} us; loop {tot / 2000:.4f} us per call, p50 {p50:.3f}, "
          f"p99 {p99:.3f}")
    assert 0 < mean_wall <= tot / 2000 + p99


@pytest.mark.parametrize("which", ["one", "all"])
@pytest.mark.parametrize("racks", RACKS)
def test_answers_unchanged(svc_engine, monkeypatch, racks, which):
    """The oracle's assign[] when a lease is taken, and after a one-row patch
    for the crossing and the two leased answers behind it."""
    p = start(svc_engine, monkeypatch, racks)
    J = n_jobs(p, which)
    oracle = lambda: O.place_c(dataclasses.replace(p, job_class=np.zeros(J, dtype=np.uint32)))[0]  # noqa: E731
    want = oracle()
    row = int(p.nodes.leaf_start[int(want[0])])
    renew(svc_engine, p)
    got, host = place(svc_engine, J)
    assert host
    np.testing.assert_array_equal(got.assign, want)
    set_taint(svc_engine, p, [row], [BAD])
    want2 = oracle()  # (the call behind a patch crosses whenever it comes)
    assert want2[0] != want[0]
    for k in range(3):
        got, host = place(svc_engine, J)
        assert host == (k > 0), k
        np.testing.assert_array_equal(got.assign, want2, err_msg=f"call {k} after the patch")
