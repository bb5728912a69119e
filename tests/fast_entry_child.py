"""Child process of test_fast_entry_gpu.test_lease_ends_by_the_clock_either_way
(the service's idle limit is read once per process, from the environment the
test gives it). Per snapshot and per fast_clock = 1 / 0: a resident service
that has answered, a request without jobs (it crosses), then
  A  a placement: leased;
     12 ms of sleep -- past a quarter of the 40 ms limit, short of the half;
  B  a placement: it crosses and renews the lease;
     2 ms of sleep;
  C  a placement: leased.
Prints one JSON line: which of A, B, C were answered under the lease, the
requests that crossed behind the warm-up by the host's count, and by the
service's own (its dispatcher's counters, read after it stopped)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jobset_amd import native  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402
from test_service_standing_gpu import snapshot, warm  # noqa: E402


def sequence(e, racks, fast):
    os.environ["JSP_TEST_HOOKS"] = f"fast_clock={fast}"
    probe = np.zeros(3, dtype=np.int64)
    assert native.lib().jspb_fast_clock_probe(1, probe.ctypes.data) == 0
    p = snapshot(racks)
    for attempt in range(3):  # (a sleep that overran towards the half of the limit: once more, from a fresh start)
        e.load(p)  # hooks are read at upload
        e.set_service(True)
        e.set_fused(True)
        warm(e, p)
        e.lease_counters(reset=True)
        leased, crossings, slept = [], 0, []

        def place(J):
            nonlocal crossings
            before = e.lease_counters()["answered"]
            got = e.place(p.job_class[:J])
            assert got.fused == 3, got.fused
            host = e.lease_counters()["answered"] - before == 1
            crossings += 0 if host else 1
            return host

        assert not place(0)  # no lease without jobs: the lease is fresh from here
        for pause in (0.0, 0.012, 0.002):
            t = time.perf_counter()
            if pause:
                time.sleep(pause)
            slept.append(time.perf_counter() - t)
            leased.append(place(p.job_class.size))
        lc = e.lease_counters()
        e.service_stop()
        c = e.service_counters()
        if slept[1] < 0.018:
            break
    return {"tsc": int(probe[2]), "leased": leased, "crossings": crossings, "host_answered": lc["answered"],
            "service_requests": c["answered"] + c["handed"]}


def main():
    res = {}
    with Engine(0) as e:
        for racks in (60, 1000):
            res[str(racks)] = {str(fast): sequence(e, racks, fast) for fast in (1, 0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
