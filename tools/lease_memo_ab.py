"""The lease's kept list, interleaved A/B in one process (diagnostic): test
hook lease_memo = 0 (every host answer under the lease expands the lines) and
1 (from the second host answer on, the answer is copied from the list the
lines expand to: the default). Host-API calls timed in C (jspb_place_loop);
the lease's and the list's counters say which path answered; host_wait_us per
call is the leased call's wall inside the library (jsp_timing).
Usage: lease_memo_ab.py [alternations] [calls per run]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401
from jobset_amd import synth  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402
from jobset_amd.snapshot import job_runs  # noqa: E402
from oracle import oracle as O  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
e = Engine(0)
for cfg in (2, 1):
    p = synth.CONFIGS[cfg]()
    ref = O.place_c(p)[0]
    res = {0: [], 1: []}
    for r in range(reps):
        for memo in (0, 1):
            os.environ["JSP_TEST_HOOKS"] = f"lease_memo={memo}"
            e.load(p)  # hooks are read at upload
            call = e.host_placer(*job_runs(p.job_class))
            for _ in range(200):
                call()
            e.timing(reset=True)
            e.lease_counters(reset=True)
            e.lease_memo_counters(reset=True)
            tot, p50, p99 = call.loop(iters)
            t = e.timing(reset=True)
            lc, mc = e.lease_counters(), e.lease_memo_counters()
            assert np.array_equal(call.assign, ref), memo
            n = max(int(t.host_calls), 1)
            e.service_stop()
            res[memo].append((p50, p99, tot / iters, lc["answered"], lc["taken"], mc["answered"], mc["built"],
                              t.host_prep_us / n, t.host_wait_us / n))
    os.environ.pop("JSP_TEST_HOOKS", None)
    for memo, v in res.items():
        a = np.array(v)
        print(f"cfg{cfg} lease_memo={memo}: per call p50 {np.median(a[:, 0]):.3f} us p99 {np.median(a[:, 1]):.3f} mean "
              f"{np.median(a[:, 2]):.3f} | p50 runs: {' '.join(f'{x:.3f}' for x in a[:, 0])} spread "
              f"{a[:, 0].max() - a[:, 0].min():.3f} | mean runs: {' '.join(f'{x:.3f}' for x in a[:, 2])} | "
              f"host-answered {int(a[-1, 3])} leases {int(a[-1, 4])} from a list {int(a[-1, 5])} lists built "
              f"{int(a[-1, 6])} | phases per call: prep {np.median(a[:, 7]):.3f} wait {np.median(a[:, 8]):.3f}",
              flush=True)
e.close()
