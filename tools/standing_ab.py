"""Standing answers of the compaction service, interleaved A/B in one process
(diagnostic): test hook svc_standing = 0 (every request evaluates), 1 (the
resident tiles answer from their last evaluation), 2 (the dispatcher answers
from the tiles' standing lines), 3 (and the host from the last answer's lines
while nothing changed: the lease, the default). Host-API calls timed in C
(jspb_place_loop); the host's phase clocks from jsp_timing (entry -> post,
post -> first / last answer line; under the lease: entry -> the lines, their
expansion); the service's and the lease's counters say which path answered.
Usage: standing_ab.py [alternations] [calls per run] [modes, e.g. 2,3]"""
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
modes = [int(m) for m in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0, 1, 2, 3]
e = Engine(0)
floor = e.link_floor(2000)[0]
print(f"host-link floor p50 {floor:.2f} us", flush=True)
for cfg in (2, 1):
    p = synth.CONFIGS[cfg]()
    ref = O.place_c(p)[0]
    res = {m: [] for m in modes}
    for r in range(reps):
        for mode in modes:
            os.environ["JSP_TEST_HOOKS"] = f"svc_standing={mode}"
            e.load(p)  # hooks are read at upload
            call = e.host_placer(*job_runs(p.job_class))
            for _ in range(200):
                call()
            e.timing(reset=True)
            e.lease_counters(reset=True)
            tot, p50, p99 = call.loop(iters)
            t = e.timing(reset=True)
            lc = e.lease_counters()
            assert np.array_equal(call.assign, ref), mode
            n = max(int(t.svc_calls), 1)
            e.service_stop()
            c = e.service_counters()
            res[mode].append((p50, p99, t.svc_first_us / n, t.svc_answer_us / n, tot / iters,
                              c["answered"], c["handed"], c["evals"], lc["answered"], t.host_prep_us / n,
                              t.host_wait_us / n, t.svc_pre_us / n))
    os.environ.pop("JSP_TEST_HOOKS", None)
    for mode, v in res.items():
        a = np.array(v)
        print(f"cfg{cfg} svc_standing={mode}: per call p50 {np.median(a[:, 0]):.3f} us p99 {np.median(a[:, 1]):.3f} mean "
              f"{np.median(a[:, 4]):.3f} | post->first {np.median(a[:, 2]):.3f} ->last {np.median(a[:, 3]):.3f} "
              f"(beyond the floor {np.median(a[:, 3]) - floor:.3f}) | p50 runs: {' '.join(f'{x:.3f}' for x in a[:, 0])} "
              f"spread {a[:, 0].max() - a[:, 0].min():.3f} | answered/handed/evals {int(a[-1, 5])}/{int(a[-1, 6])}/"
              f"{int(a[-1, 7])} host-answered {int(a[-1, 8])} | phases: prep {np.median(a[:, 9]):.3f} wait "
              f"{np.median(a[:, 10]):.3f} (pre {np.median(a[:, 11]):.3f} answer {np.median(a[:, 3]):.3f})", flush=True)
e.close()
