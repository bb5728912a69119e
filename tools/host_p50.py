#!/usr/bin/env python3
"""Host-API p50 of jsp_place on one config (diagnostic): REPS C-timed loops of
ITERS calls (jspb_place_loop) behind 50 warm-up calls, each with the path the
calls took (the timing's host / service / one-shot counts). JSP_TEST_HOOKS and
JSP_LIB_PATH as set by the caller: an A/B runs it once per library and hook.
Usage: host_p50.py CFG [REPS] [ITERS]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch  # noqa: F401
    from jobset_amd import synth
    from jobset_amd.engine import Engine
    from jobset_amd.snapshot import job_runs
    cfg = int(sys.argv[1])
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    eng = Engine(0)
    p = synth.CONFIGS[cfg]()
    eng.load(p)
    rc, rl = job_runs(p.job_class)
    call = eng.host_placer(rc, rl)
    for _ in range(50):
        call()
    for rep in range(reps):
        _, med, p99 = call.loop(iters)
        tm = eng.timing(reset=True)
        print(f"cfg{cfg} hooks={os.environ.get('JSP_TEST_HOOKS', '')} lib={os.environ.get('JSP_LIB_PATH', '') or 'tree'} "
              f"rep{rep}: host API p50 {med:.3f} us p99 {p99:.2f} placed {int(call.stats.placed)} "
              f"shape {int(call.stats.fused)} calls {int(tm.calls)} host {int(tm.host_calls)} svc {int(tm.svc_calls)} "
              f"oneshot {int(tm.oneshot_calls)}", flush=True)
    eng.service_stop()
    eng.close()


if __name__ == "__main__":
    main()
