"""jsp_bind_pods beside jsp_place on the launch path (DESIGN.md §4 "Pod
binding"): same process, resident service off, assign = the config's own
placement. After 10 warm-up calls, the median of `repeat` C-timed loops of
`iters` calls each (jspb_bind_loop, jspb_place_loop); then, on the device, one
event pair around repeated launches (jspb_bind_kernel_loop): the call's whole
stream work, its bind launches alone, and the tally, which streams the same
columns over every row. Bytes are algorithmic: bound rows x (8 W + 8 + 4 R),
4 bytes per pod written, 24 bytes per job read and 8 written, 8 bytes per
domain of all levels for the claim tables.

    python tools/bind_probe.py [--cfg 2] [--iters 200] [--repeat 5] [--wg] [--nodes N --domains D]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from jobset_amd import synth  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402
from jobset_amd.snapshot import job_runs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=int, default=2, choices=(2, 3, 4, 5))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--wg", action="store_true", help="force the workgroup form (JSP_TEST_HOOKS bind_wg=1)")
    ap.add_argument("--nodes", type=int, default=0, help="cfg4 only: rows (default 1M)")
    ap.add_argument("--domains", type=int, default=0, help="cfg4 only: racks (default 50,000)")
    a = ap.parse_args()
    if a.wg:
        os.environ["JSP_TEST_HOOKS"] = "bind_wg=1"
    if a.cfg == 4 and a.nodes:
        p = synth.config4(n_nodes=a.nodes, n_domains=a.domains or 50_000)
    else:
        p = synth.CONFIGS[a.cfg]()
    rc, rl = job_runs(p.job_class)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        plain = e.place(p.job_class)
        assign = plain.assign.copy()
        rows, off, st = e.bind_pods_runs(rc, rl, assign)
        call = e.host_placer(rc, rl)
        for _ in range(10):
            call()
            e.bind_pods_runs(rc, rl, assign)
        bind_us = [e.bind_loop(rc, rl, assign, a.iters)[0][1] for _ in range(a.repeat)]
        place_us = [call.loop(a.iters)[1] for _ in range(a.repeat)]
        dev = [e.bind_kernel_loop(a.iters) for _ in range(a.repeat)]
    nd, topo = p.nodes, p.topology
    placed = np.nonzero(assign >= 0)[0]
    ls = nd.leaf_start.astype(np.int64)
    span = []
    for j in placed:
        fl = topo.first_leaf[p.classes[int(p.job_class[j])].level]
        span.append(int(ls[int(fl[assign[j] + 1])] - ls[int(fl[assign[j]])]))
    row_bytes = 8 * nd.n_label_words + 8 + 4 * nd.n_res
    n_wave = int(sum(1 for s in span if s <= 252)) if not a.wg else 0   # at any alignment; the engine decides per job
    bind_bytes = sum(span) * row_bytes + 4 * int(st.pods) + 32 * p.n_jobs + 8 * sum(topo.n_domains)
    tally_bytes = nd.n_nodes * row_bytes + 4 * (len(p.classes) + 1) * topo.n_leaves
    all_us, bind_k_us, tally_k_us = (med([d[i] for d in dev]) for i in range(3))
    out = {"cfg": a.cfg, "rows": nd.n_nodes, "jobs": p.n_jobs, "classes": len(p.classes), "iters": a.iters,
           "repeat": a.repeat, "form": "workgroup" if a.wg else "auto", "bound": int(st.bound), "stale": int(st.stale),
           "pods": int(st.pods), "pods_bound": int(st.pods_bound), "rows_used": int(st.rows_used),
           "bound_rows_read": int(sum(span)), "largest_domain_rows": max(span) if span else 0,
           "jobs_at_most_252_rows": n_wave, "place_shape": int(plain.fused),
           "bind_us": bind_us, "place_us": place_us, "bind_us_median": med(bind_us), "place_us_median": med(place_us),
           "stream_ops_per_bind_call": 2 + (1 if 0 < n_wave else 0) + (1 if n_wave < len(span) or a.wg else 0),
           "device_us_call": all_us, "device_us_bind_launches": bind_k_us, "device_us_tally": tally_k_us,
           "bind_over_tally": bind_k_us / tally_k_us if tally_k_us else None,
           "bind_bytes": int(bind_bytes), "tally_bytes": int(tally_bytes),
           "bind_GBps": bind_bytes / bind_k_us / 1e3 if bind_k_us else None,
           "tally_GBps": tally_bytes / tally_k_us / 1e3 if tally_k_us else None,
           "pods_per_second": int(st.pods_bound) / med(bind_us) * 1e6 if bind_us else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
