"""jsp_place_gangs beside jsp_place on the launch path (DESIGN.md §4 "Gang
placement"): same process, same runs, resident service off. The batch is
config5's 496 rack JobSets regrouped into 124 gangs of 4, each inside one zone
(span level 0). After 10 warm-up calls of each, `repeat` rounds that alternate
a C-timed loop of `iters` jsp_place_gangs calls (jspb_place_gangs_loop) with one
of jsp_place (jspb_place_loop): the same tally and feasibility, then the plain
host walk. The span-count launches' own device time comes from events on
their dispatches (jspb_span_counts). One JSON line.

    python tools/gang_probe.py [--iters 200] [--repeat 7]
"""
import argparse
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from jobset_amd import synth  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=7)
    a = ap.parse_args()
    p = synth.config5()
    rack = np.array([p.classes[int(c)].level == 1 for c in p.job_class])
    p = dataclasses.replace(p, job_class=np.ascontiguousarray(p.job_class[rack]), job_names=None)
    J = p.n_jobs
    # runs never cross a gang: one run per stretch of one class inside a gang of 4
    gang = np.arange(J) // 4
    cut = np.nonzero((np.diff(p.job_class.astype(np.int64)) != 0) | (np.diff(gang) != 0))[0] + 1
    start = np.concatenate([[0], cut])
    rc = p.job_class[start]
    rl = np.diff(np.concatenate([start, [J]])).astype(np.uint32)
    gr = np.bincount(gang[start]).astype(np.uint32)
    gs = np.zeros(gr.shape[0], dtype=np.uint32)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        got, span, st = e.place_gangs_runs(rc, rl, gr, gs)
        call = e.host_placer(rc, rl)
        plain = call()
        for _ in range(10):
            call()
            e.place_gangs_runs(rc, rl, gr, gs)
        gang_us, place_us = [], []
        for _ in range(a.repeat):
            gang_us.append(e.place_gangs_loop(rc, rl, gr, gs, a.iters)[1])
            place_us.append(call.loop(a.iters)[1])
        n_cnt = sum(sum(p.topology.n_domains[:c.level + 1]) for c in p.classes)
        e.span_counts(n_cnt, iters=50)
        counts_us = [e.span_counts(n_cnt, iters=a.iters)[1][0] for _ in range(a.repeat)]
    out = {"rows": p.nodes.n_nodes, "jobs": J, "runs": int(rc.shape[0]), "gangs": int(gr.shape[0]),
           "classes": len(p.classes), "iters": a.iters, "repeat": a.repeat,
           "gangs_placed": int(st.gangs_placed), "placed": int(st.placed), "plain_placed": int(plain.placed),
           "gang_shape": int(st.fused), "place_shape": int(plain.fused),
           "gang_us": gang_us, "place_us": place_us, "gang_us_median": med(gang_us), "place_us_median": med(place_us),
           "difference_us": med(gang_us) - med(place_us), "span_counts": n_cnt, "span_counts_device_us": counts_us,
           "span_counts_device_us_median": med(counts_us)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
