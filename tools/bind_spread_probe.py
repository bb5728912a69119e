"""jsp_bind_pods_spread beside jsp_bind_pods and jsp_bind_pods_even on the same
snapshot and assignment (DESIGN.md §9 "Spread pod binding"), one process,
resident service off, the three calls alternating: per round `iters` calls of
each in turn, a call's time its own wall_us (a host clock around the call,
which ends in a stream synchronise); the median of each round, then min / p50
/ max over the rounds.

Shapes: tools/bind_even_probe.py's. The spread level is one below the coarsest
class level where the topology has one (cfg5: racks inside zones), else that
level (cfg2: one group per job).

One JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bind_even_probe import SHAPES, spread  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402


def most_per_group(p, s, rows):
    """The fullest level-s domain's pods (the jobs' domains are disjoint: a group serves one job)."""
    edges = p.nodes.leaf_start[p.topology.first_leaf[s]].astype(np.int64)
    rows = rows[rows >= 0].astype(np.int64)
    return int(np.bincount(np.searchsorted(edges, rows, side="right") - 1).max()) if rows.size else 0


def probe(name, iters, repeat):
    p = SHAPES[name]()
    s = min(min(c.level for c in p.classes) + 1, p.topology.n_levels - 1)
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        assign = e.place(p.job_class).assign.copy()
        first = e.bind_pods(p.job_class, assign)[0]
        even = e.bind_pods_even(p.job_class, assign)[0]
        rows, _, level, ss = e.bind_pods_spread(p.job_class, assign, s)
        fm, em, sm = [], [], []
        for r in range(repeat + 1):  # round 0 warms all three up
            f, v, w = [], [], []
            for _ in range(iters):
                f.append(e.bind_pods(p.job_class, assign)[2].wall_us)
                v.append(e.bind_pods_even(p.job_class, assign)[3].wall_us)
                w.append(e.bind_pods_spread(p.job_class, assign, s)[3].wall_us)
            if r > 0:
                fm.append(float(np.median(f)))
                em.append(float(np.median(v)))
                sm.append(float(np.median(w)))
    return {"shape": name, "rows": p.nodes.n_nodes, "jobs": p.n_jobs, "spread_level": s, "bound": int(ss.bound),
            "pods_bound": int(ss.pods_bound), "pods_on_other_rows": int((first != rows).sum()),
            "first_fit_max_per_group": most_per_group(p, s, first), "even_max_per_group": most_per_group(p, s, even),
            "spread_max_per_group": int(ss.max_per_group), "groups_used": int(ss.groups_used),
            "max_level": int(level.max()), "iters": iters, "repeat": repeat, "bind_call_us": spread(fm),
            "even_call_us": spread(em), "spread_call_us": spread(sm)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    for name in [x for x in a.shapes.split(",") if x]:
        print(json.dumps(probe(name, a.iters, a.repeat)), flush=True)


if __name__ == "__main__":
    main()
