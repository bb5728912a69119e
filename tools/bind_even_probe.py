"""jsp_bind_pods_even beside jsp_bind_pods on the same snapshot and assignment
(DESIGN.md §9 "Even pod binding"), one process, resident service off, the two
calls alternating: per round `iters` calls of each in turn, a call's time its
own wall_us (a host clock around the call, which ends in a stream
synchronise); the median of each round, then min / p50 / max over the rounds.

Shapes: cfg2 and cfg5 as they are (one pod per row: both rules give the same
rows), and cfg5 with zone 1 made whole and every row's free resources raised
to a seeded 4..32 times a pod's request, so the rules differ and a zone job
(2,048 rows: two chunks) is bound.

One JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jobset_amd import synth  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402


def cfg5_caps():
    p = synth.config5()
    r0, r1 = 2048, 4096
    p.nodes.taints[r0:r1] = 0
    p.nodes.excl[r0:r1] = -1
    p.nodes.labels[0, r0:r1] |= np.uint64(1)
    k = np.random.default_rng(5).integers(4, 33, p.nodes.n_nodes).astype(np.uint32)
    p.nodes.free[:] = np.array(p.classes[0].res()[:p.nodes.n_res], dtype=np.uint32)[:, None] * k[None, :]
    return p


SHAPES = {"cfg2": synth.config2, "cfg5": synth.config5, "cfg5_caps": cfg5_caps}


def spread(v):
    v = sorted(v)
    return {"min": v[0], "p50": v[len(v) // 2], "max": v[-1]}


def most_per_row(rows):
    return int(np.bincount(rows[rows >= 0]).max()) if (rows >= 0).any() else 0


def probe(name, iters, repeat):
    p = SHAPES[name]()
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        assign = e.place(p.job_class).assign.copy()
        first, _, fs = e.bind_pods(p.job_class, assign)
        even, _, level, es = e.bind_pods_even(p.job_class, assign)
        fm, em = [], []
        for r in range(repeat + 1):  # round 0 warms both up
            f, v = [], []
            for _ in range(iters):
                f.append(e.bind_pods(p.job_class, assign)[2].wall_us)
                v.append(e.bind_pods_even(p.job_class, assign)[3].wall_us)
            if r > 0:
                fm.append(float(np.median(f)))
                em.append(float(np.median(v)))
    return {"shape": name, "rows": p.nodes.n_nodes, "jobs": p.n_jobs, "bound": int(es.bound), "pods_bound": int(es.pods_bound),
            "pods_on_other_rows": int((first != even).sum()), "first_fit_max_per_row": most_per_row(first),
            "even_max_per_row": int(es.max_per_row), "first_fit_rows_used": int(fs.rows_used),
            "even_rows_used": int(es.rows_used), "max_level": int(level.max()), "iters": iters, "repeat": repeat,
            "bind_call_us": spread(fm), "even_call_us": spread(em)}


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
