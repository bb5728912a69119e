"""jsp_place_preempt beside jsp_place_fit (TIGHTEST) on the same snapshot
(DESIGN.md §9 "Preemptive placement"): same process, same engine. Fit is the
same pipeline minus the row pass, the leaf pass, the second tally and the
gather.

Per shape (config2 and config5 as they are; config4 reduced to 2^17 nodes and
6,000 domains) 30 % of the leaf-level domains get an owner from a seeded
overlay: a fresh id per domain on all its rows, a rank uniform in 0..3, 15 %
of the owners left out of the table; evict_free = max(free, 3/4 of the
column's maximum); prio = 4. With and without evict_free:
  call:  `repeat` C-timed loops of `iters` jsp_place_preempt calls
         (jspb_place_preempt_loop: median and p99 per call, host wall time,
         every call ends in the host's wait for the device);
  order: the device time of the launches behind the staging copy
         (jspb_preempt_order: events on the dispatches, median and mean);
  fit:   the same for jspb_place_fit_loop and jspb_fit_order under TIGHTEST.
Every loop is warmed by a first, untimed round.

    python tools/preempt_probe.py [--iters 200] [--repeat 5] [--order-iters 200]

One JSON line per shape and evict_free setting.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from jobset_amd import native, synth  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402
from jobset_amd.snapshot import job_runs  # noqa: E402

SHAPES = {
    "config2": lambda: synth.config2(),
    "config5": lambda: synth.config5(),
    "config4-reduced": lambda: synth.config4(n_nodes=1 << 17, n_domains=6000),
}


def overlay(p, seed, share=0.3, ranks=4, absent=0.15):
    """(excl with the owners laid over it, owners, owner_prio, evict_free)"""
    n = p.nodes
    ls = np.asarray(n.leaf_start, dtype=np.int64)
    L = ls.shape[0] - 1
    pick = synth.bernoulli(seed, 1, L, share) & (np.diff(ls) > 0)
    leaves = np.nonzero(pick)[0]
    ids = (3000 + np.arange(leaves.shape[0])).astype(np.int32)
    excl = n.excl.copy()
    owner_of_leaf = np.full(L, -1, dtype=np.int64)
    owner_of_leaf[leaves] = ids
    per_row = np.repeat(owner_of_leaf, np.diff(ls))
    excl[per_row >= 0] = per_row[per_row >= 0]
    rank = synth.uniform_int(seed, 2, ids.shape[0], 0, ranks - 1).astype(np.uint32)
    keep = ~synth.bernoulli(seed, 3, ids.shape[0], absent)
    top = n.free.max(axis=1, keepdims=True).astype(np.int64)
    ef = np.maximum(n.free.astype(np.int64), top * 3 // 4).astype(np.uint32)
    return excl, ids[keep], rank[keep], ef


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def probe(name, iters, repeat, order_iters):
    p = SHAPES[name]()
    excl, ids, rk, ef = overlay(p, 17)
    p.nodes.excl[:] = excl
    rc, rl = job_runs(p.job_class)
    out = []
    with Engine(0) as e:
        e.load(p)
        for evict in (False, True):
            col = ef if evict else None
            a, off, v, st = e.place_preempt_runs(rc, rl, 4, ids, rk, col)
            e.place_preempt_loop(rc, rl, 4, ids, rk, col, iters=20)                      # warm
            med, p99 = [], []
            for _ in range(repeat):
                _, m, q = e.place_preempt_loop(rc, rl, 4, ids, rk, col, iters=iters)
                med.append(m)
                p99.append(q)
            e.preempt_order(4, ids, rk, col, iters=20)
            *_, (o_med, o_mean) = e.preempt_order(4, ids, rk, col, iters=order_iters)
            e.place_fit_loop(rc, rl, native.JSP_FIT_TIGHTEST, iters=20)
            f_med = [e.place_fit_loop(rc, rl, native.JSP_FIT_TIGHTEST, iters=iters)[1] for _ in range(repeat)]
            e.fit_order(native.JSP_FIT_TIGHTEST, iters=20)
            _, _, (fo_med, fo_mean) = e.fit_order(native.JSP_FIT_TIGHTEST, iters=order_iters)
            _, fst = e.place_fit_runs(rc, rl, native.JSP_FIT_TIGHTEST)
            out.append({"shape": name, "rows": p.nodes.n_nodes, "leaves": p.topology.n_leaves, "jobs": p.n_jobs,
                        "classes": len(p.classes), "owners_in_table": int(ids.shape[0]), "evict_free": evict,
                        "placed": int(st.placed), "preempting": int(st.preempting), "victims": int(st.victims),
                        "fit_placed": int(fst.placed), "iters": iters, "repeat": repeat,
                        "preempt_call_us": {"min": min(med), "p50": pct(med, 0.5), "max": max(med)},
                        "preempt_call_p99_us": pct(p99, 0.5),
                        "preempt_order_device_us": {"median": o_med, "mean": o_mean},
                        "fit_call_us": {"min": min(f_med), "p50": pct(f_med, 0.5), "max": max(f_med)},
                        "fit_order_device_us": {"median": fo_med, "mean": fo_mean}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--order-iters", type=int, default=200)
    a = ap.parse_args()
    for name in [x for x in a.shapes.split(",") if x]:
        for rec in probe(name, a.iters, a.repeat, a.order_iters):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
