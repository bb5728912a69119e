"""jsp_place_spread beside jsp_place_fit (TIGHTEST) and jsp_place_gangs on the
same snapshot (DESIGN.md §9 "Spread placement"): same process, same engine.
The three calls share the tally and the feasibility launches; spread adds the
fits words, the peer passes and two span-count launches on the device and its
own walk on the host.

Per shape (config2 and config5 as they are; config4 reduced to 2^17 nodes and
6,000 domains) the spread level is the coarsest level that is not finer than
any class of the batch, max_skew 1; 5 % of the leaf-level domains get a peer
from a seeded overlay (a fresh id per domain on all its rows). Gangs: one gang
per run, anywhere (JSP_SPAN_ANY).
  call:   `repeat` C-timed loops of `iters` calls (jspb_place_*_loop: median
          and p99 per call, host wall time, every call ends in the host's wait
          for the device); for spread also the median host walk inside a call;
  tables: the device time of spread's launches behind the tally and the
          feasibility words (jspb_spread_tables: events on the dispatches).
Every loop is warmed by a first, untimed round.

    python tools/spread_probe.py [--iters 200] [--repeat 5] [--table-iters 200]

One JSON line per shape.
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


def overlay(p, seed, share=0.05):
    """(excl with the peers laid over it, peer ids)"""
    n = p.nodes
    ls = np.asarray(n.leaf_start, dtype=np.int64)
    L = ls.shape[0] - 1
    pick = synth.bernoulli(seed, 1, L, share) & (np.diff(ls) > 0)
    leaves = np.nonzero(pick)[0]
    ids = (3000 + np.arange(leaves.shape[0])).astype(np.int32)
    owner_of_leaf = np.full(L, -1, dtype=np.int64)
    owner_of_leaf[leaves] = ids
    per_row = np.repeat(owner_of_leaf, np.diff(ls))
    excl = n.excl.copy()
    excl[per_row >= 0] = per_row[per_row >= 0]
    return excl, ids


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def probe(name, iters, repeat, table_iters):
    p = SHAPES[name]()
    excl, ids = overlay(p, 23)
    p.nodes.excl[:] = excl
    rc, rl = job_runs(p.job_class)
    lvl = min(p.classes[int(c)].level for c in rc)
    gr = np.ones(rc.shape[0], dtype=np.uint32)
    gs = np.full(rc.shape[0], native.JSP_SPAN_ANY, dtype=np.uint32)
    with Engine(0) as e:
        e.load(p)
        a, sp, cnt, st = e.place_spread_runs(rc, rl, lvl, 1, ids)
        e.place_spread_loop(rc, rl, lvl, 1, ids, iters=20)                           # warm
        med, p99, walk = [], [], []
        for _ in range(repeat):
            _, m, q, w = e.place_spread_loop(rc, rl, lvl, 1, ids, iters=iters)
            med.append(m)
            p99.append(q)
            walk.append(w)
        e.spread_tables(lvl, ids, iters=20)
        *_, (t_med, t_mean) = e.spread_tables(lvl, ids, iters=table_iters)
        e.place_fit_loop(rc, rl, native.JSP_FIT_TIGHTEST, iters=20)
        f_med = [e.place_fit_loop(rc, rl, native.JSP_FIT_TIGHTEST, iters=iters)[1] for _ in range(repeat)]
        e.place_gangs_loop(rc, rl, gr, gs, iters=20)
        g_med = [e.place_gangs_loop(rc, rl, gr, gs, iters=iters)[1] for _ in range(repeat)]
        return {"shape": name, "rows": p.nodes.n_nodes, "leaves": p.topology.n_leaves, "jobs": p.n_jobs,
                "classes": len(p.classes), "spread_level": lvl, "spread_domains": int(p.topology.n_domains[lvl]),
                "peers": int(ids.shape[0]), "placed": int(st.placed), "refused": int(st.refused), "skew": int(st.skew),
                "iters": iters, "repeat": repeat,
                "spread_call_us": {"min": min(med), "p50": pct(med, 0.5), "max": max(med)},
                "spread_call_p99_us": pct(p99, 0.5),
                "spread_walk_us": {"min": min(walk), "p50": pct(walk, 0.5), "max": max(walk)},
                "spread_tables_device_us": {"median": t_med, "mean": t_mean},
                "fit_call_us": {"min": min(f_med), "p50": pct(f_med, 0.5), "max": max(f_med)},
                "gangs_call_us": {"min": min(g_med), "p50": pct(g_med, 0.5), "max": max(g_med)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--table-iters", type=int, default=200)
    a = ap.parse_args()
    for name in [x for x in a.shapes.split(",") if x]:
        print(json.dumps(probe(name, a.iters, a.repeat, a.table_iters)), flush=True)


if __name__ == "__main__":
    main()
