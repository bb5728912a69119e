"""jsp_place_whatif beside the old way of asking the same question (DESIGN.md
§9 "What-if placement"): same process, same engine, resident service in its
default mode (AUTO).

Per config (3, 5: the multi-class shapes) and S in 1, 8, 64: S scenarios of 16
random rows each, every row given a foreign owner (the excl_owner column
alone).
  what-if: `repeat` C-timed loops of `iters` jsp_place_whatif calls
    (jspb_place_whatif_loop: median and p99 per call);
  old way: per scenario jsp_snapshot_patch, jsp_place, jsp_snapshot_patch
    back, `trials` times; each triple by the host clock around the three
    ctypes calls (no C-timed loop covers a 16-row patch; an empty ctypes call
    is timed beside it and reported as `ctypes_call_us`);
  after each: the wall time of the first ordinary jsp_place (jsp_stats.wall_us)
    and the shape that answered it.
Both ways' answers are compared before anything is timed.

    python tools/whatif_probe.py [--configs 3,5] [--iters 100] [--repeat 5] [--trials 30]

One JSON line per config and S.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from jobset_amd import synth  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402
from jobset_amd.snapshot import job_runs  # noqa: E402

ROWS = 16


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def spread(v):
    return {"p10": pct(v, 0.1), "p50": pct(v, 0.5), "p90": pct(v, 0.9)}


def probe(cfg, S, iters, repeat, trials):
    p = synth.CONFIGS[cfg]()
    rc, rl = job_runs(p.job_class)
    N = p.nodes.n_nodes
    rows = [np.sort(synth.permutation(1000 * cfg + s, 1, N)[:ROWS]).astype(np.uint32) for s in range(S)]
    so = (np.arange(S + 1) * ROWS).astype(np.uint32)
    allrows = np.concatenate(rows)
    own = np.full(S * ROWS, 77, dtype=np.int32)
    with Engine(0) as e:
        e.load(p)
        call = e.host_placer(rc, rl)
        for _ in range(5):
            call()
        got, placed, st = e.place_whatif_runs(rc, rl, so, allrows, excl_owner=own)

        def old_way(s):
            r = rows[s]
            e.patch_rows(r, excl=own[:ROWS])
            call()
            a = call.assign.copy()
            e.patch_rows(r, excl=p.nodes.excl[r])
            return a

        for s in range(S):
            assert np.array_equal(old_way(s), got[s]), (cfg, s)
        # what-if, then the first ordinary placement
        wi_med, wi_p99, after_wi, shape_wi = [], [], [], []
        for _ in range(repeat):
            _, m, q = e.place_whatif_loop(rc, rl, so, allrows, excl_owner=own, iters=iters)
            wi_med.append(m)
            wi_p99.append(q)
        for _ in range(trials):
            call()
            call()
            e.place_whatif_runs(rc, rl, so, allrows, excl_owner=own)
            r = call()
            after_wi.append(float(r.wall_us))
            shape_wi.append(int(r.fused))
        # the old way, then the first ordinary placement
        old_call, after_old, shape_old = [], [], []
        for _ in range(trials):
            call()
            call()
            t0 = time.perf_counter()
            for s in range(S):
                old_way(s)
            old_call.append((time.perf_counter() - t0) * 1e6)
            r = call()
            after_old.append(float(r.wall_us))
            shape_old.append(int(r.fused))
        t0 = time.perf_counter()
        for _ in range(1000):
            e._lib.jsp_abi_version()
        ctypes_us = (time.perf_counter() - t0) * 1e3
        return {"config": cfg, "rows": N, "jobs": p.n_jobs, "classes": len(p.classes), "scenarios": S,
                "rows_per_scenario": ROWS, "flips": int(st.flips), "iters": iters, "repeat": repeat, "trials": trials,
                "whatif_call_us": spread(wi_med), "whatif_call_p99_us": pct(wi_p99, 0.5),
                "whatif_per_scenario_us": pct(wi_med, 0.5) / S,
                "old_call_us": spread(old_call), "old_per_scenario_us": pct(old_call, 0.5) / S,
                "ctypes_call_us": ctypes_us,
                "place_after_whatif_us": spread(after_wi), "place_after_whatif_shapes": sorted(set(shape_wi)),
                "place_after_old_us": spread(after_old), "place_after_old_shapes": sorted(set(shape_old))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--scenarios", default="1,8,64")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--trials", type=int, default=30)
    a = ap.parse_args()
    for cfg in [int(x) for x in a.configs.split(",") if x]:
        for S in [int(x) for x in a.scenarios.split(",") if x]:
            print(json.dumps(probe(cfg, S, a.iters, a.repeat, a.trials)), flush=True)


if __name__ == "__main__":
    main()
