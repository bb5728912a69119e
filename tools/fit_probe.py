"""jsp_place_fit beside jsp_place on the launch path (DESIGN.md §4 "Fit
placement"): same process, same runs, resident service off, so jsp_place runs
the same tally and feasibility and then the plain host walk (shape 7), and the
difference is the order step, its copy and the list walk.

Per config (2, 5, 4) and policy: placed jobs and slack beside jsp_place's
placed count; `repeat` rounds that alternate a C-timed loop of `iters`
jsp_place_fit calls (jspb_place_fit_loop: median and p99) with one of jsp_place
(jspb_place_loop); the order launches' own device time per form, from events
on their dispatches (jspb_fit_order); and the time numpy's sort takes on the
host for the same u64 keys (np.sort per class segment, labelled as such: it is
a sort alone, without the key build and without the copy of the tally to the
host that a host order step would need).

--sizes: the two order forms on config4's generator cut to D domains of 20
nodes (4 classes at one level), for the crossover behind kFitRankMax.

    python tools/fit_probe.py [--configs 2,5,4] [--sizes 256,1024,4096,16384,50000] [--iters 100] [--repeat 5]

One JSON line per config and per size.
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

POLICIES = {"lowest": 0, "tightest": 1, "roomiest": 2}
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731


def host_keys(p, cap, occ, policy):
    """The order step's u64 keys per class, from the engine's own tallies."""
    occ_cs = np.concatenate([[0], np.cumsum(occ.astype(np.int64))])
    out = []
    for c, jc in enumerate(p.classes):
        fl = np.asarray(p.topology.first_leaf[jc.level], dtype=np.int64)
        cs = np.concatenate([[0], np.cumsum(cap[c].astype(np.int64))])
        capsum = cs[fl[1:]] - cs[fl[:-1]]
        ok = (capsum >= jc.pods) & ((occ_cs[fl[1:]] - occ_cs[fl[:-1]]) == 0)
        fit = np.minimum(capsum, 0xFFFFFFFF).astype(np.uint64)
        k32 = fit if policy == 1 else (np.uint64(0xFFFFFFFF) - fit if policy == 2 else np.zeros_like(fit))
        key = (k32 << np.uint64(32)) | np.arange(fit.shape[0], dtype=np.uint64)
        out.append(np.where(ok, key, np.uint64(0xFFFFFFFFFFFFFFFF)))
    return out


def numpy_sort_us(keys, repeat):
    us = []
    for _ in range(max(repeat, 3)):
        t0 = time.perf_counter()
        for k in keys:
            np.sort(k)
        us.append((time.perf_counter() - t0) * 1e6)
    return med(us)


def order_times(e, policy, iters, repeat, forms=(0, 1, 2)):
    out = {}
    for f in forms:
        e.fit_order(policy, form=f, iters=20)
        out[("own", "rank", "block")[f]] = med([e.fit_order(policy, form=f, iters=iters)[2][0] for _ in range(repeat)])
    return out


def probe_config(cfg, iters, repeat):
    p = synth.CONFIGS[cfg]()
    rc, rl = job_runs(p.job_class)
    it = iters if cfg != 4 else max(iters // 5, 10)
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        call = e.host_placer(rc, rl)
        plain = call()
        tally = e.place(p.job_class, want_tally=True)
        out = {"config": cfg, "rows": p.nodes.n_nodes, "jobs": p.n_jobs, "runs": int(rc.shape[0]),
               "classes": len(p.classes), "domains_per_class": [int(p.topology.n_domains[c.level]) for c in p.classes],
               "iters": it, "repeat": repeat, "plain_placed": int(plain.placed), "place_shape": int(plain.fused),
               "policies": {}}
        for name, pol in POLICIES.items():
            got, st = e.place_fit_runs(rc, rl, pol)
            for _ in range(5):
                call()
                e.place_fit_runs(rc, rl, pol)
            fit_med, fit_p99, place_med = [], [], []
            for _ in range(repeat):
                _, m, q = e.place_fit_loop(rc, rl, pol, it)
                fit_med.append(m)
                fit_p99.append(q)
                place_med.append(call.loop(it)[1])
            out["policies"][name] = {
                "placed": int(st.placed), "slack": int(st.slack), "fit_shape": int(st.fused),
                "fit_us_median": med(fit_med), "fit_us_p99": med(fit_p99), "place_us_median": med(place_med),
                "difference_us": med(fit_med) - med(place_med),
                "order_device_us": order_times(e, pol, it, repeat),
                "numpy_sort_us": numpy_sort_us(host_keys(p, tally.cap, tally.occ, pol), repeat)}
    return out


def probe_size(D, iters, repeat):
    p = synth.config4(n_nodes=20 * D, n_domains=D, jobs=(4, 3, 1, 2))
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        tally = e.place(p.job_class, want_tally=True)
        t = order_times(e, 1, iters, repeat, forms=(1, 2))
        _, nf, _ = e.fit_order(1)
        return {"size": D, "classes": len(p.classes), "feasible": nf.tolist(), "policy": "tightest", "iters": iters,
                "repeat": repeat, "rank_device_us": t["rank"], "block_device_us": t["block"],
                "numpy_sort_us": numpy_sort_us(host_keys(p, tally.cap, tally.occ, 1), repeat)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,5,4")
    ap.add_argument("--sizes", default="")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    for D in [int(x) for x in a.sizes.split(",") if x]:
        print(json.dumps(probe_size(D, a.iters, a.repeat)), flush=True)
    for cfg in [int(x) for x in a.configs.split(",") if x]:
        print(json.dumps(probe_config(cfg, a.iters, a.repeat)), flush=True)


if __name__ == "__main__":
    main()
