"""jsp_place_prefer beside jsp_place_fit (TIGHTEST) on the same snapshot and
runs (DESIGN.md §9 "Preferred placement"): fit is the same pipeline without
the row pass. Per shape, label bit 62 on a seeded third of the racks and one
term per class; one process, resident service off.

  call:   C-timed back-to-back calls (jspb_place_prefer_loop,
          jspb_place_fit_loop), the median of each of `repeat` rounds of
          `iters`; min / p50 / max over the rounds.
  device: the three score launches (base, rows, keys) alone, events on the
          dispatches (jspb_prefer_order), median and mean of `order_iters`.

One JSON line per shape."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jobset_amd import native, synth  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402
from jobset_amd.snapshot import job_runs  # noqa: E402

SHAPES = {"cfg2": synth.config2, "cfg5": synth.config5}


def spread(v):
    v = sorted(v)
    return {"min": v[0], "p50": v[len(v) // 2], "max": v[-1]}


def probe(name, iters, repeat, order_iters):
    p = SHAPES[name]()
    terms = synth.prefer_racks(p, 7)
    rc, rl = job_runs(p.job_class)
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        plain = e.place(p.job_class).assign.copy()
        a, sc, st = e.place_prefer_runs(rc, rl, terms)
        e.place_prefer_loop(rc, rl, terms, iters=20)                                  # warm
        pm = [e.place_prefer_loop(rc, rl, terms, iters=iters)[1] for _ in range(repeat)]
        e.place_fit_loop(rc, rl, native.JSP_FIT_TIGHTEST, iters=20)
        fm = [e.place_fit_loop(rc, rl, native.JSP_FIT_TIGHTEST, iters=iters)[1] for _ in range(repeat)]
        e.prefer_order(terms, iters=20)
        *_, (d_med, d_mean) = e.prefer_order(terms, iters=order_iters)
    return {"shape": name, "rows": p.nodes.n_nodes, "leaves": p.topology.n_leaves, "jobs": p.n_jobs,
            "classes": len(p.classes), "placed": int(st.placed), "score": int(st.score),
            "differs_from_place": int((a != plain).sum()), "iters": iters, "repeat": repeat,
            "prefer_call_us": spread(pm), "fit_call_us": spread(fm),
            "score_launches_device_us": {"median": d_med, "mean": d_mean}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--order-iters", type=int, default=200)
    a = ap.parse_args()
    for name in [x for x in a.shapes.split(",") if x]:
        print(json.dumps(probe(name, a.iters, a.repeat, a.order_iters)), flush=True)


if __name__ == "__main__":
    main()
