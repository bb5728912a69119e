"""jsp_explain's row pass beside the tally on one snapshot:
device microseconds per launch of explain_rows_kernel and of the tally, HIP
events around back-to-back launches after a warm-up (jspb_explain_rows_loop),
and the algorithmic bytes / time of each as a fraction of 8 TB/s.

    python tools/explain_probe.py [--cfg 4] [--iters 200] [--repeat 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jobset_amd import synth  # noqa: E402
from jobset_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    p = synth.CONFIGS[a.cfg]()
    N, W, R = p.nodes.n_nodes, p.nodes.n_label_words, p.nodes.n_res
    row_bytes = N * (8 * W + 8 + 4 * R)
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        e.explain()
        runs = [e.explain_rows_loop(a.iters) for _ in range(a.repeat)]
    rows_us = sorted(r[0] for r in runs)
    tally_us = sorted(r[1] for r in runs)
    med = lambda v: v[len(v) // 2]  # noqa: E731
    print(json.dumps({"cfg": a.cfg, "rows": N, "classes": len(p.classes), "iters": a.iters, "repeat": a.repeat,
                      "row_bytes": row_bytes, "explain_rows_us": rows_us, "tally_us": tally_us,
                      "explain_rows_us_median": med(rows_us), "tally_us_median": med(tally_us),
                      "explain_rows_frac_8TBs": row_bytes / (med(rows_us) * 1e-6) / 8e12,
                      "tally_frac_8TBs": row_bytes / (med(tally_us) * 1e-6) / 8e12}))


if __name__ == "__main__":
    main()
