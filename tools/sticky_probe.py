"""jsp_place_sticky beside jsp_place on the launch path (DESIGN.md §4 "Sticky
placement"): same process, resident service off. prev = the placement of the
undamaged snapshot, the call runs on the damaged one. After 10 warm-up calls,
the median of `repeat` C-timed loops of `iters` calls each
(jspb_place_sticky_loop, jspb_place_loop), the launches of each call (derived
from the code by the shape the call reports), and the
dispatch-event time of an empty launch measured in the same process
(jspb_tally_device_spans).

    python tools/sticky_probe.py [--cfg 2] [--iters 200] [--repeat 5] [--grid]
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


def damage(cfg, p, prev):
    """The scenarios of DESIGN.md §4: rows of placed jobs' racks get a taint their class does not tolerate."""
    ls = p.nodes.leaf_start
    placed = np.nonzero(prev >= 0)[0]
    if cfg == 2:
        r = int(prev[5])
        p.nodes.taints[next(n for n in range(r * 15, r * 15 + 15) if p.nodes.taints[n] == 0)] |= 1
    elif cfg == 5:
        j = next(j for j in placed if p.classes[int(p.job_class[j])].level == 1)
        p.nodes.taints[int(prev[j]) * 16] |= 0x10
    else:
        for j in (placed[3], placed[len(placed) // 2], placed[-2]):
            d = int(prev[j])
            p.nodes.taints[int(ls[d]):int(ls[d + 1])] |= 0x100


def launches(fused, p, n_runs, sticky, grid):
    """Kernel launches of one call, derived from the code by the shape the call reports (jsp_stats.fused),
    not observed: a kernel trace of this probe (rocprofv3 --kernel-trace --stats) shows the same kernels,
    calls / iterations each. The grid form's one H2D copy of the staging is not a kernel launch."""
    tally = (len(p.classes) + 15) // 16
    level_walk = len({c.level for c in p.classes}) == 1 and n_runs <= 32
    if not sticky:
        # 0: tally (feasibility folded in for <= 4 leaf-level classes) + the walker
        fold = len(p.classes) <= 4 and all(c.level + 1 == p.topology.n_levels for c in p.classes)
        return {0: tally + (0 if fold else 1) + (1 if level_walk else 2), 1: 1, 2: 1, 7: tally + 2, 8: 1}.get(fused)
    if fused == 7:
        return tally + 1 + (4 if grid else 1) + 2          # feasibility, keep, words copy + tag; the host scatters
    return tally + 1 + (4 if grid else 1) + (1 if level_walk else 2) + 1   # ..., the walker (+ expansion), scatter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=int, default=2, choices=(2, 4, 5))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", action="store_true", help="force the grid keep form (JSP_TEST_HOOKS sticky_grid=1)")
    a = ap.parse_args()
    if a.grid:
        os.environ["JSP_TEST_HOOKS"] = "sticky_grid=1"
    p = synth.CONFIGS[a.cfg]()
    rc, rl = job_runs(p.job_class)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        prev = e.place(p.job_class).assign.copy()
        damage(a.cfg, p, prev)
        e.load(p)
        plain = e.place(p.job_class)
        got, st = e.place_sticky_runs(rc, rl, prev)
        call = e.host_placer(rc, rl)
        for _ in range(10):
            call()
            e.place_sticky_runs(rc, rl, prev)
        sticky_us = [e.place_sticky_loop(rc, rl, prev, a.iters)[1] for _ in range(a.repeat)]
        place_us = [call.loop(a.iters)[1] for _ in range(a.repeat)]
        empty_us = None
        try:
            import torch
            L = p.topology.n_leaves
            cap = torch.zeros((len(p.classes), L), dtype=torch.int32, device="cuda")
            occ = torch.zeros(L, dtype=torch.int32, device="cuda")
            empty_us = e.tally_device_spans(cap.data_ptr(), occ.data_ptr(), L, 200)[2]
        except Exception as ex:  # the span probe needs the wave-tile tally
            empty_us = str(ex)
    grid = a.grid or p.n_jobs > 1024
    n_s, n_p = launches(int(st.fused), p, len(rc), True, grid), launches(plain.fused, p, len(rc), False, grid)
    out = {"cfg": a.cfg, "rows": p.nodes.n_nodes, "jobs": p.n_jobs, "classes": len(p.classes), "iters": a.iters,
           "repeat": a.repeat, "keep_form": "grid" if grid else "one-workgroup",
           "moved_plain": int(((prev >= 0) & (plain.assign != prev)).sum()),
           "moved_sticky": int(((prev >= 0) & (got != prev)).sum()), "kept": int(st.kept),
           "sticky_fill_shape": int(st.fused), "place_shape": int(plain.fused),
           "sticky_us": sticky_us, "place_us": place_us, "sticky_us_median": med(sticky_us),
           "place_us_median": med(place_us), "sticky_launches": n_s, "place_launches": n_p, "empty_launch_us": empty_us}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
