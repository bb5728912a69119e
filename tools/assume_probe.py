"""jsp_assume / jsp_forget on the launch path (DESIGN.md §4 "jsp_assume /
jsp_forget (measured)"): same process, resident service off, assign = the
config's own placement, one owner per job from 0x40000000. After 10 warm-up
rounds, `repeat` C-timed loops of `iters` rounds each (jspb_assume_forget_loop:
one assume, then the forget of its owners, so every round sees the same
snapshot): the median and p99 of each half, the median over the loops.

Beside it, what a caller has without the two calls: one jsp_snapshot_patch of
the excl_owner column for the same rows (the rows of every committed domain,
computed on the host, with their owners), and one more with -1 to take it back.
Each is timed to completion (the call, then jsp_engine_sync, as jsp_assume
returns when done) and alone, from this interpreter (two ctypes calls: a few
microseconds of the figure). The host's work of computing the rows is not in
it. Bytes are algorithmic: jsp_forget reads 4 N and writes 4 per cleared row;
jsp_assume reads the committed domains' rows x (8 W + 8 + 4 R), writes 4 per
marked row, reads 28 bytes per job and writes 12.

    python tools/assume_probe.py [--cfg 2] [--iters 200] [--repeat 5] [--nodes N --domains D]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", type=int, default=2, choices=(2, 3, 4, 5))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=0, help="cfg4 only: rows (default 1M)")
    ap.add_argument("--domains", type=int, default=0, help="cfg4 only: racks (default 50,000)")
    a = ap.parse_args()
    if a.cfg == 4 and a.nodes:
        p = synth.config4(n_nodes=a.nodes, n_domains=a.domains or 50_000)
    else:
        p = synth.CONFIGS[a.cfg]()
    rc, rl = job_runs(p.job_class)
    owner = (0x40000000 + np.arange(p.n_jobs)).astype(np.int32)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    nd, topo = p.nodes, p.topology
    ls = nd.leaf_start.astype(np.int64)
    with Engine(0) as e:
        e.set_service(False)
        e.load(p)
        before = e.place(p.job_class, want_tally=True)
        assign = before.assign.copy()
        committed, st = e.assume_runs(rc, rl, assign, owner)
        held = owner[assign >= 0]
        cleared = e.forget(held)
        for _ in range(10):
            e.assume_runs(rc, rl, assign, owner)
            e.forget(held)
        loops = [e.assume_forget_loop(rc, rl, assign, owner, a.iters)[0] for _ in range(a.repeat)]
        # the alternative: the same rows through jsp_snapshot_patch
        rows, own = [], []
        for j in np.nonzero(committed)[0]:
            fl = topo.first_leaf[p.classes[int(p.job_class[j])].level]
            r0, r1 = int(ls[int(fl[assign[j]])]), int(ls[int(fl[assign[j] + 1])])
            rows.append(np.arange(r0, r1, dtype=np.uint32))
            own.append(np.full(r1 - r0, owner[j], dtype=np.int32))
        rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint32)
        own = np.concatenate(own) if own else np.zeros(0, dtype=np.int32)
        mark = e.host_patcher(rows, excl=own)
        clear = e.host_patcher(rows, excl=np.full(rows.shape[0], -1, dtype=np.int32))
        n = max(a.iters // 4, 10)
        t_mark, t_clear, t_mark_call, t_clear_call = [], [], [], []
        for i in range(10 + n):
            t0 = time.perf_counter_ns()
            mark()
            t1 = time.perf_counter_ns()
            e.sync()
            t2 = time.perf_counter_ns()
            clear()
            t3 = time.perf_counter_ns()
            e.sync()
            t4 = time.perf_counter_ns()
            if i >= 10:
                t_mark.append((t2 - t0) / 1e3)
                t_mark_call.append((t1 - t0) / 1e3)
                t_clear.append((t4 - t2) / 1e3)
                t_clear_call.append((t3 - t2) / 1e3)
        after = e.place(p.job_class, want_tally=True)
        same = bool(np.array_equal(after.assign, assign) and np.array_equal(after.occ, before.occ) and
                    np.array_equal(after.cap, before.cap))
    row_bytes = 8 * nd.n_label_words + 8 + 4 * nd.n_res
    p99 = lambda v: sorted(v)[min(len(v) - 1, int(0.99 * len(v)))]  # noqa: E731
    am, a99, fm, f99 = (med([x[i] for x in loops]) for i in range(4))
    out = {"cfg": a.cfg, "rows": nd.n_nodes, "jobs": p.n_jobs, "classes": len(p.classes), "iters": a.iters,
           "repeat": a.repeat, "committed": int(st.committed), "stale": int(st.stale),
           "rows_marked": int(st.rows_marked), "rows_cleared": int(cleared), "snapshot_restored": same,
           "assume_us_median": am, "assume_us_p99": a99, "forget_us_median": fm, "forget_us_p99": f99,
           "assume_us_loops": [x[0] for x in loops], "forget_us_loops": [x[2] for x in loops],
           "patch_rows": int(rows.shape[0]), "patch_rounds": n,
           "patch_mark_us_median": med(t_mark), "patch_mark_us_p99": p99(t_mark),
           "patch_clear_us_median": med(t_clear), "patch_clear_us_p99": p99(t_clear),
           "patch_mark_call_only_us_median": med(t_mark_call), "patch_clear_call_only_us_median": med(t_clear_call),
           "patch_mark_over_assume": med(t_mark) / am if am else None,
           "patch_clear_over_forget": med(t_clear) / fm if fm else None,
           "forget_bytes_read_min": 4 * nd.n_nodes, "forget_bytes_written": 4 * int(cleared),
           "assume_bytes": int(st.rows_marked) * (row_bytes + 4) + 40 * p.n_jobs + 8 * sum(topo.n_domains)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
