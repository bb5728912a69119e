"""The yardstick of the gang-placement tests (DESIGN.md §2 "Gang placement"):
the rule restated over the CPU oracle's tallies. It never calls the engine.

cap / occ come from oracle.place_c. The taken set T is an array of used
leaves: a domain is in T, or was taken earlier in a trial, iff one of its
leaves is used (a take marks every intersecting domain at every level, and
two domains of a nested hierarchy intersect iff they share a leaf). Every
trial works on its own copy of that array, there is no prefilter, and every
candidate S is tried in ascending order until one succeeds.

Also here: the inputs of the sweeps (sweep_case), shared by the CPU tests,
which assert the coverage floors on this reference's own output, and the GPU
tests, which compare the engine with it."""
import dataclasses

import numpy as np

from jobset_amd import synth
from jobset_amd.snapshot import JobClass
from oracle import oracle as O

ANY = 0xFFFFFFFF


def feasibility(p, cap, occ):
    """feas[c]: bool [D[level[c]]], DESIGN §2's feasible(c, d) from the tallies."""
    occ_cs = np.concatenate([[0], np.cumsum(occ.astype(np.int64))])
    out = []
    for c, jc in enumerate(p.classes):
        fl = np.asarray(p.topology.first_leaf[jc.level], dtype=np.int64)
        cs = np.concatenate([[0], np.cumsum(cap[c].astype(np.int64))])
        out.append(((cs[fl[1:]] - cs[fl[:-1]]) >= jc.pods) & ((occ_cs[fl[1:]] - occ_cs[fl[:-1]]) == 0))
    return out


def gang_ref(p, gang_jobs, gang_span, tallies=None):
    """(assign [J], span_out [G]) of the rule. gang_jobs[g]: the number of jobs
    of gang g (consecutive in p.job_class, global order; their sum is J);
    gang_span[g]: a level or ANY. tallies: (cap, occ) of O.place_c(p)."""
    cap, occ = tallies if tallies is not None else O.place_c(p)[1:]
    topo = p.topology
    fl = [np.asarray(f, dtype=np.int64) for f in topo.first_leaf]
    L = topo.n_leaves
    feas = feasibility(p, cap, occ)
    J = p.n_jobs
    assert int(np.sum(gang_jobs)) == J
    assign = np.full(J, -1, dtype=np.int32)
    span_out = np.full(len(gang_jobs), -1, dtype=np.int32)
    used = np.zeros(L, dtype=bool)
    j0 = 0
    for g, (n, s) in enumerate(zip(gang_jobs, gang_span)):
        n, s = int(n), int(s) & 0xFFFFFFFF
        jobs = range(j0, j0 + n)
        j0 += n
        if n == 0:
            continue
        cands = [(0, 0, L)] if s == ANY else [(S, int(fl[s][S]), int(fl[s][S + 1])) for S in range(topo.n_domains[s])]
        for S, a_S, b_S in cands:
            u = used.copy()
            ans = []
            for j in jobs:
                c = int(p.job_class[j])
                f = fl[p.classes[c].level]
                a, b = f[:-1], f[1:]
                ucs = np.concatenate([[0], np.cumsum(u)])
                ok = (a < b) & (a >= a_S) & (b <= b_S) & feas[c] & ((ucs[b] - ucs[a]) == 0)
                hit = np.nonzero(ok)[0]
                if hit.size == 0:
                    break
                d = int(hit[0])
                u[a[d]:b[d]] = True
                ans.append(d)
            if len(ans) == n:
                used = u
                assign[jobs.start:jobs.stop] = ans
                span_out[g] = S
                break
    return assign, span_out


def check_gangs(p, gang_jobs, gang_span, assign, span_out, tallies):
    """I1 / I2 of the answer on the snapshot's own tallies; every gang whole or
    nothing; a placed gang's domains inside its span domain; span_out consistent."""
    cap, occ = tallies
    topo = p.topology
    used = np.zeros(topo.n_leaves, dtype=bool)
    j0 = 0
    for g, (n, s) in enumerate(zip(gang_jobs, gang_span)):
        n, s = int(n), int(s) & 0xFFFFFFFF
        a_g = np.asarray(assign[j0:j0 + n])
        S = int(span_out[g])
        if n == 0 or S < 0:
            assert S == -1 and np.all(a_g == -1), f"gang {g}: refused but holds a domain"
        else:
            assert np.all(a_g >= 0), f"gang {g}: placed in part"
            assert S == 0 if s == ANY else 0 <= S < topo.n_domains[s]
            lo, hi = (0, topo.n_leaves) if s == ANY else (int(topo.first_leaf[s][S]), int(topo.first_leaf[s][S + 1]))
            for j in range(j0, j0 + n):
                c = int(p.job_class[j])
                jc = p.classes[c]
                f = topo.first_leaf[jc.level]
                a, b = int(f[assign[j]]), int(f[assign[j] + 1])
                assert a < b and lo <= a and b <= hi, f"job {j}: domain outside span domain {S} of gang {g}"
                assert int(cap[c, a:b].astype(np.int64).sum()) >= jc.pods, f"job {j}: lacks capacity (I1)"
                assert int(occ[a:b].sum()) == 0, f"job {j}: held by another exclusive job"
                assert not used[a:b].any(), f"job {j}: overlaps another job (I2)"
                used[a:b] = True
        j0 += n


def gang_runs_of(job_class, gang_jobs):
    """(run_class, run_len, gang_runs) of jsp_place_gangs for one class id per
    job and the gangs' job counts: runs never cross a gang boundary."""
    rc, rl, gr = [], [], []
    j0 = 0
    for n in gang_jobs:
        n = int(n)
        r0 = len(rc)
        for j in range(j0, j0 + n):
            c = int(job_class[j])
            if len(rc) > r0 and rc[-1] == c:
                rl[-1] += 1
            else:
                rc.append(c)
                rl.append(1)
        gr.append(len(rc) - r0)
        j0 += n
    return (np.array(rc, dtype=np.uint32), np.array(rl, dtype=np.uint32), np.array(gr, dtype=np.uint32))


def feas_words(p, cap, occ):
    """The engine's feasibility words (class c's (D + 63) // 64 words after
    those of the classes before it) from the tallies."""
    out = []
    for f in feasibility(p, cap, occ):
        bits = np.zeros(((f.shape[0] + 63) // 64) * 64, dtype=np.uint8)
        bits[:f.shape[0]] = f
        out.append(np.packbits(bits, bitorder="little").view(np.uint64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def span_counts_ref(p, cap, occ):
    """jspb_span_counts' output in numpy: for class c, s <= level[c], S: the
    feasible level[c] domains in S's child range followed down to level[c]
    (first_leaf lower bounds, as the engine's child_start), in its layout."""
    topo = p.topology
    fl = [np.asarray(f, dtype=np.int64) for f in topo.first_leaf]
    out = []
    for c, f in enumerate(feasibility(p, cap, occ)):
        lc = p.classes[c].level
        fcs = np.concatenate([[0], np.cumsum(f.astype(np.int64))])
        for s in range(lc + 1):
            lo = np.arange(topo.n_domains[s] + 1, dtype=np.int64)
            for k in range(s, lc):
                lo = np.searchsorted(fl[k + 1], fl[k][lo], side="left")
            out.append(fcs[lo[1:]] - fcs[lo[:-1]])
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, dtype=np.uint32)


# ---------------------------------------------------------------- sweep inputs
SWEEP_SEEDS = range(60)


def sweep_case(seed):
    """(problem, gang_jobs, gang_span): random_problem's topology, nodes and
    occupancy with permissive classes (no selector, half of them tolerating
    every taint bit, small requests, pods up to half the largest leaf, a random
    level), and gangs of 1-3 consecutive runs of 1-4 jobs with a random span
    among the levels not finer than the gang's classes, or ANY."""
    base = synth.random_problem(seed, max_nodes=1500, max_leaves=120, max_jobs=60)
    s = 77_000 + seed
    u = lambda stream, lo, hi: int(synth.uniform_int(s, stream, 1, lo, hi)[0])  # noqa: E731
    topo, nodes = base.topology, base.nodes
    K = topo.n_levels
    sizes = np.diff(np.asarray(nodes.leaf_start, dtype=np.int64))
    C = u(1, 1, 6)
    classes = []
    for c in range(C):
        res = tuple(u(10 + 8 * c + r, 0, max(1, int(nodes.free[r].max()) // 8)) for r in range(nodes.n_res))
        classes.append(JobClass(tolerated_taints=0xFFFF if c % 2 == 0 else 0, level=u(100 + c, 0, K - 1),
                                pods=u(200 + c, 1, max(1, int(sizes.max()) // 2)), req_res=res))
    jc, gang_jobs, gang_span = [], [], []
    n_gangs = u(2, 1, 14)
    for g in range(n_gangs):
        n = 0
        lv = K - 1
        for r in range(u(300 + 8 * g, 1, 3)):
            c = u(301 + 8 * g + r, 0, C - 1)
            m = u(304 + 8 * g + r, 1, 4)
            jc += [c] * m
            n += m
            lv = min(lv, classes[c].level)
        pick = u(307 + 8 * g, 0, lv + 1)
        gang_jobs.append(n)
        gang_span.append(ANY if pick == lv + 1 else pick)
    p = dataclasses.replace(base, classes=classes, job_class=np.array(jc, dtype=np.uint32), job_names=None,
                            name=f"gang-sweep-{seed}")
    return p, np.array(gang_jobs, dtype=np.int64), np.array(gang_span, dtype=np.int64)


def reduction_problem(i):
    """The problems of the two reductions: random_problem's seeds 0-39 (none of
    whose batches places whole), then the first jobs of 20 sweep problems
    (permissive classes: most of them place whole)."""
    if i < 40:
        return synth.random_problem(i, max_nodes=600, max_leaves=40)
    p = sweep_case(i - 40)[0]
    return dataclasses.replace(p, job_class=p.job_class[:4])
