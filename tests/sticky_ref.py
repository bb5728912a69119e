"""The yardstick of the sticky-placement tests (DESIGN.md §2 "Sticky
placement"): the rule restated over the CPU oracle. It never calls the
engine. cap / occ come from oracle.place_c; the keep step is rules 1-2 taken
literally (a claimant keeps its domain iff no earlier claimant's leaf range
intersects its own -- a scan over the earlier claimants); every kept domain's
leaves are then counted as occupied, the remaining jobs are placed by
oracle.assign_from_tallies on the problem restricted to them, and the answers
are scattered back."""
import dataclasses

import numpy as np

from jobset_amd import synth
from oracle import oracle as O


def sticky_ref(p, prev, tallies=None):
    """(assign [J], kept [J] bool) of the rule for problem p and hints prev
    (None: no hints). tallies: (cap, occ) of O.place_c(p), computed when None."""
    cap, occ = tallies if tallies is not None else O.place_c(p)[1:]
    J = p.n_jobs
    prev = np.full(J, -1, dtype=np.int64) if prev is None else np.asarray(prev, dtype=np.int64)
    assert prev.shape == (J,)
    fl = [np.asarray(f, dtype=np.int64) for f in p.topology.first_leaf]
    # rule 1: the claimants, in job order, with their leaf ranges
    cj, ca, cb = [], [], []
    for j in np.nonzero(prev >= 0)[0]:
        c = int(p.job_class[j])
        jc = p.classes[c]
        a, b = int(fl[jc.level][prev[j]]), int(fl[jc.level][prev[j] + 1])
        if int(cap[c, a:b].astype(np.int64).sum()) >= jc.pods and int(occ[a:b].sum()) == 0:
            cj.append(int(j))
            ca.append(a)
            cb.append(b)
    A, B = np.array(ca, dtype=np.int64), np.array(cb, dtype=np.int64)
    # rule 2: no earlier claimant (kept or not) intersects
    kept = np.zeros(J, dtype=bool)
    for i, j in enumerate(cj):
        kept[j] = not np.any(np.maximum(A[i], A[:i]) < np.minimum(B[i], B[:i]))
    # rule 3: kept domains are taken; the others fill in global order
    occ2 = np.array(occ, dtype=np.uint32, copy=True)
    for i, j in enumerate(cj):
        if kept[j]:
            occ2[A[i]:B[i]] += 1
    rem = np.nonzero(~kept)[0]
    q = dataclasses.replace(p, job_class=np.ascontiguousarray(p.job_class[rem], dtype=np.uint32), job_names=None)
    out = np.full(J, -1, dtype=np.int32)
    out[kept] = prev[kept]
    if rem.shape[0]:
        out[rem] = O.assign_from_tallies(q, cap, occ2)
    return out, kept


def greedy_keep(p, prev, tallies=None):
    """The sequential greedy the rule deliberately is not: a claimant keeps
    iff no earlier KEEPER intersects. Only to show where the two differ."""
    cap, occ = tallies if tallies is not None else O.place_c(p)[1:]
    fl = [np.asarray(f, dtype=np.int64) for f in p.topology.first_leaf]
    used = np.zeros(p.topology.n_leaves, dtype=bool)
    kept = np.zeros(p.n_jobs, dtype=bool)
    for j in range(p.n_jobs):
        if prev[j] < 0:
            continue
        c = int(p.job_class[j])
        jc = p.classes[c]
        a, b = int(fl[jc.level][prev[j]]), int(fl[jc.level][prev[j] + 1])
        if int(cap[c, a:b].astype(np.int64).sum()) >= jc.pods and int(occ[a:b].sum()) == 0 and not used[a:b].any():
            kept[j] = True
            used[a:b] = True
    return kept


def check_sticky(p, prev, assign, tallies):
    """I1 / I2 of the answer on the snapshot's own tallies, and that a hinted
    job that did not keep its domain is not sitting on it anyway."""
    cap, occ = tallies
    topo = p.topology
    used = np.zeros(topo.n_leaves, dtype=bool)
    for j in range(p.n_jobs):
        d = int(assign[j])
        if d < 0:
            continue
        c = int(p.job_class[j])
        jc = p.classes[c]
        fl = topo.first_leaf[jc.level]
        a, b = int(fl[d]), int(fl[d + 1])
        assert int(cap[c, a:b].astype(np.int64).sum()) >= jc.pods, f"job {j}: domain {d} lacks capacity (I1)"
        assert int(occ[a:b].sum()) == 0, f"job {j}: domain {d} is held by another exclusive job"
        assert not used[a:b].any(), f"job {j}: domain {d} overlaps another job (I2)"
        used[a:b] = True


def moved(prev, assign, kept):
    """hinted, not kept, but placed"""
    return int(((np.asarray(prev) >= 0) & ~kept & (np.asarray(assign) >= 0)).sum())


def lost(prev, assign):
    """hinted and now unplaceable"""
    return int(((np.asarray(prev) >= 0) & (np.asarray(assign) < 0)).sum())


def taint_rows(p, rows, bit):
    p.nodes.taints[np.asarray(rows, dtype=np.int64)] |= np.uint32(bit)


# ---- the three scenarios of DESIGN.md §4 "Sticky placement": (problem before
# the damage, prev = its placement, the damaged problem)
def scenario_cfg2():
    """One more node of job 5's rack tainted."""
    p = synth.config2()
    prev = O.place_c(p)[0].copy()
    r = int(prev[5])
    row = next(n for n in range(r * 15, r * 15 + 15) if p.nodes.taints[n] == 0)
    taint_rows(p, [row], 1)
    return p, prev


def scenario_cfg5():
    """One row of one placed rack job tainted (a taint no class tolerates)."""
    p = synth.config5()
    prev = O.place_c(p)[0].copy()
    j = next(j for j in range(p.n_jobs) if p.classes[int(p.job_class[j])].level == 1 and prev[j] >= 0)
    taint_rows(p, [int(prev[j]) * 16], 0x10)
    return p, prev


def scenario_cfg4(n_nodes=65_536, n_domains=3_125, jobs=(1000, 750, 250, 500)):
    """Three placed racks tainted whole (a taint no class tolerates)."""
    p = synth.config4(n_nodes=n_nodes, n_domains=n_domains, jobs=jobs)
    prev = O.place_c(p)[0].copy()
    placed = np.nonzero(prev >= 0)[0]
    ls = p.nodes.leaf_start
    for j in (placed[3], placed[len(placed) // 2], placed[-2]):
        d = int(prev[j])
        taint_rows(p, np.arange(int(ls[d]), int(ls[d + 1])), 0x100)
    return p, prev
