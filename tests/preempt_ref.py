"""The yardstick of the preemptive-placement tests (DESIGN.md §2 "Preemptive
placement"): the rule taken literally in numpy. It never calls the engine.

Every row is free, a victim (its owner is in the table with a rank below
prio) or a blocker (every other owned row). cap' is oracle.tally_nodes on a
copy of the nodes whose victim rows carry evict_free in place of free_res;
capsum' is an int64 sum over a domain's leaves. A domain is reachable when
capsum' >= pods and none of its rows is a blocker; its key is
(hp << 16) | min(seg, 0xFFFF) with hp = 0 without a victim row, else 1 + the
largest victim rank, and seg the owner segments. Every job takes, among the
reachable domains of its class's level none of whose leaves is used, the one
with the smallest (key, d): a literal O(J D) walk.

Also here: check_preempt (the answer's invariants), order_ref (the candidate
lists, keys and seg in the engine's layout), the hand cases and the sweep
generator, shared by the CPU tests, which assert the coverage floors on this
reference's own output, and the GPU tests, which compare the engine with it."""
import dataclasses

import numpy as np

from jobset_amd import synth
from jobset_amd.snapshot import Nodes, job_runs
from oracle import oracle as O
from bind_ref import cls, flat, nested
from gang_ref import feasibility, reduction_problem, sweep_case  # noqa: F401  (the tests' inputs)

BLOCKER = 0xFFFFFFFF
TAIL = 0xFFFFFFFF
MAX_PRIO = 65535
INT32_MIN = -(1 << 31)


def table(owners, owner_prio):
    ids = np.asarray(owners, dtype=np.int64).reshape(-1)
    pr = np.asarray(owner_prio, dtype=np.int64).reshape(-1)
    assert ids.shape == pr.shape and np.unique(ids).shape == ids.shape and not np.any(ids == -1)
    assert np.all((pr >= 0) & (pr < MAX_PRIO))
    return ids, pr


def row_codes(excl, prio, owners, owner_prio):
    """int64 [N]: 0 for a free row, 1 + rank for a victim row, BLOCKER else."""
    ids, pr = table(owners, owner_prio)
    rank = dict(zip(ids.tolist(), pr.tolist()))
    out = np.zeros(excl.shape[0], dtype=np.int64)
    for n, o in enumerate(np.asarray(excl, dtype=np.int64).tolist()):
        if o == -1:
            continue
        r = rank.get(o)
        out[n] = 1 + r if r is not None and r < prio else BLOCKER
    return out


def vacated(p, prio, owners, owner_prio, evict_free=None, clear=False):
    """Problem p whose victim rows carry evict_free (a copy). clear: their
    owner removed too, the snapshot the evictions would leave."""
    n = p.nodes
    code = row_codes(n.excl, prio, owners, owner_prio)
    vic = (code != 0) & (code != BLOCKER)
    free, excl = n.free.copy(), n.excl.copy()
    if evict_free is not None:
        ef = np.asarray(evict_free, dtype=np.uint32).reshape(free.shape)
        free[:, vic] = ef[:, vic]
    if clear:
        excl[vic] = -1
    nodes = Nodes(leaf_start=n.leaf_start, labels=n.labels, taints=n.taints, free=free, excl=excl,
                  leaf_begin=n.leaf_begin)
    return dataclasses.replace(p, nodes=nodes), code


def domain_table(p, prio, owners, owner_prio, evict_free=None):
    """Per class c: (reach bool [D], key int64 [D], seg int64 [D]) at level[c]."""
    q, code = vacated(p, prio, owners, owner_prio, evict_free)
    cap = O.tally_nodes(p.topology.n_leaves, q.nodes, p.classes)[0]
    excl = np.asarray(p.nodes.excl, dtype=np.int64)
    ls = np.asarray(p.nodes.leaf_start, dtype=np.int64)
    out = []
    for c, jc in enumerate(p.classes):
        fl = np.asarray(p.topology.first_leaf[jc.level], dtype=np.int64)
        D = fl.shape[0] - 1
        reach, key, seg = np.zeros(D, dtype=bool), np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64)
        for d in range(D):
            capsum = int(cap[c, fl[d]:fl[d + 1]].astype(np.int64).sum())
            r0, r1 = int(ls[fl[d]]), int(ls[fl[d + 1]])
            blockers = hp = 0
            for n in range(r0, r1):
                if excl[n] != -1 and (n == r0 or excl[n - 1] != excl[n]):
                    seg[d] += 1
                if code[n] == BLOCKER:
                    blockers += 1
                elif code[n] != 0:
                    hp = max(hp, int(code[n]))
            reach[d] = capsum >= jc.pods and blockers == 0
            key[d] = (hp << 16) | min(int(seg[d]), 0xFFFF)
        out.append((reach, key, seg))
    return out


def heads(p, level, d):
    """The owners at the segment heads of domain d, in ascending row order."""
    excl = np.asarray(p.nodes.excl, dtype=np.int64)
    fl, ls = p.topology.first_leaf[level], p.nodes.leaf_start
    r0, r1 = int(ls[int(fl[d])]), int(ls[int(fl[d + 1])])
    return [int(excl[n]) for n in range(r0, r1) if excl[n] != -1 and (n == r0 or excl[n - 1] != excl[n])]


def preempt_ref(p, prio, owners, owner_prio, evict_free=None, tab=None):
    """(assign int32 [J], victim_off uint32 [J + 1], victims int32 [total],
    stats dict) of the rule for problem p (jobs p.job_class in global order)."""
    tab = tab if tab is not None else domain_table(p, prio, owners, owner_prio, evict_free)
    topo = p.topology
    fl = [np.asarray(f, dtype=np.int64) for f in topo.first_leaf]
    J = p.n_jobs
    assign = np.full(J, -1, dtype=np.int32)
    used = np.zeros(topo.n_leaves, dtype=bool)
    off, victims = [0], []
    preempting = 0
    for j in range(J):
        c = int(p.job_class[j])
        lvl = p.classes[c].level
        reach, key, _ = tab[c]
        f = fl[lvl]
        a, b = f[:-1], f[1:]
        ucs = np.concatenate([[0], np.cumsum(used)])
        cand = np.nonzero(reach & ((ucs[b] - ucs[a]) == 0))[0]
        if cand.size:
            d = int(cand[np.lexsort((cand, key[cand]))[0]])  # the smallest (key, d)
            used[a[d]:b[d]] = True
            assign[j] = d
            v = heads(p, lvl, d)
            victims += v
            preempting += int(len(v) > 0)
        off.append(len(victims))
    stats = dict(jobs=J, placed=int((assign >= 0).sum()), preempting=preempting, victims=len(victims),
                 runs=int(job_runs(p.job_class)[0].shape[0]), fused=7)
    return assign, np.array(off, dtype=np.uint32), np.array(victims, dtype=np.int32), stats


def order_ref(p, prio, owners, owner_prio, evict_free=None, tab=None):
    """(order uint32 [n], nf uint32 [C], key uint32 [n], seg uint32 [n]) in the
    engine's layout (jsplace_bench.h jspb_preempt_order): class c's segment
    follows those of the classes before it; in `order` its nf[c] reachable
    domains in ascending (key, d) first, 0xFFFFFFFF behind them; key and seg by
    domain id."""
    tab = tab if tab is not None else domain_table(p, prio, owners, owner_prio, evict_free)
    order, nf, keys, segs = [], [], [], []
    for reach, key, seg in tab:
        cand = np.nonzero(reach)[0]
        cand = cand[np.lexsort((cand, key[cand]))]
        s = np.full(reach.shape[0], TAIL, dtype=np.uint32)
        s[:cand.shape[0]] = cand
        order.append(s)
        nf.append(cand.shape[0])
        keys.append(key.astype(np.uint32))
        segs.append(seg.astype(np.uint32))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.uint32)  # noqa: E731
    return cat(order), np.array(nf, dtype=np.uint32), cat(keys), cat(segs)


def check_preempt(p, prio, owners, owner_prio, evict_free, assign, victim_off, victims, tab=None):
    """The invariants of an answer: the taken domains are pairwise disjoint;
    each is feasible (gang_ref.feasibility) on the copy whose victim rows are
    vacated; every job took the smallest (key, d) among the reachable domains
    disjoint from the earlier ones, or had none; the victim lists are the
    segment heads."""
    tab = tab if tab is not None else domain_table(p, prio, owners, owner_prio, evict_free)
    q, _ = vacated(p, prio, owners, owner_prio, evict_free, clear=True)
    feas = feasibility(q, *O.tally_nodes(p.topology.n_leaves, q.nodes, p.classes))
    topo = p.topology
    used = np.zeros(topo.n_leaves, dtype=bool)
    assert victim_off.shape[0] == p.n_jobs + 1 and victim_off[0] == 0 and victim_off[-1] == victims.shape[0]
    for j in range(p.n_jobs):
        c = int(p.job_class[j])
        lvl = p.classes[c].level
        fl = np.asarray(topo.first_leaf[lvl], dtype=np.int64)
        reach, key, seg = tab[c]
        np.testing.assert_array_equal(reach, feas[c])
        ucs = np.concatenate([[0], np.cumsum(used)])
        cand = np.nonzero(reach & ((ucs[fl[1:]] - ucs[fl[:-1]]) == 0))[0]
        d = int(assign[j])
        mine = victims[int(victim_off[j]):int(victim_off[j + 1])]
        if d < 0:
            assert cand.size == 0, f"job {j}: domain {cand[:1]} was reachable"
            assert mine.shape[0] == 0
            continue
        assert feas[c][d], f"job {j}: domain {d} is not feasible once its victims are gone"
        assert not used[fl[d]:fl[d + 1]].any(), f"job {j}: overlaps an earlier job"
        best = min((int(key[x]), int(x)) for x in cand)
        assert (int(key[d]), d) == best, f"job {j}: took {(int(key[d]), d)}, {best} was open"
        used[fl[d]:fl[d + 1]] = True
        assert mine.tolist() == heads(p, lvl, d) and mine.shape[0] == seg[d]


def stats_dict(st):
    return dict(jobs=int(st.jobs), placed=int(st.placed), preempting=int(st.preempting), victims=int(st.victims),
                runs=int(st.runs), fused=int(st.fused))


# ---- hand cases: name -> (problem, prio, owners, owner_prio, evict_free or None, assign, victims per job)
def hand_cases():
    A, B = 7, 9
    rack = cls(0, 2)
    # three racks of two rows; rack 0 held by A (rank 1), rack 1 by B (rank 0), rack 2 free
    f3 = flat([2, 2, 2], [rack], [0, 0, 0], excl=[A, A, B, B, -1, -1])
    # rack 0 held and without room, rack 1 free
    ef = flat([2, 2], [rack], [0, 0], excl=[A, A, -1, -1], free=[0, 0, 1, 1])
    # two zones of two racks of two rows: zone 0 holds two rank-0 owners, zone 1 one rank-1 owner
    ne = nested([[0, 2, 4], np.arange(5)], [2, 2, 2, 2], [cls(0, 4)], [0, 0], excl=[1, 1, 2, 2, 3, 3, 3, 3])
    # one rack of three rows held a, b, a
    sp = flat([3], [cls(0, 3)], [0], excl=[A, B, A])
    # a zone-level owner under two rack-level jobs
    zo = nested([[0, 2], np.arange(3)], [2, 2], [cls(1, 2)], [0, 0], excl=[A, A, A, A])
    # zone 0 = racks 0, 1: A's segment crosses the leaf boundary inside the zone; zone 1 = rack 2 (4 rows), free
    lb = nested([[0, 2, 3], np.arange(4)], [2, 2, 4], [cls(0, 4), cls(1, 2)], [0],
                excl=[-1, A, A, -1, -1, -1, -1, -1])
    # A's segment crosses the boundary between racks 0 and 1
    db = flat([2, 2], [rack], [0, 0], excl=[-1, A, A, -1])
    # special ids and ranks
    si = flat([2, 2], [rack], [0, 0], excl=[0, 0, INT32_MIN, INT32_MIN])
    return {
        # the free rack first, then the lower rank, then the higher
        "flat3": (f3, 2, [A, B], [1, 0], None, [2, 1, 0], [[], [B], [A]]),
        # at prio 1 A (rank 1) is no victim: the last job gets -1
        "flat3-lower": (f3, 1, [A, B], [1, 0], None, [2, 1, -1], [[], [B], []]),
        # a holder that is not in the table blocks
        "not-in-table": (f3, 2, [B], [0], None, [2, 1, -1], [[], [B], []]),
        # a holder whose rank equals prio blocks: the comparison is strict
        "equal-rank": (f3, 1, [A, B], [1, 1], None, [2, -1, -1], [[], [], []]),
        # rack 0 is reachable only through evict_free
        "evict-free": (ef, 1, [A], [0], [[1, 1, 0, 0]], [1, 0], [[], [A]]),
        "evict-free-null": (ef, 1, [A], [0], None, [1, -1], [[], []]),
        # hp decides before the count: zone 0 (two rank-0 owners, key 1 << 16 | 2) before zone 1 (one rank-1, 2 << 16 | 1)
        "nested-hp": (ne, 5, [1, 2, 3], [0, 0, 1], None, [0, 1], [[1, 2], [3]]),
        # a, b, a: three segments, a named twice
        "split-owner": (sp, 1, [A, B], [0, 0], None, [0], [[A, B, A]]),
        # the zone's owner is named under both rack jobs
        "zone-owner": (zo, 1, [A], [0], None, [0, 1], [[A], [A]]),
        # the zone job: zone 1 is free (key 0); were it not, zone 0 counts A once
        "leaf-boundary": (lb, 1, [A], [0], None, [1], [[]]),
        "leaf-boundary-taken": (dataclasses.replace(lb, job_class=np.array([1, 0], dtype=np.uint32)), 1, [A], [0], None,
                                [2, 0], [[], [A]]),
        # the segment is counted in both racks
        "domain-boundary": (db, 1, [A], [0], None, [0, 1], [[A], [A]]),
        # owner ids 0 and INT32_MIN, ranks 0 and 65534, prio 65535
        "special": (si, 65535, [INT32_MIN, 0], [0, 65534], None, [1, 0], [[INT32_MIN], [0]]),
    }


# ---------------------------------------------------------------- sweep inputs
SWEEP_SEEDS = range(40)
SWEEP_PRIOS = (1, 2, 4)
FIRST_ID = 3000


def overlay(p, seed, p_upper=0.12, p_leaf=0.5, ranks=4, absent=0.15):
    """(problem with owners overlaid, owners, owner_prio, evict_free): level by
    level, coarse to fine, each domain that has rows and is not yet covered is
    picked with probability p_upper above the leaf level and p_leaf at it and
    gets a fresh id from FIRST_ID up on all its rows; each owner a rank uniform
    in 0..ranks-1; a share `absent` of them left out of the table; evict_free =
    max(free, 3/4 of the column's maximum)."""
    s = 91_000 + seed
    n = p.nodes
    ls = np.asarray(n.leaf_start, dtype=np.int64)
    excl = n.excl.copy()
    covered = np.zeros(n.n_nodes, dtype=bool)
    nxt = FIRST_ID
    K = p.topology.n_levels
    for k in range(K):
        fl = np.asarray(p.topology.first_leaf[k], dtype=np.int64)
        D = fl.shape[0] - 1
        pick = synth.bernoulli(s, 10 + k, D, p_leaf if k == K - 1 else p_upper)
        for d in range(D):
            r0, r1 = int(ls[fl[d]]), int(ls[fl[d + 1]])
            if not pick[d] or r0 == r1 or covered[r0:r1].any():
                continue
            excl[r0:r1] = nxt
            covered[r0:r1] = True
            nxt += 1
    n_own = nxt - FIRST_ID
    ids = np.arange(FIRST_ID, nxt, dtype=np.int32)
    rank = synth.uniform_int(s, 20, n_own, 0, ranks - 1).astype(np.uint32)
    keep = ~synth.bernoulli(s, 21, n_own, absent)
    top = n.free.max(axis=1, keepdims=True).astype(np.int64) if n.n_nodes else np.zeros((n.n_res, 1), dtype=np.int64)
    evict_free = np.maximum(n.free.astype(np.int64), top * 3 // 4).astype(np.uint32)
    nodes = Nodes(leaf_start=n.leaf_start, labels=n.labels, taints=n.taints, free=n.free, excl=excl,
                  leaf_begin=n.leaf_begin)
    return dataclasses.replace(p, nodes=nodes), ids[keep], rank[keep], evict_free


def sweep(seed):
    """(problem, owners, owner_prio, evict_free): gang_ref.sweep_case's problem
    with owners overlaid."""
    q, ids, rank, ef = overlay(sweep_case(seed)[0], seed)
    return dataclasses.replace(q, name=f"preempt-sweep-{seed}"), ids, rank, ef
