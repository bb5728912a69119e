"""The yardstick of the grow-placement tests (DESIGN.md §2 "Grow placement"):
the rule taken literally in int64 numpy and Python integers. It never calls
the engine.

cap / occ are oracle.tally_nodes on the snapshot, tcap is oracle.tally_nodes
on the templates as a snapshot of one row per leaf. A domain's plan sorts its
leaves by (-tcap, leaf) and walks them; the walk over the jobs is O(J D).
Also here: the candidate lists in the engine's layout (table_ref) and the
problems the CPU and the GPU tests share."""
import numpy as np

from jobset_amd.snapshot import JobClass, Templates
from oracle import oracle as O
from bind_ref import cls, nested

NONE = 0xFFFFFFFF
NO_LIMIT = 0xFFFFFFFF
GROUP_MAX = 512  # leaves of the largest domain the keys kernel's group form takes


def plan(tc, ma, rem):
    """One domain: (rem ends at 0, [(leaf index, n > 0)] in the rule's order)."""
    pairs = []
    for l in sorted(range(len(tc)), key=lambda l: (-int(tc[l]), l)):
        n = 0 if rem == 0 or tc[l] == 0 else min(int(ma[l]), -(-rem // int(tc[l])))
        if n:
            pairs.append((l, n))
        rem -= min(rem, n * int(tc[l]))
    return rem == 0, pairs


def domain_table(p, t):
    """Per class: reach bool [D], need int64 [D] (NONE: not covered), rec int64
    [D, 4] = (need, t*, q, leaves used), pairs: d -> [(leaf, n)] by leaf."""
    L = p.topology.n_leaves
    cap, occ = O.tally_nodes(L, p.nodes, p.classes)
    tcap = O.tally_nodes(L, t.as_nodes(), p.classes)[0]
    out = []
    for c, jc in enumerate(p.classes):
        fl = np.asarray(p.topology.first_leaf[jc.level], dtype=np.int64)
        D = fl.shape[0] - 1
        reach, need, rec, pairs = np.zeros(D, dtype=bool), np.zeros(D, dtype=np.int64), np.zeros((D, 4), dtype=np.int64), {}
        for d in range(D):
            a, b = int(fl[d]), int(fl[d + 1])
            capsum = int(cap[c, a:b].astype(np.int64).sum())
            ok, pr = plan(tcap[c, a:b], t.max_add[a:b], jc.pods - min(capsum, jc.pods))
            if not ok:
                need[d], rec[d] = NONE, (NONE, 0, 0, 0)
                continue
            need[d] = sum(n for _, n in pr)
            if pr:  # t*: the finishing leaf's tcap; q: the nodes of the leaves tied there
                ts = int(tcap[c, a + pr[-1][0]])
                rec[d] = (need[d], ts, sum(n for l, n in pr if tcap[c, a + l] == ts), len(pr))
            reach[d] = int(occ[a:b].astype(np.int64).sum()) == 0
            pairs[d] = sorted((a + l, n) for l, n in pr)
        out.append((reach, need, rec, pairs))
    return out


def table_ref(p, t, tab=None):
    """(order, nf, need, rec) as jspb_grow_table lays them out."""
    tab = tab or domain_table(p, t)
    order, nf = [], []
    for reach, need, _, _ in tab:
        ds = sorted(np.flatnonzero(reach).tolist(), key=lambda d: (int(need[d]), d))
        order += ds + [0xFFFFFFFF] * (reach.shape[0] - len(ds))
        nf.append(len(ds))
    return (np.array(order, dtype=np.uint32), np.array(nf, dtype=np.uint32),
            np.concatenate([x[1] for x in tab]).astype(np.uint32), np.concatenate([x[2] for x in tab]).astype(np.uint32))


def grow_ref(p, t, budget=NO_LIMIT, tab=None):
    """(assign int32 [J], need uint32 [J], plan_off uint32 [J + 1], plan_leaf,
    plan_nodes uint32 [total], stats dict) for the jobs p.job_class in global order."""
    tab = tab or domain_table(p, t)
    topo = p.topology
    fl = [np.asarray(f, dtype=np.int64) for f in topo.first_leaf]
    J = p.n_jobs
    assign, need_out = np.full(J, -1, dtype=np.int32), np.zeros(J, dtype=np.uint32)
    used = np.zeros(topo.n_leaves, dtype=bool)
    taken = [set() for _ in fl]
    off, leaf, nodes = [0], [], []
    left = None if budget == NO_LIMIT else int(budget)
    st = dict(jobs=J, placed=0, grown=0, over_budget=0, nodes=0)
    for j in range(J):
        c = int(p.job_class[j])
        k = p.classes[c].level
        reach, need, _, pairs = tab[c]
        best = None
        for d in np.flatnonzero(reach).tolist():
            if d in taken[k] or used[fl[k][d]:fl[k][d + 1]].any():
                continue
            if best is None or (int(need[d]), d) < (int(need[best]), best):
                best = d
        if best is not None and left is not None and int(need[best]) > left:
            st["over_budget"] += 1
        elif best is not None:
            n = int(need[best])
            left = None if left is None else left - n
            assign[j], need_out[j] = best, n
            taken[k].add(best)
            used[fl[k][best]:fl[k][best + 1]] = True
            leaf += [l for l, _ in pairs[best]]
            nodes += [m for _, m in pairs[best]]
            st["placed"] += 1
            st["grown"] += n > 0
            st["nodes"] += n
        off.append(len(leaf))
    return (assign, need_out, np.array(off, dtype=np.uint32), np.array(leaf, dtype=np.uint32),
            np.array(nodes, dtype=np.uint32), st)


def stats_dict(st):
    return dict(jobs=int(st.jobs), placed=int(st.placed), grown=int(st.grown), over_budget=int(st.over_budget),
                nodes=int(st.nodes))


# ---- the problems
# Leaves per level-0 domain. The keys kernel's form is chosen per class by its
# largest domain m: the group form with the smallest shift such that
# 8 << shift >= m while m <= GROUP_MAX, the block form above. So the level-0
# classes of these lists run with 1, 8, 16 and 64 lanes per domain (63 and 64
# leaves fill shift 3 to its last register, 65 is one past it, 512 fills shift
# 6) and, one leaf past the register limit, in the block form. Domains 0 and 1
# are the ones two classes cover exactly; the last domain is occupied.
SHAPES = {"shift0": [8, 7, 1, 2, 3], "shift3": [64, 63, 9, 3], "shift4": [65, 64, 63, 1, 2, 3],
          "shift6": [GROUP_MAX, 100, 3], "block": [GROUP_MAX + 1, GROUP_MAX, 3]}


def templates(L, free, max_add, labels=None, taints=None):
    return Templates(labels=np.ones((1, L), dtype=np.uint64) if labels is None else np.asarray(labels, dtype=np.uint64).reshape(1, L),
                     taints=np.zeros(L, dtype=np.uint32) if taints is None else np.asarray(taints, dtype=np.uint32),
                     free=np.asarray(free, dtype=np.uint32).reshape(1, L), max_add=np.asarray(max_add, dtype=np.uint32))


def shapes_case(shape, seed=0):
    """Two levels: domains of SHAPES[shape] leaves over leaves of 0 (a pool scaled to
    zero), 1 or 2 rows with one free unit each. Template capacities 0..7 with
    many ties, max_add 0..4; templates that fail by a taint on bit 31, by the
    selector, and that pass only because label word 1 is past W. Classes at
    level 0 with small, middling and large deficits, two whose deficit
    domains 0 and 1 cover exactly and two one pod short of that, a
    contradictory selector, and a leaf-level class that competes with
    them. Returns (problem, templates)."""
    rng = np.random.default_rng(seed)
    fl0 = np.concatenate([[0], np.cumsum(SHAPES[shape])])
    L = int(fl0[-1])
    rows = rng.integers(0, 3, L)
    rows[fl0[:-1]] = 0  # every domain starts on a leaf without rows
    occ_leaf = int(fl0[-2]) + 1
    rows[occ_leaf] = 1
    excl = np.full(int(rows.sum()), -1)
    excl[int(rows[:occ_leaf].sum())] = 9  # the last domain would grow, but a row of it is owned
    free_t = rng.choice([0, 1, 2, 3, 3, 7, 7, 7], L)
    add = rng.choice([0, 1, 2, 4], L)
    taints = np.where(rng.random(L) < 0.1, 1 << 31, 0)
    labels = np.where(rng.random(L) < 0.1, 2, 1)  # bit 0 missing: the selector fails
    t = templates(L, free_t, add, labels, taints)
    eff = np.where((taints == 0) & (labels == 1), free_t, 0)

    def exact(dom):  # capsum + everything the domain can add, for a class that clamps nothing
        a, b = int(fl0[dom]), int(fl0[dom + 1])
        return int(rows[a:b].sum() + (eff[a:b] * add[a:b]).sum())
    classes = [cls(0, 5), cls(0, 40), cls(0, 300), cls(0, exact(0)), cls(0, exact(0) + 1), cls(0, exact(1)),
               cls(0, exact(1) + 1), JobClass(req_labels=(1,), forbid_labels=(1,), level=0, pods=3, req_res=(1,)),
               JobClass(req_labels=(1, 0xFF), level=0, pods=7, req_res=(1,)), cls(1, 6)]
    jobs = [5, 3, 2, 1, 9, 0, 9, 8, 9, 4, 6, 7, 9, 0, 1, 9]  # the wide classes first, then the leaves compete
    return nested([fl0, np.arange(L + 1)], rows, classes, jobs, excl=excl), t


def wide_case():
    """The wide edges at the largest pods jsp_classes_upload takes, 2^22 (a
    class with more is refused there, so 0xFFFFFFFF cannot reach the call):
    tcap = max_add = 65536, whose product 2^32 saturates at pods (leaves 0 and
    1: need 64); a leaf one node short (leaf 2: 65 nodes of 65535 against
    max_add 64); need == max_add exactly (leaf 3: 63); and a request of zero,
    where tcap = pods and an empty leaf needs one node. Four leaves in two
    level-0 domains; leaf 0 has no rows, the others one."""
    P = 1 << 22
    p = nested([[0, 2, 4], np.arange(5)], [0, 1, 1, 1], [cls(0, P), cls(1, P), cls(0, P, req=0), cls(1, P, req=0)],
               [1, 3, 1, 3, 0, 2, 1], free=[1, 1, 65536])
    return p, templates(4, [65536, 65536, 65535, 65536], [65536, 65536, 64, 63])


CASES = dict({k: (lambda k=k: shapes_case(k)) for k in SHAPES}, wide=wide_case)
