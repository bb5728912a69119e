"""The yardstick of the what-if placement tests (DESIGN.md §2 "What-if
placement"): the rule taken literally. It never calls the engine.

A scenario is a dict {"rows": [n], and any of "labels" [W, n], "taints" [n],
"free_res" [R, n], "excl_owner" [n]} -- Engine.place_whatif's form. For each
scenario the Problem's node columns are copied in numpy, the delta is written
as jsp_snapshot_patch would write it, and the CPU oracle (oracle.place_c)
places the jobs on the copy. flips comes from oracle.tally_nodes plus the
feasibility restatement of tests/gang_ref.py (the one tests/fit_ref.py uses),
computed on the base columns and on the edited ones.

Also here: the hand cases and the seeded sweep generator, shared by the CPU
tests, which assert the coverage floors on this reference's own output, and
the GPU tests, which compare the engine with it."""
import dataclasses

import numpy as np

from jobset_amd import synth
from jobset_amd.snapshot import Nodes
from oracle import oracle as O
from bind_ref import cls, flat, nested
from gang_ref import feasibility, sweep_case

COLUMNS = ("labels", "taints", "free_res", "excl_owner")


def patched(p, sc):
    """Problem p with scenario sc's rows overwritten (a copy; p is unchanged)."""
    n = p.nodes
    labels, taints, free, excl = n.labels.copy(), n.taints.copy(), n.free.copy(), n.excl.copy()
    rows = np.asarray(sc.get("rows", ()), dtype=np.int64).reshape(-1)
    if rows.size:
        assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n.n_nodes
        if sc.get("labels") is not None:
            labels[:, rows] = np.asarray(sc["labels"], dtype=np.uint64).reshape(labels.shape[0], rows.size)
        if sc.get("taints") is not None:
            taints[rows] = np.asarray(sc["taints"], dtype=np.uint32)
        if sc.get("free_res") is not None:
            free[:, rows] = np.asarray(sc["free_res"], dtype=np.uint32).reshape(free.shape[0], rows.size)
        if sc.get("excl_owner") is not None:
            excl[rows] = np.asarray(sc["excl_owner"], dtype=np.int32)
    nodes = Nodes(leaf_start=n.leaf_start, labels=labels, taints=taints, free=free, excl=excl, leaf_begin=n.leaf_begin)
    return dataclasses.replace(p, nodes=nodes)


def feas_of(p):
    """feas[c]: bool [D[level[c]]] of problem p's own columns."""
    cap, occ = O.tally_nodes(p.topology.n_leaves, p.nodes, p.classes)
    return feasibility(p, cap, occ)


def whatif_ref(p, scenarios):
    """(assign int32 [S, J], placed [S], flips, opened [S], closed [S]): per
    scenario the oracle's placement on the patched copy; flips the (scenario,
    class, domain) bits that differ from the unedited snapshot's, opened /
    closed the scenario's bits that went infeasible -> feasible / back."""
    base = feas_of(p)
    S, J = len(scenarios), p.n_jobs
    assign = np.full((S, J), -1, dtype=np.int32)
    placed = np.zeros(S, dtype=np.uint32)
    opened = np.zeros(S, dtype=np.int64)
    closed = np.zeros(S, dtype=np.int64)
    for s, sc in enumerate(scenarios):
        q = patched(p, sc)
        assign[s] = O.place_c(q)[0]
        placed[s] = int((assign[s] >= 0).sum())
        for b, f in zip(base, feas_of(q)):
            opened[s] += int((~b & f).sum())
            closed[s] += int((b & ~f).sum())
    return assign, placed, int(opened.sum() + closed.sum()), opened, closed


def concat(scenarios):
    """(scen_off, rows, labels, taints, free_res, excl_owner) for
    Engine.place_whatif_runs; a column is None when no scenario carries it."""
    rows = [np.asarray(sc.get("rows", ()), dtype=np.uint32).reshape(-1) for sc in scenarios]
    so = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.uint32)
    out = []
    for name, axis in (("labels", 1), ("taints", 0), ("free_res", 1), ("excl_owner", 0)):
        parts = [np.asarray(sc[name]) for sc, r in zip(scenarios, rows) if r.shape[0] and sc.get(name) is not None]
        out.append(np.concatenate(parts, axis=axis) if parts else None)
    return (so, np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint32), *out)


def edit(p, rows, **cols):
    """A scenario over `rows` carrying all four columns: the resident values
    except where cols (labels / taints / free_res / excl_owner) gives others."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    n = p.nodes
    sc = {"rows": rows.astype(np.uint32), "labels": n.labels[:, rows].copy(), "taints": n.taints[rows].copy(),
          "free_res": n.free[:, rows].copy(), "excl_owner": n.excl[rows].copy()}
    for k, v in cols.items():
        assert k in COLUMNS
        sc[k] = np.asarray(v, dtype=sc[k].dtype).reshape(sc[k].shape)
    return sc


def only(sc, *names):
    """Scenario sc with the named columns alone."""
    return {"rows": sc["rows"], **{k: sc[k] for k in names}}


EMPTY = {"rows": np.zeros(0, dtype=np.uint32)}


# ---- hand cases: name -> (problem, scenarios, assign per scenario, flips)
def hand_cases():
    # two zones of two racks of two rows; a zone job (4 pods) then two rack jobs (2 pods)
    a = nested([[0, 2, 4], np.arange(5)], [2, 2, 2, 2], [cls(1, 2), cls(0, 4)], [1, 0, 0])
    # rack 0 owned and without room, rack 1 free: two rack jobs
    b = flat([2, 2], [cls(0, 2)], [0, 0], excl=[7, -1, -1, -1], free=[0, 1, 1, 1])
    # rack 0 holds exactly the 3 pods, rack 1 only 2
    c = flat([3, 2], [cls(0, 3)], [0, 0])
    d = flat([3, 3], [cls(0, 5)], [0])
    return {
        # an owner written onto row 0 closes rack 0 and the zone above it: the zone job moves to zone 1,
        # one rack job fits beside it in rack 1
        "close": (a, [EMPTY, only(edit(a, [0], excl_owner=[5]), "excl_owner")], [[0, 2, 3], [1, 1, -1]], 2),
        # the owner cleared and the free unit given back opens rack 0
        "open": (b, [only(edit(b, [0], free_res=[[1]], excl_owner=[-1]), "free_res", "excl_owner"), EMPTY],
                 [[0, 1], [1, -1]], 1),
        # one edit takes a pod away and closes rack 0; with a second one that gives it back the bit stays
        "flipback": (c, [only(edit(c, [0], free_res=[[0]]), "free_res"),
                         only(edit(c, [0, 1], free_res=[[0, 2]]), "free_res")],
                     [[-1, -1], [0, -1]], 1),
        # 5 pods, racks of 3: neither of two edits opens rack 1 alone, their sum does
        "sum": (d, [only(edit(d, [3], free_res=[[2]]), "free_res"), only(edit(d, [4], free_res=[[2]]), "free_res"),
                    only(edit(d, [3, 4], free_res=[[2, 2]]), "free_res")],
                [[-1], [-1], [1]], 1),
    }


# ---------------------------------------------------------------- sweep inputs
SWEEP_SEEDS = range(24)
SWEEP_SCENARIOS = 6


def _rows_of(p, level, d):
    ls = np.asarray(p.nodes.leaf_start, dtype=np.int64)
    fl = np.asarray(p.topology.first_leaf[level], dtype=np.int64)
    return np.arange(ls[fl[d]], ls[fl[d + 1]])


def _boost(p, rows):
    """rows without owner or taint and with every resource at its column's maximum"""
    return edit(p, rows, excl_owner=np.full(rows.size, -1), taints=np.zeros(rows.size),
                free_res=np.repeat(p.nodes.free.max(axis=1, keepdims=True), rows.size, axis=1))


def sweep(seed):
    """(problem, scenarios): gang_ref.sweep_case's problem (random topology,
    nodes and occupancy, permissive classes) and SWEEP_SCENARIOS scenarios, all
    carrying the four columns. The generator aims them with the oracle's
    answer on the unedited problem:
      0 an owner written onto one row of the domain the first placed job took;
      1 one foreign owner's rows vacated and boosted (no owner, no taint, every
        resource at its column's maximum); without an owner, a random leaf's;
      2 8-40 random rows with random values in every column;
      3 no rows;
      4 the rows of the largest infeasible, unoccupied (class, domain) boosted;
        where every one is feasible or occupied, those of domain 0 of class 0;
      5 the rows of the last placed job's domain drained of every resource
        (without a placed job: a random leaf's)."""
    p = sweep_case(seed)[0]
    n = p.nodes
    N = n.n_nodes
    s = 55_000 + seed
    u = lambda stream, lo, hi: int(synth.uniform_int(s, stream, 1, lo, hi)[0])  # noqa: E731
    ls = np.asarray(n.leaf_start, dtype=np.int64)
    nz = np.nonzero(np.diff(ls) > 0)[0]
    base, cap, occ = O.place_c(p)
    level = lambda j: p.classes[int(p.job_class[j])].level  # noqa: E731
    jp = np.nonzero(base >= 0)[0]
    out = []
    # 0
    rows = _rows_of(p, level(jp[0]), base[jp[0]]) if jp.size else np.arange(N)
    out.append(edit(p, [int(rows[u(1, 0, rows.size - 1)])], excl_owner=[900 + seed]))
    # 1
    owned = np.nonzero(n.excl != -1)[0]
    if owned.size:
        rows = np.nonzero(n.excl == n.excl[owned[u(2, 0, owned.size - 1)]])[0]
    else:
        leaf = int(nz[u(2, 0, nz.size - 1)])
        rows = np.arange(ls[leaf], ls[leaf + 1])
    out.append(_boost(p, rows))
    # 2
    k = min(N, u(3, 8, 40))
    rows = np.sort(synth.permutation(s, 4, N)[:k])
    W, R = n.n_label_words, n.n_res
    lab = np.stack([synth.draws(s, 10 + w, k) | synth.draws(s, 14 + w, k) for w in range(W)])
    fr = np.stack([synth.uniform_int(s, 20 + r, k, 0, int(n.free[r].max())) for r in range(R)])
    tn = np.where(synth.bernoulli(s, 30, k, 0.3), synth.uniform_int(s, 31, k, 0, 0xFFFF), 0)
    ex = np.where(synth.bernoulli(s, 32, k, 0.2), 700, -1)
    out.append(edit(p, rows, labels=lab, taints=tn, free_res=fr, excl_owner=ex))
    # 3
    out.append(EMPTY)
    # 4
    best = _rows_of(p, p.classes[0].level, 0)
    most = -1
    occ_cs = np.concatenate([[0], np.cumsum(occ.astype(np.int64))])
    for c, f in enumerate(feasibility(p, cap, occ)):
        fl = np.asarray(p.topology.first_leaf[p.classes[c].level], dtype=np.int64)
        for d in np.nonzero(~f & ((occ_cs[fl[1:]] - occ_cs[fl[:-1]]) == 0))[0]:
            rows = _rows_of(p, p.classes[c].level, int(d))
            if rows.size > most:
                best, most = rows, rows.size
    out.append(_boost(p, best))
    # 5
    if jp.size:
        rows = _rows_of(p, level(jp[-1]), base[jp[-1]])
    else:
        leaf = int(nz[u(5, 0, nz.size - 1)])
        rows = np.arange(ls[leaf], ls[leaf + 1])
    out.append(edit(p, rows, free_res=np.zeros((R, rows.size))))
    assert len(out) == SWEEP_SCENARIOS
    return p, out
