"""The yardstick of the spread pod-binding tests (DESIGN.md §2 "Spread pod binding"): the rule in int64
numpy on bind_ref's row_caps / leaf_range and bind_even_ref's water-filling. It never calls the engine."""
import numpy as np

from bind_ref import bind_ref, leaf_range, row_caps
from bind_even_ref import even_takes


def group_rows(p, level, d, s):
    """[(row0, row1)] of the level-s domains inside domain d of `level`, in id order."""
    fl, ls = p.topology.first_leaf[s], p.nodes.leaf_start
    l0, l1 = leaf_range(p, level, d)
    g0, g1 = (int(np.searchsorted(fl, x, side="left")) for x in (l0, l1))
    return [(int(ls[int(fl[g])]), int(ls[int(fl[g + 1])])) for g in range(g0, g1)]


def group_caps(p, c, d, s):
    """(G int64 [groups], the groups' rows, cap [N]) for class c on its domain d."""
    cap = row_caps(p, c)[0]
    rows = group_rows(p, p.classes[c].level, d, s)
    return np.array([min(p.classes[c].pods, int(cap[a:b].sum())) for a, b in rows], dtype=np.int64), rows, cap


def bind_spread_ref(p, assign, s):
    """(pod_row, pod_off, level uint32 [J], stats dict). bind_ref raises for the refusals and decides
    pod_off and bound / stale; a bound job's pods are then laid out group by group by the groups' takes."""
    pod_row, pod_off, st = bind_ref(p, assign)
    level = np.zeros(p.n_jobs, dtype=np.uint32)
    used = groups = most = 0
    for j in range(p.n_jobs):
        o0, o1 = int(pod_off[j]), int(pod_off[j + 1])
        if assign[j] < 0 or o1 == o0 or pod_row[o0] < 0:
            continue
        G, rows, cap = group_caps(p, int(p.job_class[j]), int(assign[j]), s)
        take, level[j], _ = even_takes(G, o1 - o0)
        out = []
        for (a, b), t in zip(rows, take):  # first fit by row inside the group
            out.append(a + np.searchsorted(np.cumsum(cap[a:b]), np.arange(int(t), dtype=np.int64), side="right"))
        pod_row[o0:o1] = np.concatenate(out)
        used += np.unique(pod_row[o0:o1]).shape[0]
        groups += int((take > 0).sum())
        most = max(most, int(take.max()))
    return pod_row, pod_off, level, dict(st, rows_used=used, groups_used=groups, max_per_group=most)


def spread_stats_dict(st):
    return {k: int(getattr(st, k)) for k in ("jobs", "bound", "stale", "rows_used", "pods", "pods_bound", "groups_used",
                                             "max_per_group")}
