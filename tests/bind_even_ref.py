"""The yardstick of the even pod-binding tests (DESIGN.md §2 "Even pod binding"): the rule in int64
numpy on bind_ref's row_caps, domain_rows and first_conflict. It never calls the engine."""
import numpy as np

from bind_ref import bind_ref, domain_rows, row_caps


def even_takes(cap, pods):
    """(take int64 [n], L, rem) for the capacities of a feasible domain's rows."""
    cap = np.asarray(cap, dtype=np.int64)

    def A(level):
        return int(np.minimum(cap, level).sum())
    assert A(pods) >= pods >= 1
    lo, hi = 1, int(pods)
    while lo < hi:  # the smallest L with A(L) >= pods (A is monotone)
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if A(mid) >= pods else (mid + 1, hi)
    rem = int(pods) - A(lo - 1)
    high = cap >= lo
    take = np.minimum(cap, lo - 1) + (high & (np.cumsum(high) <= rem))
    assert int(take.sum()) == pods and 1 <= rem <= int(high.sum())
    return take, lo, rem


def bind_even_ref(p, assign):
    """(pod_row, pod_off, level uint32 [J], stats dict). bind_ref raises for the refusals and decides
    pod_off and bound / stale; a bound job's rows are then laid out again by its takes."""
    pod_row, pod_off, st = bind_ref(p, assign)
    level = np.zeros(p.n_jobs, dtype=np.uint32)
    used = most = 0
    for j in range(p.n_jobs):
        o0, o1 = int(pod_off[j]), int(pod_off[j + 1])
        if assign[j] < 0 or o1 == o0 or pod_row[o0] < 0:
            continue
        c = int(p.job_class[j])
        r0, r1 = domain_rows(p, p.classes[c].level, int(assign[j]))
        take, level[j], _ = even_takes(row_caps(p, c)[0][r0:r1], o1 - o0)
        pod_row[o0:o1] = r0 + np.searchsorted(np.cumsum(take), np.arange(o1 - o0, dtype=np.int64), side="right")
        used += int((take > 0).sum())
        most = max(most, int(take.max()))
    return pod_row, pod_off, level, dict(st, rows_used=used, max_per_row=most)


def even_stats_dict(st):
    return {k: int(getattr(st, k)) for k in ("jobs", "bound", "stale", "rows_used", "pods", "pods_bound", "max_per_row")}
