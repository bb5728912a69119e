"""The yardstick of the assume / forget tests (DESIGN.md §2 "Assume and
forget"): the two rules restated in plain numpy on tests/bind_ref.py's helpers.
It never calls the engine."""
import dataclasses

import numpy as np

from bind_ref import BindConflict, domain_rows, first_conflict, row_caps  # noqa: F401  (BindConflict: re-exported)


def assume_ref(p, assign, owner):
    """(new_excl int32 [N], committed bool [J], stats dict) of jsp_assume for
    problem p (jobs p.job_class in global order), assign[J] and owner[J].
    Raises BindConflict for intersecting domains (the lowest job an earlier one
    intersects), ValueError for a domain out of range or an owner of -1."""
    assign = np.asarray(assign, dtype=np.int64)
    owner = np.asarray(owner, dtype=np.int64)
    J = p.n_jobs
    assert assign.shape == (J,) and owner.shape == (J,)
    for j in range(J):
        lvl = p.classes[int(p.job_class[j])].level
        if assign[j] < -1 or assign[j] >= p.topology.n_domains[lvl]:
            raise ValueError(f"job {j}: domain {assign[j]} out of range")
        if assign[j] >= 0 and owner[j] == -1:
            raise ValueError(f"job {j}: owner -1")
    bad = first_conflict(p, assign)
    if bad is not None:
        raise BindConflict(bad)
    old = p.nodes.excl
    new = old.copy()
    occupied = old != -1          # every job is judged on the snapshot as it was: domains are disjoint
    committed = np.zeros(J, dtype=bool)
    caps = {}
    stale = rows_marked = 0
    for j in range(J):
        if assign[j] < 0:
            continue
        c = int(p.job_class[j])
        if c not in caps:
            caps[c] = row_caps(p, c)[0]
        r0, r1 = domain_rows(p, p.classes[c].level, int(assign[j]))
        if int(caps[c][r0:r1].sum()) < p.classes[c].pods or occupied[r0:r1].any():
            stale += 1
            continue
        new[r0:r1] = np.int32(owner[j])
        committed[j] = True
        rows_marked += r1 - r0
    stats = dict(jobs=J, committed=int(committed.sum()), stale=stale, reserved=0, rows_marked=int(rows_marked))
    return new, committed, stats


def forget_ref(excl, owners):
    """(new_excl, cleared) of jsp_forget: rows whose owner is in owners get -1."""
    excl = np.asarray(excl, dtype=np.int32)
    hit = np.isin(excl, np.asarray(owners, dtype=np.int32).reshape(-1)) & (excl != -1)
    new = excl.copy()
    new[hit] = -1
    return new, int(hit.sum())


def with_excl(p, excl):
    """Problem p on another excl column (p itself is left as it is)."""
    return dataclasses.replace(p, nodes=dataclasses.replace(p.nodes, excl=np.asarray(excl, dtype=np.int32)))


def stats_dict(st):
    return dict(jobs=int(st.jobs), committed=int(st.committed), stale=int(st.stale), reserved=int(st.reserved),
                rows_marked=int(st.rows_marked))


def domains_intersect(p, job_class_a, assign_a, job_class_b, assign_b):
    """Pairs (i, j): placed job i of batch a and placed job j of batch b whose domains' row ranges intersect."""
    out = []
    for i, d in enumerate(np.asarray(assign_a).tolist()):
        if d < 0:
            continue
        a0, a1 = domain_rows(p, p.classes[int(job_class_a[i])].level, d)
        for j, e in enumerate(np.asarray(assign_b).tolist()):
            if e < 0:
                continue
            b0, b1 = domain_rows(p, p.classes[int(job_class_b[j])].level, e)
            if max(a0, b0) < min(a1, b1):
                out.append((i, j))
    return out
