"""The host mirror's preemptive planning (planner.preempt) on a cluster of
Node objects built as the planner.whatIf tests build theirs: the reply's
domains and victims equal the rule taken literally (tests/preempt_ref.py) on
the planner's own columns, with the table the planner derives from the pods'
spec.priority; a job at or above the request's priority blocks; the ledger's
entries (planner.assume) carry no priority and block; nothing is written; the
request errors name what is wrong."""
import numpy as np
import pytest

from jobset_amd import host, synth

import k8s_fixtures as K
from preempt_ref import preempt_ref
from test_sticky_host_gpu import EXCL, RES, cluster, planned
from test_whatif_host_gpu import PLAN_KEYS, RACKS, domains, key_of

pytestmark = pytest.mark.gpu

# job name -> (its rack's nodes, spec.priority or None)
FOREIGN = {"low-a-0": ("z0-r0", 10), "low-b-0": ("z0-r1", 5), "high-0": ("z0-r2", 100), "nop-0": ("z0-r3", None)}


def foreign_pod(job_name, i, node_name, priority):
    """A running pod of another JobSet's rack-exclusive job on node_name."""
    spec = {"nodeName": node_name,
            "containers": [{"name": "train", "resources": {"requests": {"amd.com/gpu": "8"}}}]}
    if priority is not None:
        spec["priority"] = priority
    return {"metadata": {"name": f"{job_name}-{i}-abcde", "namespace": "default",
                         "labels": {K.JOBKEY: key_of(job_name)}, "annotations": {EXCL: "rack"}},
            "spec": spec, "status": {"phase": "Running"}}


def held_cluster():
    c, js, jobs = cluster()
    for name, (rack, prio) in FOREIGN.items():
        for i in range(4):
            c.add_pod(foreign_pod(name, i, f"{rack}-n{i}", prio))
    return c, js, jobs


def preempt(c, jobs, priority):
    r, e = c.preempt(jobs, priority)
    assert e is None, e
    assert set(r) == PLAN_KEYS | {"evict"}
    assert all(set(j) == {"name", "topologyKey", "domainId", "domain", "victims"} for j in r["jobs"])
    assert r["evict"] == sorted({k for j in r["jobs"] for k in j["victims"]})
    assert r["placed"] == sum(j["domain"] is not None for j in r["jobs"])
    return r


def reference(c, plan, priority):
    """preempt_ref on the planner's columns: the table from FOREIGN as the
    planner derives it (candidates below `priority`, ranks their distinct
    priorities in ascending order, prio the number of ranks), evict_free the
    free column with the candidates' rows as a node nobody uses."""
    cols = c.planner_columns()
    q = K.problem_from_planner(synth.config1(), cols, plan)
    row = {n: i for i, n in enumerate(cols["rows"])}
    cand = {n: (rack, pr or 0) for n, (rack, pr) in FOREIGN.items() if (pr or 0) < priority}
    ranks = sorted({pr for _, pr in cand.values()})
    ids, rk, id_key = [], [], {}
    ef = q.nodes.free.copy()
    unused = ef[:, row["z1-r3-n3"]].copy()
    for n, (rack, pr) in cand.items():
        rows = [row[f"{rack}-n{i}"] for i in range(4)]
        owner = {int(q.nodes.excl[i]) for i in rows}
        assert len(owner) == 1 and -1 not in owner
        ids.append(owner.pop())
        rk.append(ranks.index(pr))
        id_key[ids[-1]] = key_of(n)
        ef[:, rows] = unused[:, None]
    a, off, v, st = preempt_ref(q, len(ranks), ids, rk, ef if ids else None)
    vals = cols["domainValues"]
    doms = [None if d < 0 else vals[q.classes[int(q.job_class[j])].level][d] for j, d in enumerate(a.tolist())]
    vics = [[id_key[int(x)] for x in v[off[j]:off[j + 1]]] for j in range(q.n_jobs)]
    return doms, vics


@pytest.mark.parametrize("priority", [50, 1000, 10, 0, -5])
def test_preempt_equals_the_reference(engine, priority):
    c, js, jobs = held_cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    before = planned(c, jobs)
    assert domains(before) == ["zone-1-rack-0", "zone-1-rack-1", "zone-1-rack-2", "zone-1-rack-3", None]
    r = preempt(c, jobs, priority)
    doms, vics = reference(c, before, priority)
    assert domains(r) == doms
    assert [j["victims"] for j in r["jobs"]] == vics
    if priority == 50:     # the job without a priority counts as 0: the cheapest victim; high-0 blocks
        assert doms[4] == "zone-0-rack-3" and r["evict"] == [key_of("nop-0")]
    if priority == 10:     # low-a-0's 10 is not below 10
        assert doms[4] == "zone-0-rack-3"
    if priority <= 0:      # nobody is below: planner.plan's answer
        assert domains(r) == domains(before) and r["evict"] == []
    # nothing was written: planner.plan on this cache is what it was before
    after = planned(c, jobs)
    assert set(after) == PLAN_KEYS and domains(after) == domains(before)
    assert after["snapshot"]["upload"] == "none"


def test_more_jobs_than_free_racks(engine):
    """Eight rack jobs at priority 50: the four free racks, then the victims by
    ascending priority; high-0's rack stays."""
    c, js, _ = held_cluster()
    js["spec"]["replicatedJobs"][0]["replicas"] = 8
    jobs = host.constructJobsFromTemplate(js, js["spec"]["replicatedJobs"][0], {})
    c.planner_new(engine, ["zone", "rack"], RES)
    before = planned(c, jobs)
    r = preempt(c, jobs, 50)
    doms, vics = reference(c, before, 50)
    assert domains(r) == doms == ["zone-1-rack-0", "zone-1-rack-1", "zone-1-rack-2", "zone-1-rack-3",
                                   "zone-0-rack-3", "zone-0-rack-1", "zone-0-rack-0", None]
    assert [j["victims"] for j in r["jobs"]] == vics
    assert r["evict"] == sorted(key_of(n) for n in ("nop-0", "low-b-0", "low-a-0"))


def test_ledger_entries_block(engine):
    """The first JobSet's five racks are held by the ledger alone: no priority
    evicts them."""
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan0 = planned(c, jobs)
    assert domains(plan0) == RACKS
    r, e = c.assume(jobs, plan0)
    assert e is None and r["committed"] == 5
    before = planned(c, jobs)
    assert domains(before) == ["zone-1-rack-1", "zone-1-rack-2", "zone-1-rack-3", None, None]
    r = preempt(c, jobs, 2 ** 31 - 1)
    assert domains(r) == domains(before) and r["evict"] == [] and all(j["victims"] == [] for j in r["jobs"])
    assert domains(planned(c, jobs)) == domains(before)


def test_refusals(engine):
    c, js, jobs = held_cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    before = planned(c, jobs)
    for bad in (None, "high", 2 ** 31, [3]):
        r, e = c.preempt(jobs, bad)
        assert (r is None or not r) and "priority must be an integer" in e, e
    r, e = host.Cache().preempt(jobs, 5)
    assert "no placement planner" in e, e
    assert domains(planned(c, jobs)) == domains(before)
    preempt(c, jobs, 50)
