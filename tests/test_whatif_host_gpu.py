"""The host mirror's what-if planning (planner.whatIf) on a cluster of Node
objects: a scenario that evicts a job equals planner.plan on a second cache
built without that job (domain names compared) -- for a confirmed exclusive
job, whose pods the informer shows, and for an assumed one, which only the
planner's ledger holds; planner.plan on the first cache is what it was before;
the reply's key set is pinned; an unknown job key is refused by name."""
import pytest

from jobset_amd import host

import k8s_fixtures as K
from test_sticky_host_gpu import EXCL, RES, cluster, planned

pytestmark = pytest.mark.gpu

RACKS = ["zone-0-rack-0", "zone-0-rack-1", "zone-0-rack-2", "zone-0-rack-3", "zone-1-rack-0"]
PLAN_KEYS = {"jobs", "unplaceable", "placed", "snapshot", "classes", "jobClass"}


def domains(plan):
    return [j["domain"] for j in plan["jobs"]]


def key_of(name):
    return host.jobHashKey("default", name)


def foreign_pod(job_name, i, node_name):
    """A running pod of another JobSet's rack-exclusive job on node_name."""
    return {"metadata": {"name": f"{job_name}-{i}-abcde", "namespace": "default",
                         "labels": {K.JOBKEY: key_of(job_name)}, "annotations": {EXCL: "rack"}},
            "spec": {"nodeName": node_name,
                     "containers": [{"name": "train", "resources": {"requests": {"amd.com/gpu": "8"}}}]},
            "status": {"phase": "Running"}}


def what_if(c, jobs, scenarios):
    r, e = c.whatIf(jobs, scenarios)
    assert e is None, e
    assert set(r) == PLAN_KEYS | {"scenarios"}
    assert [s["name"] for s in r["scenarios"]] == [s["name"] for s in scenarios]
    for s in r["scenarios"]:
        assert set(s) == {"name", "jobs", "placed", "unplaceable", "flips", "rows"}
        assert all(set(j) == {"name", "topologyKey", "domainId", "domain"} for j in s["jobs"])
        assert s["placed"] == sum(j["domain"] is not None for j in s["jobs"])
        assert s["unplaceable"] == [j["name"] for j in s["jobs"] if j["domain"] is None]
    return r


def test_evicting_a_confirmed_job(engine):
    """Two foreign jobs hold racks zone-0-rack-0 and zone-0-rack-2 (their pods
    are bound there and use the GPUs)."""
    c, js, jobs = cluster()
    for i in range(4):
        c.add_pod(foreign_pod("old-a-0", i, f"z0-r0-n{i}"))
        c.add_pod(foreign_pod("old-b-0", i, f"z0-r2-n{i}"))
    c.planner_new(engine, ["zone", "rack"], RES)
    before = planned(c, jobs)
    assert domains(before) == ["zone-0-rack-1", "zone-0-rack-3", "zone-1-rack-0", "zone-1-rack-1", "zone-1-rack-2"]
    r = what_if(c, jobs, [{"name": "without a", "evict": [key_of("old-a-0")]},
                          {"name": "nothing", "evict": []},
                          {"name": "without both", "evict": [key_of("old-b-0"), key_of("old-a-0")]}])
    assert domains(r) == domains(before) and r["placed"] == before["placed"]
    a, nothing, both = r["scenarios"]
    assert domains(nothing) == domains(before) and (nothing["flips"], nothing["rows"]) == (0, 0)
    assert (a["flips"], a["rows"]) == (1, 4) and (both["flips"], both["rows"]) == (2, 8)
    # planner.plan on this cache is what it was before, and the cache's columns too
    after = planned(c, jobs)
    assert set(after) == PLAN_KEYS and domains(after) == domains(before)
    assert after["snapshot"]["upload"] == "none"
    # the same questions asked the long way: a cache without those pods
    c2, _, _ = cluster()
    for i in range(4):
        c2.add_pod(foreign_pod("old-b-0", i, f"z0-r2-n{i}"))
    c2.planner_new(engine, ["zone", "rack"], RES)
    assert domains(a) == domains(planned(c2, jobs)) == ["zone-0-rack-0", "zone-0-rack-1", "zone-0-rack-3",
                                                         "zone-1-rack-0", "zone-1-rack-1"]
    c3, _, _ = cluster()
    c3.planner_new(engine, ["zone", "rack"], RES)
    assert domains(both) == domains(planned(c3, jobs)) == RACKS


def test_evicting_an_assumed_job(engine):
    """The first JobSet's five racks are held by the ledger alone."""
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan0 = planned(c, jobs)
    assert domains(plan0) == RACKS
    r, e = c.assume(jobs, plan0)
    assert e is None and r["committed"] == 5
    before = planned(c, jobs)
    assert domains(before) == ["zone-1-rack-1", "zone-1-rack-2", "zone-1-rack-3", None, None]
    gone = ["train-workers-0", "train-workers-1"]
    r = what_if(c, jobs, [{"name": "two forgotten", "evict": [key_of(n) for n in gone]}])
    assert domains(r) == domains(before)
    sc = r["scenarios"][0]
    assert (sc["flips"], sc["rows"]) == (2, 8)
    after = planned(c, jobs)
    assert domains(after) == domains(before) and after["snapshot"]["upload"] == "none"
    # a second cache that assumed only the other three
    c2, _, jobs2 = cluster()
    c2.planner_new(engine, ["zone", "rack"], RES)
    keep = {j["name"]: j["domain"] for j in planned(c2, jobs2)["jobs"] if j["name"] not in gone}
    r2, e = c2.assume(jobs2, keep)
    assert e is None and r2["committed"] == 3
    assert domains(sc) == domains(planned(c2, jobs2)) == ["zone-0-rack-0", "zone-0-rack-1", "zone-1-rack-1",
                                                          "zone-1-rack-2", "zone-1-rack-3"]


def test_refusals(engine):
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    before = planned(c, jobs)
    r, e = c.whatIf(jobs, [{"name": "ok", "evict": []}, {"name": "drain-7", "evict": ["no-such-key"]}])
    assert r is None or not r
    assert 'scenario "drain-7": unknown job key "no-such-key"' in e, e
    r, e = c.whatIf(jobs, {"name": "x"})
    assert "scenarios must be an array" in e, e
    r, e = c.whatIf(jobs, [{"name": "x", "evict": "key"}])
    assert "scenarios must be an array" in e, e
    r, e = host.Cache().whatIf(jobs, [])
    assert "no placement planner" in e, e
    assert domains(planned(c, jobs)) == domains(before)
