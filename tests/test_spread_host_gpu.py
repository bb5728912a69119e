"""The host mirror's spread planning (planner.planSpread) on a two-zone cluster
of Node objects with one JobSet partly running: the reply's domains, spread
domains and counts equal the rule taken literally (tests/spread_ref.py) on the
planner's own columns, with the peers the planner derives from the cache (the
JobSet's running jobs, then its assumed ones) or takes from the request; a
foreign JobSet's jobs are no peers; nothing is written; the request errors
name what is wrong."""
import pytest

from jobset_amd import host, synth

import k8s_fixtures as K
from spread_ref import SOFT, spread_ref
from test_sticky_host_gpu import EXCL, RES, cluster, planned
from test_whatif_host_gpu import PLAN_KEYS, domains, key_of

pytestmark = pytest.mark.gpu

JSNAME = "jobset.sigs.k8s.io/jobset-name"
# running jobs: name -> (rack, JobSet)
RUNNING = {"train-workers-0": ("z0-r0", "train"), "train-workers-1": ("z0-r1", "train"), "other-w-0": ("z1-r0", "other")}


def running_pod(job_name, i, node_name, jobset):
    return {"metadata": {"name": f"{job_name}-{i}-abcde", "namespace": "default",
                         "labels": {K.JOBKEY: key_of(job_name), JSNAME: jobset}, "annotations": {EXCL: "rack"}},
            "spec": {"nodeName": node_name,
                     "containers": [{"name": "train", "resources": {"requests": {"amd.com/gpu": "8"}}}]},
            "status": {"phase": "Running"}}


def partly_running():
    """test_sticky_host_gpu's cluster (2 zones x 4 racks x 4 nodes; JobSet
    `train`, 5 rack-exclusive jobs) with train's jobs 0 and 1 running on zone
    0's first two racks and a foreign JobSet's job on zone 1's first: the
    request is train's jobs 2, 3 and 4."""
    c, js, jobs = cluster()
    for name, (rack, jobset) in RUNNING.items():
        for i in range(4):
            c.add_pod(running_pod(name, i, f"{rack}-n{i}", jobset))
    assert [j["metadata"]["name"] for j in jobs[:2]] == ["train-workers-0", "train-workers-1"]
    assert jobs[2]["metadata"]["labels"][JSNAME] == "train"
    return c, js, jobs[2:]


def plan_spread(c, jobs, key, skew, when="DoNotSchedule", peers=None):
    r, e = c.plan_spread(jobs, key, skew, when, peers)
    assert e is None, e
    assert set(r) == PLAN_KEYS | {"topologyKey", "maxSkew", "whenUnsatisfiable", "peers", "counts", "refused", "skew"}
    assert all(set(j) == {"name", "topologyKey", "domainId", "domain", "spreadDomain"} for j in r["jobs"])
    assert r["placed"] == sum(j["domain"] is not None for j in r["jobs"])
    return r


def reference(c, plan, level, skew, peer_names):
    """spread_ref on the planner's columns; the peers' ids are what their racks' rows carry."""
    cols = c.planner_columns()
    q = K.problem_from_planner(synth.config1(), cols, plan)
    row = {n: i for i, n in enumerate(cols["rows"])}
    ids = []
    for n in peer_names:
        owner = {int(q.nodes.excl[row[f"{RUNNING[n][0]}-n{i}"]]) for i in range(4)}
        assert len(owner) == 1 and -1 not in owner
        ids.append(owner.pop())
    a, sp, cnt, st, _ = spread_ref(q, level, skew, ids)
    vals = cols["domainValues"]
    doms = [None if d < 0 else vals[q.classes[int(q.job_class[j])].level][d] for j, d in enumerate(a.tolist())]
    sdoms = [None if s < 0 else vals[level][s] for s in sp.tolist()]
    return doms, sdoms, {vals[level][S]: int(n) for S, n in enumerate(cnt.tolist())}, st


@pytest.mark.parametrize("when,skew", [("DoNotSchedule", 1), ("DoNotSchedule", 2), ("ScheduleAnyway", 1)])
def test_plan_spread_equals_the_reference(engine, when, skew):
    c, js, jobs = partly_running()
    c.planner_new(engine, ["zone", "rack"], RES)
    before = planned(c, jobs)
    assert domains(before) == ["zone-0-rack-2", "zone-0-rack-3", "zone-1-rack-1"]     # the plain plan piles into zone 0
    r = plan_spread(c, jobs, "zone", skew, when)
    mine = ["train-workers-0", "train-workers-1"]
    assert r["peers"] == sorted(key_of(n) for n in mine)                               # the foreign JobSet's job is none
    doms, sdoms, counts, st = reference(c, before, 0, skew if when == "DoNotSchedule" else SOFT, mine)
    assert domains(r) == doms and [j["spreadDomain"] for j in r["jobs"]] == sdoms
    assert r["counts"] == counts and (r["refused"], r["skew"]) == (st["refused"], st["skew"])
    if skew == 1:    # zone 0 starts two ahead: zone 1 twice, then zone 0 again
        assert doms == ["zone-1-rack-1", "zone-1-rack-2", "zone-0-rack-2"] and counts == {"zone-0": 3, "zone-1": 2}
    assert (r["topologyKey"], r["maxSkew"], r["whenUnsatisfiable"]) == ("zone", skew, when)
    # nothing was written: planner.plan on this cache is what it was before
    after = planned(c, jobs)
    assert set(after) == PLAN_KEYS and domains(after) == domains(before)
    assert after["snapshot"]["upload"] == "none"


def test_explicit_peers_and_the_rack_level(engine):
    c, js, jobs = partly_running()
    c.planner_new(engine, ["zone", "rack"], RES)
    before = planned(c, jobs)
    r = plan_spread(c, jobs, "zone", 1, peers=[key_of("other-w-0")])                   # the foreign job alone counts
    doms, sdoms, counts, st = reference(c, before, 0, 1, ["other-w-0"])
    assert domains(r) == doms == ["zone-0-rack-2", "zone-0-rack-3", "zone-1-rack-1"] and r["counts"] == counts
    r = plan_spread(c, jobs, "zone", 1, peers=[])                                      # nobody counts
    assert domains(r) == reference(c, before, 0, 1, [])[0] and r["peers"] == []
    r = plan_spread(c, jobs, "rack", 1)                                                # the jobs' own level
    doms, sdoms, counts, st = reference(c, before, 1, 1, ["train-workers-0", "train-workers-1"])
    assert domains(r) == doms and [j["spreadDomain"] for j in r["jobs"]] == doms and r["counts"] == counts


def test_assumed_jobs_of_the_jobset_are_peers(engine):
    """Jobs 0 and 1 held by planner.assume alone (no pods yet): the ledger makes them peers."""
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan0 = planned(c, jobs[:2])
    assert domains(plan0) == ["zone-0-rack-0", "zone-0-rack-1"]
    r, e = c.assume(jobs[:2], plan0)
    assert e is None and r["committed"] == 2
    r = plan_spread(c, jobs[2:], "zone", 1)
    assert r["peers"] == sorted(key_of(f"train-workers-{i}") for i in range(2))
    assert domains(r) == ["zone-1-rack-0", "zone-1-rack-1", "zone-0-rack-2"]
    assert r["counts"] == {"zone-0": 3, "zone-1": 2} and (r["refused"], r["skew"]) == (0, 1)
    # the request's own jobs are never their own peers
    r = plan_spread(c, jobs[:2], "zone", 1)
    assert r["peers"] == []


def test_refusals(engine):
    c, js, jobs = partly_running()
    c.planner_new(engine, ["zone", "rack"], RES)
    before = planned(c, jobs)
    for bad in (None, 0, -1, "two", 2 ** 31):
        r, e = c.plan_spread(jobs, "zone", bad)
        assert (r is None or not r) and "maxSkew must be an integer >= 1" in e, e
    r, e = c.plan_spread(jobs, "zone", 1, "Sometimes")
    assert "whenUnsatisfiable" in e and "Sometimes" in e, e
    r, e = c.plan_spread(jobs, "region", 1)
    assert "region" in e and "no level" in e, e
    r, e = c.plan_spread(jobs, "zone", 1, peers=[key_of("nobody-0")])
    assert "holds no domain" in e and key_of("nobody-0") in e, e
    r, e = c.plan_spread(jobs, "zone", 1, peers="all")
    assert "peers must be a list" in e, e
    r, e = host.Cache().plan_spread(jobs, "zone", 1)
    assert "no placement planner" in e, e
    assert domains(planned(c, jobs)) == domains(before)
    plan_spread(c, jobs, "zone", 1)
    # a key finer than the jobs' own (a second cache, whose planner takes the engine over)
    c2, _, zone_jobs = cluster()
    for j in zone_jobs:
        j["metadata"]["annotations"][EXCL] = "zone"
    c2.planner_new(engine, ["zone", "rack"], RES)
    r, e = c2.plan_spread(zone_jobs, "rack", 1)
    assert "finer than" in e, e
