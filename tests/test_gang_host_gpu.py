"""The host mirror's gang planning (planner.planGangs) on a cluster of Node
objects: gangs are the runs of consecutive jobs of one JobSet, spans travel as
topology keys, the answer is the rule restated over the CPU oracle
(tests/gang_ref.py) on the planner's own snapshot, the two "spans" errors name
the JobSet, and planner.plan on the same cache is what it was before."""
import copy

import numpy as np
import pytest

from jobset_amd import host, synth
from gang_ref import ANY, gang_ref

import k8s_fixtures as K

pytestmark = pytest.mark.gpu

EXCL = "alpha.jobset.sigs.k8s.io/exclusive-topology"
RES = ["cpu", "memory", "amd.com/gpu"]


def node(z, r, n):
    name = f"z{z}-r{r}-n{n}"
    return {"metadata": {"name": name, "labels": {"zone": f"zone-{z}", "rack": f"zone-{z}-rack-{r}",
                                                  "kubernetes.io/hostname": name}},
            "spec": {"taints": []},
            "status": {"allocatable": {"cpu": "192", "memory": "1536000Mi", "amd.com/gpu": "8"}}}


def jobset(name, replicas, key="rack", pods=4):
    js = {"metadata": {"name": name, "namespace": "default", "annotations": {EXCL: key}},
          "spec": {"replicatedJobs": [{"name": "workers", "replicas": replicas, "template": {
              "spec": {"parallelism": pods, "completions": pods, "template": {"spec": {
                  "containers": [{"name": "train", "resources": {"requests": {"amd.com/gpu": "8"}}}]}}}}}],
              "network": {}},
          "status": {"restarts": 0}}
    return host.constructJobsFromTemplate(js, js["spec"]["replicatedJobs"][0], {})


def cluster():
    """2 zones x 4 racks x 4 nodes; JobSets a, b, c of 3 rack-exclusive jobs of 4 pods each."""
    c = host.Cache()
    for z in range(2):
        for r in range(4):
            for n in range(4):
                c.add_node(node(z, r, n))
    return c, jobset("a", 3) + jobset("b", 3) + jobset("c", 3)


def reference(c, plan, spans):
    """The rule on the planner's own snapshot and classes; gangs and spans from the reply's names."""
    cols = c.planner_columns()
    q = K.problem_from_planner(synth.config1(), cols, plan)
    sets = [j["jobSet"] for j in plan["jobs"]]
    gj, gs = [], []
    for i, s in enumerate(sets):
        if i == 0 or s != sets[i - 1]:
            gj.append(0)
            gs.append(["zone", "rack"].index(spans[s]) if s in spans else ANY)
        gj[-1] += 1
    return gang_ref(q, gj, gs), cols


def test_plan_gangs_whole_jobsets_inside_their_zone(engine):
    c, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    before, e = c.plan(jobs)
    assert e is None, e
    spans = {"default/a": "zone", "default/b": "zone"}
    r, e = c.planGangs(jobs, spans)
    assert e is None, e
    assert set(r) == {"jobs", "unplaceable", "placed", "snapshot", "classes", "jobClass", "jobSets", "gangsPlaced"}
    assert all(set(j) == {"name", "topologyKey", "domainId", "domain", "jobSet"} for j in r["jobs"])
    (want, want_span), cols = reference(c, r, spans)
    np.testing.assert_array_equal([j["domainId"] for j in r["jobs"]], want)
    # a fills three racks of zone 0, b does not fit behind it and takes zone 1, c finds two racks for three jobs
    assert [j["domain"] for j in r["jobs"]] == ["zone-0-rack-0", "zone-0-rack-1", "zone-0-rack-2", "zone-1-rack-0",
                                                "zone-1-rack-1", "zone-1-rack-2", None, None, None]
    assert r["jobSets"] == [{"name": "default/a", "spanKey": "zone", "spanDomain": "zone-0", "placed": True},
                            {"name": "default/b", "spanKey": "zone", "spanDomain": "zone-1", "placed": True},
                            {"name": "default/c", "spanKey": None, "spanDomain": None, "placed": False}]
    assert [x["placed"] for x in r["jobSets"]] == (want_span >= 0).tolist()
    assert (r["gangsPlaced"], r["placed"]) == (2, 6)
    assert r["unplaceable"] == [j["metadata"]["name"] for j in jobs[6:]]
    # job by job the same batch strands c with two of its three jobs placed
    after, e = c.plan(jobs)
    assert e is None, e
    assert [j["domain"] for j in after["jobs"]][3:] == ["zone-0-rack-3", "zone-1-rack-0", "zone-1-rack-1",
                                                        "zone-1-rack-2", "zone-1-rack-3", None]
    # ... and planner.plan is what it was before planGangs ran on this cache
    assert set(after) == set(before) == {"jobs", "unplaceable", "placed", "snapshot", "classes", "jobClass"}
    for k in ("jobs", "unplaceable", "placed", "classes", "jobClass"):
        assert after[k] == before[k], k


def test_plan_gangs_without_spans_and_split_jobsets(engine):
    """No spans: whole or nothing anywhere. A JobSet whose jobs are not consecutive is two gangs."""
    c, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    r, e = c.planGangs(jobs)
    assert e is None, e
    (want, want_span), _ = reference(c, r, {})
    np.testing.assert_array_equal([j["domainId"] for j in r["jobs"]], want)
    assert [x["placed"] for x in r["jobSets"]] == [True, True, False] and r["gangsPlaced"] == 2
    assert all(x["spanKey"] is None and x["spanDomain"] is None for x in r["jobSets"])
    mixed = jobs[0:2] + jobs[3:5] + jobs[2:3]          # a a b b a
    r, e = c.planGangs(mixed, {"default/a": "zone"})
    assert e is None, e
    assert [x["name"] for x in r["jobSets"]] == ["default/a", "default/b", "default/a"]
    (want, want_span), _ = reference(c, r, {"default/a": "zone"})
    np.testing.assert_array_equal([j["domainId"] for j in r["jobs"]], want)
    assert r["gangsPlaced"] == 3


def test_plan_gangs_span_errors_name_the_jobset(engine):
    c, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    r, e = c.planGangs(jobs, {"default/b": "row"})
    assert e is not None and "default/b" in e and "row" in e
    zoned = jobset("z", 1, key="zone", pods=16)
    r, e = c.planGangs(jobs + zoned, {"default/z": "rack"})
    assert e is not None and "default/z" in e and "finer" in e
    # a span equal to the job's own key is allowed: a's three jobs do not fit one rack, b fills zone 0, z takes zone 1
    r, e = c.planGangs(jobs[:6] + zoned, {"default/z": "zone", "default/a": "rack"})
    assert e is None, e
    assert r["jobSets"][0] == {"name": "default/a", "spanKey": "rack", "spanDomain": None, "placed": False}
    assert r["jobSets"][2] == {"name": "default/z", "spanKey": "zone", "spanDomain": "zone-1", "placed": True}
    plain, e = c.plan(copy.deepcopy(jobs))
    assert e is None and plain["placed"] == 8
