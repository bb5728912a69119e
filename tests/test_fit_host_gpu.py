"""The host mirror's fit planning (planner.planFit) on a cluster of Node
objects: for each policy the domain names equal the engine's own answer
(jsp_place_fit on the planner's snapshot and classes) mapped through the
topology values, and the rule restated over the CPU oracle (tests/fit_ref.py);
an unknown policy is refused by name; planner.plan on the same cache is what
it was before."""
import numpy as np
import pytest

from jobset_amd import host, synth
from fit_ref import fit_ref

import k8s_fixtures as K

pytestmark = pytest.mark.gpu

EXCL = "alpha.jobset.sigs.k8s.io/exclusive-topology"
RES = ["cpu", "memory", "amd.com/gpu"]
POLICY_ID = {"lowest": 0, "tightest": 1, "roomiest": 2}


def node(r, n):
    name = f"r{r}-n{n}"
    return {"metadata": {"name": name, "labels": {"zone": "zone-0", "rack": f"rack-{r}", "kubernetes.io/hostname": name}},
            "spec": {"taints": []},
            "status": {"allocatable": {"cpu": "192", "memory": "1536000Mi", "amd.com/gpu": "8"}}}


def jobset(name, pods):
    """One replicated job named after the JobSet: the planner keys a class by
    (replicated job name, topology key)."""
    js = {"metadata": {"name": name, "namespace": "default", "annotations": {EXCL: "rack"}},
          "spec": {"replicatedJobs": [{"name": name, "replicas": 1, "template": {
              "spec": {"parallelism": pods, "completions": pods, "template": {"spec": {
                  "containers": [{"name": "train", "resources": {"requests": {"amd.com/gpu": "8"}}}]}}}}}],
              "network": {}},
          "status": {"restarts": 0}}
    return host.constructJobsFromTemplate(js, js["spec"]["replicatedJobs"][0], {})


def cluster():
    """Racks of 8, 2, 4 and 2 one-pod nodes; a job of 2 pods, then one of 6."""
    c = host.Cache()
    for r, n_nodes in enumerate([8, 2, 4, 2]):
        for n in range(n_nodes):
            c.add_node(node(r, n))
    return c, jobset("a-small", 2) + jobset("b-big", 6)   # in name order, the planner's job order


WANT = {"lowest": ["rack-0", None], "tightest": ["rack-1", "rack-0"], "roomiest": ["rack-0", None]}


@pytest.mark.parametrize("policy", list(WANT))
def test_plan_fit_is_the_engines_answer(engine, policy):
    c, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    before, e = c.plan(jobs)
    assert e is None, e
    r, e = c.planFit(jobs, policy)
    assert e is None, e
    assert set(r) == {"jobs", "unplaceable", "placed", "snapshot", "classes", "jobClass", "policy", "slack"}
    assert all(set(j) == {"name", "topologyKey", "domainId", "domain"} for j in r["jobs"])
    assert r["policy"] == policy
    assert [j["domain"] for j in r["jobs"]] == WANT[policy]
    # the engine's own answer on the snapshot and classes the planner left in it, through the topology values
    cols = c.planner_columns()
    q = K.problem_from_planner(synth.config1(), cols, r)
    got, st = engine.place_fit(q.job_class, POLICY_ID[policy])
    assert [j["domainId"] for j in r["jobs"]] == got.tolist()
    assert [j["domain"] for j in r["jobs"]] == K.assign_values(q, got, dict(enumerate(cols["domainValues"])))
    assert (r["placed"], r["slack"]) == (int(st.placed), int(st.slack))
    assert r["unplaceable"] == [j["name"] for j in r["jobs"] if j["domain"] is None]
    # ... and the rule over the CPU oracle
    want, want_st = fit_ref(q, POLICY_ID[policy])
    np.testing.assert_array_equal(got, want)
    assert (r["placed"], r["slack"]) == (want_st["placed"], want_st["slack"])
    # planner.plan is what it was before planFit ran on this cache, and "lowest" is its answer
    after, e = c.plan(jobs)
    assert e is None, e
    assert set(after) == set(before) == {"jobs", "unplaceable", "placed", "snapshot", "classes", "jobClass"}
    for k in ("jobs", "unplaceable", "placed", "classes", "jobClass"):
        assert after[k] == before[k], k
    if policy == "lowest":
        assert r["jobs"] == after["jobs"] and r["placed"] == after["placed"]


def test_plan_fit_refuses_an_unknown_policy_by_name(engine):
    c, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    r, e = c.planFit(jobs, "snuggest")
    assert e is not None and "snuggest" in e and "tightest" in e
    r, e = c.planFit(jobs, "")
    assert e is not None and "policy" in e
    r, e = c.planFit(jobs, "tightest")
    assert e is None and r["placed"] == 2
