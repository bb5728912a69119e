"""The host mirror's sticky planning (planner.plan with "previous",
controllers.reconcileRecreate with "previousPlan") on a cluster of Node
objects: previous domains travel as topology values, an unknown value is no
hint, the kept / moved / lost totals are those of the rule restated over the
CPU oracle (tests/sticky_ref.py) on the planner's own snapshot, and a plan
without "previous" has exactly the fields it always had."""
import numpy as np
import pytest

from jobset_amd import host, synth
from oracle import oracle as O
from sticky_ref import sticky_ref

import k8s_fixtures as K

pytestmark = pytest.mark.gpu

EXCL = "alpha.jobset.sigs.k8s.io/exclusive-topology"
RES = ["cpu", "memory", "amd.com/gpu"]
MAINT = [{"key": "maintenance", "value": "", "effect": "NoSchedule"}]


def node(z, r, n, taints=()):
    name = f"z{z}-r{r}-n{n}"
    return {"metadata": {"name": name, "labels": {"zone": f"zone-{z}", "rack": f"zone-{z}-rack-{r}",
                                                  "kubernetes.io/hostname": name}},
            "spec": {"taints": list(taints)},
            "status": {"allocatable": {"cpu": "192", "memory": "1536000Mi", "amd.com/gpu": "8"}}}


def cluster():
    """2 zones x 4 racks x 4 nodes, a planner on the session engine, 5 rack-exclusive jobs of 4 pods."""
    c = host.Cache()
    for z in range(2):
        for r in range(4):
            for n in range(4):
                c.add_node(node(z, r, n))
    js = {"metadata": {"name": "train", "namespace": "default", "annotations": {EXCL: "rack"}},
          "spec": {"replicatedJobs": [{"name": "workers", "replicas": 5, "template": {
              "spec": {"parallelism": 4, "completions": 4, "template": {"spec": {
                  "containers": [{"name": "train", "resources": {"requests": {"amd.com/gpu": "8"}}}]}}}}}],
              "network": {}},
          "status": {"restarts": 0}}
    return c, js, host.constructJobsFromTemplate(js, js["spec"]["replicatedJobs"][0], {})


def planned(c, jobs, previous=None):
    r, e = c.plan(jobs, previous)
    assert e is None, e
    return r


def reference(c, plan, previous):
    """The rule on the planner's own snapshot and classes; hints by value."""
    cols = c.planner_columns()
    q = K.problem_from_planner(synth.config1(), cols, plan)
    prev = []
    for j, job in enumerate(plan["jobs"]):
        vals = cols["domainValues"][q.classes[int(q.job_class[j])].level]
        v = previous.get(job["name"])
        prev.append(vals.index(v) if v in vals else -1)
    return sticky_ref(q, np.array(prev, dtype=np.int32)), np.array(prev)


def test_plan_without_previous_is_unchanged(engine):
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    r = planned(c, jobs)
    assert set(r) == {"jobs", "unplaceable", "placed", "snapshot", "classes", "jobClass"}
    assert all(set(j) == {"name", "topologyKey", "domainId", "domain"} for j in r["jobs"])
    assert [j["domain"] for j in r["jobs"]] == ["zone-0-rack-0", "zone-0-rack-1", "zone-0-rack-2", "zone-0-rack-3",
                                                "zone-1-rack-0"]
    q = K.problem_from_planner(synth.config1(), c.planner_columns(), r)
    np.testing.assert_array_equal([j["domainId"] for j in r["jobs"]], O.place_c(q)[0])


def test_plan_with_previous_keeps_moves_and_loses(engine):
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan0 = planned(c, jobs)
    previous = {j["name"]: j["domain"] for j in plan0["jobs"]}
    # job 1's rack loses a node; job 4's previous value is one the cluster no longer has
    c.add_node(node(0, 1, 2, MAINT))
    previous["train-workers-4"] = "zone-9-rack-9"
    r = planned(c, jobs, previous)
    (want, kept), prev = reference(c, r, previous)
    np.testing.assert_array_equal([j["domainId"] for j in r["jobs"]], want)
    assert [j["domain"] for j in r["jobs"]] == ["zone-0-rack-0", "zone-1-rack-0", "zone-0-rack-2", "zone-0-rack-3",
                                                "zone-1-rack-1"]
    assert [j["kept"] for j in r["jobs"]] == [True, False, True, True, False] == kept.tolist()
    assert [j["previousDomain"] for j in r["jobs"]] == ["zone-0-rack-0", "zone-0-rack-1", "zone-0-rack-2",
                                                        "zone-0-rack-3", None]
    assert (r["hinted"], r["kept"], r["moved"], r["lost"], r["placed"]) == (4, 3, 1, 0, 5)
    # the cluster gets tight: three more racks lose a node, job 1 has nowhere to go
    for rk in (1, 2, 3):
        c.add_node(node(1, rk, 0, MAINT))
    previous = {j["name"]: j["domain"] for j in plan0["jobs"]}
    r = planned(c, jobs, previous)
    (want, kept), prev = reference(c, r, previous)
    np.testing.assert_array_equal([j["domainId"] for j in r["jobs"]], want)
    assert [j["domain"] for j in r["jobs"]] == ["zone-0-rack-0", None, "zone-0-rack-2", "zone-0-rack-3",
                                                "zone-1-rack-0"]
    assert (r["hinted"], r["kept"], r["moved"], r["lost"], r["placed"]) == (5, 4, 0, 1, 4)
    assert r["unplaceable"] == ["train-workers-1"]
    # what the lowest-index rule alone does with the same snapshot: everything behind job 1 shifts
    plain = planned(c, jobs)
    assert [j["domain"] for j in plain["jobs"]] == ["zone-0-rack-0", "zone-0-rack-2", "zone-0-rack-3",
                                                    "zone-1-rack-0", None]


def test_reconcile_recreate_with_previous_plan(engine):
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan0 = planned(c, jobs)
    c.add_node(node(0, 2, 3, MAINT))
    js1 = host.failurePolicyRecreateAll(js, True)
    out, err = c.reconcileRecreate(js1, [], plan0)
    assert err is None and "planError" not in out and len(out["create"]) == 5
    plan = out["plan"]
    assert [j["domain"] for j in plan["jobs"]] == ["zone-0-rack-0", "zone-0-rack-1", "zone-1-rack-1", "zone-0-rack-3",
                                                   "zone-1-rack-0"]
    assert (plan["hinted"], plan["kept"], plan["moved"], plan["lost"]) == (5, 4, 1, 0)
    out, err = c.reconcileRecreate(js1, [])          # without it: the lowest-index plan, and its fields only
    assert err is None and "kept" not in out["plan"] and "kept" not in out["plan"]["jobs"][0]
    assert [j["domain"] for j in out["plan"]["jobs"]] == ["zone-0-rack-0", "zone-0-rack-1", "zone-0-rack-3",
                                                          "zone-1-rack-0", "zone-1-rack-1"]
