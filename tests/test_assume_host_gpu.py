"""The host mirror's planner.assume / planner.forget on a cluster of Node
objects: a plan's domains are held across plans, syncs and full uploads by the
planner's ledger, a sync that sees a job's leader pod confirms it (the rows go
to the informer's id), and planner.forget frees the rest. After every step the
engine's placement equals the CPU oracle's on the planner's own columns, so the
host columns and the engine's snapshot stay equal."""
import numpy as np
import pytest

from jobset_amd import host, synth
from oracle import oracle as O

import k8s_fixtures as K
from test_sticky_host_gpu import EXCL, MAINT, RES, cluster, node, planned

pytestmark = pytest.mark.gpu

BASE = 0x40000000
RACKS = ["zone-0-rack-0", "zone-0-rack-1", "zone-0-rack-2", "zone-0-rack-3", "zone-1-rack-0"]


def domains(plan):
    return [j["domain"] for j in plan["jobs"]]


def plan_checked(c, jobs):
    """planner.plan, equal to the oracle on the planner's own columns."""
    r = planned(c, jobs)
    q = K.problem_from_planner(synth.config1(), c.planner_columns(), r)
    np.testing.assert_array_equal([j["domainId"] for j in r["jobs"]], O.place_c(q)[0])
    return r


def assumed(c, jobs, assignment):
    r, e = c.assume(jobs, assignment)
    assert e is None, e
    return r


def forgot(c, names):
    r, e = c.forget(names)
    assert e is None, e
    return r


def leader_pod(job, node_name):
    name = job["metadata"]["name"]
    return {"metadata": {"name": f"{name}-0-abcde", "namespace": "default",
                         "labels": {K.JOBKEY: host.jobHashKey("default", name)}, "annotations": {EXCL: "rack"}},
            "spec": {"nodeName": node_name,
                     "containers": [{"name": "train", "resources": {"requests": {"amd.com/gpu": "8"}}}]},
            "status": {"phase": "Running"}}


def test_plan_assume_plan_sync_forget(engine):
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan0 = plan_checked(c, jobs)
    assert domains(plan0) == RACKS
    assert domains(plan_checked(c, jobs)) == RACKS                    # nothing remembers the first plan
    r = assumed(c, jobs, plan0)
    assert [j["committed"] for j in r["jobs"]] == [True] * 5 and domains(r) == RACKS
    owners = [j["owner"] for j in r["jobs"]]
    assert owners == [BASE + i for i in range(5)]
    assert (r["committed"], r["stale"], r["rowsMarked"], r["assumed"]) == (5, 0, 20, 5)
    cols = c.planner_columns()
    for j, d in enumerate(RACKS):
        rows = [i for i, n in enumerate(cols["rows"]) if n.startswith(d.replace("zone-", "z").replace("-rack-", "-r") + "-")]
        assert len(rows) == 4 and all(cols["excl"][i] == owners[j] for i in rows)
    plan1 = plan_checked(c, jobs)                                     # the second JobSet avoids the first one's racks
    assert domains(plan1) == ["zone-1-rack-1", "zone-1-rack-2", "zone-1-rack-3", None, None]
    again = assumed(c, jobs, plan0)                                   # a repeated assume is stale and changes nothing
    assert (again["committed"], again["stale"], again["assumed"]) == (0, 5, 5)
    assert [j["owner"] for j in again["jobs"]] == owners
    # an unrelated Node event (a node of a free rack loses its GPUs): a patch of that node's row, the holds stay
    broken = node(1, 3, 0)
    broken["status"]["allocatable"]["amd.com/gpu"] = "0"
    c.add_node(broken)
    s = c.planner_sync()
    assert (s["upload"], s["patchedRows"]) == ("patch", 1)
    assert domains(plan_checked(c, jobs)) == ["zone-1-rack-1", "zone-1-rack-2", None, None, None]
    c.add_node(node(1, 3, 0))
    assert c.planner_sync()["patchedRows"] == 1
    # forget two of them: their racks are free again, the others are not
    f = forgot(c, ["train-workers-3", "train-workers-1", "no-such-job"])
    assert (f["rowsCleared"], sorted(f["forgotten"]), f["assumed"]) == (8, ["train-workers-1", "train-workers-3"], 3)
    assert domains(plan_checked(c, jobs)) == ["zone-0-rack-1", "zone-0-rack-3", "zone-1-rack-1", "zone-1-rack-2",
                                              "zone-1-rack-3"]
    f = forgot(c, [j["metadata"]["name"] for j in jobs])
    assert (f["rowsCleared"], f["assumed"]) == (12, 0)
    assert domains(plan_checked(c, jobs)) == RACKS                    # the next plan equals the first
    assert all(x == -1 for x in c.planner_columns()["excl"])
    assert c.planner_sync()["upload"] == "none"                       # and the host columns equal the engine's


def test_confirmation_and_full_upload_keep_the_ledger(engine):
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan0 = plan_checked(c, jobs)
    r = assumed(c, jobs, {j["name"]: j["domain"] for j in plan0["jobs"]})      # the map form of the assignment
    assert r["committed"] == 5
    # job 2's leader shows up: its hold is confirmed, the rack's rows go to the informer's id
    c.add_pod(leader_pod(jobs[2], "z0-r2-n1"))
    s = c.planner_sync()
    assert (s["upload"], s["patchedRows"], s["exclusiveJobs"]) == ("patch", 4, 1)
    cols = c.planner_columns()
    assert sorted(set(cols["excl"])) == [-1, 0, BASE, BASE + 1, BASE + 3, BASE + 4]
    assert domains(plan_checked(c, jobs)) == ["zone-1-rack-1", "zone-1-rack-2", "zone-1-rack-3", None, None]
    f = forgot(c, ["train-workers-2"])                                # confirmed: the ledger no longer holds it
    assert (f["rowsCleared"], f["forgotten"], f["assumed"]) == (0, [], 4)
    # a structural change: a node joins rack zone-1-rack-3, everything is uploaded again with the holds in it
    c.add_node(node(1, 3, 4))
    s = c.planner_sync()
    assert (s["upload"], s["rows"]) == ("full", 33)
    assert domains(plan_checked(c, jobs)) == ["zone-1-rack-1", "zone-1-rack-2", "zone-1-rack-3", None, None]
    cols = c.planner_columns()
    assert sorted(set(cols["excl"])) == [-1, 0, BASE, BASE + 1, BASE + 3, BASE + 4]
    # a rack that disappears takes its hold with it
    for n in range(4):
        c.remove_node(f"z1-r0-n{n}")
    s = c.planner_sync()
    assert s["upload"] == "full"
    f = forgot(c, ["train-workers-4"])
    assert (f["rowsCleared"], f["forgotten"], f["assumed"]) == (0, [], 3)
    f = forgot(c, [j["metadata"]["name"] for j in jobs])
    assert (f["rowsCleared"], sorted(f["forgotten"]), f["assumed"]) == \
        (12, ["train-workers-0", "train-workers-1", "train-workers-3"], 0)
    # job 2's rack stays with the informer; the rest is free again
    assert domains(plan_checked(c, jobs)) == ["zone-0-rack-0", "zone-0-rack-1", "zone-0-rack-3", "zone-1-rack-1",
                                              "zone-1-rack-2"]


def test_assume_after_damage_and_refusal(engine):
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan0 = plan_checked(c, jobs)
    by_name = {j["name"]: j["domain"] for j in plan0["jobs"]}
    c.add_node(node(0, 1, 2, MAINT))                     # job 1's rack loses a node: its domain is stale
    by_name["train-workers-4"] = "zone-9-rack-9"        # a value the cluster does not have: unplaced
    r = assumed(c, jobs, by_name)
    assert [j["committed"] for j in r["jobs"]] == [True, False, True, True, False]
    assert r["jobs"][4]["domain"] is None and r["jobs"][4]["owner"] is None
    assert (r["committed"], r["stale"], r["rowsMarked"], r["assumed"]) == (3, 1, 12, 3)
    by_name["train-workers-4"] = "zone-0-rack-0"        # the rack job 0 holds: refused, with the job named
    r, e = c.assume(jobs, by_name)
    assert e is not None and "job 4" in e
    assert forgot(c, [j["metadata"]["name"] for j in jobs])["rowsCleared"] == 12
