"""The host mirror's planner.bind on a cluster of Node objects: a plan's
domains travel as topology values, and the node name per completion index is
the yardstick's row (tests/bind_ref.py on the planner's own snapshot and
classes) mapped through the planner's row -> node table."""
import numpy as np
import pytest

from jobset_amd import host, synth
from bind_ref import bind_ref

import k8s_fixtures as K
from test_sticky_host_gpu import MAINT, RES, cluster, node, planned

pytestmark = pytest.mark.gpu


def bound(c, jobs, assignment):
    r, e = c.bind(jobs, assignment)
    assert e is None, e
    return r


def reference(c, plan, by_name):
    """Per job the node names bind_ref gives on the planner's snapshot."""
    cols = c.planner_columns()
    q = K.problem_from_planner(synth.config1(), cols, plan)
    assign = []
    for j, job in enumerate(plan["jobs"]):
        vals = cols["domainValues"][q.classes[int(q.job_class[j])].level]
        v = by_name.get(job["name"])
        assign.append(vals.index(v) if v in vals else -1)
    rows, off, st = bind_ref(q, np.array(assign, dtype=np.int32))
    names = [[None if r < 0 else cols["rows"][int(r)] for r in rows[int(off[j]):int(off[j + 1])]]
             for j in range(len(assign))]
    return names, st


def test_bind_a_plan(engine):
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan = planned(c, jobs)
    r = bound(c, jobs, plan)
    by_name = {j["name"]: j["domain"] for j in plan["jobs"]}
    want, st = reference(c, plan, by_name)
    assert [j["nodes"] for j in r["jobs"]] == want
    assert [j["domain"] for j in r["jobs"]] == [j["domain"] for j in plan["jobs"]]
    assert all(j["bound"] for j in r["jobs"])
    assert sorted(r["jobs"][1]["nodes"]) == ["z0-r1-n0", "z0-r1-n1", "z0-r1-n2", "z0-r1-n3"]
    assert (r["bound"], r["stale"], r["rowsUsed"], r["pods"], r["podsBound"]) == (5, 0, 20, 20, 20)
    assert (st["bound"], st["rows_used"]) == (5, 20)
    assert bound(c, jobs, by_name)["jobs"] == r["jobs"]                                # the map form of the assignment


def test_bind_after_damage_and_with_unknown_values(engine):
    c, js, jobs = cluster()
    c.planner_new(engine, ["zone", "rack"], RES)
    plan = planned(c, jobs)
    by_name = {j["name"]: j["domain"] for j in plan["jobs"]}
    c.add_node(node(0, 1, 2, MAINT))                     # job 1's rack loses a node: its domain is stale
    by_name["train-workers-4"] = "zone-9-rack-9"        # a value the cluster does not have: unplaced
    r = bound(c, jobs, by_name)
    want, st = reference(c, plan, by_name)
    assert [j["nodes"] for j in r["jobs"]] == want
    assert [j["bound"] for j in r["jobs"]] == [True, False, True, True, False]
    assert r["jobs"][1]["nodes"] == [None] * 4 and r["jobs"][1]["domain"] == "zone-0-rack-1"
    assert r["jobs"][4]["domain"] is None
    assert (r["bound"], r["stale"], r["podsBound"]) == (3, 1, 12) == (st["bound"], st["stale"], st["pods_bound"])
    by_name["train-workers-4"] = "zone-0-rack-0"        # the rack job 0 holds: refused, with the job named
    r, e = c.bind(jobs, by_name)
    assert e is not None and "job 4" in e
