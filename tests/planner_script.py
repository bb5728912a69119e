"""One fixed cluster and one fixed sequence of planner requests through the
host mirror's JSON calls, as data: run() returns [label, result, error] per
call. A plain module like run_forms.py, not a test. tests/
test_planner_replies.py runs it without an engine, tests/
test_planner_replies_gpu.py with one, and each compares the list with a
recording of the same script (tests/golden/planner_replies_{cpu,gpu}.json):

    python tests/planner_script.py --record PATH [--engine]

writes the list to PATH through whichever library jobset_amd/native.py loads
(JSP_LIB_PATH selects another build of it). The recordings pin the order of
the checks, the error texts, the reply fields and the engineCalls accounting
of every planner.* method; they are taken from the commit before a change to
the host mirror, never from the code the change leaves behind.

The cluster: levels zone and rack; zone-0 has racks of 8 and 2 nodes, zone-1
racks of 4 and 2, every node 8 GPUs. z0-r0-n7 is tainted, zone-0-rack-1 is
held by a bound pod of a foreign exclusive job. A pod asks for a whole node, so
a rack holds a job of as many pods as it has usable nodes: 7, -, 4, 2; zone-1
holds 6, zone-0 is occupied.

The jobs, in the order they are handed over (class in brackets):
  default/train   w-0 [0]  big-0 [1]  w-1 [0]  big-1 [1]  w-2 [0]   w: 2 pods, big: 6 pods, rack
  default/plain   x-0      no exclusive annotation: not placed by the engine
  default/solo    w-0 [0]  w-1 [0]                                   train's class: same replicated job and key
  team-b/nsel     x-0      node-selector strategy: not placed by the engine
  team-b/eval     zonal-0 [2]  small-0 [3]                           zonal: 4 pods, zone; small: 1 pod, rack
Only one rack fits a 6-pod job, so train never fits as a gang.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from jobset_amd import host  # noqa: E402

EXCL = "alpha.jobset.sigs.k8s.io/exclusive-topology"
NODE_SELECTOR = "alpha.jobset.sigs.k8s.io/node-selector"
JOBKEY = "jobset.sigs.k8s.io/job-key"
RESTARTS = "jobset.sigs.k8s.io/restart-attempt"
LEVELS = ["zone", "rack"]
RES = ["cpu", "memory", "amd.com/gpu"]
RACK_NODES = {(0, 0): 8, (0, 1): 2, (1, 0): 4, (1, 1): 2}
R00, R01, R10, R11 = "zone-0-rack-0", "zone-0-rack-1", "zone-1-rack-0", "zone-1-rack-1"
POLICIES = ("lowest", "tightest", "roomiest")


def node(z, r, n, taints=()):
    name = f"z{z}-r{r}-n{n}"
    return {"metadata": {"name": name, "labels": {"zone": f"zone-{z}", "rack": f"zone-{z}-rack-{r}",
                                                  "kubernetes.io/hostname": name}},
            "spec": {"taints": list(taints)},
            "status": {"allocatable": {"cpu": "192", "memory": "1536000Mi", "amd.com/gpu": "8"}}}


def pod(name, ns, job_key, node_name):
    return {"metadata": {"name": name, "namespace": ns, "labels": {JOBKEY: job_key}, "annotations": {EXCL: "rack"}},
            "spec": {"nodeName": node_name,
                     "containers": [{"name": "train", "resources": {"requests": {"amd.com/gpu": "8"}}}]},
            "status": {"phase": "Running"}}


def rjob(name, replicas, pods, key=None):
    t = {"spec": {"parallelism": pods, "completions": pods, "template": {"spec": {
        "containers": [{"name": "train", "resources": {"requests": {"amd.com/gpu": "8"}}}]}}}}
    if key is not None:
        t["metadata"] = {"annotations": {EXCL: key}}
    return {"name": name, "replicas": replicas, "template": t}


def jobset(name, ns, rjobs, annotations):
    return {"metadata": {"name": name, "namespace": ns, "annotations": dict(annotations)},
            "spec": {"replicatedJobs": rjobs, "network": {}}, "status": {"restarts": 0}}


def made(js):
    """constructJobsFromTemplate per replicatedJob: {replicatedJob name: [Job]}."""
    return {rj["name"]: host.constructJobsFromTemplate(js, rj, {}) for rj in js["spec"]["replicatedJobs"]}


TRAIN = jobset("train", "default", [rjob("w", 3, 2), rjob("big", 2, 6)], {EXCL: "rack"})


def the_jobs():
    train = made(TRAIN)
    plain = made(jobset("plain", "default", [rjob("x", 1, 2)], {}))
    solo = made(jobset("solo", "default", [rjob("w", 2, 2)], {EXCL: "rack"}))
    nsel = made(jobset("nsel", "team-b", [rjob("x", 1, 2)], {EXCL: "rack", NODE_SELECTOR: "true"}))
    evl = made(jobset("eval", "team-b", [rjob("zonal", 1, 4, key="zone"), rjob("small", 1, 1)], {EXCL: "rack"}))
    w, big = train["w"], train["big"]
    return [w[0], big[0], w[1], big[1], w[2]] + plain["x"] + solo["w"] + nsel["x"] + evl["zonal"] + evl["small"]


def many_classes(n):
    """n one-job JobSets, each its own requirement class (the class key is replicated job + topology key)."""
    out = []
    for i in range(n):
        out += made(jobset(f"c{i}", "default", [rjob(f"r{i}", 1, 1)], {EXCL: "rack"}))[f"r{i}"]
    return out


def run(engine=None):
    """The sequence on a fresh cache; engine=None: the host-only planner."""
    out = []
    c, bare = host.Cache(), host.Cache()

    def call(label, method, cache=c, **req):
        r, e = host.call(method, cache=cache.id, **req)
        out.append([label, r, e])
        return r

    try:
        for (z, r), n in sorted(RACK_NODES.items()):
            for i in range(n):
                tainted = (z, r, i) == (0, 0, 7)
                c.add_node(node(z, r, i, [{"key": "maintenance", "value": "", "effect": "NoSchedule"}] if tainted else ()))
        c.add_pod(pod("other-0-abcde", "elsewhere", "foreign-key", "z0-r1-n0"))
        c.planner_new(engine, LEVELS, RES)
        jobs = the_jobs()
        name = [j["metadata"]["name"] for j in jobs]
        assert name == ["train-w-0", "train-big-0", "train-w-1", "train-big-1", "train-w-2", "plain-x-0", "solo-w-0",
                        "solo-w-1", "nsel-x-0", "eval-zonal-0", "eval-small-0"], name

        call("encode", "planner.encode", jobs=jobs)
        call("plan", "planner.plan", jobs=jobs)
        # kept (free rack), moved (the held rack), lost (a rack too small for 6 pods and nowhere else to go),
        # a value no domain has, a name that is not a job; the other jobs are absent
        call("plan previous", "planner.plan", jobs=jobs,
             previous={"train-w-0": R00, "train-w-1": R01, "train-big-0": R10, "solo-w-0": "zone-9-rack-9", "nobody": R00})
        call("explain", "planner.explain", jobs=jobs)
        call("gangs", "planner.planGangs", jobs=jobs, spans={})
        call("gangs zone and rack span", "planner.planGangs", jobs=jobs, spans={"default/solo": "zone", "default/train": "rack"})
        call("gangs span refuses solo", "planner.planGangs", jobs=jobs, spans={"default/solo": "rack"})
        call("gangs adjacent of one class", "planner.planGangs", jobs=[jobs[0], jobs[2], jobs[6], jobs[7]], spans={})
        for p in POLICIES:
            call("fit " + p, "planner.planFit", jobs=jobs, policy=p)
        # a plan as planner.plan replies it (null domains and all), one job on the held rack
        call("bind plan", "planner.bind", jobs=jobs, assignment={"jobs": [
            {"name": "train-w-0", "topologyKey": "rack", "domainId": 0, "domain": R00},
            {"name": "train-big-0", "topologyKey": "rack", "domainId": -1, "domain": None},
            {"name": "train-w-1", "topologyKey": "rack", "domainId": 2, "domain": R10},
            {"name": "train-w-2", "topologyKey": "rack", "domainId": 1, "domain": R01},
            {"name": "eval-small-0", "topologyKey": "rack", "domainId": 3, "domain": R11}], "placed": 4})
        call("bind map", "planner.bind", jobs=jobs,
             assignment={"train-big-0": R00, "eval-zonal-0": "zone-1", "solo-w-0": R01, "nobody": R10})
        call("bind unknown value", "planner.bind", jobs=jobs,
             assignment={"train-w-0": "zone-9-rack-9", "train-w-1": R11, "train-w-2": "zone-1", "solo-w-1": 3})
        held = {"jobs": [{"name": "train-w-0", "domain": R00}, {"name": "train-big-0", "domain": None},
                         {"name": "train-w-1", "domain": R11}, {"name": "train-w-2", "domain": R01},
                         {"name": "eval-small-0", "domain": R10}]}
        call("assume plan", "planner.assume", jobs=jobs, assignment=held)
        call("assume again", "planner.assume", jobs=jobs, assignment=held)
        # train-w-0's leader shows up: the sync confirms its hold
        c.add_pod(pod("train-w-0-0-abcde", "default", host.jobHashKey("default", "train-w-0"), "z0-r0-n0"))
        call("sync", "planner.sync")
        call("forget", "planner.forget", jobs=["train-w-1", "nobody"])
        c.add_pod(pod("train-w-0-1-abcde", "default", host.jobHashKey("default", "train-w-0"), "z0-r0-n1"))
        call("plan after assume", "planner.plan", jobs=jobs)
        # the recreate: the tainted node is gone (another row set: a full upload), eval-small-0's hold stays
        c.remove_node("z0-r0-n7")
        js1 = host.failurePolicyRecreateAll(TRAIN, True)
        call("recreate previousPlan", "controllers.reconcileRecreate", jobSet=js1, jobs=[], previousPlan={"jobs": [
            {"name": "train-w-1", "domain": R11}, {"name": "train-w-0", "domain": R00},
            {"name": "train-big-1", "domain": None}, {"name": "train-w-2", "domain": "zone-9-rack-9"}]})
        old = made(TRAIN)["w"][1]
        assert old["metadata"]["labels"][RESTARTS] == "0"
        call("recreate while deleting", "controllers.reconcileRecreate", jobSet=js1, jobs=[old], previousPlan={"jobs": []})

        # ---- errors
        for m, req in (("planner.plan", {}), ("planner.explain", {}), ("planner.planGangs", {"spans": {}}),
                       ("planner.planFit", {"policy": "lowest"}), ("planner.bind", {"assignment": {}}),
                       ("planner.assume", {"assignment": {}}), ("planner.encode", {})):
            call("no planner: " + m, m, cache=bare, jobs=jobs, **req)
        call("no planner: planner.forget", "planner.forget", cache=bare, jobs=[])
        call("no planner: planner.sync", "planner.sync", cache=bare)
        call("no planner: planner.columns", "planner.columns", cache=bare)
        call("no planner: hack.labelNodes", "hack.labelNodes", cache=bare, jobSet=TRAIN)
        # jobClasses' errors come before the sync: the pod added here is still unsynced after them
        c.add_pod(pod("train-w-0-2-abcde", "default", host.jobHashKey("default", "train-w-0"), "z0-r0-n2"))
        crowd = many_classes(65)
        rowed = made(jobset("rowed", "default", [rjob("r", 1, 1)], {EXCL: "row"}))["r"]
        for m, req in (("planner.plan", {}), ("planner.planGangs", {"spans": {}}), ("planner.planFit", {"policy": "lowest"}),
                       ("planner.bind", {"assignment": {}}), ("planner.assume", {"assignment": {}}), ("planner.encode", {})):
            call("65 classes: " + m, m, jobs=crowd, **req)
            call("unknown key: " + m, m, jobs=jobs + rowed, **req)
        call("sync after class errors", "planner.sync")
        call("span not a level", "planner.planGangs", jobs=jobs, spans={"default/solo": "row"})
        call("span finer than key", "planner.planGangs", jobs=jobs, spans={"team-b/eval": "rack"})
        call("fit bad policy", "planner.planFit", jobs=crowd, policy="snug")
        call("fit no policy", "planner.planFit", jobs=crowd)
        call("bind assignment a number", "planner.bind", jobs=jobs, assignment=7)
        call("bind assignment missing", "planner.bind", jobs=jobs)
        call("assume assignment a list", "planner.assume", jobs=jobs, assignment=[R00])
        call("assume assignment missing", "planner.assume", jobs=jobs)
        call("forget a number", "planner.forget", jobs=["eval-small-0", 3])
        call("forget no array", "planner.forget", jobs="eval-small-0")
        out.append(["engineCalls", c.stats()["engineCalls"], None])
        out.append(["engineCalls without a planner", bare.stats()["engineCalls"], None])
    finally:
        c.close()
        bare.close()
    return out


def dump(entries) -> str:
    """One entry per line: a recording's diff names the calls that moved."""
    return "[\n" + ",\n".join(json.dumps(e, sort_keys=True, separators=(",", ":")) for e in entries) + "\n]\n"


def load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", metavar="PATH", required=True)
    ap.add_argument("--engine", action="store_true", help="bind an engine on GPU 0 (default: the host-only planner)")
    a = ap.parse_args()
    if a.engine:
        from jobset_amd.engine import Engine
        with Engine(0) as eng:
            entries = run(eng)
    else:
        entries = run(None)
    with open(a.record, "w") as f:
        f.write(dump(entries))
    print(f"{len(entries)} entries -> {a.record}")


if __name__ == "__main__":
    main()
