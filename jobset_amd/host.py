"""Python face of the host-side mirror (include/jsk_host.h): the reference's
pod webhook, leader PodReconciler, child-Job construction and placement
utilities, with the Go function names. Each call goes through the C ABI into
jobset_amd/csrc/host/jobset_host.cc; objects are Kubernetes JSON dicts.
"""
from __future__ import annotations

import ctypes
import json
from typing import Any, Dict, List, Optional, Tuple

from . import native

_bound = False


def _lib():
    global _bound
    lib = native.lib()
    if not _bound:
        lib.jsk_call.restype = ctypes.c_int
        lib.jsk_call.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        lib.jsk_free.restype = None
        lib.jsk_free.argtypes = [ctypes.c_void_p]
        _bound = True
    return lib


class HostCallError(RuntimeError):
    pass


def call(method: str, **req: Any) -> Tuple[Any, Optional[str]]:
    """Returns (result, go_error_text_or_None)."""
    lib = _lib()
    out = ctypes.c_void_p()
    rc = lib.jsk_call(method.encode(), json.dumps(req).encode(), ctypes.byref(out))
    try:
        text = ctypes.string_at(out.value).decode() if out.value else "{}"
    finally:
        if out.value:
            lib.jsk_free(out.value)
    resp = json.loads(text)
    if rc != 0:
        raise HostCallError(resp.get("error", f"jsk_call rc={rc}"))
    return resp.get("result"), resp.get("error")


# ---------------------------------------------------------------- stateless helpers
def GenJobName(js: str, rjob: str, idx: int) -> str:
    return call("placement.GenJobName", jsName=js, rjobName=rjob, jobIndex=idx)[0]


def GenPodName(js: str, rjob: str, job_idx: str, pod_idx: str) -> str:
    return call("placement.GenPodName", jobSet=js, replicatedJob=rjob, jobIndex=job_idx, podIndex=pod_idx)[0]


def IsLeaderPod(pod: dict) -> bool:
    return call("placement.IsLeaderPod", pod=pod)[0]


def explainMessage(counts: dict, topology_key: str, pods: int, resources: List[str], value: str = "") -> str:
    """The operator's line for one class's jsp_explain counts;
    `value`: the best short domain's topology value. No engine call."""
    return call("placement.explainMessage", counts=counts, topologyKey=topology_key, pods=pods,
                resources=resources, value=value)[0]


def jobHashKey(ns: str, job: str) -> str:
    return call("controllers.jobHashKey", ns=ns, jobName=job)[0]


def sha1Hash(s: str) -> str:
    return call("controllers.sha1Hash", s=s)[0]


def namespacedJobName(ns: str, job: str) -> str:
    return call("controllers.namespacedJobName", ns=ns, jobName=job)[0]


def globalJobIndex(js: dict, rjob: str, idx: int) -> str:
    return call("controllers.globalJobIndex", jobSet=js, replicatedJob=rjob, jobIdx=idx)[0]


def removePodNameSuffix(name: str):
    return call("controllers.removePodNameSuffix", podName=name)


def constructJob(js: dict, rjob: dict, idx: int) -> dict:
    return call("controllers.constructJob", jobSet=js, replicatedJob=rjob, jobIdx=idx)[0]


def constructJobsFromTemplate(js: dict, rjob: dict, owned: Optional[dict] = None) -> List[dict]:
    return call("controllers.constructJobsFromTemplate", jobSet=js, replicatedJob=rjob, ownedJobs=owned or {})[0]


def shouldCreateJob(name: str, owned: dict) -> bool:
    return call("controllers.shouldCreateJob", jobName=name, ownedJobs=owned)[0]


def getChildJobs(js: dict, jobs: List[dict]):
    return call("controllers.getChildJobs", jobSet=js, jobs=jobs)


def failurePolicyRecreateAll(js: dict, should_count: bool) -> dict:
    return call("controllers.failurePolicyRecreateAll", jobSet=js, shouldCountTowardsMax=should_count)[0]


def followerPodTopology(pod: dict, key: str):
    return call("controllers.followerPodTopology", pod=pod, topologyKey=key)


def updatePodCondition(pod: dict, cond: dict):
    r = call("controllers.updatePodCondition", pod=pod, condition=cond)[0]
    return r["changed"], r["pod"]


def podIndexes(pod: dict) -> Dict[str, List[str]]:
    return call("controllers.podIndexes", pod=pod)[0]


def podPredicate(pod: dict) -> bool:
    return call("controllers.podPredicate", pod=pod)[0]


def genLeaderPodName(pod: dict):
    return call("webhooks.genLeaderPodName", pod=pod)


def podsOwnedBySameJob(leader: dict, follower: dict) -> Optional[str]:
    return call("webhooks.podsOwnedBySameJob", leaderPod=leader, followerPod=follower)[1]


def setExclusiveAffinities(pod: dict) -> dict:
    return call("webhooks.setExclusiveAffinities", pod=pod)[0]


def generateNamespacedJobs(js: dict) -> List[str]:
    return call("hack.generateNamespacedJobs", jobSet=js)[0]


# ---------------------------------------------------------------- cached client + webhook/reconciler
class Cache:
    """The controller-runtime cached client the webhook and reconciler read
    (pods with the podName / podJobKey field indexes, nodes), with
    injectable errors like the reference tests' interceptor.Funcs."""

    def __init__(self):
        self.id = call("cache.new")[0]

    def close(self):
        if self.id is not None:
            call("cache.free", cache=self.id)
            self.id = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_pod(self, pod: dict):
        call("cache.add", cache=self.id, kind="Pod", object=pod)

    def add_node(self, node: dict):
        call("cache.add", cache=self.id, kind="Node", object=node)

    def inject(self, what: str, error: Optional[str]):
        """what: "get/Node", "get/Pod", "list/Pod", "update/Pod" (status), "delete/Pod"."""
        call("cache.inject", cache=self.id, what=what, error=error)

    def stats(self) -> dict:
        return call("cache.stats", cache=self.id)[0]

    def bind_engine(self, engine, node_rows: Dict[str, int], level_keys: List[str], domain_values: List[List[str]]):
        """Answer topologyFromPod from the engine's resident snapshot."""
        call("cache.bindEngine", cache=self.id, engine=engine._h.value, nodeRows=node_rows, levelKeys=level_keys,
             domainValues=domain_values)

    # webhook (pkg/webhooks)
    def Default(self, pod: dict):
        return call("webhooks.Default", cache=self.id, pod=pod)

    def ValidateCreate(self, pod: dict) -> Optional[str]:
        return call("webhooks.ValidateCreate", cache=self.id, pod=pod)[1]

    def leaderPodForFollower(self, pod: dict):
        return call("webhooks.leaderPodForFollower", cache=self.id, pod=pod)

    # PodReconciler (pkg/controllers/pod_controller.go)
    def validatePodPlacements(self, leader: dict, pods: List[dict]):
        return call("controllers.validatePodPlacements", cache=self.id, leaderPod=leader, podList=pods)

    def deleteFollowerPods(self, pods: List[dict], now: str = "2024-10-08T00:00:00Z") -> Optional[str]:
        return call("controllers.deleteFollowerPods", cache=self.id, pods=pods, now=now)[1]

    def Reconcile(self, ns: str, name: str, now: str = "2024-10-08T00:00:00Z") -> Optional[str]:
        return call("controllers.Reconcile", cache=self.id, namespace=ns, name=name, now=now)[1]

    def remove_pod(self, ns: str, name: str):
        call("cache.remove", cache=self.id, kind="Pod", namespace=ns, name=name)

    def remove_node(self, name: str):
        call("cache.remove", cache=self.id, kind="Node", name=name)

    # placement planner (jobset_amd/csrc/host/placement.h): the engine's snapshot
    # built from this cache's Node / Pod objects
    def planner_new(self, engine, level_keys: List[str], resources: List[str]):
        """engine=None: a host-only planner (ingestion without uploads)."""
        call("planner.new", cache=self.id, engine=engine._h.value if engine is not None else 0,
             levelKeys=level_keys, resources=resources)

    def _ok(self, method: str, **req):
        r, e = call(method, cache=self.id, **req)
        if e is not None:
            raise HostCallError(e)
        return r

    def planner_sync(self) -> dict:
        return self._ok("planner.sync")

    def planner_columns(self) -> dict:
        return self._ok("planner.columns")

    def planner_encode(self, jobs: List[dict]) -> dict:
        return self._ok("planner.encode", jobs=jobs)

    def plan(self, jobs: List[dict], previous: Optional[Dict[str, str]] = None):
        """previous: job name -> the topology value of the domain it held
        before (jsp_place_sticky): a job whose previous domain is still
        feasible keeps it. Each job then also reports "previousDomain" and
        "kept", the plan "hinted", "kept", "moved" and "lost"."""
        if previous is None:
            return call("planner.plan", cache=self.id, jobs=jobs)
        return call("planner.plan", cache=self.id, jobs=jobs, previous=previous)

    def planGangs(self, jobs: List[dict], spans: Optional[Dict[str, str]] = None):
        """planner.planGangs: plan()'s jobs placed JobSet by JobSet
        (jsp_place_gangs): each maximal run of consecutive jobs of one
        "<namespace>/<jobset name>" lands whole or not at all, inside one
        domain of the topology key spans names for it (no entry: anywhere).
        The reply is plan()'s plus "jobSet" per job, "jobSets" ({"name",
        "spanKey", "spanDomain", "placed"} per gang) and "gangsPlaced"."""
        return call("planner.planGangs", cache=self.id, jobs=jobs, spans=spans or {})

    def planFit(self, jobs: List[dict], policy: str):
        """planner.planFit: plan()'s jobs placed by jsp_place_fit under policy
        "lowest" (plan()'s answer), "tightest" (every job on the free feasible
        domain with the least pod capacity that still fits) or "roomiest" (the
        most); any other policy is an error that names it. The reply is
        plan()'s plus "policy" and "slack"."""
        return call("planner.planFit", cache=self.id, jobs=jobs, policy=policy)

    def whatIf(self, jobs: List[dict], scenarios: List[dict]):
        """planner.whatIf: plan()'s jobs placed under hypothetical evictions
        (jsp_place_whatif; nothing is written). scenarios: [{"name": ...,
        "evict": [job keys]}] -- the job-key label values (jobHashKey) of the
        jobs to think away, their bound pods and their assumed domains with
        them; an unknown key is an error that names it. The reply is plan()'s
        (the unedited answer) plus "scenarios": per scenario "name", "jobs",
        "placed", "unplaceable", "flips" and "rows"."""
        return call("planner.whatIf", cache=self.id, jobs=jobs, scenarios=scenarios)

    def preempt(self, jobs: List[dict], priority: int):
        """planner.preempt: plan()'s jobs placed at `priority` (an int32, as a
        pod's spec.priority) by jsp_place_preempt; nothing is written. An
        exclusive job whose bound pods all carry a lower spec.priority
        (absent: 0) may be evicted; one at or above it, and a domain held by
        assume(), blocks. The reply is plan()'s plus "victims" per job (the
        job keys to evict for it) and "evict", those keys sorted, each once."""
        return call("planner.preempt", cache=self.id, jobs=jobs, priority=priority)

    def plan_spread(self, jobs: List[dict], topology_key: str, max_skew: int = 1,
                    when_unsatisfiable: str = "DoNotSchedule", peers: Optional[List[str]] = None):
        """planner.planSpread: plan()'s jobs spread evenly over the domains of
        `topology_key` by jsp_place_spread, as a topologySpreadConstraints
        entry asks: "DoNotSchedule" leaves a job unplaced that would put its
        domain more than max_skew ahead of the emptiest eligible one,
        "ScheduleAnyway" never does. The jobs that count as already placed are
        the exclusive jobs of the same JobSets that hold domains by the
        cache's pods or by assume(), or exactly the job keys in `peers`. The
        reply is plan()'s plus "spreadDomain" per job, "peers", "counts"
        (domain value -> jobs), "refused" and "skew"."""
        kw = dict(cache=self.id, jobs=jobs, topologyKey=topology_key, maxSkew=max_skew,
                  whenUnsatisfiable=when_unsatisfiable)
        if peers is not None:
            kw["peers"] = peers
        return call("planner.planSpread", **kw)

    def bind(self, jobs: List[dict], assignment: dict):
        """planner.bind: the jobs of plan() plus their assignment -- a plan()
        reply, or job name -> the topology value of its domain. Per job its
        "domain", "bound" and "nodes": the node name per completion index
        (jsp_bind_pods), None for an unbound pod."""
        return call("planner.bind", cache=self.id, jobs=jobs, assignment=assignment)

    def assume(self, jobs: List[dict], assignment: dict):
        """planner.assume: bind()'s request. The jobs whose domains are
        feasible now are held (jsp_assume): a later plan() does not hand their
        domains out again, across syncs and full uploads, until a sync sees a
        job's pods or forget() names it. Per job "committed" and "owner"."""
        return call("planner.assume", cache=self.id, jobs=jobs, assignment=assignment)

    def forget(self, names: List[str]):
        """planner.forget: the named jobs' holds are dropped and their rows
        freed (jsp_forget); "rowsCleared", "forgotten", "assumed"."""
        return call("planner.forget", cache=self.id, jobs=list(names))

    def explain(self, jobs: List[dict]):
        """planner.plan plus "explanations": per class with an unplaceable
        job, {"class", "jobs", "counts", "message"}."""
        return call("planner.explain", cache=self.id, jobs=jobs)

    def reconcileRecreate(self, js: dict, jobs: List[dict], previous_plan: Optional[dict] = None):
        """previous_plan: the "plan" of an earlier reply; its jobs keep their
        domains where they still can."""
        if previous_plan is None:
            return call("controllers.reconcileRecreate", cache=self.id, jobSet=js, jobs=jobs)
        return call("controllers.reconcileRecreate", cache=self.id, jobSet=js, jobs=jobs, previousPlan=previous_plan)

    def labelNodes(self, js: dict):
        return call("hack.labelNodes", cache=self.id, jobSet=js)

    def DefaultBatch(self, pods: List[dict]) -> List[Tuple[dict, Optional[str]]]:
        r = call("webhooks.DefaultBatch", cache=self.id, pods=pods)[0]
        return [(x["pod"], x["error"]) for x in r]
