/*
 * jsk_host.h — C ABI of the host-side mirror of JobSet's exclusive-placement
 * path (webhook mutation/admission, leader PodReconciler, child-Job
 * construction and restart bucketing, placement utilities). One JSON call
 * entry point keeps the boundary to plain pointers: `method` names the
 * reference function ("webhooks.Default", "controllers.validatePodPlacements",
 * "placement.GenJobName", ...; full list in
 * jobset_amd/csrc/host/jobset_host.cc:dispatch), `request_json` carries its
 * arguments as Kubernetes objects in JSON, and the response is
 * {"result": ..., "error": "<Go error text>"} (error absent on success).
 * Beside the mirrored functions the placement planner has its own methods
 * ("planner.plan", "planner.explain", "planner.planGangs": planner.plan's jobs
 * placed JobSet by JobSet, each whole inside one domain of the topology key
 * "spans" names for it or not at all, jsp_place_gangs; "planner.planFit":
 * planner.plan's jobs plus "policy": "lowest" | "tightest" | "roomiest", every
 * job on the free feasible domain of the least / the most pod capacity,
 * jsp_place_fit; "planner.whatIf": planner.plan's jobs plus "scenarios":
 * [{"name", "evict": [job keys]}], the plan as it is and, per scenario, as it
 * would be without those jobs' pods and assumed domains, nothing written,
 * jsp_place_whatif; "planner.preempt": planner.plan's jobs plus "priority"
 * (int32), placed where exclusive jobs whose pods all have a lower
 * spec.priority would be evicted, with the victims' job keys per job and
 * "evict" in all, nothing written, jsp_place_preempt; "planner.planSpread":
 * planner.plan's jobs plus "topologyKey", "maxSkew" and "whenUnsatisfiable"
 * ("DoNotSchedule" | "ScheduleAnyway"), spread evenly over the key's domains
 * with the JobSets' running and assumed jobs (or "peers": [job keys]) counted
 * as placed, the key's domain per job and the jobs per domain in the reply,
 * jsp_place_spread; "planner.bind": a plan's
 * domains -> the
 * node per completion index of every job, jsp_bind_pods; "planner.assume":
 * planner.bind's request -> the jobs' domains held in the engine's snapshot
 * (jsp_assume) and in the planner's ledger until a sync sees their pods or
 * "planner.forget" {"jobs": [names]} frees them, jsp_forget).
 *
 * Reference interfaces mirrored (file:line):
 *   pkg/webhooks/pod_mutating_webhook.go:64-194, pod_admission_webhook.go:24-161
 *   pkg/controllers/pod_controller.go:66-327
 *   pkg/controllers/jobset_controller.go:267-305, 638-818, 1034-1065
 *   pkg/controllers/failure_policy.go:155-175
 *   pkg/util/placement/placement.go:14-28
 *   hack/label_nodes/label_nodes.py:99-112
 */
#ifndef JSK_HOST_H
#define JSK_HOST_H

#ifdef __cplusplus
extern "C" {
#endif

/* Returns 0, or JSP_EINVAL (-1) for malformed JSON / unknown method (the
 * response then holds {"error": ...}), or JSP_ENOMEM. *response_json is
 * malloc'd: release it with jsk_free. */
int jsk_call(const char* method, const char* request_json, char** response_json);
void jsk_free(char* p);

#ifdef __cplusplus
}
#endif
#endif /* JSK_HOST_H */
