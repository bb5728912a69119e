// jobset_host.cc — host-side mirror of the reference's exclusive-placement
// path around the engine: the pod webhook (mutation + admission), the leader
// PodReconciler, the child-Job construction / restart bucketing slice of the
// JobSet reconciler, and the placement utilities. Same function names,
// argument meaning and error strings as the Go reference (file:line at each
// function), over Kubernetes objects as JSON (what an AdmissionReview
// carries). The reference's controller-runtime cached client is a small
// in-memory store with the same field indexes and injectable errors (the
// reference's unit tests use controller-runtime's fake client with
// interceptor.Funcs the same way, pkg/controllers/pod_controller_test.go:171-184).
//
// The engine is consulted, behind the unchanged mutation, for the follower's
// topology value (batched A5) and the placement audit (batched A9) when a
// cache is bound to an engine (cache.bindEngine).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../../include/jsk_host.h"
#include "../../../include/jsplace.h"
#include "json.h"
#include "placement.h"
#include "sha1.h"

namespace jsk {

// ---- api/jobset/v1alpha2/jobset_types.go:22-58, pkg/constants/constants.go
const char* const kJobSetNameKey = "jobset.sigs.k8s.io/jobset-name";
const char* const kReplicatedJobReplicas = "jobset.sigs.k8s.io/replicatedjob-replicas";
const char* const kReplicatedJobNameKey = "jobset.sigs.k8s.io/replicatedjob-name";
const char* const kJobIndexKey = "jobset.sigs.k8s.io/job-index";
const char* const kJobGlobalIndexKey = "jobset.sigs.k8s.io/job-global-index";
const char* const kJobKey = "jobset.sigs.k8s.io/job-key";
const char* const kExclusiveKey = "alpha.jobset.sigs.k8s.io/exclusive-topology";
const char* const kNodeSelectorStrategyKey = "alpha.jobset.sigs.k8s.io/node-selector";
const char* const kNamespacedJobKey = "alpha.jobset.sigs.k8s.io/namespaced-job";
const char* const kNoScheduleTaintKey = "alpha.jobset.sigs.k8s.io/no-schedule";
const char* const kCoordinatorKey = "jobset.sigs.k8s.io/coordinator";
const char* const kRestartsKey = "jobset.sigs.k8s.io/restart-attempt";
const char* const kJobCompletionIndexAnnotation = "batch.kubernetes.io/job-completion-index";
const char* const kExclusivePlacementViolationReason = "ExclusivePlacementViolation";
const char* const kExclusivePlacementViolationMessage = "Pod violated JobSet exclusive placement policy";
const char* const kPodNameKey = "podName";      // pkg/controllers/pod_controller.go:43
const char* const kPodJobKey = "podJobKey";     // pkg/controllers/pod_controller.go:48

// ---- Go-like error value
struct Err {
    bool ok = true;
    bool not_found = false;
    std::string msg;
    static Err none() { return Err(); }
    static Err e(std::string m) { Err r; r.ok = false; r.msg = std::move(m); return r; }
    static Err nf(std::string m) { Err r = e(std::move(m)); r.not_found = true; return r; }
};

// fmt %q of a string (strconv.Quote for the ASCII range)
std::string go_quote(const std::string& s) {
    std::string o = "\"";
    for (unsigned char c : s) {
        if (c == '"') o += "\\\"";
        else if (c == '\\') o += "\\\\";
        else if (c == '\n') o += "\\n";
        else if (c == '\t') o += "\\t";
        else if (c == '\r') o += "\\r";
        else if (c < 0x20 || c == 0x7f) {
            char b[8];
            std::snprintf(b, sizeof b, "\\x%02x", c);
            o += b;
        } else o += (char)c;
    }
    return o + "\"";
}

std::string errors_join(const std::vector<std::string>& errs) {  // errors.Join
    std::string o;
    for (size_t i = 0; i < errs.size(); ++i) o += (i ? "\n" : "") + errs[i];
    return o;
}

// ---- object accessors
const Json& meta(const Json& o) { return o.get("metadata"); }
const Json& labels(const Json& o) { return meta(o).get("labels"); }
const Json& annotations(const Json& o) { return meta(o).get("annotations"); }
std::string name_of(const Json& o) { return meta(o).get("name").as_string(); }
std::string ns_of(const Json& o) { return meta(o).get("namespace").as_string(); }
std::string node_name(const Json& pod) { return pod.get("spec").get("nodeName").as_string(); }

// metav1.GetControllerOf: the owner reference with controller == true
const Json* controller_of(const Json& o) {
    for (const auto& r : meta(o).get("ownerReferences").elems())
        if (r.get("controller").as_bool()) return &r;
    return nullptr;
}

Json clone_map(const Json& m) { return m.is_object() ? m : Json::object(); }  // collections.CloneMap

// ============================================================ pkg/util/placement/placement.go
// GenJobName, placement.go:14-16
std::string GenJobName(const std::string& js, const std::string& rjob, int64_t idx) {
    return js + "-" + rjob + "-" + std::to_string(idx);
}
// GenPodName, placement.go:20-22
std::string GenPodName(const std::string& js, const std::string& rjob, const std::string& jobIdx,
                       const std::string& podIdx) {
    return js + "-" + rjob + "-" + jobIdx + "-" + podIdx;
}
// IsLeaderPod, placement.go:26-28
bool IsLeaderPod(const Json& pod) { return str_at(annotations(pod), kJobCompletionIndexAnnotation) == "0"; }

// ============================================================ pkg/controllers/jobset_controller.go
// sha1Hash / jobHashKey, :809-818
std::string sha1Hash(const std::string& s) { return sha1_hex(s); }
std::string jobHashKey(const std::string& ns, const std::string& jobName) { return sha1Hash(ns + "/" + jobName); }
// namespacedJobName, :804-806
std::string namespacedJobName(const std::string& ns, const std::string& job) { return ns + "_" + job; }

// globalJobIndex, :1056-1065
std::string globalJobIndex(const Json& js, const std::string& rjobName, int64_t jobIdx) {
    int64_t total = 0;
    for (const auto& rj : js.get("spec").get("replicatedJobs").elems()) {
        if (rj.get("name").as_string() == rjobName) return std::to_string(total + jobIdx);
        total += rj.get("replicas").as_int();
    }
    return "";
}

// GetSubdomain, :790-798
std::string GetSubdomain(const Json& js) {
    const std::string sd = js.get("spec").get("network").get("subdomain").as_string();
    return sd.empty() ? name_of(js) : sd;
}
bool dnsHostnamesEnabled(const Json& js) { return js.get("spec").get("network").get("enableDNSHostnames").as_bool(); }
bool jobSetSuspended(const Json& js) { return js.get("spec").get("suspend").as_bool(); }

// coordinatorEndpoint, :1034-1036
std::string coordinatorEndpoint(const Json& js) {
    const Json& c = js.get("spec").get("coordinator");
    return name_of(js) + "-" + c.get("replicatedJob").as_string() + "-" + std::to_string(c.get("jobIndex").as_int()) +
           "-" + std::to_string(c.get("podIndex").as_int()) + "." + GetSubdomain(js);
}

// labelAndAnnotateObject, :722-770 (A1: the exclusive-topology block is :751-766)
void labelAndAnnotateObject(Json& objMeta, const Json& js, const Json& rjob, int64_t jobIdx) {
    const std::string jsName = name_of(js), rjName = rjob.get("name").as_string();
    const std::string jobName = GenJobName(jsName, rjName, jobIdx);
    const std::string restarts = std::to_string(js.get("status").get("restarts").as_int());
    const std::string replicas = std::to_string(rjob.get("replicas").as_int());
    const std::string key = jobHashKey(ns_of(js), jobName);
    const std::string gidx = globalJobIndex(js, rjName, jobIdx);
    Json lab = clone_map(objMeta.get("labels"));
    Json ann = clone_map(objMeta.get("annotations"));
    for (Json* m : {&lab, &ann}) {
        (*m)[kJobSetNameKey] = jsName;
        (*m)[kReplicatedJobNameKey] = rjName;
        (*m)[kRestartsKey] = restarts;
        (*m)[kReplicatedJobReplicas] = replicas;
        (*m)[kJobIndexKey] = std::to_string(jobIdx);
        (*m)[kJobKey] = key;
        (*m)[kJobGlobalIndexKey] = gidx;
    }
    if (!js.get("spec").get("coordinator").is_null()) {
        lab[kCoordinatorKey] = coordinatorEndpoint(js);
        ann[kCoordinatorKey] = coordinatorEndpoint(js);
    }
    // JobSet-level exclusive placement
    const Json& jsAnn = annotations(js);
    if (has_key(jsAnn, kExclusiveKey)) {
        ann[kExclusiveKey] = str_at(jsAnn, kExclusiveKey);
        if (has_key(jsAnn, kNodeSelectorStrategyKey)) ann[kNodeSelectorStrategyKey] = str_at(jsAnn, kNodeSelectorStrategyKey);
    }
    // ReplicatedJob-level exclusive placement (overrides)
    const Json& rjAnn = rjob.get("template").get("metadata").get("annotations");
    if (has_key(rjAnn, kExclusiveKey)) {
        ann[kExclusiveKey] = str_at(rjAnn, kExclusiveKey);
        if (has_key(rjAnn, kNodeSelectorStrategyKey)) ann[kNodeSelectorStrategyKey] = str_at(rjAnn, kNodeSelectorStrategyKey);
    }
    objMeta["labels"] = lab;
    objMeta["annotations"] = ann;
}

// addNamespacedJobNodeSelector, :795-800; addTaintToleration, :688-696
void addNamespacedJobNodeSelector(Json& job) {
    Json& ps = job["spec"]["template"]["spec"];
    if (!ps.get("nodeSelector").is_object()) ps["nodeSelector"] = Json::object();
    ps["nodeSelector"][kNamespacedJobKey] = namespacedJobName(ns_of(job), name_of(job));
}
void addTaintToleration(Json& job) {
    Json& ps = job["spec"]["template"]["spec"];
    Json t = Json::object();
    t["key"] = kNoScheduleTaintKey;
    t["operator"] = "Exists";
    t["effect"] = "NoSchedule";
    if (!ps.get("tolerations").is_array()) ps["tolerations"] = Json::array();
    ps["tolerations"].push_back(t);
}

// constructJob, :651-686
Json constructJob(const Json& js, const Json& rjob, int64_t jobIdx) {
    const Json& tmpl = rjob.get("template");
    Json job = Json::object();
    job["metadata"]["labels"] = clone_map(tmpl.get("metadata").get("labels"));
    job["metadata"]["annotations"] = clone_map(tmpl.get("metadata").get("annotations"));
    job["metadata"]["name"] = GenJobName(name_of(js), rjob.get("name").as_string(), jobIdx);
    job["metadata"]["namespace"] = ns_of(js);
    job["spec"] = tmpl.get("spec").is_object() ? tmpl.get("spec") : Json::object();
    labelAndAnnotateObject(job["metadata"], js, rjob, jobIdx);
    labelAndAnnotateObject(job["spec"]["template"]["metadata"], js, rjob, jobIdx);
    if (dnsHostnamesEnabled(js)) job["spec"]["template"]["spec"]["subdomain"] = GetSubdomain(js);
    const Json& ann = job.get("metadata").get("annotations");
    if (has_key(ann, kExclusiveKey) && has_key(ann, kNodeSelectorStrategyKey)) {
        addNamespacedJobNodeSelector(job);
        addTaintToleration(job);
    }
    job["spec"]["suspend"] = jobSetSuspended(js);
    return job;
}

// shouldCreateJob, :698-709
bool shouldCreateJob(const std::string& jobName, const Json& owned) {
    for (const char* b : {"active", "successful", "failed", "delete"})
        for (const auto& j : owned.get(b).elems())
            if (name_of(j) == jobName) return false;
    return true;
}

// constructJobsFromTemplate, :638-649
Json constructJobsFromTemplate(const Json& js, const Json& rjob, const Json& owned) {
    Json jobs = Json::array();
    for (int64_t i = 0; i < rjob.get("replicas").as_int(); ++i) {
        const std::string n = GenJobName(name_of(js), rjob.get("name").as_string(), i);
        if (!shouldCreateJob(n, owned)) continue;
        jobs.push_back(constructJob(js, rjob, i));
    }
    return jobs;
}

// JobFinished, :772-779
std::string jobFinishedType(const Json& job) {
    for (const auto& c : job.get("status").get("conditions").elems()) {
        const std::string t = c.get("type").as_string();
        if ((t == "Complete" || t == "Failed") && c.get("status").as_string() == "True") return t;
    }
    return "";
}

// getChildJobs bucketing, :267-305 (restart attempts older than status.restarts -> delete)
Err getChildJobs(const Json& js, const Json& jobs, Json* out) {
    Json b = Json::object();
    for (const char* k : {"active", "successful", "failed", "delete"}) b[k] = Json::array();
    const int64_t restarts = js.get("status").get("restarts").as_int();
    for (const auto& job : jobs.elems()) {
        const std::string v = str_at(labels(job), kRestartsKey);
        char* end = nullptr;
        const long r = std::strtol(v.c_str(), &end, 10);
        if (v.empty() || *end != '\0') {
            b["delete"].push_back(job);
            *out = b;
            return Err::e("strconv.Atoi: parsing " + go_quote(v) + ": invalid syntax");
        }
        if (r < restarts) {
            b["delete"].push_back(job);
            continue;
        }
        const std::string t = jobFinishedType(job);
        if (t.empty()) b["active"].push_back(job);
        else if (t == "Failed") b["failed"].push_back(job);
        else b["successful"].push_back(job);
    }
    *out = b;
    return Err::none();
}

// failurePolicyRecreateAll, pkg/controllers/failure_policy.go:155-175 (A10 trigger)
void failurePolicyRecreateAll(Json& js, bool shouldCountTowardsMax) {
    Json& st = js["status"];
    st["restarts"] = st.get("restarts").as_int() + 1;
    if (shouldCountTowardsMax) st["restartsCountTowardsMax"] = st.get("restartsCountTowardsMax").as_int() + 1;
}

// ============================================================ pkg/controllers/pod_controller.go
// removePodNameSuffix, :297-306
Err removePodNameSuffix(const std::string& podName, std::string* out) {
    std::vector<std::string> parts;
    size_t st = 0;
    while (true) {
        size_t p = podName.find('-', st);
        parts.push_back(podName.substr(st, p == std::string::npos ? std::string::npos : p - st));
        if (p == std::string::npos) break;
        st = p + 1;
    }
    if (parts.size() < 5) return Err::e("invalid pod name: " + podName);
    std::string r;
    for (size_t i = 0; i + 1 < parts.size(); ++i) r += (i ? "-" : "") + parts[i];
    *out = r;
    return Err::none();
}

// SetupPodIndexes extractors, :75-106 (A11)
std::vector<std::string> podJobKeyIndex(const Json& pod) {
    if (!has_key(annotations(pod), kExclusiveKey)) return {};
    if (!has_key(labels(pod), kJobKey)) return {};
    return {str_at(labels(pod), kJobKey)};
}
std::vector<std::string> podNameIndex(const Json& pod) {
    if (!has_key(annotations(pod), kExclusiveKey)) return {};
    std::string n;
    if (!removePodNameSuffix(name_of(pod), &n).ok) return {};
    return {n};
}

bool usingExclusivePlacement(const Json& pod) { return has_key(annotations(pod), kExclusiveKey); }
bool podScheduled(const Json& pod) { return !node_name(pod).empty(); }
bool podDeleted(const Json& pod) { return !meta(pod).get("deletionTimestamp").is_null(); }

// followerPodTopology, :268-277
Err followerPodTopology(const Json& pod, const std::string& key, std::string* out) {
    const Json& ns = pod.get("spec").get("nodeSelector");
    if (!ns.is_object()) return Err::e("pod " + name_of(pod) + " nodeSelector is nil");
    if (!ns.has(key)) return Err::e("pod " + name_of(pod) + " nodeSelector is missing key: " + key);
    *out = ns.get(key).as_string();
    return Err::none();
}

// updatePodCondition, :309-327 (LastTransitionTime is set by the caller's clock)
bool updatePodCondition(Json& pod, Json cond) {
    Json& conds = pod["status"]["conditions"];
    if (!conds.is_array()) conds = Json::array();
    for (auto& c : conds.elems()) {
        const bool sameType = c.get("type") == cond.get("type");
        if (sameType && c.get("status") != cond.get("status")) {
            c = cond;
            return true;
        }
        if (sameType) return false;
    }
    if (cond.get("status").as_string() == "True") {
        conds.push_back(cond);
        return true;
    }
    return false;
}

// ============================================================ cached client
struct Cache {
    std::mutex mu;
    std::map<std::string, Json> pods;   // ns/name
    std::map<std::string, Json> nodes;  // name
    std::map<std::string, std::string> inject;  // "get/Node", "list/Pod", "update/Pod", "delete/Pod" -> error text
    // engine binding (the snapshot mirrors the node cache)
    jsp_engine* eng = nullptr;
    std::map<std::string, int32_t> node_rows;
    std::vector<std::string> level_keys;
    std::vector<std::vector<std::string>> domain_values;
    std::vector<std::map<std::string, int32_t>> domain_ids;
    // planner: the engine's snapshot built from this cache's objects (placement.h)
    std::unique_ptr<Planner> planner;
    // call counters (tests check which path ran)
    int64_t node_gets = 0, pod_lists = 0, engine_calls = 0;
    std::vector<std::string> deleted, status_updates;
};

Err injected(Cache& c, const std::string& what) {
    auto it = c.inject.find(what);
    if (it == c.inject.end()) return Err::none();
    return Err::e(it->second);
}

Err getNode(Cache& c, const std::string& name, Json* out) {
    ++c.node_gets;
    if (Err e = injected(c, "get/Node"); !e.ok) return e;
    auto it = c.nodes.find(name);
    if (it == c.nodes.end()) return Err::nf("nodes " + go_quote(name) + " not found");
    *out = it->second;
    return Err::none();
}

Err getPod(Cache& c, const std::string& ns, const std::string& name, Json* out) {
    if (Err e = injected(c, "get/Pod"); !e.ok) return e;
    auto it = c.pods.find(ns + "/" + name);
    if (it == c.pods.end()) return Err::nf("pods " + go_quote(name) + " not found");
    *out = it->second;
    return Err::none();
}

// client.List(InNamespace(ns), MatchingFields{field: value})
Err listPods(Cache& c, const std::string& ns, const std::string& field, const std::string& value, Json* out) {
    ++c.pod_lists;
    if (Err e = injected(c, "list/Pod"); !e.ok) return e;
    Json items = Json::array();
    for (const auto& kv : c.pods) {
        if (ns_of(kv.second) != ns) continue;
        const auto idx = field == kPodNameKey ? podNameIndex(kv.second) : podJobKeyIndex(kv.second);
        if (std::find(idx.begin(), idx.end(), value) != idx.end()) items.push_back(kv.second);
    }
    *out = items;
    return Err::none();
}

// Topology value of the node a pod is bound to: pod_mutating_webhook.go:173-194
// and pod_controller.go:242-263 (identical logic). With an engine bound, the
// domain of a node the snapshot holds, at one of its topology levels, comes
// from the resident snapshot (jsp_resolve_leader_domains). Anything else -- a
// key that is not an engine level, a node the snapshot does not hold (absent
// from the cache, or lacking a level label) -- takes the reference's Node Get
// path, so NotFound stays "" + nil and a missing label stays its error.
bool engineTopology(Cache& c, const std::string& node, const std::string& key, int32_t* row, uint32_t* level) {
    if (!c.eng) return false;
    if (c.planner) {
        const int lk = c.planner->level_of(key);
        if (lk < 0 || !c.planner->serving() || !c.planner->row_of(node, row)) return false;
        *level = (uint32_t)lk;
        return true;
    }
    auto lk = std::find(c.level_keys.begin(), c.level_keys.end(), key);
    auto it = c.node_rows.find(node);
    if (lk == c.level_keys.end() || it == c.node_rows.end()) return false;
    *row = it->second;
    *level = (uint32_t)(lk - c.level_keys.begin());
    return true;
}

const std::string& domainValue(Cache& c, uint32_t level, int32_t dom) {
    static const std::string empty;
    const std::vector<std::string>& v = c.planner ? c.planner->domain_values((int)level) : c.domain_values[level];
    return dom >= 0 && (size_t)dom < v.size() ? v[dom] : empty;
}

Err topologyFromPod(Cache& c, const Json& pod, const std::string& key, std::string* out) {
    const std::string node = node_name(pod);
    int32_t row = -1;
    uint32_t level = 0;
    if (engineTopology(c, node, key, &row, &level)) {
        int32_t dom = -1;
        ++c.engine_calls;
        if (jsp_resolve_leader_domains(c.eng, &row, &level, 1, &dom) != JSP_OK)
            return Err::e(std::string("placement engine: ") + jsp_last_error());
        *out = domainValue(c, level, dom);
        return Err::none();
    }
    Json n;
    Err e = getNode(c, node, &n);
    if (!e.ok) {
        *out = "";
        return e.not_found ? Err::none() : e;  // client.IgnoreNotFound
    }
    if (!has_key(labels(n), key)) return Err::e("node does not have topology label: " + key);
    *out = str_at(labels(n), key);
    return Err::none();
}

// ============================================================ pkg/webhooks
// genLeaderPodName, pod_admission_webhook.go:128-144
Err genLeaderPodName(const Json& pod, std::string* out) {
    const Json& l = labels(pod);
    for (const char* k : {kJobSetNameKey, kReplicatedJobNameKey, kJobIndexKey})
        if (!has_key(l, k)) return Err::e(std::string("pod missing label: ") + k);
    *out = GenPodName(str_at(l, kJobSetNameKey), str_at(l, kReplicatedJobNameKey), str_at(l, kJobIndexKey), "0");
    return Err::none();
}

// podsOwnedBySameJob, pod_admission_webhook.go:148-161
Err podsOwnedBySameJob(const Json& leader, const Json& follower) {
    const Json* f = controller_of(follower);
    if (!f) return Err::e("follower pod has no owner reference");
    const Json* l = controller_of(leader);
    if (!l) return Err::e("leader pod " + go_quote(name_of(leader)) + " has no owner reference");
    if (f->get("uid").as_string() != l->get("uid").as_string())
        return Err::e("follower pod owner UID (" + f->get("uid").as_string() + ") != leader pod owner UID (" +
                      l->get("uid").as_string() + ")");
    return Err::none();
}

// leaderPodForFollower, pod_admission_webhook.go:91-124
Err leaderPodForFollower(Cache& c, const Json& pod, Json* leader) {
    std::string ln;
    if (Err e = genLeaderPodName(pod, &ln); !e.ok) return e;
    Json list;
    if (Err e = listPods(c, ns_of(pod), kPodNameKey, ln, &list); !e.ok) return e;
    if (list.size() != 1)
        return Err::e("expected 1 leader pod (" + ln + "), but got " + std::to_string(list.size()) +
                      ". this is an expected, transient error");
    if (Err e = podsOwnedBySameJob(list.at(0), pod); !e.ok) return e;
    *leader = list.at(0);
    return Err::none();
}

// setExclusiveAffinities, pod_mutating_webhook.go:95-135 (A4): appends, never dedupes
void setExclusiveAffinities(Json& pod) {
    const std::string own = str_at(labels(pod), kJobKey);
    const std::string topo = str_at(annotations(pod), kExclusiveKey);
    Json& aff = pod["spec"]["affinity"];
    Json term = Json::object();
    Json req = Json::object();
    req["key"] = kJobKey;
    req["operator"] = "In";
    req["values"] = Json::array();
    req["values"].push_back(own);
    term["labelSelector"]["matchExpressions"] = Json::array();
    term["labelSelector"]["matchExpressions"].push_back(req);
    term["topologyKey"] = topo;
    term["namespaceSelector"] = Json::object();
    Json& pa = aff["podAffinity"]["requiredDuringSchedulingIgnoredDuringExecution"];
    if (!pa.is_array()) pa = Json::array();
    pa.push_back(term);

    Json anti = Json::object();
    Json e1 = Json::object();
    e1["key"] = kJobKey;
    e1["operator"] = "Exists";
    Json e2 = Json::object();
    e2["key"] = kJobKey;
    e2["operator"] = "NotIn";
    e2["values"] = Json::array();
    e2["values"].push_back(own);
    anti["labelSelector"]["matchExpressions"] = Json::array();
    anti["labelSelector"]["matchExpressions"].push_back(e1);
    anti["labelSelector"]["matchExpressions"].push_back(e2);
    anti["topologyKey"] = topo;
    anti["namespaceSelector"] = Json::object();
    Json& paa = aff["podAntiAffinity"]["requiredDuringSchedulingIgnoredDuringExecution"];
    if (!paa.is_array()) paa = Json::array();
    paa.push_back(anti);
}

// setNodeSelector, pod_mutating_webhook.go:137-171 (A5)
Err setNodeSelector(Cache& c, Json& pod) {
    Json leader;
    if (Err e = leaderPodForFollower(c, pod, &leader); !e.ok) return Err::none();  // validation webhook rejects
    if (node_name(leader).empty()) return Err::none();
    const Json& ann = annotations(pod);
    if (!has_key(ann, kExclusiveKey)) return Err::e(std::string("pod missing annotation: ") + kExclusiveKey);
    const std::string key = str_at(ann, kExclusiveKey);
    std::string value;
    if (Err e = topologyFromPod(c, leader, key, &value); !e.ok) return e;
    Json& ns = pod["spec"]["nodeSelector"];
    if (!ns.is_object()) ns = Json::object();
    ns[key] = value;
    return Err::none();
}

// Default, pod_mutating_webhook.go:64-93
Err Default(Cache& c, Json& pod) {
    const Json& ann = annotations(pod);
    if (!has_key(ann, kExclusiveKey) || has_key(ann, kNodeSelectorStrategyKey)) return Err::none();
    if (str_at(ann, kJobCompletionIndexAnnotation) == "0") {
        setExclusiveAffinities(pod);
        return Err::none();
    }
    return setNodeSelector(c, pod);
}

// Default over a batch of pods -- every pod of a JobSet's (re)created Jobs as
// the Job controller creates them: per pod exactly
// Default's result and error, but the followers whose leader node the engine
// holds at a level key are resolved by ONE jsp_resolve_leader_domains call.
Json DefaultBatch(Cache& c, const Json& pods) {
    struct Pending {
        size_t i;
        int32_t row;
        uint32_t level;
        std::string key;
    };
    std::vector<Pending> pend;
    std::vector<Json> res;
    std::vector<Err> errs;
    for (size_t i = 0; i < pods.size(); ++i) {
        Json pod = pods.at(i);
        Err e = Err::none();
        const Json& ann = annotations(pod);
        if (has_key(ann, kExclusiveKey) && !has_key(ann, kNodeSelectorStrategyKey)) {
            if (str_at(ann, kJobCompletionIndexAnnotation) == "0") {
                setExclusiveAffinities(pod);
            } else {
                // setNodeSelector's order: leader lookup, leader bound, then the topology value
                Json leader;
                if (leaderPodForFollower(c, pod, &leader).ok && !node_name(leader).empty()) {
                    const std::string key = str_at(ann, kExclusiveKey);
                    int32_t row = -1;
                    uint32_t level = 0;
                    if (engineTopology(c, node_name(leader), key, &row, &level)) {
                        pend.push_back({i, row, level, key});
                    } else {
                        std::string value;
                        e = topologyFromPod(c, leader, key, &value);
                        if (e.ok) {
                            Json& ns = pod["spec"]["nodeSelector"];
                            if (!ns.is_object()) ns = Json::object();
                            ns[key] = value;
                        }
                    }
                }
            }
        }
        res.push_back(std::move(pod));
        errs.push_back(e);
    }
    if (!pend.empty()) {
        std::vector<int32_t> rows, doms(pend.size(), -1);
        std::vector<uint32_t> levels;
        for (const auto& p : pend) {
            rows.push_back(p.row);
            levels.push_back(p.level);
        }
        ++c.engine_calls;
        const bool ok = jsp_resolve_leader_domains(c.eng, rows.data(), levels.data(), (uint32_t)rows.size(),
                                                   doms.data()) == JSP_OK;
        const std::string msg = ok ? "" : std::string("placement engine: ") + jsp_last_error();
        for (size_t k = 0; k < pend.size(); ++k) {
            if (!ok) {
                errs[pend[k].i] = Err::e(msg);
                continue;
            }
            Json& ns = res[pend[k].i]["spec"]["nodeSelector"];
            if (!ns.is_object()) ns = Json::object();
            ns[pend[k].key] = domainValue(c, pend[k].level, doms[k]);
        }
    }
    Json out = Json::array();
    for (size_t i = 0; i < res.size(); ++i) {
        Json x = Json::object();
        x["pod"] = res[i];
        x["error"] = errs[i].ok ? Json() : Json(errs[i].msg);
        out.push_back(x);
    }
    return out;
}

// leaderPodScheduled, pod_admission_webhook.go:78-89
Err leaderPodScheduled(Cache& c, const Json& pod, bool* scheduled) {
    Json leader;
    if (Err e = leaderPodForFollower(c, pod, &leader); !e.ok) return e;
    *scheduled = !node_name(leader).empty();
    return Err::none();
}

// ValidateCreate, pod_admission_webhook.go:24-67 (A6)
Err ValidateCreate(Cache& c, const Json& pod) {
    const Json& ann = annotations(pod);
    if (!has_key(ann, kJobSetNameKey)) return Err::none();
    if (has_key(ann, kNodeSelectorStrategyKey)) return Err::none();
    if (!has_key(ann, kExclusiveKey)) return Err::none();
    const std::string key = str_at(ann, kExclusiveKey);
    if (IsLeaderPod(pod)) return Err::none();
    const Json& ns = pod.get("spec").get("nodeSelector");
    if (!ns.is_object()) return Err::e("follower pod node selector not set");
    if (!ns.has(key))
        return Err::e("follower pod node selector for topology domain not found. missing selector: " + key);
    bool scheduled = false;
    if (Err e = leaderPodScheduled(c, pod, &scheduled); !e.ok) return e;
    if (!scheduled)
        return Err::e("leader pod not yet scheduled, not creating follower pod. this is an expected, transient error");
    return Err::none();
}

// ============================================================ PodReconciler
// validatePodPlacements, pod_controller.go:172-194 (A9). With an engine
// holding the leader's node at the key's level, the whole job is checked by
// one jsp_audit_placements call (followers' selector values as domain ids
// against the leader's row); only when it reports a mismatch are the
// followers walked on the host, to return the reference's first error.
Err validatePodPlacements(Cache& c, const Json& leader, const Json& podList, bool* valid) {
    *valid = false;
    const std::string key = str_at(annotations(leader), kExclusiveKey);
    int32_t row = -1;
    uint32_t level = 0;
    if (c.planner && engineTopology(c, node_name(leader), key, &row, &level)) {
        std::vector<int32_t> fdom;
        bool selector_error = false;
        for (const auto& pod : podList.elems()) {
            if (IsLeaderPod(pod)) continue;
            std::string ft;
            if (!followerPodTopology(pod, key, &ft).ok) {
                selector_error = true;
                break;
            }
            const int32_t d = c.planner->domain_id((int)level, ft);
            fdom.push_back(d < 0 ? -2 : d);  // a value no domain has never matches
        }
        if (!selector_error) {
            const uint32_t off[2] = {0, (uint32_t)fdom.size()};
            uint32_t bad = 0;
            ++c.engine_calls;
            if (jsp_audit_placements(c.eng, &row, &level, off, fdom.empty() ? nullptr : fdom.data(), 1, &bad) != JSP_OK)
                return Err::e(std::string("placement engine: ") + jsp_last_error());
            if (bad == 0) {
                *valid = true;
                return Err::none();
            }
        }
        // the reference's walk, for its first error (leader value from the snapshot)
        const std::string lt = domainValue(c, level, c.planner->row_domain((uint32_t)row, (int)level));
        for (const auto& pod : podList.elems()) {
            if (IsLeaderPod(pod)) continue;
            std::string ft;
            if (Err e = followerPodTopology(pod, key, &ft); !e.ok) return e;
            if (ft != lt) return Err::e("follower topology " + go_quote(ft) + " != leader topology " + go_quote(lt));
        }
        *valid = true;
        return Err::none();
    }
    std::string lt;
    if (Err e = topologyFromPod(c, leader, key, &lt); !e.ok) return e;
    for (const auto& pod : podList.elems()) {
        if (IsLeaderPod(pod)) continue;
        std::string ft;
        if (Err e = followerPodTopology(pod, key, &ft); !e.ok) return e;
        if (ft != lt) return Err::e("follower topology " + go_quote(ft) + " != leader topology " + go_quote(lt));
    }
    *valid = true;
    return Err::none();
}

// deleteFollowerPods, pod_controller.go:197-237 (sequential; deterministic order)
Err deleteFollowerPods(Cache& c, const Json& pods, const std::string& now) {
    std::vector<std::string> errs;
    for (auto pod : pods.elems()) {
        if (IsLeaderPod(pod)) continue;
        Json cond = Json::object();
        cond["type"] = "DisruptionTarget";
        cond["status"] = "True";
        cond["reason"] = kExclusivePlacementViolationReason;
        cond["message"] = kExclusivePlacementViolationMessage;
        cond["lastTransitionTime"] = now;
        if (updatePodCondition(pod, cond)) {
            if (Err e = injected(c, "update/Pod"); !e.ok) {
                errs.push_back(e.msg);
                continue;
            }
            c.status_updates.push_back(name_of(pod));
            auto it = c.pods.find(ns_of(pod) + "/" + name_of(pod));
            if (it != c.pods.end()) it->second = pod;
        }
        if (Err e = injected(c, "delete/Pod"); !e.ok) {
            errs.push_back(e.msg);
            continue;
        }
        c.pods.erase(ns_of(pod) + "/" + name_of(pod));  // absent pods are NotFound: ignored
        c.deleted.push_back(name_of(pod));
    }
    return errs.empty() ? Err::none() : Err::e(errors_join(errs));
}

// Reconcile, pod_controller.go:115-157. The reference returns on the
// validation error before its `!valid` branch (:148-155), so a mismatch is an
// error + requeue, never a deletion; kept as is.
Err Reconcile(Cache& c, const std::string& ns, const std::string& name, const std::string& now) {
    Json leader;
    if (Err e = getPod(c, ns, name, &leader); !e.ok) return e.not_found ? Err::none() : e;
    if (!has_key(labels(leader), kJobKey))
        return Err::e("job key label not found on leader pod: " + go_quote(name_of(leader)));
    Json list;
    if (Err e = listPods(c, ns_of(leader), kPodJobKey, str_at(labels(leader), kJobKey), &list); !e.ok) return e;
    bool valid = false;
    if (Err e = validatePodPlacements(c, leader, list, &valid); !e.ok) return e;
    if (!valid) return deleteFollowerPods(c, list, now);
    return Err::none();
}

// ============================================================ engine placement (A10, §8f rows 1 and 4)
// Plan child Jobs through the engine: one requirement class per
// (replicatedJob, exclusive-topology key), runs in the jobs' order (the order
// constructJobsFromTemplate produces them: globalJobIndex), the snapshot
// re-synced from this cache's Node / Pod objects first. Jobs without the
// exclusive annotation, or with the node-selector strategy, are not placed by
// the engine (the reference's webhooks skip them too, pod_mutating_webhook.go:72-76).
Json classesJson(const Planner& pl, const std::vector<ClassSpec>& classes) {
    std::vector<jsp_job_class> jc;
    pl.encode(classes, &jc);
    Json out = Json::array();
    for (size_t i = 0; i < classes.size(); ++i) {
        const jsp_job_class& x = jc[i];
        Json o = Json::object(), req = Json::array(), fb = Json::array(), res = Json::array();
        for (int w = 0; w < JSP_MAX_LABEL_WORDS; ++w) {
            char a[24], b[24];
            std::snprintf(a, sizeof a, "%016llx", (unsigned long long)x.req_labels[w]);
            std::snprintf(b, sizeof b, "%016llx", (unsigned long long)x.forbid_labels[w]);
            req.push_back(std::string(a));
            fb.push_back(std::string(b));
        }
        for (int r = 0; r < JSP_MAX_RES; ++r) res.push_back((int64_t)x.req_res[r]);
        o["reqLabels"] = req;
        o["forbidLabels"] = fb;
        o["toleratedTaints"] = (int64_t)x.tolerated_taints;
        o["level"] = (int64_t)x.level;
        o["pods"] = (int64_t)x.pods;
        o["reqRes"] = res;
        out.push_back(o);
    }
    return out;
}

// ---- the front every planner.* request with `jobs` shares
Err needPlanner(const Cache& c) {
    return c.planner ? Err::none() : Err::e("no placement planner bound to this cache");
}

// The engine places this job: the exclusive annotation, and not the node-selector strategy.
bool enginePlaces(const Json& job) {
    const Json& ann = annotations(job);
    return has_key(ann, kExclusiveKey) && !has_key(ann, kNodeSelectorStrategyKey);
}

struct PlacedJob {
    std::string name, key;  // the Job's name and its exclusive-topology key
    uint32_t cls;           // index into PlanRequest::classes
    const Json* job;        // the request's Job object
};

struct PlanRequest {
    Planner* pl = nullptr;
    std::vector<ClassSpec> classes;
    std::vector<PlacedJob> jobs;  // the jobs the engine places, in the request's order
    Json snapshot;                // Planner::sync's stats
    int level(size_t j) const { return pl->level_of(jobs[j].key); }
};

// The requirement classes of `jobs` and the placed jobs with their class index.
Err jobClasses(Planner& pl, const Json& jobs, std::vector<ClassSpec>* classes, std::vector<PlacedJob>* placed) {
    std::map<std::string, uint32_t> class_of_rj;
    for (const auto& job : jobs.elems()) {
        if (!enginePlaces(job)) continue;
        const std::string key = str_at(annotations(job), kExclusiveKey);
        const std::string ck = str_at(labels(job), kReplicatedJobNameKey) + "\n" + key;
        auto it = class_of_rj.find(ck);
        uint32_t ci = 0;
        if (it == class_of_rj.end()) {
            ClassSpec cs;
            const Json& js = job.get("spec");
            const int64_t par = js.has("parallelism") ? js.get("parallelism").as_int() : 1;
            if (Err2 e = pl.class_of(js.get("template"), par, key, &cs); !e.ok()) return Err::e(e.msg);
            ci = (uint32_t)classes->size();
            classes->push_back(std::move(cs));
            class_of_rj[ck] = ci;
        } else {
            ci = it->second;
        }
        placed->push_back({name_of(job), key, ci, &job});
    }
    if (classes->size() > JSP_MAX_CLASSES) return Err::e("placement planner: more than 64 requirement classes");
    return Err::none();
}

// A planner; the classes (their errors come before the sync, so nothing is
// synced then); the snapshot re-synced from the cache.
Err openRequest(Cache& c, const Json& jobs, PlanRequest* q) {
    if (Err e = needPlanner(c); !e.ok) return e;
    q->pl = c.planner.get();
    if (Err e = jobClasses(*q->pl, jobs, &q->classes, &q->jobs); !e.ok) return e;
    if (Err2 e = q->pl->sync(c.nodes, c.pods, &q->snapshot); !e.ok()) return Err::e(e.msg);
    return Err::none();
}

// The runs (class, job count) of jobs [first, end) appended to rc / rl; a run
// never reaches back over `first`. Returns how many runs that were.
uint32_t appendRuns(const std::vector<PlacedJob>& jobs, size_t first, size_t end, std::vector<uint32_t>* rc,
                    std::vector<uint32_t>* rl) {
    const size_t before = rc->size();
    for (size_t j = first; j < end; ++j) {
        if (rc->size() == before || rc->back() != jobs[j].cls) {
            rc->push_back(jobs[j].cls);
            rl->push_back(0);
        }
        ++rl->back();
    }
    return (uint32_t)(rc->size() - before);
}

// An assignment as job name -> domain value: a plan (planner.plan's reply:
// its jobs' "domain", null domains skipped) or such an object itself. Anything
// else comes back as it is, for the caller to refuse.
Json byName(const Json& assignment) {
    if (!assignment.is_object() || !assignment.get("jobs").is_array()) return assignment;
    Json by_name = Json::object();
    for (const auto& j : assignment.get("jobs").elems())
        if (j.get("domain").is_string()) by_name[j.get("name").as_string()] = j.get("domain");
    return by_name;
}

// by_name's values as domain ids at each placed job's level; an unknown value
// or an absent job is -1. Values, not ids, are the durable form (a re-upload
// renumbers the domains), so this is called after the sync: the ids are those
// of the snapshot the engine now holds.
std::vector<int32_t> domainIds(const PlanRequest& q, const Json& by_name) {
    std::vector<int32_t> ids;
    for (size_t j = 0; j < q.jobs.size(); ++j) {
        const Json& v = by_name.get(q.jobs[j].name);
        ids.push_back(v.is_string() ? q.pl->domain_id(q.level(j), v.as_string()) : -1);
    }
    return ids;
}

Json domainOf(const PlanRequest& q, size_t j, int32_t d) {  // null: no domain
    return d >= 0 ? Json(q.pl->domain_values(q.level(j))[d]) : Json();
}

// A reply's "jobs": per placed job "name", "topologyKey" and "domain" (the
// value, null: none). With `unplaceable` (the placing methods) also "domainId",
// and the names without a domain are appended to it.
Json jobEntries(const PlanRequest& q, const std::vector<int32_t>& assign, Json* unplaceable) {
    Json js = Json::array();
    for (size_t j = 0; j < q.jobs.size(); ++j) {
        Json x = Json::object();
        x["name"] = q.jobs[j].name;
        x["topologyKey"] = q.jobs[j].key;
        x["domain"] = domainOf(q, j, assign[j]);
        if (unplaceable) {
            x["domainId"] = (int64_t)assign[j];
            if (assign[j] < 0) unplaceable->push_back(q.jobs[j].name);
        }
        js.push_back(x);
    }
    return js;
}

// A reply's tail: "snapshot" (the sync's stats), "classes" and each placed job's class index.
void replyTail(const PlanRequest& q, Json* r, bool snapshot = true) {
    if (snapshot) (*r)["snapshot"] = q.snapshot;
    (*r)["classes"] = classesJson(*q.pl, q.classes);
    Json jcj = Json::array();
    for (const auto& j : q.jobs) jcj.push_back((int64_t)j.cls);
    (*r)["jobClass"] = jcj;
}

// What the placing methods reply: "jobs", "unplaceable", "placed" and the tail.
Json planReply(const PlanRequest& q, const std::vector<int32_t>& assign, uint32_t placed) {
    Json r = Json::object(), un = Json::array();
    r["jobs"] = jobEntries(q, assign, &un);
    r["unplaceable"] = un;
    r["placed"] = (int64_t)placed;
    replyTail(q, &r);
    return r;
}

// planner.plan: planReply.
// explain: also "explanations", one entry per class with an unplaceable job
// (planner.explain); the plan's own fields are the same either way.
// previous (an object, else ignored): job name -> the topology value of the
// domain the job held before. The jobs are then placed by jsp_place_sticky,
// each job also reports "previousDomain" and "kept", and the plan "hinted",
// "kept", "moved" (hinted, not kept, but placed) and "lost" (hinted and now
// unplaceable). Without `previous` the reply is what it was before the sticky
// placement existed.
Err planJobs(Cache& c, const Json& jobs, Json* out, bool explain = false, const Json& previous = Json()) {
    PlanRequest q;
    if (Err e = openRequest(c, jobs, &q); !e.ok) return e;
    Planner& pl = *q.pl;
    std::vector<uint32_t> rc, rl;
    appendRuns(q.jobs, 0, q.jobs.size(), &rc, &rl);
    std::vector<int32_t> assign, prev;
    jsp_stats st{};
    jsp_sticky_stats sst{};
    const bool sticky = previous.is_object();
    ++c.engine_calls;
    if (sticky) {
        prev = domainIds(q, previous);
        if (Err2 e = pl.place_sticky(q.classes, rc, rl, prev, &assign, &sst); !e.ok()) return Err::e(e.msg);
        st.placed = sst.placed;
    } else if (Err2 e = pl.place(q.classes, rc, rl, &assign, &st); !e.ok()) {
        return Err::e(e.msg);
    }
    Json r = planReply(q, assign, st.placed);
    if (sticky) {
        int64_t moved = 0, lost = 0;
        for (size_t j = 0; j < q.jobs.size(); ++j) {
            // the fill never hands a job a hinted domain it did not keep, unless the
            // hints of one plan overlapped: kept is "sits on its previous domain"
            const bool kept = prev[j] >= 0 && assign[j] == prev[j];
            r["jobs"].at(j)["previousDomain"] = domainOf(q, j, prev[j]);
            r["jobs"].at(j)["kept"] = kept;
            if (prev[j] >= 0 && !kept) ++(assign[j] >= 0 ? moved : lost);
        }
        r["hinted"] = (int64_t)sst.hinted;
        r["kept"] = (int64_t)sst.hinted - moved - lost;
        r["moved"] = moved;
        r["lost"] = lost;
    }
    if (explain) {
        Json ex = Json::array();
        std::vector<std::vector<std::string>> stuck(q.classes.size());
        for (size_t j = 0; j < q.jobs.size(); ++j)
            if (assign[j] < 0) stuck[q.jobs[j].cls].push_back(q.jobs[j].name);
        std::vector<jsp_class_explain> recs;
        if (r.get("unplaceable").size() > 0) {
            ++c.engine_calls;
            if (Err2 e = pl.explain(q.classes, &recs); !e.ok()) return Err::e(e.msg);
        }
        const std::vector<std::string>& res = pl.resources();
        for (size_t ci = 0; ci < q.classes.size() && ci < recs.size(); ++ci) {
            if (stuck[ci].empty()) continue;
            const int level = q.classes[ci].level;
            const std::string& key = pl.level_keys()[level];
            Json x = Json::object(), jn = Json::array();
            for (const auto& nm : stuck[ci]) jn.push_back(nm);
            const Json counts = explain_counts(recs[ci], res.size());
            const int32_t bd = recs[ci].best_short_domain;
            x["class"] = (int64_t)ci;
            x["jobs"] = jn;
            x["counts"] = counts;
            x["message"] = explain_message(counts, key, q.classes[ci].pods, res,
                                           bd >= 0 ? pl.domain_values(level)[bd] : std::string());
            ex.push_back(x);
        }
        r["explanations"] = ex;
    }
    *out = r;
    return Err::none();
}

// planner.planGangs: the jobs of planner.plan, placed JobSet by JobSet
// (jsp_place_gangs): a gang is a maximal run of consecutive placed jobs with
// the same namespace and jobset.sigs.k8s.io/jobset-name label, and it is
// placed whole or not at all. spans (an object, else no spans):
// "<namespace>/<jobset name>" -> a topology key; the JobSet's jobs then all
// land inside one domain of that key. No entry: anywhere in the cluster. A key
// that is not one of the engine's levels, or one finer than the topology key
// of one of the JobSet's jobs, is an error that names the JobSet. The reply is
// planner.plan's plus, per job, "jobSet"; "jobSets", one entry per gang in
// order: {"name", "spanKey" (null: none), "spanDomain" (the domain's value;
// null without a span or when refused), "placed"}; and "gangsPlaced".
Err planGangs(Cache& c, const Json& jobs, const Json& spans, Json* out) {
    PlanRequest q;
    if (Err e = openRequest(c, jobs, &q); !e.ok) return e;
    Planner& pl = *q.pl;
    std::vector<std::string> sets;
    for (const auto& j : q.jobs) sets.push_back(ns_of(*j.job) + "/" + str_at(labels(*j.job), kJobSetNameKey));
    std::vector<uint32_t> gs;
    std::vector<size_t> gang_first;  // first job of each gang
    for (size_t j = 0; j < q.jobs.size(); ++j) {
        if (j == 0 || sets[j] != sets[j - 1]) {
            gang_first.push_back(j);
            gs.push_back(JSP_SPAN_ANY);
            const Json& v = spans.is_object() ? spans.get(sets[j]) : Json();
            if (v.is_string()) {
                const int lvl = pl.level_of(v.as_string());
                if (lvl < 0)
                    return Err::e("planner.planGangs: JobSet " + go_quote(sets[j]) + ": span key " +
                                  go_quote(v.as_string()) + " is not one of the engine's topology levels");
                gs.back() = (uint32_t)lvl;
            }
        }
        if (gs.back() != JSP_SPAN_ANY && q.level(j) >= 0 && (uint32_t)q.level(j) < gs.back())
            return Err::e("planner.planGangs: JobSet " + go_quote(sets[j]) + ": span key " +
                          go_quote(pl.level_keys()[gs.back()]) + " is finer than the topology key " +
                          go_quote(q.jobs[j].key) + " of job " + go_quote(q.jobs[j].name));
    }
    // every gang starts a new run, even when the class repeats
    std::vector<uint32_t> rc, rl, gr;
    for (size_t g = 0; g < gang_first.size(); ++g)
        gr.push_back(appendRuns(q.jobs, gang_first[g], g + 1 < gang_first.size() ? gang_first[g + 1] : q.jobs.size(), &rc, &rl));
    std::vector<int32_t> assign, span_domain;
    jsp_gang_stats st{};
    ++c.engine_calls;
    if (Err2 e = pl.place_gangs(q.classes, rc, rl, gr, gs, &assign, &span_domain, &st); !e.ok()) return Err::e(e.msg);
    Json r = planReply(q, assign, st.placed), sj = Json::array();
    for (size_t j = 0; j < q.jobs.size(); ++j) r["jobs"].at(j)["jobSet"] = sets[j];
    for (size_t g = 0; g < gang_first.size(); ++g) {
        Json x = Json::object();
        const bool spanned = gs[g] != JSP_SPAN_ANY;
        x["name"] = sets[gang_first[g]];
        x["spanKey"] = spanned ? Json(pl.level_keys()[gs[g]]) : Json();
        x["spanDomain"] = spanned && span_domain[g] >= 0 ? Json(pl.domain_values((int)gs[g])[span_domain[g]]) : Json();
        x["placed"] = span_domain[g] >= 0;
        sj.push_back(x);
    }
    r["jobSets"] = sj;
    r["gangsPlaced"] = (int64_t)st.gangs_placed;
    *out = r;
    return Err::none();
}

// planner.planFit: the jobs of planner.plan placed by jsp_place_fit under
// `policy`: "lowest" (planner.plan's answer), "tightest" (every job takes the
// free feasible domain with the least pod capacity that still fits) or
// "roomiest" (the most). Any other policy is an error that names it, before
// the jobs are looked at. The reply is planner.plan's plus "policy" and
// "slack", the pod capacity the placed jobs leave unused in their domains
// (jsp_fit_stats.slack).
Err planFit(Cache& c, const Json& jobs, const Json& policy, Json* out) {
    if (Err e = needPlanner(c); !e.ok) return e;  // as in every method, this comes before the policy error
    static const char* const kPolicies[] = {"lowest", "tightest", "roomiest"};
    uint32_t pol = 0;
    while (pol < 3 && !(policy.is_string() && policy.as_string() == kPolicies[pol])) ++pol;
    if (pol == 3)
        return Err::e("planner.planFit: policy " + (policy.is_string() ? go_quote(policy.as_string()) : std::string("(none)")) +
                      " is none of \"lowest\", \"tightest\", \"roomiest\"");
    PlanRequest q;
    if (Err e = openRequest(c, jobs, &q); !e.ok) return e;
    std::vector<uint32_t> rc, rl;
    appendRuns(q.jobs, 0, q.jobs.size(), &rc, &rl);
    std::vector<int32_t> assign;
    jsp_fit_stats st{};
    ++c.engine_calls;
    if (Err2 e = q.pl->place_fit(q.classes, rc, rl, pol, &assign, &st); !e.ok()) return Err::e(e.msg);
    Json r = planReply(q, assign, st.placed);
    r["policy"] = kPolicies[pol];
    r["slack"] = (int64_t)st.slack;
    *out = r;
    return Err::none();
}

// planner.whatIf: the jobs of planner.plan placed under hypothetical evictions
// (jsp_place_whatif: nothing is written, the cache and the engine's snapshot
// stay as they are). scenarios: [{"name": ..., "evict": [job keys]}] -- the
// job-key label values (jobHashKey) of the jobs to think away: their bound
// pods' requests go back to their nodes, their exclusive covers and their
// assumed domains (planner.assume's ledger) are lifted. A key that no pod and
// no ledger entry carries is an error that names it and the scenario. The
// reply is planner.plan's (the unedited answer) plus "scenarios": per scenario
// "name", "jobs" (name, topologyKey, domainId, domain), "placed",
// "unplaceable", "flips" (the (class, domain) feasibility bits that differ
// from the snapshot's) and "rows" (the node rows the eviction changes). One
// engine call per scenario and one for the unedited plan: jsp_whatif_stats
// counts flips per call.
Err whatIf(Cache& c, const Json& jobs, const Json& scenarios, Json* out) {
    if (Err e = needPlanner(c); !e.ok) return e;
    if (!scenarios.is_array()) return Err::e("planner.whatIf: scenarios must be an array of {\"name\", \"evict\"} objects");
    for (const auto& sc : scenarios.elems()) {
        bool good = sc.is_object() && sc.get("evict").is_array();
        for (const auto& k : sc.get("evict").elems()) good = good && k.is_string();
        if (!good) return Err::e("planner.whatIf: scenarios must be an array of {\"name\", \"evict\"} objects");
    }
    PlanRequest q;
    if (Err e = openRequest(c, jobs, &q); !e.ok) return e;
    Planner& pl = *q.pl;
    std::vector<uint32_t> rc, rl;
    appendRuns(q.jobs, 0, q.jobs.size(), &rc, &rl);
    // every scenario's delta first: an unknown key is refused before the engine is asked anything
    struct Delta {
        std::vector<uint32_t> rows, fr;
        std::vector<int32_t> ex;
    };
    std::vector<Delta> deltas(scenarios.size());
    for (size_t s = 0; s < scenarios.size(); ++s) {
        const Json& sc = scenarios.at(s);
        std::set<std::string> keys;
        for (const auto& k : sc.get("evict").elems()) keys.insert(k.as_string());
        std::string unknown;
        if (Err2 e = pl.evict_delta(c.nodes, c.pods, keys, &deltas[s].rows, &deltas[s].fr, &deltas[s].ex, &unknown); !e.ok())
            return Err::e(e.msg);
        if (!unknown.empty())
            return Err::e("planner.whatIf: scenario " + (sc.get("name").is_string() ? go_quote(sc.get("name").as_string()) : std::to_string(s)) +
                          ": unknown job key " + go_quote(unknown));
    }
    std::vector<int32_t> assign;
    jsp_whatif_stats st{};
    ++c.engine_calls;
    if (Err2 e = pl.place_whatif(q.classes, rc, rl, {}, {}, {}, &assign, &st); !e.ok()) return Err::e(e.msg);
    uint32_t placed = 0;
    for (int32_t d : assign) placed += d >= 0;
    Json r = planReply(q, assign, placed), sj = Json::array();
    for (size_t s = 0; s < scenarios.size(); ++s) {
        ++c.engine_calls;
        if (Err2 e = pl.place_whatif(q.classes, rc, rl, deltas[s].rows, deltas[s].fr, deltas[s].ex, &assign, &st); !e.ok())
            return Err::e(e.msg);
        Json x = Json::object(), un = Json::array();
        placed = 0;
        for (int32_t d : assign) placed += d >= 0;
        x["name"] = scenarios.at(s).get("name");
        x["jobs"] = jobEntries(q, assign, &un);
        x["placed"] = (int64_t)placed;
        x["unplaceable"] = un;
        x["flips"] = (int64_t)st.flips;
        x["rows"] = (int64_t)deltas[s].rows.size();
        sj.push_back(x);
    }
    r["scenarios"] = sj;
    *out = r;
    return Err::none();
}

// planner.preempt: the jobs of planner.plan placed at "priority" (an int32, as
// a pod's spec.priority) by jsp_place_preempt: nothing is written. An
// exclusive job of the cache whose bound, non-terminal pods all carry a
// spec.priority below it (absent: 0) may be evicted; a job at or above it
// blocks its domain, and so does a domain that planner.assume holds (the
// ledger carries no priority). Every job takes the reachable domain with no
// victims first, then the lowest highest-victim priority, then the fewest
// victims, then the lowest id. The reply is planner.plan's plus, per job,
// "victims" (the job-key label values of the jobs to evict for it, in node
// order) and, at top level, "evict": those keys sorted, each once. Evicting
// them, waiting for the informer and planner.assume are the caller's steps.
Err preemptJobs(Cache& c, const Json& jobs, const Json& priority, Json* out) {
    if (Err e = needPlanner(c); !e.ok) return e;
    if (!priority.is_number() || priority.as_int() < INT32_MIN || priority.as_int() > INT32_MAX)
        return Err::e("planner.preempt: priority must be an integer (int32)");
    PlanRequest q;
    if (Err e = openRequest(c, jobs, &q); !e.ok) return e;
    std::vector<uint32_t> rc, rl;
    appendRuns(q.jobs, 0, q.jobs.size(), &rc, &rl);
    std::vector<int32_t> assign;
    std::vector<uint32_t> off;
    std::vector<std::string> victims;
    jsp_preempt_stats st{};
    ++c.engine_calls;
    if (Err2 e = q.pl->place_preempt(q.classes, rc, rl, (int32_t)priority.as_int(), c.nodes, c.pods, &assign, &off,
                                     &victims, &st);
        !e.ok())
        return Err::e(e.msg);
    Json r = planReply(q, assign, st.placed), ev = Json::array();
    for (size_t j = 0; j < q.jobs.size(); ++j) {
        Json v = Json::array();
        for (uint32_t i = off[j]; i < off[j + 1]; ++i) v.push_back(victims[i]);
        r["jobs"].at(j)["victims"] = v;
    }
    for (const auto& k : std::set<std::string>(victims.begin(), victims.end())) ev.push_back(k);
    r["evict"] = ev;
    *out = r;
    return Err::none();
}

// planner.planSpread: the jobs of planner.plan spread evenly over the domains
// of "topologyKey" (an engine level not finer than any job's own key) by
// jsp_place_spread, as a pod's topologySpreadConstraints entry asks: "maxSkew"
// (an integer >= 1) and "whenUnsatisfiable", "DoNotSchedule" (the default: a
// job that would put its domain more than maxSkew ahead of the emptiest
// eligible one stays unplaced and counts in "refused") or "ScheduleAnyway"
// (never refused: the emptiest domain with room). The peers, the jobs that
// count as already placed, are the exclusive jobs of the request's JobSets
// that hold domains by the cache's pods or by planner.assume's ledger, the
// request's own jobs left out, or exactly the job keys in "peers". The reply is
// planner.plan's plus, per job, "spreadDomain" (the value of the
// topologyKey's domain, null: unplaced) and, at top level, "topologyKey",
// "maxSkew", "whenUnsatisfiable", "peers" (the keys counted, sorted),
// "counts" (domain value -> peers and placed jobs), "refused" and "skew".
Err planSpread(Cache& c, const Json& jobs, const Json& topology_key, const Json& max_skew, const Json& when,
               const Json& peers, Json* out) {
    if (Err e = needPlanner(c); !e.ok) return e;
    const std::string mode = when.is_string() ? when.as_string() : std::string("DoNotSchedule");
    if (mode != "DoNotSchedule" && mode != "ScheduleAnyway")
        return Err::e("planner.planSpread: whenUnsatisfiable " + go_quote(mode) +
                      " is neither \"DoNotSchedule\" nor \"ScheduleAnyway\"");
    if (!max_skew.is_number() || max_skew.as_int() < 1 || max_skew.as_int() > INT32_MAX)
        return Err::e("planner.planSpread: maxSkew must be an integer >= 1");
    if (!topology_key.is_string()) return Err::e("planner.planSpread: topologyKey is needed");
    if (!peers.is_null() && !peers.is_array()) return Err::e("planner.planSpread: peers must be a list of job keys");
    PlanRequest q;
    if (Err e = openRequest(c, jobs, &q); !e.ok) return e;
    const int level = q.pl->level_of(topology_key.as_string());
    if (level < 0)
        return Err::e("planner.planSpread: topologyKey " + go_quote(topology_key.as_string()) + " is no level of the planner");
    for (size_t j = 0; j < q.jobs.size(); ++j)
        if (q.level(j) < level)
            return Err::e("planner.planSpread: topologyKey " + go_quote(topology_key.as_string()) +
                          " is finer than the exclusive topology of job " + q.jobs[j].name);
    std::vector<uint32_t> rc, rl;
    appendRuns(q.jobs, 0, q.jobs.size(), &rc, &rl);
    std::set<std::string> jobsets, own;
    for (const auto& j : q.jobs) {
        if (has_key(labels(*j.job), kJobSetNameKey)) jobsets.insert(ns_of(*j.job) + "/" + str_at(labels(*j.job), kJobSetNameKey));
        own.insert(has_key(labels(*j.job), kJobKey) ? str_at(labels(*j.job), kJobKey) : jobHashKey(ns_of(*j.job), j.name));
    }
    std::vector<std::string> given, used;
    if (peers.is_array())
        for (const auto& k : peers.elems()) {
            if (!k.is_string()) return Err::e("planner.planSpread: peers must be a list of job keys");
            given.push_back(k.as_string());
        }
    std::vector<int32_t> assign, spread;
    std::vector<uint32_t> count;
    std::string unknown;
    jsp_spread_stats st{};
    ++c.engine_calls;
    if (Err2 e = q.pl->place_spread(q.classes, rc, rl, level, mode == "DoNotSchedule" ? (uint32_t)max_skew.as_int() : JSP_SPREAD_SOFT,
                                    peers.is_array() ? &given : nullptr, jobsets, own, c.nodes, c.pods, &assign, &spread,
                                    &count, &used, &unknown, &st);
        !e.ok())
        return Err::e(e.msg);
    if (!unknown.empty()) return Err::e("planner.planSpread: peer " + go_quote(unknown) + " holds no domain");
    Json r = planReply(q, assign, st.placed), pk = Json::array(), cn = Json::object();
    const std::vector<std::string>& values = q.pl->domain_values(level);
    for (size_t j = 0; j < q.jobs.size(); ++j)
        r["jobs"].at(j)["spreadDomain"] = spread[j] >= 0 ? Json(values[spread[j]]) : Json();
    for (const auto& k : used) pk.push_back(k);
    for (size_t S = 0; S < values.size(); ++S) cn[values[S]] = (int64_t)count[S];
    r["topologyKey"] = topology_key.as_string();
    r["maxSkew"] = max_skew.as_int();
    r["whenUnsatisfiable"] = mode;
    r["peers"] = pk;
    r["counts"] = cn;
    r["refused"] = (int64_t)st.refused;
    r["skew"] = (int64_t)st.skew;
    *out = r;
    return Err::none();
}

// The front of planner.bind and planner.assume: planner.plan's, then
// `assignment` (byName) as one domain id per placed job and the runs.
Err openAssigned(Cache& c, const Json& jobs, const Json& assignment, const char* method, PlanRequest* q,
                 std::vector<uint32_t>* rc, std::vector<uint32_t>* rl, std::vector<int32_t>* assign) {
    if (Err e = openRequest(c, jobs, q); !e.ok) return e;
    const Json by_name = byName(assignment);
    if (!by_name.is_object())
        return Err::e(std::string(method) + ": assignment must be a plan or an object of job name -> domain");
    *assign = domainIds(*q, by_name);
    appendRuns(q->jobs, 0, q->jobs.size(), rc, rl);
    return Err::none();
}

// planner.bind: the jobs of planner.plan plus `assignment`, either a plan (the
// reply of planner.plan) or an object job name -> domain value; an unknown
// value or an absent job is unplaced. Every pod of a job whose domain is
// feasible on the current snapshot gets a node (jsp_bind_pods: first fit by
// row, pod 0 -- the leader -- on the domain's first fitting node). Per job:
// "name", "domain" (null: unplaced), "bound", and "nodes", the node name per
// completion index (null: unbound). The pod webhook pins a pod by its
// completion index (batch.kubernetes.io/job-completion-index) to nodes[index].
Err bindJobs(Cache& c, const Json& jobs, const Json& assignment, Json* out) {
    PlanRequest q;
    std::vector<uint32_t> rc, rl;
    std::vector<int32_t> assign;
    if (Err e = openAssigned(c, jobs, assignment, "planner.bind", &q, &rc, &rl, &assign); !e.ok) return e;
    std::vector<int32_t> pod_row;
    std::vector<uint64_t> pod_off;
    jsp_bind_stats st{};
    ++c.engine_calls;
    if (Err2 e = q.pl->bind(q.classes, rc, rl, assign, &pod_row, &pod_off, &st); !e.ok()) return Err::e(e.msg);
    Json r = Json::object();
    r["jobs"] = jobEntries(q, assign, nullptr);
    for (size_t j = 0; j < q.jobs.size(); ++j) {
        Json nodes = Json::array();
        bool bound = pod_off[j + 1] > pod_off[j];
        for (uint64_t p = pod_off[j]; p < pod_off[j + 1]; ++p) {
            if (pod_row[p] >= 0) {
                nodes.push_back(q.pl->row_node((uint32_t)pod_row[p]));
            } else {
                nodes.push_back(Json());
                bound = false;
            }
        }
        r["jobs"].at(j)["bound"] = bound;
        r["jobs"].at(j)["nodes"] = nodes;
    }
    r["bound"] = (int64_t)st.bound;
    r["stale"] = (int64_t)st.stale;
    r["rowsUsed"] = (int64_t)st.rows_used;
    r["pods"] = (int64_t)st.pods;
    r["podsBound"] = (int64_t)st.pods_bound;
    r["snapshot"] = q.snapshot;
    *out = r;
    return Err::none();
}

// planner.assume: planner.bind's request. Every job whose domain is feasible
// on the current snapshot is held: its rows are owned in the engine's snapshot
// (jsp_assume) and the planner's ledger keeps the hold across syncs and full
// uploads until a sync sees the job's pods (confirmed) or planner.forget names
// it. Per job: "name", "domain" (null: unplaced), "committed" and "owner" (the
// id its rows carry; null: unplaced); the totals "committed", "stale",
// "rowsMarked" and "assumed" (ledger entries now held). The sequence is plan
// -> bind -> assume -> create the Jobs; a bind after the assume finds the
// domains occupied.
Err assumeJobs(Cache& c, const Json& jobs, const Json& assignment, Json* out) {
    PlanRequest q;
    std::vector<uint32_t> rc, rl;
    std::vector<int32_t> assign;
    if (Err e = openAssigned(c, jobs, assignment, "planner.assume", &q, &rc, &rl, &assign); !e.ok) return e;
    std::vector<std::string> job_keys, names, jobsets;  // the key the jobs' pods will carry
    for (const auto& j : q.jobs) {
        job_keys.push_back(has_key(labels(*j.job), kJobKey) ? str_at(labels(*j.job), kJobKey)
                                                            : jobHashKey(ns_of(*j.job), j.name));
        names.push_back(j.name);
        jobsets.push_back(has_key(labels(*j.job), kJobSetNameKey)
                              ? ns_of(*j.job) + "/" + str_at(labels(*j.job), kJobSetNameKey)
                              : std::string());
    }
    std::vector<uint8_t> committed;
    std::vector<int32_t> owner;
    jsp_assume_stats st{};
    if (c.eng) ++c.engine_calls;
    if (Err2 e = q.pl->assume(q.classes, rc, rl, assign, job_keys, names, &committed, &owner, &st, &jobsets); !e.ok())
        return Err::e(e.msg);
    Json r = Json::object();
    r["jobs"] = jobEntries(q, assign, nullptr);
    for (size_t j = 0; j < q.jobs.size(); ++j) {
        r["jobs"].at(j)["committed"] = committed[j] != 0;
        r["jobs"].at(j)["owner"] = owner[j] != -1 ? Json((int64_t)owner[j]) : Json();
    }
    r["committed"] = (int64_t)st.committed;
    r["stale"] = (int64_t)st.stale;
    r["rowsMarked"] = (int64_t)st.rows_marked;
    r["assumed"] = (int64_t)q.pl->assumed();
    r["snapshot"] = q.snapshot;
    *out = r;
    return Err::none();
}

// planner.forget: {"jobs": [names]} -- the named jobs' holds are dropped and
// their rows freed (jsp_forget); names the ledger does not hold are ignored
// (a confirmed job's rows belong to the informer's id). "rowsCleared",
// "forgotten" (the names that were held) and "assumed" (entries still held).
Err forgetJobs(Cache& c, const Json& jobs, Json* out) {
    if (Err e = needPlanner(c); !e.ok) return e;
    if (!jobs.is_array()) return Err::e("planner.forget: jobs must be an array of job names");
    std::vector<std::string> names, forgotten;
    for (const auto& n : jobs.elems()) {
        if (!n.is_string()) return Err::e("planner.forget: jobs must be an array of job names");
        names.push_back(n.as_string());
    }
    uint64_t cleared = 0;
    if (c.eng) ++c.engine_calls;
    if (Err2 e = c.planner->forget(names, &cleared, &forgotten); !e.ok()) return Err::e(e.msg);
    Json r = Json::object(), fj = Json::array();
    for (const auto& n : forgotten) fj.push_back(n);
    r["rowsCleared"] = (int64_t)cleared;
    r["forgotten"] = fj;
    r["assumed"] = (int64_t)c.planner->assumed();
    *out = r;
    return Err::none();
}

// The recreate path consulting the engine (A10): the reconcile step after
// failurePolicyRecreateAll bumped status.restarts (failure_policy.go:155-175).
// getChildJobs buckets the old attempt into `delete` (jobset_controller.go:
// 281-290); while any is listed nothing is created (shouldCreateJob, :698-709,
// and the Foreground deletion, :553-576). Once they are gone, every
// replicatedJob's Jobs are constructed (constructJobsFromTemplate, :638-649,
// unchanged) and placed by the engine on the post-delete snapshot. The plan is
// reported beside the Jobs; the Jobs and the pods' mutations are not changed.
// previous_plan (optional): the `plan` object of an earlier reply; its jobs'
// name -> domain value map goes to the planner as the jobs' previous domains.
Err reconcileRecreate(Cache& c, const Json& js, const Json& jobs, Json* out, const Json& previous_plan = Json()) {
    Json owned;
    if (Err e = getChildJobs(js, jobs, &owned); !e.ok) return e;
    Json r = Json::object(), del = Json::array(), create = Json::array();
    for (const auto& j : owned.get("delete").elems()) del.push_back(name_of(j));
    if (owned.get("delete").size() == 0)
        for (const auto& rj : js.get("spec").get("replicatedJobs").elems()) {
            const Json made = constructJobsFromTemplate(js, rj, owned);  // outlives the loop below
            for (const auto& j : made.elems()) create.push_back(j);
        }
    r["delete"] = del;
    r["create"] = create;
    r["plan"] = Json();
    if (create.size() > 0 && c.planner) {
        Json plan, previous;
        // a plan only, never the map form: an object without "jobs" hints nothing
        if (previous_plan.is_object()) previous = previous_plan.get("jobs").is_array() ? byName(previous_plan) : Json::object();
        if (Err e = planJobs(c, create, &plan, false, previous); !e.ok) r["planError"] = e.msg;
        else r["plan"] = plan;
    }
    *out = r;
    return Err::none();
}

// ============================================================ node-selector strategy
// generate_namespaced_jobs, hack/label_nodes/label_nodes.py:99-112
Json generateNamespacedJobs(const Json& js) {
    const std::string ns = ns_of(js).empty() ? "default" : ns_of(js);
    Json out = Json::array();
    for (const auto& rj : js.get("spec").get("replicatedJobs").elems()) {
        const int64_t n = rj.has("replicas") ? rj.get("replicas").as_int() : 1;
        for (int64_t i = 0; i < n; ++i)
            out.push_back(ns + "_" + name_of(js) + "-" + rj.get("name").as_string() + "-" + std::to_string(i));
    }
    return out;
}

// Deterministic replacement for label_nodes.py (hack/label_nodes/
// label_nodes.py:36-120; its job -> node-pool map iterates a Python set,
// :115-120): the JobSet's jobs (generate_namespaced_jobs order) are placed on
// the exclusive-topology key's domains by the engine's lowest-index rule, and
// every node of a job's domain gets the script's patch body (:65-80).
Err labelNodes(Cache& c, const Json& js, Json* out) {
    if (Err e = needPlanner(c); !e.ok) return e;
    Planner& pl = *c.planner;
    const Json ns_jobs = generateNamespacedJobs(js);
    std::vector<ClassSpec> classes;
    std::vector<uint32_t> rc, rl;
    std::string key;
    for (const auto& rj : js.get("spec").get("replicatedJobs").elems()) {
        std::string k = "cloud.google.com/gke-nodepool";  // label_nodes.py:33 NODE_POOL_KEY
        if (has_key(annotations(js), kExclusiveKey)) k = str_at(annotations(js), kExclusiveKey);
        const Json& rja = rj.get("template").get("metadata").get("annotations");
        if (has_key(rja, kExclusiveKey)) k = str_at(rja, kExclusiveKey);
        if (!key.empty() && k != key) return Err::e("label nodes: replicated jobs use different topology keys");
        key = k;
        const Json& jspec = rj.get("template").get("spec");
        ClassSpec cs;
        const int64_t par = jspec.has("parallelism") ? jspec.get("parallelism").as_int() : 1;
        if (Err2 e = pl.class_of(jspec.get("template"), par, key, &cs); !e.ok()) return Err::e(e.msg);
        rc.push_back((uint32_t)classes.size());
        rl.push_back((uint32_t)(rj.has("replicas") ? rj.get("replicas").as_int() : 1));
        classes.push_back(std::move(cs));
    }
    if (classes.size() > JSP_MAX_CLASSES) return Err::e("label nodes: more than 64 replicated jobs");
    Json stats;
    if (Err2 e = pl.sync(c.nodes, c.pods, &stats); !e.ok()) return Err::e(e.msg);
    std::vector<int32_t> assign;
    jsp_stats st{};
    ++c.engine_calls;
    if (Err2 e = pl.place(classes, rc, rl, &assign, &st); !e.ok()) return Err::e(e.msg);
    std::vector<std::string> names;
    for (const auto& n : ns_jobs.elems()) names.push_back(n.as_string());
    const int level = pl.level_of(key);
    Json mapping = Json::object(), un = Json::array();
    for (size_t j = 0; j < names.size() && j < assign.size(); ++j) {
        if (assign[j] >= 0) mapping[names[j]] = pl.domain_values(level)[assign[j]];
        else un.push_back(names[j]);
    }
    Json r = Json::object();
    r["mapping"] = mapping;
    r["unplaceable"] = un;
    r["patches"] = label_nodes(pl, level, names, assign);
    *out = r;
    return Err::none();
}

// ============================================================ registry of caches
std::mutex g_mu;
std::map<int64_t, std::unique_ptr<Cache>> g_caches;
int64_t g_next = 1;

Cache* cache_of(const Json& req) {
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_caches.find(req.get("cache").as_int());
    if (it == g_caches.end()) throw std::runtime_error("unknown cache handle");
    return it->second.get();
}

Json ok(Json v) {
    Json r = Json::object();
    r["result"] = std::move(v);
    return r;
}
Json err_json(const Err& e, Json v = Json()) {
    Json r = Json::object();
    r["result"] = std::move(v);
    if (!e.ok) r["error"] = e.msg;
    return r;
}

Json dispatch(const std::string& m, const Json& q) {
    // ---- stateless
    if (m == "placement.GenJobName") return ok(GenJobName(q.get("jsName").as_string(), q.get("rjobName").as_string(), q.get("jobIndex").as_int()));
    if (m == "placement.GenPodName")
        return ok(GenPodName(q.get("jobSet").as_string(), q.get("replicatedJob").as_string(), q.get("jobIndex").as_string(),
                             q.get("podIndex").as_string()));
    if (m == "placement.IsLeaderPod") return ok(IsLeaderPod(q.get("pod")));
    if (m == "placement.explainMessage") {
        std::vector<std::string> res;
        for (const auto& r : q.get("resources").elems()) res.push_back(r.as_string());
        return ok(explain_message(q.get("counts"), q.get("topologyKey").as_string(), q.get("pods").as_int(), res,
                                  q.get("value").as_string()));
    }
    if (m == "controllers.sha1Hash") return ok(sha1Hash(q.get("s").as_string()));
    if (m == "controllers.jobHashKey") return ok(jobHashKey(q.get("ns").as_string(), q.get("jobName").as_string()));
    if (m == "controllers.namespacedJobName") return ok(namespacedJobName(q.get("ns").as_string(), q.get("jobName").as_string()));
    if (m == "controllers.globalJobIndex")
        return ok(globalJobIndex(q.get("jobSet"), q.get("replicatedJob").as_string(), q.get("jobIdx").as_int()));
    if (m == "controllers.removePodNameSuffix") {
        std::string out;
        Err e = removePodNameSuffix(q.get("podName").as_string(), &out);
        return err_json(e, out);
    }
    if (m == "controllers.labelAndAnnotateObject") {
        Json obj = q.get("obj");
        Json md = obj.get("metadata").is_object() ? obj.get("metadata") : Json::object();
        labelAndAnnotateObject(md, q.get("jobSet"), q.get("replicatedJob"), q.get("jobIdx").as_int());
        obj["metadata"] = md;
        return ok(obj);
    }
    if (m == "controllers.constructJob") return ok(constructJob(q.get("jobSet"), q.get("replicatedJob"), q.get("jobIdx").as_int()));
    if (m == "controllers.constructJobsFromTemplate")
        return ok(constructJobsFromTemplate(q.get("jobSet"), q.get("replicatedJob"), q.get("ownedJobs")));
    if (m == "controllers.shouldCreateJob") return ok(shouldCreateJob(q.get("jobName").as_string(), q.get("ownedJobs")));
    if (m == "controllers.getChildJobs") {
        Json out;
        Err e = getChildJobs(q.get("jobSet"), q.get("jobs"), &out);
        return err_json(e, out);
    }
    if (m == "controllers.failurePolicyRecreateAll") {
        Json js = q.get("jobSet");
        failurePolicyRecreateAll(js, q.get("shouldCountTowardsMax").as_bool());
        return ok(js);
    }
    if (m == "controllers.followerPodTopology") {
        std::string out;
        Err e = followerPodTopology(q.get("pod"), q.get("topologyKey").as_string(), &out);
        return err_json(e, out);
    }
    if (m == "controllers.updatePodCondition") {
        Json pod = q.get("pod");
        const bool changed = updatePodCondition(pod, q.get("condition"));
        Json r = Json::object();
        r["changed"] = changed;
        r["pod"] = pod;
        return ok(r);
    }
    if (m == "controllers.podIndexes") {
        Json r = Json::object();
        r[kPodNameKey] = Json::array();
        r[kPodJobKey] = Json::array();
        for (const auto& v : podNameIndex(q.get("pod"))) r[kPodNameKey].push_back(v);
        for (const auto& v : podJobKeyIndex(q.get("pod"))) r[kPodJobKey].push_back(v);
        return ok(r);
    }
    if (m == "controllers.podPredicate") {  // SetupWithManager event filter, pod_controller.go:66-71
        const Json& p = q.get("pod");
        return ok(IsLeaderPod(p) && podScheduled(p) && usingExclusivePlacement(p) && !podDeleted(p));
    }
    if (m == "webhooks.genLeaderPodName") {
        std::string out;
        Err e = genLeaderPodName(q.get("pod"), &out);
        return err_json(e, out);
    }
    if (m == "webhooks.podsOwnedBySameJob") return err_json(podsOwnedBySameJob(q.get("leaderPod"), q.get("followerPod")));
    if (m == "webhooks.setExclusiveAffinities") {
        Json pod = q.get("pod");
        setExclusiveAffinities(pod);
        return ok(pod);
    }
    if (m == "hack.generateNamespacedJobs") return ok(generateNamespacedJobs(q.get("jobSet")));
    // ---- caches
    if (m == "cache.new") {
        std::lock_guard<std::mutex> g(g_mu);
        const int64_t id = g_next++;
        g_caches[id] = std::make_unique<Cache>();
        return ok(id);
    }
    if (m == "cache.free") {
        std::lock_guard<std::mutex> g(g_mu);
        g_caches.erase(q.get("cache").as_int());
        return ok(true);
    }
    Cache& c = *cache_of(q);
    std::lock_guard<std::mutex> g(c.mu);
    if (m == "cache.add") {  // watch Added / Modified
        const Json& o = q.get("object");
        if (q.get("kind").as_string() == "Node") {
            c.nodes[name_of(o)] = o;
            if (c.planner) c.planner->note_node_event();  // its labels may have moved it to another domain
        } else {
            c.pods[ns_of(o) + "/" + name_of(o)] = o;
        }
        return ok(true);
    }
    if (m == "cache.remove") {  // watch Deleted
        if (q.get("kind").as_string() == "Node") {
            c.nodes.erase(q.get("name").as_string());
            if (c.planner) c.planner->note_node_event();  // a Node Get now answers NotFound -> ""
        } else {
            c.pods.erase(q.get("namespace").as_string() + "/" + q.get("name").as_string());
        }
        return ok(true);
    }
    if (m == "planner.new") {
        std::vector<std::string> lk, res;
        for (const auto& k : q.get("levelKeys").elems()) lk.push_back(k.as_string());
        for (const auto& r : q.get("resources").elems()) res.push_back(r.as_string());
        c.eng = reinterpret_cast<jsp_engine*>((uintptr_t)q.get("engine").as_int());
        c.planner = std::make_unique<Planner>(c.eng, lk, res);
        return ok(true);
    }
    if (m == "planner.sync" || m == "planner.columns") {
        if (Err e = needPlanner(c); !e.ok) return err_json(e);
        Json stats;
        if (Err2 e = c.planner->sync(c.nodes, c.pods, &stats); !e.ok()) return err_json(Err::e(e.msg));
        return ok(m == "planner.sync" ? stats : c.planner->columns());
    }
    if (m == "planner.encode") {  // classes of `jobs` without placing (tests, oracle inputs): the front and the tail
        PlanRequest pq;
        if (Err e = openRequest(c, q.get("jobs"), &pq); !e.ok) return err_json(e);
        Json r = Json::object();
        replyTail(pq, &r, false);
        return ok(r);
    }
    if (m == "planner.plan") {
        Json out;
        Err e = planJobs(c, q.get("jobs"), &out, false, q.get("previous"));
        return err_json(e, out);
    }
    if (m == "planner.planGangs") {
        Json out;
        Err e = planGangs(c, q.get("jobs"), q.get("spans"), &out);
        return err_json(e, out);
    }
    if (m == "planner.planFit") {
        Json out;
        Err e = planFit(c, q.get("jobs"), q.get("policy"), &out);
        return err_json(e, out);
    }
    if (m == "planner.whatIf") {
        Json out;
        Err e = whatIf(c, q.get("jobs"), q.get("scenarios"), &out);
        return err_json(e, out);
    }
    if (m == "planner.preempt") {
        Json out;
        Err e = preemptJobs(c, q.get("jobs"), q.get("priority"), &out);
        return err_json(e, out);
    }
    if (m == "planner.planSpread") {
        Json out;
        Err e = planSpread(c, q.get("jobs"), q.get("topologyKey"), q.get("maxSkew"), q.get("whenUnsatisfiable"),
                           q.get("peers"), &out);
        return err_json(e, out);
    }
    if (m == "planner.bind") {
        Json out;
        Err e = bindJobs(c, q.get("jobs"), q.get("assignment"), &out);
        return err_json(e, out);
    }
    if (m == "planner.assume") {
        Json out;
        Err e = assumeJobs(c, q.get("jobs"), q.get("assignment"), &out);
        return err_json(e, out);
    }
    if (m == "planner.forget") {
        Json out;
        Err e = forgetJobs(c, q.get("jobs"), &out);
        return err_json(e, out);
    }
    if (m == "planner.explain") {
        Json out;
        Err e = planJobs(c, q.get("jobs"), &out, true);
        return err_json(e, out);
    }
    if (m == "controllers.reconcileRecreate") {
        Json out;
        Err e = reconcileRecreate(c, q.get("jobSet"), q.get("jobs"), &out, q.get("previousPlan"));
        return err_json(e, out);
    }
    if (m == "hack.labelNodes") {
        Json out;
        Err e = labelNodes(c, q.get("jobSet"), &out);
        return err_json(e, out);
    }
    if (m == "webhooks.DefaultBatch") return ok(DefaultBatch(c, q.get("pods")));
    if (m == "cache.inject") {
        if (q.get("error").is_null()) c.inject.erase(q.get("what").as_string());
        else c.inject[q.get("what").as_string()] = q.get("error").as_string();
        return ok(true);
    }
    if (m == "cache.stats") {
        Json r = Json::object();
        r["nodeGets"] = c.node_gets;
        r["podLists"] = c.pod_lists;
        r["engineCalls"] = c.engine_calls;
        r["deleted"] = Json::array();
        for (auto& d : c.deleted) r["deleted"].push_back(d);
        r["statusUpdates"] = Json::array();
        for (auto& d : c.status_updates) r["statusUpdates"].push_back(d);
        r["pods"] = Json::array();
        for (auto& kv : c.pods) r["pods"].push_back(kv.second);
        return ok(r);
    }
    if (m == "cache.bindEngine") {
        c.eng = reinterpret_cast<jsp_engine*>((uintptr_t)q.get("engine").as_int());
        c.node_rows.clear();
        for (const auto& kv : q.get("nodeRows").items()) c.node_rows[kv.first] = (int32_t)kv.second.as_int();
        c.level_keys.clear();
        for (const auto& k : q.get("levelKeys").elems()) c.level_keys.push_back(k.as_string());
        c.domain_values.clear();
        for (const auto& lv : q.get("domainValues").elems()) {
            std::vector<std::string> v;
            for (const auto& x : lv.elems()) v.push_back(x.as_string());
            c.domain_values.push_back(std::move(v));
        }
        return ok(true);
    }
    if (m == "webhooks.Default") {
        Json pod = q.get("pod");
        Err e = Default(c, pod);
        return err_json(e, pod);
    }
    if (m == "webhooks.ValidateCreate") return err_json(ValidateCreate(c, q.get("pod")));
    if (m == "webhooks.leaderPodForFollower") {
        Json leader;
        Err e = leaderPodForFollower(c, q.get("pod"), &leader);
        return err_json(e, leader);
    }
    if (m == "controllers.validatePodPlacements") {
        bool valid = false;
        Err e = validatePodPlacements(c, q.get("leaderPod"), q.get("podList"), &valid);
        return err_json(e, valid);
    }
    if (m == "controllers.deleteFollowerPods")
        return err_json(deleteFollowerPods(c, q.get("pods"), q.get("now").as_string()));
    if (m == "controllers.Reconcile")
        return err_json(Reconcile(c, q.get("namespace").as_string(), q.get("name").as_string(), q.get("now").as_string()));
    throw std::runtime_error("unknown method " + m);
}

}  // namespace jsk

extern "C" int jsk_call(const char* method, const char* request_json, char** response_json) {
    if (!method || !response_json) return JSP_EINVAL;
    std::string out;
    int rc = JSP_OK;
    try {
        const jsk::Json q = jsk::Json::parse(request_json ? request_json : "{}");
        out = jsk::dispatch(method, q).dump();
    } catch (const std::exception& ex) {
        jsk::Json r = jsk::Json::object();
        r["error"] = std::string("jsk_call: ") + ex.what();
        out = r.dump();
        rc = JSP_EINVAL;
    }
    char* p = static_cast<char*>(std::malloc(out.size() + 1));
    if (!p) return JSP_ENOMEM;
    std::memcpy(p, out.c_str(), out.size() + 1);
    *response_json = p;
    return rc;
}

extern "C" void jsk_free(char* p) { std::free(p); }
