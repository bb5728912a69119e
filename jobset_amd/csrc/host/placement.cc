// placement.cc — see placement.h. Snapshot ingestion from informer-cache
// objects, requirement classes from pod templates, and the plan call.
//
// Reference reads this replaces: the per-pod Node Gets of topologyFromPod
// (pkg/webhooks/pod_mutating_webhook.go:181-189) and leaderPodTopology
// (pkg/controllers/pod_controller.go:250-258), over the nodes the manager may
// list and watch (config/components/rbac/role.yaml:16-23). The predicate
// semantics restate kube-scheduler's NodeAffinity / TaintToleration /
// NodeResourcesFit filters, which are not in the reference:
// parity unpinned, see DESIGN.md §2.
#include "placement.h"

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

namespace jsk {

namespace {

const char* const kExclusiveKey = "alpha.jobset.sigs.k8s.io/exclusive-topology";  // jobset_types.go:41
const char* const kJobKey = "jobset.sigs.k8s.io/job-key";                         // jobset_types.go:35
const char* const kJobSetNameKey = "jobset.sigs.k8s.io/jobset-name";
const char* const kNamespacedJobKey = "alpha.jobset.sigs.k8s.io/namespaced-job";  // jobset_types.go:47
const char* const kNoScheduleTaintKey = "alpha.jobset.sigs.k8s.io/no-schedule";   // jobset_types.go:48
const char* const kUnschedulableTaint = "node.kubernetes.io/unschedulable";        // what the node controller sets for spec.unschedulable

bool parse_int64(const std::string& s, int64_t* v) {  // strconv.ParseInt(s, 10, 64)
    if (s.empty()) return false;
    char* end = nullptr;
    errno = 0;
    const long long x = std::strtoll(s.c_str(), &end, 10);
    if (errno != 0 || *end != '\0' || std::isspace((unsigned char)s[0])) return false;
    *v = x;
    return true;
}

const Json& labels_of(const Json& o) { return o.get("metadata").get("labels"); }

Err2 engine_error() { return {std::string("placement engine: ") + jsp_last_error()}; }  // after a jsp_* call failed

}  // namespace

// ------------------------------------------------------------------ dictionaries
bool LabelPred::operator<(const LabelPred& o) const {
    if (key != o.key) return key < o.key;
    if (op != o.op) return op < o.op;
    return values < o.values;
}
bool LabelPred::operator==(const LabelPred& o) const { return key == o.key && op == o.op && values == o.values; }

bool LabelPred::holds(const Json& labels) const {
    if (!has_key(labels, key)) return false;
    const std::string& v = labels.get(key).as_string();
    if (op == "Exists") return true;
    if (op == "In") return std::binary_search(values.begin(), values.end(), v);
    int64_t a = 0, b = 0;
    if (values.size() != 1 || !parse_int64(v, &a) || !parse_int64(values[0], &b)) return false;
    return op == "Gt" ? a > b : a < b;
}

bool TaintKey::operator<(const TaintKey& o) const {
    if (key != o.key) return key < o.key;
    if (value != o.value) return value < o.value;
    return effect < o.effect;
}
bool TaintKey::operator==(const TaintKey& o) const { return key == o.key && value == o.value && effect == o.effect; }

// ToleratesTaint (k8s.io/api/core/v1/toleration.go)
static bool tolerates(const Json& t, const TaintKey& taint) {
    const std::string eff = t.get("effect").as_string(), key = t.get("key").as_string();
    const std::string op = t.get("operator").as_string();
    if (!eff.empty() && eff != taint.effect) return false;
    if (!key.empty() && key != taint.key) return false;
    if (op.empty() || op == "Equal") return t.get("value").as_string() == taint.value;
    return op == "Exists";
}

// ------------------------------------------------------------------ quantities
bool parse_quantity(const std::string& q, const std::string& resource, bool round_up, uint64_t* out) {
    if (q.empty()) return false;
    size_t i = 0;
    if (q[i] == '+') ++i;
    const size_t num_begin = i;
    while (i < q.size() && (std::isdigit((unsigned char)q[i]) || q[i] == '.')) ++i;
    if (i == num_begin) return false;
    long double v = std::strtold(q.substr(num_begin, i - num_begin).c_str(), nullptr);
    const std::string suf = q.substr(i);
    long double mul = 1;
    if (suf.empty()) mul = 1;
    else if (suf == "m") mul = 1e-3L;
    else if (suf == "k") mul = 1e3L;
    else if (suf == "M") mul = 1e6L;
    else if (suf == "G") mul = 1e9L;
    else if (suf == "T") mul = 1e12L;
    else if (suf == "P") mul = 1e15L;
    else if (suf == "E") mul = 1e18L;
    else if (suf == "Ki") mul = 1024.0L;
    else if (suf == "Mi") mul = 1024.0L * 1024;
    else if (suf == "Gi") mul = 1024.0L * 1024 * 1024;
    else if (suf == "Ti") mul = 1024.0L * 1024 * 1024 * 1024;
    else if (suf == "Pi") mul = 1024.0L * 1024 * 1024 * 1024 * 1024;
    else if (suf == "Ei") mul = 1024.0L * 1024 * 1024 * 1024 * 1024 * 1024;
    else if (suf[0] == 'e' || suf[0] == 'E') {
        char* end = nullptr;
        const long e = std::strtol(suf.c_str() + 1, &end, 10);
        if (*end != '\0' || suf.size() < 2) return false;
        mul = std::pow(10.0L, (long double)e);
    } else {
        return false;
    }
    v *= mul;
    long double unit = 1;
    if (resource == "cpu") unit = 1e-3L;                                          // millicores
    else if (resource == "memory" || resource == "ephemeral-storage") unit = 1024.0L * 1024;  // MiB
    long double x = v / unit;
    x = round_up ? std::ceil(x - 1e-9L) : std::floor(x + 1e-9L);
    if (x < 0) x = 0;
    *out = x > 1.8e19L ? ~0ull : (uint64_t)x;
    return true;
}

static uint64_t container_sum(const Json& containers, const std::string& resource) {
    uint64_t s = 0;
    for (const auto& c : containers.elems()) {
        uint64_t v = 0;
        const Json& r = c.get("resources").get("requests");
        if (has_key(r, resource) && parse_quantity(r.get(resource).as_string(), resource, true, &v)) s += v;
    }
    return s;
}

uint64_t pod_request(const Json& podSpec, const std::string& resource) {
    const uint64_t sum = container_sum(podSpec.get("containers"), resource);
    uint64_t init_max = 0;
    for (const auto& c : podSpec.get("initContainers").elems()) {
        Json one = Json::array();
        one.push_back(c);
        init_max = std::max(init_max, container_sum(one, resource));
    }
    return std::max(sum, init_max);
}

// ------------------------------------------------------------------ planner
Planner::Planner(jsp_engine* e, std::vector<std::string> level_keys, std::vector<std::string> resources)
    : eng_(e), level_keys_(std::move(level_keys)), res_(std::move(resources)) {}

int Planner::level_of(const std::string& key) const {
    for (size_t k = 0; k < level_keys_.size(); ++k)
        if (level_keys_[k] == key) return (int)k;
    return -1;
}

bool Planner::row_of(const std::string& node, int32_t* row) const {
    auto it = node_row_.find(node);
    if (it == node_row_.end()) return false;
    *row = it->second;
    return true;
}

int32_t Planner::domain_id(int level, const std::string& value) const {
    if (level < 0 || (size_t)level >= domain_ids_.size()) return -1;
    auto it = domain_ids_[level].find(value);
    return it == domain_ids_[level].end() ? -1 : it->second;
}

void Planner::domain_rows(int level, int32_t d, uint32_t* first, uint32_t* end) const {
    const uint32_t a = first_leaf_[level][d], b = first_leaf_[level][d + 1];
    *first = leaf_start_[a];
    *end = leaf_start_[b];
}

int32_t Planner::row_domain(uint32_t row, int level) const {
    const uint32_t leaf = (uint32_t)(std::upper_bound(leaf_start_.begin(), leaf_start_.end(), row) - leaf_start_.begin()) - 1;
    const auto& fl = first_leaf_[level];
    return (int32_t)(std::upper_bound(fl.begin(), fl.end(), leaf) - fl.begin()) - 1;
}

int Planner::pred_bit(const LabelPred& p) const {
    auto it = std::lower_bound(preds_.begin(), preds_.end(), p);
    return (it != preds_.end() && *it == p) ? (int)(it - preds_.begin()) : -1;
}

// A node's allocatable resources into row i of fr [R][N].
void Planner::allocatable(const Json& node, uint32_t N, uint32_t i, std::vector<uint32_t>* fr) const {
    const Json& alloc = node.get("status").get("allocatable");
    for (size_t r = 0; r < res_.size(); ++r) {
        uint64_t v = 0;
        if (has_key(alloc, res_[r])) parse_quantity(alloc.get(res_[r]).as_string(), res_[r], false, &v);
        (*fr)[r * N + i] = (uint32_t)std::min<uint64_t>(v, 0xFFFFFFFFull);
    }
}

// Bound, non-terminal pods: their requests come off their node's free
// resources (fr, saturating per pod); an exclusive pod covers its node's domain
// at its key's level with its job's dense id (sorted job keys). Then the
// assumed domains (Planner::assume): an entry whose job the informer's pods
// now cover is confirmed, one whose domain value is gone is void -- both go to
// `drop` -- and the others lie over the rows the informer leaves free.
// without (planner.whatIf's evictions): the pods carrying one of these job
// keys and the ledger entries of these keys are left out. seen: every job key
// met, on a pod or in the ledger.
void Planner::occupy(const std::map<std::string, Json>& pods, const std::map<std::string, int32_t>& node_row,
                     const std::vector<const Json*>& row_json, const std::vector<std::map<std::string, int32_t>>& did,
                     const std::vector<uint32_t>& leaf_start, const std::vector<std::vector<uint32_t>>& fl,
                     const std::set<std::string>* without, std::vector<uint32_t>* fr_io, std::vector<int32_t>* ex_io,
                     std::map<std::string, int32_t>* job_ids_out, std::vector<std::string>* drop,
                     std::set<std::string>* seen) const {
    const size_t K = level_keys_.size(), R = res_.size();
    const uint32_t N = (uint32_t)row_json.size();
    std::vector<uint32_t>& fr = *fr_io;
    std::vector<int32_t>& ex = *ex_io;
    std::map<std::string, int32_t> job_ids;  // job-key -> dense id (sorted)
    std::vector<std::pair<std::string, std::pair<int, int32_t>>> covers;  // job-key, (level, domain)
    for (const auto& kv : pods) {
        const Json& pod = kv.second;
        const bool keyed = has_key(labels_of(pod), kJobKey);
        const std::string jk = keyed ? labels_of(pod).get(kJobKey).as_string() : std::string();
        if (keyed && seen) seen->insert(jk);
        if (keyed && without && without->count(jk)) continue;
        const std::string nn = pod.get("spec").get("nodeName").as_string();
        const std::string phase = pod.get("status").get("phase").as_string();
        if (nn.empty() || phase == "Succeeded" || phase == "Failed") continue;
        auto it = node_row.find(nn);
        if (it == node_row.end()) continue;
        const uint32_t i = (uint32_t)it->second;
        for (size_t r = 0; r < R; ++r) {
            const uint64_t q = pod_request(pod.get("spec"), res_[r]);
            fr[r * N + i] = (uint32_t)(q >= fr[r * N + i] ? 0 : fr[r * N + i] - q);
        }
        const Json& ann = pod.get("metadata").get("annotations");
        if (!has_key(ann, kExclusiveKey) || !keyed) continue;
        const int lvl = level_of(ann.get(kExclusiveKey).as_string());
        if (lvl < 0) continue;  // a key that is not an engine level: not modelled
        const std::string& v = labels_of(*row_json[i]).get(level_keys_[lvl]).as_string();
        const auto dv = did[lvl].find(v);
        if (dv == did[lvl].end()) continue;  // (a node relabelled since the sync: never inside rebuild)
        covers.push_back({jk, {lvl, dv->second}});
        job_ids[jk] = 0;
    }
    int32_t next = 0;
    for (auto& kv : job_ids) kv.second = next++;
    for (const auto& c : covers) {
        const uint32_t a = leaf_start[fl[c.second.first][c.second.second]];
        const uint32_t b = leaf_start[fl[c.second.first][c.second.second + 1]];
        for (uint32_t i = a; i < b; ++i) ex[i] = job_ids[c.first];
    }
    for (const auto& kv : ledger_) {
        const Assumed& a = kv.second;
        if (seen) seen->insert(kv.first);
        if (without && without->count(kv.first)) continue;
        int32_t d = -1;
        if (!job_ids.count(kv.first) && a.level >= 0 && (size_t)a.level < K) {
            const auto f = did[a.level].find(a.value);
            if (f != did[a.level].end()) d = f->second;
        }
        if (d < 0) {
            if (drop) drop->push_back(kv.first);
            continue;
        }
        const uint32_t r0 = leaf_start[fl[a.level][d]], r1 = leaf_start[fl[a.level][d + 1]];
        for (uint32_t i = r0; i < r1; ++i)
            if (ex[i] == -1) ex[i] = a.owner;
    }
    if (job_ids_out) *job_ids_out = std::move(job_ids);
}

Err2 Planner::cache_columns(const std::map<std::string, Json>& nodes, const std::map<std::string, Json>& pods,
                            const std::set<std::string>* without, std::vector<uint32_t>* fr, std::vector<int32_t>* ex,
                            std::map<std::string, int32_t>* job_ids, std::set<std::string>* seen) const {
    if (Err2 e = in_step(); !e.ok()) return e;
    const uint32_t N = (uint32_t)row_node_.size(), R = (uint32_t)res_.size();
    std::vector<const Json*> row_json(N);
    for (uint32_t i = 0; i < N; ++i) {
        const auto it = nodes.find(row_node_[i]);
        if (it == nodes.end()) return {"planner: snapshot out of date (node " + row_node_[i] + " is gone)"};
        row_json[i] = &it->second;
    }
    fr->assign((size_t)R * N, 0);
    ex->assign(N, -1);
    for (uint32_t i = 0; i < N; ++i) allocatable(*row_json[i], N, i, fr);
    occupy(pods, node_row_, row_json, domain_ids_, leaf_start_, first_leaf_, without, fr, ex, job_ids, nullptr, seen);
    return {};
}

// planner.whatIf's scenario: the free_res and excl_owner columns sync would
// build from the same cache without the pods and the ledger entries of `keys`
// (occupy with its filter, so the per-pod saturating subtraction stays exact),
// as a delta against the current columns. A row enters iff its free_res
// differs or it becomes unowned; a row that stays owned keeps its current
// owner value (the dense ids would shift). *unknown: a key no pod and no
// ledger entry carries ("" = none).
Err2 Planner::evict_delta(const std::map<std::string, Json>& nodes, const std::map<std::string, Json>& pods,
                          const std::set<std::string>& keys, std::vector<uint32_t>* rows, std::vector<uint32_t>* fr_out,
                          std::vector<int32_t>* ex_out, std::string* unknown) const {
    const uint32_t N = (uint32_t)row_node_.size(), R = (uint32_t)res_.size();
    std::vector<uint32_t> fr;
    std::vector<int32_t> ex;
    std::set<std::string> seen;
    if (Err2 e = cache_columns(nodes, pods, &keys, &fr, &ex, nullptr, &seen); !e.ok()) return e;
    unknown->clear();
    for (const auto& k : keys)
        if (!seen.count(k)) {
            *unknown = k;
            return {};
        }
    rows->clear();
    for (uint32_t i = 0; i < N; ++i) {
        bool d = excl_[i] != -1 && ex[i] == -1;
        for (uint32_t r = 0; r < R && !d; ++r) d = fr[(size_t)r * N + i] != free_[(size_t)r * N + i];
        if (d) rows->push_back(i);
    }
    const size_t n = rows->size();
    fr_out->assign((size_t)R * n, 0);
    ex_out->assign(n, -1);
    for (size_t j = 0; j < n; ++j) {
        const uint32_t i = (*rows)[j];
        for (uint32_t r = 0; r < R; ++r) (*fr_out)[(size_t)r * n + j] = fr[(size_t)r * N + i];
        (*ex_out)[j] = ex[i] == -1 ? -1 : excl_[i];
    }
    return {};
}

Err2 Planner::rebuild(const std::map<std::string, Json>& nodes, const std::map<std::string, Json>& pods) {
    const size_t K = level_keys_.size(), R = res_.size();
    if (K < 1 || K > JSP_MAX_LEVELS) return {"planner: 1.." + std::to_string(JSP_MAX_LEVELS) + " topology keys"};
    if (R < 1 || R > JSP_MAX_RES) return {"planner: 1.." + std::to_string(JSP_MAX_RES) + " resources"};
    if (preds_.size() > 64u * JSP_MAX_LABEL_WORDS)
        return {"planner: " + std::to_string(preds_.size()) + " label predicates exceed the engine's " +
                std::to_string(64 * JSP_MAX_LABEL_WORDS)};
    // nodes carrying every level label, sorted by (level values..., name)
    struct Row {
        std::vector<std::string> key;
        const Json* node;
    };
    std::vector<Row> rows;
    std::vector<std::string> skipped;
    std::set<TaintKey> taint_set;
    for (const auto& kv : nodes) {
        const Json& lab = labels_of(kv.second);
        Row r{{}, &kv.second};
        bool ok = true;
        for (const auto& k : level_keys_) {
            if (!has_key(lab, k)) { ok = false; break; }
            r.key.push_back(lab.get(k).as_string());
        }
        if (!ok) { skipped.push_back(kv.first); continue; }
        r.key.push_back(kv.first);
        rows.push_back(std::move(r));
        for (const auto& t : kv.second.get("spec").get("taints").elems()) {
            const std::string eff = t.get("effect").as_string();
            if (eff == "NoSchedule" || eff == "NoExecute")
                taint_set.insert({t.get("key").as_string(), t.get("value").as_string(), eff});
        }
        if (kv.second.get("spec").get("unschedulable").as_bool()) taint_set.insert({kUnschedulableTaint, "", "NoSchedule"});
    }
    if (taint_set.size() > 32) return {"planner: " + std::to_string(taint_set.size()) + " distinct NoSchedule/NoExecute taints exceed 32"};
    std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.key < b.key; });
    const uint32_t N = (uint32_t)rows.size();
    // domains per level; a level-k value must sit under exactly one level-(k-1) domain
    std::vector<std::vector<std::string>> dv(K);
    std::vector<std::map<std::string, int32_t>> did(K);
    std::vector<std::vector<uint32_t>> dstart(K);  // first row of each domain
    for (uint32_t i = 0; i < N; ++i) {
        for (size_t k = 0; k < K; ++k) {
            bool fresh = i == 0;
            for (size_t j = 0; j <= k && !fresh; ++j) fresh = rows[i].key[j] != rows[i - 1].key[j];
            if (!fresh) continue;
            const std::string& v = rows[i].key[k];
            if (did[k].count(v))
                return {"planner: topology key " + level_keys_[k] + " value " + v + " spans several " +
                        (k ? level_keys_[k - 1] : std::string("")) + " domains (keys must nest)"};
            did[k][v] = (int32_t)dv[k].size();
            dv[k].push_back(v);
            dstart[k].push_back(i);
        }
    }
    const uint32_t L = (uint32_t)dv[K - 1].size();
    std::vector<uint32_t> leaf_start(dstart[K - 1]);
    leaf_start.push_back(N);
    std::vector<std::vector<uint32_t>> fl(K);
    for (size_t k = 0; k < K; ++k) {
        for (uint32_t r0 : dstart[k])  // the leaf that starts at a domain's first row
            fl[k].push_back((uint32_t)(std::lower_bound(dstart[K - 1].begin(), dstart[K - 1].end(), r0) - dstart[K - 1].begin()));
        fl[k].push_back(L);
    }
    // columns
    std::vector<TaintKey> taints(taint_set.begin(), taint_set.end());
    const uint32_t W = std::max<uint32_t>(1, (uint32_t)((preds_.size() + 63) / 64));
    std::vector<uint64_t> lab((size_t)W * N, 0);
    std::vector<uint32_t> tb(N, 0), fr((size_t)R * N, 0);
    std::vector<int32_t> ex(N, -1);
    std::map<std::string, int32_t> node_row;
    std::vector<std::string> row_node(N);
    for (uint32_t i = 0; i < N; ++i) {
        const Json& node = *rows[i].node;
        const std::string name = rows[i].key.back();
        row_node[i] = name;
        node_row[name] = (int32_t)i;
        const Json& nl = labels_of(node);
        for (size_t b = 0; b < preds_.size(); ++b)
            if (preds_[b].holds(nl)) lab[(b >> 6) * N + i] |= 1ull << (b & 63);
        for (const auto& t : node.get("spec").get("taints").elems()) {
            const TaintKey key{t.get("key").as_string(), t.get("value").as_string(), t.get("effect").as_string()};
            auto it = std::lower_bound(taints.begin(), taints.end(), key);
            if (it != taints.end() && *it == key) tb[i] |= 1u << (it - taints.begin());
        }
        if (node.get("spec").get("unschedulable").as_bool()) {
            const TaintKey key{kUnschedulableTaint, "", "NoSchedule"};
            tb[i] |= 1u << (std::lower_bound(taints.begin(), taints.end(), key) - taints.begin());
        }
        allocatable(node, N, i, &fr);
    }
    // bound pods' requests, the exclusive jobs' covers and the assumed domains (occupy)
    std::vector<const Json*> row_json(N);
    for (uint32_t i = 0; i < N; ++i) row_json[i] = rows[i].node;
    std::map<std::string, int32_t> job_ids;
    std::vector<std::string> drop;
    occupy(pods, node_row, row_json, did, leaf_start, fl, nullptr, &fr, &ex, &job_ids, &drop, nullptr);
    for (const auto& k : drop) ledger_.erase(k);
    // commit
    taints_ = std::move(taints);
    row_node_ = std::move(row_node);
    node_row_ = std::move(node_row);
    domain_values_ = std::move(dv);
    domain_ids_ = std::move(did);
    first_leaf_ = std::move(fl);
    leaf_start_ = std::move(leaf_start);
    W_ = W;
    labels_ = std::move(lab);
    taint_bits_ = std::move(tb);
    free_ = std::move(fr);
    excl_ = std::move(ex);
    skipped_ = std::move(skipped);
    exclusive_jobs_ = (uint32_t)job_ids.size();
    return {};
}

Err2 Planner::upload_full() {
    const uint32_t K = (uint32_t)level_keys_.size();
    jsp_topology t{};
    t.n_levels = K;
    for (uint32_t k = 0; k < K; ++k) {
        t.n_domains[k] = (uint32_t)domain_values_[k].size();
        t.first_leaf[k] = first_leaf_[k].data();
    }
    if (jsp_topology_upload(eng_, &t) != JSP_OK) return engine_error();
    jsp_nodes n{};
    n.n_nodes = (uint32_t)row_node_.size();
    n.leaf_begin = 0;
    n.n_leaves = (uint32_t)leaf_start_.size() - 1;
    n.leaf_start = leaf_start_.data();
    n.n_label_words = W_;
    n.labels = labels_.data();
    n.taints = taint_bits_.data();
    n.n_res = (uint32_t)res_.size();
    n.free_res = free_.data();
    n.excl_owner = excl_.data();
    if (jsp_snapshot_upload(eng_, &n) != JSP_OK) return engine_error();
    classes_gone_ = true;  // a topology upload drops the engine's classes
    return {};
}

Err2 Planner::sync(const std::map<std::string, Json>& nodes, const std::map<std::string, Json>& pods, Json* stats) {
    // previous structure and columns, to decide between a patch and a full upload
    const std::vector<std::string> old_rows = row_node_;
    const std::vector<std::vector<uint32_t>> old_fl = first_leaf_;
    const std::vector<uint32_t> old_ls = leaf_start_;
    const std::vector<TaintKey> old_taints = taints_;
    const uint32_t old_W = W_;
    const std::vector<uint64_t> old_lab = labels_;
    const std::vector<uint32_t> old_tb = taint_bits_, old_fr = free_;
    const std::vector<int32_t> old_ex = excl_;
    if (Err2 e = rebuild(nodes, pods); !e.ok()) return e;
    nodes_dirty_ = false;  // the rebuilt host columns reflect every Node event so far
    const uint32_t N = (uint32_t)row_node_.size(), R = (uint32_t)res_.size();
    const bool same = synced_ && !preds_dirty_ && old_rows == row_node_ && old_fl == first_leaf_ &&
                      old_ls == leaf_start_ && old_taints == taints_ && old_W == W_;
    std::string upload = "none";
    uint32_t patched = 0;
    if (eng_ == nullptr) {  // host-only planner (tests of the ingestion itself)
        preds_dirty_ = false;
        synced_ = true;
        upload = "none (no engine)";
    } else if (!same) {
        if (Err2 e = upload_full(); !e.ok()) { synced_ = false; return e; }
        upload = "full";
        preds_dirty_ = false;
        synced_ = true;
    } else {
        std::vector<uint32_t> rows;
        for (uint32_t i = 0; i < N; ++i) {
            bool d = old_tb[i] != taint_bits_[i] || old_ex[i] != excl_[i];
            for (uint32_t w = 0; w < W_ && !d; ++w) d = old_lab[(size_t)w * N + i] != labels_[(size_t)w * N + i];
            for (uint32_t r = 0; r < R && !d; ++r) d = old_fr[(size_t)r * N + i] != free_[(size_t)r * N + i];
            if (d) rows.push_back(i);
        }
        if (!rows.empty()) {
            const uint32_t n = (uint32_t)rows.size();
            std::vector<uint64_t> dl((size_t)W_ * n);
            std::vector<uint32_t> dt(n), df((size_t)R * n);
            std::vector<int32_t> de(n);
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t i = rows[j];
                for (uint32_t w = 0; w < W_; ++w) dl[(size_t)w * n + j] = labels_[(size_t)w * N + i];
                for (uint32_t r = 0; r < R; ++r) df[(size_t)r * n + j] = free_[(size_t)r * N + i];
                dt[j] = taint_bits_[i];
                de[j] = excl_[i];
            }
            if (jsp_snapshot_patch(eng_, rows.data(), n, dl.data(), dt.data(), df.data(), de.data()) != JSP_OK) {
                // the host columns are already the new ones: without this the
                // next sync would find nothing to patch and the engine would
                // keep the old rows for good; a full upload repairs it
                synced_ = false;
                return engine_error();
            }
            upload = "patch";
            patched = n;
        }
    }
    if (stats) {
        Json s = Json::object();
        s["rows"] = (int64_t)N;
        s["leaves"] = (int64_t)(leaf_start_.size() - 1);
        Json dom = Json::array();
        for (const auto& v : domain_values_) dom.push_back((int64_t)v.size());
        s["domains"] = dom;
        s["labelWords"] = (int64_t)W_;
        s["labelPredicates"] = (int64_t)preds_.size();
        s["taintBits"] = (int64_t)taints_.size();
        Json sk = Json::array();
        for (const auto& n : skipped_) sk.push_back(n);
        s["skippedNodes"] = sk;
        s["upload"] = upload;
        s["patchedRows"] = (int64_t)patched;
        s["exclusiveJobs"] = (int64_t)exclusive_jobs_;
        *stats = s;
    }
    return {};
}

Err2 Planner::class_of(const Json& tmpl, int64_t parallelism, const std::string& topology_key, ClassSpec* out) {
    ClassSpec c;
    c.level = level_of(topology_key);
    if (c.level < 0) return {"planner: exclusive-topology key " + topology_key + " is not one of the engine's topology keys"};
    c.pods = (uint32_t)std::max<int64_t>(1, parallelism);
    const Json& spec = tmpl.get("spec");
    for (const auto& kv : spec.get("nodeSelector").items())
        c.req.push_back({kv.first, "In", {kv.second.as_string()}});
    const Json& terms =
        spec.get("affinity").get("nodeAffinity").get("requiredDuringSchedulingIgnoredDuringExecution").get("nodeSelectorTerms");
    if (terms.size() > 1) return {"planner: more than one nodeSelectorTerm (ORed terms) is not supported"};
    for (const auto& term : terms.elems()) {
        if (term.get("matchFields").size() > 0) return {"planner: nodeSelectorTerm matchFields is not supported"};
        for (const auto& e : term.get("matchExpressions").elems()) {
            const std::string key = e.get("key").as_string(), op = e.get("operator").as_string();
            std::vector<std::string> vals;
            for (const auto& v : e.get("values").elems()) vals.push_back(v.as_string());
            std::sort(vals.begin(), vals.end());
            vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
            if (op == "In") c.req.push_back({key, "In", vals});
            else if (op == "NotIn") c.forbid.push_back({key, "In", vals});
            else if (op == "Exists") c.req.push_back({key, "Exists", {}});
            else if (op == "DoesNotExist") c.forbid.push_back({key, "Exists", {}});
            else if ((op == "Gt" || op == "Lt") && vals.size() == 1) c.req.push_back({key, op, vals});
            else return {"planner: node selector operator " + op + " is not supported"};
        }
    }
    c.tolerations = spec.get("tolerations").is_array() ? spec.get("tolerations") : Json::array();
    for (const auto& r : res_) c.res.push_back(pod_request(spec, r));
    // register the predicates (sorted dictionary; a new one changes the columns)
    std::set<LabelPred> all(preds_.begin(), preds_.end());
    const size_t before = all.size();
    for (const auto& p : c.req) all.insert(p);
    for (const auto& p : c.forbid) all.insert(p);
    if (all.size() != before) {
        preds_.assign(all.begin(), all.end());
        preds_dirty_ = true;
    }
    *out = std::move(c);
    return {};
}

Err2 Planner::encode(const std::vector<ClassSpec>& classes, std::vector<jsp_job_class>* out) const {
    std::vector<jsp_job_class>& jc = *out;
    jc.assign(std::max<size_t>(classes.size(), 1), jsp_job_class{});
    for (size_t i = 0; i < classes.size(); ++i) {
        const ClassSpec& c = classes[i];
        jsp_job_class& x = jc[i];
        std::memset(&x, 0, sizeof x);
        for (const auto& p : c.req) {
            const int b = pred_bit(p);
            if (b < 0) return {"planner: unregistered predicate"};
            x.req_labels[b >> 6] |= 1ull << (b & 63);
        }
        for (const auto& p : c.forbid) {
            const int b = pred_bit(p);
            if (b < 0) return {"planner: unregistered predicate"};
            x.forbid_labels[b >> 6] |= 1ull << (b & 63);
        }
        for (size_t t = 0; t < taints_.size(); ++t)
            for (const auto& tol : c.tolerations.elems())
                if (tolerates(tol, taints_[t])) { x.tolerated_taints |= 1u << t; break; }
        x.level = (uint32_t)c.level;
        x.pods = c.pods;
        for (size_t r = 0; r < res_.size(); ++r) x.req_res[r] = (uint32_t)std::min<uint64_t>(c.res[r], 0xFFFFFFFFull);
    }
    return {};
}

Err2 Planner::in_step() const {
    if (!synced_ || preds_dirty_) return {"planner: snapshot out of date (sync after registering templates)"};
    return {};
}

Err2 Planner::upload_classes(const std::vector<ClassSpec>& classes, std::vector<jsp_job_class>* jc) {
    if (Err2 e = encode(classes, jc); !e.ok()) return e;
    if (jsp_classes_upload(eng_, jc->data(), (uint32_t)classes.size()) != JSP_OK) return engine_error();
    return {};
}

Err2 Planner::begin(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_len,
                    std::vector<jsp_job_class>* jc, uint64_t* jobs, const char* arg_error) {
    if (eng_ == nullptr) return {"planner: no engine bound"};
    if (Err2 e = in_step(); !e.ok()) return e;
    if (arg_error) return {arg_error};
    if (Err2 e = upload_classes(classes, jc); !e.ok()) return e;
    *jobs = 0;
    for (uint32_t n : run_len) *jobs += n;
    return {};
}

Err2 Planner::place(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                    const std::vector<uint32_t>& run_len, std::vector<int32_t>* assign, jsp_stats* st) {
    std::vector<jsp_job_class> jc;
    uint64_t J = 0;
    if (Err2 e = begin(classes, run_len, &jc, &J); !e.ok()) return e;
    assign->assign(std::max<uint64_t>(J, 1), -1);
    if (jsp_place(eng_, run_class.data(), run_len.data(), (uint32_t)run_class.size(), assign->data(), nullptr, nullptr,
                  st) != JSP_OK)
        return engine_error();
    assign->resize(J);
    return {};
}

Err2 Planner::place_sticky(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                           const std::vector<uint32_t>& run_len, const std::vector<int32_t>& prev,
                           std::vector<int32_t>* assign, jsp_sticky_stats* st) {
    std::vector<jsp_job_class> jc;
    uint64_t J = 0;
    if (Err2 e = begin(classes, run_len, &jc, &J); !e.ok()) return e;
    if (prev.size() != J) return {"planner: one previous domain per job is needed"};
    assign->assign(std::max<uint64_t>(J, 1), -1);
    if (jsp_place_sticky(eng_, run_class.data(), run_len.data(), (uint32_t)run_class.size(), prev.data(), assign->data(),
                         st) != JSP_OK)
        return engine_error();
    assign->resize(J);
    return {};
}

Err2 Planner::place_gangs(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                          const std::vector<uint32_t>& run_len, const std::vector<uint32_t>& gang_runs,
                          const std::vector<uint32_t>& gang_span, std::vector<int32_t>* assign,
                          std::vector<int32_t>* span_domain, jsp_gang_stats* st) {
    std::vector<jsp_job_class> jc;
    uint64_t J = 0;
    if (Err2 e = begin(classes, run_len, &jc, &J,
                       gang_runs.size() != gang_span.size() ? "planner: one span per gang is needed" : nullptr);
        !e.ok())
        return e;
    assign->assign(std::max<uint64_t>(std::min<uint64_t>(J, JSP_GANG_MAX_JOBS), 1), -1);
    span_domain->assign(std::max<size_t>(gang_runs.size(), 1), -1);
    if (jsp_place_gangs(eng_, run_class.data(), run_len.data(), (uint32_t)run_class.size(), gang_runs.data(),
                        gang_span.data(), (uint32_t)gang_runs.size(), 0, assign->data(), span_domain->data(), st) != JSP_OK)
        return engine_error();
    assign->resize(J);
    span_domain->resize(gang_runs.size());
    return {};
}

Err2 Planner::place_fit(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                        const std::vector<uint32_t>& run_len, uint32_t policy, std::vector<int32_t>* assign,
                        jsp_fit_stats* st) {
    std::vector<jsp_job_class> jc;
    uint64_t J = 0;
    if (Err2 e = begin(classes, run_len, &jc, &J); !e.ok()) return e;
    assign->assign(std::max<uint64_t>(std::min<uint64_t>(J, JSP_FIT_MAX_JOBS), 1), -1);
    if (jsp_place_fit(eng_, run_class.data(), run_len.data(), (uint32_t)run_class.size(), policy, 0, assign->data(), st) !=
        JSP_OK)
        return engine_error();
    assign->resize(J);
    return {};
}

// One scenario of free_res / excl_owner edits (jsp_place_whatif, S = 1; no
// rows: jsp_place's answer). Nothing in the engine is written.
Err2 Planner::place_whatif(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                           const std::vector<uint32_t>& run_len, const std::vector<uint32_t>& rows,
                           const std::vector<uint32_t>& free_res, const std::vector<int32_t>& excl,
                           std::vector<int32_t>* assign, jsp_whatif_stats* st) {
    std::vector<jsp_job_class> jc;
    uint64_t J = 0;
    if (Err2 e = begin(classes, run_len, &jc, &J,
                       excl.size() != rows.size() || free_res.size() != res_.size() * rows.size()
                           ? "planner: one free_res column per resource and one owner per row are needed"
                           : nullptr);
        !e.ok())
        return e;
    const uint32_t so[2] = {0, (uint32_t)rows.size()};
    assign->assign(std::max<uint64_t>(std::min<uint64_t>(J, JSP_WHATIF_MAX_JOBS), 1), -1);
    if (jsp_place_whatif(eng_, run_class.data(), run_len.data(), (uint32_t)run_class.size(), so, 1, rows.data(), nullptr,
                         nullptr, rows.empty() ? nullptr : free_res.data(), rows.empty() ? nullptr : excl.data(), 0,
                         assign->data(), nullptr, st) != JSP_OK)
        return engine_error();
    assign->resize(J);
    return {};
}

// planner.preempt's engine call. The victim table comes from the cache: the
// exclusive jobs sync gave dense ids (occupy's job_ids, the ids in the
// excl_owner column) whose bound, non-terminal pods all have a priority below
// the request's. Ledger entries are in no table: they block.
Err2 Planner::place_preempt(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                            const std::vector<uint32_t>& run_len, int32_t priority,
                            const std::map<std::string, Json>& nodes, const std::map<std::string, Json>& pods,
                            std::vector<int32_t>* assign, std::vector<uint32_t>* victim_off,
                            std::vector<std::string>* victims, jsp_preempt_stats* st) {
    std::vector<jsp_job_class> jc;
    uint64_t J = 0;
    if (Err2 e = begin(classes, run_len, &jc, &J); !e.ok()) return e;
    std::vector<uint32_t> fr;
    std::vector<int32_t> ex;
    std::map<std::string, int32_t> job_ids;
    if (Err2 e = cache_columns(nodes, pods, nullptr, &fr, &ex, &job_ids, nullptr); !e.ok()) return e;
    // every exclusive job's highest pod priority, over the pods occupy counts
    std::map<std::string, int64_t> top;
    for (const auto& kv : pods) {
        const Json& pod = kv.second;
        if (!has_key(labels_of(pod), kJobKey)) continue;
        const std::string jk = labels_of(pod).get(kJobKey).as_string();
        if (!job_ids.count(jk)) continue;
        const std::string phase = pod.get("status").get("phase").as_string();
        if (pod.get("spec").get("nodeName").as_string().empty() || phase == "Succeeded" || phase == "Failed") continue;
        const Json& pr = pod.get("spec").get("priority");
        const int64_t v = pr.is_number() ? pr.as_int() : 0;
        const auto it = top.find(jk);
        if (it == top.end()) top[jk] = v;
        else it->second = std::max(it->second, v);
    }
    std::set<std::string> cand;
    std::set<int64_t> distinct;
    for (const auto& kv : top)
        if (kv.second < (int64_t)priority) {
            cand.insert(kv.first);
            distinct.insert(kv.second);
        }
    if (distinct.size() > JSP_PREEMPT_MAX_PRIO)
        return {"planner: " + std::to_string(distinct.size()) + " distinct victim priorities exceed the engine's " +
                std::to_string(JSP_PREEMPT_MAX_PRIO)};
    const std::vector<int64_t> ranks(distinct.begin(), distinct.end());
    std::vector<int32_t> ids;
    std::vector<uint32_t> rk;
    std::map<int32_t, std::string> key_of;
    for (const auto& k : cand) {
        const int32_t id = job_ids[k];
        ids.push_back(id);
        rk.push_back((uint32_t)(std::lower_bound(ranks.begin(), ranks.end(), top[k]) - ranks.begin()));
        key_of[id] = k;
    }
    // the free column without the candidates' pods, dense
    std::vector<uint32_t> evict_free;
    if (!cand.empty())
        if (Err2 e = cache_columns(nodes, pods, &cand, &evict_free, &ex, nullptr, nullptr); !e.ok()) return e;
    const uint32_t N = (uint32_t)row_node_.size();
    const uint64_t Jb = std::max<uint64_t>(std::min<uint64_t>(J, JSP_PREEMPT_MAX_JOBS), 1);
    assign->assign(Jb, -1);
    victim_off->assign(Jb + 1, 0);
    std::vector<int32_t> vic(std::max<uint32_t>(N, 1), -1);
    if (jsp_place_preempt(eng_, run_class.data(), run_len.data(), (uint32_t)run_class.size(), (uint32_t)ranks.size(),
                          ids.data(), rk.data(), (uint32_t)ids.size(), cand.empty() ? nullptr : evict_free.data(), 0,
                          assign->data(), victim_off->data(), vic.data(), N, st) != JSP_OK)
        return engine_error();
    assign->resize(J);
    victim_off->resize(J + 1);
    victims->clear();
    for (uint32_t i = 0; i < (*victim_off)[J]; ++i) victims->push_back(key_of[vic[i]]);
    return {};
}

// planner.planSpread's engine call. The peers' owner ids come from the cache
// the way planner.preempt's victims do: an exclusive job the pods show has the
// dense id sync gave it (occupy's job_ids), one that only the ledger holds has
// its ledger owner.
Err2 Planner::place_spread(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                           const std::vector<uint32_t>& run_len, int level, uint32_t max_skew,
                           const std::vector<std::string>* peer_keys, const std::set<std::string>& jobsets,
                           const std::set<std::string>& own, const std::map<std::string, Json>& nodes,
                           const std::map<std::string, Json>& pods, std::vector<int32_t>* assign,
                           std::vector<int32_t>* spread, std::vector<uint32_t>* count,
                           std::vector<std::string>* peers_out, std::string* unknown, jsp_spread_stats* st) {
    std::vector<jsp_job_class> jc;
    uint64_t J = 0;
    if (Err2 e = begin(classes, run_len, &jc, &J); !e.ok()) return e;
    if (level < 0 || (size_t)level >= level_keys_.size()) return {"planner: the spread level is no engine level"};
    std::vector<uint32_t> fr;
    std::vector<int32_t> ex;
    std::map<std::string, int32_t> job_ids;
    if (Err2 e = cache_columns(nodes, pods, nullptr, &fr, &ex, &job_ids, nullptr); !e.ok()) return e;
    const auto owner_of = [&](const std::string& k, int32_t* id) {
        const auto a = job_ids.find(k);
        if (a != job_ids.end()) {
            *id = a->second;
            return true;
        }
        const auto b = ledger_.find(k);
        if (b == ledger_.end()) return false;
        *id = b->second.owner;
        return true;
    };
    std::set<std::string> keys;
    unknown->clear();
    if (peer_keys) {
        int32_t id;
        for (const auto& k : *peer_keys) {
            if (!owner_of(k, &id)) {
                *unknown = k;
                return {};
            }
            keys.insert(k);
        }
    } else {
        for (const auto& kv : pods) {
            const Json& l = labels_of(kv.second);
            if (!has_key(l, kJobKey) || !has_key(l, kJobSetNameKey)) continue;
            const std::string jk = l.get(kJobKey).as_string();
            if (!job_ids.count(jk) || own.count(jk)) continue;
            if (jobsets.count(kv.second.get("metadata").get("namespace").as_string() + "/" +
                              l.get(kJobSetNameKey).as_string()))
                keys.insert(jk);
        }
        for (const auto& kv : ledger_)
            if (!kv.second.jobset.empty() && jobsets.count(kv.second.jobset) && !own.count(kv.first)) keys.insert(kv.first);
    }
    std::vector<int32_t> ids;
    std::set<int32_t> once;
    for (const auto& k : keys) {
        int32_t id = -1;
        owner_of(k, &id);
        if (once.insert(id).second) ids.push_back(id);
    }
    peers_out->assign(keys.begin(), keys.end());
    const uint64_t Jb = std::max<uint64_t>(std::min<uint64_t>(J, JSP_SPREAD_MAX_JOBS), 1);
    assign->assign(Jb, -1);
    spread->assign(Jb, -1);
    count->assign(std::max<size_t>(domain_values_[level].size(), 1), 0);
    if (jsp_place_spread(eng_, run_class.data(), run_len.data(), (uint32_t)run_class.size(), (uint32_t)level, max_skew,
                         ids.data(), (uint32_t)ids.size(), 0, assign->data(), spread->data(), count->data(), st) != JSP_OK)
        return engine_error();
    assign->resize(J);
    spread->resize(J);
    count->resize(domain_values_[level].size());
    return {};
}

Err2 Planner::bind(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                   const std::vector<uint32_t>& run_len, const std::vector<int32_t>& assign,
                   std::vector<int32_t>* pod_row, std::vector<uint64_t>* pod_off, jsp_bind_stats* st) {
    std::vector<jsp_job_class> jc;
    uint64_t J = 0, P = 0;
    if (Err2 e = begin(classes, run_len, &jc, &J); !e.ok()) return e;
    for (size_t i = 0; i < run_len.size(); ++i) {
        if (run_class[i] >= classes.size()) return {"planner: a run's class is out of range"};
        P += (uint64_t)run_len[i] * jc[run_class[i]].pods;
    }
    if (assign.size() != J) return {"planner: one domain per job is needed"};
    if (P > JSP_BIND_MAX_PODS) return {"planner: more pods than one bind call takes"};
    pod_row->assign(std::max<uint64_t>(P, 1), -1);
    pod_off->assign(J + 1, 0);
    if (jsp_bind_pods(eng_, run_class.data(), run_len.data(), (uint32_t)run_class.size(), assign.data(), 0,
                      pod_row->data(), pod_off->data(), st) != JSP_OK)
        return engine_error();
    pod_row->resize(P);
    return {};
}

Err2 Planner::assume(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                     const std::vector<uint32_t>& run_len, const std::vector<int32_t>& assign,
                     const std::vector<std::string>& job_keys, const std::vector<std::string>& names,
                     std::vector<uint8_t>* committed, std::vector<int32_t>* owner, jsp_assume_stats* st,
                     const std::vector<std::string>* jobsets) {
    if (Err2 e = in_step(); !e.ok()) return e;  // no engine is needed: the ledger alone then
    uint64_t J = 0;
    std::vector<int> level;
    for (size_t i = 0; i < run_len.size(); ++i) {
        if (i >= run_class.size() || run_class[i] >= classes.size()) return {"planner: a run's class is out of range"};
        J += run_len[i];
        level.insert(level.end(), run_len[i], classes[run_class[i]].level);
    }
    if (assign.size() != J || job_keys.size() != J || names.size() != J)
        return {"planner: one domain, job key and name per job are needed"};
    // owner ids: a job the ledger already holds keeps its id
    owner->assign(J, -1);
    int32_t next = next_owner_;
    for (uint64_t j = 0; j < J; ++j) {
        if (assign[j] < 0) continue;
        if (level[j] < 0 || (size_t)assign[j] >= domain_values_[level[j]].size())
            return {"planner: job " + std::to_string(j) + ": domain out of range"};
        auto it = ledger_.find(job_keys[j]);
        if (it != ledger_.end()) {
            (*owner)[j] = it->second.owner;
        } else {
            (*owner)[j] = next;
            next = next == 0x7FFFFFFF ? 0x40000000 : next + 1;
        }
    }
    committed->assign(std::max<uint64_t>(J, 1), 0);
    jsp_assume_stats s{};
    if (eng_ != nullptr) {
        std::vector<jsp_job_class> jc;
        if (Err2 e = upload_classes(classes, &jc); !e.ok()) return e;
        if (jsp_assume(eng_, run_class.data(), run_len.data(), (uint32_t)run_class.size(), assign.data(), owner->data(),
                       0, committed->data(), &s) != JSP_OK)
            return engine_error();
    } else {
        s.jobs = (uint32_t)J;
        for (uint64_t j = 0; j < J; ++j) {
            if (assign[j] < 0) continue;
            uint32_t r0, r1;
            domain_rows(level[j], assign[j], &r0, &r1);
            bool free_rows = r1 > r0;
            for (uint32_t i = r0; i < r1 && free_rows; ++i) free_rows = excl_[i] == -1;
            for (uint64_t q = 0; q < j && free_rows; ++q) {  // an earlier job of this call on intersecting rows
                if (assign[q] < 0 || !(*committed)[q]) continue;
                uint32_t q0, q1;
                domain_rows(level[q], assign[q], &q0, &q1);
                free_rows = q1 <= r0 || r1 <= q0;
            }
            (*committed)[j] = free_rows ? 1 : 0;
            s.committed += free_rows ? 1u : 0u;
            s.stale += free_rows ? 0u : 1u;
            s.rows_marked += free_rows ? r1 - r0 : 0u;
        }
    }
    next_owner_ = next;
    // the host columns follow the engine's, and the ledger keeps the hold
    for (uint64_t j = 0; j < J; ++j) {
        if (assign[j] < 0 || !(*committed)[j]) continue;
        uint32_t r0, r1;
        domain_rows(level[j], assign[j], &r0, &r1);
        for (uint32_t i = r0; i < r1; ++i) excl_[i] = (*owner)[j];
        ledger_[job_keys[j]] = Assumed{names[j], (*owner)[j], level[j], domain_values_[level[j]][assign[j]],
                                       jobsets && j < jobsets->size() ? (*jobsets)[j] : std::string()};
    }
    committed->resize(J);
    if (st) *st = s;
    return {};
}

Err2 Planner::forget(const std::vector<std::string>& names, uint64_t* rows_cleared,
                     std::vector<std::string>* forgotten) {
    const std::set<std::string> want(names.begin(), names.end());
    std::vector<int32_t> owners;
    for (auto it = ledger_.begin(); it != ledger_.end();) {
        if (!want.count(it->second.name)) {
            ++it;
            continue;
        }
        owners.push_back(it->second.owner);
        if (forgotten) forgotten->push_back(it->second.name);
        it = ledger_.erase(it);
    }
    std::sort(owners.begin(), owners.end());
    uint64_t cleared = 0;
    if (!owners.empty())
        for (int32_t& x : excl_)
            if (x != -1 && std::binary_search(owners.begin(), owners.end(), x)) {
                x = -1;
                ++cleared;
            }
    if (eng_ != nullptr && synced_) {
        // the engine's own count is reported (an engine that is not in step
        // gets the cleared column with the next full upload instead)
        cleared = 0;
        // jsp_forget wants an engine that is ready as for jsp_assume, classes included, though it reads
        // none: after a full upload it gets an empty class set (every placing call uploads its own first)
        if (classes_gone_ && !owners.empty()) {
            if (jsp_classes_upload(eng_, nullptr, 0) != JSP_OK) {
                synced_ = false;
                return engine_error();
            }
            classes_gone_ = false;
        }
        for (size_t i = 0; i < owners.size(); i += JSP_FORGET_MAX_OWNERS) {
            const uint32_t n = (uint32_t)std::min<size_t>(owners.size() - i, JSP_FORGET_MAX_OWNERS);
            uint64_t c = 0;
            if (jsp_forget(eng_, owners.data() + i, n, &c) != JSP_OK) {
                synced_ = false;  // the host column is ahead of the engine's: a full upload repairs it
                return engine_error();
            }
            cleared += c;
        }
    }
    if (rows_cleared) *rows_cleared = cleared;
    return {};
}

Err2 Planner::explain(const std::vector<ClassSpec>& classes, std::vector<jsp_class_explain>* out) {
    std::vector<jsp_job_class> jc;
    uint64_t J = 0;  // no runs: the classes alone are explained
    if (Err2 e = begin(classes, {}, &jc, &J); !e.ok()) return e;
    out->assign(std::max<size_t>(classes.size(), 1), jsp_class_explain{});
    if (jsp_explain(eng_, out->data(), (uint32_t)classes.size()) != JSP_OK)
        return engine_error();
    out->resize(classes.size());
    return {};
}

Json explain_counts(const jsp_class_explain& x, size_t n_res) {
    Json c = Json::object(), ins = Json::array();
    for (size_t r = 0; r < n_res && r < JSP_MAX_RES; ++r) ins.push_back((int64_t)x.rows_insufficient[r]);
    c["rows"] = (int64_t)x.rows;
    c["rowsSelector"] = (int64_t)x.rows_selector;
    c["rowsTaint"] = (int64_t)x.rows_taint;
    c["rowsNoCapacity"] = (int64_t)x.rows_no_capacity;
    c["rowsInsufficient"] = ins;
    c["rowsFit"] = (int64_t)x.rows_fit;
    c["rowsOccupied"] = (int64_t)x.rows_occupied;
    c["domains"] = (int64_t)x.domains;
    c["domOccupied"] = (int64_t)x.dom_occupied;
    c["domShort"] = (int64_t)x.dom_short;
    c["domFeasible"] = (int64_t)x.dom_feasible;
    c["bestShortCap"] = (int64_t)x.best_short_cap;
    c["bestShortDomain"] = (int64_t)x.best_short_domain;
    return c;
}

namespace {
// "head: a, b" -- or just "head" when every clause was omitted
std::string join_group(const std::string& head, const std::vector<std::string>& clauses) {
    std::string s = head;
    for (size_t i = 0; i < clauses.size(); ++i) s += (i == 0 ? ": " : ", ") + clauses[i];
    return s + ".";
}
}  // namespace

std::string explain_message(const Json& counts, const std::string& topology_key, int64_t pods,
                            const std::vector<std::string>& resources, const std::string& best_value) {
    auto n = [&](const char* k) { return counts.get(k).as_int(); };
    auto num = [](int64_t v) { return std::to_string(v); };
    std::vector<std::string> dom, row;
    if (n("domOccupied") > 0) dom.push_back(num(n("domOccupied")) + " held by another exclusive job");
    if (n("domShort") > 0) {
        std::string c = num(n("domShort")) + " too small";
        if (!best_value.empty()) c += " (largest, " + best_value + ", fits " + num(n("bestShortCap")) + " pods)";
        dom.push_back(c);
    }
    if (n("rowsSelector") > 0) row.push_back(num(n("rowsSelector")) + " didn't match the node selector");
    if (n("rowsTaint") > 0) row.push_back(num(n("rowsTaint")) + " had untolerated taints");
    if (n("rowsNoCapacity") > 0) {
        std::string c = num(n("rowsNoCapacity")) + " lacked resources", in;
        const Json& ins = counts.get("rowsInsufficient");
        for (size_t r = 0; r < ins.size() && r < resources.size(); ++r) {
            if (ins.at(r).as_int() <= 0) continue;
            in += (in.empty() ? "" : ", ") + ("Insufficient " + resources[r] + ": " + num(ins.at(r).as_int()));
        }
        if (!in.empty()) c += " (" + in + ")";
        row.push_back(c);
    }
    if (n("rowsFit") > 0) row.push_back(num(n("rowsFit")) + " fit at least one pod");
    return join_group(num(n("domFeasible")) + "/" + num(n("domains")) + " " + topology_key + " domains can hold a job of " +
                          num(pods) + " pods",
                      dom) +
           " " + join_group(num(n("rows")) + " nodes", row);
}

Json Planner::columns() const {
    Json c = Json::object();
    Json rows = Json::array();
    for (const auto& n : row_node_) rows.push_back(n);
    c["rows"] = rows;
    const size_t N = row_node_.size();
    Json lab = Json::array(), tb = Json::array(), fr = Json::array(), ex = Json::array();
    for (size_t i = 0; i < N; ++i) {
        Json words = Json::array();
        for (uint32_t w = 0; w < W_; ++w) {
            char buf[24];
            std::snprintf(buf, sizeof buf, "%016llx", (unsigned long long)labels_[(size_t)w * N + i]);
            words.push_back(std::string(buf));
        }
        lab.push_back(words);
        tb.push_back((int64_t)taint_bits_[i]);
        Json f = Json::array();
        for (size_t r = 0; r < res_.size(); ++r) f.push_back((int64_t)free_[r * N + i]);
        fr.push_back(f);
        ex.push_back((int64_t)excl_[i]);
    }
    c["labels"] = lab;
    c["taints"] = tb;
    c["free"] = fr;
    c["excl"] = ex;
    Json ls = Json::array();
    for (uint32_t v : leaf_start_) ls.push_back((int64_t)v);
    c["leafStart"] = ls;
    Json fl = Json::array();
    for (const auto& lv : first_leaf_) {
        Json a = Json::array();
        for (uint32_t v : lv) a.push_back((int64_t)v);
        fl.push_back(a);
    }
    c["firstLeaf"] = fl;
    Json dv = Json::array();
    for (const auto& lv : domain_values_) {
        Json a = Json::array();
        for (const auto& v : lv) a.push_back(v);
        dv.push_back(a);
    }
    c["domainValues"] = dv;
    Json pr = Json::array();
    for (const auto& p : preds_) {
        Json x = Json::object();
        x["key"] = p.key;
        x["op"] = p.op;
        Json vs = Json::array();
        for (const auto& v : p.values) vs.push_back(v);
        x["values"] = vs;
        pr.push_back(x);
    }
    c["predicates"] = pr;
    Json ts = Json::array();
    for (const auto& t : taints_) {
        Json x = Json::object();
        x["key"] = t.key;
        x["value"] = t.value;
        x["effect"] = t.effect;
        ts.push_back(x);
    }
    c["taintKeys"] = ts;
    return c;
}

Json label_nodes(const Planner& pl, int level, const std::vector<std::string>& namespaced_jobs,
                 const std::vector<int32_t>& assign) {
    Json out = Json::array();
    for (size_t j = 0; j < assign.size() && j < namespaced_jobs.size(); ++j) {
        if (assign[j] < 0) continue;
        uint32_t a = 0, b = 0;
        pl.domain_rows(level, assign[j], &a, &b);
        for (uint32_t r = a; r < b; ++r) {
            Json body = Json::object();
            body["metadata"]["labels"][kNamespacedJobKey] = namespaced_jobs[j];
            Json taint = Json::object();
            taint["key"] = kNoScheduleTaintKey;
            taint["value"] = "true";
            taint["effect"] = "NoSchedule";
            body["spec"]["taints"] = Json::array();
            body["spec"]["taints"].push_back(taint);
            Json patch = Json::object();
            patch["node"] = pl.row_node(r);
            patch["body"] = body;
            out.push_back(patch);
        }
    }
    return out;
}

}  // namespace jsk
