// placement.h — the host side of the engine boundary that the reference's
// controller would own: the Go
// `pkg/placement` package restated in C++ over Kubernetes objects as JSON.
//
//   Planner::sync     informer-cache Nodes and bound Pods -> the engine's SoA
//                     snapshot (deterministic sorted dictionaries), uploaded
//                     whole when its structure changed, else as a row patch
//                     (jsp_snapshot_patch) of the rows whose columns changed
//   Planner::plan     a JobSet's child Jobs (replicated-job runs in
//                     globalJobIndex order, one requirement class per pod
//                     template) -> jsp_place -> a domain per job; with the
//                     jobs' previous domains, jsp_place_sticky
//   Planner::place_gangs  the same runs cut into JobSets, each whole inside
//                     one domain of its span level or not at all,
//                     jsp_place_gangs
//   Planner::place_fit    the same runs, every job on the tightest or the
//                     roomiest free feasible domain, jsp_place_fit
//   Planner::place_whatif the same runs under one scenario of hypothetical
//                     row edits, nothing written, jsp_place_whatif
//   Planner::place_preempt the same runs at a priority: exclusive jobs whose
//                     pods all have a lower one may be evicted,
//                     jsp_place_preempt -> a domain and the victims per job
//   Planner::place_spread the same runs spread evenly over the domains of one
//                     level (maxSkew; the JobSets' running jobs count as
//                     peers), jsp_place_spread -> a domain and the level's
//                     domain per job, and the jobs per domain of the level
//   Planner::bind     a plan's domains -> jsp_bind_pods -> a node row per pod
//                     (completion index) of every job whose domain still fits
//   Planner::assume   a plan's domains -> jsp_assume: held in the snapshot (and
//                     in a ledger that outlives syncs and full uploads) until
//                     the informer shows the jobs' pods or Planner::forget
//   label_nodes       the node-selector strategy's node patches from a plan
//                     (deterministic replacement for hack/label_nodes/
//                     label_nodes.py:36-120)
#pragma once
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../../include/jsplace.h"
#include "json.h"

namespace jsk {

// One node-label predicate of the dictionary: a node's bit is set when the
// predicate holds on its labels. Selector terms map onto them:
//   nodeSelector {k: v} / In [v..]  -> required  (k In {v..})
//   NotIn [v..]                       -> forbidden (k In {v..})
//   Exists / DoesNotExist             -> required / forbidden (k Exists)
//   Gt / Lt v                         -> required  (k Gt v) / (k Lt v)
struct LabelPred {
    std::string key;
    std::string op;                  // "In", "Exists", "Gt", "Lt"
    std::vector<std::string> values; // sorted (In), one value (Gt/Lt)
    bool operator<(const LabelPred& o) const;
    bool operator==(const LabelPred& o) const;
    bool holds(const Json& labels) const;
};

// A NoSchedule / NoExecute taint of the dictionary (PreferNoSchedule is a
// preference, not a predicate).
struct TaintKey {
    std::string key, value, effect;
    bool operator<(const TaintKey& o) const;
    bool operator==(const TaintKey& o) const;
};

// One pod template's requirements, as the engine sees them.
struct ClassSpec {
    std::vector<LabelPred> req, forbid;
    Json tolerations;                 // the template's tolerations (array)
    std::vector<uint64_t> res;        // per configured resource, in its unit
    uint32_t pods = 1;                // parallelism
    int level = -1;                   // index of the exclusive-topology key
};

struct Err2 {  // error text ("" = ok) and an error class for the JSON layer
    std::string msg;
    bool ok() const { return msg.empty(); }
};

// Kubernetes quantity ("500m", "1536000Mi", "2", "1.5Gi", "1e3") in the
// unit of a resource: cpu -> millicores, memory / ephemeral-storage -> MiB,
// anything else -> whole units. round_up: requests round up, allocatable down.
bool parse_quantity(const std::string& q, const std::string& resource, bool round_up, uint64_t* out);

// Effective pod request of one resource: max(sum over containers, max over
// init containers), in the resource's unit.
uint64_t pod_request(const Json& podSpec, const std::string& resource);

class Planner {
public:
    Planner(jsp_engine* e, std::vector<std::string> level_keys, std::vector<std::string> resources);

    // Rebuild the snapshot from the cache objects and bring the engine up to
    // date. Returns {"rows","leaves","domains","labelWords","taintBits",
    // "skippedNodes","upload": "full"|"patch"|"none","patchedRows",
    // "exclusiveJobs"}.
    Err2 sync(const std::map<std::string, Json>& nodes, const std::map<std::string, Json>& pods, Json* stats);

    // The requirement class of a pod template (job template spec.template);
    // registers its label predicates in the dictionary (a new predicate makes
    // the next sync a full upload). `topology_key` = the exclusive-topology key.
    Err2 class_of(const Json& podTemplateSpec, int64_t parallelism, const std::string& topology_key, ClassSpec* out);

    // The engine's form of classes (label/taint bits of the current dictionaries).
    Err2 encode(const std::vector<ClassSpec>& classes, std::vector<jsp_job_class>* out) const;

    // Place runs (class index, job count) in global order. Classes are
    // uploaded to the engine first. assign: domain id per job, -1 unplaceable.
    Err2 place(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
               const std::vector<uint32_t>& run_len, std::vector<int32_t>* assign, jsp_stats* st);

    // place with each job's previous domain id at its class's level (-1: no
    // hint): jsp_place_sticky -- a job whose previous domain is still feasible
    // and unclaimed by an earlier job keeps it, the others fill around them.
    Err2 place_sticky(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                      const std::vector<uint32_t>& run_len, const std::vector<int32_t>& prev,
                      std::vector<int32_t>* assign, jsp_sticky_stats* st);

    // place with the runs cut into gangs (jsp_place_gangs): gang g is the next
    // gang_runs[g] runs and lands whole inside one domain of level
    // gang_span[g] (JSP_SPAN_ANY: anywhere) or not at all. span_domain[g]: that
    // domain's id (0 for JSP_SPAN_ANY), -1 when the gang was refused.
    Err2 place_gangs(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                     const std::vector<uint32_t>& run_len, const std::vector<uint32_t>& gang_runs,
                     const std::vector<uint32_t>& gang_span, std::vector<int32_t>* assign,
                     std::vector<int32_t>* span_domain, jsp_gang_stats* st);

    // place with a choice among the feasible domains (jsp_place_fit): policy
    // JSP_FIT_LOWEST is place's answer, JSP_FIT_TIGHTEST / JSP_FIT_ROOMIEST
    // give every job the free feasible domain of the least / the most pod
    // capacity; st->slack is what the placed jobs leave unused.
    Err2 place_fit(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                   const std::vector<uint32_t>& run_len, uint32_t policy, std::vector<int32_t>* assign,
                   jsp_fit_stats* st);

    // place under one scenario of hypothetical row edits (jsp_place_whatif):
    // rows ascending, free_res [R][n] and excl [n] for them; nothing is
    // written. st->flips: the (class, domain) feasibility bits that differ.
    Err2 place_whatif(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                      const std::vector<uint32_t>& run_len, const std::vector<uint32_t>& rows,
                      const std::vector<uint32_t>& free_res, const std::vector<int32_t>& excl,
                      std::vector<int32_t>* assign, jsp_whatif_stats* st);
    // The rows (with their free_res [R][n] and excl [n]) that differ when the
    // pods and the ledger entries of the job keys `keys` are left out of the
    // columns sync builds from this cache. *unknown: a key nothing carries.
    Err2 evict_delta(const std::map<std::string, Json>& nodes, const std::map<std::string, Json>& pods,
                     const std::set<std::string>& keys, std::vector<uint32_t>* rows, std::vector<uint32_t>* free_res,
                     std::vector<int32_t>* excl, std::string* unknown) const;

    // place at `priority` (jsp_place_preempt; nothing is written). A candidate
    // victim is an exclusive job of this cache whose bound, non-terminal pods
    // all carry spec.priority below `priority` (absent: 0); the planner's own
    // ledger entries carry no priority, stay out of the table and so block.
    // Ranks are the candidates' distinct priorities in ascending order;
    // evict_free is the free column sync would build without the candidates'
    // pods. victims[victim_off[j] .. victim_off[j+1]): the job keys to evict for
    // job j, in row order.
    Err2 place_preempt(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                       const std::vector<uint32_t>& run_len, int32_t priority, const std::map<std::string, Json>& nodes,
                       const std::map<std::string, Json>& pods, std::vector<int32_t>* assign,
                       std::vector<uint32_t>* victim_off, std::vector<std::string>* victims, jsp_preempt_stats* st);

    // place spread evenly over the domains of `level` (jsp_place_spread):
    // max_skew >= 1 refuses a job that would put its domain more than that
    // ahead of the emptiest eligible one, JSP_SPREAD_SOFT never refuses. The
    // peers, the jobs that count as already placed, are `peer_keys` (job keys;
    // *unknown: one that holds no domain, and nothing is placed) or, when it
    // is null, the exclusive jobs of `jobsets` ("namespace/jobset-name") that
    // hold domains by the cache's pods or by the ledger, the keys in `own`
    // (the jobs being placed) left out. A key becomes the owner id its rows
    // carry: the dense id sync gave it, or its ledger entry's. peers_out: the
    // keys used, sorted; count[S]: the peers and the placed jobs per domain
    // of `level`.
    Err2 place_spread(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                      const std::vector<uint32_t>& run_len, int level, uint32_t max_skew,
                      const std::vector<std::string>* peer_keys, const std::set<std::string>& jobsets,
                      const std::set<std::string>& own, const std::map<std::string, Json>& nodes,
                      const std::map<std::string, Json>& pods, std::vector<int32_t>* assign,
                      std::vector<int32_t>* spread, std::vector<uint32_t>* count, std::vector<std::string>* peers_out,
                      std::string* unknown, jsp_spread_stats* st);

    // A node row for every pod of the jobs' domains (jsp_bind_pods): assign is
    // a domain id at each job's class level or -1; pod p of job j is
    // pod_row[pod_off[j] + p], a row of row_node() or -1 (unplaced, or the
    // domain no longer fits).
    Err2 bind(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
              const std::vector<uint32_t>& run_len, const std::vector<int32_t>& assign, std::vector<int32_t>* pod_row,
              std::vector<uint64_t>* pod_off, jsp_bind_stats* st);

    // Hold the jobs' domains (jsp_assume; DESIGN.md §2 "Assume and forget"):
    // every job with a domain gets an owner id (from 0x40000000 upward, never
    // an informer-derived id) and, when its domain is feasible now, its rows
    // are owned by it in the engine and in the host columns alike, so sync's
    // diff stays correct. The ledger (job key -> owner, level, domain value)
    // keeps the mark alive: rebuild lays every entry over the rebuilt column
    // where it holds -1, drops an entry whose job key the informer's pods now
    // cover (confirmed: sync patches the rows to the informer's id) and one
    // whose domain value is gone. committed[j] 1/0; owner[j] the id or -1
    // (unplaced). Without an engine (host-only planner) a job commits when its
    // domain has rows and none of them is owned: the ledger alone is exercised.
    // jobsets (nullable): per job "namespace/jobset-name", kept in the ledger
    // so that place_spread finds a JobSet's assumed jobs.
    Err2 assume(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_class,
                const std::vector<uint32_t>& run_len, const std::vector<int32_t>& assign,
                const std::vector<std::string>& job_keys, const std::vector<std::string>& names,
                std::vector<uint8_t>* committed, std::vector<int32_t>* owner, jsp_assume_stats* st,
                const std::vector<std::string>* jobsets = nullptr);
    // Drop the ledger entries of the named jobs and free their rows
    // (jsp_forget); names without an entry are ignored. forgotten: the names
    // that had one.
    Err2 forget(const std::vector<std::string>& names, uint64_t* rows_cleared, std::vector<std::string>* forgotten);
    size_t assumed() const { return ledger_.size(); }

    // Why jobs of these classes cannot be placed (jsp_explain): the classes
    // are uploaded as place does, out gets one record per class.
    Err2 explain(const std::vector<ClassSpec>& classes, std::vector<jsp_class_explain>* out);

    // snapshot lookups
    int level_of(const std::string& key) const;
    bool row_of(const std::string& node, int32_t* row) const;
    const std::vector<std::string>& domain_values(int level) const { return domain_values_[level]; }
    int32_t domain_id(int level, const std::string& value) const;
    // rows [first, end) of domain d at `level`
    void domain_rows(int level, int32_t d, uint32_t* first, uint32_t* end) const;
    // domain id at `level` of snapshot row `row` (host lookup, no engine call)
    int32_t row_domain(uint32_t row, int level) const;
    const std::string& row_node(uint32_t row) const { return row_node_[row]; }
    jsp_engine* engine() const { return eng_; }
    const std::vector<std::string>& level_keys() const { return level_keys_; }
    const std::vector<std::string>& resources() const { return res_; }
    bool synced() const { return synced_; }
    // A Node was added, modified or removed in the cache since the last sync:
    // the snapshot's row -> domain answers may be stale, so the webhook and
    // reconciler lookups take the reference's Node Get path until the next
    // sync (serving() false). Pod events do not change a row's domain.
    void note_node_event() { nodes_dirty_ = true; }
    bool serving() const { return synced_ && !nodes_dirty_; }
    // the host copy of the columns (tests compare a patched engine with a re-ingest)
    Json columns() const;

private:
    Err2 rebuild(const std::map<std::string, Json>& nodes, const std::map<std::string, Json>& pods);
    Err2 upload_full();
    void allocatable(const Json& node, uint32_t N, uint32_t i, std::vector<uint32_t>* fr) const;
    void occupy(const std::map<std::string, Json>& pods, const std::map<std::string, int32_t>& node_row,
                const std::vector<const Json*>& row_json, const std::vector<std::map<std::string, int32_t>>& did,
                const std::vector<uint32_t>& leaf_start, const std::vector<std::vector<uint32_t>>& fl,
                const std::set<std::string>* without, std::vector<uint32_t>* fr, std::vector<int32_t>* ex,
                std::map<std::string, int32_t>* job_ids_out, std::vector<std::string>* drop,
                std::set<std::string>* seen) const;
    // The free_res and excl_owner columns sync would build from this cache
    // (allocatable, then occupy with its `without` filter), for the synced rows.
    Err2 cache_columns(const std::map<std::string, Json>& nodes, const std::map<std::string, Json>& pods,
                       const std::set<std::string>* without, std::vector<uint32_t>* fr, std::vector<int32_t>* ex,
                       std::map<std::string, int32_t>* job_ids, std::set<std::string>* seen) const;
    int pred_bit(const LabelPred& p) const;
    // How every engine call starts, in this order: an engine is bound; in_step():
    // the snapshot is synced and holds every registered template's predicates;
    // arg_error, the caller's own argument check (null: none); upload_classes():
    // the classes encoded (*jc) and uploaded; *jobs = the sum of run_len.
    // assume, which needs no engine, takes the two steps on their own.
    Err2 begin(const std::vector<ClassSpec>& classes, const std::vector<uint32_t>& run_len,
               std::vector<jsp_job_class>* jc, uint64_t* jobs, const char* arg_error = nullptr);
    Err2 in_step() const;
    Err2 upload_classes(const std::vector<ClassSpec>& classes, std::vector<jsp_job_class>* jc);

    jsp_engine* eng_;
    std::vector<std::string> level_keys_, res_;
    std::vector<LabelPred> preds_;    // sorted dictionary
    bool preds_dirty_ = true;
    std::vector<TaintKey> taints_;    // sorted dictionary
    bool synced_ = false;
    bool nodes_dirty_ = false;
    // structure
    std::vector<std::string> row_node_;
    std::map<std::string, int32_t> node_row_;
    std::vector<std::vector<std::string>> domain_values_;
    std::vector<std::map<std::string, int32_t>> domain_ids_;
    std::vector<std::vector<uint32_t>> first_leaf_;  // per level, [D_k + 1]
    std::vector<uint32_t> leaf_start_;               // [L + 1]
    // columns
    uint32_t W_ = 1;
    std::vector<uint64_t> labels_;  // [W][N]
    std::vector<uint32_t> taint_bits_;
    std::vector<uint32_t> free_;    // [R][N]
    std::vector<int32_t> excl_;
    std::vector<std::string> skipped_;
    uint32_t exclusive_jobs_ = 0;
    // assumed domains: job key -> its hold (placement.h Planner::assume)
    struct Assumed {
        std::string name;    // the Job's name (planner.forget names jobs)
        int32_t owner;
        int level;
        std::string value;   // the domain's topology value: ids are renumbered by a re-upload
        std::string jobset;  // "namespace/jobset-name" of the Job, or empty (place_spread's peers)
    };
    std::map<std::string, Assumed> ledger_;
    int32_t next_owner_ = 0x40000000;
    bool classes_gone_ = true;  // no class upload since the last full upload (Planner::forget)
};

// One class's jsp_explain record as JSON: {"rows","rowsSelector","rowsTaint",
// "rowsNoCapacity","rowsInsufficient":[per configured resource],"rowsFit",
// "rowsOccupied","domains","domOccupied","domShort","domFeasible",
// "bestShortCap","bestShortDomain"}.
Json explain_counts(const jsp_class_explain& x, size_t n_res);

// The operator's line for one class's counts (DESIGN.md §6 fixes the format).
// best_value: the best short domain's topology value ("" = not known).
std::string explain_message(const Json& counts, const std::string& topology_key, int64_t pods,
                            const std::vector<std::string>& resources, const std::string& best_value);

// Node patches of the node-selector strategy for the jobs of a plan: every
// node of job j's domain gets the namespaced-job label and the no-schedule
// taint, as label_nodes.py's patch body (hack/label_nodes/label_nodes.py:65-80).
Json label_nodes(const Planner& pl, int level, const std::vector<std::string>& namespaced_jobs,
                 const std::vector<int32_t>& assign);

}  // namespace jsk
