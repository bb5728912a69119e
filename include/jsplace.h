/*
 * jsplace.h — C ABI of the MI355X exclusive-topology placement engine.
 *
 * This is the drop-in boundary for JobSet's exclusive-placement path
 * (SURVEY.md §8b). Every entry point takes plain pointers and sizes; no Go,
 * torch or HIP types cross it (device pointers and streams are passed as
 * void* / uintptr-sized handles). Return value: 0 on success, a negative
 * JSP_E* code on failure; the message is available from jsp_last_error()
 * (thread-local). Nothing aborts or throws across the ABI.
 *
 * Which reference interface each entry point replaces (file:line under the
 * reference tree, danielvegamyhre/jobset @ 2024-10-08):
 *
 *  jsp_engine_create / jsp_engine_create_multi / jsp_engine_destroy
 *      Constructed beside NewPodReconciler / NewPodWebhook in main.go:168,186
 *      and injected into them (there is no engine in the reference: the domain
 *      is chosen by kube-scheduler); the device-set form is
 *      the manager process's handle over several GPUs.
 *  jsp_topology_upload / jsp_snapshot_upload / jsp_snapshot_patch
 *      Replace the per-pod cached Node Get of topologyFromPod
 *      (pkg/webhooks/pod_mutating_webhook.go:173-194) and leaderPodTopology
 *      (pkg/controllers/pod_controller.go:242-263) with one resident snapshot
 *      of the node informer cache (RBAC nodes get/list/watch,
 *      config/components/rbac/role.yaml:16-23).
 *  jsp_place / jsp_place_device (= jsp_tally_device + jsp_assign_device)
 *      The placement decision that the leader's exclusive affinity terms
 *      (setExclusiveAffinities, pod_mutating_webhook.go:95-135) delegate to
 *      kube-scheduler, evaluated for every child Job of a JobSet at first
 *      admission and at full recreate (failurePolicyRecreateAll,
 *      pkg/controllers/failure_policy.go:155-175 -> reconcile,
 *      pkg/controllers/jobset_controller.go:172-176, 523-551).
 *      Job order = globalJobIndex (jobset_controller.go:1056-1065).
 *  jsp_resolve_leader_domains
 *      Batched form of setNodeSelector/topologyFromPod
 *      (pod_mutating_webhook.go:137-194): leader node row -> domain id at the
 *      job's topology level (the follower nodeSelector value).
 *  jsp_audit_placements
 *      Batched form of validatePodPlacements / leaderPodTopology /
 *      followerPodTopology (pod_controller.go:172-277).
 *
 * Threading: one engine is not re-entrant; calls on one engine are
 * serialised by an internal mutex (the Go wrapper also holds one).
 *
 * Stream ordering: uploads, patches, jsp_place and the webhook batches run on
 * the engine's own stream and return after it has finished; the *_device
 * entry points enqueue on the caller's stream and return at once -- except
 * where the walk runs on the host (ABI v7, jsp_stats.fused 7 and 8: the
 * multi-class / multi-level shapes the GPU level walker does not take, 256 to
 * 65536 jobs): there the call waits for its own kernels' answer (the stream's
 * earlier work first), walks, and returns with the assign[] copy enqueued on
 * the stream behind them (it waits for the walk's release, so no launch
 * separates the walk from the copy). Every call
 * is ordered after all work the engine enqueued earlier, on whatever stream
 * (the first call on a different stream waits on an event of the previous
 * one), so a patch after a jsp_place_device never races its tally.
 *
 * Kernel-side failures: every wait inside a launch is bounded -- the
 * single-class compaction's look-back, the pipelined batch walk's wait for an
 * earlier batch, the one-launch level walk's expanders' wait for the walker.
 * A wait that gives up writes the launch's tag to an error word and leaves
 * that launch's assign[] invalid. jsp_place reports it (JSP_EHIP) before it
 * returns; the device path reports it from jsp_engine_check (which waits for
 * the engine's work) or, once visible, from the next call on the engine. No
 * timeout returns JSP_OK with a stale assign[].
 *
 * Environment: JSP_SERVICE=0 (no resident service) / =parked, JSP_SERVICE_IDLE_MS
 * (its idle exit, default 50), JSP_RCCL_LIB (device sets) are the operational
 * switches; JSP_TEST_HOOKS is for tests only (jsp_engine.cc TestHooks). It
 * can shorten every bounded in-kernel wait to zero and force test-only shapes:
 * it must never be set in a production process.
 *
 * This header is the product boundary: every entry point in it is one the Go
 * binding calls (tests/test_abi.py checks the two agree).
 * The bench's and probes' entry points -- C-timed loops, dispatch-timed
 * kernels, the host-link floor, phase clocks, shape selection -- are a
 * separate symbol set, jspb_*, declared in jsplace_bench.h (ABI v7).
 */
#ifndef JSPLACE_H
#define JSPLACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JSP_ABI_VERSION 7

#define JSP_MAX_LEVELS 4      /* topology levels, 0 = coarsest (zone) .. K-1 = finest (rack) */
#define JSP_MAX_LABEL_WORDS 4 /* 256 interned (key,value) label bits */
#define JSP_MAX_RES 4         /* cpu-milli, memory-MiB, gpu, pods (any 4 the host chooses) */
#define JSP_MAX_CLASSES 64

/* error codes */
#define JSP_OK 0
#define JSP_EINVAL -1   /* bad argument / malformed snapshot */
#define JSP_EHIP -2     /* HIP runtime error (includes: no GPU) */
#define JSP_ENOMEM -3   /* device or host allocation failed */
#define JSP_ESTATE -4   /* call order: no topology / snapshot / classes yet */
#define JSP_ERANGE -5   /* problem exceeds an engine limit (message says which) */

typedef struct jsp_engine jsp_engine;

/* Global domain hierarchy; identical on every shard. Level K-1 domains are the
 * "leaves". Domain ids at each level are dense 0..D_k-1 and ordered so that
 * each domain covers a contiguous leaf range [first_leaf[k][d], first_leaf[k][d+1]).
 * Nesting is required: every level-k boundary is also a level-(k+1) boundary. */
typedef struct jsp_topology {
    uint32_t n_levels;                           /* K, 1..JSP_MAX_LEVELS */
    uint32_t n_domains[JSP_MAX_LEVELS];          /* D_k */
    const uint32_t* first_leaf[JSP_MAX_LEVELS];  /* [D_k+1]; entry K-1 ignored (identity) */
} jsp_topology;

/* Node rows held by this engine (one shard), sorted by leaf domain.
 * Column layout is SoA so every column streams coalesced from HBM. */
typedef struct jsp_nodes {
    uint32_t n_nodes;          /* N rows */
    uint32_t leaf_begin;       /* global id of the first leaf held here */
    uint32_t n_leaves;         /* leaves held here: [leaf_begin, leaf_begin+n_leaves) */
    const uint32_t* leaf_start;/* [n_leaves+1] row offsets (0 .. N) */
    uint32_t n_label_words;    /* W, 1..JSP_MAX_LABEL_WORDS */
    const uint64_t* labels;    /* [W][N] interned (key,value) label bits */
    const uint32_t* taints;    /* [N] interned NoSchedule/NoExecute taint bits */
    uint32_t n_res;            /* R, 1..JSP_MAX_RES */
    const uint32_t* free_res;  /* [R][N] allocatable minus requested */
    const int32_t* excl_owner; /* [N] id of the exclusive job whose domain covers the
                                  row (existing placements), -1 = none */
} jsp_nodes;

/* One requirement class: jobs are deduplicated into classes on the host.
 * A row passes the class's selector iff every bit of req_labels is set AND
 * every bit of forbid_labels is clear: two independent tests.
 *  - A bit in both req_labels and forbid_labels makes the class unsatisfiable:
 *    no row passes, every job of the class is answered -1 (a contradictory
 *    selector is an unschedulable job, as for kube-scheduler, not JSP_EINVAL).
 *  - Words at and past the snapshot's n_label_words are ignored, whatever
 *    they hold (an overlap there included).
 *  - Requests at and past the snapshot's n_res are ignored.
 *  - All 32 taint bits count: a row passes iff taints & ~tolerated_taints == 0.
 * A row counts as occupied (jsp_nodes.excl_owner) for any value other than
 * -1: 0, other negative values and INT32_MIN name an owner like any id. */
typedef struct jsp_job_class {
    uint64_t req_labels[JSP_MAX_LABEL_WORDS];    /* bits that must be set (nodeSelector) */
    uint64_t forbid_labels[JSP_MAX_LABEL_WORDS]; /* bits that must be clear (NotIn/DoesNotExist) */
    uint32_t tolerated_taints;                   /* taint bits this class tolerates */
    uint32_t level;                              /* topology level of its exclusive-topology key */
    uint32_t pods;                               /* pods per job (parallelism), >= 1 */
    uint32_t req_res[JSP_MAX_RES];               /* per-pod request per resource, 0 = none */
} jsp_job_class;

typedef struct jsp_stats {
    uint32_t jobs;             /* J */
    uint32_t placed;           /* assign[j] != -1 */
    uint32_t runs;             /* replicated-job runs the assignment walked */
    uint32_t fused;            /* launch shape: 0 tally->feas->assign, 1 fused tail, 2 one-class compaction,
                                  3 one-class compaction answered by the resident service,
                                  4 (unused since ABI v6: the fused resident kernel was retired),
                                  5 split service: resident tiles + the walk on the host,
                                  6 device set: shard tallies combined (RCCL / on-device add), then assign,
                                  7 (ABI v7) tally + feasibility on the GPU, the walk on the host: every
                                    shape the GPU level walker does not take (several levels, or more
                                    than 32 runs), up to 65536 jobs -- launch path and device paths
                                    (jspb_set_fused OFF keeps the GPU walkers: shape 0),
                                  8 (ABI v7) the split service's tiles launched for this one request, the
                                    walk on the host: the launch path and the device paths of every shape
                                    the split service takes, when no tallies are requested */
    double wall_us;            /* host wall time of the call */
} jsp_stats;

/* Engine metrics (ABI v7; SURVEY.md §5 "engine histograms"): what a
 * Prometheus exporter in the Go manager publishes beside the reference's
 * jobset_failed_total / jobset_completed_total counters
 * (pkg/metrics/metrics.go:24-38). Always on, per engine, cheap (a few adds
 * per call under a lock of their own).
 *
 * Consistency of a read (jsp_engine_get_metrics): after the calls have
 * returned, every total is exact. A placement answered under the lease
 *  records place_us, batch_jobs, placed, unplaceable and
 * svc_calls itself, while it holds the engine's lock, and a read never waits
 * for that lock: while such a call is in flight a read may hold that one call
 * in some of the five and not yet in the others (a read retries until it sees
 * whole calls only, and gives up on that after a writer was seen inside its
 * stores a thousand times running). A reset during such a call may leave that
 * call's value out of the next period's `max`. stats.wall_us of a jsp_place
 * call is the value place_us holds for it.
 *
 * A log2 histogram: bucket 0 counts values below lo, bucket i (1..30) values
 * in [lo * 2^(i-1), lo * 2^i), bucket 31 the rest. Counts are per bucket (not
 * cumulative: an exporter sums them up for its `le` boundaries lo * 2^i). */
#define JSP_HIST_BUCKETS 32
typedef struct jsp_hist {
    uint64_t count;
    double sum;
    double max;
    uint64_t bucket[JSP_HIST_BUCKETS];
} jsp_hist;

#define JSP_HIST_LO_US 0.5     /* lo of the latency histograms (us): bucket 30 ends at ~537 s */
#define JSP_HIST_LO_JOBS 1.0   /* lo of the batch-size histogram */

typedef struct jsp_metrics {
    jsp_hist place_us;         /* jsp_place / jsp_place_jobs: host wall per call, us (failed calls too) */
    jsp_hist patch_us;         /* jsp_snapshot_patch: host wall per call, us */
    jsp_hist batch_jobs;       /* jobs per successful jsp_place call */
    jsp_hist device_us;        /* device time per placement, us: the resident service's in-kernel request
                                  time, or a single-launch placement's kernel events. Recorded only while
                                  device timing is on (jsplace_bench.h jspb_set_timing): the stamps and
                                  events cost ~1 us per call */
    uint64_t placed;           /* jobs given a domain */
    uint64_t unplaceable;      /* jobs answered -1 */
    uint64_t place_errors;     /* jsp_place calls that returned an error */
    uint64_t patch_errors;     /* jsp_snapshot_patch calls that returned an error */
    uint64_t svc_calls;        /* placements the resident service answered (stats.fused 3 or 5), those
                                  included that the host expanded from the lines of the service's last
                                  answer because nothing had changed since (the lease) */
    uint64_t svc_starts;       /* resident service launches (first use, after uploads, idle exits, wakes) */
    uint64_t svc_fallbacks;    /* placements the service could not answer (answered on the launch path) */
} jsp_metrics;

/* jsp_engine_set_service modes. With AUTO, a host-API jsp_place of the
 * one-class compaction shape or of a multi-class / multi-level shape whose
 * tiles fit the GPU at once (no tallies requested) is answered by a resident
 * service kernel: one workgroup per tile stays on the
 * GPU, a dispatcher workgroup polls a request word in pinned host memory, and
 * assign[] goes back into pinned memory -- no launch per placement. It is started by the first such
 * jsp_place, stopped by every upload, jsp_engine_set_service/set_fused and
 * jsp_engine_destroy, and leaves by itself after JSP_SERVICE_IDLE_MS
 * (default 50 ms) without a request; jsp_place restarts it when needed, and
 * so does a jsp_snapshot_patch after a placement it answered (the deletions of
 * a recovery patch the snapshot before the recreate places it).
 * While it runs, a device-wide synchronize (hipDeviceSynchronize,
 * torch.cuda.synchronize) waits for it to leave: call
 * jsp_engine_service_stop first (which also keeps patches from restarting it
 * until the next jsp_place it answers). */
#define JSP_SERVICE_OFF 0
#define JSP_SERVICE_AUTO 1     /* default: the multi-class / multi-level shapes are answered by the split
                                  service -- resident tiles tally and hand back per-domain feasibility,
                                  the host walks (stats.fused = 5) */
#define JSP_SERVICE_PARKED 2   /* AUTO without the idle exit (ABI v6): the service stays on the GPU
                                  between requests however long the gap -- a dedicated GPU, where a
                                  recovery hours after the last placement finds it polling (the
                                  GPU analogue of a CPU pool whose threads spin). It leaves on
                                  jsp_engine_service_stop, an upload, a mode change or destroy;
                                  a device-wide synchronize needs the stop first. JSP_SERVICE=parked
                                  in the environment selects it. Freeing device memory waits for
                                  every kernel on the device as well: with several engines on one
                                  GPU, stop a parked service before another engine's destroy or
                                  re-upload (whose frees would otherwise wait for it). */

/* ---- lifecycle ---- */
int jsp_abi_version(void);
const char* jsp_last_error(void);
int jsp_device_count(int* out);
int jsp_engine_create(int device_id, jsp_engine** out);
/* A device-set engine: one handle over n_devices shard engines (device_ids
 * may repeat: several shards on one GPU). The snapshot given to
 * jsp_snapshot_upload (whole: leaves 0..L) is split by whole level-0 domains
 * into row-balanced shards; jsp_place tallies every shard on its device,
 * SUM-combines the per-(class, leaf) tallies -- one RCCL all-reduce over the
 * distinct devices (ncclCommInitAll in this process; librccl.so.1 is loaded
 * at run time), an on-device add between shards that share a device -- and
 * runs feasibility + assignment on device_ids[0]. Results are bit-identical
 * to a single-device engine (integer sums). Uploads, patches, jsp_place /
 * jsp_place_jobs, jsp_resolve_leader_domains, jsp_audit_placements and the
 * settings work as on a single engine; the *_device entry points return
 * JSP_ESTATE (the device buffers span devices). stats.fused = 6.
 * Replaces, for the Go manager's one process (main.go:161-190), the
 * per-rank torch.distributed step of jobset_amd/distributed.py. */
int jsp_engine_create_multi(const int* device_ids, int n_devices, jsp_engine** out);
/* shards of a device-set engine and its distinct devices (1 and 1 for a
 * single-device engine) */
int jsp_engine_shards(jsp_engine* e, int* shards, int* devices);
void jsp_engine_destroy(jsp_engine* e);

/* ---- snapshot ---- */
int jsp_topology_upload(jsp_engine* e, const jsp_topology* topo);
int jsp_snapshot_upload(jsp_engine* e, const jsp_nodes* nodes);
/* Overwrite n rows (ids in `rows`, local to this shard) of the resident
 * snapshot. delta columns are [W][n], [n], [R][n], [n] (NULL: column
 * unchanged); structure (leaf ranges) is unchanged. The call copies the delta
 * into pinned staging and returns without waiting for the device (ABI v5);
 * every later call sees the patched rows. Who applies it:
 *  - the resident service, when it is up: its dispatcher workgroup reads the
 *    staged delta (up to 4096 rows in one host-link round trip) and writes the
 *    rows; no launch. The patch is posted at once, so it lands during the gap
 *    before the next request, and a request that finds it not yet taken
 *    carries it again (writing a staged delta twice writes the same values);
 *    a dispatcher that never takes it (bounded wait) is stopped and the patch
 *    kernel applies it;
 *  - after the service left, while it is armed (the last jsp_place was
 *    answered by it): a patch is the first sign of a recovery, so the engine's
 *    waker thread restarts the service and posts the patch, followed by a
 *    warm-up request without jobs, off the caller's thread;
 *  - otherwise a patch kernel on the engine stream.
 * Later launches wait for its completion word (or are stream-ordered after
 * the patch kernel); uploads and jsp_engine_sync apply pending patches first. */
int jsp_snapshot_patch(jsp_engine* e, const uint32_t* rows, uint32_t n,
                       const uint64_t* labels, const uint32_t* taints,
                       const uint32_t* free_res, const int32_t* excl_owner);
int jsp_classes_upload(jsp_engine* e, const jsp_job_class* classes, uint32_t n_classes);

/* ---- placement (host buffers; includes H2D of the runs and D2H of results) ----
 * Jobs arrive as replicated-job runs in global order: run i is run_len[i]
 * consecutive jobs of class run_class[i] (one ReplicatedJob with
 * rjob.Replicas children, jobset_controller.go:638-649; global job index =
 * globalJobIndex, :1056-1065). n_jobs = sum of run_len.
 * The list is taken as it comes, one run per ReplicatedJob: run_len[i] == 0 is
 * allowed (replicas: 0; its class id must still be < n_classes), adjacent runs
 * may share a class, and neither changes the answer, which depends on the job
 * sequence alone. jsp_stats.runs counts the runs as passed, empty ones
 * included, and the launch-shape choice looks at that count (more than 32
 * runs leave the level walker, jsp_stats.fused above). The same holds for the
 * device-resident lists of jsp_place_device and jsp_assign_device.
 * assign_out [n_jobs]: domain id at the job's class level, -1 = unplaceable.
 * tally_out (nullable) [C][n_leaves_total]: per-(class, leaf) pod capacity.
 * occ_out (nullable) [n_leaves_total]: rows covered by other exclusive jobs. */
int jsp_place(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
              int32_t* assign_out, uint32_t* tally_out, uint32_t* occ_out, jsp_stats* stats);
/* Same with one class id per job (run-length encoded on the host). */
int jsp_place_jobs(jsp_engine* e, const uint32_t* job_class, uint32_t n_jobs,
                   int32_t* assign_out, uint32_t* tally_out, uint32_t* occ_out, jsp_stats* stats);

/* ---- sticky placement: jobs keep their previous domains at recreate ----
 * jsp_place's batch plus prev_assign[n_jobs]: the domain (at the level of the
 * job's class) the job held before, or -1 for no hint; NULL = no hint at all.
 * The rule (DESIGN.md §2 "Sticky placement"), on the current snapshot after
 * every pending patch:
 *  1. job j with prev d >= 0 is a claimant iff d is feasible for its class;
 *  2. a claimant keeps d iff no claimant j' < j claims a domain whose leaf
 *     range intersects d's (the same domain, an ancestor or a descendant);
 *     kept jobs get assign[j] = prev[j];
 *  3. all other jobs, in global order, are placed by jsp_place's lowest-index
 *     rule, with every domain that intersects a kept one taken from the start.
 * prev all -1 (or NULL) gives jsp_place's answer; prev equal to jsp_place's
 * answer on the same snapshot is a fixed point. A kept job has assign[j] ==
 * prev[j]; for pairwise disjoint hints (any earlier placement) no other hinted
 * job has.
 * Host buffers; runs on the engine's stream (ordered after every pending
 * patch, those posted to the resident service's dispatcher included) and
 * returns when done. The resident service, when up, stays up and keeps its
 * tiles. Counts in the place_us, batch_jobs, placed, unplaceable and
 * place_errors metrics as jsp_place does.
 * JSP_EINVAL: NULL engine, NULL assign_out with jobs, a run class out of
 * range, prev[j] < -1 or >= the domains of job j's level (the message names
 * the job); JSP_ESTATE: no topology, snapshot or classes yet, a device-set
 * engine, a sharded engine.
 * Added within ABI v7 (JSP_ABI_VERSION is unchanged: nothing existing moved);
 * a caller that may meet an older library detects it by symbol (dlsym). */
typedef struct jsp_sticky_stats {
    uint32_t jobs;             /* J */
    uint32_t placed;           /* assign[j] != -1, kept jobs included */
    uint32_t hinted;           /* prev[j] >= 0 */
    uint32_t kept;             /* jobs that kept their domain by rule 2 */
    uint32_t runs;             /* runs the fill walked */
    uint32_t fused;            /* shape of the fill's walk: 0 on the GPU, 7 on the host (jsp_stats.fused) */
    double wall_us;            /* host wall time of the call */
} jsp_sticky_stats;                                  /* 32 bytes */
int jsp_place_sticky(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                     const int32_t* prev_assign, int32_t* assign_out, jsp_sticky_stats* stats);

/* ---- gang placement: whole JobSets inside one span domain, or nothing ----
 * jsp_place decides job by job: a JobSet whose last job finds no domain keeps
 * the domains of its first jobs, and nothing keeps its jobs together. Here the
 * batch is cut into gangs (one JobSet each): gang g is the next gang_runs[g]
 * consecutive runs (their sum is n_runs), and gang_span[g] is a topology level
 * or JSP_SPAN_ANY. The rule (DESIGN.md §2 "Gang placement"), on the current
 * snapshot after every pending patch, with jsp_place's feasibility and
 * intersection marking and a taken set T that starts empty; gangs in order:
 *  1. the candidates are the domains S of level gang_span[g] in ascending id
 *     (JSP_SPAN_ANY: one candidate, the whole cluster);
 *  2. trial(S): the gang's jobs in global order; a job of class c takes the
 *     lowest domain d at level[c] whose leaf range is non-empty and lies inside
 *     S's, that is feasible for c and neither in T nor taken earlier in the
 *     trial (a take marks every intersecting domain at every level); the trial
 *     succeeds iff every job got a domain;
 *  3. the gang takes the lowest S whose trial succeeds: assign[] is that
 *     trial's answer, T its taken set, gang_span_out[g] = S (0 for
 *     JSP_SPAN_ANY); with no such S every job of the gang gets -1, T stays as
 *     it was and gang_span_out[g] = -1. A gang without jobs takes nothing, gets
 *     -1 and is not counted as placed.
 * One gang per job with JSP_SPAN_ANY is jsp_place's answer; one gang over the
 * whole batch with JSP_SPAN_ANY is jsp_place's answer if that places every job
 * and all -1 otherwise. The trial is greedy: on a gang of several classes it
 * can refuse an S in which another matching exists.
 * Host buffers; runs on the engine's stream (ordered after every pending
 * patch, those posted to the resident service's dispatcher included) and
 * returns when done. The resident service, when up, stays up and keeps its
 * tiles. Counts in jsp_metrics as jsp_place_sticky does. The walk runs on the
 * host behind the GPU's feasibility words and span counts: stats.fused = 7.
 * JSP_EINVAL (the message names the gang): NULL engine, NULL buffers where
 * counts are nonzero, a run class out of range, flags != 0, sum(gang_runs) !=
 * n_runs, a gang_span[g] that is neither JSP_SPAN_ANY nor a level < n_levels,
 * a span finer than the level of a class among the gang's non-empty runs (a
 * span equal to it is allowed); JSP_ESTATE: no topology, snapshot or classes
 * yet, a device-set engine, a sharded engine; JSP_ERANGE: more than
 * JSP_GANG_MAX_JOBS jobs (checked before anything is allocated). After a
 * refusal the output buffers are unspecified and the engine stays usable.
 * Added within ABI v7 (JSP_ABI_VERSION is unchanged: nothing existing moved);
 * a caller that may meet an older library detects it by symbol (dlsym). */
#define JSP_SPAN_ANY 0xFFFFFFFFu
#define JSP_GANG_MAX_JOBS 65536u
typedef struct jsp_gang_stats {
    uint32_t jobs;             /* J */
    uint32_t placed;           /* assign[j] != -1 */
    uint32_t gangs;            /* G */
    uint32_t gangs_placed;     /* gangs that got a span domain */
    uint32_t runs;             /* non-empty runs */
    uint32_t fused;            /* 7: the walk runs on the host (jsp_stats.fused) */
    double wall_us;            /* host wall time of the call */
} jsp_gang_stats;                                    /* 32 bytes */
int jsp_place_gangs(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                    const uint32_t* gang_runs, const uint32_t* gang_span, uint32_t n_gangs,
                    uint32_t flags /* must be 0 */, int32_t* assign_out /* [J] */,
                    int32_t* gang_span_out /* nullable, [G] */, jsp_gang_stats* stats /* nullable */);

/* ---- fit placement: the tightest or the roomiest feasible domain per job ----
 * Replaces kube-scheduler's score phase (NodeResourcesFit MostAllocated /
 * LeastAllocated), which is out of tree for the reference: its requirements
 * (go.mod:5-25) hold the API and client modules and no scheduler, so the
 * choice among the feasible nodes is the cluster's scheduler's. jsp_place, jsp_place_sticky and
 * jsp_place_gangs hand a job the lowest-id feasible domain; with exclusive
 * placement a job owns its whole domain, so a small job on the big rack
 * strands the rest of that rack. The rule (DESIGN.md §2 "Fit placement"), on
 * the current snapshot after every pending patch, with jsp_place's cap,
 * capsum, feasibility and intersection marking:
 *   fit(c,d) = min(capsum(c,d), 0xFFFFFFFF)      capsum: the 64-bit sum of the
 *              u32 per-leaf tallies (tally_out) over the leaves of d at level[c]
 * Jobs in global order; job j of class c takes, among the domains d at
 * level[c] that are feasible for c and not taken, the one with the smallest
 * (key(c,d), d), or gets -1; a take marks every intersecting domain at every
 * level.
 *   JSP_FIT_LOWEST:   key = 0                    jsp_place's answer, bit for bit
 *   JSP_FIT_TIGHTEST: key = fit(c,d)             smallest domain that still fits
 *   JSP_FIT_ROOMIEST: key = 0xFFFFFFFF - fit(c,d)  most capacity
 * Ties go to the lowest id. Keys depend on the snapshot and the classes only,
 * never on the batch. Both fit policies are greedy: nothing promises more
 * placed jobs than jsp_place.
 * Host buffers; runs on the engine's stream (ordered after every pending
 * patch, those posted to the resident service's dispatcher included) and
 * returns when done. The resident service, when up, stays up and keeps its
 * tiles. Counts in jsp_metrics as jsp_place_sticky does. The walk runs on the
 * host behind the GPU's per-class candidate lists: stats.fused = 7.
 * JSP_EINVAL (the message names the run where there is one): NULL engine,
 * NULL run buffers with runs, NULL assign_out with jobs, a run class out of
 * range, flags != 0, policy > 2; JSP_ESTATE: no topology, snapshot or classes
 * yet, a device-set engine, a sharded engine; JSP_ERANGE: more than
 * JSP_FIT_MAX_JOBS jobs (checked before anything is allocated). After a
 * refusal the output is unspecified and the engine stays usable.
 * Added within ABI v7 (JSP_ABI_VERSION is unchanged: nothing existing moved);
 * a caller that may meet an older library detects it by symbol (dlsym). */
#define JSP_FIT_LOWEST 0u
#define JSP_FIT_TIGHTEST 1u
#define JSP_FIT_ROOMIEST 2u
#define JSP_FIT_MAX_JOBS 65536u
typedef struct jsp_fit_stats {
    uint32_t jobs;             /* J */
    uint32_t placed;           /* assign[j] != -1 */
    uint32_t runs;             /* non-empty runs */
    uint32_t fused;            /* 7: the walk runs on the host (jsp_stats.fused) */
    uint64_t slack;            /* sum over placed jobs of fit(c_j, assign[j]) - min(pods[c_j], 0xFFFFFFFF) */
    double wall_us;            /* host wall time of the call */
} jsp_fit_stats;                                     /* 32 bytes */
int jsp_place_fit(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                  uint32_t policy, uint32_t flags /* must be 0 */, int32_t* assign_out /* [J] */,
                  jsp_fit_stats* stats /* nullable */);

/* ---- what-if placement: place under hypothetical row edits, nothing written ----
 * Replaces the dry run behind kube-scheduler's PostFilter phase (preemption:
 * "if this lower-priority JobSet went away, would mine fit, and where?") and
 * the cluster autoscaler's scale-down simulation ("without these nodes, does
 * the recreate still place?"). Both are out of tree for the reference, as the
 * score phase is (jsp_place_fit above): its requirements (go.mod:5-25) hold no
 * scheduler and no autoscaler. The rule (DESIGN.md §2 "What-if placement"):
 * scenario s is the row delta rows[scen_off[s] .. scen_off[s+1]) with its
 * slice of the four delta columns, laid out as jsp_snapshot_patch's over all
 * n_total = scen_off[S] rows (labels [W][n_total], free_res [R][n_total]); a
 * NULL column keeps the resident values, in every scenario.
 *   assign_out[s][0..J) = to the bit, what jsp_place would answer on the
 *     snapshot jsp_snapshot_patch(rows of s, delta of s) would make of the
 *     current one (after every pending patch, those posted to the resident
 *     service's dispatcher included);
 *   placed_out[s] = its entries that are not -1.
 * Scenarios are independent of each other; one without rows gives jsp_place's
 * answer. Inside a scenario the rows are strictly ascending (a row once);
 * across scenarios a row may come again with other values.
 * Nothing moves: the resident snapshot is never written, the resident service,
 * when up, stays up and keeps its tiles, the host lease and its kept list stay
 * valid, a jsp_place behind the call is answered as if it had not happened,
 * and the call is not counted in jsp_metrics. The GPU re-decides the touched
 * (class, domain) bits per scenario in a copy of the feasibility words; the
 * walk runs on the host, once per scenario: stats.fused = 7.
 * JSP_EINVAL (the message names the scenario and the position where there is
 * one): NULL engine, NULL run buffers with runs, NULL assign_out with S J > 0,
 * NULL scen_off with scenarios, NULL rows with n_total > 0, all four delta
 * columns NULL with n_total > 0, a run class out of range, flags != 0,
 * scen_off[0] != 0 or a decreasing scen_off, a row >= N, rows of one scenario
 * not strictly ascending; JSP_ESTATE: no topology, snapshot or classes yet, a
 * device-set engine, a sharded engine; JSP_ERANGE (checked before anything is
 * allocated): more than JSP_WHATIF_MAX_JOBS jobs, JSP_WHATIF_MAX_SCENARIOS
 * scenarios or JSP_WHATIF_MAX_ROWS rows in all. n_scen == 0 or J == 0 is
 * JSP_OK with nothing written. After a refusal the outputs are unspecified
 * and the engine stays usable.
 * Added within ABI v7 (JSP_ABI_VERSION is unchanged: nothing existing moved);
 * a caller that may meet an older library detects it by symbol (dlsym). */
#define JSP_WHATIF_MAX_JOBS 65536u
#define JSP_WHATIF_MAX_SCENARIOS 64u
#define JSP_WHATIF_MAX_ROWS 65536u
typedef struct jsp_whatif_stats {
    uint32_t jobs;             /* J */
    uint32_t scenarios;        /* S */
    uint32_t rows;             /* n_total */
    uint32_t runs;             /* non-empty runs */
    uint32_t fused;            /* 7: the walks run on the host (jsp_stats.fused) */
    uint32_t flips;            /* (scenario, class, domain at level[class]) triples whose feasibility
                                  bit differs from the unedited snapshot's */
    double wall_us;            /* host wall time of the call */
} jsp_whatif_stats;                                  /* 32 bytes */
int jsp_place_whatif(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                     const uint32_t* scen_off /* [S+1], scen_off[0] == 0, non-decreasing */, uint32_t n_scen,
                     const uint32_t* rows /* [n_total = scen_off[S]] engine-local row ids */,
                     const uint64_t* labels /* nullable, [W][n_total] */,
                     const uint32_t* taints /* nullable, [n_total] */,
                     const uint32_t* free_res /* nullable, [R][n_total] */,
                     const int32_t* excl_owner /* nullable, [n_total] */, uint32_t flags /* must be 0 */,
                     int32_t* assign_out /* [S][J] */, uint32_t* placed_out /* nullable, [S] */,
                     jsp_whatif_stats* stats /* nullable */);

/* ---- preemptive placement: place jobs by evicting lower-priority owners ----
 * Replaces the search of kube-scheduler's PostFilter phase (preemption: which
 * domain, at what cost, with which victims) on the exclusive-placement path.
 * It is out of tree for the reference, as the score phase and the dry run are
 * (jsp_place_fit, jsp_place_whatif above): its requirements (go.mod:5-25) hold
 * no scheduler, and its troubleshooting page (section 3) leaves preemption to
 * Kueue. The rule (DESIGN.md §2 "Preemptive placement"): the batch has one
 * priority rank `prio` (0..65535); owner_ids[n_owners] with owner_prio[n_owners]
 * (ranks 0..65534; the caller maps its PriorityClass values to dense ranks) is
 * the victim table. On the current snapshot (after every pending patch, those
 * posted to the resident service's dispatcher included) a row n with
 * o = excl_owner[n] is
 *   free     o == -1;
 *   victim   o is in the table with a rank < prio (strict: equal priority
 *            never preempts);
 *   blocker  every other owned row (an id not in the table, a rank >= prio).
 * cap'(c, n) is the tally's per-row pod capacity with free_res replaced, on
 * victim rows only, by evict_free[.][n] (the free values the row has once its
 * owner's pods are gone; NULL: free_res as it is, the right value for domains
 * held by jsp_assume, which writes excl_owner alone). Per-leaf sums are u32
 * (modulo 2^32), capsum'(c, d) over a domain's leaves is 64-bit, as the
 * tally's. For domain d at level[c] with rows [r0, r1):
 *   reach(c, d)  capsum'(c, d) >= pods[c] and no row of d is a blocker;
 *   seg(d)       the rows n of d with excl_owner[n] != -1 and (n == r0 or
 *                excl_owner[n-1] != excl_owner[n]): the owner segments, which
 *                are the distinct owners when each owner's rows are contiguous;
 *   hp(d)        0 without a victim row, else 1 + the largest victim rank;
 *   key(c, d)    (hp(d) << 16) | min(seg(d), 0xFFFF): 0 exactly for the
 *                domains jsp_place calls feasible.
 * Jobs in global order; job j of class c takes, among the reachable domains
 * not yet taken, the one with the smallest (key(c, d), d), or gets -1; a take
 * marks every intersecting domain at every level, as in jsp_place. This is
 * the order of kube-scheduler's pickOneNodeForPreemption: no victims, then the
 * lowest highest-victim priority, then the fewest victims, then the lowest id.
 * Keys are static across the walk. n_owners == 0 or prio == 0 gives jsp_place's
 * answer bit for bit, without victims.
 *   assign_out[j]      the domain or -1;
 *   victim_off_out     (nullable) [J + 1]: job j's victims are
 *                      victims_out[victim_off_out[j] .. victim_off_out[j+1]);
 *   victims_out        (nullable: the list is not wanted; offsets and stats
 *                      are still filled) the owners at the segment heads of
 *                      each placed job's domain, in ascending row order; an
 *                      owner with rows in two taken domains is named under
 *                      both. More entries than victims_cap: JSP_ERANGE, the
 *                      message carries the total; victims_cap >= N never
 *                      refuses (taken domains are disjoint).
 * Nothing moves: the resident snapshot is never written, the resident service,
 * when up, stays up and keeps its tiles, the host lease and its kept list stay
 * valid, a jsp_place behind the call is answered as if it had not happened,
 * and the call is not counted in jsp_metrics. The caller evicts the victims,
 * lets the informer's patch (or jsp_forget) open the domains, and calls
 * jsp_assume on the answer. The GPU classifies the rows, tallies cap', builds
 * and orders the keys and gathers the victims; the walk runs on the host:
 * stats.fused = 7.
 * JSP_EINVAL (the message names the run or the table index): NULL engine, NULL
 * run buffers with runs, NULL assign_out with J > 0, NULL owner_ids or
 * owner_prio with n_owners > 0, a run class out of range, flags != 0,
 * prio > JSP_PREEMPT_MAX_PRIO, an owner_prio[i] >= JSP_PREEMPT_MAX_PRIO, -1 in
 * owner_ids, the same id twice in owner_ids; JSP_ESTATE: no topology, snapshot
 * or classes yet, a device-set engine, a sharded engine; JSP_ERANGE (checked
 * before anything is allocated): more than JSP_PREEMPT_MAX_JOBS jobs or
 * JSP_PREEMPT_MAX_OWNERS owners. J == 0 is JSP_OK with nothing launched. After
 * a refusal the outputs are unspecified and the engine stays usable.
 * Added within ABI v7 (JSP_ABI_VERSION is unchanged: nothing existing moved);
 * a caller that may meet an older library detects it by symbol (dlsym). */
#define JSP_PREEMPT_MAX_JOBS 65536u
#define JSP_PREEMPT_MAX_OWNERS 65536u
#define JSP_PREEMPT_MAX_PRIO 65535u   /* prio <= this; owner_prio[i] < this */
typedef struct jsp_preempt_stats {
    uint32_t jobs;             /* J */
    uint32_t placed;           /* entries of assign_out that are not -1 */
    uint32_t preempting;       /* placed jobs with at least one victim */
    uint32_t victims;          /* entries of the victim list (sum of seg over placed jobs) */
    uint32_t runs;             /* non-empty runs */
    uint32_t fused;            /* 7: the walk runs on the host (jsp_stats.fused) */
    double wall_us;            /* host wall time of the call */
} jsp_preempt_stats;                                 /* 32 bytes */
int jsp_place_preempt(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                      uint32_t prio, const int32_t* owner_ids, const uint32_t* owner_prio, uint32_t n_owners,
                      const uint32_t* evict_free /* nullable, [R][N] */, uint32_t flags /* must be 0 */,
                      int32_t* assign_out /* [J] */, uint32_t* victim_off_out /* nullable, [J+1] */,
                      int32_t* victims_out /* nullable, [victims_cap] */, uint32_t victims_cap,
                      jsp_preempt_stats* stats /* nullable */);

/* ---- spread placement: a batch's jobs spread evenly over a topology level ----
 * Replaces kube-scheduler's PodTopologySpread plugin (topologySpreadConstraints:
 * topologyKey, maxSkew, whenUnsatisfiable) on the exclusive-placement path. It
 * is out of tree for the reference, as the score phase and preemption are
 * (jsp_place_fit, jsp_place_preempt above): its requirements (go.mod:5-25)
 * hold no scheduler. jsp_place_gangs keeps jobs together; this call keeps them
 * apart, evenly. The rule (DESIGN.md §2 "Spread placement"): the call takes
 * jsp_place's runs, a spread level s (the topologyKey), max_skew (>= 1:
 * DoNotSchedule; JSP_SPREAD_SOFT: ScheduleAnyway with the spread score as the
 * only score) and peer_ids[n_peers], the excl_owner ids of the jobs that count
 * as already placed (the JobSet's jobs still running at a partial recreate or
 * a scale-up). On the current snapshot (after every pending patch, those
 * posted to the resident service's dispatcher included), with cap, capsum,
 * occsum, feasibility and the marking of intersecting domains as in jsp_place:
 *   fits(c, d)   capsum(c, d) >= pods[c], occupancy ignored;
 *                feasible(c, d) = fits(c, d) && occsum(d) == 0, as ever;
 *   elig(c, S)   for a level-s domain S: some domain d at level[c] inside S
 *                has fits(c, d). Only eligible S enter the minimum below: an S
 *                that could never host the class does not pin it at 0, one
 *                that is merely full does, as in kube-scheduler;
 *   peers(S)     the rows n of S, rows [r0, r1), with excl_owner[n] in
 *                peer_ids and (n == r0 or excl_owner[n-1] != excl_owner[n]):
 *                jsp_place_preempt's owner segments restarted at r0, the peer
 *                jobs in S when each owner's rows are contiguous; an owner
 *                whose rows span two S counts in both.
 * n[S] starts at peers(S). Jobs in global order; for job j of class c:
 * m = min n[S] over the S with elig(c, S); the candidates are the eligible S
 * that hold a feasible d at level[c] not yet taken and, with max_skew >= 1,
 * satisfy n[S] + 1 - m <= max_skew; without a candidate the job gets -1
 * (counted in stats.refused when an eligible S with a free feasible d existed
 * and the skew test alone removed it) and nothing changes; else it takes the
 * candidate with the smallest (n[S], S) and inside it the lowest such d,
 * n[S] += 1, and the take marks every intersecting domain at every level. The
 * rule is greedy, and static apart from n[] and the taken set: a full eligible
 * S with few peers can make later jobs unplaceable, which is kube-scheduler's
 * behaviour. minDomains, several constraints per job and per-class spread
 * levels are left out. A topology with one level-s domain gives jsp_place's
 * answer bit for bit; so does one class with level[c] == s and no peers.
 *   assign_out[j]   the domain at level[c] or -1;
 *   spread_out[j]   (nullable) the level-s domain S the job went to, or -1;
 *   count_out[S]    (nullable, [D_s]) the final n[].
 * The call is host-buffered and runs on the engine's stream; the resident
 * service and the host lease are left as jsp_place_fit leaves them, and the
 * call counts in jsp_metrics as jsp_place_fit does. The GPU tallies, builds
 * the feasibility and the fits words, counts both per (class, S) and counts
 * the peers; the walk runs on the host: stats.fused = 7.
 * JSP_EINVAL (the message names the run or the table index): NULL engine, NULL
 * run buffers with runs, NULL assign_out with J > 0, NULL peer_ids with
 * n_peers > 0, a run class out of range, flags != 0,
 * spread_level >= n_levels, a spread level finer than
 * the level of a class among the non-empty runs (equal is allowed), -1 in
 * peer_ids, the same id twice in peer_ids; JSP_ESTATE: no topology, snapshot
 * or classes yet, a device-set engine, a sharded engine; JSP_ERANGE (checked
 * before anything is allocated): more than JSP_SPREAD_MAX_JOBS jobs or
 * JSP_SPREAD_MAX_PEERS peers. J == 0 is JSP_OK, and count_out, where given,
 * is still filled with peers(S). After a refusal the outputs are unspecified
 * and the engine stays usable.
 * Added within ABI v7 (JSP_ABI_VERSION is unchanged: nothing existing moved);
 * a caller that may meet an older library detects it by symbol (dlsym). */
#define JSP_SPREAD_SOFT 0u
#define JSP_SPREAD_MAX_JOBS 65536u
#define JSP_SPREAD_MAX_PEERS 65536u
typedef struct jsp_spread_stats {
    uint32_t jobs;             /* J */
    uint32_t placed;           /* entries of assign_out that are not -1 */
    uint32_t refused;          /* -1 by the skew test alone */
    uint32_t skew;             /* max n - min n after the walk, over the S eligible for a class of a non-empty run */
    uint32_t runs;             /* non-empty runs */
    uint32_t fused;            /* 7: the walk runs on the host (jsp_stats.fused) */
    double wall_us;            /* host wall time of the call */
} jsp_spread_stats;                                  /* 32 bytes */
int jsp_place_spread(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                     uint32_t spread_level, uint32_t max_skew, const int32_t* peer_ids, uint32_t n_peers,
                     uint32_t flags /* must be 0 */, int32_t* assign_out /* [J] */,
                     int32_t* spread_out /* nullable, [J] */, uint32_t* count_out /* nullable, [D_s]: final n[] */,
                     jsp_spread_stats* stats /* nullable */);

/* ---- pod binding: a node row for every pod of a placed job ----
 * Replaces kube-scheduler's per-pod node choice inside a domain the exclusive
 * affinity terms already fixed: after the leader lands, the reference leaves
 * every follower pod to the scheduler, which re-evaluates the selector, taint
 * and resource predicates per pod to pick a node of the leader's domain (the
 * scheduler is out of tree for the reference, go.mod:5-25; its published
 * 290 pods/s at 15k nodes, README.md:30, is this leg). The pod webhook can pin
 * a pod to its row's node by completion index, which is how it finds the
 * leader today (pod_mutating_webhook.go:95-171).
 * Input: jsp_place's runs and assign[n_jobs], a domain id at the level of the
 * job's class or -1 -- any assignment, not only one jsp_place produced. The
 * rule (DESIGN.md §2 "Pod binding"), on the current snapshot after every
 * pending patch, for job j of class c with d = assign[j] >= 0:
 *  1. j is bound iff d is feasible for c now (the sum of cap(c, n) over d's
 *     rows reaches pods[c] and no row of d has an exclusive owner), else
 *     stale: every pod of a stale or unplaced job gets -1;
 *  2. pod p of a bound job goes to the row n of d with pre(n) <= p < pre(n) +
 *     cap(c, n), pre(n) the sum of cap(c, m) over d's rows m < n: first fit by
 *     row, pod 0 (the leader) on the domain's first fitting row;
 *  3. pod_row_out[pod_off[j] + p] is the engine-local row or -1, pod_off[j]
 *     the pods of all jobs before j (unplaced ones included), P = pod_off[J].
 * pod_off_out (nullable) receives pod_off[0..J].
 * Host buffers; runs on the engine's stream (ordered after every pending
 * patch, those posted to the resident service's dispatcher included) and
 * returns when done. The resident service, when up, stays up and keeps its
 * tiles. The snapshot is not modified: the bound rows are not reserved.
 * Not counted in jsp_metrics (its layout is fixed within ABI v7).
 * JSP_EINVAL: NULL engine, NULL assign or pod_row_out with jobs, a run class
 * out of range, flags != 0, assign[j] < -1 or >= the domains of job j's level
 * (the message names the job), two jobs whose domains' leaf ranges intersect
 * (the same domain, an ancestor or a descendant: the message names the lowest
 * job that an earlier job intersects); JSP_ESTATE: no topology, snapshot or
 * classes yet, a device-set engine, a sharded engine; JSP_ERANGE: P >
 * JSP_BIND_MAX_PODS (checked before anything is allocated). After a refusal
 * the output buffers are unspecified and the engine stays usable.
 * Added within ABI v7 (JSP_ABI_VERSION is unchanged: nothing existing moved);
 * a caller that may meet an older library detects it by symbol (dlsym). */
#define JSP_BIND_MAX_PODS (1u << 24)
typedef struct jsp_bind_stats {
    uint32_t jobs;             /* J */
    uint32_t bound;            /* jobs whose pods all got a row */
    uint32_t stale;            /* assign[j] >= 0 but the domain is not feasible now */
    uint32_t rows_used;        /* distinct rows that received at least one pod */
    uint64_t pods;             /* P */
    uint64_t pods_bound;       /* entries of pod_row_out that are not -1 */
    double wall_us;            /* host wall time of the call */
} jsp_bind_stats;                                    /* 40 bytes */
int jsp_bind_pods(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                  const int32_t* assign, uint32_t flags /* must be 0 */,
                  int32_t* pod_row_out /* [P] */, uint64_t* pod_off_out /* nullable, [J+1] */,
                  jsp_bind_stats* stats /* nullable */);

/* ---- assume and forget: hold placed domains until the informer shows them ----
 * jsp_place, jsp_place_sticky and jsp_bind_pods leave the resident snapshot as
 * it is, so two batches placed back to back get the same domains until the
 * first batch's pods exist, the informer has seen them and a patch has reached
 * the engine. jsp_assume closes that window as kube-scheduler's assume step
 * does: the decision enters the snapshot at once and is confirmed by the
 * informer's patch or taken back by jsp_forget (DESIGN.md §2 "Assume and
 * forget").
 *
 * jsp_assume takes jsp_place's runs, an assignment and one owner id per job.
 * On the current snapshot, after every pending patch, job j of class c with
 * d = assign[j] >= 0 is
 *   committed  iff feasible(c, d) holds now -- jsp_bind_pods' rule and the
 *              tally's cap, to the bit; every row n < N of d then gets
 *              excl_owner[n] = owner[j];
 *   stale      otherwise: nothing is written for it.
 * Only excl_owner is written: labels, taints and free_res stay as they are.
 * An owned domain is closed to every class at every level whatever its free
 * columns say (occsum > 0); the informer's patch brings the real values later.
 * So a committed job is infeasible for everyone afterwards, itself included:
 * a second jsp_assume of it is stale and so is a jsp_bind_pods of it (bind
 * first, then assume), and a recreate that wants to keep its domains through
 * jsp_place_sticky forgets its owners first. A domain without leaves claims
 * nothing, conflicts with nothing and is stale; owner[j] of an unplaced job
 * (assign[j] == -1) is ignored. Owner ids are the caller's; a caller that
 * mixes them with informer-derived ids (dense from 0) draws them from
 * 0x40000000 upward.
 *
 * All or nothing: after JSP_EINVAL (NULL engine; NULL assign or owner with
 * jobs; a run class out of range; flags != 0; owner[j] == -1 for a placed job;
 * assign[j] < -1 or >= D_level; two jobs whose domains' leaf ranges intersect:
 * the message names the lowest job that an earlier one intersects) or
 * JSP_ESTATE (no topology, snapshot or classes yet; a device-set or sharded
 * engine) no row of any job has been written.
 *
 * jsp_forget: every row n < N whose excl_owner is in owners[] gets -1, and the
 * count of such rows goes to rows_cleared_out. A pure function of the snapshot
 * and the list (the engine keeps no ledger): rows owned by any other id --
 * those the informer has confirmed in the meantime included -- are untouched.
 * Duplicates are allowed; n_owners == 0 clears nothing. JSP_EINVAL: a NULL
 * list with n_owners > 0, or -1 in the list; JSP_ERANGE: more than
 * JSP_FORGET_MAX_OWNERS; JSP_ESTATE as for jsp_assume.
 *
 * Both take host buffers, run on the engine's stream ordered after every
 * pending patch and return when done. The resident service, when up, stays
 * up: its tiles reload their rows with the next request. Neither call is
 * counted in jsp_metrics. Added within ABI v7 (JSP_ABI_VERSION is unchanged);
 * a caller detects them by symbol. */
typedef struct jsp_assume_stats {
    uint32_t jobs;             /* J */
    uint32_t committed;        /* jobs whose domain was marked */
    uint32_t stale;            /* assign[j] >= 0 but the domain is not feasible now: nothing written for it */
    uint32_t reserved;         /* 0 */
    uint64_t rows_marked;      /* rows whose excl_owner was written */
    double wall_us;            /* host wall time of the call */
} jsp_assume_stats;                                  /* 32 bytes */
int jsp_assume(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
               const int32_t* assign /* [J] */, const int32_t* owner /* [J] */, uint32_t flags /* must be 0 */,
               uint8_t* committed_out /* nullable, [J]: 1 committed, 0 stale or unplaced */,
               jsp_assume_stats* stats /* nullable */);

#define JSP_FORGET_MAX_OWNERS 65536u
int jsp_forget(jsp_engine* e, const int32_t* owners, uint32_t n_owners,
               uint64_t* rows_cleared_out /* nullable */);

/* ---- placement (device-resident buffers) ----
 * `stream` is a hipStream_t used as given: NULL = the HIP null stream (torch's
 * default stream), jsp_engine_stream(e) = the engine's own stream.
 * d_cap [C][ld] and d_occ [ld] with ld >= total leaves; a shard writes only
 * columns [leaf_begin, leaf_begin+n_leaves) so the caller can SUM-all-reduce
 * zero-initialised buffers across shards before jsp_assign_device.
 * d_run_class / d_run_len [n_runs] as for jsp_place; n_jobs = their sum. */
int jsp_tally_device(jsp_engine* e, uint32_t* d_cap, uint32_t* d_occ, uint32_t ld,
                     void* stream);
int jsp_assign_device(jsp_engine* e, const uint32_t* d_cap, const uint32_t* d_occ,
                      uint32_t ld, const uint32_t* d_run_class, const uint32_t* d_run_len,
                      uint32_t n_runs, uint32_t n_jobs, int32_t* d_assign, void* stream);
int jsp_place_device(jsp_engine* e, const uint32_t* d_run_class, const uint32_t* d_run_len,
                     uint32_t n_runs, uint32_t n_jobs, int32_t* d_assign, void* stream);

/* ---- follower pinning and audit (batched webhook / PodReconciler work) ----
 * jsp_resolve_leader_domains: for each job, the domain (at `levels[i]`) of
 * the node row its leader is bound to; -1 when the row is -1 (leader not
 * bound / node unknown). Host buffers.
 * jsp_audit_placements: for each job i, followers [follower_off[i],
 * follower_off[i+1]) carry the interned domain id their nodeSelector names
 * (-1 = selector missing); bad_out[i] = number of followers whose domain
 * differs from the domain of leader_rows[i] at levels[i], or 0xFFFFFFFF when
 * the leader row is -1 (leader node unknown). */
int jsp_resolve_leader_domains(jsp_engine* e, const int32_t* leader_rows,
                               const uint32_t* levels, uint32_t n, int32_t* domain_out);
int jsp_audit_placements(jsp_engine* e, const int32_t* leader_rows, const uint32_t* levels,
                         const uint32_t* follower_off, const int32_t* follower_domains,
                         uint32_t n_jobs, uint32_t* bad_out);

/* ---- why jobs cannot be placed ----
 * Per class, the counts behind an `assign[j] = -1`: what kube-scheduler's
 * FailedScheduling message ("0/N nodes are available: X didn't match node
 * selector, Y had untolerated taint, Z Insufficient cpu") tells an operator,
 * and what the reference never sees, because the scheduler that takes the
 * decision is out of tree (go.mod:5-25). Snapshot-only and independent of any
 * batch: over the N rows the engine holds, after every pending
 * patch, each row is counted under the first test of its class it fails --
 * selector, then taints, then resources -- or as fitting at least one pod:
 *   rows == rows_selector + rows_taint + rows_no_capacity + rows_fit.
 * A row short of several resources counts once in rows_no_capacity and once
 * in each rows_insufficient[r]. rows_occupied (rows covered by another
 * exclusive job) does not depend on the class and is repeated in every record.
 * The domains are those of the class's level, classified by the engine's own
 * capsum / occsum (the sums of jsp_place's tally_out / occ_out over a domain's
 * leaves): domains == dom_occupied + dom_short + dom_feasible, and
 * dom_feasible is the popcount of the class's feasibility bitmap.
 * best_short_cap is the largest capsum among the dom_short domains (0 when
 * there are none), best_short_domain the lowest id that attains it (-1). */
typedef struct jsp_class_explain {
    uint64_t rows, rows_selector, rows_taint, rows_no_capacity;
    uint64_t rows_insufficient[JSP_MAX_RES];
    uint64_t rows_fit, rows_occupied;
    uint32_t domains, dom_occupied, dom_short, dom_feasible;
    uint32_t best_short_cap;
    int32_t best_short_domain;
} jsp_class_explain;                       /* 104 bytes */

/* out[n_classes], n_classes == the count given to jsp_classes_upload. Host
 * buffers; runs on the engine's stream (ordered after every pending patch,
 * those posted to the resident service's dispatcher included) and returns
 * when done. The resident service, when up, stays up and keeps its tiles: a
 * jsp_place after it is answered as before. JSP_EINVAL: NULL engine, NULL out,
 * wrong n_classes; JSP_ESTATE: no topology, snapshot or classes yet. On a
 * device-set engine every shard counts its rows on its device and the
 * domains are classified on device_ids[0] over the combined tallies: the
 * records equal a single-device engine's.
 * Added within ABI v7 (JSP_ABI_VERSION is unchanged: nothing existing moved);
 * a caller that may meet an older library detects it by symbol (dlsym). */
int jsp_explain(jsp_engine* e, jsp_class_explain* out, uint32_t n_classes);

/* ---- resident service, metrics, synchronisation ---- */
int jsp_engine_set_service(jsp_engine* e, int mode);
/* Stops the resident service (if running) and waits (bounded: 2 s, then
 * JSP_EHIP and the service stays off until the next upload) for its
 * workgroups to leave. */
int jsp_engine_service_stop(jsp_engine* e);
/* The engine's metrics since creation or the last reset (jsp_metrics). */
int jsp_engine_get_metrics(jsp_engine* e, jsp_metrics* out, int reset);
/* The engine's own stream (a caller may pass it to the *_device calls). */
void* jsp_engine_stream(jsp_engine* e);
/* Waits for every patch and launch the engine has issued. */
int jsp_engine_sync(jsp_engine* e);
/* Waits for every launch the engine has enqueued (on any stream) and returns
 * JSP_EHIP if one of them failed on the device (see "Kernel-side failures"). */
int jsp_engine_check(jsp_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* JSPLACE_H */
