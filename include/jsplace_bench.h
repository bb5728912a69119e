/*
 * jsplace_bench.h -- the measurement and diagnostic symbol set of
 * libjsplace.so (prefix jspb_, ABI v7). Not part of the product boundary
 * (include/jsplace.h): no Go caller binds these. bench.py, the GPU tests and
 * the probes under tools/ use them to time the product entry points from C
 * (no interpreter between calls), to time kernels by events on their own
 * dispatch packets, to read the resident service's device stamps, and to
 * force a launch shape.
 */
#ifndef JSPLACE_BENCH_H
#define JSPLACE_BENCH_H

#include "jsplace.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Phase clocks of the engine's calls (sums since the last reset). The host
 * phases are always accumulated; the device ones (HIP events, service
 * stamps) only while jspb_set_timing(e, 1).
 * A jsp_place answered at once under the host lease (nothing to settle, no
 * patch pending) reads the clock twice, at entry and at exit, and has no
 * phases: its wall (entry -> exit, inside the library) goes to host_wait_us
 * and to svc_answer_us, nothing to host_prep_us / svc_pre_us / svc_first_us;
 * host_calls and svc_calls count it. (host_prep_us + host_wait_us) /
 * host_calls stays the call's wall. Calls that cross the link, and a leased
 * answer that first had a request to settle or a carried patch to book (a
 * recovery's place), keep every phase. */
typedef struct jsp_timing {
    uint64_t calls;            /* timed placements (or tallies) since last reset */
    double tally_ms;           /* summed HIP-event time of the tally kernel */
    double feas_ms;            /* summed HIP-event time of the feasibility-bitmap kernel */
    double assign_ms;          /* summed HIP-event time of the assignment kernel */
    double fused_ms;           /* summed HIP-event time of single-launch placements (fused / compaction) */
    uint64_t fused_calls;      /* placements that ran as a single launch */
    /* host-API placements (jsp_place), host wall clock, always accumulated */
    uint64_t host_calls;
    double host_prep_us;       /* entry to launch: checks, run list into the pinned staging buffer */
    double host_launch_us;     /* the kernel launch call(s) */
    double host_wait_us;       /* launch return to completion seen (completion words or stream sync) */
    double host_post_us;       /* assign[] (and tallies) out, stats; the split service: its host walk (inside wait) */
    /* resident service (jsp_engine_set_service) */
    uint64_t svc_calls;        /* jsp_place calls it answered */
    uint64_t svc_starts;       /* service launches (first use, after uploads, idle exits, restarts) */
    double svc_us;             /* summed in-kernel request time (first tile saw the request -> last tile
                                  done, 100 MHz device clock); accumulated while timing is on */
    uint64_t svc_fallbacks;    /* jsp_place calls the service could not answer (its grid does not fit the
                                  CUs, it left twice, or a request failed on the device): answered by the
                                  launch path instead. When its grid cannot be co-resident the service stays
                                  off until the next upload; otherwise the next call starts it again */
    double svc_ready_us;       /* host time spent waiting for a (re)started service's dispatcher to poll */
    double svc_pre_us;         /* service-answered jsp_place: entry of the service path to the request post
                                  (a queued wake, settling the previous request, patch bookkeeping) (ABI v6) */
    double svc_answer_us;      /* ... the request post to the answer's last entry seen (ABI v6) */
    double svc_first_us;       /* ... the request post to its first answer entry seen (compaction service) */
    /* jsp_snapshot_patch (ABI v5), host wall clock, always accumulated */
    uint64_t patches;          /* patch calls with at least one row */
    double patch_us;           /* their host time (a waker-thread restart is not in it) */
    double wake_us;            /* host time (re)starting the service for a coming recovery, wherever it ran */
    /* the split tiles launched for one request (stats.fused 8, ABI v7), host wall clock */
    uint64_t oneshot_calls;
    double oneshot_launch_us;  /* entry to the launch's return */
    double oneshot_wait_us;    /* ... to every tile's lines seen */
    double oneshot_walk_us;    /* ... the host walk and (device paths) the assign[] copy launch */
    double oneshot_stage_us;   /* the part of oneshot_launch_us before the launch call (staging slot, set-up) */
} jsp_timing;

/* jspb_set_fused modes: which launch shape the launch path takes */
#define JSP_FUSED_OFF 0       /* always tally -> feas -> assign (three launches) */
#define JSP_FUSED_AUTO 1      /* one launch when possible (default): the single-class compaction
                                 for one leaf-level class, the fused tail for small snapshots */

/* ---- C-timed loops of the product calls ---- */
/* `iters` jsp_place calls back to back, timed in C (ABI v6): what a cgo
 * caller's loop sees, with no interpreter between the calls (the bench's
 * host-API steps). With n_patch > 0, each call is preceded by a one-row
 * jsp_snapshot_patch of the taint column (row patch_rows[i % n_patch] set to
 * patch_taints[i % n_patch]: a watch event between recoveries). out_us[0]
 * total wall, [1] median and [2] p99 per step, microseconds; assign_out holds
 * the last call's answer. */
int jspb_place_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                   int32_t* assign_out, uint32_t iters, const uint32_t* patch_rows, const uint32_t* patch_taints,
                   uint32_t n_patch, double* out_us);
/* `iters` jsp_place_sticky calls back to back with the same prev_assign,
 * timed in C as jspb_place_loop times jsp_place: out_us[0] total wall, [1]
 * median and [2] p99 per call, microseconds; assign_out holds the last call's
 * answer. */
int jspb_place_sticky_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                          const int32_t* prev_assign, int32_t* assign_out, uint32_t iters, double* out_us);
/* `iters` jsp_place_gangs calls back to back with the same gangs, timed in C
 * the same way: out_us[0] total wall, [1] median and [2] p99 per call,
 * microseconds; assign_out and gang_span_out (nullable) hold the last call's
 * answer. */
int jspb_place_gangs_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                          const uint32_t* gang_runs, const uint32_t* gang_span, uint32_t n_gangs, int32_t* assign_out,
                          int32_t* gang_span_out, uint32_t iters, double* out_us);
/* jsp_place_gangs' span counts alone (DESIGN.md section 4 "Gang placement"):
 * the tally and the feasibility words on the current snapshot, then the
 * counts. For class c at level lc, every level s <= lc and every level-s
 * domain S, the set feasibility bits of c among the level-lc domains of S
 * (S's child range followed down to lc). Class c's counts follow those of
 * the classes before it, level s's the domains of the levels before s:
 * cnt_out[sum over c' < c of (D[0] + .. + D[level[c']]) + D[0] + .. + D[s-1]
 * + S]; n_cnt is their total and must match. form 0: the launch form per
 * (c, s) as jsp_place_gangs picks it; 1: one thread per S everywhere; 2: one
 * wave per S everywhere. iters > 0: out_us[0] median and [1] mean device time
 * of the count launches alone over `iters` (<= 4096) repetitions (events on
 * the dispatches, as jspb_tally_device_timed). JSP_ESTATE on a device-set or
 * sharded engine. The resident service is not touched. */
int jspb_span_counts(jsp_engine* e, int form, uint32_t* cnt_out, uint32_t n_cnt, uint32_t iters, double* out_us);
/* `iters` jsp_place_fit calls back to back with the same runs and policy,
 * timed in C the same way: out_us[0] total wall, [1] median and [2] p99 per
 * call, microseconds; assign_out holds the last call's answer. */
int jspb_place_fit_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                        uint32_t policy, int32_t* assign_out, uint32_t iters, double* out_us);
/* jsp_place_fit's order lists alone (DESIGN.md section 4 "Fit placement"):
 * the tally and the feasibility words on the current snapshot, then the order
 * step. Class c's segment starts at the sum over c' < c of D[level[c']] and
 * holds D[level[c]] entries: its nf_out[c] feasible domains in ascending
 * (key, id) under `policy`, then 0xFFFFFFFF; n_order is the segments' total
 * and must match, nf_out takes one count per class. form 0: the order form
 * per class as jsp_place_fit picks it; 1: the rank form everywhere; 2: the
 * block form everywhere (its block from the fit_block test hook, else the
 * engine's). iters > 0: out_us[0] median and [1] mean device time of the order
 * launches alone over `iters` (<= 4096) repetitions (events on the dispatches,
 * as jspb_span_counts). JSP_ESTATE on a device-set or sharded engine. The
 * resident service is not touched. */
int jspb_fit_order(jsp_engine* e, uint32_t policy, int form, uint32_t* order_out, uint32_t n_order, uint32_t* nf_out,
                   uint32_t iters, double* out_us);
/* `iters` jsp_place_whatif calls back to back with the same runs and
 * scenarios, timed in C the same way: out_us[0] total wall, [1] median and
 * [2] p99 per call, microseconds; assign_out ([S][J]) holds the last call's
 * answer. */
int jspb_place_whatif_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                           const uint32_t* scen_off, uint32_t n_scen, const uint32_t* rows, const uint64_t* labels,
                           const uint32_t* taints, const uint32_t* free_res, const int32_t* excl_owner,
                           int32_t* assign_out, uint32_t iters, double* out_us);
/* `iters` jsp_place_preempt calls back to back with the same arguments, timed
 * in C the same way: out_us[0] total wall, [1] median and [2] p99 per call,
 * microseconds; assign_out, victim_off_out, victims_out and stats (nullable as
 * in jsp_place_preempt) hold the last call's. */
int jspb_place_preempt_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                            uint32_t prio, const int32_t* owner_ids, const uint32_t* owner_prio, uint32_t n_owners,
                            const uint32_t* evict_free, int32_t* assign_out, uint32_t* victim_off_out,
                            int32_t* victims_out, uint32_t victims_cap, jsp_preempt_stats* stats, uint32_t iters,
                            double* out_us);
/* jsp_place_preempt's candidate lists alone (DESIGN.md section 4 "Preemptive
 * placement"): the row and leaf passes, cap', the keys and the order step on
 * the current snapshot, without the walk and the gather. The segments are laid
 * out as jspb_fit_order's: order_out holds class c's nf_out[c] reachable
 * domains in ascending (key, id), then 0xFFFFFFFF; key_out and seg_out hold
 * key(c, d) and seg(d) by domain id for every domain of the segment, reachable
 * or not (hp counts victim rows only). n_order is the segments' total and must
 * match. form as jspb_fit_order's (the fit_form / fit_block test hooks apply).
 * iters > 0: out_us[0] median and [1] mean device time of those launches over
 * `iters` (<= 4096) repetitions (events on the dispatches), the staging copy
 * not included. The table and prio are checked as jsp_place_preempt checks
 * them. JSP_ESTATE on a device-set or sharded engine. The resident service is
 * not touched. */
int jspb_preempt_order(jsp_engine* e, uint32_t prio, const int32_t* owner_ids, const uint32_t* owner_prio,
                       uint32_t n_owners, const uint32_t* evict_free /* nullable, [R][N] */, int form,
                       uint32_t* order_out, uint32_t n_order, uint32_t* nf_out, uint32_t* key_out, uint32_t* seg_out,
                       uint32_t iters, double* out_us);
/* `iters` jsp_place_spread calls back to back with the same arguments, timed
 * in C the same way: out_us[0] total wall, [1] median and [2] p99 per call,
 * microseconds, and [3] the median host walk inside a call; assign_out,
 * spread_out, count_out and stats (nullable as in jsp_place_spread) hold the
 * last call's. */
int jspb_place_spread_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                           uint32_t spread_level, uint32_t max_skew, const int32_t* peer_ids, uint32_t n_peers,
                           int32_t* assign_out, int32_t* spread_out, uint32_t* count_out, jsp_spread_stats* stats,
                           uint32_t iters, double* out_us /* [4] */);
/* jsp_place_spread's tables alone (DESIGN.md section 4 "Spread placement"):
 * tally, feasibility and fits words, the peer passes and the span counts on
 * the current snapshot, without the walk. fits_out [n_words] holds the fits
 * words in the feasibility words' layout (class c's (D[level[c]] + 63) / 64
 * words behind those of the classes before it; n_words is their total and must
 * match), feas_out (nullable) the feasibility words beside them; peers_out
 * [D_s] is peers(S); cnt_feas_out and cnt_fits_out [C][D_s] (nullable) are the
 * span counts of the two kinds of words, row c zero for a class finer than the
 * spread level. form 0: each class's span-count form by its mean segment, as
 * the call picks it; 1 / 2: every class in the thread / the wave form. shift
 * < 0: the leaf pass's lanes per leaf as the call picks them, else 1 << shift
 * (0..6). iters > 0: out_us[0] median and [1] mean device time of the
 * launches behind the tally and the feasibility words over `iters` (<= 4096)
 * repetitions. The peer table is checked as jsp_place_spread checks it.
 * JSP_ESTATE on a device-set or sharded engine. The resident service is not
 * touched. */
int jspb_spread_tables(jsp_engine* e, uint32_t spread_level, const int32_t* peer_ids, uint32_t n_peers, int form,
                       int shift, uint64_t* fits_out, uint64_t* feas_out, uint32_t n_words, uint32_t* peers_out,
                       uint32_t* cnt_feas_out, uint32_t* cnt_fits_out, uint32_t iters, double* out_us);
/* `iters` jsp_bind_pods calls back to back with the same assign, timed in C
 * the same way: out_us[0] total wall, [1] median and [2] p99 per call,
 * microseconds; pod_row_out and stats (nullable) hold the last call's. */
int jspb_bind_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                   const int32_t* assign, int32_t* pod_row_out, jsp_bind_stats* stats, uint32_t iters, double* out_us);
/* `iters` times one jsp_assume followed by the jsp_forget of the owners of its
 * placed jobs (at most JSP_FORGET_MAX_OWNERS jobs), so every iteration sees
 * the same snapshot; each half timed in C. out_us[0] median and [1] p99 of
 * jsp_assume, [2] median and [3] p99 of jsp_forget, microseconds; stats and
 * rows_cleared_out (both nullable) hold the last iteration's. */
int jspb_assume_forget_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                            const int32_t* assign, const int32_t* owner, uint32_t iters, jsp_assume_stats* stats,
                            uint64_t* rows_cleared_out, double* out_us);
/* The realistic recovery timed in C (ABI v6), `trials` times: the idle period
 * (idle_us, slept -- or spun when spin != 0), a one-row taint patch
 * (patch_rows[t % n_patch] := patch_taints[t % n_patch]; the failed job's
 * node back to schedulable), the gap (gap_us: the reconciler's round trips
 * between the deletions and the recreate), then jsp_place. out_us[3t] = the
 * patch call, [3t+1] = the place call, [3t+2] = the gap as it passed (us). */
int jspb_recovery_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                      int32_t* assign_out, uint32_t trials, double idle_us, double gap_us, int spin,
                      const uint32_t* patch_rows, const uint32_t* patch_taints, uint32_t n_patch, double* out_us);
/* ---- shapes, device timing, clocks ---- */
int jspb_set_fused(jsp_engine* e, int mode);
/* With timing on: the last service request's 100 MHz device-clock stamps, 8
 * per tile (0 request seen, 1 after the acquire, 2 tallied, 3 feasible count
 * scanned, 4 look-back done, 5 assign[] drained; 6-7 unused). Copies up to
 * cap/8 tiles; *n_tiles = how many (0 when no timed request is held). When
 * cap leaves room for one more row after all the tiles, it receives the
 * dispatcher's {0 request seen in the mailbox, 1 bell rung} (ABI v6). */
int jspb_service_clock(jsp_engine* e, uint32_t* out, uint32_t cap, uint32_t* n_tiles);
/* Totals of the resident service that left last (its dispatcher writes them
 * once, on a stop or an idle exit; stop the service first -- JSP_ESTATE while
 * one runs): out[0] its tiles, out[1] requests its dispatcher answered itself
 * from the tiles' standing lines, out[2] requests without a patch that it
 * handed to the tiles, out[3] evaluate-rings (its first ring, dirty rings,
 * micro-patch rings). Zeros before any service has left. */
int jspb_service_counters(jsp_engine* e, uint64_t out[4]);
/* The host lease of the compaction service: while
 * nothing has changed the rows, the classes, the topology or the service
 * since the last request that crossed the link, jsp_place expands the lines
 * of that request's answer on the host and posts nothing. out[0] placements
 * answered on the host, out[1] leases taken (the first host answer after a
 * request that crossed the link), out[2] leases dropped (a change, a stop, a
 * line that was not whole). Counted since engine creation or the last reset;
 * out may be NULL with reset != 0. Readable while the service runs. */
int jspb_lease_counters(jsp_engine* e, uint64_t out[3], int reset);
/* The expansion of a bitmap answer, a pure host function (no engine, no GPU):
 * `lines` holds n_tiles lines of 8 words, tile t's leaves' feasibility as four
 * 64-leaf words, each as two halves (seq << 32 | 32 bits), low half first;
 * l0[t] is tile t's first leaf and base the snapshot's. Job j gets the j-th
 * feasible leaf in tile order, out[j] = base + l0[t] + bit index. Returns 0
 * when the answer is complete: J jobs have a leaf or every line was taken,
 * out[*placed..J) = -1. Returns 1 when a line it needed has a half with
 * another tag: *placed = the jobs placed from the whole lines before it, and
 * out[] past them is not written. */
int jspb_expand_lines(const uint64_t* lines, uint32_t n_tiles, const uint32_t* l0, uint32_t base, uint32_t seq,
                      uint32_t J, int32_t* out, uint32_t* placed);
/* Whether all 8 * n_tiles halves of the first n_tiles lines carry seq (1) or
 * not (0): the check the lease's kept list makes on every answer. A pure host
 * function. */
int jspb_lines_tagged(const uint64_t* lines, uint32_t n_tiles, uint32_t seq);
/* The answer for J jobs from a kept list of n_list feasible leaves in answer
 * order (what jspb_expand_lines gives for J >= n_list): out[j] = list[j] for
 * j < min(J, n_list), -1 up to J, *placed = min(J, n_list). Never writes
 * out[J] or beyond. A pure host function. */
int jspb_list_answer(const int32_t* list, uint32_t n_list, uint32_t J, int32_t* out, uint32_t* placed);
/* The lease's kept list: from the second host answer
 * of a lease on, the answer is copied from the list of feasible leaves the
 * lines expand to, decoded once. out[0] host answers copied from a kept list
 * (the call that built it included), out[1] lists built. Both stay 0 under the
 * test hook lease_memo=0. Counted and reset as jspb_lease_counters. */
int jspb_lease_memo_counters(jsp_engine* e, uint64_t out[2], int reset);
/* The entry stamps' clock: n pairs out[2i] = the
 * clock jsp_place stamps its entry with, out[2i + 1] = steady_clock at the
 * same moment (the middle of two reads around the first; a pair whose reads
 * lie more than 2 us apart is taken again), both in nanoseconds since
 * steady_clock's epoch; out[2n] = 1 when the first is read off the TSC, 0 when
 * it is steady_clock itself (no invariant TSC, the kernel keeps time by
 * another source, or the test hook fast_clock=0, read at this call). out holds
 * 2n + 1 values. Takes the clock's once-per-process calibration (10 ms) when
 * no engine has. No engine, no GPU. */
int jspb_fast_clock_probe(uint32_t n, int64_t* out);
/* jsp_engine_get_metrics called back to back for `seconds` (0 < seconds <= 10)
 * and timed in C, for a metrics scrape beside placing threads: out[0] scrapes
 * made, out[1] the longest one in nanoseconds, out[2] scrapes whose
 * place_us.count was below the previous scrape's, out[3] the last scrape's
 * place_us.count. A scrape takes the metrics' lock only: it never waits for a
 * placement that holds the engine's across a GPU round trip. */
int jspb_scrape_loop(jsp_engine* e, double seconds, uint64_t out[4]);
/* The timing loops' order statistics (jspb_place_loop and the others'
 * out_us[1], out_us[2]): of n >= 1 durations in integer nanoseconds, out[0] =
 * the median and out[1] = the p99 in microseconds -- bit for bit the values at
 * ranks n / 2 and min(n - 1, (size_t)(0.99 n)) of the sorted samples converted
 * to microseconds (ns / 1000.0), selected without sorting them. A pure host
 * function. */
int jspb_select_median_p99(const int64_t* samples_ns, uint32_t n, double out[2]);
/* Device time of `iters` back-to-back steps on the engine stream (the bench's
 * kernel-time legs): each step carries a start event on its first dispatch and
 * a stop event on its last (hipExtLaunchKernel: the dispatch packets' own
 * timestamps, as a kernel trace reports them, with no host submit time between
 * them). d_scrub (nullable): a device buffer larger than the caches, read
 * (never written) before every step, so each step starts cold.
 * out_us[0] = median, out_us[1] = mean per step, in microseconds.
 * jspb_tally_device_timed: the tally of jsp_tally_device.
 * jspb_place_device_timed: the whole placement of jsp_place_device. */
int jspb_tally_device_timed(jsp_engine* e, uint32_t* d_cap, uint32_t* d_occ, uint32_t ld, uint32_t iters,
                           const void* d_scrub, size_t scrub_bytes, double* out_us);
int jspb_place_device_timed(jsp_engine* e, const uint32_t* d_run_class, const uint32_t* d_run_len, uint32_t n_runs,
                           uint32_t n_jobs, int32_t* d_assign, uint32_t iters, const void* d_scrub,
                           size_t scrub_bytes, double* out_us);
/* The host-link floor (ABI v6): `iters` host -> device -> host round trips
 * through pinned memory with the resident service's polling (four device
 * waves a quarter of a round trip apart poll a request word; the first to
 * see request i writes an ack the host spins on). out_us[0] median, [1]
 * p99, [2] mean, microseconds. Every host-API request pays this at least
 * once; the bench reports it beside the host-API latency. */
int jspb_link_floor(jsp_engine* e, uint32_t iters, double* out_us);
/* The tally's in-kernel span (ABI v6): `iters` back-to-back launches of the
 * one-tile wave tally with per-wave stamps of the device's 100 MHz clock
 * (every wave's start, and its end once its stores drained); per launch the
 * span from the first wave's start to the last wave's end -- a third measure
 * beside the dispatch-packet events and a kernel trace, with no tracer and no
 * dispatch overhead in it. out_us[0] median, [1] mean; out_us[2] the median
 * dispatch-event time of an empty one-workgroup launch (the fixed cost events
 * on the dispatch packets add to a kernel's own span); out_us[3] the launches'
 * period by the same clock (first wave of the first launch to first wave of
 * the last, per launch: execution plus the gap dispatch leaves between
 * back-to-back launches). JSP_ESTATE when the snapshot's tally runs another
 * shape. */
int jspb_tally_device_spans(jsp_engine* e, uint32_t* d_cap, uint32_t* d_occ, uint32_t ld, uint32_t iters,
                           double* out_us);
/* jsp_explain's row pass beside the tally, which streams the same columns:
 * after a warm-up of 10 launches each, one HIP event pair around `iters`
 * (1..4096) back-to-back launches of explain_rows_kernel, then the same
 * around `iters` tallies into the engine's own buffers (what jsp_tally_device
 * launches). out_us[0] = the row pass, out_us[1] = the tally: elapsed / iters,
 * microseconds per launch. The resident service is not touched. */
int jspb_explain_rows_loop(jsp_engine* e, uint32_t iters, double* out_us);
/* jsp_bind_pods' launches beside the tally, on the device: the launches of
 * the last successful jsp_bind_pods call on this snapshot (its staging is
 * still in place) are repeated. After a warm-up of 10 each, one HIP event
 * pair around `iters` (1..4096) repetitions of: [0] the call's whole stream
 * work (the tables' fill, the claim launch, the bind launches), [1] the bind
 * launches alone (the tables keep the last claims: the same answer), [2] the
 * tally into the engine's own buffers. Elapsed / iters, microseconds.
 * JSP_ESTATE when no such call preceded. The resident service is not touched. */
int jspb_bind_kernel_loop(jsp_engine* e, uint32_t iters, double* out_us);
int jspb_set_timing(jsp_engine* e, int enable);
int jspb_get_timing(jsp_engine* e, jsp_timing* out, int reset);

/* ---- which path answered ---- */
/* The launch plan of the engine's last placement, tally or assignment: what
 * the host decided where it issued the launches (DESIGN.md section 4
 * "Launch-shape thresholds and their tests"). Written on the launch paths
 * and at a resident service's start only; a call the service (or its lease)
 * answered reports the plan of that service's start. Fields that a path does
 * not use are 0. jsp_tally_device starts a plan of its own (shape 0,
 * JSPB_WALK_NONE); a jsp_assign_device behind it adds the walk to it. */
#define JSPB_TALLY_IN_TILE 0   /* no tally launch: the single-launch shapes tally inside their tiles */
#define JSPB_TALLY_WAVE_ONE 1  /* wave tiles, one tile per wave (one register set) */
#define JSPB_TALLY_WAVE_DB 2   /* wave tiles taken in turn, double-buffered */
#define JSPB_TALLY_BLOCK 3     /* workgroup row blocks */
#define JSPB_WALK_NONE 0       /* no walk yet (a tally alone) */
#define JSPB_WALK_LEVEL 1      /* assign_level_kernel<level_wpt, level_threads> */
#define JSPB_WALK_ASSIGN 2     /* assign_kernel + expand_kernel */
#define JSPB_WALK_FUSED_TAIL 3 /* the fused launch's last workgroup */
#define JSPB_WALK_COMPACT 4    /* one leaf-level class: the compaction's look-back (launch or service) */
#define JSPB_WALK_HOST 5       /* the host walk over the GPU's feasibility words (shape 7) */
#define JSPB_WALK_SPLIT_HOST 6 /* the host walk over the split tiles' lines (shape 8, the split service) */
typedef struct jspb_plan {
    uint32_t shape;          /* as jsp_stats.fused */
    uint32_t tally;          /* JSPB_TALLY_* */
    uint32_t tally_passes;   /* tally launches (16 classes each); 0 with JSPB_TALLY_IN_TILE */
    uint32_t folded;         /* the wave tally set the feasibility words itself (no feasibility launch) */
    uint32_t walker;         /* JSPB_WALK_* */
    uint32_t level_wpt;      /* JSPB_WALK_LEVEL: bitmap words per thread */
    uint32_t level_threads;  /* JSPB_WALK_LEVEL: threads of the walker's workgroup */
    uint32_t feas_in_lds;    /* JSPB_WALK_ASSIGN: the feasibility words staged in LDS */
    uint32_t topo_in_lds;    /* JSPB_WALK_ASSIGN / FUSED_TAIL: the hierarchy tables staged in LDS */
    uint32_t stage_cap;      /* JSPB_WALK_ASSIGN: ranks staged per long-run step */
    uint32_t fscr_words;     /* JSPB_WALK_FUSED_TAIL: upper-level scratch words in LDS (0: none) */
    uint32_t groups;         /* class groups of the fused / split tiles (1 elsewhere) */
    uint32_t cpg;            /* classes per group */
    uint32_t n_blocks;       /* tally row blocks of the snapshot */
    uint32_t n_wtiles;       /* its wave tiles (0: a leaf exceeds a wave tile) */
} jspb_plan;
int jspb_last_plan(jsp_engine* e, jspb_plan* out);


#ifdef __cplusplus
}
#endif
#endif /* JSPLACE_BENCH_H */
