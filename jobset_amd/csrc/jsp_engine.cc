// jsp_engine.cc — host side of the exclusive-topology placement engine:
// the C ABI of include/jsplace.h over HIP device buffers and the kernels of
// jsp_kernels.hip. See DESIGN.md for the data layout and the rules.
#include <emmintrin.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/jsplace_bench.h"
#include "jsp_clock.h"
#include "jsp_internal.h"
#include "jsp_leased_metrics.h"
#include "jsp_lines.h"
#include "jsp_multi.h"
#include "jsp_select.h"
#include "jsp_wait.h"
#include "jsp_walk.h"

namespace {

thread_local std::string g_err;

int set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// One value into a log2 histogram (jsplace.h jsp_hist): bucket 0 below lo,
// bucket i in [lo 2^(i-1), lo 2^i), the last one the rest.
void hist_add(jsp_hist& h, double v, double lo) {
    h.count += 1;
    h.sum += v;
    if (v > h.max) h.max = v;
    h.bucket[hist_bucket(v, lo)] += 1;
}

// Microseconds from t0 to t1 (left out: to now).
double us_between(std::chrono::steady_clock::time_point t0,
                  std::chrono::steady_clock::time_point t1 = std::chrono::steady_clock::now()) {
    return std::chrono::duration<double, std::micro>(t1 - t0).count();
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return set_err(JSP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),  \
                           __FILE__, __LINE__);                                              \
    } while (0)

// Buffers a grow-only buffer gave up while the resident service ran: hipFree
// and hipHostFree wait for every kernel on the device, the resident service
// included, which leaves only after JSP_SERVICE_IDLE_MS without a request --
// a free while it runs stalls the caller for up to that long
// (tools/block_probe.hip). They are freed once the service has stopped.
struct Grave {
    std::vector<void*> dev, host;
    void flush() {
        for (void* p : dev) (void)hipFree(p);
        for (void* p : host) (void)hipHostFree(p);
        dev.clear();
        host.clear();
    }
    ~Grave() { flush(); }
};

// Grow-only device buffer. `g`: where the old buffer goes when it must grow
// while a kernel that never ends by itself runs (nullptr: freed at once).
// The calling thread's current device, restored when an entry point that
// switches devices returns (the device-set engine walks its devices; a
// caller -- a torch rank, a Go thread -- keeps the device it had).
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { (void)hipGetDevice(&prev); }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t reserve(size_t n, Grave* g = nullptr) {
        if (n <= bytes && p) return hipSuccess;
        if (g && p) {
            g->dev.push_back(p);
            p = nullptr;
            bytes = 0;
        }
        release();
        hipError_t e = hipMalloc(&p, n ? n : 16);
        if (e == hipSuccess) bytes = n ? n : 16;
        return e;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// Pinned, device-mapped host memory: the host placement path hands run lists
// to the kernels and takes assign[] back through it without DMA copies
// (kernels read and write it over the host link directly).
struct HostBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~HostBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t reserve(size_t n, Grave* g = nullptr) {
        if (n <= bytes && p) return hipSuccess;
        if (g && p) {
            g->host.push_back(p);
            p = nullptr;
            bytes = 0;
        }
        release();
        hipError_t e = hipHostMalloc(&p, n ? n : 16, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) bytes = n ? n : 16;
        return e;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

struct EvPair {
    hipEvent_t a = nullptr, b = nullptr;
    int tag = 0;  // 0 tally, 1 feas, 2 assign, 3 fused
};

// Test hooks: JSP_TEST_HOOKS="name=value,...", read at engine creation and
// again at each snapshot upload. They force, at test sizes, the shapes the
// engine otherwise picks only for large geometries (the double-buffered and
// workgroup tallies, multi-chunk tally blocks), shorten the kernels' bounded
// waits so that their error path runs, and stand in for a smaller GPU. Every
// hook but waker_poll_us (kept for pricing the armed waker: 0 turns its polling
// off) is one that a test sets; finished experiments' hooks do not stay. The
// library's other environment switches are operational only: JSP_SERVICE,
// JSP_SERVICE_IDLE_MS and (device sets) JSP_RCCL_LIB.
struct TestHooks {
    bool tally_one = true;          // tally_one=0: the double-buffered wave tally at any size
    bool tally_block = false;       // tally_block=1: the workgroup tally instead of the wave tiles
    uint32_t block_chunks = 1;      // block_chunks=N (1..8): 1024-row chunks per tally workgroup
    uint32_t block_rows = 0;        // block_rows=N (>= 60): smaller tally row blocks (more tiles)
    uint32_t lookback_spins = 1u << 22;  // lookback_spins=N: compaction look-back polls before giving up
    uint32_t pipe_spins = 1u << 24;      // pipe_spins=N: the pipelined batch walk's polls of an earlier batch
    uint64_t wait_ticks = 200000000ull;  // wait_us=N: the level walk's expanders' wait (100 MHz ticks; 2 s)
    int cu_limit = 0;               // cu_limit=N: CUs the resident service may count on
    bool svc_xcd = true;            // svc_xcd=0: the compaction service spread over the XCDs (the
                                    //   write-through protocol a partition mode would run)
    uint32_t seq0 = 0;              // seq0=N: the service's first request number
    bool have_seq0 = false;
    bool svc_entries = false;       // svc_entries=1: the compaction service answers with per-job entries
                                    //   after a look-back instead of tile bitmaps (A/B)
    uint32_t micro_spins = 1u << 22;  // micro_spins=N: a resident tile's passes over the microbox (kErrMicro)
    uint32_t svc_standing = 3;      // svc_standing=N: 0 every service request evaluates, 1 a resident tile answers
                                    //   from its last evaluation, 2 and the dispatcher from the tiles' standing lines,
                                    //   3 and the host from the last answer's lines while nothing changed (the lease)
    bool lease_memo = true;         // lease_memo=0: every host answer under the lease expands the lines (A/B)
    bool fast_clock = true;         // fast_clock=0: jsp_place / jsp_snapshot_patch stamp with steady_clock (A/B)
    uint32_t waker_poll_us = 200;   // waker_poll_us=N: the armed waker's poll period; 0 = condition variable only
    bool sticky_grid = false;       // sticky_grid=1: jsp_place_sticky's grid keep form at any job count
    bool bind_wg = false;           // bind_wg=1: jsp_bind_pods' workgroup form for every job
    uint32_t fit_form = 0;          // fit_form=1|2: jsp_place_fit's rank / block order form at any segment size
    uint32_t fit_block = 0;         // fit_block=N (a power of two, 64..4096): keys per block of the block form
};

TestHooks read_hooks() {
    TestHooks h;
    const char* s = std::getenv("JSP_TEST_HOOKS");
    if (!s) return h;
    std::string all(s);
    size_t p = 0;
    while (p < all.size()) {
        size_t q = all.find(',', p);
        if (q == std::string::npos) q = all.size();
        const std::string kv = all.substr(p, q - p);
        p = q + 1;
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) continue;
        const std::string k = kv.substr(0, eq);
        const unsigned long long v = std::strtoull(kv.c_str() + eq + 1, nullptr, 0);
        if (k == "tally_one") h.tally_one = v != 0;
        else if (k == "tally_block") h.tally_block = v != 0;
        else if (k == "block_chunks" && v >= 1 && v <= 8) h.block_chunks = (uint32_t)v;
        else if (k == "block_rows" && v >= 60) h.block_rows = (uint32_t)v;
        else if (k == "lookback_spins") h.lookback_spins = (uint32_t)v;
        else if (k == "pipe_spins") h.pipe_spins = (uint32_t)v;
        else if (k == "wait_us") h.wait_ticks = v * 100ull;
        else if (k == "cu_limit") h.cu_limit = (int)v;
        else if (k == "svc_xcd") h.svc_xcd = v != 0;
        else if (k == "svc_entries") h.svc_entries = v != 0;
        else if (k == "micro_spins") h.micro_spins = (uint32_t)v;
        else if (k == "svc_standing" && v <= 3) h.svc_standing = (uint32_t)v;
        else if (k == "lease_memo") h.lease_memo = v != 0;
        else if (k == "fast_clock") h.fast_clock = v != 0;
        else if (k == "waker_poll_us") h.waker_poll_us = (uint32_t)v;
        else if (k == "sticky_grid") h.sticky_grid = v != 0;
        else if (k == "bind_wg") h.bind_wg = v != 0;
        else if (k == "fit_form" && v <= 2) h.fit_form = (uint32_t)v;
        else if (k == "fit_block" && v >= 64 && v <= jsp::kFitBlockMax && (v & (v - 1)) == 0) h.fit_block = (uint32_t)v;
        else if (k == "seq0") {
            h.seq0 = (uint32_t)v;
            h.have_seq0 = true;
        }
    }
    return h;
}

}  // namespace

int jsp_internal_set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

struct jsp_engine {
    int device = 0;
    jspm::Multi* multi = nullptr;  // a device-set engine (jsp_engine_create_multi): every call goes there
    int n_cu = 0;  // compute units (multiProcessorCount)
    hipStream_t stream = nullptr;
    std::mutex mu;

    // topology
    bool have_topo = false;
    uint32_t K = 0;
    uint32_t D[JSP_MAX_LEVELS] = {0, 0, 0, 0};
    uint32_t L_total = 0;
    DevBuf fl[JSP_MAX_LEVELS], cs[JSP_MAX_LEVELS], par[JSP_MAX_LEVELS];
    uint32_t t_off_h[JSP_MAX_LEVELS + 1] = {0, 0, 0, 0, 0};
    DevBuf t_off;
    jsp::TopoDev topo{};
    // host copies of the hierarchy tables (the split service's host walk)
    std::vector<uint32_t> h_fl[JSP_MAX_LEVELS], h_cs[JSP_MAX_LEVELS];
    std::vector<int32_t> h_par[JSP_MAX_LEVELS];
    std::vector<uint32_t> blk_l0, blk_l1;  // leaf range of each tally row block
    uint32_t max_blk_span = 0;             // rows a tally block's first chunk spans, max over blocks
    TestHooks hooks;                       // JSP_TEST_HOOKS (tests only; defaults otherwise)
    jsp::HostWalk walk;

    // snapshot
    bool have_snap = false;
    uint32_t N = 0, npad = 0, W = 0, R = 0, leaf_begin = 0, n_leaves = 0, max_leaf_rows = 0;
    uint32_t blk_leaves = 4;  // most leaves any tally workgroup owns, rounded up to 4 (LDS tally stride)
    DevBuf labels, taints, freer, excl, leaf_start, blk;
    DevBuf wtiles;              // wave tiles of the three-launch tally (tally_wave_kernel)
    uint32_t n_wtiles = 0;
    uint32_t n_blocks = 0;
    uint32_t epoch = 0;  // compaction launches so far (granule tags)

    // classes
    bool have_cls = false;
    uint32_t C = 0;
    std::vector<jsp::DevClass> cls_h;
    DevBuf cls, word_off, feas;
    uint32_t feas_words = 0;

    // scratch
    DevBuf cap, occ, run_class, run_len, assign, stats, ticket, granules, recs;
    HostBuf h_runs, h_assign, h_stats;  // zero-copy staging of the host placement path
    HostBuf h_done;                     // [n_blocks] completion words of the host placement path
    HostBuf h_err;                      // [1] error word: a failed launch writes its epoch (sticky)
    // snapshot patches run asynchronously: the delta is staged in pinned
    // memory the patch kernel reads in place, whose last workgroup writes
    // patch_seq to h_patch_done (patch_wait)
    HostBuf h_patch, h_patch_done;
    HostBuf h_batch;                    // pinned staging of the webhook / reconciler batches (A5, A9)
    // jsp_explain: the row pass's per-workgroup counts, the records on the
    // device (zeroed per call) and their pinned copy
    DevBuf ex_parts, ex_out;
    HostBuf h_explain;
    // jsp_place_sticky: the claim tables (0xFFFFFFFF at rest: filled when they
    // are allocated or the topology changed, put back by every call), the
    // grid form's device copy of the call's input and its scratch, the job
    // map, and the pinned staging: the input {prev, job_run, run_class,
    // run_len}, the fill's run list, the fill's answers, the keeper count
    DevBuf sk_tab, sk_taken, sk_in, sk_state, sk_run_kept, sk_wg, sk_map, sk_nrem;
    HostBuf h_sk_in, h_sk_runs, h_sk_fill, h_sk_stat, h_sk_map;
    bool sk_tab_ready = false;
    void* sk_run_kept_p = nullptr;      // the allocation of sk_run_kept that was zeroed
    // jsp_bind_pods: its own claim tables (filled on the stream by every
    // call), the pinned input {job records, assign, order} the kernels read in
    // place and the pinned output {per-job results, pod rows} they write
    DevBuf bd_tab, bd_in;               // bd_in: the input's device copy (calls above kBindInPlaceMax jobs)
    HostBuf h_bd_in, h_bd_out;
    std::vector<uint32_t> h_ls;         // host copy of leaf_start (jsp_bind_pods' job records)
    jsp::BindArgs bd_last{};            // the last successful call's launches (jspb_bind_kernel_loop); J == 0: none
    uint32_t bd_last_wave = 0, bd_last_n = 0;  // its wave form's jobs, its launched jobs
    DevBuf patch_ctr;                  // workgroups of every patch launch so far (device counter)
    unsigned long long patch_target = 0;
    uint32_t patch_seq = 0;
    bool patch_pending = false;
    // the device paths' host walks (host_walk_impl, split_oneshot): the
    // feasibility words (and a completion tag) in pinned memory, and a ring
    // of staging slots for the device paths' run list and assign[]:
    // a back-to-back call never waits for the previous call's assign[] copy
    // (it waited ~12 us for that copy's completion report, profiles/r06)
    struct WalkStage {
        HostBuf io;
        hipEvent_t ev = nullptr;
        bool pending = false;
    };
    static constexpr int kWalkStages = 4;
    WalkStage hw_stage[kWalkStages];
    uint32_t hw_next = 0;
    uint32_t hw_tag = 0;
    HostBuf hw_feas;
    // the split tiles launched for one request (split_oneshot): their answer
    // lines (pinned), the geometry the host walk's tile table was set for,
    // and the request numbers of these launches
    HostBuf os_split;
    unsigned long long os_key = ~0ull;
    uint32_t os_seq = 0;
    DevBuf lvl_ready;                   // the one-launch level walk's published record count
    uint32_t lvl_epoch = 0;
    uint32_t err_tag = 0;               // launches that may report a timed-out wait (kernel error words)
    bool patch_svc = false;             // the pending patch goes to the service's dispatcher
    bool patch_deferred = false;        // ... and is held back for the next request (not posted yet)
    uint32_t patch_bits = 0;            // its request bits (kReqPatch, kReqPatchInline)
    uint32_t patch_nf = 0;              // inline: n | column flags << 16 (the request's n_runs word)
    uint32_t patch_req = 0;             // the request that posted it alone (0: none)
    // A micro-patch (jsp_internal.h kMailbox*): a patch small enough to ride
    // in the next request's line, held back until a request carries it (no
    // staging read, no post of its own); patches of the same columns merge
    // into it while it is held
    bool patch_micro = false;
    uint32_t micro_n = 0, micro_fl = 0;  // its rows (distinct) and column flags
    uint32_t micro_w[jsp::kMailboxPayload] = {};
    // The waker: a host thread that restarts the service for a recovery's
    // first patch off the caller's thread (the launch after an idle period
    // costs ~10 us of host time). wake_job is guarded by mu; the thread
    // sleeps on wake_cv (wake_ring / wake_quit under wake_mu).
    bool wake_job = false;
    std::thread waker;
    std::mutex wake_mu;
    std::condition_variable wake_cv;
    std::atomic<bool> wake_ring{false}, wake_quit{false};
    // a ring is delivered after the caller releases mu (wake_notify) -- only
    // while the waker sleeps on wake_cv: while the service is armed it polls
    // wake_ring instead (waker_poll), so a recovery's first patch call makes
    // no system call
    std::atomic<bool> wake_notify{false};
    std::atomic<bool> waker_poll{false};     // the service is armed: the waker polls
    std::atomic<bool> waker_polling{false};  // the waker is in its polling loop
    jsp::PatchArgs last_patch{};        // its kernel form (the fallback when the service left without it)
    uint32_t err_ack = 0;               // last error word value reported to a caller
    uint32_t* stats_override = nullptr;  // kernels' stats go here when set (host path)
    int fused_mode = JSP_FUSED_AUTO;
    uint32_t last_shape = 0;  // 0 three launches, 1 fused tail, 2 single-class compaction
    // draws on the single-launch kernels' tickets so far (DevBuf ticket [0]
    // tiles, [1] finished tiles): every launch adds its grid / tile count
    unsigned long long tile_draws = 0, done_draws = 0;
    // look-back polls before a compaction tile gives up (hooks.lookback_spins,
    // taken at snapshot upload)
    uint32_t spin_limit = 1u << 22;

    // stream ordering: work is enqueued on the engine stream or a caller's;
    // the first call on a different stream waits for the previous one. A
    // caller's stream is touched only inside the call that was given it: the
    // call records ev_last on it before returning, and later calls wait on
    // that engine-owned event (the caller may destroy its stream meanwhile).
    hipStream_t last_stream = nullptr;  // compared, never used after its call returned
    bool foreign_pending = false;       // device-path work on a caller's stream not yet waited for (ev_last)
    bool have_last = false;
    bool last_foreign = false;          // the last call enqueued on a caller's stream
    hipEvent_t ev_switch = nullptr;     // recorded on the engine stream
    hipEvent_t ev_last = nullptr;       // recorded on the last caller stream, at the end of its call
    // ev_last alternates between two events: a launch that carries an event
    // still pending from the previous call (its kernel running) waits in the
    // runtime for it -- ~7 us of host time per device-path call (profiles/r06)
    hipEvent_t ev_ring[2] = {nullptr, nullptr};
    int ev_i = 0;

    // resident placement service: the compaction shape kept on the GPU
    // between host-API placements (place_service_kernel), fed by a host-mapped
    // request word instead of a launch
    struct Service {
        bool running = false;
        hipStream_t stream = nullptr;
        hipEvent_t ev_exit = nullptr;  // recorded behind the kernel at its stop (svc_stop)
        HostBuf box;     // request: [0] (J << 32) | seq, [1] (n_runs << 32) | seq; u32 [8] ready
        HostBuf words;   // done[nb] | stats[2] | err[1] | clk[kSvcClkSlots nb]
        HostBuf assign;  // [cap]
        HostBuf bits;    // compaction: the bitmap answer, one 64-byte line per tile (ServiceArgs::bits)
        DevBuf granules; // compaction granules | bell, one 128-B line each after the granules | XCC votes | microbox |
                         // the tiles' standing lines (ServiceArgs::stand)
        HostBuf counters;  // [kSvcCounters] the last service's totals, written by its dispatcher as it leaves
        HostBuf split;   // split shape: the tiles' feasibility slots (jsp_internal.h SplitArgs)
        HostBuf pdesc;   // the patch descriptor its dispatcher reads (kReqPatch)
        HostBuf pstage;  // inline patch staging (kReqPatchInline, jsp_internal.h), sized at snapshot upload
        uint32_t groups = 1, cpg = 1;  // split shape: class groups of its tiles
        uint32_t blocks = 0;           // row blocks the running service was started for
        uint32_t cap = 0, nb = 0, seq = 0, err_ack = 0, gen = 0;
        int shape = 0;   // 2 compaction, 3 split
        bool clk = false;
        bool rows_dirty = true;  // a patch since the last request: its tiles reload their rows from memory
        // a micro-patch since the last request: the request that carries it
        // hands its rows to the resident tiles (the dispatcher's microbox), any
        // other request reloads them (rows_dirty)
        bool micro_dirty = false;
        uint32_t pending = 0;    // a compaction request answered early: its tiles' done words still to come
        bool resume = false;  // an upload stopped it: start it again once the engine is ready
        bool pending_ready = false;  // launched; the dispatcher's ready word not seen yet
        std::chrono::steady_clock::time_point t_launch{};
        bool broken = false;  // the service cannot run on this geometry (its grid is not co-resident): the
                              // launch path answers until the next upload (every upload clears it)
        bool start_failed = false;  // the last start never saw its dispatcher poll (-> broken)
        bool armed = false;   // the host API was answered by the service: a patch (re)starts it (svc_wake)
        unsigned long long zero_key = ~0ull;  // geometry the granule / bell lines were last zeroed for
        unsigned long long layout_key = ~0ull;  // geometry the host-side slots / words were laid out for
        unsigned long long occ_key = ~0ull;   // (shape, LDS, grid) whose co-residency was last checked
        int occ_fit = 0;
        std::chrono::steady_clock::time_point last{};
        std::chrono::steady_clock::time_point first_seen{};  // the current request's first answer entry (svc_wait_entries)
        bool bitmap = false;  // compaction answers with tile bitmaps (ServiceArgs::bits)
    } svc;
    int svc_mode = JSP_SERVICE_AUTO;
    Grave grave;  // buffers replaced while the service ran: freed when it stops

    // metrics (jsp_engine_get_metrics): their own lock, so that reading them
    // never waits for a placement; taken after mu where both are held
    std::mutex met_mu;
    jsp_metrics met{};

    // timing
    bool timing = false;
    std::vector<EvPair> tev;  // jsp_*_device_timed: one start/stop pair per step
    DevBuf tmp_scrub;         // the scrub kernel's sink word
    std::vector<EvPair> ev;
    size_t ev_used = 0;
    jsp_timing acc{};

    ~jsp_engine() {
        if (waker.joinable()) {  // jsp_engine_destroy joins it; any other delete too
            {
                std::lock_guard<std::mutex> l(wake_mu);
                wake_quit.store(true);
            }
            wake_cv.notify_one();
            waker.join();
        }
        if (multi) jspm::destroy(multi);
        (void)hipSetDevice(device);
        for (auto* v : {&ev, &tev})
            for (auto& p : *v) {
                if (p.a) (void)hipEventDestroy(p.a);
                if (p.b) (void)hipEventDestroy(p.b);
            }
        if (ev_switch) (void)hipEventDestroy(ev_switch);
        for (auto& w : hw_stage)
            if (w.ev) (void)hipEventDestroy(w.ev);
        for (hipEvent_t x : ev_ring)
            if (x) (void)hipEventDestroy(x);
        if (stream) (void)hipStreamDestroy(stream);
        if (svc.ev_exit) (void)hipEventDestroy(svc.ev_exit);
        if (svc.stream) (void)hipStreamDestroy(svc.stream);
    }
    // jsp_assume (on jsp_bind_pods' buffers): the jobs' states and the conflict
    // word; jsp_forget: the sorted owner list (pinned, then its device copy)
    // and the workgroups' counts (pinned). Behind every other member: the
    // layout of what the placement path reads is the one it was measured with.
    DevBuf as_state, fg_own;
    HostBuf h_fg_own, h_fg_parts;
    // The host lease: the answer lines are a function of the
    // rows and the class record alone, and the host (under mu) is their only
    // writer -- so while nothing has changed since the request whose lines sit
    // in svc.bits was posted, a placement without a patch is expanded from
    // those lines and never crosses the link. gen counts the changes: every
    // writer of rows, classes, topology, service state, timing or hooks goes
    // through lease_drop. seq / posted: the last request that leaves lines (0:
    // none) and gen as it was posted.
    struct Lease {
        uint64_t gen = 1, posted = 0;
        uint32_t seq = 0;
        bool held = false;                        // a placement was answered under it
        std::chrono::steady_clock::time_point t_end{};  // when the last such call returned (place_call: a hot caller)
        uint64_t answered = 0, taken = 0, dropped = 0;  // jspb_lease_counters
    } lease;
    // The lease's kept list (DESIGN.md §4.3 "the kept list"): the feasible
    // leaves the lines of request lease.seq expand to, in answer order, kept
    // from the second host answer of a lease on, so that a later one copies
    // its first min(J, n_list) entries instead of decoding the lines again.
    // Valid iff (gen, seq) equal the lease's: lease_drop and lease_posted end
    // it. The buffer grows at a build only (256 leaves per tile).
    struct LeaseMemo {
        std::vector<int32_t> list;
        uint32_t n_list = 0;      // leaves kept
        uint32_t lines_used = 0;  // lines read when the list was built (tag-checked on every answer)
        bool complete = false;    // the lines ran out before the jobs did: the list is every feasible leaf
        uint64_t gen = 0;         // the key: lease.gen and lease.seq at the build (gen 0: none)
        uint32_t seq = 0;
        uint64_t answered = 0, built = 0;  // jspb_lease_memo_counters
    } memo;
    // jsp_place_gangs: the span counts' rows (one per class and span level,
    // the thread form's first; built at the first call after a class upload)
    // and the counts in pinned memory. Behind every other member, as the
    // members above
    DevBuf gs_rows;
    HostBuf h_gs_cnt;
    bool gs_ready = false;
    int gs_form = 0;                    // how the rows were split (0: by segment size; jspb_span_counts forces one)
    uint32_t gs_n_thread = 0, gs_n_wave = 0, gs_max_thread = 0, gs_max_wave = 0;
    std::vector<jsp::SpanRow> gs_rows_h;
    jsp::GangState gs_state;            // the gang walk's state and the counts' layout (jsp_walk.h)
    // jsp_place_fit: the order step's rows (one per class, the rank form's
    // first; built at the first call after a class upload), its keys, the
    // block form's sorted keys and its output {order [n], fit [n], nf [C]} on
    // the device, and that output's pinned copy for the walk
    DevBuf fit_rows, fit_keys, fit_sorted, fit_out;
    HostBuf h_fit_out;
    bool fit_ready = false;
    int fit_form = 0;                   // how the rows were split (0: by segment size; jspb_fit_order forces one)
    uint32_t fit_n_rank = 0, fit_n_block = 0, fit_max_rank = 0, fit_max_block = 0, fit_max_threads = 0;
    uint32_t fit_n = 0;                 // entries of all segments
    std::vector<jsp::FitRow> fit_rows_h;
    std::vector<uint32_t> fit_off_h;    // [C + 1] first entry of each class's segment
    // jspb_last_plan: what the launch paths decided last (place_impl,
    // tally_impl, assign_impl), and the plan of the last service start, which
    // stands for the calls that service answers. Never touched on an answer path.
    jspb_plan plan{}, svc_plan{};
    // jsp_place_whatif: the scenarios' rows and delta columns (pinned staging
    // and its device copy), the scenarios' feasibility words and flip counts
    // on the device, and their pinned copy for the walks. Behind every other
    // member, as the members above: no offset the placement path reads moves.
    DevBuf wi_in, wi_out;
    HostBuf h_wi_in, h_wi_out;
    // jsp_place_preempt: the call's victim table and evict_free (pinned staging
    // and its device copy), the row codes, the merged free column, the leaf
    // words and cap' on the device, the order step's output {order [n],
    // key32 [n], seg [n], nf [C]} on the device and its pinned copy, and the
    // pinned job records and victim list of the gather. Behind every other
    // member too.
    DevBuf pre_in, pre_code, pre_free, pre_leaf, pre_cap, pre_out;
    HostBuf h_pre_in, h_pre_out, h_pre_jobs, h_pre_vic;
    // jsp_place_spread: the call's sorted peer table and span-count rows
    // (pinned staging and its device copy), the peer flag per row and the leaf
    // words on the device, the tables {fits words, the two span-count tables
    // [C][D_s], peers [D_s]} on the device and, behind the feasibility words,
    // their pinned copy for the walk, the walk's state, and the last call's
    // host walk time (jspb_place_spread_loop). Behind every other member too.
    DevBuf sp_in, sp_flag, sp_leaf, sp_out;
    HostBuf h_sp_in, h_sp_out;
    jsp::SpreadState sp_state;
    double sp_walk_us = 0.0;
    // The entry stamps: hooks.fast_clock where jsp_place and
    // jsp_snapshot_patch read it before they take mu, and the metrics of the
    // placements answered under the lease, written under mu by the answering
    // call and added to `met` by jsp_engine_get_metrics under met_mu. Behind
    // every other member too.
    std::atomic<bool> fast_clock{true};
    LeasedMetrics lmet;
};

namespace {

// An entry or exit stamp of jsp_place / jsp_snapshot_patch: the TSC's
// (jsp_clock.h), steady_clock's under the test hook fast_clock=0.
inline std::chrono::steady_clock::time_point stamp_now(const jsp_engine* e) {
    return e->fast_clock.load(std::memory_order_relaxed) ? jsp_clock::fast_now() : std::chrono::steady_clock::now();
}

// 1024-row chunks per tally workgroup: one (hooks.block_chunks in tests).
// Measured on MI355X (cfg4, 1M rows, C=4) the tally takes 14.2 / 18.9 / 23.2 /
// 28.4 / 39.2 us at 1/2/3/4/8 chunks per workgroup -- the chunk's row/leaf
// passes, not its HBM loads, set a workgroup's time, and more, smaller-grid
// workgroups hide each other's latency better than a next-chunk prefetch does.
constexpr size_t kMaxEvents = 3 * 4096;
// Above this many tally workgroups the three-launch shape wins: the fused tail
// runs feasibility + assignment on one 256-thread workgroup.
constexpr uint32_t kFusedMaxBlocks = 256;

// Make stream s wait for everything the engine enqueued before (on any
// stream): the engine stream's work through an event recorded on it now, a
// caller stream's through ev_last, recorded at the end of the call that used
// it (that stream itself is never touched again: it may be gone). ev_last
// rides on the call's kernel launches as their stop event
// (jsp::set_launch_stop), so it completes with the last kernel and no marker
// packet follows it; a call that launched nothing records it. Its release is
// device scope: ordering a later stream after the device call needs no more.
int wait_prior(jsp_engine* e, hipStream_t s) {
    if (!e->have_last) return JSP_OK;
    if (e->last_foreign) {
        HIP_TRY(hipStreamWaitEvent(s, e->ev_last, 0));
    } else {
        if (!e->ev_switch) HIP_TRY(hipEventCreateWithFlags(&e->ev_switch, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(e->ev_switch, e->stream));
        HIP_TRY(hipStreamWaitEvent(s, e->ev_switch, 0));
    }
    return JSP_OK;
}

// Order work on stream s after everything the engine enqueued before on
// another stream (uploads and jsp_place use the engine stream, the device
// entry points the caller's). Calls on one stream cost nothing here.
int patch_fence(jsp_engine* e);
int enter_stream(jsp_engine* e, hipStream_t s) {
    // a patch the service applies is not stream-ordered: wait for its word
    if (int rc = patch_fence(e)) return rc;
    if (e->have_last && e->last_stream != s)
        if (int rc = wait_prior(e, s)) return rc;
    if (s != e->stream) jsp::set_launch_stop(e->ev_ring[e->ev_i ^ 1]);  // this call's end (ev_last after it)
    return JSP_OK;
}

// After a call enqueued its work on s: a caller's stream gets ev_last
// recorded on it (when no launch carried it) while the handle is known to be
// valid.
int leave_stream(jsp_engine* e, hipStream_t s) {
    const bool launched = jsp::launch_stop_used();
    jsp::set_launch_stop(nullptr);
    e->last_stream = s;
    e->have_last = true;
    e->last_foreign = s != e->stream;
    e->foreign_pending = e->last_foreign;
    if (e->last_foreign) {
        e->ev_i ^= 1;
        e->ev_last = e->ev_ring[e->ev_i];
        if (!launched) HIP_TRY(hipEventRecord(e->ev_last, s));
    }
    return JSP_OK;
}

// Host wait for the last caller-stream call's work.
int wait_last_foreign(jsp_engine* e) {
    HIP_TRY(hipEventSynchronize(e->ev_last));
    return JSP_OK;
}

// Entry of a call that enqueues on the engine's own stream: ordered after
// earlier caller-stream work, and later calls order after it by an event on
// the engine stream (no HIP call needed at its end).
int use_engine_stream(jsp_engine* e) {
    if (int rc = enter_stream(e, e->stream)) return rc;
    return leave_stream(e, e->stream);
}

// Non-blocking: a launch whose bounded wait timed out has written its tag to
// the host-mapped error word (jsp_internal.h kErr*: the kind in the top two
// bits). Reported once, by the next call.
int check_launch_error(jsp_engine* e) {
    const uint32_t w = __atomic_load_n(e->h_err.as<uint32_t>(), __ATOMIC_ACQUIRE);
    if (w != e->err_ack) {
        e->err_ack = w;
        const uint32_t kind = w & jsp::kErrKindMask, n = w & ~jsp::kErrKindMask;
        if (kind == jsp::kErrExpand)
            return set_err(JSP_EHIP, "placement launch %u failed: the level walk's expanders timed out waiting for "
                                     "the walker's records; that launch's assign[] is invalid", n);
        if (kind == jsp::kErrPipe)
            return set_err(JSP_EHIP, "placement launch %u failed: the pipelined batch walk timed out waiting for an "
                                     "earlier batch; that launch's assign[] is invalid", n);
        if (kind == jsp::kErrCopyWait)
            return set_err(JSP_EHIP, "placement launch %u failed: its assign[] copy timed out waiting for the host "
                                     "walk; that launch's assign[] is invalid", n);
        return set_err(JSP_EHIP, "placement launch %u failed: the compaction look-back timed out (a workgroup "
                                 "never published its count); that launch's assign[] is invalid", n);
    }
    return JSP_OK;
}

// The next error tag of a launch that may time out in a bounded wait (never
// 0 in the low 30 bits, so it always differs from an acknowledged word).
uint32_t next_err_tag(jsp_engine* e, uint32_t kind) {
    e->err_tag = e->err_tag % 0x3FFFFFFFu + 1u;
    return kind | e->err_tag;
}

// Something the standing answer depends on changes (or may have): rows,
// classes, topology, the service's state or mode, timing, hooks. The lines the
// host holds answer nothing from here on; the next placement crosses the link.
void lease_drop(jsp_engine* e) {
    auto& l = e->lease;
    l.gen += 1;
    if (l.held) {
        l.held = false;
        l.dropped += 1;
    }
    e->memo.gen = 0;  // (its key no longer matches either way)
}

// Request `seq` is posted to the service: lines, when every tile will write
// its tagged line for it (the compaction service's bitmap answer, whatever
// its J -- the waker's warm-up included).
void lease_posted(jsp_engine* e, uint32_t seq, bool lines) {
    e->lease.seq = lines ? seq : 0u;
    e->lease.posted = e->lease.gen;
    e->lease.held = false;  // renewed, not dropped: the next host answer takes it again
    e->memo.gen = 0;        // other lines: the list is built again, by the second host answer
}

// The waits' stream query (guarded_wait, jsp_wait.h): has the stream finished,
// or failed? The status stays here for the caller's error text.
struct StreamQuery {
    hipStream_t s;
    hipError_t q = hipSuccess;
    StreamState operator()() {
        q = hipStreamQuery(s);
        return q == hipSuccess ? StreamState::finished : q == hipErrorNotReady ? StreamState::running : StreamState::failed;
    }
};

// Host placement path: wait for the kernel's completion words (one per
// signalling workgroup) instead of the kernel-end signal. A finished stream
// whose words are missing, or a failed stream, is an error.
int wait_done(jsp_engine* e, hipStream_t s, uint32_t n, uint32_t epoch) {
    const uint32_t* words = e->h_done.as<uint32_t>();
    uint32_t i = 0;
    StreamQuery sq{s};
    const WaitResult r = guarded_wait(
        [&](uint64_t) {
            while (i < n && __atomic_load_n(words + i, __ATOMIC_ACQUIRE) == epoch) ++i;
            return i == n;
        },
        NoSideCheck{}, sq);
    if (r == WaitResult::gone) return set_err(JSP_EHIP, "placement kernel ended without completion word %u", i);
    if (r == WaitResult::failed) return set_err(JSP_EHIP, "placement kernel failed: %s", hipGetErrorString(sq.q));
    return JSP_OK;
}

int resolve_timing(jsp_engine* e) {
    if (e->ev_used == 0) return JSP_OK;
    HIP_TRY(hipEventSynchronize(e->ev[e->ev_used - 1].b));
    for (size_t i = 0; i < e->ev_used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->ev[i].a, e->ev[i].b));
        if (e->ev[i].tag == 0) e->acc.tally_ms += ms;
        else if (e->ev[i].tag == 1) e->acc.feas_ms += ms;
        else if (e->ev[i].tag == 2) e->acc.assign_ms += ms;
        else {
            e->acc.fused_ms += ms;
            std::lock_guard<std::mutex> l(e->met_mu);
            hist_add(e->met.device_us, ms * 1e3, JSP_HIST_LO_US);
        }
    }
    e->ev_used = 0;
    return JSP_OK;
}

// Returns the pair to bracket a launch with (nullptr when timing is off).
EvPair* ev_begin(jsp_engine* e, int tag, hipStream_t s) {
    if (!e->timing) return nullptr;
    if (e->ev_used == kMaxEvents && resolve_timing(e) != JSP_OK) return nullptr;
    if (e->ev_used == e->ev.size()) {
        EvPair p;
        if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return nullptr;
        e->ev.push_back(p);
    }
    EvPair* p = &e->ev[e->ev_used++];
    p->tag = tag;
    if (tag == 0 || tag == 3) e->acc.calls += 1;
    if (tag == 3) e->acc.fused_calls += 1;
    (void)hipEventRecord(p->a, s);
    return p;
}

void ev_end(EvPair* p, hipStream_t s) {
    if (p) (void)hipEventRecord(p->b, s);
}

// The caller's stream is used as given: NULL is the HIP null stream (what
// torch's default stream is), jsp_engine_stream(e) the engine's own.
hipStream_t pick(jsp_engine*, void* s) { return static_cast<hipStream_t>(s); }

int check_engine(jsp_engine* e) {
    if (!e) return set_err(JSP_EINVAL, "engine is NULL");
    if (hipSetDevice(e->device) != hipSuccess) return set_err(JSP_EHIP, "hipSetDevice(%d) failed", e->device);
    return JSP_OK;
}

// Where a buffer that must grow now leaves its old allocation: the grave
// while the resident service runs (freed when it stops), else nowhere.
Grave* grave(jsp_engine* e) { return e->svc.running ? &e->grave : nullptr; }

template <class T>
hipError_t upload(DevBuf& b, const T* src, size_t n, hipStream_t s, Grave* g = nullptr) {
    hipError_t err = b.reserve(n * sizeof(T), g);
    if (err != hipSuccess || n == 0) return err;
    return hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, s);
}

jsp::TallyArgs tally_args(jsp_engine* e, uint32_t* d_cap, uint32_t* d_occ, uint32_t ld) {
    jsp::TallyArgs a{};
    a.labels = e->labels.as<uint64_t>();
    a.taints = e->taints.as<uint32_t>();
    a.freer = e->freer.as<uint32_t>();
    a.excl = e->excl.as<int32_t>();
    a.npad = e->npad;
    a.leaf_start = e->leaf_start.as<uint32_t>();
    a.blk = e->blk.as<uint4>();
    a.n_blocks = e->n_blocks;
    a.la = e->blk_leaves;
    a.cls = e->cls.as<jsp::DevClass>();
    a.cap_out = d_cap;
    a.occ_out = d_occ;
    a.ld = ld;
    a.leaf_base = e->leaf_begin;
    a.W = (int)e->W;
    a.R = (int)e->R;
    a.c0 = 0;
    a.nc = std::min<uint32_t>(e->C, jsp::kTallyClasses);
    a.do_occ = 1;
    return a;
}

// Workgroups of the wave-tile tally: 4 waves per SIMD (best warm and cold of
// 1-8 on cfg4, profiles/r03) over the CUs, never more than the tiles need and
// never fewer than 64 tiles per wave allow.
uint32_t tally_wave_grid(jsp_engine* e) {
    // one tile per wave (grid 0: the one-set kernel) while every tile fits
    // 6 waves per SIMD; beyond that the double-buffered kernel
    if (e->hooks.tally_one && e->n_wtiles <= (uint32_t)std::max(e->n_cu, 1) * 4u * 6u) return 0;
    constexpr uint32_t wps = 4;
    // at least n_wtiles / 64 waves: a wave holds at most 64 tile descriptors
    const uint32_t waves = std::max<uint32_t>(std::min<uint32_t>(e->n_wtiles, (uint32_t)std::max(e->n_cu, 1) * 4u * wps),
                                              (e->n_wtiles + 63) / 64);
    return std::max<uint32_t>(1, (waves + jsp::kTallyWaves - 1) / jsp::kTallyWaves);
}

// Whether the wave tally can fold the feasibility words into itself (the
// three-launch shape on the engine's own unsharded tallies): at most 4
// classes (one wave pass), all at the leaf level, wave tiles available.
bool fold_ok(jsp_engine* e, bool shard = false) {
    if (e->C < 1 || e->C > 4 || e->n_wtiles == 0 || e->hooks.tally_block) return false;
    if (!shard && (e->leaf_begin != 0 || e->n_leaves != e->L_total)) return false;
    for (const auto& c : e->cls_h)
        if (c.level + 1 != e->K) return false;
    return (uint64_t)(e->C + 1) * e->L_total * 4 < (1ull << 31);
}

// The tally alone (three-launch shape, jsp_tally_device): the wave-tile
// kernel when every leaf fits a wave tile, else the workgroup-block kernel.
// fold_feas (null: none): the wave tally sets the leaf classes' feasibility
// words there (fold_ok's shape; a shard of a device set folds into the words
// of the set's assigning engine)
int tally_impl(jsp_engine* e, uint32_t* d_cap, uint32_t* d_occ, uint32_t ld, hipStream_t s,
               uint64_t* fold_feas = nullptr) {
    jsp::TallyArgs a = tally_args(e, d_cap, d_occ, ld);
    if (fold_feas) {
        a.feas_fold = fold_feas;
        a.fold_nw = (e->L_total + 63) / 64;
    }
    jspb_plan& pl = e->plan;
    pl.tally = JSPB_TALLY_IN_TILE;
    pl.tally_passes = 0;
    pl.folded = fold_feas ? 1u : 0u;
    pl.n_blocks = e->n_blocks;
    pl.n_wtiles = e->n_wtiles;
    if (e->n_blocks == 0) return JSP_OK;
    const bool block = e->hooks.tally_block;
    EvPair* p = ev_begin(e, 0, s);
    uint32_t c0 = 0;
    do {
        a.c0 = c0;
        a.nc = std::min<uint32_t>(e->C - c0, jsp::kTallyClasses);
        a.do_occ = (c0 == 0);
        // the wave-tile kernel takes 1-4 classes with the occupancy count in one pass
        const bool wave = !block && e->n_wtiles > 0 && a.do_occ && a.nc >= 1 && a.nc <= 4 &&
                          (uint64_t)(e->C + 1) * ld * 4 < (1ull << 31);
        const uint32_t wgrid = wave ? tally_wave_grid(e) : 0u;
        if (!wave) HIP_TRY(jsp::launch_tally(a, s));
        else HIP_TRY(jsp::launch_tally_wave(a, e->wtiles.as<uint4>(), e->n_wtiles, e->n_leaves, wgrid, s));
        if (c0 == 0) pl.tally = !wave ? JSPB_TALLY_BLOCK : wgrid == 0 ? JSPB_TALLY_WAVE_ONE : JSPB_TALLY_WAVE_DB;
        pl.tally_passes += 1;
        c0 += a.nc;
    } while (c0 < e->C);
    ev_end(p, s);
    return JSP_OK;
}

uint32_t* stats_ptr(jsp_engine* e) { return e->stats_override ? e->stats_override : e->stats.as<uint32_t>(); }

// The level walker's shape: every class at one level of <= kLevelMaxWords
// words, <= kLevelMaxRuns runs.
bool level_walk_ok(jsp_engine* e, uint32_t n_runs) {
    if (e->C < 1 || n_runs > jsp::kLevelMaxRuns) return false;
    const uint32_t lvl = e->cls_h[0].level;
    for (const auto& c : e->cls_h)
        if (c.level != lvl) return false;
    const uint32_t nw = (e->D[lvl] + 63) / 64;
    return nw >= 1 && nw <= jsp::kLevelMaxWords && jsp::level_walk_lds_bytes(e->C, nw) <= 128u * 1024u;
}

// The walk on the host (ABI v7) for every shape the level walker does not
// take -- several levels, or many runs -- up to kHostWalkMaxJobs jobs: there
// the GPU walk is one wave's dependent scalar chain at ~100 shader cycles per
// job visit (cfg5: 49.6 us, SQ_WAIT_ANY 82 % of its wave cycles, DESIGN.md
// §4.2), while the host walks the same bitmaps in ~2.5 us (jsp_walk.cc, the
// split service's walk; SURVEY.md §7 step 5 allows the sequential part of A7
// on the host). The GPU computes the feasibility words; the host reads them,
// walks, and writes assign[].
constexpr uint32_t kHostWalkMaxJobs = 1u << 16;
// Below this many jobs the GPU walk (~40 ns per job visit) costs less than the
// host round trip of the walk on the host (~15 us: the answer out, the copy
// of assign[] back): cfg3's 64 jobs take 16.6 us on the fused launch against
// 26.8 us walked on the host; cfg5's 500 take 49.6 against 30.5 (profiles/r06).
constexpr uint32_t kHostWalkMinJobs = 256;

// (JSP_FUSED_OFF keeps every walk on the GPU: the three-launch shape, which
// the tests use to exercise the GPU walkers on the shapes AUTO walks here)
bool host_walk_ok(jsp_engine* e, uint32_t n_runs, uint32_t J) {
    return e->fused_mode == JSP_FUSED_AUTO && e->C >= 1 && n_runs > 0 && J >= kHostWalkMinJobs &&
           J <= kHostWalkMaxJobs && !level_walk_ok(e, n_runs);
}

// The next staging slot of the device paths' walks, `bytes` large: its last
// copy has long finished by the time the ring comes round (a wait only then).
int walk_stage(jsp_engine* e, size_t bytes, jsp_engine::WalkStage** out) {
    jsp_engine::WalkStage& w = e->hw_stage[e->hw_next];
    if (w.pending) {
        HIP_TRY(hipEventSynchronize(w.ev));
        w.pending = false;
    }
    if (!w.ev) HIP_TRY(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
    HIP_TRY(w.io.reserve(bytes + 64, grave(e)));  // + the host's release word of the copy (copy_wait_kernel)
    *out = &w;
    return JSP_OK;
}

// The assign[] copy of a device-path walk, launched before the host walks:
// it waits for the host's release of the slot's flag (walk_release), so the
// copy needs no launch after the walk. Carries the call's stop event.
int walk_copy_launch(jsp_engine* e, jsp_engine::WalkStage* w, size_t flag_off, const int32_t* staged, int32_t* d_assign,
                     uint32_t J, hipStream_t s, uint32_t* tag) {
    uint32_t* flag = reinterpret_cast<uint32_t*>(static_cast<char*>(w->io.p) + flag_off);
    e->hw_tag = e->hw_tag % 0x7FFFFFFFu + 1u;
    *tag = e->hw_tag;
    __atomic_store_n(flag, 0u, __ATOMIC_RELEASE);
    HIP_TRY(jsp::launch_copy_wait(flag, *tag, reinterpret_cast<const uint32_t*>(staged),
                                  reinterpret_cast<uint32_t*>(d_assign), J, e->h_err.as<uint32_t>(),
                                  next_err_tag(e, jsp::kErrCopyWait), e->hooks.wait_ticks, s));
    return JSP_OK;
}

// The host's side of walk_copy_launch: the walk's assign[] is in the staging
// (ok), or the call fails and nothing is copied (!ok).
void walk_release(jsp_engine::WalkStage* w, size_t flag_off, uint32_t tag, bool ok) {
    uint32_t* flag = reinterpret_cast<uint32_t*>(static_cast<char*>(w->io.p) + flag_off);
    __atomic_store_n(flag, ok ? tag : (tag | 0x80000000u), __ATOMIC_RELEASE);
}

// After the assign[] copy out of slot w was launched on stream s.
int walk_stage_done(jsp_engine* e, jsp_engine::WalkStage* w, hipStream_t s) {
    HIP_TRY(hipEventRecord(w->ev, s));
    w->pending = true;
    e->hw_next = (e->hw_next + 1) % jsp_engine::kWalkStages;
    return JSP_OK;
}

// The classes' feasibility words of the tallies d_cap / d_occ into dst
// (e->feas, or the host walk's pinned copy).
int feas_launch(jsp_engine* e, const uint32_t* d_cap, const uint32_t* d_occ, uint32_t ld, uint64_t* dst, hipStream_t s) {
    HIP_TRY(jsp::launch_feas(d_cap, d_occ, ld, e->cls.as<jsp::DevClass>(), e->C, e->word_off.as<uint32_t>(),
                             e->feas_words, e->topo, dst, s));
    return JSP_OK;
}

// A tag written behind a stream's launches tells the host they are done (an
// event's completion reaches the host microseconds later). The word follows
// the feasibility words of hw_feas, which the caller has reserved.
struct StreamTag {
    uint32_t* word;
    uint32_t want;
};
int tag_post(jsp_engine* e, hipStream_t s, StreamTag* t) {
    t->word = e->hw_feas.as<uint32_t>() + 2 * (size_t)std::max<uint32_t>(e->feas_words, 1);
    e->hw_tag = e->hw_tag % 0x7FFFFFFFu + 1u;
    t->want = e->hw_tag;
    HIP_TRY(jsp::launch_tag(t->word, t->want, s));
    return JSP_OK;
}

// What a tag wait's three errors call the work they waited for.
struct TagWork {
    const char *ended, *its, *failed, *late;
};

// The host's wait for a posted tag: a stream that finished without it, a
// failed stream and 10 s without either are errors.
int tag_wait(jsp_engine* e, hipStream_t s, const StreamTag& t, const TagWork& w) {
    e->walk.prefetch_state();  // while the device works
    const WaitBound<> bound{std::chrono::steady_clock::now(), std::chrono::seconds(10)};
    StreamQuery sq{s};
    const uint32_t* const word = t.word;  // (by value: the spin loads the word alone, not t beside it)
    const uint32_t want = t.want;
    const WaitResult r = guarded_wait([=](uint64_t) { return __atomic_load_n(word, __ATOMIC_ACQUIRE) == want; },
                                      NoSideCheck{}, sq, WaitPause::yes, &bound);
    if (r == WaitResult::gone) return set_err(JSP_EHIP, "%s ended without %s tag", w.ended, w.its);
    if (r == WaitResult::failed) return set_err(JSP_EHIP, "%s failed: %s", w.failed, hipGetErrorString(sq.q));
    if (r == WaitResult::late) return set_err(JSP_EHIP, "%s did not complete within 10 s", w.late);
    return JSP_OK;
}

// Feasibility (feas_kernel into pinned memory, or the folded words copied
// there), the run list staged when it is device-resident, one wait, the walk,
// and assign[] copied back when it is device-resident. host_io: run_class,
// run_len and d_assign are pinned host memory (the host API's staging) -- no
// copies, the walk writes assign[] in place and the stats too. The call's
// stop event (a caller stream's end-of-call marker) rides on its last launch,
// the assign[] copy.
int host_walk_impl(jsp_engine* e, const uint32_t* d_cap, const uint32_t* d_occ, uint32_t ld,
                   const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, uint32_t J, int32_t* assign,
                   hipStream_t s, bool folded, bool host_io) {
    const uint32_t fw = std::max<uint32_t>(e->feas_words, 1);
    HIP_TRY(e->hw_feas.reserve((size_t)fw * 8 + 64, grave(e)));  // + the tag word
    jsp_engine::WalkStage* st = nullptr;
    if (!host_io)
        if (int rc = walk_stage(e, (size_t)n_runs * 8 + (size_t)J * 4, &st)) return rc;
    uint32_t* hrc = host_io ? const_cast<uint32_t*>(run_class) : st->io.as<uint32_t>();
    uint32_t* hrl = host_io ? const_cast<uint32_t*>(run_len) : hrc + n_runs;
    int32_t* out = host_io ? assign : reinterpret_cast<int32_t*>(hrc + 2 * (size_t)n_runs);
    // a caller stream's end-of-call event rides on the last launch only (each
    // launch that carries one costs its dispatch an event write)
    const hipEvent_t stop = jsp::take_launch_stop();
    EvPair* p = ev_begin(e, 1, s);
    if (folded)
        HIP_TRY(jsp::launch_copy_u32(e->feas.as<uint32_t>(), e->hw_feas.as<uint32_t>(), 2 * e->feas_words, s));
    else if (int rc = feas_launch(e, d_cap, d_occ, ld, e->hw_feas.as<uint64_t>(), s))
        return rc;
    ev_end(p, s);
    if (!host_io) {
        HIP_TRY(jsp::launch_copy_u32(run_class, hrc, n_runs, s));
        HIP_TRY(jsp::launch_copy_u32(run_len, hrl, n_runs, s));
    }
    StreamTag tag{};
    if (int rc = tag_post(e, s, &tag)) return rc;
    // the assign[] copy is queued now (it waits for the walk's release): no
    // launch between the walk and the copy
    const size_t flag_off = (size_t)n_runs * 8 + (size_t)J * 4;
    uint32_t ctag = 0;
    if (!host_io) {
        jsp::set_launch_stop(stop);
        if (int rc = walk_copy_launch(e, st, flag_off, out, assign, J, s, &ctag)) return rc;
        if (int rc = walk_stage_done(e, st, s)) {
            walk_release(st, flag_off, ctag, false);
            return rc;
        }
    }
    if (int rc = tag_wait(e, s, tag, {"host walk: the feasibility", "its", "host walk: feasibility",
                                      "host walk: the device feasibility"})) {
        if (!host_io) walk_release(st, flag_off, ctag, false);
        return rc;
    }
    p = ev_begin(e, 2, s);
    const uint32_t placed = e->walk.walk(e->hw_feas.as<uint64_t>(), hrc, hrl, n_runs, out);
    if (e->stats_override) {  // the host API reads them (pinned)
        e->stats_override[0] = n_runs;
        e->stats_override[1] = placed;
    }
    if (!host_io) walk_release(st, flag_off, ctag, true);
    else jsp::set_launch_stop(stop);
    ev_end(p, s);
    return JSP_OK;
}

int assign_impl(jsp_engine* e, const uint32_t* d_cap, const uint32_t* d_occ, uint32_t ld,
                const uint32_t* d_run_class, const uint32_t* d_run_len, uint32_t n_runs, uint32_t J,
                int32_t* d_assign, hipStream_t s, bool folded = false, bool host_io = false) {
    jspb_plan& pl = e->plan;
    pl.walker = JSPB_WALK_NONE;
    pl.level_wpt = pl.level_threads = pl.feas_in_lds = pl.topo_in_lds = pl.stage_cap = pl.fscr_words = 0;
    pl.groups = pl.cpg = 1;
    pl.folded = folded ? 1u : 0u;
    // (last_shape too: after a call the service answered, jspb_last_plan must
    // report this launch, also when jsp_assign_device issued it)
    if (host_walk_ok(e, n_runs, J)) {
        pl.shape = e->last_shape = 7;
        pl.walker = JSPB_WALK_HOST;
        return host_walk_impl(e, d_cap, d_occ, ld, d_run_class, d_run_len, n_runs, J, d_assign, s, folded, host_io);
    }
    pl.shape = e->last_shape = 0;
    EvPair* p = ev_begin(e, 1, s);
    if (!folded)
        if (int rc = feas_launch(e, d_cap, d_occ, ld, e->feas.as<uint64_t>(), s)) return rc;
    ev_end(p, s);
    p = ev_begin(e, 2, s);
    if (e->recs.reserve(sizeof(jsp::AssignRec) * (size_t)std::max<uint32_t>(J, 1), grave(e)) != hipSuccess)
        return set_err(JSP_ENOMEM, "assignment records (%u jobs)", J);
    jsp::WaitErr we{e->h_err.as<uint32_t>(), 0u, e->hooks.pipe_spins, e->hooks.wait_ticks};
    if (level_walk_ok(e, n_runs)) {
        // the expansion rides in the walker's launch: its expanders wait
        // (bounded) for the walker's record count, and one that gives up
        // writes the launch's tag to the error word (kErrExpand)
        const uint32_t nw = (e->D[e->cls_h[0].level] + 63) / 64;
        if (!e->lvl_ready.p) {
            HIP_TRY(e->lvl_ready.reserve(64));
            HIP_TRY(hipMemsetAsync(e->lvl_ready.p, 0, 64, s));
        }
        e->lvl_epoch = e->lvl_epoch % 0x7FFFFFFFu + 1u;
        we.tag = next_err_tag(e, jsp::kErrExpand);
        pl.walker = JSPB_WALK_LEVEL;
        jsp::level_walk_shape(nw, &pl.level_wpt, &pl.level_threads);
        HIP_TRY(jsp::launch_assign_level(e->feas.as<uint64_t>(), e->C, nw, d_run_class, d_run_len, n_runs, J, d_assign,
                                         stats_ptr(e), e->stats.as<uint32_t>() + 3, e->recs.as<jsp::AssignRec>(), s,
                                         e->lvl_ready.as<unsigned long long>(), e->lvl_epoch, we));
        ev_end(p, s);
        return JSP_OK;
    }
    we.tag = next_err_tag(e, jsp::kErrPipe);
    {
        // launch_assign's own plan, from the same arguments
        const jsp::AssignPlan ap = jsp::plan_assign(e->t_off_h[e->K], e->feas_words,
                                                    e->K > 1 ? jsp::topo_table_words(e->K, e->topo.D) : 0u);
        pl.walker = JSPB_WALK_ASSIGN;
        pl.feas_in_lds = ap.feas_in_lds;
        pl.topo_in_lds = ap.topo_in_lds;
        pl.stage_cap = ap.stage_cap;
    }
    HIP_TRY(jsp::launch_assign(e->feas.as<uint64_t>(), e->word_off.as<uint32_t>(), e->cls.as<jsp::DevClass>(),
                               e->C, e->topo, e->t_off_h[e->K], e->feas_words, d_run_class, d_run_len, n_runs, J,
                               d_assign, stats_ptr(e), e->stats.as<uint32_t>() + 3, e->recs.as<jsp::AssignRec>(), s,
                               we));
    ev_end(p, s);
    return JSP_OK;
}

bool fused_ok(jsp_engine* e) {
    return e->fused_mode == JSP_FUSED_AUTO && e->n_blocks > 0 && e->n_blocks <= kFusedMaxBlocks &&
           e->C <= (uint32_t)jsp::kTallyClasses &&
           e->leaf_begin == 0 && e->n_leaves == e->L_total &&
           e->t_off_h[e->K] + e->feas_words <= jsp::kFusedMaxWords;
}

// One class at the leaf level: job j takes the j-th feasible leaf (any size).
bool compact_ok(jsp_engine* e) {
    return e->fused_mode == JSP_FUSED_AUTO && e->n_blocks > 0 && e->C == 1 && e->cls_h[0].level + 1 == e->K &&
           e->leaf_begin == 0 && e->n_leaves == e->L_total;
}

// Launch arguments of the fused shape (the launch path and the resident
// service); sets a.sc1_out, the tallies' write-through hand-off to the tail.
jsp::FusedArgs fused_args(jsp_engine* e, jsp::TallyArgs& a, const uint32_t* d_run_class, const uint32_t* d_run_len,
                          uint32_t n_runs, uint32_t J, int32_t* d_assign, uint32_t* stats) {
    jsp::FusedArgs f{};
    f.ticket = e->ticket.as<unsigned long long>();
    f.tile_base = e->tile_draws;
    f.done_base = e->done_draws;
    f.C = e->C;
    f.topo = e->topo;
    f.t_off = e->t_off.as<uint32_t>();
    f.t_words = e->t_off_h[e->K];
    f.word_off = e->word_off.as<uint32_t>();
    f.feas_words = e->feas_words;
    f.run_class = d_run_class;
    f.run_len = d_run_len;
    f.n_runs = n_runs;
    f.J = J;
    f.assign = d_assign;
    f.stats = stats;
    const uint32_t topo_words = e->K > 1 ? jsp::topo_table_words(e->K, e->topo.D) : 0u;
    f.topo_in_lds = topo_words > 0 && topo_words <= jsp::kFusedTopoMax ? 1u : 0u;
    f.topo_lds_words = f.topo_in_lds ? topo_words : 0u;
    {
        uint32_t lv[jsp::kMaxClasses];
        for (uint32_t c = 0; c < e->C; ++c) lv[c] = e->cls_h[c].level;
        f.fscr_words = jsp::fused_scratch_words(e->K, e->topo.D, lv, e->C);
        bool upper = false;
        for (uint32_t c = 0; c < e->C; ++c) upper |= lv[c] + 1 < e->K;
        // write-through hand-off of the tallies to the tail (no release/acquire
        // fences) unless the tail's per-wave upper-class path, which reads them
        // with plain loads, will run
        a.sc1_out = !upper || f.fscr_words != 0 ? 1 : 0;
    }
    // class groups: a small snapshot's tiles are VALU-bound over many classes;
    // splitting the classes over up to 4 groups of >= 2 multiplies the tiles
    // (each row block read once per group), within 128 tiles
    f.groups = 1;
    if (e->C > 2) {
        const uint32_t by_c = std::min<uint32_t>(4, (e->C + 1) / 2);
        const uint32_t by_t = std::max<uint32_t>(1, 128 / std::max<uint32_t>(e->n_blocks, 1));
        f.groups = std::max<uint32_t>(1, std::min(by_c, by_t));
    }
    f.cpg = (a.nc + f.groups - 1) / f.groups;
    f.we = jsp::WaitErr{e->h_err.as<uint32_t>(), next_err_tag(e, jsp::kErrPipe), e->hooks.pipe_spins,
                        e->hooks.wait_ticks};
    f.lds_bytes = jsp::fused_lds_bytes(f.t_words, f.feas_words, f.cpg, f.cpg + a.do_occ, a.la,
                                       f.topo_in_lds ? topo_words : 0u, f.fscr_words);
    return f;
}

bool split_ok(jsp_engine* e);
uint32_t split_groups(jsp_engine* e);
uint32_t next_seq(uint32_t q);

// The split shape launched for one request (ABI v7, shape 8): the resident
// split service's tiles (tally, per-leaf feasibility ballots, upper-domain
// partial sums, tagged lines into pinned memory) as one launch of tiles only
// -- no dispatcher, no residency -- and the host walk over their lines, as
// the service's answer is walked. The launch path and the device paths of
// every multi-class / multi-level shape the split service takes, up to
// kHostWalkMaxJobs jobs. host_io: the run list and assign[] are pinned host
// memory (the host API's staging); otherwise they are device buffers, staged
// through pinned memory by copy launches on the same stream.
bool split_oneshot_ok(jsp_engine* e, uint32_t n_runs, uint32_t J) {
    return e->fused_mode == JSP_FUSED_AUTO && n_runs > 0 && J >= kHostWalkMinJobs && J <= kHostWalkMaxJobs &&
           split_ok(e);
}

int split_oneshot(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, uint32_t J,
                  int32_t* assign, hipStream_t s, bool host_io) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const uint32_t g = split_groups(e), cpg = (e->C + g - 1) / g, nb = e->n_blocks, n_tiles = nb * g;
    const uint32_t nw = jsp::split_waves(e->blk_l0, e->blk_l1);
    const size_t sb = (size_t)n_tiles * jsp::split_tile_words(cpg, nw) * 8;
    if (sb > e->os_split.bytes || !e->os_split.p) {
        HIP_TRY(e->os_split.reserve(sb, grave(e)));
        std::memset(e->os_split.p, 0, e->os_split.bytes);  // tags: request 0 is never posted
    }
    const unsigned long long key = ((unsigned long long)nb << 40) | ((unsigned long long)g << 32) | cpg;
    if (e->os_key != key) {
        e->walk.set_tiles(e->blk_l0, e->blk_l1, g, cpg);
        e->os_key = key;
        e->svc.layout_key = ~0ull;  // the service re-lays its own slots (and the walk's tiles) at its next start
    }
    jsp_engine::WalkStage* st = nullptr;
    if (!host_io)
        if (int rc = walk_stage(e, (size_t)n_runs * 8 + (size_t)J * 4, &st)) return rc;
    uint32_t* hrc = host_io ? const_cast<uint32_t*>(run_class) : st->io.as<uint32_t>();
    uint32_t* hrl = host_io ? const_cast<uint32_t*>(run_len) : hrc + n_runs;
    int32_t* out = host_io ? assign : reinterpret_cast<int32_t*>(hrc + 2 * (size_t)n_runs);
    e->os_seq = next_seq(e->os_seq);
    const uint32_t seq = e->os_seq;
    const jsp::TallyArgs ta = tally_args(e, nullptr, nullptr, e->L_total);
    jsp::SplitArgs sp{};
    sp.groups = g;
    sp.cpg = cpg;
    sp.nw = nw;
    sp.C = e->C;
    sp.out = e->os_split.as<uint64_t>();
    sp.topo = e->topo;
    if (!host_io) {  // the device-resident run list comes out with tile 0's answer
        sp.run_class = run_class;
        sp.run_len = run_len;
        sp.run_dst = hrc;
        sp.n_runs = n_runs;
    }
    jsp::ServiceArgs a{};
    a.oneshot = seq;
    a.anc_words = jsp::split_anc_words(cpg, e->blk_leaves, (int)e->W, (int)e->R, false);
    // the assign[] copy rides in the same launch: one extra workgroup waits
    // for the walk's release and copies (no launch between walk and copy)
    const size_t flag_off = (size_t)n_runs * 8 + (size_t)J * 4;
    uint32_t ctag = 0;
    if (!host_io) {
        uint32_t* flag = reinterpret_cast<uint32_t*>(static_cast<char*>(st->io.p) + flag_off);
        e->hw_tag = e->hw_tag % 0x7FFFFFFFu + 1u;
        ctag = e->hw_tag;
        __atomic_store_n(flag, 0u, __ATOMIC_RELEASE);
        sp.cw_flag = flag;
        sp.cw_tag = ctag;
        sp.cw_src = reinterpret_cast<const uint32_t*>(out);
        sp.cw_dst = reinterpret_cast<uint32_t*>(assign);
        sp.cw_n = J;
        sp.cw_err = e->h_err.as<uint32_t>();
        sp.cw_err_tag = next_err_tag(e, jsp::kErrCopyWait);
        sp.cw_ticks = e->hooks.wait_ticks;
    }
    EvPair* p = ev_begin(e, 3, s);
    const auto tl = clk::now();
    // one launch (the copy as a kernel of its own behind the tiles measured the
    // same: 20.9 against 21.7 us per back-to-back call, profiles/r06/g2)
    HIP_TRY(jsp::launch_split_oneshot(ta, sp, a, s));  // carries the call's stop event, if any
    e->acc.oneshot_stage_us += std::chrono::duration<double, std::micro>(tl - t0).count();
    ev_end(p, s);
    if (!host_io)
        if (int rc = walk_stage_done(e, st, s)) {
            walk_release(st, flag_off, ctag, false);
            return rc;
        }
    const auto t1 = clk::now();
    e->walk.prefetch_state();
    // every tile's tagged lines (the answer), bounded; a failed stream is an error
    const uint64_t* slots = e->os_split.as<uint64_t>();
    uint32_t t = 0;
    const WaitBound<clk> bound{t1, std::chrono::seconds(10)};
    // (the stream also holds the queued copy, which waits for this walk: a
    // query reports the split launch's failure, never success)
    StreamQuery sq{s};
    const WaitResult r = guarded_wait<clk>(
        [&](uint64_t spins) {
            while (t < n_tiles && e->walk.tile_ready(slots, t, seq)) ++t;
            if (t == n_tiles) return true;
            if ((spins & 7) == 1)
                for (uint32_t u = t + 1; u < n_tiles; ++u) e->walk.prefetch_tile(slots, u);
            return false;
        },
        NoSideCheck{}, sq, WaitPause::no, &bound);
    const int wrc = r == WaitResult::gone     ? set_err(JSP_EHIP, "split launch ended without the answer of tile %u", t)
                    : r == WaitResult::failed ? set_err(JSP_EHIP, "split launch failed: %s", hipGetErrorString(sq.q))
                    : r == WaitResult::late   ? set_err(JSP_EHIP, "split launch: no answer within 10 s")
                                              : JSP_OK;
    if (wrc) {
        if (!host_io) walk_release(st, flag_off, ctag, false);
        return wrc;
    }
    // (a device-resident run list came out with tile 0's lines: its stores
    // were released before them)
    const auto t2 = clk::now();
    const uint32_t placed = e->walk.place(slots, hrc, hrl, n_runs, out);
    if (e->stats_override) {
        e->stats_override[0] = n_runs;
        e->stats_override[1] = placed;
    }
    if (!host_io) walk_release(st, flag_off, ctag, true);
    // the phases (jspb_get_timing): set-up and launch, the wait for the
    // tiles' lines, the walk and the copy launch
    using us = std::chrono::duration<double, std::micro>;
    const auto t3 = clk::now();
    e->acc.oneshot_calls += 1;
    e->acc.oneshot_launch_us += us(t1 - t0).count();
    e->acc.oneshot_wait_us += us(t2 - t1).count();
    e->acc.oneshot_walk_us += us(t3 - t2).count();
    return JSP_OK;
}

// Whole placement on the engine's own tally buffers: one compaction launch for
// a single leaf-level class, one fused launch when the snapshot is small, else
// tally -> feas -> assign. `signal`: the single-launch shapes write host
// completion words (e->h_done) tagged e->epoch; *n_signals says how many.
int place_impl(jsp_engine* e, const uint32_t* d_run_class, const uint32_t* d_run_len, uint32_t n_runs, uint32_t J,
               int32_t* d_assign, hipStream_t s, bool signal = false, uint32_t* n_signals = nullptr,
               bool want_tally = false, bool host_io = false) {
    e->epoch = e->epoch % 0x3FFFFFFFu + 1u;
    if (n_signals) *n_signals = 0;
    jspb_plan& pl = e->plan;
    pl = jspb_plan{};
    pl.groups = pl.cpg = 1;
    pl.n_blocks = e->n_blocks;
    pl.n_wtiles = e->n_wtiles;
    if (compact_ok(e)) {
        e->last_shape = 2;
        pl.shape = 2;
        pl.walker = JSPB_WALK_COMPACT;
        // the compaction keeps its sums in LDS; they go out only when asked for
        jsp::TallyArgs a = want_tally ? tally_args(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total)
                                      : tally_args(e, nullptr, nullptr, e->L_total);
        jsp::CompactArgs f{};
        f.ticket = e->ticket.as<unsigned long long>();
        f.tile_base = e->tile_draws;
        f.granules = e->granules.as<unsigned long long>();
        f.pods = e->cls_h[0].pods;
        f.n_runs = n_runs;
        f.J = J;
        f.assign = d_assign;
        f.stats = stats_ptr(e);
        f.epoch = e->epoch;
        f.err = e->h_err.as<uint32_t>();
        f.spin_limit = e->spin_limit;
        f.done = signal ? e->h_done.as<uint32_t>() : nullptr;
        if (n_signals && signal) *n_signals = e->n_blocks;
        EvPair* p = ev_begin(e, 3, s);
        HIP_TRY(jsp::launch_compact(a, f, s));
        ev_end(p, s);
        e->tile_draws += e->n_blocks + jsp::kSpareBlocks;
        return JSP_OK;
    }
    // the split tiles launched for this request, the walk on the host (shape
    // 8: no tallies wanted -- they stay in the tiles' LDS)
    if (!want_tally && split_oneshot_ok(e, n_runs, J)) {
        e->last_shape = 8;
        pl.shape = 8;
        pl.walker = JSPB_WALK_SPLIT_HOST;
        pl.groups = split_groups(e);
        pl.cpg = (e->C + pl.groups - 1) / pl.groups;
        return split_oneshot(e, d_run_class, d_run_len, n_runs, J, d_assign, s, host_io);
    }
    // the walk on the host after the GPU's tally and feasibility (shape 7), or
    // on the GPU: one fused launch (shape 1), three launches (shape 0)
    const bool hw = host_walk_ok(e, n_runs, J);
    e->last_shape = hw ? 7 : fused_ok(e) ? 1 : 0;
    if (e->last_shape != 1) {
        const bool fold = fold_ok(e);
        if (int rc = tally_impl(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, s,
                                fold ? e->feas.as<uint64_t>() : nullptr))
            return rc;
        return assign_impl(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, d_run_class, d_run_len,
                           n_runs, J, d_assign, s, fold, host_io);
    }
    jsp::TallyArgs a = tally_args(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total);
    jsp::FusedArgs f = fused_args(e, a, d_run_class, d_run_len, n_runs, J, d_assign, stats_ptr(e));
    f.done = signal ? e->h_done.as<uint32_t>() : nullptr;
    f.epoch = e->epoch;
    if (n_signals && signal) *n_signals = 1;
    pl.shape = 1;
    pl.walker = JSPB_WALK_FUSED_TAIL;
    pl.topo_in_lds = f.topo_in_lds;
    pl.fscr_words = f.fscr_words;
    pl.groups = f.groups;
    pl.cpg = f.cpg;
    EvPair* p = ev_begin(e, 3, s);
    HIP_TRY(jsp::launch_fused(a, f, s));
    ev_end(p, s);
    e->tile_draws += e->n_blocks * f.groups + jsp::kSpareBlocks;
    e->done_draws += e->n_blocks * f.groups;
    return JSP_OK;
}

// ---- resident placement service ----
// Host side of place_service_kernel. The request word is written last with one
// 64-bit store (x86 keeps store order; the kernel reads it with system-scope
// vector loads). The host answers from the done words, as for a launch.
// Idle exit: a workgroup leaves after JSP_SERVICE_IDLE_MS without a request;
// the host restarts the service when its own last request is older than half
// of that, so it never posts into an exit (and if it ever did, the dead
// service is seen by a stream query and the request re-posted once).
constexpr uint32_t kSvcMaxBlocks = 255;  // one tile per workgroup + the dispatcher, all co-resident (<= one per CU)
constexpr int kSvcGone = 1;
constexpr int kSvcFailed = 3;  // a tile reported a failed wait through the service's error word
// svc_stop's bound on the kernel's exit after the stop word (it leaves within
// ~2 us; the runtime reports it ~8 us later)
constexpr std::chrono::milliseconds kStopLimit{2000};

double svc_idle_ms() {
    static const double ms = [] {
        const char* v = std::getenv("JSP_SERVICE_IDLE_MS");
        const double x = v ? std::strtod(v, nullptr) : 50.0;
        return x >= 1.0 && x <= 5000.0 ? x : 50.0;
    }();
    return ms;
}

// The engine's idle limit: JSP_SERVICE_PARKED never idles out (a dedicated
// GPU; the service leaves on jsp_engine_service_stop, an upload or destroy).
constexpr double kParkedIdleMs = 1e15;
double idle_ms(const jsp_engine* e) { return e->svc_mode == JSP_SERVICE_PARKED ? kParkedIdleMs : svc_idle_ms(); }

// Class groups of the split service's tiles: as the fused shape's (up to 4
// groups of >= 2 classes, within 128 tiles), capped by the co-resident tile
// limit.
uint32_t split_groups(jsp_engine* e) {
    uint32_t g = 1;
    if (e->C > 2) {
        const uint32_t by_c = std::min<uint32_t>(4, (e->C + 1) / 2);
        const uint32_t by_t = std::max<uint32_t>(1, 128 / std::max<uint32_t>(e->n_blocks, 1));
        g = std::max<uint32_t>(1, std::min(by_c, by_t));
    }
    while (g > 1 && e->n_blocks * g > kSvcMaxBlocks) --g;
    return g;
}

// The split shape (tiles resident, the walk on the host): any snapshot whose
// tiles fit the service, all classes in <= 16 per group.
bool split_ok(jsp_engine* e) {
    if (e->fused_mode != JSP_FUSED_AUTO || e->n_blocks == 0 || e->leaf_begin != 0 || e->n_leaves != e->L_total)
        return false;
    const uint32_t g = split_groups(e);
    // an upper class's records carry its domain in 20 bits (jsp_internal.h SplitArgs)
    for (uint32_t c = 0; c < e->C; ++c)
        if (e->cls_h[c].level + 1 < e->K && e->D[e->cls_h[c].level] >= jsp::kSplitMaxDomains) return false;
    return e->n_blocks * g <= kSvcMaxBlocks && (e->C + g - 1) / g <= (uint32_t)jsp::kTallyClasses && e->C > 0;
}

// The shape the service would run for the engine's current state (2
// compaction, 3 split), 0 = none. The split shape answers every multi-class
// or multi-level shape the fused launch would (and more: no LDS limit on the
// walk, which runs on the host).
int svc_shape(jsp_engine* e) {
    if (e->svc_mode == JSP_SERVICE_OFF || !e->have_topo || !e->have_snap || !e->have_cls ||
        e->n_blocks > kSvcMaxBlocks || e->svc.broken)
        return 0;
    if (compact_ok(e)) return 2;
    if (split_ok(e)) return 3;
    return 0;
}
bool svc_ok(jsp_engine* e) { return svc_shape(e) != 0; }

// The request line (pinned host memory the dispatcher polls, jsp_internal.h
// kMailbox*) and, on a line of its own after it, the dispatcher's ready word.
// A request line in device memory written through the BAR was measured
// slower on every shape.
constexpr size_t kBoxBytes = jsp::kMailboxBytes + 128;
constexpr size_t kReadyWord = jsp::kMailboxBytes / 4 + 16;

// One 16-byte chunk of the request line in one store (aligned 16-byte SSE
// stores are single-copy atomic on x86-64 processors with AVX).
inline void store16(uint32_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    _mm_store_si128(reinterpret_cast<__m128i*>(p), _mm_set_epi32((int)d, (int)c, (int)b, (int)a));
}

// Post request `seq`: the micro-patch payload chunks (micro: the held-back
// micro-patch rides in it), chunk 1 {seq, rows, patch number, flags}, then
// chunk 0 -- its second half first: the dispatcher reads the whole line in
// one load and takes a read whose chunks disagree on seq for none.
void svc_request(jsp_engine* e, uint32_t seq, uint32_t jw, uint32_t w2, bool micro = false) {
    uint32_t* b = e->svc.box.as<uint32_t>();
    uint32_t m = 0, fl = 0, pseq = (jw & jsp::kReqPatch) ? e->patch_seq : 0u;
    if (micro && e->micro_n > 0) {
        m = e->micro_n;
        fl = e->micro_fl;
        pseq = e->patch_seq;
        const uint32_t words = m * jsp::micro_row_words(e->W, e->R);
        for (uint32_t c = 0; 3 * c < words; ++c)
            store16(b + 4 * (2 + c), seq, e->micro_w[3 * c], e->micro_w[3 * c + 1], e->micro_w[3 * c + 2]);
    }
    store16(b + 4, seq, m, pseq, fl);
    unsigned long long* r = reinterpret_cast<unsigned long long*>(b);
    __atomic_store_n(r + 1, ((unsigned long long)w2 << 32) | seq, __ATOMIC_RELEASE);
    __atomic_store_n(r, ((unsigned long long)jw << 32) | seq, __ATOMIC_RELEASE);
}

// The stop word (every workgroup of the service leaves).
void svc_post_stop(jsp_engine* e) {
    __atomic_store_n(e->svc.box.as<unsigned long long>(), (unsigned long long)jsp::kSvcStop, __ATOMIC_RELEASE);
}

int patch_wait(jsp_engine* e);
int svc_stop(jsp_engine* e) {
    auto& v = e->svc;
    lease_drop(e);  // whoever stops it is about to change something, or found it gone
    // a patch posted to the dispatcher lands first (the stop word would
    // replace its request); one held back stays so (patch_wait applies it)
    if (e->patch_pending && e->patch_svc && !e->patch_deferred)
        if (int rc = patch_wait(e)) return rc;
    v.pending = 0;  // the stop waits for the kernel to leave, i.e. for every tile to finish
    if (!v.running) return JSP_OK;
    v.running = false;
    // The kernel leaves within ~2 us of the stop word; the runtime reports it
    // complete ~7-9 us later whatever the host does (tools/stop_anatomy.hip,
    // profiles/r05/probes/stop_anatomy.txt). An event recorded behind it
    // (before the stop word: the record's own host time overlaps the exit)
    // and its synchronize report it soonest: 7.7 us from the stop word,
    // against 9.3 us polling hipStreamQuery.
    if (!v.ev_exit) HIP_TRY(hipEventCreateWithFlags(&v.ev_exit, hipEventDisableTiming));
    const hipError_t rec = hipEventRecord(v.ev_exit, v.stream);
    svc_post_stop(e);
    // Bounded: a kernel that never reads the stop word -- a wedged
    // dispatcher -- would hold a blocking synchronize forever. The event is
    // polled instead, up to kStopLimit; past it the service is marked broken
    // (the launch path answers until the next upload) and the call fails.
    // (not a guarded_wait: it polls an event, not words beside a stream)
    hipError_t q = hipSuccess;
    if (rec == hipSuccess) {
        const auto t0 = std::chrono::steady_clock::now();
        while ((q = hipEventQuery(v.ev_exit)) == hipErrorNotReady) {
            if (std::chrono::steady_clock::now() - t0 > kStopLimit) {
                v.broken = true;
                return set_err(JSP_EHIP, "placement service did not leave within %lld ms of its stop word",
                               (long long)std::chrono::duration_cast<std::chrono::milliseconds>(kStopLimit).count());
            }
            _mm_pause();
        }
    } else {
        q = hipStreamSynchronize(v.stream);
    }
    if (q != hipSuccess) return set_err(JSP_EHIP, "placement service failed: %s", hipGetErrorString(q));
    e->grave.flush();  // nothing resident any more: a free no longer waits
    return JSP_OK;
}

// Uploads stop the service (it holds the old buffers and geometry) and start
// it again at their end when it was running, so the next jsp_place -- the
// recovery path: post-delete snapshot uploaded, then placed -- finds it ready.
int svc_suspend(jsp_engine* e) {
    // every patch lands before an upload replaces what it patched
    lease_drop(e);  // an upload: rows, classes, topology or hooks change
    if (int rc = patch_wait(e)) return rc;
    e->svc.resume |= e->svc.running;
    e->svc.broken = false;  // new geometry: the service may fit again
    e->svc.zero_key = ~0ull;  // and its lines are zeroed again at the next start
    e->svc.layout_key = ~0ull;
    return svc_stop(e);
}

int svc_start(jsp_engine* e, uint32_t J, bool wait_ready);
int svc_wait_ready(jsp_engine* e);
// The upload returns once the new service polls, so the recovery's "post-delete
// snapshot uploaded -> jsp_place" finds it ready instead of waiting for its
// launch inside the placement (a failure here resurfaces at the next jsp_place).
void svc_resume(jsp_engine* e) {
    if (e->svc.resume && svc_ok(e)) {
        e->svc.resume = false;
        (void)svc_start(e, 0, true);
    }
}

void start_waker(jsp_engine* e);
void notify_waker_poll(jsp_engine* e);

int svc_start(jsp_engine* e, uint32_t J, bool wait_ready) {
    auto& v = e->svc;
    lease_drop(e);  // a new service: its answer buffer may be laid out (and zeroed) again
    if (!v.stream) HIP_TRY(hipStreamCreateWithFlags(&v.stream, hipStreamNonBlocking));
    start_waker(e);  // created with the first service, never on a recovery's path
    const uint32_t nb = e->n_blocks;
    if (J > v.cap || !v.assign.p) {
        const uint32_t cap = std::max<uint32_t>(4096, J + J / 2);
        HIP_TRY(v.assign.reserve((size_t)cap * 8));  // compaction: u64 (seq << 32 | domain) entries
        v.cap = cap;
    }
    const int shape = svc_shape(e);
    if (shape == 0) return set_err(JSP_ESTATE, "no resident-service shape for this engine state");
    uint32_t n_tiles = nb;  // workgroups that answer (and write a done word), dispatcher excluded
    // The host-side layout (split slots, the host walk's tile table, the done
    // and stamp words) is rebuilt only when the geometry changes: every
    // request rewrites the slots the walk reads, done words are compared with
    // request numbers that never repeat, and the error word is acknowledged at
    // its current value -- so a restart after an idle exit (a recovery's cold
    // start) costs the launch alone.
    if (shape == 3) {
        v.groups = split_groups(e);
        v.cpg = (e->C + v.groups - 1) / v.groups;
        n_tiles = nb * v.groups;
    }
    const unsigned long long lkey = ((unsigned long long)nb << 40) | ((unsigned long long)v.groups << 32) |
                                    ((unsigned long long)v.cpg << 8) | (unsigned)shape;
    const size_t nw = (size_t)(1 + jsp::kSvcClkSlots) * n_tiles + 3 + jsp::kSvcClkSlots;  // + the dispatcher's clk row
    if (v.layout_key != lkey || !v.words.p || nw * 4 > v.words.bytes) {
        if (shape == 3) {
            const size_t sb = (size_t)n_tiles * jsp::split_tile_words(v.cpg, jsp::split_waves(e->blk_l0, e->blk_l1)) * 8;
            HIP_TRY(v.split.reserve(sb));
            std::memset(v.split.p, 0, sb);
            e->walk.set_tiles(e->blk_l0, e->blk_l1, v.groups, v.cpg);
        }
        HIP_TRY(v.words.reserve(nw * 4));
        std::memset(v.words.p, 0, nw * 4);  // done words: seq 0 is never posted
        if (shape == 2) {
            HIP_TRY(v.bits.reserve((size_t)64 * std::max<uint32_t>(n_tiles, 1)));
            std::memset(v.bits.p, 0, (size_t)64 * std::max<uint32_t>(n_tiles, 1));  // tags: seq 0 is never posted
        }
        v.layout_key = lkey;
    }
    HIP_TRY(v.box.reserve(kBoxBytes));
    const size_t gbytes = (size_t)8 * std::max<uint32_t>(nb, 1), gpad = (gbytes + 127) & ~size_t(127);
    // granules, then the bell on a line of its own, then the XCC votes.
    // Zeroed only when allocated or the geometry changes: granule tags and
    // request numbers never repeat across starts and a stop in the bell
    // carries its service's generation -- so a restart after an idle exit
    // (the recovery's cold start) costs the launch alone. Every write the
    // service stages from (uploads) was synchronous, and rows are fenced per
    // request (patch_wait), so the launch need not wait for the engine's
    // streams.
    const size_t xbytes = ((size_t)4 * (nb + 1) + 127) & ~size_t(127);  // XCC vote words (co-located service)
    const size_t mbytes = (size_t)8 * (1 + jsp::kMailboxPayload);       // the microbox (not zeroed: seq-tagged)
    const size_t mpad = (mbytes + 127) & ~size_t(127);
    const size_t sbytes = (size_t)64 * std::max<uint32_t>(nb, 1);       // standing lines (the dispatcher zeroes them)
    if (gpad + 128 + xbytes + mpad + sbytes > v.granules.bytes || !v.granules.p) v.zero_key = ~0ull;
    HIP_TRY(v.granules.reserve(gpad + 128 + xbytes + mpad + sbytes));
    if (!v.counters.p) {
        HIP_TRY(v.counters.reserve(128));
        std::memset(v.counters.p, 0, 128);
    }
    const unsigned long long key = ((unsigned long long)nb << 8) | ((unsigned long long)n_tiles << 40) | (unsigned)shape;
    if (v.zero_key != key) {
        HIP_TRY(hipMemsetAsync(v.granules.p, 0, gpad + 128, v.stream));
        v.zero_key = key;
    }
    svc_request(e, v.seq, 0u, 0u);  // already answered: the new dispatcher starts after it
    v.gen = v.gen % 0x7FFFFFFFu + 1u;
    uint32_t* ready = v.box.as<uint32_t>() + kReadyWord;
    __atomic_store_n(ready, 0u, __ATOMIC_RELEASE);
    uint32_t* w = v.words.as<uint32_t>();
    jsp::ServiceArgs a{};
    a.mailbox = v.box.as<unsigned long long>();
    a.granules = v.granules.as<unsigned long long>();
    a.bell = reinterpret_cast<unsigned long long*>(static_cast<char*>(v.granules.p) + gpad);
    a.xcc = reinterpret_cast<uint32_t*>(static_cast<char*>(v.granules.p) + gpad + 128);
    if (!v.pdesc.p) HIP_TRY(v.pdesc.reserve(sizeof(jsp::PatchDesc)));
    if (!e->h_patch_done.p) {
        HIP_TRY(e->h_patch_done.reserve(128));
        std::memset(e->h_patch_done.p, 0, 128);
    }
    // the inline staging was sized for this W/R at snapshot upload (the
    // service was stopped then, and no patch was pending): never reallocated
    // here, where a staged patch may be waiting in it
    if (jsp::patch_inline_layout(jsp::kPatchInlineRows, 15u, e->W, e->R).bytes > v.pstage.bytes)
        return set_err(JSP_ESTATE, "inline patch staging not sized for W=%u R=%u", e->W, e->R);
    a.pstage = v.pstage.as<const char>();
    a.pdesc = v.pdesc.as<jsp::PatchDesc>();
    a.pdone = e->h_patch_done.as<uint32_t>();
    a.taken = e->h_patch_done.as<uint32_t>() + 16;  // its own line
    // co-located compaction service: all its workgroups on one XCD when it
    // fits one (32 CUs, one workgroup per CU)
    a.spread = shape == 2 && nb + 1 <= 32 && e->hooks.svc_xcd ? 8u : 1u;
    a.pods = e->cls_h[0].pods;
    a.seq0 = v.seq;
    a.assign = v.assign.as<int32_t>();
    // the bitmap answer (test hook svc_entries=1: the per-job entries after a
    // look-back, for A/B runs)
    v.bitmap = shape == 2 && !e->hooks.svc_entries;
    a.bits = v.bitmap ? v.bits.as<unsigned long long>() : nullptr;
    // the microbox: a micro-patch's rows for the co-located resident tiles
    a.mbox = shape == 2 ? reinterpret_cast<unsigned long long*>(static_cast<char*>(v.granules.p) + gpad + 128 + xbytes) : nullptr;
    a.micro_spins = e->hooks.micro_spins;
    a.stand = shape == 2 ? reinterpret_cast<unsigned long long*>(static_cast<char*>(v.granules.p) + gpad + 128 + xbytes + mpad)
                         : nullptr;
    a.standing = shape == 2 ? std::min(e->hooks.svc_standing, 2u) : 0u;  // (3: the host's lease on top of 2)
    a.counters = v.counters.as<uint32_t>();
    a.done = w;
    a.stats = w + n_tiles;
    a.err = w + n_tiles + 2;
    a.clk = e->timing && (shape == 2 || shape == 3) ? w + n_tiles + 3 : nullptr;
    a.n_tiles = n_tiles;
    a.spin_limit = e->spin_limit;
    // 100 MHz ticks; parked: 2^62 (never reached, and twice it does not wrap)
    a.idle_ticks = e->svc_mode == JSP_SERVICE_PARKED ? (1ull << 62) : (unsigned long long)(svc_idle_ms() * 1e5);
    a.ready = ready;
    a.gen = v.gen;
    v.err_ack = __atomic_load_n(w + n_tiles + 2, __ATOMIC_ACQUIRE);  // an earlier instance's error is not ours
    v.nb = n_tiles;
    v.blocks = nb;
    v.clk = e->timing;
    v.shape = shape;
    // Every workgroup of the grid must be resident at once (tiles wait on each
    // other and on the dispatcher): check the grid against what the CUs hold
    // at this LDS size before launching; a service that cannot fit is not
    // started and the launch path answers instead.
    const jsp::TallyArgs ta0 = tally_args(e, nullptr, nullptr, e->L_total);
    size_t lds = 0;
    uint32_t grid = 0;
    jsp::SplitArgs sp{};
    // the tiles keep their rows on chip between requests when each is one
    // chunk: the compaction tiles in registers (the resident path), the
    // split tiles in LDS
    const bool one_chunk = e->max_blk_span <= (uint32_t)jsp::kChunkRows;
    if (shape == 2) {
        a.resident = one_chunk ? 1u : 0u;
        a.row_cache_words = 0u;
        lds = jsp::service_lds_bytes(e->blk_leaves, (int)e->W, (int)e->R, false);
        grid = nb + 1;
    } else {
        sp.groups = v.groups;
        sp.cpg = v.cpg;
        sp.nw = jsp::split_waves(e->blk_l0, e->blk_l1);
        sp.C = e->C;
        sp.out = v.split.as<uint64_t>();
        sp.topo = e->topo;
        a.row_cache_words = one_chunk ? jsp::split_row_cache_words(v.cpg, e->blk_leaves) : 0u;
        a.anc_words = jsp::split_anc_words(v.cpg, e->blk_leaves, (int)e->W, (int)e->R, one_chunk);
        lds = jsp::split_service_lds_bytes(v.cpg, e->blk_leaves, (int)e->W, (int)e->R, one_chunk);
        grid = n_tiles + 1;
    }
    {
        // the API answer can be one workgroup per CU high at high SGPR counts
        // (MI355X_MICROARCH.md, Residency): keep that margin. Asked once per
        // (shape, W, R, LDS size).
        const unsigned long long okey = ((unsigned long long)lds << 16) | ((unsigned long long)shape << 8) |
                                        ((unsigned long long)e->W << 4) | e->R;
        if (v.occ_key != okey) {
            int per_cu = 0;
            HIP_TRY(jsp::service_occupancy(ta0, shape, lds, &per_cu));
            v.occ_fit = std::max(per_cu > 1 ? per_cu - 1 : per_cu, 0);
            v.occ_key = okey;
        }
        const int64_t fit = (int64_t)v.occ_fit * e->n_cu;
        if ((int64_t)grid > fit)
            return set_err(JSP_ERANGE, "placement service needs %u co-resident workgroups; %d CUs hold %lld at %zu B "
                                       "of LDS each", grid, e->n_cu, (long long)fit, lds);
    }
    if (shape == 2) HIP_TRY(jsp::launch_service(ta0, a, v.stream));
    else HIP_TRY(jsp::launch_split_service(ta0, sp, a, v.stream));
    e->svc_plan = jspb_plan{};
    e->svc_plan.shape = shape == 3 ? 5u : 3u;  // as place_call reports the service's answers
    e->svc_plan.walker = shape == 3 ? JSPB_WALK_SPLIT_HOST : JSPB_WALK_COMPACT;
    e->svc_plan.groups = shape == 3 ? v.groups : 1u;
    e->svc_plan.cpg = shape == 3 ? v.cpg : 1u;
    e->svc_plan.n_blocks = nb;
    e->svc_plan.n_wtiles = e->n_wtiles;
    v.running = true;
    v.pending_ready = true;
    v.t_launch = std::chrono::steady_clock::now();
    v.last = v.t_launch;
    e->acc.svc_starts += 1;
    {
        std::lock_guard<std::mutex> l(e->met_mu);
        e->met.svc_starts += 1;
    }
    return wait_ready ? svc_wait_ready(e) : JSP_OK;
}

// Return once the dispatcher polls: a request posted then is answered without
// waiting for the launch (bounded: a dispatcher that cannot get a CU within
// 2 s means the grid is not co-resident).
int svc_wait_ready(jsp_engine* e) {
    auto& v = e->svc;
    if (!v.pending_ready) return JSP_OK;
    const uint32_t* ready = v.box.as<uint32_t>() + kReadyWord;
    const auto t_start = v.t_launch;
    const WaitBound<> bound{t_start, std::chrono::seconds(2)};
    // any status but not-ready is an error here (a service whose stream has
    // ended will never poll): finished counts as failed, with no last look
    hipError_t q = hipSuccess;
    const WaitResult r = guarded_wait(
        [&](uint64_t) { return __atomic_load_n(ready, __ATOMIC_ACQUIRE) == v.gen; }, NoSideCheck{},
        [&] { return (q = hipStreamQuery(v.stream)) == hipErrorNotReady ? StreamState::running : StreamState::failed; },
        WaitPause::no, &bound);
    if (r == WaitResult::failed) {
        v.running = false;
        lease_drop(e);
        return set_err(JSP_EHIP, "placement service ended before it started polling: %s", hipGetErrorString(q));
    }
    if (r == WaitResult::late) {
        (void)svc_stop(e);
        v.start_failed = true;  // not co-resident on this GPU as launched: off until the next upload
        return set_err(JSP_EHIP, "placement service did not start polling within 2 s");
    }
    v.pending_ready = false;
    e->acc.svc_ready_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count();
    v.last = std::chrono::steady_clock::now();
    return JSP_OK;
}

// Tile t's bitmap answer line to request seq has arrived whole (its 8
// halves carry seq): the tile is past its row reads -- the bitmap answer's
// done signal (timing off: the tiles write no done word then).
static inline bool bits_line_done(const unsigned long long* b, uint32_t t, uint32_t seq) {
    uint32_t bad = 0;
    for (int k = 0; k < 8; ++k) bad |= (uint32_t)(__atomic_load_n(b + 8u * t + k, __ATOMIC_ACQUIRE) >> 32) ^ seq;
    return bad == 0;
}

// What a service wait's result is to its caller: kSvcFailed, a tile's error
// word moved; kSvcGone, the service left before answering.
static int svc_wait_rc(WaitResult r, const StreamQuery& sq) {
    if (r == WaitResult::abandoned) return kSvcFailed;
    if (r == WaitResult::gone) return kSvcGone;
    if (r == WaitResult::failed) return set_err(JSP_EHIP, "placement service failed: %s", hipGetErrorString(sq.q));
    return JSP_OK;
}

// Waits for every tile's done word == seq (timing off, the bitmap answer:
// every tile's tagged line instead). kSvcGone: the service left before answering (its stream
// finished).
int svc_wait(jsp_engine* e, uint32_t seq, uint32_t J) {
    auto& v = e->svc;
    const uint32_t* words = v.words.as<uint32_t>();
    const unsigned long long* lines = v.bitmap && !v.clk ? v.bits.as<unsigned long long>() : nullptr;
    const uint32_t n = v.nb;
    const bool split = v.shape == 3;
    // (the split service writes done words for requests without jobs, the
    // only ones this waits for; with jobs the host reads its lines,
    // svc_wait_split)
    // every tile's line(s) at once: read one after another they would miss
    // one after another (a settle usually comes after the host slept or
    // worked, with none of them cached)
    if (lines)
        for (uint32_t t = 0; t < n; ++t) __builtin_prefetch(lines + 8u * t, 0, 3);

    // compaction: tiles 0..i-1 have answered, so assign[] up to about i/n of
    // J is final (tiles own consecutive ranges of roughly equal size): start
    // those lines' misses before the copy-out (cfg2 copy-out 0.55 us cold)
    const char* as = v.shape == 2 ? static_cast<const char*>(v.assign.p) : nullptr;
    size_t pf = 0;
    uint32_t i = 0;
    StreamQuery sq{v.stream};
    const WaitResult r = guarded_wait(
        [&](uint64_t) JSP_WAIT_INLINE {
            while (i < n &&
                   (lines ? bits_line_done(lines, i, seq) : __atomic_load_n(words + i, __ATOMIC_ACQUIRE) == seq)) {
                if (split) e->walk.prefetch_tile(v.split.as<uint64_t>(), i);  // its slots are final: start their misses
                ++i;
                if (as) {
                    const size_t upto = ((size_t)J * 8 * i / n) & ~size_t(63);
                    for (; pf + 64 <= upto; pf += 64) __builtin_prefetch(as + pf, 0, 3);
                }
            }
            return i == n;
        },
        // a tile whose microbox wait gave up writes no line, but the error word
        [&] { return lines && __atomic_load_n(words + n + 2, __ATOMIC_ACQUIRE) != v.err_ack; }, sq);
    return svc_wait_rc(r, sq);
}

// The compaction request the host returned from early (its assign[] entries
// had all arrived): wait for its tiles' done words before anything that needs
// them idle -- the next request (tiles past the J-th feasible leaf may still be
// tallying, and the look-back granules are per tile), a patch of the rows.
int svc_settle(jsp_engine* e) {
    auto& v = e->svc;
    if (v.pending == 0) return JSP_OK;
    const uint32_t q = v.pending;
    v.pending = 0;
    if (!v.running) return JSP_OK;
    const int rc = svc_wait(e, q, 0);
    if (rc == kSvcGone) {  // it left after answering: nothing is outstanding
        v.running = false;
        lease_drop(e);
        return JSP_OK;
    }
    if (rc == kSvcFailed) {
        // a tile past the early answer's last job gave up its microbox wait
        // (the answer itself was complete: that tile's line was not needed).
        // Its registers may be stale: the service is stopped, and the next
        // request starts it afresh from the rows in memory.
        v.err_ack = __atomic_load_n(v.words.as<uint32_t>() + v.nb + 2, __ATOMIC_ACQUIRE);
        return svc_stop(e);
    }
    // The early answer had all J entries, so a tile past them that timed out
    // in its look-back (it scattered nothing) did not touch it: acknowledge
    // its error word here rather than blame the next request for it.
    if (rc == JSP_OK && v.words.p)
        v.err_ack = __atomic_load_n(v.words.as<uint32_t>() + v.nb + 2, __ATOMIC_ACQUIRE);
    return rc;
}


// The compaction service's answer read from the entries themselves: entry j
// is (seq << 32 | domain) in one 8-byte store, so the host copies each out as
// soon as it carries this request's seq and returns when all J have -- before
// the tiles drain and publish their done words (those gate the next request:
// svc_settle). kSvcGone: the service left; kSvcFailed: a tile timed out.
int svc_wait_entries(jsp_engine* e, uint32_t seq, uint32_t J, int32_t* out, uint32_t* placed) {
    auto& v = e->svc;
    const unsigned long long* a = v.assign.as<unsigned long long>();
    const uint32_t* w = v.words.as<uint32_t>();
    uint32_t i = 0, n = 0;
    StreamQuery sq{v.stream};
    const WaitResult r = guarded_wait(
        [&](uint64_t) {
            const uint32_t i0 = i;
            while (i < J) {
                const unsigned long long x = __atomic_load_n(a + i, __ATOMIC_ACQUIRE);
                if ((uint32_t)(x >> 32) != seq) break;
                const int32_t d = (int32_t)(uint32_t)x;
                out[i++] = d;
                n += d >= 0 ? 1u : 0u;
            }
            if (i0 == 0 && i > 0) v.first_seen = std::chrono::steady_clock::now();
            return i == J;
        },
        [&] { return __atomic_load_n(w + v.nb + 2, __ATOMIC_ACQUIRE) != v.err_ack; }, sq);
    if (r == WaitResult::ready) *placed = n;
    return svc_wait_rc(r, sq);
}

// The compaction service's bitmap answer (ServiceArgs::bits): tile t's line
// holds its leaves' feasibility as four 64-leaf words, each as two (seq << 32
// | 32 bits) halves. Tiles own consecutive leaf ranges in leaf order, so job
// j's domain is the j-th feasible leaf: the host takes the lines in tile
// order as they arrive, bit by bit, and returns once J jobs have a leaf or
// every tile has answered (the rest get -1). kSvcGone: the service left.
// *all: every tile's line arrived -- each tile then has read its rows and
// holds no state of this request that a patch or the next request could
// disturb, so neither waits for the tiles' done words (svc_settle); after an
// answer complete before its last tiles, they do.
// (the expansion itself, expand_lines: jsp_lines.h)

int svc_wait_bits(jsp_engine* e, uint32_t seq, uint32_t J, int32_t* out, uint32_t* placed, bool* all) {
    auto& v = e->svc;
    const unsigned long long* b = v.bits.as<unsigned long long>();
    const uint32_t n = v.nb, base = e->leaf_begin;
    const uint32_t* l0 = e->blk_l0.data();
    uint32_t t = 0, j = 0;
    StreamQuery sq{v.stream};
    const WaitResult r = guarded_wait(
        [&](uint64_t) JSP_WAIT_INLINE {
            // touch every line still to come (independent loads: their misses
            // overlap), so a line that has landed is in cache when its turn
            // comes -- not one miss after another in tile order
            for (uint32_t u = t + 1; u < n; ++u) __builtin_prefetch(b + 8u * u, 0, 3);
            // (after the service left, this takes every line already complete)
            return expand_lines(b, n, l0, base, seq, J, out, &t, &j,
                                [&v] { v.first_seen = std::chrono::steady_clock::now(); });
        },
        // a tile whose microbox wait gave up writes no line, but the error word
        [&] { return __atomic_load_n(e->svc.words.as<uint32_t>() + n + 2, __ATOMIC_ACQUIRE) != v.err_ack; }, sq);
    if (r == WaitResult::ready) {
        *placed = j;
        *all = t == n;
        for (uint32_t i = j; i < J; ++i) out[i] = -1;
    }
    return svc_wait_rc(r, sq);
}

// The split service's answer (jsp_internal.h SplitArgs): every tile's lines and
// records carry the request, so the host takes tile after tile as each has
// arrived whole -- touching the lines still to come every few polls, so
// their misses overlap -- with no done word in between. kSvcGone: the
// service left.
int svc_wait_split(jsp_engine* e, uint32_t seq) {
    auto& v = e->svc;
    const uint64_t* s = v.split.as<uint64_t>();
    const uint32_t n = v.nb;
    uint32_t t = 0;
    StreamQuery sq{v.stream};
    const WaitResult r = guarded_wait(
        [&](uint64_t spins) {
            while (t < n && e->walk.tile_ready(s, t, seq)) ++t;
            if (t == n) return true;
            if ((spins & 7) == 1)
                for (uint32_t u = t + 1; u < n; ++u) e->walk.prefetch_tile(s, u);
            return false;
        },
        NoSideCheck{}, sq);
    return svc_wait_rc(r, sq);
}

// The request number after q. Never 0 (the done words' initial value) or
// kSvcStop, and never a value whose low 30 bits are 0: the compaction tiles
// tag their look-back granules with seq & 0x3FFFFFFF (0 -> 1), so 2^30 would
// share its tag with the request after it and a tile could take that request
// predecessor's stale granule as current.
uint32_t next_seq(uint32_t q) {
    uint32_t s = q + 1;
    while (s == 0 || s == jsp::kSvcStop || (s & 0x3FFFFFFFu) == 0) ++s;
    return s;
}


// Wait for the last snapshot patch's completion word (the rows are then in
// memory for every later reader, the resident tiles' `sc1` loads included).
// A patch held back for the next request, posted on its own now (a service
// that has left meanwhile is caught by patch_wait, and the patch kernel
// applies it).
void patch_post_deferred(jsp_engine* e) {
    if (!e->patch_deferred) return;
    e->patch_deferred = false;
    auto& v = e->svc;
    const uint32_t seq = next_seq(v.seq);
    v.seq = seq;
    v.last = std::chrono::steady_clock::now();
    svc_request(e, seq, e->patch_bits | jsp::kReqPatchOnly, e->patch_nf, e->patch_micro);
    lease_posted(e, seq, false);  // a patch alone: no tile answers it
    e->patch_req = seq;
    // applied on its own: the next request's tiles reload the rows
    v.rows_dirty |= v.micro_dirty;
    v.micro_dirty = false;
}

int patch_wait(jsp_engine* e) {
    if (!e->patch_pending) return JSP_OK;
    e->wake_job = false;  // a reader other than a placement: no wake, the patch lands now
    if (e->patch_deferred && !e->svc.running) {
        // held back for a service that is not up: the patch kernel applies it
        e->patch_deferred = false;
        e->patch_svc = false;
        if (int rc = use_engine_stream(e)) return rc;
        e->patch_target += (e->last_patch.n + 255) / 256;
        e->last_patch.target = e->patch_target;
        HIP_TRY(jsp::launch_patch(e->last_patch, e->stream));
    }
    patch_post_deferred(e);
    const uint32_t* w = e->h_patch_done.as<uint32_t>();
    const auto t0 = std::chrono::steady_clock::now();
    const auto limit = std::chrono::duration<double, std::milli>(2.0 * svc_idle_ms() + 100.0);
    // (not a guarded_wait: it relaunches the patch and stops the service from inside its loop)
    for (uint64_t spins = 1; __atomic_load_n(w, __ATOMIC_ACQUIRE) != e->patch_seq; ++spins) {
        if ((spins & 255) == 0 && e->patch_svc) {
            // posted to the dispatcher: if the service left without taking it
            // (an idle exit racing the post), apply it with the patch kernel.
            // A live service that never takes it (bounded: it polls every few
            // microseconds) is stopped, and the patch kernel applies it too
            // (the staged delta is unchanged: writing it twice writes the
            // same values)
            const hipError_t q = hipStreamQuery(e->svc.stream);
            if (q == hipErrorNotReady && std::chrono::steady_clock::now() - t0 < limit) continue;
            if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == e->patch_seq) break;
            e->patch_svc = false;
            if (q == hipErrorNotReady) {
                e->svc.pending = 0;
                if (int rc = svc_stop(e)) return rc;  // patch_svc is off: the stop does not wait for it
            }
            e->svc.running = false;
            lease_drop(e);
            if (int rc = use_engine_stream(e)) return rc;
            e->patch_target += (e->last_patch.n + 255) / 256;
            e->last_patch.target = e->patch_target;
            HIP_TRY(jsp::launch_patch(e->last_patch, e->stream));
            continue;
        }
        if ((spins & 255) == 0) {
            const hipError_t q = hipStreamQuery(e->stream);
            if (q == hipErrorNotReady) continue;
            if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == e->patch_seq) break;
            e->patch_pending = false;
            if (q == hipSuccess) return set_err(JSP_EHIP, "snapshot patch %u ended without its completion word", e->patch_seq);
            return set_err(JSP_EHIP, "snapshot patch %u failed: %s", e->patch_seq, hipGetErrorString(q));
        }
    }
    e->patch_pending = false;
    e->patch_svc = false;
    return JSP_OK;
}

// Launches that read the rows are stream-ordered after a patch kernel, but
// not after a patch the service applies: they wait for its word first.
int patch_fence(jsp_engine* e) { return e->patch_pending && e->patch_svc ? patch_wait(e) : JSP_OK; }

// How patches reach the resident service's dispatcher: posted at once, so the
// dispatcher applies them during the gap before the next request (a
// recovery's deletions take milliseconds), and a request posted before the
// patch's completion word came back carries it again (applying a staged
// patch twice writes the same values; the request may have replaced the
// patch's own in the mailbox).

// A snapshot patch is the first sign of a recovery: the watch events of the
// deleted Jobs' pods arrive while the reconciler deletes them in the
// foreground, before it recreates and places them
// (pkg/controllers/jobset_controller.go:553-576, 698-709). When the host API
// has been answered by the resident service (armed), a patch (re)starts it
// here without waiting: the GPU wakes from idle and the grid comes up while
// the deletions finish, and the recreate's jsp_place finds it polling.
// Whether a patch should (re)start the service: the host API has been
// answered by it and it is not up (or about to idle out).
bool svc_wake_wanted(jsp_engine* e) {
    auto& v = e->svc;
    if (!v.armed || !svc_ok(e)) return false;
    const double since = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - v.last).count();
    return !(v.running && since <= 0.5 * idle_ms(e));
}

// (Re)start the service without waiting for its dispatcher to poll. Long
// idle (a recovery after hours): the service has left by itself and its
// stream is done -- a query, not a synchronize, tells; otherwise it is
// stopped. On failure it stays stopped (the next jsp_place starts it, or
// answers on the launch path) and the error is dropped.
int svc_restart_quiet(jsp_engine* e) {
    auto& v = e->svc;
    const double since = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - v.last).count();
    if (v.running && since > idle_ms(e) + 5.0 && hipStreamQuery(v.stream) == hipSuccess) {
        v.running = false;
        v.pending = 0;
        lease_drop(e);
        e->grave.flush();
    }
    if (svc_stop(e) != JSP_OK || svc_start(e, 0, false) != JSP_OK) {
        (void)svc_stop(e);
        g_err.clear();
        return JSP_EHIP;
    }
    v.resume = false;
    return JSP_OK;
}

void svc_wake(jsp_engine* e) {
    auto& v = e->svc;
    if (!svc_wake_wanted(e) || svc_restart_quiet(e) != JSP_OK) return;
    // A warm-up request (no jobs, rows marked patched): the fresh tiles load
    // their rows, run every phase once and pull the kernel's code into the
    // instruction caches while the deletions finish, so the recreate's
    // request runs warm. Posted without waiting (the dispatcher finds it when
    // it starts polling); the next request settles it first (svc_settle).
    const uint32_t seq = next_seq(v.seq);
    v.seq = seq;
    v.last = std::chrono::steady_clock::now();
    svc_request(e, seq, jsp::kReqDirty, 0u);
    lease_posted(e, seq, v.shape == 2 && v.bitmap);  // (rows_dirty stays set: no lease from these lines)
    // rows marked patched, and they stay marked: the patch kernel may not
    // have landed when the warm-up loads them, so the next request (which
    // waits for the patch's completion word) loads them again
    v.pending = seq;
}

// The waker's job (or the next caller's, whichever takes the engine lock
// first): restart the service, post the held-back patch and, for the tile
// shapes, a warm-up request (no jobs) behind it -- the fresh tiles load the
// patched rows and pull the code into the instruction caches while the
// deletions finish, so the recreate's request runs warm. A patch already
// taken care of (patch_wait) leaves nothing to do; a start that fails
// leaves the patch held back, and patch_wait hands it to the patch kernel.
void run_wake(jsp_engine* e) {
    if (!e->wake_job) return;
    e->wake_job = false;
    if (!(e->patch_pending && e->patch_svc && e->patch_deferred)) return;
    const auto t0 = std::chrono::steady_clock::now();
    if (svc_restart_quiet(e) != JSP_OK) return;
    auto& v = e->svc;
    const uint32_t seq = next_seq(v.seq);
    v.seq = seq;
    v.last = std::chrono::steady_clock::now();
    svc_request(e, seq, e->patch_bits | jsp::kReqDirty, (e->patch_bits & jsp::kReqPatchInline) ? e->patch_nf : 0u,
                e->patch_micro);
    lease_posted(e, seq, v.shape == 2 && v.bitmap);  // its lines are the patched rows' (the lease's recovery case)
    e->patch_req = seq;
    e->patch_deferred = false;
    v.pending = seq;
    v.rows_dirty = v.micro_dirty = false;  // the warm-up loads the patched rows
    e->acc.wake_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

// The waker's loop. While the service is armed (a placement it answered may
// be followed by a recovery's first patch, hours later) the waker polls the
// ring every waker_poll_us (200 us: ~5k sleeps a second, ~1 % of one core),
// so the patch call that rings it only stores a flag -- a futex wake from a
// core that slept was the default service's cold-recovery tail (patch call
// p95 9.9 us against 4.7 us with no wake, profiles/r06/g2). Otherwise it
// sleeps on wake_cv. The ring is consumed whichever way it arrives; a ring
// the waker has not taken yet is run by the next placement itself (run_wake).
void waker_main(jsp_engine* e) {
    // Normal priority: at SCHED_IDLE (measured, profiles/r05) a waker
    // preempted while it held the engine lock stalled the next placement by
    // milliseconds (a 5.2 ms cold-recovery p99 on a shared host).
    (void)hipSetDevice(e->device);
    const auto period = std::chrono::microseconds(e->hooks.waker_poll_us);
    for (;;) {
        if (e->wake_quit.load(std::memory_order_acquire)) return;
        if (e->wake_ring.exchange(false, std::memory_order_acq_rel)) {
            std::lock_guard<std::mutex> g(e->mu);
            run_wake(e);
            continue;
        }
        if (period.count() > 0 && e->waker_poll.load(std::memory_order_acquire)) {
            e->waker_polling.store(true, std::memory_order_release);
            std::this_thread::sleep_for(period);
            continue;
        }
        e->waker_polling.store(false, std::memory_order_release);
        std::unique_lock<std::mutex> l(e->wake_mu);
        e->wake_cv.wait_for(l, std::chrono::milliseconds(50), [e, period] {
            return e->wake_ring.load() || e->wake_quit.load() || (period.count() > 0 && e->waker_poll.load());
        });
    }
}

// The waker thread, created with the engine's first service (thread creation
// costs ~100 us, which must never land in a recovery's patch call).
void start_waker(jsp_engine* e) {
    if (!e->waker.joinable()) e->waker = std::thread(waker_main, e);
}

// Hand the wake to the waker thread. Called with mu held; the caller delivers
// it (notify_waker) after releasing mu, so the waker never wakes into a held
// lock.
void ring_waker(jsp_engine* e) {
    e->wake_job = true;
    start_waker(e);
    e->wake_ring.store(true, std::memory_order_release);
    if (e->waker_polling.load(std::memory_order_acquire)) return;  // it polls: no notify
    {
        std::lock_guard<std::mutex> l(e->wake_mu);  // no lost wake-up between its predicate and its wait
    }
    e->wake_notify.store(true, std::memory_order_relaxed);
}

// The service became armed: the waker leaves its condition variable for its
// polling loop (once per arming; a waiter that misses it polls within 50 ms).
void notify_waker_poll(jsp_engine* e) { e->wake_cv.notify_one(); }

// Deliver a ring (mu not held). Keeping the waker off the ringing thread's
// CPU (an affinity change when the caller's CPU changed) was measured and
// dropped: the affinity call costs the patch call 6-15 us at p50
// (profiles/r05/probes/cold4_waker_affinity_ab.txt).
void notify_waker(jsp_engine* e) {
    if (!e->wake_notify.exchange(false, std::memory_order_relaxed)) return;
    e->wake_cv.notify_one();
}

// Whether the lines of the last posted request may answer a placement on the
// host (the lease): the compaction service's bitmap answer
// with the stamps off, that request the service's latest and settled, posted
// after the last change (lease_drop) with no patch marked against the tiles'
// rows, and recent enough that the service is not near its idle exit.
bool lease_ok(const jsp_engine* e, int shape, std::chrono::steady_clock::time_point now) {
    const auto& v = e->svc;
    const auto& l = e->lease;
    return e->hooks.svc_standing == 3 && shape == 2 && v.shape == 2 && v.bitmap && !e->timing && !v.clk && v.running &&
           !v.pending_ready && v.pending == 0 && l.seq != 0 && l.seq == v.seq && l.posted == l.gen && !v.rows_dirty &&
           !v.micro_dirty && !e->patch_deferred && !e->wake_job &&
           std::chrono::duration<double, std::milli>(now - v.last).count() <= 0.25 * idle_ms(e);
}

// One placement answered on the host under the lease (lease_ok holds, no
// patch is pending): from the lines themselves for a lease's first host
// answer (a recovery's place writes no line of a list), from the kept list
// from the second on (DESIGN.md §4.3 "the kept list"). The second builds it
// with its own J; a later call that asks for more than an incomplete list
// holds builds it again with that J, never further than asked. Every answer
// checks the error word and the tags of the lines the list was built from.
// false: a line with another tag, or an error word -- the lease is dropped
// and the request goes to the device, as ever.
bool lease_answer(jsp_engine* e, uint32_t J, int32_t* assign_out, uint32_t* placed) {
    auto& v = e->svc;
    auto& l = e->lease;
    auto& m = e->memo;
    const unsigned long long* b = v.bits.as<unsigned long long>();
    bool whole = __atomic_load_n(v.words.as<uint32_t>() + v.nb + 2, __ATOMIC_ACQUIRE) == v.err_ack;
    if (whole && (!l.held || !e->hooks.lease_memo)) {
        uint32_t t = 0, j = 0;
        whole = expand_lines(b, v.nb, e->blk_l0.data(), e->leaf_begin, l.seq, J, assign_out, &t, &j, [] {});
        if (whole) {
            for (uint32_t i = j; i < J; ++i) assign_out[i] = -1;
            *placed = j;
        }
    } else if (whole) {
        if (m.gen != l.gen || m.seq != l.seq || (J > m.n_list && !m.complete)) {
            if (m.list.size() < 256u * (size_t)v.nb) m.list.resize(256u * (size_t)v.nb);
            uint32_t t = 0, j = 0;
            whole = expand_lines(b, v.nb, e->blk_l0.data(), e->leaf_begin, l.seq, J, m.list.data(), &t, &j, [] {});
            m.n_list = j;
            m.lines_used = t;
            m.complete = j < J;  // the lines ran out first (J reached: there may be more leaves)
            m.gen = whole ? l.gen : 0;
            m.seq = l.seq;
            m.built += whole ? 1 : 0;
        } else {
            whole = lines_tagged(b, m.lines_used, l.seq);
        }
        if (whole) {
            list_answer(m.list.data(), m.n_list, J, assign_out, placed);
            m.answered += 1;
        }
    }
    if (!whole) {
        lease_drop(e);
        return false;
    }
    if (!l.held) {
        l.held = true;
        l.taken += 1;
    }
    l.answered += 1;
    e->acc.svc_calls += 1;
    return true;
}

// One placement through the service: J jobs of the engine's one class. t0 is
// the call's entry stamp (jsp_place) and shape the service's for the engine's
// state (svc_shape). *leased: answered on the host with no clock read and no
// HIP call here (the caller accounts the call's wall); otherwise *t_svc is
// the stamp at which the service path proper began, and the device is set.
int svc_place(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, uint32_t J,
              int32_t* assign_out, uint32_t* placed, std::chrono::steady_clock::time_point t0, int shape,
              bool* leased, std::chrono::steady_clock::time_point* t_svc) {
    auto& v = e->svc;
    *leased = false;
    // The lease's own entry: nothing queued or pending that the steps below
    // would have to run first (a wake, a patch, a start, an early answer's
    // tiles), no reason to restart, and lease_ok by the entry stamp.
    if (J > 0 && !e->patch_pending && J <= v.cap && v.blocks == e->n_blocks && lease_ok(e, shape, t0) &&
        lease_answer(e, J, assign_out, placed)) {
        *leased = true;
        return JSP_OK;
    }
    if (hipSetDevice(e->device) != hipSuccess) return set_err(JSP_EHIP, "hipSetDevice(%d) failed", e->device);
    const auto t_in = std::chrono::steady_clock::now();
    *t_svc = t_in;
    const bool wake = e->wake_job;
    run_wake(e);  // a recovery's wake the waker has not run yet: run it here
    const auto now = wake ? std::chrono::steady_clock::now() : t_in;
    bool restart = !v.running || J > v.cap || v.clk != e->timing || v.blocks != e->n_blocks || v.shape != shape ||
                   std::chrono::duration<double, std::milli>(now - v.last).count() > 0.5 * idle_ms(e);
    // the request's tiles must read the patched rows: a patch held back for
    // the running service rides on this request (its dispatcher applies it
    // before ringing the tiles); any other is waited for
    bool carry = !restart && e->patch_pending && e->patch_svc;
    if (!carry)
        if (int rc = patch_wait(e)) return rc;
    // A cold start -- the first request after an idle exit (recoveries are
    // hours apart, and a recovery's first patch has normally restarted it
    // already), an upload or a geometry change -- launches the service, waits
    // for its dispatcher to poll and posts to it. Measured after 60 ms idle on
    // MI355X (profiles/r03): cfg2 p50 33 us, max 67 us this way, against 66 /
    // 428 us when the launch path answered the cold call while the service
    // came up -- the polling dispatcher brings the GPU out of its idle state
    // while the host waits, and a launch after idling pays that wake-up inside
    // the kernel.
    if (!restart) {
        if (int rc = svc_wait_ready(e)) return rc;
        if (int rc = svc_settle(e)) return rc;
        if (!v.running) {  // the settle stopped it (kSvcFailed): a fresh start, the patch applied first
            restart = true;
            if (carry) {
                carry = false;
                if (int rc = patch_wait(e)) return rc;
            }
        }
    }
    // The host lease: the lines of the request with v.seq are
    // whole (svc_settle returned) and nothing they depend on changed since it
    // was posted, so they are this request's answer as well. Within a quarter
    // of the idle limit only: a host answer does not refresh v.last, so the
    // request that follows crosses the link well before the restart test
    // above would stop the service, keeps it alive and renews the lease.
    if (!restart && J > 0 && lease_ok(e, shape, now)) {
        // a patch the wake's warm-up carried (run_wake): landed when its word is
        // back -- the warm-up's lines, tagged after it, are the patched rows'
        if (e->patch_pending && e->patch_svc && !e->patch_deferred &&
            __atomic_load_n(e->h_patch_done.as<uint32_t>(), __ATOMIC_ACQUIRE) == e->patch_seq) {
            if (int rc = patch_wait(e)) return rc;  // at once: bookkeeping only
            carry = false;
        }
        // (a call that had something to settle first -- the recovery's place
        // behind the warm-up, an early answer's last tiles: its phase clocks
        // as ever)
        if (!e->patch_pending && v.running && lease_answer(e, J, assign_out, placed)) {
            e->acc.svc_pre_us += std::chrono::duration<double, std::micro>(now - t_in).count();
            e->acc.svc_answer_us +=
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - now).count();
            return JSP_OK;
        }
    }
    if (carry) {  // held back, or posted and its completion word not back yet
        // (a posted patch the dispatcher has taken is applied before it takes
        // this request: no need to carry it again)
        const uint32_t* pw = e->h_patch_done.as<uint32_t>();
        carry = e->patch_deferred || (__atomic_load_n(pw, __ATOMIC_ACQUIRE) != e->patch_seq &&
                                      __atomic_load_n(pw + 16, __ATOMIC_ACQUIRE) != e->patch_req);
        e->patch_deferred = false;
    }
    // the compaction answer is read from its tagged entries (timing on: the
    // done words, which carry the per-tile stamps)
    // (timing on too: the stamps are read once the tiles' done words are in)
    const bool early = shape == 2 && J > 0;
    uint32_t seq = 0, n_early = 0;
    bool all_tiles = false;
    std::chrono::steady_clock::time_point t_post{};
    for (int attempt = 0;; ++attempt) {
        if (restart) {
            if (int rc = svc_stop(e)) return rc;
            if (int rc = svc_start(e, J, true)) return rc;
        }
        seq = next_seq(v.seq);
        v.seq = seq;
        v.last = std::chrono::steady_clock::now();
        // second half first: the dispatcher reads both halves in one 16-byte
        // load (an inline patch carried here: its n | flags in place of n_runs,
        // which the tiles do not read)
        const uint32_t w2 = carry && (e->patch_bits & jsp::kReqPatchInline) ? e->patch_nf : n_runs;
        // the tiles keep their rows on chip: bit 31 of J tells them the
        // snapshot was patched since their previous request (J < 2^28)
        // (a micro-patch carried here: the dispatcher hands its rows to the
        // resident tiles, or marks the rows patched itself)
        const bool micro = carry && e->patch_micro;
        const bool dirty = v.rows_dirty || (v.micro_dirty && !micro);
        const uint32_t jw = J | (dirty ? jsp::kReqDirty : 0u) | (carry ? e->patch_bits : 0u);
        carry = false;  // a retry finds it applied, or applied by the patch kernel (patch_wait)
        v.rows_dirty = v.micro_dirty = false;
        if (attempt == 0) {
            t_post = std::chrono::steady_clock::now();
            e->acc.svc_pre_us += std::chrono::duration<double, std::micro>(t_post - t_in).count();
        }
        svc_request(e, seq, jw, w2, micro);
        lease_posted(e, seq, v.shape == 2 && v.bitmap);
        // (the split shape, timing off and J > 0: its tagged lines; with the
        // stamps on, the done words, which follow the stamps)
        const int rc = !early ? (v.shape == 3 && !v.clk && J > 0 ? svc_wait_split(e, seq) : svc_wait(e, seq, J))
                       : v.bitmap ? svc_wait_bits(e, seq, J, assign_out, &n_early, &all_tiles)
                                  : svc_wait_entries(e, seq, J, assign_out, &n_early);
        if (rc == kSvcFailed) {
            const uint32_t ew = __atomic_load_n(v.words.as<uint32_t>() + v.nb + 2, __ATOMIC_ACQUIRE);
            v.err_ack = ew;
            (void)svc_stop(e);
            return set_err(JSP_EHIP, "placement service request %u failed: %s; its assign[] is invalid", seq,
                           (ew & jsp::kErrKindMask) == jsp::kErrMicro
                               ? "a resident tile's wait for the request's micro-patch rows gave up"
                               : "the compaction look-back timed out");
        }
        if (rc == kSvcGone && attempt == 0) {
            v.running = false;
            lease_drop(e);
            restart = true;
            continue;
        }
        if (rc == kSvcGone) {
            lease_drop(e);
            return set_err(JSP_EHIP, "placement service left before answering request %u", seq);
        }
        if (rc) return rc;
        break;
    }
    e->acc.svc_answer_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_post).count();
    if (early && J > 0) e->acc.svc_first_us += std::chrono::duration<double, std::micro>(v.first_seen - t_post).count();
    if (v.clk && v.nb > 0) {
        if (early) {  // the tiles' stamps land with their done words
            v.pending = seq;
            if (int rc = svc_settle(e)) return rc;
        }
        // the request's device time: first tile saw it -> last tile drained
        const uint32_t* clk = v.words.as<uint32_t>() + v.nb + 3;
        const uint32_t ref = clk[0];
        int32_t lo = 0, hi = 0;
        for (uint32_t t = 0; t < v.nb; ++t) {
            lo = std::min(lo, (int32_t)(clk[jsp::kSvcClkSlots * t] - ref));
            hi = std::max(hi, (int32_t)(clk[jsp::kSvcClkSlots * t + 5] - ref));
        }
        e->acc.svc_us += (double)(hi - lo) / 100.0;
        std::lock_guard<std::mutex> l(e->met_mu);
        hist_add(e->met.device_us, (double)(hi - lo) / 100.0, JSP_HIST_LO_US);
    }
    if (v.shape == 3) {  // the tiles answered: the walk, into the caller's buffer
        const auto tw = std::chrono::steady_clock::now();
        *placed = e->walk.place(v.split.as<uint64_t>(), run_class, run_len, n_runs, assign_out);
        // the host walk's share of the wait (jsp_timing.host_post_us on this path)
        e->acc.host_post_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tw).count();
        e->acc.svc_calls += 1;
        return JSP_OK;
    }
    if (early) {
        v.pending = all_tiles ? 0u : seq;
        *placed = n_early;
        e->acc.svc_calls += 1;
        return JSP_OK;
    }
    const uint32_t* w = v.words.as<uint32_t>();
    const uint32_t ew = __atomic_load_n(w + v.nb + 2, __ATOMIC_ACQUIRE);
    if (ew != v.err_ack) {
        v.err_ack = ew;
        (void)svc_stop(e);
        return set_err(JSP_EHIP, "placement service request %u failed: the compaction look-back timed out; "
                                 "its assign[] is invalid", seq);
    }
    const auto tc = std::chrono::steady_clock::now();
    {  // u64 entries: the domain is the low half
        const unsigned long long* a = v.assign.as<unsigned long long>();
        for (uint32_t j = 0; j < J; ++j) assign_out[j] = (int32_t)(uint32_t)a[j];
    }
    // (the bitmap answer writes no stats: it runs this path only for J = 0)
    *placed = v.bitmap ? 0u : __atomic_load_n(w + v.nb + 1, __ATOMIC_ACQUIRE);
    // the copy-out's share of the wait (jsp_timing.host_post_us on this path)
    e->acc.host_post_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tc).count();
    e->acc.svc_calls += 1;
    return JSP_OK;
}

// ---- micro-patches (jsp_internal.h kMailbox*)
// Whether the resident service is up and fresh enough to take a patch
// through its dispatcher (not about to idle out, the engine's shape).
bool svc_up(jsp_engine* e) {
    auto& v = e->svc;
    const double since = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - v.last).count();
    return v.running && since <= 0.5 * idle_ms(e) && svc_ok(e) && svc_shape(e) == v.shape;
}

// Merge n rows of one patch call (columns fl) into the held micro-patch: a
// row already held takes the new values, a new row is appended. All or
// nothing: false when the rows do not fit.
bool micro_merge(jsp_engine* e, const uint32_t* rows, uint32_t n, const uint64_t* labels, const uint32_t* taints,
                 const uint32_t* free_res, const int32_t* excl) {
    const uint32_t W = e->W, R = e->R, rw = jsp::micro_row_words(W, R), cap = jsp::micro_rows_max(W, R);
    uint32_t w[jsp::kMailboxPayload];
    std::memcpy(w, e->micro_w, sizeof w);
    uint32_t m = e->micro_n;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t r = 0;
        while (r < m && w[r * rw] != rows[i]) ++r;
        if (r == m) {
            if (m == cap) return false;
            std::memset(w + r * rw, 0, rw * 4);
            w[r * rw] = rows[i];
            ++m;
        }
        uint32_t* x = w + r * rw;
        if (labels)
            for (uint32_t k = 0; k < W; ++k) {
                const uint64_t l = labels[(size_t)k * n + i];
                x[1 + 2 * k] = (uint32_t)l;
                x[2 + 2 * k] = (uint32_t)(l >> 32);
            }
        if (taints) x[1 + 2 * W] = taints[i];
        if (free_res)
            for (uint32_t k = 0; k < R; ++k) x[2 + 2 * W + k] = free_res[(size_t)k * n + i];
        if (excl) x[2 + 2 * W + R] = (uint32_t)excl[i];
    }
    std::memcpy(e->micro_w, w, sizeof w);
    e->micro_n = m;
    return true;
}

// The held micro-patch in its kernel form too (engine staging, pinned): the
// patch kernel applies it if the service leaves before a request carries it.
int micro_stage_kernel_form(jsp_engine* e) {
    const uint32_t W = e->W, R = e->R, rw = jsp::micro_row_words(W, R), m = e->micro_n, fl = e->micro_fl;
    const jsp::PatchInlineLayout L = jsp::patch_inline_layout(m, 15u, W, R);
    HIP_TRY(e->h_patch.reserve(L.bytes, grave(e)));
    char* hp = static_cast<char*>(e->h_patch.p) - 64;  // the inline layout without its header
    for (uint32_t r = 0; r < m; ++r) {
        const uint32_t* x = e->micro_w + r * rw;
        reinterpret_cast<uint32_t*>(hp + L.rows)[r] = x[0];
        for (uint32_t k = 0; k < W; ++k)
            reinterpret_cast<uint64_t*>(hp + L.lab)[(size_t)k * m + r] = ((uint64_t)x[2 + 2 * k] << 32) | x[1 + 2 * k];
        reinterpret_cast<uint32_t*>(hp + L.taint)[r] = x[1 + 2 * W];
        for (uint32_t k = 0; k < R; ++k) reinterpret_cast<uint32_t*>(hp + L.free)[(size_t)k * m + r] = x[2 + 2 * W + k];
        reinterpret_cast<uint32_t*>(hp + L.excl)[r] = x[2 + 2 * W + R];
    }
    jsp::PatchArgs& a = e->last_patch;
    a = jsp::PatchArgs{};
    a.rows = reinterpret_cast<const uint32_t*>(hp + L.rows);
    a.n = m;
    a.npad = e->npad;
    a.W = W;
    a.R = R;
    a.dlab = (fl & jsp::kPatchLab) ? reinterpret_cast<const uint64_t*>(hp + L.lab) : nullptr;
    a.dtaint = (fl & jsp::kPatchTaint) ? reinterpret_cast<const uint32_t*>(hp + L.taint) : nullptr;
    a.dfree = (fl & jsp::kPatchFree) ? reinterpret_cast<const uint32_t*>(hp + L.free) : nullptr;
    a.dexcl = (fl & jsp::kPatchExcl) ? reinterpret_cast<const int32_t*>(hp + L.excl) : nullptr;
    a.labels = e->labels.as<uint64_t>();
    a.taints = e->taints.as<uint32_t>();
    a.freer = e->freer.as<uint32_t>();
    a.excl = e->excl.as<int32_t>();
    a.counter = e->patch_ctr.as<unsigned long long>();
    a.done = e->h_patch_done.as<uint32_t>();
    a.seq = e->patch_seq;
    return JSP_OK;
}

// Host-side validation of a run list; returns the job count through *J.
int check_runs(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, uint64_t* J) {
    uint64_t n = 0;
    for (uint32_t i = 0; i < n_runs; ++i) {
        if (run_class[i] >= e->C) return set_err(JSP_EINVAL, "run %u: class %u out of range (%u classes)", i,
                                                  run_class[i], e->C);
        n += run_len[i];
    }
    if (n > (1u << 30)) return set_err(JSP_ERANGE, "%llu jobs exceed the 2^30 limit", (unsigned long long)n);
    *J = n;
    return JSP_OK;
}

// The f64 reciprocal r of d >= 2 with floor(double(n) * r) == floor(n / d)
// for every u32 n (the device truncates fl(n * r) to u32). With r = (1/d)(1 + e):
// fl(n * r) >= n/d needs e above the two roundings (2^-52); below q + 1 it
// needs (n/d)(1 + e + 2^-52) < q + 1, i.e. e < 1/(n + d) - 2^-52, which holds
// for e < 2^-34 as n + d < 2^33. r = fl(fl(1/d) (1 + 2^-45)) has e within
// 2^-45 +- 2^-52. tests/test_engine_gpu.py checks the edges (n = kd - 1, kd).
double divisor_rcp(uint32_t d) { return d >= 2 ? (1.0 / (double)d) * (1.0 + 0x1p-45) : d == 1 ? 1.0 : 0.0; }

int ready(jsp_engine* e, bool need_cls) {
    if (!e->have_topo) return set_err(JSP_ESTATE, "no topology uploaded");
    if (!e->have_snap) return set_err(JSP_ESTATE, "no snapshot uploaded");
    if (need_cls && !e->have_cls) return set_err(JSP_ESTATE, "no job classes uploaded");
    return JSP_OK;
}

// The entry frame of `call`, which runs on one device with topology, snapshot
// and classes loaded: a device-set engine is refused before the lock, g takes
// the engine's lock (and holds it when a later check refuses), and with
// `whole` a sharded engine is refused too.
int single_engine(jsp_engine* e, const char* call, std::unique_lock<std::mutex>& g, bool whole = true) {
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: %s runs on a single-device engine", call);
    g = std::unique_lock<std::mutex>(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (whole && (e->leaf_begin != 0 || e->n_leaves != e->L_total))
        return set_err(JSP_ESTATE, "sharded engine: %s needs the whole snapshot on one engine", call);
    return JSP_OK;
}

// A host call's run list: its buffers, its classes (check_runs) and the job
// count, which check_runs has bounded by 2^30.
int run_front(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, uint32_t* J) {
    if (n_runs > 0 && (!run_class || !run_len)) return set_err(JSP_EINVAL, "run buffers are NULL");
    uint64_t J64 = 0;
    if (int rc = check_runs(e, run_class, run_len, n_runs, &J64)) return rc;
    *J = (uint32_t)J64;
    return JSP_OK;
}

// A host call enters the engine stream (*s): a pending launch error is
// reported first; a call that writes rows settles the resident service's last
// request (no tile may still be reading them) and gives up the host's lease on
// the standing answer; then the stream is ordered after every pending patch
// (one the service's dispatcher applies is posted alone and waited for). The
// service itself stays as it is.
int enter_engine_stream(jsp_engine* e, bool writes_rows, hipStream_t* s) {
    if (int rc = check_launch_error(e)) return rc;
    if (writes_rows) {
        if (int rc = svc_settle(e)) return rc;
        lease_drop(e);
    }
    if (int rc = use_engine_stream(e)) return rc;
    *s = e->stream;
    return JSP_OK;
}

// The whole snapshot's tally into the engine's cap / occ.
int tally_whole(jsp_engine* e, hipStream_t s) {
    uint32_t* cap = e->cap.as<uint32_t>();
    uint32_t* occ = e->occ.as<uint32_t>();
    if (e->n_blocks == 0) {  // no rows: the tally launches nothing
        HIP_TRY(hipMemsetAsync(cap, 0, (size_t)e->C * e->L_total * 4, s));
        HIP_TRY(hipMemsetAsync(occ, 0, (size_t)e->L_total * 4, s));
    }
    return tally_impl(e, cap, occ, e->L_total, s);
}

// The metrics of a finished placement call that took `us` and returned rc.
int record_placement(jsp_engine* e, double us, int rc, uint32_t jobs, uint32_t placed) {
    std::lock_guard<std::mutex> l(e->met_mu);
    hist_add(e->met.place_us, us, JSP_HIST_LO_US);
    if (rc != JSP_OK) {
        e->met.place_errors += 1;
        return rc;
    }
    hist_add(e->met.batch_jobs, (double)jobs, JSP_HIST_LO_JOBS);
    e->met.placed += placed;
    e->met.unplaceable += jobs - placed;
    return rc;
}

// The arguments every timing loop takes.
int check_timed(uint32_t iters, uint32_t max_iters, const double* out_us) {
    if (iters == 0 || iters > max_iters) return set_err(JSP_EINVAL, "iters %u out of range [1,%u]", iters, max_iters);
    if (!out_us) return set_err(JSP_EINVAL, "out_us is NULL");
    return JSP_OK;
}

// out[0] median and out[1] p99, in microseconds, of the samples (integer
// nanoseconds): what sorting their us_between values gives at ranks
// iters / 2 and min(iters - 1, (size_t)(0.99 iters)), selected without the
// sort (jsp_select.h).
void median_p99(const std::vector<int64_t>& ns, double* out) { select_median_p99(ns.data(), ns.size(), out); }

// `iters` back-to-back calls of step(i) by the host clock: out_us[0] the
// total, [1] the median and [2] the p99 call.
template <class Step>
int timed_calls(uint32_t iters, double* out_us, Step step) {
    std::vector<int64_t> ns(iters);
    const auto t0 = std::chrono::steady_clock::now();
    auto tp = t0;
    for (uint32_t i = 0; i < iters; ++i) {
        if (int rc = step(i)) return rc;
        const auto t = std::chrono::steady_clock::now();
        ns[i] = (t - tp).count();
        tp = t;
    }
    out_us[0] = us_between(t0, tp);
    median_p99(ns, out_us + 1);
    return JSP_OK;
}

// At least n event pairs in e->tev.
int timing_events(jsp_engine* e, size_t n) {
    while (e->tev.size() < n) {
        EvPair p;
        HIP_TRY(hipEventCreate(&p.a));
        HIP_TRY(hipEventCreate(&p.b));
        e->tev.push_back(p);
    }
    return JSP_OK;
}

// Device time of rep(leg) for each of `legs`: ten warm-up repetitions, then
// the first event pair (timing_events) around `iters` more; out_us[leg]
// microseconds per repetition.
template <class Rep>
int time_legs(jsp_engine* e, hipStream_t s, int legs, uint32_t iters, double* out_us, Rep rep) {
    for (int leg = 0; leg < legs; ++leg) {
        for (uint32_t i = 0; i < 10 + iters; ++i) {
            if (i == 10) HIP_TRY(hipEventRecord(e->tev[0].a, s));
            if (int rc = rep(leg)) return rc;
        }
        HIP_TRY(hipEventRecord(e->tev[0].b, s));
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->tev[0].a, e->tev[0].b));
        out_us[leg] = (double)ms * 1e3 / iters;
    }
    return JSP_OK;
}

// `iters` back-to-back device steps on the engine stream, each bracketed by
// a start event on its first dispatch and a stop event on its last
// (hipExtLaunchKernel: the dispatch packets' own timestamps, as a kernel
// trace reports them -- no host submit time, no marker packets). With a
// scrub buffer, a read-only sweep of it precedes every step (cold caches).
// out_us[0] median, out_us[1] mean over the steps.
template <class Step>
int time_steps(jsp_engine* e, uint32_t iters, const void* d_scrub, size_t scrub_bytes, double* out_us, Step step) {
    if (int rc = check_timed(iters, 4096, out_us)) return rc;
    if (scrub_bytes > 0 && !d_scrub) return set_err(JSP_EINVAL, "scrub buffer is NULL");
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    if (int rc = timing_events(e, iters)) return rc;
    if (scrub_bytes > 0) HIP_TRY(e->tmp_scrub.reserve(64, grave(e)));
    int rc = JSP_OK;
    for (uint32_t i = 0; i < iters && rc == JSP_OK; ++i) {
        if (scrub_bytes > 0) HIP_TRY(jsp::launch_scrub(d_scrub, scrub_bytes, e->tmp_scrub.as<uint32_t>(), s));
        jsp::set_launch_start(e->tev[i].a);
        jsp::set_launch_stop(e->tev[i].b);
        rc = step(s);
        jsp::set_launch_start(nullptr);
        jsp::set_launch_stop(nullptr);
    }
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<double> us(iters);
    double sum = 0.0;
    for (uint32_t i = 0; i < iters; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->tev[i].a, e->tev[i].b));
        us[i] = ms * 1e3;
        sum += us[i];
    }
    std::sort(us.begin(), us.end());
    out_us[0] = us[iters / 2];
    out_us[1] = sum / iters;
    return check_launch_error(e);
}
}  // namespace

extern "C" {

int jsp_abi_version(void) { return JSP_ABI_VERSION; }

const char* jsp_last_error(void) { return g_err.c_str(); }

int jsp_device_count(int* out) {
    if (!out) return set_err(JSP_EINVAL, "out is NULL");
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess) {
        *out = 0;
        return set_err(JSP_EHIP, "hipGetDeviceCount: %s", hipGetErrorString(err));
    }
    *out = n;
    return JSP_OK;
}

int jsp_engine_create(int device_id, jsp_engine** out) {
    DeviceGuard dg;
    if (!out) return set_err(JSP_EINVAL, "out is NULL");
    jsp_clock::calibrate();  // once per process: the entry stamps' ticks -> ns factor
    *out = nullptr;
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess || n == 0)
        return set_err(JSP_EHIP, "no HIP device available (%s)", hipGetErrorString(err));
    if (device_id < 0 || device_id >= n) return set_err(JSP_EINVAL, "device %d out of range [0,%d)", device_id, n);
    HIP_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(JSP_EHIP, "device %d is %s; this engine is built for gfx950 (MI355X) only", device_id,
                       prop.gcnArchName);
    auto* e = new (std::nothrow) jsp_engine();
    if (!e) return set_err(JSP_ENOMEM, "engine allocation failed");
    e->device = device_id;
    e->n_cu = prop.multiProcessorCount;
    err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (err != hipSuccess) {
        delete e;
        return set_err(JSP_EHIP, "hipStreamCreate: %s", hipGetErrorString(err));
    }
    if (hipEventCreateWithFlags(&e->ev_ring[0], hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_ring[1], hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) {
        delete e;
        return set_err(JSP_EHIP, "hipEventCreate failed");
    }
    if (e->stats.reserve(16) != hipSuccess || hipMemset(e->stats.p, 0, 16) != hipSuccess) {
        delete e;
        return set_err(JSP_ENOMEM, "stats buffer");
    }
    if (e->h_err.reserve(64) != hipSuccess) {
        delete e;
        return set_err(JSP_ENOMEM, "error word");
    }
    std::memset(e->h_err.p, 0, 64);
    // operational: JSP_SERVICE=0 keeps the resident service off
    if (const char* v = std::getenv("JSP_SERVICE"))
        e->svc_mode = std::strcmp(v, "0") == 0 ? JSP_SERVICE_OFF
                      : std::strcmp(v, "parked") == 0 ? JSP_SERVICE_PARKED : JSP_SERVICE_AUTO;
    e->hooks = read_hooks();
    e->fast_clock.store(e->hooks.fast_clock, std::memory_order_relaxed);
    // test hooks: CUs the service may count on (stands in for a smaller GPU
    // or a partition), the service's first request number (next to 2^30)
    if (e->hooks.cu_limit > 0) e->n_cu = std::min<int>(e->n_cu, e->hooks.cu_limit);
    if (e->hooks.have_seq0) e->svc.seq = e->hooks.seq0;
    *out = e;
    return JSP_OK;
}

int jsp_engine_create_multi(const int* device_ids, int n_devices, jsp_engine** out) {
    DeviceGuard dg;
    if (!out) return set_err(JSP_EINVAL, "out is NULL");
    *out = nullptr;
    jsp_clock::calibrate();
    jspm::Multi* m = nullptr;
    if (int rc = jspm::create(device_ids, n_devices, &m)) return rc;
    auto* e = new (std::nothrow) jsp_engine();
    if (!e) {
        jspm::destroy(m);
        return set_err(JSP_ENOMEM, "engine allocation failed");
    }
    e->device = jspm::device_of(m);
    e->multi = m;
    *out = e;
    return JSP_OK;
}

int jsp_engine_shards(jsp_engine* e, int* shards, int* devices) {
    if (!e) return set_err(JSP_EINVAL, "engine is NULL");
    if (shards) *shards = e->multi ? jspm::shard_count(e->multi) : 1;
    if (devices) *devices = e->multi ? jspm::n_devices(e->multi) : 1;
    return JSP_OK;
}

void jsp_engine_destroy(jsp_engine* e) {
    if (!e) return;
    DeviceGuard dg;
    if (e->multi) {
        delete e;  // the destructor tears the device set down
        return;
    }
    if (e->waker.joinable()) {  // not under mu: the waker may be waiting for it
        {
            std::lock_guard<std::mutex> l(e->wake_mu);
            e->wake_quit.store(true);
        }
        e->wake_cv.notify_one();
        e->waker.join();
    }
    {
        std::lock_guard<std::mutex> g(e->mu);
        (void)hipSetDevice(e->device);
        e->wake_job = false;
        (void)svc_stop(e);
        if (e->stream) (void)hipStreamSynchronize(e->stream);
    }
    delete e;
}

int jsp_topology_upload(jsp_engine* e, const jsp_topology* t) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::topology_upload(e->multi, t); }
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = svc_suspend(e)) return rc;  // it holds the old buffers and geometry
    if (!t) return set_err(JSP_EINVAL, "topology is NULL");
    // a failed upload leaves the engine without topology (buffers may be gone)
    e->have_topo = e->have_snap = e->have_cls = false;
    e->sk_tab_ready = false;  // the sticky claim tables are laid out by the levels' domain counts
    const uint32_t K = t->n_levels;
    if (K < 1 || K > JSP_MAX_LEVELS) return set_err(JSP_EINVAL, "n_levels %u out of range [1,%d]", K, JSP_MAX_LEVELS);
    const uint32_t L = t->n_domains[K - 1];
    std::vector<std::vector<uint32_t>> fl(K);
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t D = t->n_domains[k];
        fl[k].resize(D + 1);
        if (k + 1 == K || t->first_leaf[k] == nullptr) {
            if (k + 1 != K) return set_err(JSP_EINVAL, "first_leaf[%u] is NULL", k);
            for (uint32_t d = 0; d <= D; ++d) fl[k][d] = d;
        } else {
            std::memcpy(fl[k].data(), t->first_leaf[k], sizeof(uint32_t) * (D + 1));
        }
        if (fl[k][0] != 0 || fl[k][D] != L) return set_err(JSP_EINVAL, "first_leaf[%u] must run 0..%u", k, L);
        for (uint32_t d = 0; d < D; ++d)
            if (fl[k][d] > fl[k][d + 1]) return set_err(JSP_EINVAL, "first_leaf[%u] not monotone at %u", k, d);
    }
    for (uint32_t k = 0; k + 1 < K; ++k)
        for (uint32_t d = 0; d <= t->n_domains[k]; ++d)
            if (!std::binary_search(fl[k + 1].begin(), fl[k + 1].end(), fl[k][d]))
                return set_err(JSP_EINVAL, "level %u is not nested in level %u (boundary %u)", k, k + 1, fl[k][d]);
    // taken-bitmap layout in LDS
    uint32_t off = 0;
    for (uint32_t k = 0; k < K; ++k) {
        e->t_off_h[k] = off;
        off += (t->n_domains[k] + 63) / 64;
    }
    e->t_off_h[K] = off;
    if (off > jsp::kMaxTakenWords)
        return set_err(JSP_ERANGE, "topology has %u bitmap words over all levels; engine limit is %u (%u domains)",
                       off, jsp::kMaxTakenWords, jsp::kMaxTakenWords * 64);
    hipStream_t s = e->stream;
    if (int rc = use_engine_stream(e)) return rc;
    jsp::TopoDev td{};
    td.K = K;
    for (uint32_t k = 0; k < K; ++k) {
        td.D[k] = t->n_domains[k];
        HIP_TRY(upload(e->fl[k], fl[k].data(), fl[k].size(), s));
        td.fl[k] = e->fl[k].as<uint32_t>();
        if (k + 1 < K) {  // child_start: level-(k+1) range of each level-k domain
            std::vector<uint32_t> cs(t->n_domains[k] + 1);
            for (uint32_t d = 0; d <= t->n_domains[k]; ++d)
                cs[d] = (uint32_t)(std::lower_bound(fl[k + 1].begin(), fl[k + 1].end(), fl[k][d]) - fl[k + 1].begin());
            HIP_TRY(upload(e->cs[k], cs.data(), cs.size(), s));
            td.cs[k] = e->cs[k].as<uint32_t>();
            e->h_cs[k] = cs;
        }
        if (k > 0) {  // parent at level k-1 of each level-k domain (by its first leaf)
            std::vector<int32_t> par(std::max<uint32_t>(t->n_domains[k], 1));
            for (uint32_t d = 0; d < t->n_domains[k]; ++d)
                par[d] = (int32_t)(std::upper_bound(fl[k - 1].begin(), fl[k - 1].end(), fl[k][d]) - fl[k - 1].begin()) - 1;
            HIP_TRY(upload(e->par[k], par.data(), par.size(), s));
            td.par[k] = e->par[k].as<int32_t>();
            e->h_par[k] = par;
        }
    }
    HIP_TRY(upload(e->t_off, e->t_off_h, K + 1, s));
    HIP_TRY(hipStreamSynchronize(s));
    e->topo = td;
    for (uint32_t k = 0; k < K; ++k) e->h_fl[k] = fl[k];
    e->walk.set_topology(K, t->n_domains, e->h_fl, e->h_cs, e->h_par);
    e->K = K;
    for (uint32_t k = 0; k < JSP_MAX_LEVELS; ++k) e->D[k] = k < K ? t->n_domains[k] : 0;
    e->L_total = L;
    e->have_topo = true;
    e->have_snap = false;  // a snapshot is tied to its topology
    e->have_cls = false;
    return JSP_OK;
}

int jsp_snapshot_upload(jsp_engine* e, const jsp_nodes* nd) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::snapshot_upload(e->multi, nd); }
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = svc_suspend(e)) return rc;  // it holds the old buffers and geometry
    if (!e->have_topo) return set_err(JSP_ESTATE, "upload the topology first");
    if (!nd || !nd->leaf_start) return set_err(JSP_EINVAL, "nodes / leaf_start is NULL");
    e->have_snap = false;  // until every column is resident again
    const uint32_t N = nd->n_nodes, W = nd->n_label_words, R = nd->n_res, NL = nd->n_leaves;
    if (W < 1 || W > JSP_MAX_LABEL_WORDS) return set_err(JSP_EINVAL, "n_label_words %u out of range", W);
    if (R < 1 || R > JSP_MAX_RES) return set_err(JSP_EINVAL, "n_res %u out of range", R);
    if ((uint64_t)nd->leaf_begin + NL > e->L_total)
        return set_err(JSP_EINVAL, "leaves [%u,%u) exceed topology (%u leaves)", nd->leaf_begin,
                       nd->leaf_begin + NL, e->L_total);
    if (N > 0 && (!nd->labels || !nd->taints || !nd->free_res || !nd->excl_owner))
        return set_err(JSP_EINVAL, "a node column is NULL");
    if (N > (1u << 30)) return set_err(JSP_ERANGE, "%u rows exceed the 2^30 row limit", N);
    const uint32_t* ls = nd->leaf_start;
    if (ls[0] != 0 || ls[NL] != N) return set_err(JSP_EINVAL, "leaf_start must run 0..%u", N);
    uint32_t max_rows = 0;
    for (uint32_t l = 0; l < NL; ++l) {
        if (ls[l] > ls[l + 1]) return set_err(JSP_EINVAL, "leaf_start not monotone at %u", l);
        max_rows = std::max(max_rows, ls[l + 1] - ls[l]);
    }
    // workgroup partition: whole leaves, <= 256 leaves each, one 1024-row
    // chunk each (test hooks: more chunks, or smaller row blocks)
    e->hooks = read_hooks();
    e->fast_clock.store(e->hooks.fast_clock, std::memory_order_relaxed);
    e->fit_ready = false;  // jsp_place_fit's rows are keyed by the hooks' order form and block too
    const uint32_t chunks = e->hooks.block_chunks;
    uint32_t target_rows = chunks * (uint32_t)jsp::kChunkRows - 4;  // fits even when unaligned
    if (e->hooks.block_rows >= 60 && e->hooks.block_rows < target_rows) target_rows = e->hooks.block_rows;
    std::vector<uint32_t> blk{0};
    {
        uint32_t rows = 0, leaves = 0;
        for (uint32_t l = 0; l < NL; ++l) {
            const uint32_t r = ls[l + 1] - ls[l];
            if (leaves > 0 && (rows + r > target_rows || leaves == (uint32_t)jsp::kMaxBlkLeaves)) {
                blk.push_back(l);
                rows = 0;
                leaves = 0;
            }
            rows += r;
            ++leaves;
        }
        if (NL > 0) blk.push_back(NL);
    }
    const uint32_t npad = ((N + 63) / 64) * 64 + 64;
    hipStream_t s = e->stream;
    if (int rc = use_engine_stream(e)) return rc;
    HIP_TRY(e->labels.reserve((size_t)W * npad * 8));
    HIP_TRY(e->taints.reserve((size_t)npad * 4));
    HIP_TRY(e->freer.reserve((size_t)R * npad * 4));
    HIP_TRY(e->excl.reserve((size_t)npad * 4));
    HIP_TRY(hipMemsetAsync(e->labels.p, 0, (size_t)W * npad * 8, s));
    HIP_TRY(hipMemsetAsync(e->taints.p, 0, (size_t)npad * 4, s));
    HIP_TRY(hipMemsetAsync(e->freer.p, 0, (size_t)R * npad * 4, s));
    HIP_TRY(hipMemsetAsync(e->excl.p, 0xFF, (size_t)npad * 4, s));
    if (N > 0) {
        for (uint32_t w = 0; w < W; ++w)
            HIP_TRY(hipMemcpyAsync(e->labels.as<uint64_t>() + (size_t)w * npad, nd->labels + (size_t)w * N,
                                   (size_t)N * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(e->taints.p, nd->taints, (size_t)N * 4, hipMemcpyHostToDevice, s));
        for (uint32_t r = 0; r < R; ++r)
            HIP_TRY(hipMemcpyAsync(e->freer.as<uint32_t>() + (size_t)r * npad, nd->free_res + (size_t)r * N,
                                   (size_t)N * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(e->excl.p, nd->excl_owner, (size_t)N * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(upload(e->leaf_start, ls, (size_t)NL + 1, s));
    e->h_ls.assign(ls, ls + NL + 1);
    e->bd_last.J = 0;
    std::vector<uint4> bt(blk.size() > 0 ? blk.size() - 1 : 0);
    uint32_t span = 0;
    for (size_t b = 0; b + 1 < blk.size(); ++b) {
        bt[b] = make_uint4(blk[b], blk[b + 1], ls[blk[b]], ls[blk[b + 1]]);
        span = std::max(span, bt[b].w - (bt[b].z & ~3u));
    }
    e->blk_l0.assign(blk.begin(), blk.end() - (blk.empty() ? 0 : 1));
    e->blk_l1.assign(blk.begin() + (blk.empty() ? 0 : 1), blk.end());
    // the host walk's tile table holds the blocks' leaf ranges: the same
    // block count, groups and classes per group over another partition (one
    // leaf more in the last block) must lay it out again, for the split
    // tiles of one request and for the split service alike
    e->os_key = ~0ull;
    e->svc.layout_key = ~0ull;
    if (bt.empty()) bt.push_back(make_uint4(0, 0, 0, 0));  // no rows: never read
    HIP_TRY(upload(e->blk, bt.data(), bt.size(), s));
    {
        // wave tiles: up to kWaveTileLeaves whole leaves in <= kWaveTileRows - 4
        // rows (one wave chunk at any row alignment), or one larger leaf alone
        // (none when a leaf is larger than a tile or a column reaches 2^31 bytes:
        // the workgroup tally then runs)
        std::vector<uint4> wt;
        const uint32_t max_rows = (uint32_t)jsp::kWaveTileRows - 4;
        bool ok = (uint64_t)W * npad * 8 < (1ull << 31) && (uint64_t)R * npad * 4 < (1ull << 31) &&
                  (uint64_t)jsp::kMaxClasses * std::max<uint32_t>(e->L_total, 1) * 4 < (1ull << 31);
        for (uint32_t l = 0; l < NL && ok; ++l) ok = ls[l + 1] - ls[l] <= max_rows;
        for (uint32_t l = 0; ok && l < NL;) {
            const uint32_t r0 = ls[l];
            uint32_t end = l;
            while (end < NL && end - l < (uint32_t)jsp::kWaveTileLeaves && ls[end + 1] - r0 <= max_rows) ++end;
            wt.push_back(make_uint4(l, end, r0, ls[end]));
            l = end;
        }
        e->n_wtiles = (uint32_t)wt.size();
        if (wt.empty()) wt.push_back(make_uint4(0, 0, 0, 0));  // never read (n_wtiles == 0)
        HIP_TRY(upload(e->wtiles, wt.data(), wt.size(), s));
    }
    HIP_TRY(e->ticket.reserve(16));
    HIP_TRY(hipMemsetAsync(e->ticket.p, 0, 16, s));  // single-launch tickets (tile draws, finished tiles)
    HIP_TRY(e->granules.reserve(8 * blk.size()));
    HIP_TRY(hipMemsetAsync(e->granules.p, 0, 8 * blk.size(), s));  // look-back granules (epoch 0 never matches)
    HIP_TRY(e->h_done.reserve(4 * blk.size()));
    // the service's inline patch staging, sized for this W/R now: the service
    // is stopped and no patch is pending (svc_suspend), so nothing staged can
    // be lost, and svc_start never reallocates it under a staged patch
    HIP_TRY(e->svc.pstage.reserve(jsp::patch_inline_layout(jsp::kPatchInlineRows, 15u, W, R).bytes));
    HIP_TRY(hipStreamSynchronize(s));
    std::memset(e->h_done.p, 0, 4 * blk.size());  // completion words (epoch 0 never matches)
    e->N = N;
    e->npad = npad;
    e->W = W;
    e->R = R;
    e->leaf_begin = nd->leaf_begin;
    e->n_leaves = NL;
    e->max_leaf_rows = max_rows;
    e->n_blocks = (uint32_t)blk.size() - 1;
    e->max_blk_span = span;
    {
        uint32_t most = 1;
        for (size_t b = 0; b + 1 < blk.size(); ++b) most = std::max(most, blk[b + 1] - blk[b]);
        e->blk_leaves = (most + 3) & ~3u;
    }
    e->tile_draws = e->done_draws = 0;
    e->spin_limit = e->hooks.lookback_spins;
    e->have_snap = true;
    if (e->have_cls) {
        for (auto& c : e->cls_h)
            if ((uint64_t)c.pods * max_rows >= (1ull << 32)) {
                e->have_cls = false;
                return set_err(JSP_ERANGE, "pods x rows per leaf overflows 32-bit tallies; re-upload classes");
            }
    }
    svc_resume(e);
    return JSP_OK;
}

static int snapshot_patch_locked(jsp_engine* e, const uint32_t* rows, uint32_t n, const uint64_t* labels,
                                 const uint32_t* taints, const uint32_t* free_res, const int32_t* excl_owner,
                                 std::chrono::steady_clock::time_point t0);

// The first calls of a recovery run on a host core that slept for hours (or
// for the bench's 60 ms): its caches are gone, and every line a call touches
// would miss in turn -- the engine's fields, the request and answer lines in
// pinned memory, the tables the answer is expanded with. Touched up front by
// independent prefetches their misses overlap instead. (On a warm core: ~100
// prefetches of lines already cached.) Measured on the cold recovery, data
// lines only (profiles/r05/probes/warm_ab.txt): cfg2 p50
// 11.0 -> 9.4 us at a 10 ms gap on one box, 16.7 -> 11.8 us at 1 ms on a
// slower-waking one; prefetching the hot code into L2 as well showed no
// consistent gain and is not done.
static inline void warm_lines(const void* p, size_t bytes) {
    const char* c = static_cast<const char*>(p);
    if (!c) return;
    for (size_t i = 0; i < bytes; i += 64) __builtin_prefetch(c + i, 0, 3);
}

static void warm_engine(const jsp_engine* e, bool place) {
    warm_lines(e, std::min<size_t>(sizeof(jsp_engine), 16384));
    warm_lines(e->svc.box.p, 128);
    warm_lines(e->h_patch_done.p, 128);
    if (place) {
        warm_lines(e->svc.words.p, std::min<size_t>(e->svc.words.bytes, 4096));
        warm_lines(e->svc.bits.p, std::min<size_t>(e->svc.bits.bytes, 8192));
        warm_lines(e->blk_l0.data(), 4 * e->blk_l0.size());
        // the split service's host walk: its bitmaps, sums, taken words and
        // hierarchy tables (a cold core's walk was ~2 us slower, cfg5)
        if (e->svc.shape == 3) e->walk.prefetch_state();
    } else {
        warm_lines(e->h_patch.p, std::min<size_t>(e->h_patch.bytes, 1024));
        warm_lines(e->svc.pstage.p, 256);
    }
}

static int snapshot_patch_call(jsp_engine* e, const uint32_t* rows, uint32_t n, const uint64_t* labels,
                               const uint32_t* taints, const uint32_t* free_res, const int32_t* excl_owner) {
    if (e->multi) { DeviceGuard dg; return jspm::snapshot_patch(e->multi, rows, n, labels, taints, free_res, excl_owner); }
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    {
        std::lock_guard<std::mutex> g(e->mu);
        warm_engine(e, false);  // under the lock: the waker may be replacing the buffers it touches
        rc = snapshot_patch_locked(e, rows, n, labels, taints, free_res, excl_owner, t0);
    }
    notify_waker(e);
    return rc;
}

int jsp_snapshot_patch(jsp_engine* e, const uint32_t* rows, uint32_t n, const uint64_t* labels,
                       const uint32_t* taints, const uint32_t* free_res, const int32_t* excl_owner) {
    if (int rc = check_engine(e)) return rc;
    const auto t0 = stamp_now(e);
    const int rc = snapshot_patch_call(e, rows, n, labels, taints, free_res, excl_owner);
    const double us = us_between(t0, stamp_now(e));
    std::lock_guard<std::mutex> l(e->met_mu);
    hist_add(e->met.patch_us, us, JSP_HIST_LO_US);
    if (rc != JSP_OK) e->met.patch_errors += 1;
    return rc;
}

static int snapshot_patch_locked(jsp_engine* e, const uint32_t* rows, uint32_t n, const uint64_t* labels,
                                 const uint32_t* taints, const uint32_t* free_res, const int32_t* excl_owner,
                                 std::chrono::steady_clock::time_point t0) {
    if (!e->have_snap) return set_err(JSP_ESTATE, "no snapshot uploaded");
    if (n == 0) return JSP_OK;
    if (!rows) return set_err(JSP_EINVAL, "rows is NULL");
    for (uint32_t i = 0; i < n; ++i)
        if (rows[i] >= e->N) return set_err(JSP_EINVAL, "row %u out of range (%u rows)", rows[i], e->N);
    run_wake(e);  // an earlier patch's wake still queued: run it (that patch then goes to the service)
    lease_drop(e);  // the rows change, whichever way the patch travels
    // A patch the service's dispatcher applies is not stream-ordered: device-
    // path work still in flight on a caller's stream (it may be reading the
    // rows) finishes first. (The patch kernel is ordered by the stream.)
    if (e->foreign_pending) {
        HIP_TRY(hipEventSynchronize(e->ev_last));
        e->foreign_pending = false;
    }
    const uint32_t fl = (labels ? jsp::kPatchLab : 0u) | (taints ? jsp::kPatchTaint : 0u) |
                        (free_res ? jsp::kPatchFree : 0u) | (excl_owner ? jsp::kPatchExcl : 0u);
    // A patch small enough to ride in the next request's line, while the
    // service is up: held back (a watch event's few rows; more of the same
    // columns merge into it) and applied by the dispatcher from the request
    // itself -- no staging read, no request of its own. Whatever else reads
    // the rows first posts it alone and waits (patch_wait).
    const bool small = n <= jsp::micro_rows_max(e->W, e->R);
    bool micro = false;
    if (small && e->patch_pending && e->patch_micro && e->patch_deferred && e->micro_fl == fl && svc_up(e))
        micro = micro_merge(e, rows, n, labels, taints, free_res, excl_owner);  // same patch number: not sent yet
    if (!micro) {
        if (int rc = svc_settle(e)) return rc;  // no tile may still be reading the rows of the last request
        if (int rc = patch_wait(e)) return rc;  // the staging buffer is free again
    }
    hipStream_t s = e->stream;
    auto& v = e->svc;
    if (!e->patch_ctr.p) {
        if (int rc = use_engine_stream(e)) return rc;
        HIP_TRY(e->patch_ctr.reserve(64));
        HIP_TRY(hipMemsetAsync(e->patch_ctr.p, 0, 64, s));
    }
    if (!e->h_patch_done.p) {
        HIP_TRY(e->h_patch_done.reserve(128));
        std::memset(e->h_patch_done.p, 0, 128);
    }
    if (!micro && small && svc_up(e)) {
        e->micro_n = 0;
        e->micro_fl = fl;
        micro = micro_merge(e, rows, n, labels, taints, free_res, excl_owner);  // fits: n <= the row capacity
        if (micro) {
            e->patch_seq = e->patch_seq % 0x7FFFFFFFu + 1u;
            e->patch_bits = 0u;  // the request's chunk 1 says it carries micro rows
            e->patch_nf = 0u;
            e->patch_req = 0;
            e->patch_micro = e->patch_pending = e->patch_svc = e->patch_deferred = true;
        }
    }
    if (micro) {
        e->svc.micro_dirty = true;  // the resident tiles' on-chip row copies are stale
        if (int rc = micro_stage_kernel_form(e)) return rc;
        const auto t2 = std::chrono::steady_clock::now();
        e->acc.patches += 1;
        e->acc.patch_us += std::chrono::duration<double, std::micro>(t2 - t0).count();
        return JSP_OK;
    }
    e->patch_micro = false;
    e->svc.rows_dirty = true;  // the resident tiles' on-chip row copies are stale
    // Who applies it: the running service's dispatcher (posted at once; a
    // request that finds it not yet taken carries it again; whatever else
    // reads the rows first waits for it, patch_wait); after the service left,
    // a recovery's first patch restarts it (the waker thread: its grid comes
    // up while the deletions finish) and the dispatcher applies it followed by
    // a warm-up request; otherwise the patch kernel.
    const auto t1 = std::chrono::steady_clock::now();
    const double since = std::chrono::duration<double, std::milli>(t1 - v.last).count();
    const bool up = v.running && since <= 0.5 * idle_ms(e) && svc_ok(e) && svc_shape(e) == v.shape;
    const bool wake = !up && svc_wake_wanted(e);
    // The delta into pinned staging, read in place. Patches for the service
    // of up to kPatchInlineRows rows go to its fixed inline buffer (layout
    // from n and the column flags, which ride in the request; sized for this
    // W/R at snapshot upload); larger ones, and the patch kernel's, to the
    // engine's staging through a descriptor.
    const uint32_t W = e->W, R = e->R;
    const bool inl = (up || wake) && n <= jsp::kPatchInlineRows && v.pstage.p &&
                     jsp::patch_inline_layout(jsp::kPatchInlineRows, 15u, W, R).bytes <= v.pstage.bytes;
    const jsp::PatchInlineLayout L = jsp::patch_inline_layout(n, inl ? fl : 15u, W, R);
    char* hp;
    size_t base = 0;
    if (inl) {
        hp = static_cast<char*>(v.pstage.p);
    } else {
        base = 64;  // the same layout without its header
        HIP_TRY(e->h_patch.reserve(L.bytes, grave(e)));
        hp = static_cast<char*>(e->h_patch.p) - base;
    }
    std::memcpy(hp + L.rows, rows, (size_t)n * 4);
    if (labels) std::memcpy(hp + L.lab, labels, (size_t)W * n * 8);
    if (taints) std::memcpy(hp + L.taint, taints, (size_t)n * 4);
    if (free_res) std::memcpy(hp + L.free, free_res, (size_t)R * n * 4);
    if (excl_owner) std::memcpy(hp + L.excl, excl_owner, (size_t)n * 4);
    e->patch_seq = e->patch_seq % 0x7FFFFFFFu + 1u;
    if (inl) __atomic_store_n(reinterpret_cast<uint32_t*>(hp), e->patch_seq, __ATOMIC_RELAXED);  // header
    jsp::PatchArgs a{};
    a.rows = reinterpret_cast<const uint32_t*>(hp + L.rows);
    a.n = n;
    a.npad = e->npad;
    a.W = W;
    a.R = R;
    a.dlab = labels ? reinterpret_cast<const uint64_t*>(hp + L.lab) : nullptr;
    a.dtaint = taints ? reinterpret_cast<const uint32_t*>(hp + L.taint) : nullptr;
    a.dfree = free_res ? reinterpret_cast<const uint32_t*>(hp + L.free) : nullptr;
    a.dexcl = excl_owner ? reinterpret_cast<const int32_t*>(hp + L.excl) : nullptr;
    a.labels = e->labels.as<uint64_t>();
    a.taints = e->taints.as<uint32_t>();
    a.freer = e->freer.as<uint32_t>();
    a.excl = e->excl.as<int32_t>();
    a.counter = e->patch_ctr.as<unsigned long long>();
    a.done = e->h_patch_done.as<uint32_t>();
    a.seq = e->patch_seq;
    e->last_patch = a;
    e->patch_bits = jsp::kReqPatch | (inl ? jsp::kReqPatchInline : 0u);
    e->patch_req = 0;
    e->patch_nf = inl ? (n | fl << 16) : 0u;
    if (up || wake) {
        if (!inl && v.pdesc.p) *v.pdesc.as<jsp::PatchDesc>() = jsp::PatchDesc{a.rows, a.dlab, a.dtaint, a.dfree, a.dexcl, n, a.seq};
        e->patch_pending = e->patch_svc = true;
    }
    // No wait here: later work is ordered after the patch -- service requests
    // and launches by its completion word (patch_wait / patch_fence), or by
    // the stream for the patch kernel.
    if (up) {
        e->patch_deferred = true;
        patch_post_deferred(e);  // posted now: it lands during the gap before the next request
    } else if (wake) {
        // held back; the waker restarts the service and posts it (run_wake)
        e->patch_deferred = true;
        ring_waker(e);
    } else {
        if (int rc = use_engine_stream(e)) return rc;
        // the patch kernel's workgroups count up to the target (patches the
        // service applied do not touch the counter)
        e->patch_target += (n + 255) / 256;
        a.target = e->patch_target;
        HIP_TRY(jsp::launch_patch(a, s));
        e->patch_pending = true;
        e->patch_svc = false;
        svc_resume(e);
        svc_wake(e);
    }
    const auto t2 = std::chrono::steady_clock::now();
    using us = std::chrono::duration<double, std::micro>;
    e->acc.patches += 1;
    e->acc.patch_us += us(t2 - t0).count();
    if (!wake) e->acc.wake_us += us(t2 - t1).count();  // a wake's own time is counted where it runs
    return JSP_OK;
}

int jsp_classes_upload(jsp_engine* e, const jsp_job_class* classes, uint32_t C) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::classes_upload(e->multi, classes, C); }
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = svc_suspend(e)) return rc;  // it holds the old buffers and geometry
    if (!e->have_topo) return set_err(JSP_ESTATE, "upload the topology first");
    if (C > (uint32_t)jsp::kMaxClasses) return set_err(JSP_ERANGE, "%u classes exceed the limit of %d", C, jsp::kMaxClasses);
    if (C > 0 && !classes) return set_err(JSP_EINVAL, "classes is NULL");
    e->have_cls = false;  // until the new classes are resident
    std::vector<jsp::DevClass> h(std::max<uint32_t>(C, 1));
    std::vector<uint32_t> woff(C + 1, 0);
    for (uint32_t c = 0; c < C; ++c) {
        const jsp_job_class& x = classes[c];
        if (x.level >= e->K) return set_err(JSP_EINVAL, "class %u: level %u >= n_levels %u", c, x.level, e->K);
        if (x.pods < 1) return set_err(JSP_EINVAL, "class %u: pods must be >= 1", c);
        if (x.pods > (1u << 22)) return set_err(JSP_ERANGE, "class %u: pods %u exceed 2^22", c, x.pods);
        if (e->have_snap && (uint64_t)x.pods * e->max_leaf_rows >= (1ull << 32))
            return set_err(JSP_ERANGE, "class %u: pods x rows per leaf overflows 32-bit tallies", c);
        jsp::DevClass& d = h[c];
        std::memset(&d, 0, sizeof d);
        for (int w = 0; w < 4; ++w) {
            // A bit both required and forbidden makes the class unsatisfiable (jsplace.h): it stays in
            // req and leaves mask, so (labels & mask) never holds it and never equals req.
            const uint64_t both = x.req_labels[w] & x.forbid_labels[w];
            d.req[w] = x.req_labels[w];
            d.mask[w] = (x.req_labels[w] | x.forbid_labels[w]) & ~both;
        }
        d.tol_inv = ~x.tolerated_taints;
        d.level = x.level;
        d.pods = x.pods;
        for (int r = 0; r < 4; ++r) {
            d.res[r] = x.req_res[r];
            d.rcp[r] = divisor_rcp(x.req_res[r]);
        }
        woff[c + 1] = woff[c] + (e->D[x.level] + 63) / 64;
    }
    hipStream_t s = e->stream;
    if (int rc = use_engine_stream(e)) return rc;
    HIP_TRY(upload(e->cls, h.data(), h.size(), s));
    HIP_TRY(upload(e->word_off, woff.data(), woff.size(), s));
    HIP_TRY(e->feas.reserve((size_t)std::max<uint32_t>(woff[C], 1) * 8));
    // the folded feasibility (fold_ok) never writes the bits past the last leaf
    HIP_TRY(hipMemsetAsync(e->feas.p, 0, (size_t)std::max<uint32_t>(woff[C], 1) * 8, s));
    HIP_TRY(e->cap.reserve((size_t)std::max<uint32_t>(C, 1) * std::max<uint32_t>(e->L_total, 1) * 4));
    HIP_TRY(e->occ.reserve((size_t)std::max<uint32_t>(e->L_total, 1) * 4));
    HIP_TRY(hipStreamSynchronize(s));
    e->cls_h.assign(h.begin(), h.begin() + C);
    e->bd_last.J = 0;  // its records name classes of the previous upload
    e->walk.set_classes(e->cls_h);
    e->gs_ready = false;  // the span counts' rows follow the classes' levels
    e->fit_ready = false;  // and so do the order step's rows and segments
    e->C = C;
    e->feas_words = woff[C];
    e->have_cls = true;
    svc_resume(e);
    return JSP_OK;
}

int jsp_tally_device(jsp_engine* e, uint32_t* d_cap, uint32_t* d_occ, uint32_t ld, void* stream) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: use jsp_place (the shards tally and combine inside it)");
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (!d_occ || (e->C > 0 && !d_cap)) return set_err(JSP_EINVAL, "output buffer is NULL");
    if (ld < e->L_total) return set_err(JSP_EINVAL, "ld %u < total leaves %u", ld, e->L_total);
    if (int rc = check_launch_error(e)) return rc;
    hipStream_t s = pick(e, stream);
    if (int rc = enter_stream(e, s)) return rc;
    // a tally alone: no shape, no walk (jspb_last_plan: JSPB_WALK_NONE, the other fields 0)
    e->plan = jspb_plan{};
    e->plan.groups = e->plan.cpg = 1;
    e->last_shape = 0;
    const int rc = tally_impl(e, d_cap, d_occ, ld, s);
    if (int lr = leave_stream(e, s)) return lr;
    return rc;
}

int jsp_assign_device(jsp_engine* e, const uint32_t* d_cap, const uint32_t* d_occ, uint32_t ld,
                      const uint32_t* d_run_class, const uint32_t* d_run_len, uint32_t n_runs, uint32_t n_jobs,
                      int32_t* d_assign, void* stream) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: use jsp_place");
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (ld < e->L_total) return set_err(JSP_EINVAL, "ld %u < total leaves %u", ld, e->L_total);
    if (!d_cap || !d_occ) return set_err(JSP_EINVAL, "tally buffers are NULL");
    if (n_runs > 0 && (!d_run_class || !d_run_len)) return set_err(JSP_EINVAL, "run buffers are NULL");
    if (n_jobs > 0 && !d_assign) return set_err(JSP_EINVAL, "assign buffer is NULL");
    if (int rc = check_launch_error(e)) return rc;
    hipStream_t s = pick(e, stream);
    if (int rc = enter_stream(e, s)) return rc;
    const int rc = assign_impl(e, d_cap, d_occ, ld, d_run_class, d_run_len, n_runs, n_jobs, d_assign, s);
    if (int lr = leave_stream(e, s)) return lr;
    return rc;
}

int jsp_place_device(jsp_engine* e, const uint32_t* d_run_class, const uint32_t* d_run_len, uint32_t n_runs,
                     uint32_t n_jobs, int32_t* d_assign, void* stream) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: use jsp_place");
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (e->leaf_begin != 0 || e->n_leaves != e->L_total)
        return set_err(JSP_ESTATE, "sharded engine: use jsp_tally_device + all-reduce + jsp_assign_device");
    if (n_runs > 0 && (!d_run_class || !d_run_len)) return set_err(JSP_EINVAL, "run buffers are NULL");
    if (n_jobs > 0 && !d_assign) return set_err(JSP_EINVAL, "assign buffer is NULL");
    if (int rc = check_launch_error(e)) return rc;
    hipStream_t s = pick(e, stream);
    if (int rc = enter_stream(e, s)) return rc;
    const int rc = place_impl(e, d_run_class, d_run_len, n_runs, n_jobs, d_assign, s);
    if (int lr = leave_stream(e, s)) return lr;
    return rc;
}


int jspb_tally_device_timed(jsp_engine* e, uint32_t* d_cap, uint32_t* d_occ, uint32_t ld, uint32_t iters,
                           const void* d_scrub, size_t scrub_bytes, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: time its shard engines");
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (!d_occ || (e->C > 0 && !d_cap)) return set_err(JSP_EINVAL, "output buffer is NULL");
    if (ld < e->L_total) return set_err(JSP_EINVAL, "ld %u < total leaves %u", ld, e->L_total);
    return time_steps(e, iters, d_scrub, scrub_bytes, out_us,
                      [&](hipStream_t s) { return tally_impl(e, d_cap, d_occ, ld, s); });
}

int jspb_explain_rows_loop(jsp_engine* e, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: time its shard engines");
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (int rc = check_timed(iters, 4096, out_us)) return rc;
    if (e->C == 0) return set_err(JSP_ESTATE, "no job classes uploaded");
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    if (int rc = timing_events(e, 1)) return rc;
    const uint32_t grid = jsp::explain_rows_grid(e->N, e->n_cu);
    HIP_TRY(e->ex_parts.reserve(jsp::explain_parts_bytes(grid, e->C), grave(e)));
    const jsp::TallyArgs a = tally_args(e, nullptr, nullptr, 0);
    if (int rc = time_legs(e, s, 2, iters, out_us, [&](int leg) -> int {
            if (leg == 0) HIP_TRY(jsp::launch_explain_rows(a, e->N, e->C, grid, e->ex_parts.as<uint32_t>(), s));
            else return tally_impl(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, s);
            return JSP_OK;
        }))
        return rc;
    return check_launch_error(e);
}

int jspb_bind_kernel_loop(jsp_engine* e, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    std::unique_lock<std::mutex> g;
    // (a sharded engine has no jsp_bind_pods call to repeat: refused below)
    if (int rc = single_engine(e, "jsp_bind_pods", g, false)) return rc;
    if (int rc = check_timed(iters, 4096, out_us)) return rc;
    if (e->bd_last.J == 0) return set_err(JSP_ESTATE, "no jsp_bind_pods call on this snapshot yet");
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    if (int rc = timing_events(e, 1)) return rc;
    const jsp::BindArgs b = e->bd_last;
    const jsp::TallyArgs a = tally_args(e, nullptr, nullptr, e->L_total);
    if (int rc = time_legs(e, s, 3, iters, out_us, [&](int leg) -> int {
            if (leg == 0) {
                HIP_TRY(hipMemsetAsync(e->bd_tab.p, 0xFF, e->bd_tab.bytes, s));
                HIP_TRY(jsp::launch_bind_claim(b, a.cls, s));
            }
            if (leg <= 1) {
                HIP_TRY(jsp::launch_bind(a, b, 0, e->bd_last_wave, false, s));
                HIP_TRY(jsp::launch_bind(a, b, e->bd_last_wave, e->bd_last_n - e->bd_last_wave, true, s));
                return JSP_OK;
            }
            return tally_impl(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, s);
        }))
        return rc;
    return check_launch_error(e);
}

int jspb_tally_device_spans(jsp_engine* e, uint32_t* d_cap, uint32_t* d_occ, uint32_t ld, uint32_t iters,
                           double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: time its shard engines");
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (!d_occ || (e->C > 0 && !d_cap)) return set_err(JSP_EINVAL, "output buffer is NULL");
    if (ld < e->L_total) return set_err(JSP_EINVAL, "ld %u < total leaves %u", ld, e->L_total);
    if (int rc = check_timed(iters, 1024, out_us)) return rc;
    if (e->n_wtiles == 0 || e->C < 1 || e->C > 4 || tally_wave_grid(e) != 0 || e->hooks.tally_block)
        return set_err(JSP_ESTATE, "the span probe times the one-tile wave tally; this snapshot runs another shape");
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    const size_t per = (size_t)2 * e->n_wtiles;
    DevBuf st;
    HIP_TRY(st.reserve(per * iters * 8));
    for (uint32_t i = 0; i < iters; ++i) {
        jsp::TallyArgs a = tally_args(e, d_cap, d_occ, ld);
        a.wstamps = st.as<unsigned long long>() + per * i;
        HIP_TRY(jsp::launch_tally_wave(a, e->wtiles.as<uint4>(), e->n_wtiles, e->n_leaves, 0, s));
    }
    std::vector<unsigned long long> h(per * iters);
    HIP_TRY(hipMemcpyAsync(h.data(), st.p, per * iters * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<double> us(iters);
    double sum = 0.0;
    unsigned long long lo0 = 0, lo_last = 0;
    for (uint32_t i = 0; i < iters; ++i) {
        unsigned long long lo = ~0ull, hi = 0;
        for (size_t k = 0; k < per; k += 2) {
            lo = std::min(lo, h[per * i + k]);
            hi = std::max(hi, h[per * i + k + 1]);
        }
        us[i] = (double)(hi - lo) / 100.0;  // 100 MHz ticks
        sum += us[i];
        if (i == 0) lo0 = lo;
        lo_last = lo;
    }
    std::sort(us.begin(), us.end());
    out_us[0] = us[iters / 2];
    out_us[1] = sum / iters;
    // the launches' period by the kernels' own clock: first wave of launch 0
    // to first wave of the last launch, per launch (execution + the gap the
    // dispatch leaves between back-to-back launches)
    out_us[3] = iters > 1 ? (double)(lo_last - lo0) / 100.0 / (iters - 1) : out_us[1];
    // an empty one-workgroup launch timed by events on its dispatch packet:
    // the fixed cost events add to a kernel's own span
    const uint32_t grid = 1;  // the launch's fixed packet and completion cost (a grid's dispatch overlaps its work)
    std::vector<EvPair> ev(iters);
    for (auto& p : ev) {
        HIP_TRY(hipEventCreate(&p.a));
        HIP_TRY(hipEventCreate(&p.b));
    }
    int rc = JSP_OK;
    for (uint32_t i = 0; i < iters && rc == JSP_OK; ++i) {
        jsp::set_launch_start(ev[i].a);
        jsp::set_launch_stop(ev[i].b);
        if (jsp::launch_empty(grid, s) != hipSuccess) rc = set_err(JSP_EHIP, "empty launch failed");
        jsp::set_launch_start(nullptr);
        jsp::set_launch_stop(nullptr);
    }
    if (rc == JSP_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_err(JSP_EHIP, "empty launches failed");
    std::vector<double> eu(iters, 0.0);
    for (uint32_t i = 0; i < iters && rc == JSP_OK; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[i].a, ev[i].b) != hipSuccess) rc = set_err(JSP_EHIP, "event time failed");
        eu[i] = ms * 1e3;
    }
    for (auto& p : ev) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    if (rc) return rc;
    std::sort(eu.begin(), eu.end());
    out_us[2] = eu[iters / 2];
    return check_launch_error(e);
}

int jspb_place_device_timed(jsp_engine* e, const uint32_t* d_run_class, const uint32_t* d_run_len, uint32_t n_runs,
                           uint32_t n_jobs, int32_t* d_assign, uint32_t iters, const void* d_scrub, size_t scrub_bytes,
                           double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: use jsp_place");
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (e->leaf_begin != 0 || e->n_leaves != e->L_total)
        return set_err(JSP_ESTATE, "sharded engine: use jsp_tally_device + all-reduce + jsp_assign_device");
    if (n_runs > 0 && (!d_run_class || !d_run_len)) return set_err(JSP_EINVAL, "run buffers are NULL");
    if (n_jobs > 0 && !d_assign) return set_err(JSP_EINVAL, "assign buffer is NULL");
    return time_steps(e, iters, d_scrub, scrub_bytes, out_us, [&](hipStream_t s) {
        return place_impl(e, d_run_class, d_run_len, n_runs, n_jobs, d_assign, s);
    });
}

// t0: the call's entry stamp (jsp_place). *leased: the call was answered
// under the lease; stats->wall_us then holds its wall to the one other clock
// read of the call, and no HIP call was made (nor the device set).
static int place_call(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                      int32_t* assign_out, uint32_t* tally_out, uint32_t* occ_out, jsp_stats* stats,
                      std::chrono::steady_clock::time_point t0, bool* leased) {
    if (e->multi) {
        if (hipSetDevice(e->device) != hipSuccess) return set_err(JSP_EHIP, "hipSetDevice(%d) failed", e->device);
        DeviceGuard dg;
        return jspm::place(e->multi, run_class, run_len, n_runs, assign_out, tally_out, occ_out, stats);
    }
    std::lock_guard<std::mutex> g(e->mu);
    // A hot caller under the lease: its previous placement was answered on the
    // host a few microseconds ago, so every line this one touches is in its
    // cache and the two prefetch sweeps (some 350 instructions) buy nothing.
    // Any other call -- a recovery's, on a core that slept -- makes them.
    const bool hot = e->lease.held && t0 - e->lease.t_end < std::chrono::microseconds(20);
    if (!hot) warm_engine(e, true);  // under the lock: the waker may be replacing the buffers it touches
    if (int rc = ready(e, true)) return rc;
    if (e->leaf_begin != 0 || e->n_leaves != e->L_total)
        return set_err(JSP_ESTATE, "sharded engine: use jsp_tally_device + all-reduce + jsp_assign_device");
    if (n_runs > 0 && (!run_class || !run_len)) return set_err(JSP_EINVAL, "run buffers are NULL");
    uint64_t J64 = 0;
    if (int rc = check_runs(e, run_class, run_len, n_runs, &J64)) return rc;
    const uint32_t J = (uint32_t)J64;
    if (J > 0 && !assign_out) return set_err(JSP_EINVAL, "assign_out is NULL");
    // the caller's assign[], written by the answer's expansion: for write, ahead of the wait
    for (size_t i = 0; !hot && i < std::min<size_t>((size_t)J * 4, 16384); i += 64)
        __builtin_prefetch(reinterpret_cast<char*>(assign_out) + i, 1, 3);
    const bool want_tally = (tally_out && e->C > 0) || occ_out;
    const int shape = want_tally || J >= jsp::kReqPatchInline ? 0 : svc_shape(e);  // J and the request bits share a word
    if (shape != 0) {
        std::chrono::steady_clock::time_point t1 = t0;
        uint32_t placed = 0;
        const int src = svc_place(e, run_class, run_len, n_runs, J, assign_out, &placed, t0, shape, leased, &t1);
        if (src != JSP_OK) {
            // the service could not answer: stop it and answer this call on the
            // launch path. A geometry failure (its grid cannot be co-resident,
            // JSP_ERANGE, or its dispatcher never polled) keeps it off until
            // the next upload; a transient one (it left twice, a look-back
            // timed out) lets the next call start it again.
            (void)svc_stop(e);
            if (src == JSP_ERANGE || e->svc.start_failed) e->svc.broken = true;
            e->svc.start_failed = false;
            e->acc.svc_fallbacks += 1;
            {
                std::lock_guard<std::mutex> l(e->met_mu);
                e->met.svc_fallbacks += 1;
            }
            g_err.clear();  // answered: the call succeeds (jsp_timing.svc_fallbacks counts it)
            goto launch_path;
        }
        {
        const auto t2 = stamp_now(e);
        if (e->lease.held) e->lease.t_end = t2;
        e->svc.armed = true;
        if (!e->waker_poll.load(std::memory_order_relaxed)) {
            e->waker_poll.store(true, std::memory_order_release);
            notify_waker_poll(e);
        }
        e->last_shape = e->svc.shape == 3 ? 5 : 3;
        if (stats) {
            stats->jobs = J;
            stats->runs = n_runs;
            stats->placed = n_runs > 0 ? placed : 0;
            stats->fused = e->last_shape;
            stats->wall_us = std::chrono::duration<double, std::micro>(t2 - t0).count();
        }
        using us = std::chrono::duration<double, std::micro>;
        e->acc.host_calls += 1;
        e->acc.host_prep_us += us(t1 - t0).count();  // (a leased answer: t1 = t0, its wall is all wait)
        e->acc.host_wait_us += us(t2 - t1).count();
        if (*leased) {
            e->acc.svc_answer_us += us(t2 - t0).count();
            // its metrics here, under mu: jsp_place takes no second lock for it
            e->lmet.record(us(t2 - t0).count(), J, n_runs > 0 ? placed : 0);
        }
        return JSP_OK;
        }
    }
launch_path:
    if (hipSetDevice(e->device) != hipSuccess) return set_err(JSP_EHIP, "hipSetDevice(%d) failed", e->device);
    hipStream_t s = e->stream;
    if (int rc = check_launch_error(e)) return rc;
    if (int rc = use_engine_stream(e)) return rc;
    // runs in, assign[] and stats out through pinned mapped host memory: one
    // launch sequence, no DMA round trips. The single-launch shapes signal
    // completion through host words (wait_done); the others, and calls that
    // copy the tallies out, synchronise the stream.
    HIP_TRY(e->h_runs.reserve((size_t)std::max<uint32_t>(n_runs, 1) * 8, grave(e)));
    HIP_TRY(e->h_assign.reserve((size_t)std::max<uint32_t>(J, 1) * 4, grave(e)));
    HIP_TRY(e->h_stats.reserve(16));
    uint32_t* h_rc = e->h_runs.as<uint32_t>();
    uint32_t* h_rl = h_rc + std::max<uint32_t>(n_runs, 1);
    if (n_runs > 0) {
        std::memcpy(h_rc, run_class, (size_t)n_runs * 4);
        std::memcpy(h_rl, run_len, (size_t)n_runs * 4);
    }
    e->stats_override = e->h_stats.as<uint32_t>();
    uint32_t n_sig = 0;
    const auto t1 = std::chrono::steady_clock::now();
    const int prc = place_impl(e, h_rc, h_rl, n_runs, J, e->h_assign.as<int32_t>(), s, !want_tally, &n_sig,
                               want_tally, true);
    e->stats_override = nullptr;
    if (prc) return prc;
    const auto t2 = std::chrono::steady_clock::now();
    if (want_tally) {
        if (tally_out && e->C > 0)
            HIP_TRY(hipMemcpyAsync(tally_out, e->cap.p, (size_t)e->C * e->L_total * 4, hipMemcpyDeviceToHost, s));
        if (occ_out) HIP_TRY(hipMemcpyAsync(occ_out, e->occ.p, (size_t)e->L_total * 4, hipMemcpyDeviceToHost, s));
    }
    if (!want_tally && (e->last_shape == 7 || e->last_shape == 8)) {
        // the host walked: assign[] is complete, and nothing the stream still
        // runs writes what the caller reads
    } else if (n_sig > 0) {
        if (int rc = wait_done(e, s, n_sig, e->epoch)) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(s));
    }
    const auto t3 = std::chrono::steady_clock::now();
    if (J > 0) std::memcpy(assign_out, e->h_assign.p, (size_t)J * 4);
    if (int rc = check_launch_error(e)) return rc;
    uint32_t st[2];
    std::memcpy(st, e->h_stats.p, sizeof st);
    if (stats) {
        stats->jobs = J;
        stats->runs = n_runs > 0 ? st[0] : 0;
        stats->placed = n_runs > 0 ? st[1] : 0;
        stats->fused = e->last_shape;
        stats->wall_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    const auto t4 = std::chrono::steady_clock::now();
    using us = std::chrono::duration<double, std::micro>;
    e->acc.host_calls += 1;
    e->acc.host_prep_us += us(t1 - t0).count();
    e->acc.host_launch_us += us(t2 - t1).count();
    e->acc.host_wait_us += us(t3 - t2).count();
    e->acc.host_post_us += us(t4 - t3).count();
    return JSP_OK;
}

int jsp_place(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
              int32_t* assign_out, uint32_t* tally_out, uint32_t* occ_out, jsp_stats* stats) {
    // (the device is set where a HIP call can follow: a leased answer makes none)
    if (!e) return set_err(JSP_EINVAL, "engine is NULL");
    const bool fast = e->fast_clock.load(std::memory_order_relaxed);
    const auto t0 = fast ? jsp_clock::fast_now() : std::chrono::steady_clock::now();
    jsp_stats local{};
    jsp_stats* st = stats ? stats : &local;
    bool leased = false;
    const int rc = place_call(e, run_class, run_len, n_runs, assign_out, tally_out, occ_out, st, t0, &leased);
    // (a leased answer: its exit stamp was read and its metrics recorded under
    // the engine's lock. Any other call reads the real clock here, which
    // refreshes the entry stamps' anchor)
    if (leased) return rc;
    const double us = us_between(t0, fast ? jsp_clock::anchor_now() : std::chrono::steady_clock::now());
    // (one wall per call: what its stats report is what the histogram holds)
    if (rc == JSP_OK) st->wall_us = us;
    std::lock_guard<std::mutex> l(e->met_mu);
    hist_add(e->met.place_us, us, JSP_HIST_LO_US);
    if (rc != JSP_OK) {
        e->met.place_errors += 1;
        return rc;
    }
    hist_add(e->met.batch_jobs, (double)st->jobs, JSP_HIST_LO_JOBS);
    e->met.placed += st->placed;
    e->met.unplaceable += st->jobs - st->placed;
    if (st->fused == 3 || st->fused == 5) e->met.svc_calls += 1;
    return rc;
}

// ---- sticky placement (DESIGN.md §2 "Sticky placement") ----
// On the engine stream: the tally into the engine's cap / occ, the unfolded
// feasibility words, the keep step (keepers answer for themselves and clear
// the bits of what they intersect), the fill of the remaining jobs through
// assign_impl on the words as they now stand (any of the level walker, the
// generic GPU walker or the host walk), the scatter of the fill's answers (on
// the host when the host walked: no launch and no wait behind the walk).
// The fill's run list keeps the call's runs (a run's length minus its
// keepers, possibly zero: every walker steps over an empty run) and its job
// bound stays J, so nothing the host decides depends on the keepers' count.
static int sticky_call(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs_in,
                       const int32_t* prev, int32_t* assign_out, jsp_sticky_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> g;
    // The claim tables, the taken bitmap and the per-run keeper counts are at
    // rest only after every launch of a call ran: a call that fails anywhere
    // under the lock has them filled again by the next one.
    struct AtRest {
        jsp_engine* e;
        const std::unique_lock<std::mutex>& g;
        bool ok = false;
        ~AtRest() {
            if (!ok && g.owns_lock()) {
                e->sk_tab_ready = false;
                e->sk_run_kept_p = nullptr;
            }
        }
    } at_rest{e, g};
    if (int rc = single_engine(e, "jsp_place_sticky", g)) return rc;
    uint32_t J = 0;
    if (int rc = run_front(e, run_class, run_len, n_runs_in, &J)) return rc;
    if (J > 0 && !assign_out) return set_err(JSP_EINVAL, "assign_out is NULL");
    uint32_t n_runs = 0;  // without the empty runs
    for (uint32_t i = 0; i < n_runs_in; ++i) n_runs += run_len[i] > 0 ? 1u : 0u;
    // the input staging {prev [J], job_run [J], job_cls [J], run_len [n_runs]}, hints checked
    HIP_TRY(e->h_sk_in.reserve(((size_t)3 * std::max<uint32_t>(J, 1) + (size_t)std::max<uint32_t>(n_runs, 1)) * 4,
                               grave(e)));
    HIP_TRY(e->h_sk_runs.reserve((size_t)2 * std::max<uint32_t>(n_runs, 1) * 4, grave(e)));
    int32_t* h_prev = e->h_sk_in.as<int32_t>();
    uint32_t* h_jr = e->h_sk_in.as<uint32_t>() + J;
    uint32_t* h_jc = h_jr + J;
    uint32_t* h_rl = h_jc + J;
    uint32_t* f_rc = e->h_sk_runs.as<uint32_t>();  // the fill's run list: the classes, then the remaining lengths
    uint32_t* f_rl = f_rc + n_runs;
    uint32_t hinted = 0;
    {
        uint32_t j = 0, r = 0;
        for (uint32_t i = 0; i < n_runs_in; ++i) {
            if (run_len[i] == 0) continue;
            const uint32_t Dl = e->D[e->cls_h[run_class[i]].level];
            f_rc[r] = run_class[i];
            h_rl[r] = run_len[i];
            for (uint32_t q = 0; q < run_len[i]; ++q, ++j) {
                const int32_t d = prev ? prev[j] : -1;
                if (d < -1 || (d >= 0 && (uint32_t)d >= Dl))
                    return set_err(JSP_EINVAL, "job %u: previous domain %d out of range [-1,%u) at level %u", j, d, Dl,
                                   e->cls_h[run_class[i]].level);
                h_prev[j] = d;
                h_jr[j] = r;
                h_jc[j] = run_class[i];
                hinted += d >= 0 ? 1u : 0u;
            }
            ++r;
        }
    }
    if (J == 0) {
        if (stats) {
            *stats = jsp_sticky_stats{};
            stats->wall_us = us_between(t0);
        }
        at_rest.ok = true;
        return JSP_OK;
    }
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    const bool grid = J > jsp::kStickyOneMax || e->hooks.sticky_grid;
    const uint32_t DT = jsp::sticky_dom_off(e->D, e->K);
    HIP_TRY(e->sk_tab.reserve((size_t)2 * std::max<uint32_t>(DT, 1) * 4, grave(e)));
    HIP_TRY(e->sk_taken.reserve((size_t)std::max<uint32_t>(e->t_off_h[e->K], 1) * 8, grave(e)));
    if (!e->sk_tab_ready) {
        HIP_TRY(hipMemsetAsync(e->sk_taken.p, 0, e->sk_taken.bytes, s));
        HIP_TRY(hipMemsetAsync(e->sk_tab.p, 0xFF, e->sk_tab.bytes, s));
        e->sk_tab_ready = true;
    }
    // the fill walks on the host: the host scatters too, from a host-mapped job map
    const bool host_fill = host_walk_ok(e, n_runs, J);
    if (host_fill) HIP_TRY(e->h_sk_map.reserve((size_t)J * 4, grave(e)));
    else HIP_TRY(e->sk_map.reserve((size_t)J * 4, grave(e)));
    HIP_TRY(e->sk_nrem.reserve(16));
    HIP_TRY(e->h_sk_fill.reserve((size_t)J * 4, grave(e)));
    HIP_TRY(e->h_sk_stat.reserve(16));
    HIP_TRY(e->h_assign.reserve((size_t)J * 4, grave(e)));
    HIP_TRY(e->h_stats.reserve(16));
    jsp::StickyArgs a{};
    a.prev = h_prev;
    a.job_run = h_jr;
    a.job_cls = h_jc;
    a.run_len = h_rl;
    if (grid) {
        const uint32_t n_wg = (J + jsp::kStickyGridThreads - 1) / jsp::kStickyGridThreads;
        const size_t in_bytes = ((size_t)3 * J + (size_t)n_runs) * 4;
        HIP_TRY(e->sk_in.reserve(in_bytes, grave(e)));
        HIP_TRY(e->sk_state.reserve((size_t)J * 4, grave(e)));
        HIP_TRY(e->sk_wg.reserve((size_t)n_wg * 4, grave(e)));
        // (a buffer that grew may come back at the address of the one it
        // replaced, with whatever that memory holds now: its size counts too)
        const size_t kept_bytes = e->sk_run_kept.bytes;
        HIP_TRY(e->sk_run_kept.reserve((size_t)n_runs * 4, grave(e)));
        if (e->sk_run_kept.p != e->sk_run_kept_p || e->sk_run_kept.bytes != kept_bytes) {
            HIP_TRY(hipMemsetAsync(e->sk_run_kept.p, 0, e->sk_run_kept.bytes, s));
            e->sk_run_kept_p = e->sk_run_kept.p;
        }
        HIP_TRY(hipMemcpyAsync(e->sk_in.p, e->h_sk_in.p, in_bytes, hipMemcpyHostToDevice, s));
        a.prev = e->sk_in.as<int32_t>();
        a.job_run = e->sk_in.as<uint32_t>() + J;
        a.job_cls = a.job_run + J;
        a.run_len = a.job_cls + J;
        a.state = e->sk_state.as<uint32_t>();
        a.run_kept = e->sk_run_kept.as<uint32_t>();
        a.wg_rem = e->sk_wg.as<uint32_t>();
    }
    a.n_runs = n_runs;
    a.J = J;
    a.cls = e->cls.as<jsp::DevClass>();
    a.C = e->C;
    a.word_off = e->word_off.as<uint32_t>();
    a.feas = e->feas.as<uint64_t>();
    a.topo = e->topo;
    a.taken = e->sk_taken.as<unsigned long long>();
    a.t_words = e->t_off_h[e->K];
    a.own = e->sk_tab.as<uint32_t>();
    a.sub = a.own + std::max<uint32_t>(DT, 1);
    a.assign = e->h_assign.as<int32_t>();
    a.rem_len = f_rl;
    a.map = host_fill ? e->h_sk_map.as<uint32_t>() : e->sk_map.as<uint32_t>();
    a.n_rem = e->sk_nrem.as<uint32_t>();
    a.kept_out = e->h_sk_stat.as<uint32_t>();
    uint32_t* cap = e->cap.as<uint32_t>();
    uint32_t* occ = e->occ.as<uint32_t>();
    if (int rc = tally_whole(e, s)) return rc;
    if (int rc = feas_launch(e, cap, occ, e->L_total, a.feas, s)) return rc;
    if (grid) HIP_TRY(jsp::launch_sticky_keep_grid(a, s));
    else HIP_TRY(jsp::launch_sticky_keep_one(a, s));
    e->stats_override = e->h_stats.as<uint32_t>();
    const int frc = assign_impl(e, cap, occ, e->L_total, f_rc, f_rl, n_runs, J, e->h_sk_fill.as<int32_t>(), s, true, true);
    e->stats_override = nullptr;
    if (frc) return frc;
    if (host_fill) {
        // the walk waited for the stream's last launch: the keepers' answers, the
        // map and the keeper count are in host memory and nothing is in flight
        const uint32_t n_rem = J - e->h_sk_stat.as<uint32_t>()[0];
        const uint32_t* map = e->h_sk_map.as<uint32_t>();
        const int32_t* fill = e->h_sk_fill.as<int32_t>();
        int32_t* out = e->h_assign.as<int32_t>();
        for (uint32_t r = 0; r < n_rem && r < J; ++r)
            if (map[r] < J) out[map[r]] = fill[r];
    } else {
        HIP_TRY(jsp::launch_sticky_scatter(e->h_sk_fill.as<int32_t>(), a.map, a.n_rem, J, a.assign, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    std::memcpy(assign_out, e->h_assign.p, (size_t)J * 4);
    if (int rc = check_launch_error(e)) return rc;
    if (stats) {
        const uint32_t kept = e->h_sk_stat.as<uint32_t>()[0];
        stats->jobs = J;
        stats->placed = kept + e->h_stats.as<uint32_t>()[1];
        stats->hinted = hinted;
        stats->kept = kept;
        stats->runs = e->h_stats.as<uint32_t>()[0];
        stats->fused = host_fill ? 7u : 0u;
        stats->wall_us = us_between(t0);
    }
    at_rest.ok = true;
    return JSP_OK;
}

int jsp_place_sticky(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                     const int32_t* prev_assign, int32_t* assign_out, jsp_sticky_stats* stats) {
    if (int rc = check_engine(e)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    jsp_sticky_stats local{};
    jsp_sticky_stats* st = stats ? stats : &local;
    const int rc = sticky_call(e, run_class, run_len, n_runs, prev_assign, assign_out, st);
    return record_placement(e, us_between(t0), rc, st->jobs, st->placed);
}

int jspb_place_sticky_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                           const int32_t* prev_assign, int32_t* assign_out, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (int rc = check_timed(iters, 1000000, out_us)) return rc;
    return timed_calls(iters, out_us, [&](uint32_t) {
        return jsp_place_sticky(e, run_class, run_len, n_runs, prev_assign, assign_out, nullptr);
    });
}

// ---- gang placement (DESIGN.md §2 "Gang placement") ----
// The span counts' rows, one per class c and span level s <= level[c], the
// thread form's first. form 0: by the mean segment (kSpanWaveDomains);
// 1 / 2: every row in the thread / the wave form (jspb_span_counts).
static int gang_rows(jsp_engine* e, int form, hipStream_t s) {
    if (e->gs_ready && e->gs_form == form) return JSP_OK;
    e->gs_ready = false;
    e->walk.gang_layout(e->gs_state);
    std::vector<jsp::SpanRow> th, wv;
    uint32_t mt = 0, mw = 0, woff = 0;
    for (uint32_t c = 0; c < e->C; ++c) {
        const uint32_t lc = e->cls_h[c].level;
        for (uint32_t k = 0; k <= lc; ++k) {
            jsp::SpanRow r{};
            r.word0 = woff;
            r.s = k;
            r.lc = lc;
            r.D = e->D[k];
            r.cnt_off = e->gs_state.span_off(c, k);
            const bool wave = form == 2 || (form == 0 && e->D[lc] > jsp::kSpanWaveDomains * std::max<uint32_t>(e->D[k], 1));
            (wave ? wv : th).push_back(r);
            (wave ? mw : mt) = std::max(wave ? mw : mt, r.D);
        }
        woff += (e->D[lc] + 63) / 64;
    }
    e->gs_n_thread = (uint32_t)th.size();
    e->gs_n_wave = (uint32_t)wv.size();
    e->gs_max_thread = mt;
    e->gs_max_wave = mw;
    e->gs_rows_h = th;
    e->gs_rows_h.insert(e->gs_rows_h.end(), wv.begin(), wv.end());
    HIP_TRY(upload(e->gs_rows, e->gs_rows_h.data(), e->gs_rows_h.size(), s, grave(e)));
    HIP_TRY(e->h_gs_cnt.reserve(((size_t)e->gs_state.span_total() + 1) * 4, grave(e)));
    e->gs_form = form;
    e->gs_ready = true;
    return JSP_OK;
}

// the span counts of the feasibility words in e->feas, into the pinned counts
static int gang_counts(jsp_engine* e, hipStream_t s) {
    const jsp::SpanRow* rows = e->gs_rows.as<jsp::SpanRow>();
    uint32_t* cnt = e->h_gs_cnt.as<uint32_t>();
    HIP_TRY(jsp::launch_span_counts(e->feas.as<uint64_t>(), e->topo, rows, 0, e->gs_n_thread, e->gs_max_thread, false,
                                    cnt, s));
    HIP_TRY(jsp::launch_span_counts(e->feas.as<uint64_t>(), e->topo, rows, e->gs_n_thread, e->gs_n_wave,
                                    e->gs_max_wave, true, cnt, s));
    return JSP_OK;
}

// tally, feasibility words (device, and their pinned copy for the walk), span counts
static int gang_device_part(jsp_engine* e, hipStream_t s) {
    if (int rc = tally_whole(e, s)) return rc;
    if (int rc = feas_launch(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, e->feas.as<uint64_t>(), s))
        return rc;
    HIP_TRY(jsp::launch_copy_u32(e->feas.as<uint32_t>(), e->hw_feas.as<uint32_t>(), 2 * e->feas_words, s));
    return gang_counts(e, s);
}

// the host's wait for the device part, by a tag behind its launches
static int gang_wait(jsp_engine* e, hipStream_t s) {
    StreamTag tag{};
    if (int rc = tag_post(e, s, &tag)) return rc;
    return tag_wait(e, s, tag, {"gang placement: the span counts", "their", "gang placement: the device part",
                                "gang placement: the device part"});
}

// The argument checks, the engine stream behind every pending patch, tally +
// feasibility + span counts into host-visible memory, the wait, the gang walk
// on the host (jsp_walk.cc walk_gangs).
static int gang_call(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                     const uint32_t* gang_runs, const uint32_t* gang_span, uint32_t n_gangs, uint32_t flags,
                     int32_t* assign_out, int32_t* gang_span_out, jsp_gang_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jsp_place_gangs", g)) return rc;
    if (flags != 0) return set_err(JSP_EINVAL, "jsp_place_gangs: flags %u must be 0 (for every gang)", flags);
    if (n_runs > 0 && (!run_class || !run_len)) return set_err(JSP_EINVAL, "jsp_place_gangs: run buffers are NULL (gang 0)");
    if (n_gangs > 0 && (!gang_runs || !gang_span)) return set_err(JSP_EINVAL, "jsp_place_gangs: gang buffers are NULL (gang 0)");
    uint64_t covered = 0;
    for (uint32_t g2 = 0; g2 < n_gangs; ++g2) {
        covered += gang_runs[g2];
        if (covered > n_runs)
            return set_err(JSP_EINVAL, "gang %u: the gangs' runs reach %llu, past the %u runs given", g2,
                           (unsigned long long)covered, n_runs);
    }
    if (covered != n_runs)
        return set_err(JSP_EINVAL, "gang %u is the last and the gangs cover %llu of %u runs", n_gangs ? n_gangs - 1 : 0u,
                       (unsigned long long)covered, n_runs);
    uint64_t J64 = 0;
    uint32_t runs_walked = 0;
    {
        uint32_t r = 0;
        for (uint32_t g2 = 0; g2 < n_gangs; ++g2) {
            const uint32_t sp = gang_span[g2];
            if (sp != JSP_SPAN_ANY && sp >= e->K)
                return set_err(JSP_EINVAL, "gang %u: span %u is neither the whole-cluster span nor a level below %u", g2, sp, e->K);
            for (uint32_t q = 0; q < gang_runs[g2]; ++q, ++r) {
                if (run_class[r] >= e->C)
                    return set_err(JSP_EINVAL, "gang %u: run %u: class %u out of range (%u classes)", g2, r, run_class[r],
                                   e->C);
                if (run_len[r] == 0) continue;
                const uint32_t lc = e->cls_h[run_class[r]].level;
                if (sp != JSP_SPAN_ANY && sp > lc)
                    return set_err(JSP_EINVAL, "gang %u: span level %u is finer than level %u of class %u (run %u)", g2, sp,
                                   lc, run_class[r], r);
                J64 += run_len[r];
                runs_walked += 1;
            }
        }
    }
    if (J64 > JSP_GANG_MAX_JOBS)
        return set_err(JSP_ERANGE, "%llu jobs in the gangs exceed the limit of %u per call", (unsigned long long)J64,
                       JSP_GANG_MAX_JOBS);
    const uint32_t J = (uint32_t)J64;
    if (J > 0 && !assign_out) return set_err(JSP_EINVAL, "jsp_place_gangs: assign_out is NULL (gang 0)");
    uint32_t placed = 0, gangs_placed = 0;
    if (J == 0) {
        for (uint32_t g2 = 0; gang_span_out && g2 < n_gangs; ++g2) gang_span_out[g2] = -1;
    } else {
        hipStream_t s = nullptr;
        if (int rc = enter_engine_stream(e, false, &s)) return rc;
        HIP_TRY(e->hw_feas.reserve((size_t)std::max<uint32_t>(e->feas_words, 1) * 8 + 64, grave(e)));
        if (int rc = gang_rows(e, 0, s)) return rc;
        if (int rc = gang_device_part(e, s)) return rc;
        if (int rc = gang_wait(e, s)) return rc;
        placed = e->walk.walk_gangs(e->gs_state, e->hw_feas.as<uint64_t>(), e->h_gs_cnt.as<uint32_t>(), run_class, run_len, n_runs,
                                    gang_runs, gang_span, n_gangs, assign_out, gang_span_out, &gangs_placed);
        if (int rc = check_launch_error(e)) return rc;
    }
    if (stats) {
        stats->jobs = J;
        stats->placed = placed;
        stats->gangs = n_gangs;
        stats->gangs_placed = gangs_placed;
        stats->runs = runs_walked;
        stats->fused = 7u;
        stats->wall_us = us_between(t0);
    }
    return JSP_OK;
}

int jsp_place_gangs(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                    const uint32_t* gang_runs, const uint32_t* gang_span, uint32_t n_gangs, uint32_t flags,
                    int32_t* assign_out, int32_t* gang_span_out, jsp_gang_stats* stats) {
    if (int rc = check_engine(e)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    jsp_gang_stats local{};
    jsp_gang_stats* st = stats ? stats : &local;
    const int rc = gang_call(e, run_class, run_len, n_runs, gang_runs, gang_span, n_gangs, flags, assign_out,
                             gang_span_out, st);
    return record_placement(e, us_between(t0), rc, st->jobs, st->placed);
}

int jspb_place_gangs_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                          const uint32_t* gang_runs, const uint32_t* gang_span, uint32_t n_gangs, int32_t* assign_out,
                          int32_t* gang_span_out, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (int rc = check_timed(iters, 1000000, out_us)) return rc;
    return timed_calls(iters, out_us, [&](uint32_t) {
        return jsp_place_gangs(e, run_class, run_len, n_runs, gang_runs, gang_span, n_gangs, 0, assign_out,
                               gang_span_out, nullptr);
    });
}

int jspb_span_counts(jsp_engine* e, int form, uint32_t* cnt_out, uint32_t n_cnt, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jspb_span_counts", g)) return rc;
    if (form < 0 || form > 2) return set_err(JSP_EINVAL, "form %d out of range [0,2]", form);
    if (!e->gs_ready) e->walk.gang_layout(e->gs_state);
    if (n_cnt != e->gs_state.span_total())
        return set_err(JSP_EINVAL, "n_cnt %u is not the %u span counts of the classes", n_cnt, e->gs_state.span_total());
    if (n_cnt > 0 && !cnt_out) return set_err(JSP_EINVAL, "cnt_out is NULL");
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    HIP_TRY(e->hw_feas.reserve((size_t)std::max<uint32_t>(e->feas_words, 1) * 8 + 64, grave(e)));
    if (int rc = gang_rows(e, form, s)) return rc;
    // a canary behind the last count: the kernels write inside their rows only
    e->h_gs_cnt.as<uint32_t>()[n_cnt] = 0xC0FFEE00u;
    if (int rc = gang_device_part(e, s)) return rc;
    if (int rc = gang_wait(e, s)) return rc;
    if (e->h_gs_cnt.as<uint32_t>()[n_cnt] != 0xC0FFEE00u)
        return set_err(JSP_EHIP, "span counts: a count was written past the classes' rows");
    std::memcpy(cnt_out, e->h_gs_cnt.p, (size_t)n_cnt * 4);
    if (iters > 0 && n_cnt > 0) {
        if (int rc = time_steps(e, iters, nullptr, 0, out_us, [&](hipStream_t st) { return gang_counts(e, st); }))
            return rc;
    }
    return check_launch_error(e);
}

// ---- fit placement (DESIGN.md §2 "Fit placement") ----
// The order step's rows, one per class, the rank form's first, and its
// buffers. form 0: by the segment size (kFitRankMax), or what the fit_form
// hook forces; 1 / 2: every class in the rank / the block form.
// keys per block of the block form: the fit_block hook's, else kFitBlock, cut
// to the power of two that holds the longest block-form segment
static uint32_t fit_block_keys(const jsp_engine* e) {
    if (e->hooks.fit_block) return e->hooks.fit_block;
    uint32_t B = 64;
    while (B < jsp::kFitBlock && B < e->fit_max_block) B <<= 1;
    return B;
}

static int fit_rows(jsp_engine* e, int form, hipStream_t s) {
    if (form == 0) form = (int)e->hooks.fit_form;
    if (e->fit_ready && e->fit_form == form) return JSP_OK;
    e->fit_ready = false;
    std::vector<jsp::FitRow> rk, bl;
    uint32_t mr = 0, mb = 0, mt = 0, woff = 0, off = 0;
    e->fit_off_h.assign(e->C + 1, 0u);
    for (uint32_t c = 0; c < e->C; ++c) {
        const uint32_t lvl = e->cls_h[c].level, D = e->D[lvl];
        jsp::FitRow r{};
        r.c = c;
        r.word0 = woff;
        r.lvl = lvl;
        r.D = D;
        r.off = off;
        // lanes per domain in the keys launch: about 8 leaves per lane of the mean domain
        const uint32_t mean = lvl + 1 < e->K ? e->L_total / std::max<uint32_t>(D, 1) : 1u;
        while (r.shift < 6 && (8u << r.shift) < mean) r.shift += 1;
        mt = std::max(mt, D << r.shift);
        const bool block = form == 2 || (form == 0 && D > jsp::kFitRankMax);
        (block ? bl : rk).push_back(r);
        (block ? mb : mr) = std::max(block ? mb : mr, D);
        e->fit_off_h[c] = off;
        woff += (D + 63) / 64;
        off += D;
    }
    e->fit_off_h[e->C] = off;
    e->fit_n = off;
    e->fit_n_rank = (uint32_t)rk.size();
    e->fit_n_block = (uint32_t)bl.size();
    e->fit_max_rank = mr;
    e->fit_max_block = mb;
    e->fit_max_threads = mt;
    e->fit_rows_h = rk;
    e->fit_rows_h.insert(e->fit_rows_h.end(), bl.begin(), bl.end());
    HIP_TRY(upload(e->fit_rows, e->fit_rows_h.data(), e->fit_rows_h.size(), s, grave(e)));
    const size_t n = std::max<uint32_t>(off, 1);
    HIP_TRY(e->fit_keys.reserve(n * 8, grave(e)));
    HIP_TRY(e->fit_sorted.reserve(n * 8, grave(e)));
    HIP_TRY(e->fit_out.reserve((2 * n + e->C + 1) * 4, grave(e)));
    HIP_TRY(e->h_fit_out.reserve((2 * n + e->C + 1) * 4, grave(e)));
    e->fit_form = form;
    e->fit_ready = true;
    return JSP_OK;
}

// the order step: keys, then each class's list in its form, from the
// feasibility words in e->feas and the tally in e->cap
static int fit_order_step(jsp_engine* e, uint32_t policy, hipStream_t s) {
    const jsp::FitRow* rows = e->fit_rows.as<jsp::FitRow>();
    uint32_t* order = e->fit_out.as<uint32_t>();
    HIP_TRY(jsp::launch_fit_keys(e->cap.as<uint32_t>(), e->L_total, e->feas.as<uint64_t>(), e->topo, rows, e->C,
                                 e->fit_max_threads, policy, e->fit_keys.as<uint64_t>(), order + e->fit_n,
                                 order + 2 * (size_t)e->fit_n, s));
    const uint32_t* nf = order + 2 * (size_t)e->fit_n;
    HIP_TRY(jsp::launch_fit_rank(e->fit_keys.as<uint64_t>(), rows, 0, e->fit_n_rank, e->fit_max_rank, nf, order, s));
    HIP_TRY(jsp::launch_fit_blocks(e->fit_keys.as<uint64_t>(), e->fit_sorted.as<uint64_t>(), rows, e->fit_n_rank,
                                   e->fit_n_block, e->fit_max_block, fit_block_keys(e), nf, order, s));
    return JSP_OK;
}

// tally, feasibility words, the order step, and its output into pinned memory
static int fit_device_part(jsp_engine* e, uint32_t policy, hipStream_t s) {
    if (int rc = tally_whole(e, s)) return rc;
    if (int rc = feas_launch(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, e->feas.as<uint64_t>(), s))
        return rc;
    if (int rc = fit_order_step(e, policy, s)) return rc;
    HIP_TRY(jsp::launch_copy_u32(e->fit_out.as<uint32_t>(), e->h_fit_out.as<uint32_t>(), 2 * e->fit_n + e->C, s));
    return JSP_OK;
}

// the host's wait for the device part, by a tag behind its launches
static int fit_wait(jsp_engine* e, hipStream_t s) {
    StreamTag tag{};
    if (int rc = tag_post(e, s, &tag)) return rc;
    return tag_wait(e, s, tag, {"fit placement: the order lists", "their", "fit placement: the device part",
                                "fit placement: the device part"});
}

// The argument checks, the engine stream behind every pending patch, tally +
// feasibility + order lists into host-visible memory, the wait, the fit walk
// on the host (jsp_walk.cc walk_fit).
static int fit_call(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, uint32_t policy,
                    uint32_t flags, int32_t* assign_out, jsp_fit_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jsp_place_fit", g)) return rc;
    if (flags != 0) return set_err(JSP_EINVAL, "jsp_place_fit: flags %u must be 0", flags);
    if (policy >= jsp::kFitPolicies)
        return set_err(JSP_EINVAL, "jsp_place_fit: policy %u is none of lowest (0), tightest (1), roomiest (2)", policy);
    if (n_runs > 0 && (!run_class || !run_len)) return set_err(JSP_EINVAL, "jsp_place_fit: run buffers are NULL (run 0)");
    uint64_t J64 = 0;
    uint32_t runs_walked = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        if (run_class[r] >= e->C)
            return set_err(JSP_EINVAL, "run %u: class %u out of range (%u classes)", r, run_class[r], e->C);
        J64 += run_len[r];
        runs_walked += run_len[r] != 0;
    }
    if (J64 > JSP_FIT_MAX_JOBS)
        return set_err(JSP_ERANGE, "%llu jobs in the runs exceed the limit of %u per call", (unsigned long long)J64,
                       JSP_FIT_MAX_JOBS);
    const uint32_t J = (uint32_t)J64;
    if (J > 0 && !assign_out) return set_err(JSP_EINVAL, "jsp_place_fit: assign_out is NULL (run 0)");
    uint32_t placed = 0;
    uint64_t slack = 0;
    if (J > 0) {
        hipStream_t s = nullptr;
        if (int rc = enter_engine_stream(e, false, &s)) return rc;
        HIP_TRY(e->hw_feas.reserve((size_t)std::max<uint32_t>(e->feas_words, 1) * 8 + 64, grave(e)));  // the tag word
        if (int rc = fit_rows(e, 0, s)) return rc;
        if (int rc = fit_device_part(e, policy, s)) return rc;
        if (int rc = fit_wait(e, s)) return rc;
        const uint32_t* out = e->h_fit_out.as<uint32_t>();
        placed = e->walk.walk_fit(out, out + 2 * (size_t)e->fit_n, e->fit_off_h.data(), out + e->fit_n, run_class, run_len,
                                  n_runs, assign_out, &slack);
        if (int rc = check_launch_error(e)) return rc;
    }
    if (stats) {
        stats->jobs = J;
        stats->placed = placed;
        stats->runs = runs_walked;
        stats->fused = 7u;
        stats->slack = slack;
        stats->wall_us = us_between(t0);
    }
    return JSP_OK;
}

int jsp_place_fit(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, uint32_t policy,
                  uint32_t flags, int32_t* assign_out, jsp_fit_stats* stats) {
    if (int rc = check_engine(e)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    jsp_fit_stats local{};
    jsp_fit_stats* st = stats ? stats : &local;
    const int rc = fit_call(e, run_class, run_len, n_runs, policy, flags, assign_out, st);
    return record_placement(e, us_between(t0), rc, st->jobs, st->placed);
}

int jspb_place_fit_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                        uint32_t policy, int32_t* assign_out, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (int rc = check_timed(iters, 1000000, out_us)) return rc;
    return timed_calls(iters, out_us, [&](uint32_t) {
        return jsp_place_fit(e, run_class, run_len, n_runs, policy, 0, assign_out, nullptr);
    });
}

int jspb_fit_order(jsp_engine* e, uint32_t policy, int form, uint32_t* order_out, uint32_t n_order, uint32_t* nf_out,
                   uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jspb_fit_order", g)) return rc;
    if (form < 0 || form > 2) return set_err(JSP_EINVAL, "form %d out of range [0,2]", form);
    if (policy >= jsp::kFitPolicies) return set_err(JSP_EINVAL, "policy %u out of range [0,2]", policy);
    uint64_t total = 0;
    for (uint32_t c = 0; c < e->C; ++c) total += e->D[e->cls_h[c].level];
    if (n_order != total)
        return set_err(JSP_EINVAL, "n_order %u is not the %llu entries of the classes' segments", n_order,
                       (unsigned long long)total);
    if ((n_order > 0 && !order_out) || !nf_out) return set_err(JSP_EINVAL, "order_out or nf_out is NULL");
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    HIP_TRY(e->hw_feas.reserve((size_t)std::max<uint32_t>(e->feas_words, 1) * 8 + 64, grave(e)));
    if (int rc = fit_rows(e, form, s)) return rc;
    // a canary behind the output's last word: the copy and the kernels write inside it only
    uint32_t* out = e->h_fit_out.as<uint32_t>();
    const size_t n_out = 2 * (size_t)e->fit_n + e->C;
    HIP_TRY(hipMemsetAsync(e->fit_out.p, 0xA5, (n_out + 1) * 4, s));
    out[n_out] = 0xC0FFEE00u;
    if (int rc = fit_device_part(e, policy, s)) return rc;
    if (int rc = fit_wait(e, s)) return rc;
    if (out[n_out] != 0xC0FFEE00u) return set_err(JSP_EHIP, "fit order: a word was written past the output");
    std::memcpy(order_out, out, (size_t)n_order * 4);
    std::memcpy(nf_out, out + 2 * (size_t)e->fit_n, (size_t)e->C * 4);
    if (iters > 0 && n_order > 0) {
        if (int rc = time_steps(e, iters, nullptr, 0, out_us, [&](hipStream_t st) { return fit_order_step(e, policy, st); }))
            return rc;
    }
    return check_launch_error(e);
}

// ---- what-if placement (DESIGN.md §2 "What-if placement") ----
// The staging of one call: {scen_off [S + 1], rows [n]} then, 8-byte aligned,
// the present delta columns in jsp_snapshot_patch's order.
struct WhatifLayout {
    size_t rows, lab, taint, free, excl, bytes;
};
static WhatifLayout whatif_layout(uint32_t S, uint32_t n, uint32_t W, uint32_t R, bool lab, bool taint, bool free_res,
                                  bool excl) {
    WhatifLayout L{};
    L.rows = ((size_t)S + 1) * 4;
    size_t o = (L.rows + (size_t)n * 4 + 7) & ~size_t(7);
    L.lab = o;
    if (lab) o += (size_t)W * n * 8;
    L.taint = o;
    if (taint) o += (size_t)n * 4;
    L.free = o;
    if (free_res) o += (size_t)R * n * 4;
    L.excl = o;
    if (excl) o += (size_t)n * 4;
    L.bytes = o;
    return L;
}

// tally, feasibility words, the scenarios' staged rows to the device, the
// scenarios' words (and flip counts) built there and copied to pinned memory
static int whatif_device_part(jsp_engine* e, const WhatifLayout& L, uint32_t S, uint32_t n_total, uint32_t max_rows,
                              bool lab, bool taint, bool free_res, bool excl, hipStream_t s) {
    if (int rc = tally_whole(e, s)) return rc;
    if (int rc = feas_launch(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, e->feas.as<uint64_t>(), s))
        return rc;
    HIP_TRY(e->wi_in.reserve(L.bytes, grave(e)));
    HIP_TRY(hipMemcpyAsync(e->wi_in.p, e->h_wi_in.p, L.bytes, hipMemcpyHostToDevice, s));
    const char* in = e->wi_in.as<char>();
    jsp::WhatifArgs h{};
    h.scen_off = reinterpret_cast<const uint32_t*>(in);
    h.rows = reinterpret_cast<const uint32_t*>(in + L.rows);
    h.dlab = lab ? reinterpret_cast<const uint64_t*>(in + L.lab) : nullptr;
    h.dtaint = taint ? reinterpret_cast<const uint32_t*>(in + L.taint) : nullptr;
    h.dfree = free_res ? reinterpret_cast<const uint32_t*>(in + L.free) : nullptr;
    h.dexcl = excl ? reinterpret_cast<const int32_t*>(in + L.excl) : nullptr;
    h.n_total = n_total;
    h.S = S;
    h.C = e->C;
    h.cap = e->cap.as<uint32_t>();
    h.occ = e->occ.as<uint32_t>();
    h.ld = e->L_total;
    h.feas = e->feas.as<uint64_t>();
    h.word_off = e->word_off.as<uint32_t>();
    h.feas_words = e->feas_words;
    h.n_leaves = e->n_leaves;
    h.topo = e->topo;
    h.out = e->wi_out.as<uint64_t>();
    h.flips = reinterpret_cast<uint32_t*>(h.out + (size_t)S * e->feas_words);
    HIP_TRY(jsp::launch_whatif(tally_args(e, nullptr, nullptr, e->L_total), h, max_rows, s));
    HIP_TRY(jsp::launch_copy_u32(e->wi_out.as<uint32_t>(), e->h_wi_out.as<uint32_t>(),
                                 (uint32_t)(2 * (size_t)S * e->feas_words + (size_t)S * e->C), s));
    return JSP_OK;
}

// the host's wait for the device part, by a tag behind its launches
static int whatif_wait(jsp_engine* e, hipStream_t s) {
    StreamTag tag{};
    if (int rc = tag_post(e, s, &tag)) return rc;
    return tag_wait(e, s, tag, {"what-if placement: the scenarios' words", "their", "what-if placement: the device part",
                                "what-if placement: the device part"});
}

// The argument checks, the engine stream behind every pending patch, tally +
// feasibility + the scenarios' words into host-visible memory, the wait, one
// lowest-index walk per scenario on the host (jsp_walk.cc walk). Nothing the
// placement paths read is written: no row, no service state, no lease.
static int whatif_call(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                       const uint32_t* scen_off, uint32_t n_scen, const uint32_t* rows, const uint64_t* labels,
                       const uint32_t* taints, const uint32_t* free_res, const int32_t* excl_owner, uint32_t flags,
                       int32_t* assign_out, uint32_t* placed_out, jsp_whatif_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jsp_place_whatif", g)) return rc;
    if (flags != 0) return set_err(JSP_EINVAL, "jsp_place_whatif: flags %u must be 0", flags);
    if (n_runs > 0 && (!run_class || !run_len))
        return set_err(JSP_EINVAL, "jsp_place_whatif: run buffers are NULL (run 0)");
    if (n_scen > JSP_WHATIF_MAX_SCENARIOS)
        return set_err(JSP_ERANGE, "%u scenarios exceed the limit of %u per call", n_scen, JSP_WHATIF_MAX_SCENARIOS);
    if (n_scen > 0 && !scen_off) return set_err(JSP_EINVAL, "jsp_place_whatif: scen_off is NULL (scenario 0)");
    if (n_scen > 0 && scen_off[0] != 0)
        return set_err(JSP_EINVAL, "scenario 0: scen_off[0] is %u, not 0", scen_off[0]);
    uint32_t max_rows = 0;
    for (uint32_t sc = 0; sc < n_scen; ++sc) {
        if (scen_off[sc + 1] < scen_off[sc])
            return set_err(JSP_EINVAL, "scenario %u: scen_off decreases from %u to %u", sc, scen_off[sc], scen_off[sc + 1]);
        max_rows = std::max(max_rows, scen_off[sc + 1] - scen_off[sc]);
    }
    const uint32_t n_total = n_scen ? scen_off[n_scen] : 0u;
    if (n_total > JSP_WHATIF_MAX_ROWS)
        return set_err(JSP_ERANGE, "%u rows in the scenarios exceed the limit of %u per call", n_total, JSP_WHATIF_MAX_ROWS);
    uint64_t J64 = 0;
    uint32_t runs_walked = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        if (run_class[r] >= e->C)
            return set_err(JSP_EINVAL, "run %u: class %u out of range (%u classes)", r, run_class[r], e->C);
        J64 += run_len[r];
        runs_walked += run_len[r] != 0;
    }
    if (J64 > JSP_WHATIF_MAX_JOBS)
        return set_err(JSP_ERANGE, "%llu jobs in the runs exceed the limit of %u per call", (unsigned long long)J64,
                       JSP_WHATIF_MAX_JOBS);
    const uint32_t J = (uint32_t)J64;
    if (n_scen > 0 && J > 0 && !assign_out) return set_err(JSP_EINVAL, "jsp_place_whatif: assign_out is NULL (scenario 0)");
    if (n_total > 0 && !rows) return set_err(JSP_EINVAL, "jsp_place_whatif: rows is NULL (scenario 0)");
    if (n_total > 0 && !labels && !taints && !free_res && !excl_owner)
        return set_err(JSP_EINVAL, "jsp_place_whatif: all four delta columns are NULL (scenario 0)");
    for (uint32_t sc = 0; sc < n_scen; ++sc)
        for (uint32_t i = scen_off[sc]; i < scen_off[sc + 1]; ++i) {
            if (rows[i] >= e->N)
                return set_err(JSP_EINVAL, "scenario %u: position %u: row %u out of range (%u rows)", sc,
                               i - scen_off[sc], rows[i], e->N);
            if (i > scen_off[sc] && rows[i] <= rows[i - 1])
                return set_err(JSP_EINVAL, "scenario %u: position %u: row %u after row %u is not strictly ascending", sc,
                               i - scen_off[sc], rows[i], rows[i - 1]);
        }
    uint32_t flips = 0;
    if (n_scen > 0 && J > 0) {
        const uint32_t W = e->W, R = e->R;
        const WhatifLayout L = whatif_layout(n_scen, n_total, W, R, labels, taints, free_res, excl_owner);
        hipStream_t s = nullptr;
        if (int rc = enter_engine_stream(e, false, &s)) return rc;
        HIP_TRY(e->hw_feas.reserve((size_t)std::max<uint32_t>(e->feas_words, 1) * 8 + 64, grave(e)));  // the tag word
        const size_t out_bytes = (size_t)n_scen * e->feas_words * 8 + (size_t)n_scen * e->C * 4;
        HIP_TRY(e->h_wi_in.reserve(L.bytes, grave(e)));
        HIP_TRY(e->wi_out.reserve(out_bytes, grave(e)));
        HIP_TRY(e->h_wi_out.reserve(out_bytes, grave(e)));
        char* in = e->h_wi_in.as<char>();
        std::memcpy(in, scen_off, ((size_t)n_scen + 1) * 4);
        if (n_total > 0) {
            std::memcpy(in + L.rows, rows, (size_t)n_total * 4);
            if (labels) std::memcpy(in + L.lab, labels, (size_t)W * n_total * 8);
            if (taints) std::memcpy(in + L.taint, taints, (size_t)n_total * 4);
            if (free_res) std::memcpy(in + L.free, free_res, (size_t)R * n_total * 4);
            if (excl_owner) std::memcpy(in + L.excl, excl_owner, (size_t)n_total * 4);
        }
        if (int rc = whatif_device_part(e, L, n_scen, n_total, max_rows, labels, taints, free_res, excl_owner, s))
            return rc;
        if (int rc = whatif_wait(e, s)) return rc;
        const uint64_t* words = e->h_wi_out.as<uint64_t>();
        const uint32_t* fl = reinterpret_cast<const uint32_t*>(words + (size_t)n_scen * e->feas_words);
        for (uint32_t sc = 0; sc < n_scen; ++sc) {
            const uint32_t placed =
                e->walk.walk(words + (size_t)sc * e->feas_words, run_class, run_len, n_runs, assign_out + (size_t)sc * J);
            if (placed_out) placed_out[sc] = placed;
            for (uint32_t c = 0; c < e->C; ++c) flips += fl[(size_t)sc * e->C + c];
        }
        if (int rc = check_launch_error(e)) return rc;
    }
    if (stats) {
        stats->jobs = J;
        stats->scenarios = n_scen;
        stats->rows = n_total;
        stats->runs = runs_walked;
        stats->fused = 7u;
        stats->flips = flips;
        stats->wall_us = us_between(t0);
    }
    return JSP_OK;
}

int jsp_place_whatif(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                     const uint32_t* scen_off, uint32_t n_scen, const uint32_t* rows, const uint64_t* labels,
                     const uint32_t* taints, const uint32_t* free_res, const int32_t* excl_owner, uint32_t flags,
                     int32_t* assign_out, uint32_t* placed_out, jsp_whatif_stats* stats) {
    if (int rc = check_engine(e)) return rc;
    return whatif_call(e, run_class, run_len, n_runs, scen_off, n_scen, rows, labels, taints, free_res, excl_owner,
                       flags, assign_out, placed_out, stats);
}

int jspb_place_whatif_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                           const uint32_t* scen_off, uint32_t n_scen, const uint32_t* rows, const uint64_t* labels,
                           const uint32_t* taints, const uint32_t* free_res, const int32_t* excl_owner,
                           int32_t* assign_out, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (int rc = check_timed(iters, 1000000, out_us)) return rc;
    return timed_calls(iters, out_us, [&](uint32_t) {
        return jsp_place_whatif(e, run_class, run_len, n_runs, scen_off, n_scen, rows, labels, taints, free_res,
                                excl_owner, 0, assign_out, nullptr, nullptr);
    });
}

// ---- preemptive placement (DESIGN.md §2 "Preemptive placement") ----
// One call's victim table and evict_free, checked and staged: the table sorted
// by id in pinned memory, evict_free ([R][N], when given) behind it, 16-byte
// aligned, and both copied to the device in one piece.
struct PreemptIn {
    uint32_t prio = 0, n_tab = 0;
    bool evict = false;
    size_t ef_off = 0;   // evict_free's byte offset in the staging
};

static int preempt_check(const char* call, uint32_t prio, const int32_t* owner_ids, const uint32_t* owner_prio,
                         uint32_t n_owners, std::vector<jsp::PreemptTabEntry>* tab) {
    if (prio > JSP_PREEMPT_MAX_PRIO) return set_err(JSP_EINVAL, "%s: prio %u exceeds %u", call, prio, JSP_PREEMPT_MAX_PRIO);
    if (n_owners > JSP_PREEMPT_MAX_OWNERS)
        return set_err(JSP_ERANGE, "%u owners in the table exceed the limit of %u per call", n_owners,
                       JSP_PREEMPT_MAX_OWNERS);
    if (n_owners > 0 && (!owner_ids || !owner_prio))
        return set_err(JSP_EINVAL, "%s: owner_ids or owner_prio is NULL (table index 0)", call);
    std::vector<std::pair<int32_t, uint32_t>> ix(n_owners);
    for (uint32_t i = 0; i < n_owners; ++i) {
        if (owner_ids[i] == -1) return set_err(JSP_EINVAL, "table index %u: owner id -1 names no owner", i);
        if (owner_prio[i] >= JSP_PREEMPT_MAX_PRIO)
            return set_err(JSP_EINVAL, "table index %u: rank %u is not below %u", i, owner_prio[i], JSP_PREEMPT_MAX_PRIO);
        ix[i] = {owner_ids[i], i};
    }
    std::sort(ix.begin(), ix.end());
    for (uint32_t i = 1; i < n_owners; ++i)
        if (ix[i].first == ix[i - 1].first)
            return set_err(JSP_EINVAL, "table index %u: owner id %d is in the table already (index %u)", ix[i].second,
                           ix[i].first, ix[i - 1].second);
    tab->resize(n_owners);
    for (uint32_t i = 0; i < n_owners; ++i) (*tab)[i] = jsp::PreemptTabEntry{ix[i].first, owner_prio[ix[i].second]};
    return JSP_OK;
}

static int preempt_stage(jsp_engine* e, uint32_t prio, const std::vector<jsp::PreemptTabEntry>& tab,
                         const uint32_t* evict_free, hipStream_t s, PreemptIn* in) {
    in->prio = prio;
    in->n_tab = (uint32_t)tab.size();
    in->evict = evict_free != nullptr;
    in->ef_off = (tab.size() * sizeof(jsp::PreemptTabEntry) + 15) & ~size_t(15);
    const size_t ef_bytes = in->evict ? (size_t)e->R * e->N * 4 : 0;
    const size_t bytes = in->ef_off + ef_bytes;
    const size_t n = std::max<uint32_t>(e->fit_n, 1);
    HIP_TRY(e->h_pre_in.reserve(bytes, grave(e)));
    HIP_TRY(e->pre_in.reserve(bytes, grave(e)));
    HIP_TRY(e->pre_code.reserve((size_t)e->npad * 4, grave(e)));
    HIP_TRY(e->pre_leaf.reserve((size_t)std::max<uint32_t>(e->L_total, 1) * 16, grave(e)));
    HIP_TRY(e->pre_out.reserve((3 * n + e->C + 1) * 4, grave(e)));
    HIP_TRY(e->h_pre_out.reserve((3 * n + e->C + 1) * 4, grave(e)));
    if (in->evict) {
        HIP_TRY(e->pre_free.reserve((size_t)e->R * e->npad * 4, grave(e)));
        HIP_TRY(e->pre_cap.reserve((size_t)e->C * std::max<uint32_t>(e->L_total, 1) * 4, grave(e)));
    }
    char* h = e->h_pre_in.as<char>();
    if (!tab.empty()) std::memcpy(h, tab.data(), tab.size() * sizeof(jsp::PreemptTabEntry));
    if (ef_bytes) std::memcpy(h + in->ef_off, evict_free, ef_bytes);
    if (bytes) HIP_TRY(hipMemcpyAsync(e->pre_in.p, h, bytes, hipMemcpyHostToDevice, s));
    return JSP_OK;
}

// lanes per leaf in the leaf pass: about 8 rows per lane of the mean leaf
static uint32_t preempt_leaf_shift(const jsp_engine* e) {
    const uint32_t mean = e->N / std::max<uint32_t>(e->L_total, 1);
    uint32_t shift = 0;
    while (shift < 6 && (8u << shift) < mean) shift += 1;
    return shift;
}

// cap' with evict_free: the tally once more over the merged free column, no
// occupancy count (the workgroup-block kernel, as every pass behind the
// tally's first), into pre_cap
static int preempt_tally(jsp_engine* e, hipStream_t s) {
    uint32_t* cap = e->pre_cap.as<uint32_t>();
    if (e->n_blocks == 0) {
        HIP_TRY(hipMemsetAsync(cap, 0, (size_t)e->C * e->L_total * 4, s));
        return JSP_OK;
    }
    jsp::TallyArgs a = tally_args(e, cap, nullptr, e->L_total);
    a.freer = e->pre_free.as<uint32_t>();
    a.do_occ = 0;
    for (uint32_t c0 = 0; c0 < e->C; c0 += a.nc) {
        a.c0 = c0;
        a.nc = std::min<uint32_t>(e->C - c0, jsp::kTallyClasses);
        HIP_TRY(jsp::launch_tally(a, s));
    }
    return JSP_OK;
}

// the launches behind the staging: row pass, leaf pass, cap', keys, order
static int preempt_order_step(jsp_engine* e, const PreemptIn& in, hipStream_t s) {
    const char* dev = e->pre_in.as<char>();
    jsp::PreemptRowArgs ra{};
    ra.excl = e->excl.as<int32_t>();
    ra.freer = e->freer.as<uint32_t>();
    ra.N = e->N;
    ra.npad = e->npad;
    ra.R = e->R;
    ra.tab = reinterpret_cast<const jsp::PreemptTabEntry*>(dev);
    ra.n_tab = in.n_tab;
    ra.prio = in.prio;
    ra.evict_free = in.evict ? reinterpret_cast<const uint32_t*>(dev + in.ef_off) : nullptr;
    ra.code = e->pre_code.as<uint32_t>();
    ra.free_out = in.evict ? e->pre_free.as<uint32_t>() : nullptr;
    HIP_TRY(jsp::launch_preempt_rows(ra, s));
    uint32_t* out = e->pre_out.as<uint32_t>();
    const size_t n = e->fit_n;
    uint32_t* nf = out + 3 * n;
    HIP_TRY(jsp::launch_preempt_leaves(ra.code, ra.excl, e->leaf_start.as<uint32_t>(), e->L_total, preempt_leaf_shift(e),
                                       e->pre_leaf.as<uint4>(), nf, e->C, s));
    if (in.evict) {
        if (int rc = preempt_tally(e, s)) return rc;
    } else if (int rc = tally_whole(e, s)) {
        return rc;
    }
    const jsp::FitRow* rows = e->fit_rows.as<jsp::FitRow>();
    HIP_TRY(jsp::launch_preempt_keys((in.evict ? e->pre_cap : e->cap).as<uint32_t>(), e->L_total, e->pre_leaf.as<uint4>(),
                                     e->leaf_start.as<uint32_t>(), e->cls.as<jsp::DevClass>(), e->topo, rows, e->C,
                                     e->fit_max_threads, e->fit_keys.as<uint64_t>(), out + n, out + 2 * n, nf, s));
    HIP_TRY(jsp::launch_fit_rank(e->fit_keys.as<uint64_t>(), rows, 0, e->fit_n_rank, e->fit_max_rank, nf, out, s));
    HIP_TRY(jsp::launch_fit_blocks(e->fit_keys.as<uint64_t>(), e->fit_sorted.as<uint64_t>(), rows, e->fit_n_rank,
                                   e->fit_n_block, e->fit_max_block, fit_block_keys(e), nf, out, s));
    return JSP_OK;
}

static int preempt_device_part(jsp_engine* e, const PreemptIn& in, hipStream_t s) {
    if (int rc = preempt_order_step(e, in, s)) return rc;
    HIP_TRY(jsp::launch_copy_u32(e->pre_out.as<uint32_t>(), e->h_pre_out.as<uint32_t>(), 3 * e->fit_n + e->C, s));
    return JSP_OK;
}

// the host's wait for a device part, by a tag behind its launches
static int preempt_wait(jsp_engine* e, hipStream_t s, bool gather) {
    StreamTag tag{};
    if (int rc = tag_post(e, s, &tag)) return rc;
    if (gather)
        return tag_wait(e, s, tag, {"preemptive placement: the victim list", "its", "preemptive placement: the gather",
                                    "preemptive placement: the gather"});
    return tag_wait(e, s, tag, {"preemptive placement: the order lists", "their", "preemptive placement: the device part",
                                "preemptive placement: the device part"});
}

// The argument checks, the engine stream behind every pending patch, the row
// and leaf passes, cap', keys and order lists into host-visible memory, the
// wait, the fit walk on the host (jsp_walk.cc walk_fit, no fit values), the
// prefix sum of seg over the placed jobs, and the gather of their victims.
// Nothing the placement paths read is written: no row, no service state, no
// lease (what-if's path).
static int preempt_call(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, uint32_t prio,
                        const int32_t* owner_ids, const uint32_t* owner_prio, uint32_t n_owners,
                        const uint32_t* evict_free, uint32_t flags, int32_t* assign_out, uint32_t* victim_off_out,
                        int32_t* victims_out, uint32_t victims_cap, jsp_preempt_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jsp_place_preempt", g)) return rc;
    if (flags != 0) return set_err(JSP_EINVAL, "jsp_place_preempt: flags %u must be 0", flags);
    if (n_runs > 0 && (!run_class || !run_len))
        return set_err(JSP_EINVAL, "jsp_place_preempt: run buffers are NULL (run 0)");
    uint64_t J64 = 0;
    uint32_t runs_walked = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        if (run_class[r] >= e->C)
            return set_err(JSP_EINVAL, "run %u: class %u out of range (%u classes)", r, run_class[r], e->C);
        J64 += run_len[r];
        runs_walked += run_len[r] != 0;
    }
    if (J64 > JSP_PREEMPT_MAX_JOBS)
        return set_err(JSP_ERANGE, "%llu jobs in the runs exceed the limit of %u per call", (unsigned long long)J64,
                       JSP_PREEMPT_MAX_JOBS);
    const uint32_t J = (uint32_t)J64;
    std::vector<jsp::PreemptTabEntry> tab;
    if (int rc = preempt_check("jsp_place_preempt", prio, owner_ids, owner_prio, n_owners, &tab)) return rc;
    if (J > 0 && !assign_out) return set_err(JSP_EINVAL, "jsp_place_preempt: assign_out is NULL (run 0)");
    uint32_t placed = 0, preempting = 0;
    uint64_t total = 0;
    if (victim_off_out) victim_off_out[0] = 0;
    if (J > 0) {
        hipStream_t s = nullptr;
        if (int rc = enter_engine_stream(e, false, &s)) return rc;
        HIP_TRY(e->hw_feas.reserve((size_t)std::max<uint32_t>(e->feas_words, 1) * 8 + 64, grave(e)));  // the tag word
        if (int rc = fit_rows(e, 0, s)) return rc;
        PreemptIn in;
        if (int rc = preempt_stage(e, prio, tab, evict_free, s, &in)) return rc;
        if (int rc = preempt_device_part(e, in, s)) return rc;
        if (int rc = preempt_wait(e, s, false)) return rc;
        const uint32_t* out = e->h_pre_out.as<uint32_t>();
        const size_t n = e->fit_n;
        placed = e->walk.walk_fit(out, out + 3 * n, e->fit_off_h.data(), nullptr, run_class, run_len, n_runs, assign_out,
                                  nullptr);
        if (int rc = check_launch_error(e)) return rc;
        // the placed jobs' records: domain, first victim, end of its victims
        HIP_TRY(e->h_pre_jobs.reserve((size_t)std::max<uint32_t>(placed, 1) * sizeof(jsp::PreemptJob), grave(e)));
        jsp::PreemptJob* jobs = e->h_pre_jobs.as<jsp::PreemptJob>();
        const uint32_t* seg = out + 2 * n;
        uint32_t np = 0;
        size_t j = 0;
        for (uint32_t r = 0; r < n_runs; ++r) {
            const uint32_t c = run_class[r], lvl = e->cls_h[c].level, off = e->fit_off_h[c];
            for (uint32_t i = 0; i < run_len[r]; ++i, ++j) {
                if (assign_out[j] >= 0) {
                    const uint32_t d = (uint32_t)assign_out[j], sg = seg[off + d];
                    jobs[np++] = jsp::PreemptJob{lvl, d, (uint32_t)total, (uint32_t)(total + sg)};
                    total += sg;
                    preempting += sg != 0;
                }
                if (victim_off_out) victim_off_out[j + 1] = (uint32_t)total;
            }
        }
        if (victims_out && total > victims_cap)
            return set_err(JSP_ERANGE, "%llu victims exceed victims_cap %u", (unsigned long long)total, victims_cap);
        if (victims_out && total > 0) {
            HIP_TRY(e->h_pre_vic.reserve((size_t)total * 4, grave(e)));
            HIP_TRY(jsp::launch_preempt_gather(jobs, np, e->excl.as<int32_t>(), e->leaf_start.as<uint32_t>(), e->topo,
                                               e->h_pre_vic.as<int32_t>(), s));
            if (int rc = preempt_wait(e, s, true)) return rc;
            std::memcpy(victims_out, e->h_pre_vic.p, (size_t)total * 4);
            if (int rc = check_launch_error(e)) return rc;
        }
    }
    if (stats) {
        stats->jobs = J;
        stats->placed = placed;
        stats->preempting = preempting;
        stats->victims = (uint32_t)total;
        stats->runs = runs_walked;
        stats->fused = 7u;
        stats->wall_us = us_between(t0);
    }
    return JSP_OK;
}

int jsp_place_preempt(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, uint32_t prio,
                      const int32_t* owner_ids, const uint32_t* owner_prio, uint32_t n_owners, const uint32_t* evict_free,
                      uint32_t flags, int32_t* assign_out, uint32_t* victim_off_out, int32_t* victims_out,
                      uint32_t victims_cap, jsp_preempt_stats* stats) {
    if (int rc = check_engine(e)) return rc;
    return preempt_call(e, run_class, run_len, n_runs, prio, owner_ids, owner_prio, n_owners, evict_free, flags,
                        assign_out, victim_off_out, victims_out, victims_cap, stats);
}

int jspb_place_preempt_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                            uint32_t prio, const int32_t* owner_ids, const uint32_t* owner_prio, uint32_t n_owners,
                            const uint32_t* evict_free, int32_t* assign_out, uint32_t* victim_off_out, int32_t* victims_out,
                            uint32_t victims_cap, jsp_preempt_stats* stats, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (int rc = check_timed(iters, 1000000, out_us)) return rc;
    return timed_calls(iters, out_us, [&](uint32_t) {
        return jsp_place_preempt(e, run_class, run_len, n_runs, prio, owner_ids, owner_prio, n_owners, evict_free, 0,
                                 assign_out, victim_off_out, victims_out, victims_cap, stats);
    });
}

int jspb_preempt_order(jsp_engine* e, uint32_t prio, const int32_t* owner_ids, const uint32_t* owner_prio,
                       uint32_t n_owners, const uint32_t* evict_free, int form, uint32_t* order_out, uint32_t n_order,
                       uint32_t* nf_out, uint32_t* key_out, uint32_t* seg_out, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jspb_preempt_order", g)) return rc;
    if (form < 0 || form > 2) return set_err(JSP_EINVAL, "form %d out of range [0,2]", form);
    std::vector<jsp::PreemptTabEntry> tab;
    if (int rc = preempt_check("jspb_preempt_order", prio, owner_ids, owner_prio, n_owners, &tab)) return rc;
    uint64_t total = 0;
    for (uint32_t c = 0; c < e->C; ++c) total += e->D[e->cls_h[c].level];
    if (n_order != total)
        return set_err(JSP_EINVAL, "n_order %u is not the %llu entries of the classes' segments", n_order,
                       (unsigned long long)total);
    if ((n_order > 0 && (!order_out || !key_out || !seg_out)) || !nf_out)
        return set_err(JSP_EINVAL, "order_out, key_out, seg_out or nf_out is NULL");
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    HIP_TRY(e->hw_feas.reserve((size_t)std::max<uint32_t>(e->feas_words, 1) * 8 + 64, grave(e)));
    if (int rc = fit_rows(e, form, s)) return rc;
    PreemptIn in;
    if (int rc = preempt_stage(e, prio, tab, evict_free, s, &in)) return rc;
    // a canary behind the output's last word: the copy and the kernels write inside it only
    uint32_t* out = e->h_pre_out.as<uint32_t>();
    const size_t n = e->fit_n, n_out = 3 * n + e->C;
    HIP_TRY(hipMemsetAsync(e->pre_out.p, 0xA5, (n_out + 1) * 4, s));
    out[n_out] = 0xC0FFEE00u;
    if (int rc = preempt_device_part(e, in, s)) return rc;
    if (int rc = preempt_wait(e, s, false)) return rc;
    if (out[n_out] != 0xC0FFEE00u) return set_err(JSP_EHIP, "preempt order: a word was written past the output");
    std::memcpy(order_out, out, (size_t)n_order * 4);
    std::memcpy(key_out, out + n, (size_t)n_order * 4);
    std::memcpy(seg_out, out + 2 * n, (size_t)n_order * 4);
    std::memcpy(nf_out, out + 3 * n, (size_t)e->C * 4);
    if (iters > 0 && n_order > 0) {
        if (int rc = time_steps(e, iters, nullptr, 0, out_us, [&](hipStream_t st) { return preempt_order_step(e, in, st); }))
            return rc;
    }
    return check_launch_error(e);
}

// ---- spread placement (DESIGN.md §2 "Spread placement") ----
// One call's peer table, checked and sorted, and its span-count rows, staged:
// {peer ids [n_tab]} then, 16-byte aligned, one SpanRow per class whose level
// is not above the spread level, the thread form's first (gang_rows' split).
struct SpreadIn {
    uint32_t s = 0, Ds = 0, n_tab = 0;
    uint32_t n_thread = 0, n_wave = 0, max_thread = 0, max_wave = 0;
    uint32_t leaf_shift = 0, peer_shift = 0;
    size_t rows_off = 0;   // the rows' byte offset in the staging
    // the pinned copy's words: feasibility, fits, the two count tables, peers
    size_t w_fits = 0, w_cf = 0, w_ce = 0, w_peers = 0, w_end = 0;
};

static int spread_check_peers(const char* call, const int32_t* peer_ids, uint32_t n_peers, std::vector<int32_t>* tab) {
    if (n_peers > JSP_SPREAD_MAX_PEERS)
        return set_err(JSP_ERANGE, "%u peers in the table exceed the limit of %u per call", n_peers, JSP_SPREAD_MAX_PEERS);
    if (n_peers > 0 && !peer_ids) return set_err(JSP_EINVAL, "%s: peer_ids is NULL (table index 0)", call);
    std::vector<std::pair<int32_t, uint32_t>> ix(n_peers);
    for (uint32_t i = 0; i < n_peers; ++i) {
        if (peer_ids[i] == -1) return set_err(JSP_EINVAL, "table index %u: owner id -1 names no owner", i);
        ix[i] = {peer_ids[i], i};
    }
    std::sort(ix.begin(), ix.end());
    for (uint32_t i = 1; i < n_peers; ++i)
        if (ix[i].first == ix[i - 1].first)
            return set_err(JSP_EINVAL, "table index %u: owner id %d is in the table already (index %u)", ix[i].second,
                           ix[i].first, ix[i - 1].second);
    tab->resize(n_peers);
    for (uint32_t i = 0; i < n_peers; ++i) (*tab)[i] = ix[i].first;
    return JSP_OK;
}

// form 0: each class's span-count form by its mean segment (kSpanWaveDomains);
// 1 / 2: every class in the thread / the wave form. shift < 0: about 8 rows
// per lane of the mean leaf (preempt_leaf_shift).
static int spread_stage(jsp_engine* e, uint32_t lvl, const std::vector<int32_t>& tab, int form, int shift, hipStream_t s,
                        SpreadIn* in) {
    in->s = lvl;
    in->Ds = e->D[lvl];
    in->n_tab = (uint32_t)tab.size();
    std::vector<jsp::SpanRow> th, wv;
    uint32_t woff = 0;
    for (uint32_t c = 0; c < e->C; ++c) {
        const uint32_t lc = e->cls_h[c].level;
        if (lc >= lvl) {
            jsp::SpanRow r{};
            r.word0 = woff;
            r.s = lvl;
            r.lc = lc;
            r.D = in->Ds;
            r.cnt_off = c * in->Ds;
            const bool wave = form == 2 || (form == 0 && e->D[lc] > jsp::kSpanWaveDomains * std::max<uint32_t>(in->Ds, 1));
            (wave ? wv : th).push_back(r);
        }
        woff += (e->D[lc] + 63) / 64;
    }
    in->n_thread = (uint32_t)th.size();
    in->n_wave = (uint32_t)wv.size();
    in->max_thread = th.empty() ? 0u : in->Ds;
    in->max_wave = wv.empty() ? 0u : in->Ds;
    th.insert(th.end(), wv.begin(), wv.end());
    in->leaf_shift = shift < 0 ? preempt_leaf_shift(e) : (uint32_t)shift;
    const uint32_t mean = lvl + 1 < e->K ? e->L_total / std::max<uint32_t>(in->Ds, 1) : 1u;
    in->peer_shift = 0;
    while (in->peer_shift < 6 && (8u << in->peer_shift) < mean) in->peer_shift += 1;
    in->rows_off = (tab.size() * 4 + 15) & ~size_t(15);
    const size_t bytes = in->rows_off + th.size() * sizeof(jsp::SpanRow);
    const size_t fw2 = 2 * (size_t)e->feas_words, cd = (size_t)e->C * in->Ds;
    in->w_fits = fw2;
    in->w_cf = 2 * fw2;
    in->w_ce = in->w_cf + cd;
    in->w_peers = in->w_ce + cd;
    in->w_end = in->w_peers + in->Ds;
    HIP_TRY(e->h_sp_in.reserve(std::max<size_t>(bytes, 16), grave(e)));
    HIP_TRY(e->sp_in.reserve(std::max<size_t>(bytes, 16), grave(e)));
    HIP_TRY(e->sp_flag.reserve((size_t)std::max<uint32_t>(e->npad, 1) * 4, grave(e)));
    HIP_TRY(e->sp_leaf.reserve((size_t)std::max<uint32_t>(e->L_total, 1) * 8, grave(e)));
    HIP_TRY(e->sp_out.reserve((in->w_end - fw2 + 1) * 4, grave(e)));
    HIP_TRY(e->h_sp_out.reserve((in->w_end + 1) * 4, grave(e)));
    char* h = e->h_sp_in.as<char>();
    if (!tab.empty()) std::memcpy(h, tab.data(), tab.size() * 4);
    if (!th.empty()) std::memcpy(h + in->rows_off, th.data(), th.size() * sizeof(jsp::SpanRow));
    if (bytes) HIP_TRY(hipMemcpyAsync(e->sp_in.p, h, bytes, hipMemcpyHostToDevice, s));
    return JSP_OK;
}

// the launches behind the tally and the feasibility words: fits words, the
// peer row, leaf and per-S passes, the span counts of both kinds of words
static int spread_tables_step(jsp_engine* e, const SpreadIn& in, hipStream_t s) {
    const char* dev = e->sp_in.as<char>();
    uint32_t* out = e->sp_out.as<uint32_t>();   // {fits, cnt_feas, cnt_fits, peers}: the pinned copy's words from w_fits on
    uint64_t* fits = reinterpret_cast<uint64_t*>(out);
    uint32_t* cf = out + (in.w_cf - in.w_fits);
    uint32_t* ce = out + (in.w_ce - in.w_fits);
    uint32_t* peers = out + (in.w_peers - in.w_fits);
    HIP_TRY(jsp::launch_spread_fits(e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, e->cls.as<jsp::DevClass>(),
                                    e->C, e->word_off.as<uint32_t>(), e->feas_words, e->topo, fits, s));
    HIP_TRY(jsp::launch_spread_rows(e->excl.as<int32_t>(), e->npad, reinterpret_cast<const int32_t*>(dev), in.n_tab,
                                    e->sp_flag.as<uint32_t>(), s));
    HIP_TRY(jsp::launch_spread_leaves(e->sp_flag.as<uint32_t>(), e->excl.as<int32_t>(), e->leaf_start.as<uint32_t>(),
                                      e->L_total, in.leaf_shift, e->sp_leaf.as<uint2>(), s));
    HIP_TRY(jsp::launch_spread_peers(e->sp_leaf.as<uint2>(), e->leaf_start.as<uint32_t>(), e->L_total, e->topo, in.s,
                                     in.Ds, in.peer_shift, peers, s));
    // a class finer than the spread level has no row: its counts stay zero
    if (in.w_peers > in.w_cf) HIP_TRY(hipMemsetAsync(cf, 0, (in.w_peers - in.w_cf) * 4, s));
    const jsp::SpanRow* rows = reinterpret_cast<const jsp::SpanRow*>(dev + in.rows_off);
    const uint64_t* words[2] = {e->feas.as<uint64_t>(), fits};
    uint32_t* cnt[2] = {cf, ce};
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(jsp::launch_span_counts(words[i], e->topo, rows, 0, in.n_thread, in.max_thread, false, cnt[i], s));
        HIP_TRY(jsp::launch_span_counts(words[i], e->topo, rows, in.n_thread, in.n_wave, in.max_wave, true, cnt[i], s));
    }
    return JSP_OK;
}

// tally, feasibility words, the tables, and all of it into pinned memory
static int spread_device_part(jsp_engine* e, const SpreadIn& in, hipStream_t s) {
    if (int rc = tally_whole(e, s)) return rc;
    if (int rc = feas_launch(e, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, e->feas.as<uint64_t>(), s))
        return rc;
    if (int rc = spread_tables_step(e, in, s)) return rc;
    uint32_t* h = e->h_sp_out.as<uint32_t>();
    HIP_TRY(jsp::launch_copy_u32(e->feas.as<uint32_t>(), h, (uint32_t)in.w_fits, s));
    HIP_TRY(jsp::launch_copy_u32(e->sp_out.as<uint32_t>(), h + in.w_fits, (uint32_t)(in.w_end - in.w_fits), s));
    return JSP_OK;
}

// the host's wait for the device part, by a tag behind its launches
static int spread_wait(jsp_engine* e, hipStream_t s) {
    StreamTag tag{};
    if (int rc = tag_post(e, s, &tag)) return rc;
    return tag_wait(e, s, tag, {"spread placement: the tables", "their", "spread placement: the device part",
                                "spread placement: the device part"});
}

// The argument checks, the engine stream behind every pending patch, tally +
// feasibility + the tables into host-visible memory, the wait, the spread walk
// on the host (jsp_walk.cc walk_spread).
static int spread_call(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                       uint32_t spread_level, uint32_t max_skew, const int32_t* peer_ids, uint32_t n_peers, uint32_t flags,
                       int32_t* assign_out, int32_t* spread_out, uint32_t* count_out, jsp_spread_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jsp_place_spread", g)) return rc;
    if (flags != 0) return set_err(JSP_EINVAL, "jsp_place_spread: flags %u must be 0", flags);
    if (spread_level >= e->K)
        return set_err(JSP_EINVAL, "jsp_place_spread: spread level %u is no level below %u", spread_level, e->K);
    if (n_runs > 0 && (!run_class || !run_len)) return set_err(JSP_EINVAL, "jsp_place_spread: run buffers are NULL (run 0)");
    uint64_t J64 = 0;
    uint32_t runs_walked = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        if (run_class[r] >= e->C)
            return set_err(JSP_EINVAL, "run %u: class %u out of range (%u classes)", r, run_class[r], e->C);
        if (run_len[r] == 0) continue;
        if (e->cls_h[run_class[r]].level < spread_level)
            return set_err(JSP_EINVAL, "run %u: spread level %u is finer than level %u of class %u", r, spread_level,
                           e->cls_h[run_class[r]].level, run_class[r]);
        J64 += run_len[r];
        runs_walked += 1;
    }
    if (J64 > JSP_SPREAD_MAX_JOBS)
        return set_err(JSP_ERANGE, "%llu jobs in the runs exceed the limit of %u per call", (unsigned long long)J64,
                       JSP_SPREAD_MAX_JOBS);
    const uint32_t J = (uint32_t)J64;
    std::vector<int32_t> tab;
    if (int rc = spread_check_peers("jsp_place_spread", peer_ids, n_peers, &tab)) return rc;
    if (J > 0 && !assign_out) return set_err(JSP_EINVAL, "jsp_place_spread: assign_out is NULL (run 0)");
    uint32_t placed = 0, refused = 0, skew = 0;
    if (J > 0 || count_out) {
        hipStream_t s = nullptr;
        if (int rc = enter_engine_stream(e, false, &s)) return rc;
        HIP_TRY(e->hw_feas.reserve((size_t)std::max<uint32_t>(e->feas_words, 1) * 8 + 64, grave(e)));  // the tag word
        SpreadIn in;
        if (int rc = spread_stage(e, spread_level, tab, 0, -1, s, &in)) return rc;
        if (int rc = spread_device_part(e, in, s)) return rc;
        if (int rc = spread_wait(e, s)) return rc;
        const uint32_t* h = e->h_sp_out.as<uint32_t>();
        const auto tw = std::chrono::steady_clock::now();
        placed = e->walk.walk_spread(e->sp_state, reinterpret_cast<const uint64_t*>(h), h + in.w_cf, h + in.w_ce,
                                     h + in.w_peers, spread_level, max_skew, run_class, run_len, n_runs, assign_out,
                                     spread_out, count_out, &refused, &skew);
        e->sp_walk_us = us_between(tw);
        if (int rc = check_launch_error(e)) return rc;
    }
    if (stats) {
        stats->jobs = J;
        stats->placed = placed;
        stats->refused = refused;
        stats->skew = skew;
        stats->runs = runs_walked;
        stats->fused = 7u;
        stats->wall_us = us_between(t0);
    }
    return JSP_OK;
}

int jsp_place_spread(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                     uint32_t spread_level, uint32_t max_skew, const int32_t* peer_ids, uint32_t n_peers, uint32_t flags,
                     int32_t* assign_out, int32_t* spread_out, uint32_t* count_out, jsp_spread_stats* stats) {
    if (int rc = check_engine(e)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    jsp_spread_stats local{};
    jsp_spread_stats* st = stats ? stats : &local;
    const int rc = spread_call(e, run_class, run_len, n_runs, spread_level, max_skew, peer_ids, n_peers, flags, assign_out,
                               spread_out, count_out, st);
    return record_placement(e, us_between(t0), rc, st->jobs, st->placed);
}

int jspb_place_spread_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                           uint32_t spread_level, uint32_t max_skew, const int32_t* peer_ids, uint32_t n_peers,
                           int32_t* assign_out, int32_t* spread_out, uint32_t* count_out, jsp_spread_stats* stats,
                           uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (int rc = check_timed(iters, 1000000, out_us)) return rc;
    std::vector<double> walk_us(iters);
    const int rc = timed_calls(iters, out_us, [&](uint32_t i) {
        const int r = jsp_place_spread(e, run_class, run_len, n_runs, spread_level, max_skew, peer_ids, n_peers, 0,
                                       assign_out, spread_out, count_out, stats);
        walk_us[i] = e->sp_walk_us;
        return r;
    });
    if (rc) return rc;
    std::sort(walk_us.begin(), walk_us.end());
    out_us[3] = walk_us[iters / 2];
    return JSP_OK;
}

int jspb_spread_tables(jsp_engine* e, uint32_t spread_level, const int32_t* peer_ids, uint32_t n_peers, int form, int shift,
                       uint64_t* fits_out, uint64_t* feas_out, uint32_t n_words, uint32_t* peers_out,
                       uint32_t* cnt_feas_out, uint32_t* cnt_fits_out, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jspb_spread_tables", g)) return rc;
    if (form < 0 || form > 2) return set_err(JSP_EINVAL, "form %d out of range [0,2]", form);
    if (shift > 6) return set_err(JSP_EINVAL, "shift %d out of range [-1,6]", shift);
    if (spread_level >= e->K) return set_err(JSP_EINVAL, "spread level %u is no level below %u", spread_level, e->K);
    std::vector<int32_t> tab;
    if (int rc = spread_check_peers("jspb_spread_tables", peer_ids, n_peers, &tab)) return rc;
    if (n_words != e->feas_words)
        return set_err(JSP_EINVAL, "n_words %u is not the %u words of the classes", n_words, e->feas_words);
    if ((n_words > 0 && !fits_out) || (e->D[spread_level] > 0 && !peers_out))
        return set_err(JSP_EINVAL, "fits_out or peers_out is NULL");
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    HIP_TRY(e->hw_feas.reserve((size_t)std::max<uint32_t>(e->feas_words, 1) * 8 + 64, grave(e)));
    SpreadIn in;
    if (int rc = spread_stage(e, spread_level, tab, form, shift, s, &in)) return rc;
    // a canary behind the output's last word: the copy and the kernels write inside it only
    uint32_t* h = e->h_sp_out.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(e->sp_out.p, 0xA5, (in.w_end - in.w_fits + 1) * 4, s));
    h[in.w_end] = 0xC0FFEE00u;
    if (int rc = spread_device_part(e, in, s)) return rc;
    if (int rc = spread_wait(e, s)) return rc;
    if (h[in.w_end] != 0xC0FFEE00u) return set_err(JSP_EHIP, "spread tables: a word was written past the output");
    const size_t cd = (size_t)e->C * in.Ds;
    if (n_words) std::memcpy(fits_out, h + in.w_fits, (size_t)n_words * 8);
    if (n_words && feas_out) std::memcpy(feas_out, h, (size_t)n_words * 8);
    if (in.Ds) std::memcpy(peers_out, h + in.w_peers, (size_t)in.Ds * 4);
    if (cd && cnt_feas_out) std::memcpy(cnt_feas_out, h + in.w_cf, cd * 4);
    if (cd && cnt_fits_out) std::memcpy(cnt_fits_out, h + in.w_ce, cd * 4);
    if (iters > 0) {
        if (int rc = time_steps(e, iters, nullptr, 0, out_us, [&](hipStream_t st) { return spread_tables_step(e, in, st); }))
            return rc;
    }
    return check_launch_error(e);
}

// ---- pod binding (DESIGN.md §2 "Pod binding") ----
// jsp_bind_pods' front end, which jsp_assume shares. bind_stage: the assignment
// validated and one record per job in the pinned input staging {records [J],
// assign [J], order [J], `extra` more words per job}, the placed jobs sorted
// into the wave form's (order[0, n_wave)) and the workgroup form's (up to
// n_launch). bind_front, on the engine stream: the claim tables filled, the
// input copied to the device above kBindInPlaceMax jobs, the claim launch.
struct BindStage {
    jsp::BindJob* jobs;
    int32_t* assign;
    uint32_t* order;
    uint32_t n_wave, n_launch;
};

static int bind_stage(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                      const int32_t* assign, uint32_t J, uint32_t extra, uint64_t* pod_off_out, BindStage* st) {
    // from here on the staging of the last call is rewritten or replaced
    e->bd_last.J = 0;
    HIP_TRY(e->h_bd_in.reserve((size_t)J * (sizeof(jsp::BindJob) + 8 + 4 * (size_t)extra), grave(e)));
    jsp::BindJob* h_jobs = e->h_bd_in.as<jsp::BindJob>();
    int32_t* h_assign = reinterpret_cast<int32_t*>(h_jobs + J);
    uint32_t* h_order = reinterpret_cast<uint32_t*>(h_assign + J);
    uint32_t n_wave = 0, n_launch = 0;
    uint32_t j = 0, pod_off = 0;
    for (uint32_t i = 0; i < n_runs; ++i) {
        const uint32_t c = run_class[i], lvl = e->cls_h[c].level, Dl = e->D[lvl], pods = e->cls_h[c].pods;
        for (uint32_t q = 0; q < run_len[i]; ++q, ++j) {
            const int32_t d = assign[j];
            if (d < -1 || (d >= 0 && (uint32_t)d >= Dl))
                return set_err(JSP_EINVAL, "job %u: domain %d out of range [-1,%u) at level %u", j, d, Dl, lvl);
            jsp::BindJob& r = h_jobs[j];
            r.row0 = r.row1 = 0;
            r.cls = c | (d < 0 ? jsp::kBindUnplaced : 0u);
            r.pod_off = pod_off;
            if (d >= 0) {
                const uint32_t l0 = e->h_fl[lvl][(uint32_t)d], l1 = e->h_fl[lvl][(uint32_t)d + 1];
                r.row0 = e->h_ls[l0];
                r.row1 = e->h_ls[l1];
                // no leaves: the domain intersects no other (and is stale: it has no rows)
                if (l0 == l1) r.cls |= jsp::kBindNoClaim;
            }
            h_assign[j] = d;
            if (pod_off_out) pod_off_out[j] = pod_off;
            pod_off += pods;
            if (d >= 0 && !e->hooks.bind_wg && r.row1 - (r.row0 & ~3u) <= jsp::kBindWaveRows)
                h_order[n_wave++] = j;
        }
    }
    if (pod_off_out) pod_off_out[J] = pod_off;
    n_launch = n_wave;  // the workgroup form's jobs behind the wave form's; unplaced jobs are not launched
    for (j = 0; j < J; ++j)
        if ((h_jobs[j].cls & jsp::kBindUnplaced) == 0u &&
            (e->hooks.bind_wg || h_jobs[j].row1 - (h_jobs[j].row0 & ~3u) > jsp::kBindWaveRows))
            h_order[n_launch++] = j;
    *st = BindStage{h_jobs, h_assign, h_order, n_wave, n_launch};
    return JSP_OK;
}

static int bind_front(jsp_engine* e, const BindStage& st, uint32_t J, uint32_t extra, jsp::BindArgs* out) {
    hipStream_t s = e->stream;
    const uint32_t DT = std::max<uint32_t>(jsp::sticky_dom_off(e->D, e->K), 1);
    HIP_TRY(e->bd_tab.reserve((size_t)2 * DT * 4, grave(e)));
    HIP_TRY(hipMemsetAsync(e->bd_tab.p, 0xFF, (size_t)2 * DT * 4, s));
    jsp::BindArgs b{};
    b.jobs = st.jobs;
    b.assign = st.assign;
    b.order = st.order;
    if (J > jsp::kBindInPlaceMax) {
        // every wave starts with a chain of dependent reads of its job's input
        // (order -> record -> assign): over the host link that chain bounds a
        // launch of many small jobs, so a large batch is copied over first
        const size_t in_bytes = (size_t)J * (sizeof(jsp::BindJob) + 8 + 4 * (size_t)extra);
        HIP_TRY(e->bd_in.reserve(in_bytes, grave(e)));
        HIP_TRY(hipMemcpyAsync(e->bd_in.p, e->h_bd_in.p, in_bytes, hipMemcpyHostToDevice, s));
        b.jobs = e->bd_in.as<jsp::BindJob>();
        b.assign = reinterpret_cast<const int32_t*>(b.jobs + J);
        b.order = reinterpret_cast<const uint32_t*>(b.assign + J);
    }
    b.J = J;
    b.topo = e->topo;
    b.own = e->bd_tab.as<uint32_t>();
    b.sub = b.own + DT;
    HIP_TRY(jsp::launch_bind_claim(b, e->cls.as<jsp::DevClass>(), s));
    *out = b;
    return JSP_OK;
}

// The jobs' results, read once the stream finished: the first placed job whose
// domain intersects an earlier job's refuses the whole call.
static int bind_conflict(const BindStage& st, const jsp::BindJobOut* job_out, uint32_t J) {
    for (uint32_t j = 0; j < J; ++j)
        if ((st.jobs[j].cls & jsp::kBindUnplaced) == 0u && job_out[j].state == jsp::kBindConflict)
            return set_err(JSP_EINVAL, "job %u: its domain %d intersects the domain of an earlier job", j, st.assign[j]);
    return JSP_OK;
}

// The host validates the assignment, lays the pods out (pod_off) and prepares
// one record per job -- its domain's rows from the host copies of first_leaf
// and leaf_start -- in pinned memory the kernels read in place, sorted into
// the wave form's jobs and the workgroup form's. On the engine stream: the
// claim tables filled (one memset of 8 bytes per domain of all levels; the
// tables are not kept at rest, so a call that fails leaves nothing to repair),
// the claim launch, one bind launch per form in use. The kernels write the
// pods' rows and the per-job results to pinned memory, so no copy follows: the
// host waits for the stream, sums the jobs' results and copies the rows out.
static int bind_call(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                     const int32_t* assign, uint32_t flags, int32_t* pod_row_out, uint64_t* pod_off_out,
                     jsp_bind_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jsp_bind_pods", g)) return rc;
    if (flags != 0) return set_err(JSP_EINVAL, "flags %u: must be 0", flags);
    uint32_t J = 0;
    if (int rc = run_front(e, run_class, run_len, n_runs, &J)) return rc;
    if (J > 0 && (!assign || !pod_row_out)) return set_err(JSP_EINVAL, "assign or pod_row_out is NULL");
    uint64_t P = 0;
    for (uint32_t i = 0; i < n_runs; ++i) P += (uint64_t)run_len[i] * e->cls_h[run_class[i]].pods;
    if (P > JSP_BIND_MAX_PODS)
        return set_err(JSP_ERANGE, "%llu pods exceed the engine limit of %u per call", (unsigned long long)P,
                       (unsigned)JSP_BIND_MAX_PODS);
    if (J == 0) {
        if (pod_off_out) pod_off_out[0] = 0;
        if (stats) {
            *stats = jsp_bind_stats{};
            stats->wall_us = us_between(t0);
        }
        return JSP_OK;
    }
    BindStage st{};
    if (int rc = bind_stage(e, run_class, run_len, n_runs, assign, J, 0, pod_off_out, &st)) return rc;
    HIP_TRY(e->h_bd_out.reserve((size_t)J * sizeof(jsp::BindJobOut) + (size_t)std::max<uint64_t>(P, 1) * 4, grave(e)));
    const jsp::BindJob* h_jobs = st.jobs;
    const uint32_t n_wave = st.n_wave, n_launch = st.n_launch;
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    jsp::BindArgs b{};
    if (int rc = bind_front(e, st, J, 0, &b)) return rc;
    b.job_out = e->h_bd_out.as<jsp::BindJobOut>();
    b.pod_row = reinterpret_cast<int32_t*>(b.job_out + J);
    const jsp::TallyArgs a = tally_args(e, nullptr, nullptr, e->L_total);
    HIP_TRY(jsp::launch_bind(a, b, 0, n_wave, false, s));
    HIP_TRY(jsp::launch_bind(a, b, n_wave, n_launch - n_wave, true, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = check_launch_error(e)) return rc;
    uint32_t bound = 0, stale = 0, rows_used = 0;
    uint64_t pods_bound = 0;
    // the kernels wrote the bound jobs' pods only: a conflict first (nothing is
    // copied out then), then the rows of the bound jobs and -1 for the others
    if (int rc = bind_conflict(st, b.job_out, J)) return rc;
    std::memcpy(pod_row_out, b.pod_row, (size_t)P * 4);
    for (uint32_t j = 0; j < J; ++j) {
        const uint32_t cw = h_jobs[j].cls, pods = e->cls_h[cw & jsp::kBindClassMask].pods;
        const uint32_t state = (cw & jsp::kBindUnplaced) != 0u ? 0u : b.job_out[j].state;
        if (state == jsp::kBindBound) {
            ++bound;
            rows_used += b.job_out[j].rows_used;
            pods_bound += pods;
        } else {
            stale += state == jsp::kBindStale ? 1u : 0u;
            int32_t* dst = pod_row_out + h_jobs[j].pod_off;
            std::fill(dst, dst + pods, -1);
        }
    }
    e->bd_last = b;
    e->bd_last_wave = n_wave;
    e->bd_last_n = n_launch;
    if (stats) {
        stats->jobs = J;
        stats->bound = bound;
        stats->stale = stale;
        stats->rows_used = rows_used;
        stats->pods = P;
        stats->pods_bound = pods_bound;
        stats->wall_us = us_between(t0);
    }
    return JSP_OK;
}

int jsp_bind_pods(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                  const int32_t* assign, uint32_t flags, int32_t* pod_row_out, uint64_t* pod_off_out,
                  jsp_bind_stats* stats) {
    if (int rc = check_engine(e)) return rc;
    return bind_call(e, run_class, run_len, n_runs, assign, flags, pod_row_out, pod_off_out, stats);
}

int jspb_bind_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                   const int32_t* assign, int32_t* pod_row_out, jsp_bind_stats* stats, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (int rc = check_timed(iters, 1000000, out_us)) return rc;
    return timed_calls(iters, out_us, [&](uint32_t) {
        return jsp_bind_pods(e, run_class, run_len, n_runs, assign, 0, pod_row_out, nullptr, stats);
    });
}

// ---- assume and forget (DESIGN.md §2 "Assume and forget") ----
// jsp_assume: jsp_bind_pods' front end with the owners behind the order in the
// input staging, then on the engine stream the decide launches and behind
// them the mark launches, which read the conflict word the decide launches
// raise -- no host round trip in between, and nothing written after a refusal.
// Both calls write rows: the resident service's previous request is settled
// first (no tile may still be reading them), and its tiles reload afterwards
// (rows_dirty); the service itself stays up.
static int assume_call(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                       const int32_t* assign, const int32_t* owner, uint32_t flags, uint8_t* committed_out,
                       jsp_assume_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jsp_assume", g)) return rc;
    if (flags != 0) return set_err(JSP_EINVAL, "flags %u: must be 0", flags);
    uint32_t J = 0;
    if (int rc = run_front(e, run_class, run_len, n_runs, &J)) return rc;
    if (J > 0 && (!assign || !owner)) return set_err(JSP_EINVAL, "assign or owner is NULL");
    for (uint32_t j = 0; j < J; ++j)
        if (assign[j] >= 0 && owner[j] == -1)
            return set_err(JSP_EINVAL, "job %u: owner -1 marks a free row and cannot own a domain", j);
    BindStage st{};
    if (J > 0)
        if (int rc = bind_stage(e, run_class, run_len, n_runs, assign, J, 1, nullptr, &st)) return rc;
    if (st.n_launch == 0) {  // no job, or none placed: nothing to decide
        if (committed_out && J > 0) std::memset(committed_out, 0, J);
        if (stats) {
            *stats = jsp_assume_stats{};
            stats->jobs = J;
            stats->wall_us = us_between(t0);
        }
        return JSP_OK;
    }
    int32_t* h_owner = reinterpret_cast<int32_t*>(st.order + J);
    std::memcpy(h_owner, owner, (size_t)J * 4);
    uint32_t max_rows = 0;
    for (uint32_t i = st.n_wave; i < st.n_launch; ++i)
        max_rows = std::max(max_rows, st.jobs[st.order[i]].row1 - st.jobs[st.order[i]].row0);
    HIP_TRY(e->h_bd_out.reserve((size_t)J * sizeof(jsp::BindJobOut), grave(e)));
    HIP_TRY(e->as_state.reserve((size_t)(J + 1) * 4, grave(e)));
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, true, &s)) return rc;  // the mark launches write excl_owner
    jsp::BindArgs b{};
    if (int rc = bind_front(e, st, J, 1, &b)) return rc;
    b.job_out = e->h_bd_out.as<jsp::BindJobOut>();
    jsp::AssumeArgs m{};
    m.owner = reinterpret_cast<const int32_t*>(b.order + J);
    m.excl = e->excl.as<int32_t>();
    m.n_rows = e->N;
    m.state = e->as_state.as<uint32_t>();
    m.conflict = m.state + J;
    HIP_TRY(hipMemsetAsync(m.conflict, 0, 4, s));
    const jsp::TallyArgs a = tally_args(e, nullptr, nullptr, e->L_total);
    const uint32_t n_wave = st.n_wave, n_wg = st.n_launch - st.n_wave;
    HIP_TRY(jsp::launch_assume_decide(a, b, m, 0, n_wave, false, s));
    HIP_TRY(jsp::launch_assume_decide(a, b, m, n_wave, n_wg, true, s));
    // a large domain's fill is spread over several workgroups (2048 rows each, at most 256)
    const uint32_t split = std::min<uint32_t>(std::max<uint32_t>((max_rows + 2047u) / 2048u, 1u), 256u);
    HIP_TRY(jsp::launch_assume_mark(b, m, 0, n_wave, false, 1, s));
    HIP_TRY(jsp::launch_assume_mark(b, m, n_wave, n_wg, true, split, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = check_launch_error(e)) return rc;
    if (int rc = bind_conflict(st, b.job_out, J)) return rc;
    uint32_t committed = 0, stale = 0;
    uint64_t rows_marked = 0;
    for (uint32_t j = 0; j < J; ++j) {
        const uint32_t state = (st.jobs[j].cls & jsp::kBindUnplaced) != 0u ? 0u : b.job_out[j].state;
        if (state == jsp::kBindBound) {
            ++committed;
            rows_marked += std::min(st.jobs[j].row1, e->N) - std::min(st.jobs[j].row0, e->N);
        }
        stale += state == jsp::kBindStale ? 1u : 0u;
        if (committed_out) committed_out[j] = state == jsp::kBindBound ? 1 : 0;
    }
    if (committed > 0) e->svc.rows_dirty = true;  // the resident tiles' on-chip row copies are stale
    if (stats) {
        stats->jobs = J;
        stats->committed = committed;
        stats->stale = stale;
        stats->reserved = 0;
        stats->rows_marked = rows_marked;
        stats->wall_us = us_between(t0);
    }
    return JSP_OK;
}

int jsp_assume(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
               const int32_t* assign, const int32_t* owner, uint32_t flags, uint8_t* committed_out,
               jsp_assume_stats* stats) {
    if (int rc = check_engine(e)) return rc;
    return assume_call(e, run_class, run_len, n_runs, assign, owner, flags, committed_out, stats);
}

int jsp_forget(jsp_engine* e, const int32_t* owners, uint32_t n_owners, uint64_t* rows_cleared_out) {
    if (int rc = check_engine(e)) return rc;
    std::unique_lock<std::mutex> g;
    if (int rc = single_engine(e, "jsp_forget", g)) return rc;
    if (n_owners > 0 && !owners) return set_err(JSP_EINVAL, "owners is NULL");
    if (n_owners > JSP_FORGET_MAX_OWNERS)
        return set_err(JSP_ERANGE, "%u owners exceed the limit of %u per call", n_owners, (unsigned)JSP_FORGET_MAX_OWNERS);
    for (uint32_t i = 0; i < n_owners; ++i)
        if (owners[i] == -1) return set_err(JSP_EINVAL, "owners[%u] is -1: a free row has no owner to forget", i);
    if (rows_cleared_out) *rows_cleared_out = 0;
    if (n_owners == 0) return JSP_OK;
    const uint32_t grid = jsp::explain_rows_grid(e->N, e->n_cu);
    HIP_TRY(e->h_fg_own.reserve((size_t)n_owners * 4, grave(e)));
    HIP_TRY(e->h_fg_parts.reserve((size_t)grid * 4, grave(e)));
    HIP_TRY(e->fg_own.reserve((size_t)n_owners * 4, grave(e)));
    int32_t* h_own = e->h_fg_own.as<int32_t>();
    std::memcpy(h_own, owners, (size_t)n_owners * 4);
    if (!std::is_sorted(h_own, h_own + n_owners)) std::sort(h_own, h_own + n_owners);  // (a ledger's list often is)
    const uint32_t n = (uint32_t)(std::unique(h_own, h_own + n_owners) - h_own);
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, true, &s)) return rc;  // the launch clears excl_owner
    HIP_TRY(hipMemcpyAsync(e->fg_own.p, h_own, (size_t)n * 4, hipMemcpyHostToDevice, s));
    uint32_t* parts = e->h_fg_parts.as<uint32_t>();
    HIP_TRY(jsp::launch_forget(e->excl.as<int32_t>(), e->N, e->fg_own.as<int32_t>(), n, grid, parts, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = check_launch_error(e)) return rc;
    uint64_t cleared = 0;
    for (uint32_t i = 0; i < grid; ++i) cleared += parts[i];
    if (cleared > 0) e->svc.rows_dirty = true;  // the resident tiles' on-chip row copies are stale
    if (rows_cleared_out) *rows_cleared_out = cleared;
    return JSP_OK;
}

int jspb_assume_forget_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                            const int32_t* assign, const int32_t* owner, uint32_t iters, jsp_assume_stats* stats,
                            uint64_t* rows_cleared_out, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (int rc = check_timed(iters, 1000000, out_us)) return rc;
    if (n_runs > 0 && !run_len) return set_err(JSP_EINVAL, "run buffers are NULL");
    uint64_t J = 0;
    for (uint32_t i = 0; i < n_runs; ++i) J += run_len[i];
    if (J > JSP_FORGET_MAX_OWNERS)
        return set_err(JSP_ERANGE, "%llu jobs exceed jsp_forget's %u owners", (unsigned long long)J,
                       (unsigned)JSP_FORGET_MAX_OWNERS);
    if (J > 0 && (!assign || !owner)) return set_err(JSP_EINVAL, "assign or owner is NULL");
    std::vector<int32_t> owned;
    for (uint64_t j = 0; j < J; ++j)
        if (assign[j] >= 0) owned.push_back(owner[j]);
    std::vector<int64_t> ua(iters), uf(iters);
    for (uint32_t i = 0; i < iters; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = jsp_assume(e, run_class, run_len, n_runs, assign, owner, 0, nullptr, stats)) return rc;
        const auto t1 = std::chrono::steady_clock::now();
        if (int rc = jsp_forget(e, owned.data(), (uint32_t)owned.size(), rows_cleared_out)) return rc;
        const auto t2 = std::chrono::steady_clock::now();
        ua[i] = (t1 - t0).count();
        uf[i] = (t2 - t1).count();
    }
    median_p99(ua, out_us);
    median_p99(uf, out_us + 2);
    return JSP_OK;
}

int jsp_engine_get_metrics(jsp_engine* e, jsp_metrics* out, int reset) {
    if (!e) return set_err(JSP_EINVAL, "engine is NULL");
    if (!out && !reset) return set_err(JSP_EINVAL, "out is NULL");
    std::lock_guard<std::mutex> l(e->met_mu);
    if (out) *out = e->met;
    // the placements answered under the lease: recorded under mu, never
    // waited for here (jsp_leased_metrics.h)
    e->lmet.add_to(out, reset != 0);
    if (reset) e->met = jsp_metrics{};
    return JSP_OK;
}

int jspb_place_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                   int32_t* assign_out, uint32_t iters, const uint32_t* patch_rows, const uint32_t* patch_taints,
                   uint32_t n_patch, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (int rc = check_timed(iters, 1000000, out_us)) return rc;
    if (n_patch > 0 && (!patch_rows || !patch_taints)) return set_err(JSP_EINVAL, "patch rows / taints are NULL");
    return timed_calls(iters, out_us, [&](uint32_t i) {
        if (n_patch > 0) {
            const uint32_t k = i % n_patch;
            if (int rc = jsp_snapshot_patch(e, patch_rows + k, 1, nullptr, patch_taints + k, nullptr, nullptr)) return rc;
        }
        return jsp_place(e, run_class, run_len, n_runs, assign_out, nullptr, nullptr, nullptr);
    });
}

// The idle period or gap of jspb_recovery_loop: slept, or spun (a busy caller).
static void recovery_wait(double us, bool spin) {
    if (us <= 0.0) return;
    const auto end = std::chrono::steady_clock::now() + std::chrono::duration<double, std::micro>(us);
    if (!spin) {
        std::this_thread::sleep_until(end);
        return;
    }
    while (std::chrono::steady_clock::now() < end) __builtin_ia32_pause();
}

int jspb_recovery_loop(jsp_engine* e, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                      int32_t* assign_out, uint32_t trials, double idle_us, double gap_us, int spin,
                      const uint32_t* patch_rows, const uint32_t* patch_taints, uint32_t n_patch, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (trials == 0 || trials > 100000) return set_err(JSP_EINVAL, "trials %u out of range [1,100000]", trials);
    if (!out_us) return set_err(JSP_EINVAL, "out_us is NULL");
    if (!(idle_us >= 0.0 && idle_us <= 1e7 && gap_us >= 0.0 && gap_us <= 1e7))
        return set_err(JSP_EINVAL, "idle / gap out of range [0, 10 s]");
    if (n_patch > 0 && (!patch_rows || !patch_taints)) return set_err(JSP_EINVAL, "patch rows / taints are NULL");
    using clk = std::chrono::steady_clock;
    const auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    for (uint32_t t = 0; t < trials; ++t) {
        recovery_wait(idle_us, spin != 0);
        const uint32_t k = n_patch ? t % n_patch : 0u;
        const auto t0 = clk::now();
        if (n_patch > 0)
            if (int rc = jsp_snapshot_patch(e, patch_rows + k, 1, nullptr, patch_taints + k, nullptr, nullptr)) return rc;
        const auto t1 = clk::now();
        recovery_wait(gap_us, spin != 0);
        const auto t2 = clk::now();
        if (int rc = jsp_place(e, run_class, run_len, n_runs, assign_out, nullptr, nullptr, nullptr)) return rc;
        const auto t3 = clk::now();
        out_us[3 * t] = us(t0, t1);
        out_us[3 * t + 1] = us(t2, t3);
        out_us[3 * t + 2] = us(t1, t2);
    }
    return JSP_OK;
}

int jsp_place_jobs(jsp_engine* e, const uint32_t* job_class, uint32_t n_jobs, int32_t* assign_out,
                   uint32_t* tally_out, uint32_t* occ_out, jsp_stats* stats) {
    if (n_jobs > 0 && !job_class) return set_err(JSP_EINVAL, "job_class is NULL");
    std::vector<uint32_t> rc, rl;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        if (rc.empty() || rc.back() != job_class[j]) {
            rc.push_back(job_class[j]);
            rl.push_back(0);
        }
        ++rl.back();
    }
    return jsp_place(e, rc.data(), rl.data(), (uint32_t)rc.size(), assign_out, tally_out, occ_out, stats);
}

int jsp_resolve_leader_domains(jsp_engine* e, const int32_t* leader_rows, const uint32_t* levels, uint32_t n,
                               int32_t* domain_out) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::resolve(e->multi, leader_rows, levels, n, domain_out); }
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, false)) return rc;
    if (n == 0) return JSP_OK;
    if (!leader_rows || !levels || !domain_out) return set_err(JSP_EINVAL, "NULL buffer");
    hipStream_t s = e->stream;
    if (int rc = use_engine_stream(e)) return rc;
    // inputs and output through pinned staging the kernel reads and writes in
    // place: no copy launches (a pageable copy can stall behind the resident
    // service, tools/block_probe.hip)
    HIP_TRY(e->h_batch.reserve((size_t)n * 12, grave(e)));
    int32_t* hr = e->h_batch.as<int32_t>();
    uint32_t* hl = reinterpret_cast<uint32_t*>(hr + n);
    int32_t* ho = hr + 2 * (size_t)n;
    std::memcpy(hr, leader_rows, (size_t)n * 4);
    std::memcpy(hl, levels, (size_t)n * 4);
    HIP_TRY(jsp::launch_resolve(hr, hl, n, e->N, e->leaf_start.as<uint32_t>(), e->n_leaves, e->leaf_begin, e->topo, ho,
                                s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(domain_out, ho, (size_t)n * 4);
    return JSP_OK;
}

int jsp_audit_placements(jsp_engine* e, const int32_t* leader_rows, const uint32_t* levels,
                         const uint32_t* follower_off, const int32_t* follower_domains, uint32_t n_jobs,
                         uint32_t* bad_out) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::audit(e->multi, leader_rows, levels, follower_off, follower_domains, n_jobs, bad_out); }
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, false)) return rc;
    if (n_jobs == 0) return JSP_OK;
    if (!leader_rows || !levels || !follower_off || !bad_out) return set_err(JSP_EINVAL, "NULL buffer");
    const uint32_t M = follower_off[n_jobs];
    if (follower_off[0] != 0) return set_err(JSP_EINVAL, "follower_off[0] must be 0");
    for (uint32_t i = 0; i < n_jobs; ++i)
        if (follower_off[i] > follower_off[i + 1]) return set_err(JSP_EINVAL, "follower_off not monotone at %u", i);
    if (M > 0 && !follower_domains) return set_err(JSP_EINVAL, "follower_domains is NULL");
    hipStream_t s = e->stream;
    if (int rc = use_engine_stream(e)) return rc;
    // pinned staging read and written in place by the kernel (as the resolve)
    const size_t n = n_jobs;
    HIP_TRY(e->h_batch.reserve((n * 4 + 1 + (size_t)M) * 4, grave(e)));
    int32_t* hr = e->h_batch.as<int32_t>();
    uint32_t* hl = reinterpret_cast<uint32_t*>(hr + n);
    uint32_t* hf = hl + n;
    int32_t* hd = reinterpret_cast<int32_t*>(hf + n + 1);
    uint32_t* ho = reinterpret_cast<uint32_t*>(hd + M);
    std::memcpy(hr, leader_rows, n * 4);
    std::memcpy(hl, levels, n * 4);
    std::memcpy(hf, follower_off, (n + 1) * 4);
    if (M > 0) std::memcpy(hd, follower_domains, (size_t)M * 4);
    HIP_TRY(jsp::launch_audit(hr, hl, hf, hd, n_jobs, e->N, e->leaf_start.as<uint32_t>(), e->n_leaves, e->leaf_begin,
                              e->topo, ho, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(bad_out, ho, n * 4);
    return JSP_OK;
}

// The explain passes on the engine stream (the caller has entered it): the
// row pass over this engine's rows when `rows`, the domain pass over the
// given tallies when d_cap is not null; then one copy of the C records and
// the wait. *recs: the records in pinned memory, *occupied: the occupied rows.
static int explain_impl(jsp_engine* e, bool rows, const uint32_t* d_cap, const uint32_t* d_occ, uint32_t ld,
                        const jsp::ExplainRec** recs, uint64_t* occupied) {
    hipStream_t s = e->stream;
    const uint32_t C = e->C;
    const size_t out_bytes = jsp::explain_out_bytes(C);
    HIP_TRY(e->ex_out.reserve(out_bytes, grave(e)));
    HIP_TRY(e->h_explain.reserve(out_bytes, grave(e)));
    HIP_TRY(hipMemsetAsync(e->ex_out.p, 0, out_bytes, s));
    uint32_t grid = 0;
    if (rows) {
        grid = jsp::explain_rows_grid(e->N, e->n_cu);
        HIP_TRY(e->ex_parts.reserve(jsp::explain_parts_bytes(grid, C), grave(e)));
        const jsp::TallyArgs a = tally_args(e, nullptr, nullptr, 0);
        HIP_TRY(jsp::launch_explain_rows(a, e->N, C, grid, e->ex_parts.as<uint32_t>(), s));
    }
    HIP_TRY(jsp::launch_explain_domains(d_cap, d_occ, ld, e->cls.as<jsp::DevClass>(), C, e->word_off.as<uint32_t>(),
                                        e->feas_words, e->topo, rows ? e->ex_parts.as<uint32_t>() : nullptr, grid,
                                        e->ex_out.as<jsp::ExplainRec>(), s));
    HIP_TRY(hipMemcpyAsync(e->h_explain.p, e->ex_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *recs = e->h_explain.as<jsp::ExplainRec>();
    std::memcpy(occupied, e->h_explain.as<char>() + (size_t)C * sizeof(jsp::ExplainRec), 8);
    return JSP_OK;
}

// The row counters of a record into the ABI struct (added: shards sum).
static void explain_add_rows(jsp_class_explain* o, const jsp::ExplainRec& r, uint32_t n_rows, uint64_t occupied) {
    o->rows += n_rows;
    o->rows_selector += r.rows[0];
    o->rows_taint += r.rows[1];
    o->rows_no_capacity += r.rows[2];
    o->rows_fit += r.rows[3];
    for (int i = 0; i < JSP_MAX_RES; ++i) o->rows_insufficient[i] += r.rows[4 + i];
    o->rows_occupied += occupied;
}

static void explain_set_domains(jsp_class_explain* o, const jsp::ExplainRec& r, uint32_t domains) {
    o->domains = domains;
    o->dom_occupied = r.dom_occupied;
    o->dom_short = r.dom_short;
    o->dom_feasible = r.dom_feasible;
    o->best_short_cap = r.best ? (uint32_t)(r.best >> 32) : 0u;
    o->best_short_domain = r.best ? (int32_t)(0xFFFFFFFFu - (uint32_t)r.best) : -1;
}

int jsp_explain(jsp_engine* e, jsp_class_explain* out, uint32_t n_classes) {
    if (int rc = check_engine(e)) return rc;
    if (!out) return set_err(JSP_EINVAL, "out is NULL");
    if (e->multi) { DeviceGuard dg; return jspm::explain(e->multi, out, n_classes); }
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (n_classes != e->C) return set_err(JSP_EINVAL, "n_classes %u differs from the %u classes uploaded", n_classes, e->C);
    if (e->leaf_begin != 0 || e->n_leaves != e->L_total)
        return set_err(JSP_ESTATE, "sharded engine: the domains need every shard's tallies (use a device-set engine)");
    if (e->C == 0) return JSP_OK;
    hipStream_t s = nullptr;
    if (int rc = enter_engine_stream(e, false, &s)) return rc;
    if (int rc = tally_whole(e, s)) return rc;
    const jsp::ExplainRec* recs = nullptr;
    uint64_t occupied = 0;
    if (int rc = explain_impl(e, true, e->cap.as<uint32_t>(), e->occ.as<uint32_t>(), e->L_total, &recs, &occupied))
        return rc;
    std::memset(out, 0, sizeof(jsp_class_explain) * (size_t)e->C);
    for (uint32_t c = 0; c < e->C; ++c) {
        explain_add_rows(&out[c], recs[c], e->N, occupied);
        explain_set_domains(&out[c], recs[c], e->D[e->cls_h[c].level]);
    }
    return JSP_OK;
}

int jspb_set_fused(jsp_engine* e, int mode) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::forward(e->multi, 0, mode); }
    std::lock_guard<std::mutex> g(e->mu);
    if (mode != JSP_FUSED_OFF && mode != JSP_FUSED_AUTO) return set_err(JSP_EINVAL, "fused mode %d", mode);
    lease_drop(e);
    if (mode != e->fused_mode) {
        if (int rc = svc_stop(e)) return rc;
        e->svc.zero_key = ~0ull;
    }
    e->fused_mode = mode;
    return JSP_OK;
}

// The last plan: a call the resident service answered (place_call reports it
// as shape 3 or 5) made no launch, so the plan of that service's start stands
// for it; every other call left its plan where it issued its launches.
int jspb_last_plan(jsp_engine* e, jspb_plan* out) {
    if (int rc = check_engine(e)) return rc;
    if (!out) return set_err(JSP_EINVAL, "out is NULL");
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: the shards plan their own launches");
    std::lock_guard<std::mutex> g(e->mu);
    *out = e->last_shape == 3 || e->last_shape == 5 ? e->svc_plan : e->plan;
    return JSP_OK;
}

int jsp_engine_set_service(jsp_engine* e, int mode) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::forward(e->multi, 1, mode); }
    std::lock_guard<std::mutex> g(e->mu);
    if (mode != JSP_SERVICE_OFF && mode != JSP_SERVICE_AUTO && mode != JSP_SERVICE_PARKED)
        return set_err(JSP_EINVAL, "service mode %d", mode);
    lease_drop(e);
    if (mode != e->svc_mode) {  // the running service's shape may change
        e->svc.resume = false;
        e->svc.armed = false;
        e->waker_poll.store(false, std::memory_order_release);
        if (int rc = svc_stop(e)) return rc;
        e->svc.zero_key = ~0ull;
    }
    e->svc_mode = mode;
    return JSP_OK;
}

int jspb_service_clock(jsp_engine* e, uint32_t* out, uint32_t cap, uint32_t* n_tiles) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { if (n_tiles) *n_tiles = 0; return JSP_OK; }
    std::lock_guard<std::mutex> g(e->mu);
    if (!n_tiles) return set_err(JSP_EINVAL, "n_tiles is NULL");
    *n_tiles = 0;
    const auto& v = e->svc;
    if (!v.clk || !v.words.p) return JSP_OK;
    const uint32_t n = std::min<uint32_t>(cap / jsp::kSvcClkSlots, v.nb);
    if (n > 0 && !out) return set_err(JSP_EINVAL, "out is NULL");
    // the tiles' rows, then (room permitting) the dispatcher's {request seen, bell rung}
    const uint32_t rows = n == v.nb && cap / jsp::kSvcClkSlots > v.nb ? n + 1 : n;
    std::memcpy(out, v.words.as<uint32_t>() + v.nb + 3, (size_t)rows * jsp::kSvcClkSlots * 4);
    *n_tiles = n;
    return JSP_OK;
}

int jspb_service_counters(jsp_engine* e, uint64_t* out) {
    if (int rc = check_engine(e)) return rc;
    if (!out) return set_err(JSP_EINVAL, "out is NULL");
    std::memset(out, 0, jsp::kSvcCounters * sizeof(uint64_t));
    if (e->multi) return JSP_OK;
    std::lock_guard<std::mutex> g(e->mu);
    const auto& v = e->svc;
    if (v.running) return set_err(JSP_ESTATE, "the service is running: its counters are written when it leaves");
    if (!v.counters.p) return JSP_OK;
    for (uint32_t i = 0; i < jsp::kSvcCounters; ++i)
        out[i] = __atomic_load_n(v.counters.as<uint32_t>() + i, __ATOMIC_ACQUIRE);
    return JSP_OK;
}

int jspb_lease_counters(jsp_engine* e, uint64_t* out, int reset) {
    if (int rc = check_engine(e)) return rc;
    if (!out && !reset) return set_err(JSP_EINVAL, "out is NULL");
    if (out) out[0] = out[1] = out[2] = 0;
    if (e->multi) return JSP_OK;
    std::lock_guard<std::mutex> g(e->mu);
    auto& l = e->lease;
    if (out) {
        out[0] = l.answered;
        out[1] = l.taken;
        out[2] = l.dropped;
    }
    if (reset) l.answered = l.taken = l.dropped = 0;
    return JSP_OK;
}

int jspb_expand_lines(const uint64_t* lines, uint32_t n_tiles, const uint32_t* l0, uint32_t base, uint32_t seq,
                      uint32_t J, int32_t* out, uint32_t* placed) {
    if (!placed || (n_tiles > 0 && (!lines || !l0)) || (J > 0 && !out)) return set_err(JSP_EINVAL, "a buffer is NULL");
    uint32_t t = 0, j = 0;
    const bool whole = expand_lines(reinterpret_cast<const unsigned long long*>(lines), n_tiles, l0, base, seq, J, out,
                                    &t, &j, [] {});
    *placed = j;
    if (!whole) return 1;
    for (uint32_t i = j; i < J; ++i) out[i] = -1;
    return JSP_OK;
}

int jspb_lines_tagged(const uint64_t* lines, uint32_t n_tiles, uint32_t seq) {
    if (n_tiles > 0 && !lines) return set_err(JSP_EINVAL, "lines is NULL");
    return lines_tagged(reinterpret_cast<const unsigned long long*>(lines), n_tiles, seq) ? 1 : 0;
}

int jspb_list_answer(const int32_t* list, uint32_t n_list, uint32_t J, int32_t* out, uint32_t* placed) {
    if (!placed || (n_list > 0 && !list) || (J > 0 && !out)) return set_err(JSP_EINVAL, "a buffer is NULL");
    list_answer(list, n_list, J, out, placed);
    return JSP_OK;
}

int jspb_fast_clock_probe(uint32_t n, int64_t* out) {
    if (!out) return set_err(JSP_EINVAL, "out is NULL");
    jsp_clock::calibrate();
    const bool fast = read_hooks().fast_clock;
    using clk = std::chrono::steady_clock;
    for (uint32_t i = 0; i < n; ++i) {
        // a pair taken across a preemption says nothing about the clock: again
        for (int tries = 0;; ++tries) {
            const int64_t s0 = jsp_clock::to_ns(clk::now());
            const int64_t f = jsp_clock::to_ns(fast ? jsp_clock::fast_now() : clk::now());
            const int64_t s1 = jsp_clock::to_ns(clk::now());
            out[2 * (size_t)i] = f;
            out[2 * (size_t)i + 1] = s0 + (s1 - s0) / 2;
            if (s1 - s0 <= 2000 || tries >= 100) break;
        }
    }
    out[2 * (size_t)n] = fast && jsp_clock::tsc_in_use() ? 1 : 0;
    return JSP_OK;
}

int jspb_scrape_loop(jsp_engine* e, double seconds, uint64_t* out) {
    if (int rc = check_engine(e)) return rc;
    if (!out || !(seconds > 0.0 && seconds <= 10.0)) return set_err(JSP_EINVAL, "out is NULL, or seconds not in (0, 10]");
    using clk = std::chrono::steady_clock;
    const auto end = clk::now() + std::chrono::duration<double>(seconds);
    uint64_t n = 0, worst = 0, fell = 0, last = 0;
    for (auto t = clk::now(); t < end; ++n) {
        jsp_metrics m;
        if (int rc = jsp_engine_get_metrics(e, &m, 0)) return rc;
        const auto t1 = clk::now();
        worst = std::max<uint64_t>(worst, (uint64_t)(t1 - t).count());
        fell += m.place_us.count < last ? 1 : 0;
        last = m.place_us.count;
        t = t1;
    }
    out[0] = n;
    out[1] = worst;
    out[2] = fell;
    out[3] = last;
    return JSP_OK;
}

int jspb_select_median_p99(const int64_t* samples_ns, uint32_t n, double* out) {
    if (n == 0 || !samples_ns || !out) return set_err(JSP_EINVAL, "no samples, or a buffer is NULL");
    select_median_p99(samples_ns, n, out);
    return JSP_OK;
}

int jspb_lease_memo_counters(jsp_engine* e, uint64_t* out, int reset) {
    if (int rc = check_engine(e)) return rc;
    if (!out && !reset) return set_err(JSP_EINVAL, "out is NULL");
    if (out) out[0] = out[1] = 0;
    if (e->multi) return JSP_OK;
    std::lock_guard<std::mutex> g(e->mu);
    auto& m = e->memo;
    if (out) {
        out[0] = m.answered;
        out[1] = m.built;
    }
    if (reset) m.answered = m.built = 0;
    return JSP_OK;
}

int jsp_engine_service_stop(jsp_engine* e) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) return JSP_OK;
    std::lock_guard<std::mutex> g(e->mu);
    e->svc.resume = false;
    e->svc.armed = false;  // no patch restarts it until a jsp_place is answered by it again
    e->waker_poll.store(false, std::memory_order_release);
    e->wake_job = false;   // nor a wake still queued (its patch lands through patch_wait)
    return svc_stop(e);
}

}  // extern "C"

// ---- internal entry points of the device-set engine (jsp_multi.h)
bool jspi_fold_ok(jsp_engine* e) {
    std::lock_guard<std::mutex> g(e->mu);
    return e->have_cls && e->have_snap && fold_ok(e, true);
}

uint64_t* jspi_feas(jsp_engine* e, uint32_t* words) {
    std::lock_guard<std::mutex> g(e->mu);
    if (words) *words = e->feas_words;
    return e->feas.as<uint64_t>();
}

int jspi_tally(jsp_engine* e, uint32_t* d_cap, uint32_t* d_occ, uint32_t ld, uint64_t* fold_feas) {
    if (int rc = check_engine(e)) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (ld < e->L_total) return set_err(JSP_EINVAL, "ld %u < total leaves %u", ld, e->L_total);
    if (fold_feas && !fold_ok(e, true)) return set_err(JSP_ESTATE, "this shard cannot fold its feasibility");
    if (int rc = check_launch_error(e)) return rc;
    if (int rc = enter_stream(e, e->stream)) return rc;
    const int rc = tally_impl(e, d_cap, d_occ, ld, e->stream, fold_feas);
    if (int lr = leave_stream(e, e->stream)) return lr;
    return rc;
}

int jspi_assign(jsp_engine* e, const uint32_t* d_cap, const uint32_t* d_occ, uint32_t ld, const uint32_t* run_class,
                const uint32_t* run_len, uint32_t n_runs, uint32_t J, int32_t* assign, bool folded) {
    if (int rc = check_engine(e)) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (int rc = check_launch_error(e)) return rc;
    if (int rc = enter_stream(e, e->stream)) return rc;
    const int rc = assign_impl(e, d_cap, d_occ, ld, run_class, run_len, n_runs, J, assign, e->stream, folded, true);
    if (int lr = leave_stream(e, e->stream)) return lr;
    return rc;
}

int jspi_explain_rows(jsp_engine* e, jsp_class_explain* acc) {
    if (int rc = check_engine(e)) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (e->C == 0) return JSP_OK;
    if (int rc = check_launch_error(e)) return rc;
    if (int rc = use_engine_stream(e)) return rc;
    const jsp::ExplainRec* recs = nullptr;
    uint64_t occupied = 0;
    if (int rc = explain_impl(e, true, nullptr, nullptr, 0, &recs, &occupied)) return rc;
    for (uint32_t c = 0; c < e->C; ++c) explain_add_rows(&acc[c], recs[c], e->N, occupied);
    return JSP_OK;
}

int jspi_explain_domains(jsp_engine* e, const uint32_t* d_cap, const uint32_t* d_occ, uint32_t ld,
                         jsp_class_explain* out) {
    if (int rc = check_engine(e)) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = ready(e, true)) return rc;
    if (e->C == 0) return JSP_OK;
    if (int rc = check_launch_error(e)) return rc;
    if (int rc = use_engine_stream(e)) return rc;
    const jsp::ExplainRec* recs = nullptr;
    uint64_t occupied = 0;
    if (int rc = explain_impl(e, false, d_cap, d_occ, ld, &recs, &occupied)) return rc;
    for (uint32_t c = 0; c < e->C; ++c) explain_set_domains(&out[c], recs[c], e->D[e->cls_h[c].level]);
    return JSP_OK;
}

int jspi_check(jsp_engine* e) {
    std::lock_guard<std::mutex> g(e->mu);
    return check_launch_error(e);
}

extern "C" {

int jspb_link_floor(jsp_engine* e, uint32_t iters, double* out_us) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) return set_err(JSP_ESTATE, "device-set engine: probe a shard engine");
    std::lock_guard<std::mutex> g(e->mu);
    if (iters == 0 || iters > 100000) return set_err(JSP_EINVAL, "iters %u out of range [1,100000]", iters);
    if (!out_us) return set_err(JSP_EINVAL, "out_us is NULL");
    HostBuf box;
    HIP_TRY(box.reserve(512));
    uint32_t* req = box.as<uint32_t>();
    uint32_t* ack = req + 32;  // four ack words, 64 B apart, on lines of their own
    std::memset(box.p, 0, 512);
    hipStream_t s = e->stream;
    if (int rc = use_engine_stream(e)) return rc;
    const uint32_t warm = std::min<uint32_t>(50, iters);
    const uint32_t n = iters + warm;
    HIP_TRY(jsp::launch_link_probe(req, ack, n, 100000000ull, s));  // a wave waits <= 1 s per request
    auto acked = [&](uint32_t i) {
        for (int w = 0; w < 4; ++w)
            if (__atomic_load_n(ack + 16 * w, __ATOMIC_ACQUIRE) >= i) return true;
        return false;
    };
    std::vector<double> us;
    us.reserve(iters);
    int rc = JSP_OK;
    for (uint32_t i = 1; i <= n && rc == JSP_OK; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        __atomic_store_n(req, i, __ATOMIC_RELEASE);
        while (!acked(i)) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) {
                rc = set_err(JSP_EHIP, "host-link probe: request %u not answered within 500 ms", i);
                break;
            }
        }
        if (i > warm) us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    if (rc != JSP_OK) __atomic_store_n(req, n, __ATOMIC_RELEASE);  // let every wave finish
    HIP_TRY(hipStreamSynchronize(s));
    if (rc != JSP_OK) return rc;
    std::sort(us.begin(), us.end());
    double sum = 0;
    for (double x : us) sum += x;
    out_us[0] = us[us.size() / 2];
    out_us[1] = us[std::min(us.size() - 1, (size_t)(0.99 * us.size()))];
    out_us[2] = sum / us.size();
    return JSP_OK;
}

int jspb_set_timing(jsp_engine* e, int enable) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::forward(e->multi, 2, enable); }
    std::lock_guard<std::mutex> g(e->mu);
    lease_drop(e);  // the stamps go on or off: the service restarts for them
    e->timing = enable != 0;
    return JSP_OK;
}

int jspb_get_timing(jsp_engine* e, jsp_timing* out, int reset) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::get_timing(e->multi, out, reset); }
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = resolve_timing(e)) return rc;
    if (out) *out = e->acc;
    if (reset) e->acc = jsp_timing{};
    return JSP_OK;
}

void* jsp_engine_stream(jsp_engine* e) {
    if (e && e->multi) return jspm::stream(e->multi);
    return e ? static_cast<void*>(e->stream) : nullptr;
}

int jsp_engine_sync(jsp_engine* e) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::sync(e->multi); }
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = svc_settle(e)) return rc;  // the service's last request finished on every tile
    if (int rc = patch_wait(e)) return rc;  // and every patch landed
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->have_last && e->last_foreign) {
        if (int rc = wait_last_foreign(e)) return rc;
    }
    return JSP_OK;
}

int jsp_engine_check(jsp_engine* e) {
    if (int rc = check_engine(e)) return rc;
    if (e->multi) { DeviceGuard dg; return jspm::check(e->multi); }
    std::lock_guard<std::mutex> g(e->mu);
    // everything enqueued so far is ordered before the last call's work, so
    // waiting for that (an engine-owned event, or the engine stream) suffices
    if (e->have_last) {
        if (e->last_foreign) {
            if (int rc = wait_last_foreign(e)) return rc;
        } else {
            HIP_TRY(hipStreamSynchronize(e->stream));
        }
    }
    return check_launch_error(e);
}

}  // extern "C"
