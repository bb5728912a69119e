// jsp_leased_metrics.h -- the metrics of placements answered under the host
// lease (DESIGN.md §4.3 "the entry stamps"): the part of jsp_metrics a
// placement touches, written by the answering call itself while it holds the
// engine's lock, so that a leased answer takes no second lock. No HIP and
// nothing of the engine (tools/clock_check.cc runs it alone).
//
// One writer at a time (the engine's lock serialises them): every field is
// written with a relaxed load and a store, no read-modify-write instruction.
// Readers (jsp_engine_get_metrics) are serialised by the metrics' lock and
// never take the engine's: they read between two equal, even values of seq,
// which the writer makes odd for the ~10 stores of one call, so a snapshot
// holds whole calls only. (A reader that sees a writer in 1000 times running --
// one preempted inside its stores -- takes the fields as they stand: that one
// call may then show in some fields and not in others.)
//
// A reset zeroes nothing the writer owns: the reader keeps the snapshot it
// took as the base that later reads subtract, and bumps epoch, which only it
// writes. The maxima cannot be subtracted: the writer starts one afresh when
// it sees a new epoch, and a reader counts a maximum only when it carries the
// current one. (A leased call in flight across a reset may keep the old epoch
// on its maximum: that one value is then left out of `max`, never added to a
// later period's.)
#ifndef JSP_LEASED_METRICS_H
#define JSP_LEASED_METRICS_H

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <thread>

#include "../../include/jsplace.h"

// The bucket of one value in a log2 histogram (jsplace.h jsp_hist): 0 below
// lo, i for [lo 2^(i-1), lo 2^i), the last one the rest.
inline int hist_bucket(double v, double lo) {
    if (!(v >= lo)) return 0;
    int ex = 0;
    (void)std::frexp(v / lo, &ex);
    return std::min(ex, JSP_HIST_BUCKETS - 1);
}

struct LeasedMetrics {
    struct Hist {
        std::atomic<uint64_t> count{0};
        std::atomic<double> sum{0.0};
        std::atomic<double> max{0.0};
        std::atomic<uint32_t> max_epoch{0};  // the epoch max was started in
        std::atomic<uint64_t> bucket[JSP_HIST_BUCKETS] = {};
    };
    // what a reader took: the histograms (max: 0 unless of the current epoch) and the counters
    struct Snap {
        jsp_hist place_us, batch_jobs;
        uint64_t placed, unplaceable, svc_calls;
    };

    std::atomic<uint32_t> seq{0};
    Hist place_us, batch_jobs;
    std::atomic<uint64_t> placed{0}, unplaceable{0}, svc_calls{0};
    std::atomic<uint32_t> epoch{0};  // the readers': bumped by a reset
    Snap base{};                     // the readers': the snapshot of the last reset

    // The fields' stores are release and the readers' loads acquire (plain
    // moves on x86-64, like relaxed ones): the stores stay behind the store
    // that makes seq odd, the loads ahead of the second read of seq.
    static constexpr std::memory_order kStore = std::memory_order_release, kLoad = std::memory_order_acquire;
    static void bump(std::atomic<uint64_t>& a, uint64_t by = 1) {
        a.store(a.load(std::memory_order_relaxed) + by, kStore);
    }
    static void add(Hist& h, double v, double lo, uint32_t ep) {
        bump(h.count);
        h.sum.store(h.sum.load(std::memory_order_relaxed) + v, kStore);
        if (h.max_epoch.load(std::memory_order_relaxed) != ep) {
            h.max.store(v, kStore);
            h.max_epoch.store(ep, kStore);  // behind its max
        } else if (v > h.max.load(std::memory_order_relaxed)) {
            h.max.store(v, kStore);
        }
        bump(h.bucket[hist_bucket(v, lo)]);
    }

    // The writer (under the engine's lock): one successful placement answered
    // by the service under the lease, as jsp_place records it.
    void record(double us, uint32_t jobs, uint32_t n_placed) {
        const uint32_t ep = epoch.load(std::memory_order_acquire);
        const uint32_t s = seq.load(std::memory_order_relaxed);
        seq.store(s + 1, std::memory_order_relaxed);
        add(place_us, us, JSP_HIST_LO_US, ep);
        add(batch_jobs, (double)jobs, JSP_HIST_LO_JOBS, ep);
        bump(placed, n_placed);
        bump(unplaceable, jobs - n_placed);
        bump(svc_calls);
        seq.store(s + 2, std::memory_order_release);
    }

    static void take(const Hist& h, uint32_t ep, jsp_hist* out) {
        out->count = h.count.load(kLoad);
        out->sum = h.sum.load(kLoad);
        const bool cur = h.max_epoch.load(kLoad) == ep;  // ahead of its max
        out->max = cur ? h.max.load(kLoad) : 0.0;
        for (int i = 0; i < JSP_HIST_BUCKETS; ++i) out->bucket[i] = h.bucket[i].load(kLoad);
    }
    Snap snapshot() const {
        Snap sn;
        const uint32_t ep = epoch.load(std::memory_order_relaxed);
        for (int tries = 0;; ++tries) {
            const uint32_t s = seq.load(std::memory_order_acquire);
            take(place_us, ep, &sn.place_us);
            take(batch_jobs, ep, &sn.batch_jobs);
            sn.placed = placed.load(kLoad);
            sn.unplaceable = unplaceable.load(kLoad);
            sn.svc_calls = svc_calls.load(kLoad);
            if ((!(s & 1u) && seq.load(std::memory_order_relaxed) == s) || tries >= 1000) return sn;
            if (tries >= 100) std::this_thread::yield();  // (a writer preempted inside its stores)
        }
    }
    static void add_since(jsp_hist& to, const jsp_hist& now, const jsp_hist& was) {
        to.count += now.count - was.count;
        to.sum += now.sum - was.sum;
        to.max = std::max(to.max, now.max);
        for (int i = 0; i < JSP_HIST_BUCKETS; ++i) to.bucket[i] += now.bucket[i] - was.bucket[i];
    }

    // The readers (under the metrics' lock): what was recorded since the last
    // reset added to *m (nullable), and, with reset, a new base.
    void add_to(jsp_metrics* m, bool reset) {
        const Snap sn = snapshot();
        if (m) {
            add_since(m->place_us, sn.place_us, base.place_us);
            add_since(m->batch_jobs, sn.batch_jobs, base.batch_jobs);
            m->placed += sn.placed - base.placed;
            m->unplaceable += sn.unplaceable - base.unplaceable;
            m->svc_calls += sn.svc_calls - base.svc_calls;
        }
        if (reset) {
            base = sn;
            epoch.store(epoch.load(std::memory_order_relaxed) + 1, std::memory_order_release);
        }
    }
};

#endif  // JSP_LEASED_METRICS_H
