// jsp_clock.h -- the host entry stamps' clock (DESIGN.md §4.3 "the entry
// stamps"): steady_clock time points read off the TSC. No HIP and nothing of
// the engine, so that the stand-alone programs under tools/ (clock_check)
// compile it alone.
//
// fast_now() is anchor + (rdtsc - anchor's tsc) * factor: the anchor a pair
// (steady_clock stamp, tsc) behind a seqlock, the factor fixed-point ns per
// tick (2^-32), taken once per process by calibrate() from two pairs at least
// 10 ms apart. Where the TSC is not the kernel's own clock source (see
// tsc_usable) or calibrate() has not run, fast_now() is steady_clock::now().
//
// The anchor is refreshed from real steady_clock reads: by anchor_now(), which
// a caller uses where it reads steady_clock anyway, and by fast_now() itself
// when the anchor is older than 1 s. At the calibration's ~6 ppm (10 ms
// window, +-30 ns per pair) an anchor up to 1 s old is within ~6 us of
// steady_clock; tests/test_fast_clock.py holds it to 50 us.
//
// Per thread the values handed out never decrease, across re-anchors too: a
// new anchor may sit behind the old one's extrapolation by the drift since,
// so every value is clamped to the last one the thread was given.
#ifndef JSP_CLOCK_H
#define JSP_CLOCK_H

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>

#if defined(__x86_64__)
#include <cpuid.h>
#include <x86intrin.h>
#endif

namespace jsp_clock {

using steady = std::chrono::steady_clock;

inline int64_t to_ns(steady::time_point t) {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(t.time_since_epoch()).count();
}
inline steady::time_point from_ns(int64_t ns) {
    return steady::time_point(std::chrono::duration_cast<steady::duration>(std::chrono::nanoseconds(ns)));
}

struct State {
    std::atomic<uint64_t> mult{0};        // ns per tick, 2^-32 units; 0: the TSC is not in use
    std::atomic<uint64_t> sec_ticks{0};   // ticks in 1 s: an older anchor is not extrapolated
    std::atomic<uint64_t> pair_ticks{0};  // ticks in 2 us: a pair whose reads lie further apart is no anchor
    // the anchor, a seqlock: seq odd while a writer is in; writers exclude
    // each other by the CAS that makes it odd (the loser keeps the old anchor)
    std::atomic<uint32_t> seq{0};
    std::atomic<int64_t> a_ns{0};
    std::atomic<uint64_t> a_tsc{0};
    std::once_flag once;
};
inline State g;

// The last value handed to this thread.
inline int64_t& thread_last() {
    thread_local int64_t v = INT64_MIN;
    return v;
}
inline int64_t clamp_thread(int64_t ns) {
    int64_t& last = thread_last();
    if (ns < last) ns = last;
    last = ns;
    return ns;
}

#if defined(__x86_64__)
inline uint64_t ticks() { return __rdtsc(); }

// x86-64 with an invariant TSC (CPUID 0x80000007 EDX bit 8) that the kernel
// itself keeps time by (it has then vouched for its cross-CPU synchronisation).
inline bool tsc_usable() {
    unsigned a = 0, b = 0, c = 0, d = 0;
    if (!__get_cpuid(0x80000000u, &a, &b, &c, &d) || a < 0x80000007u) return false;
    if (!__get_cpuid(0x80000007u, &a, &b, &c, &d) || !(d & (1u << 8))) return false;
    std::FILE* f = std::fopen("/sys/devices/system/clocksource/clocksource0/current_clocksource", "r");
    if (!f) return false;
    char buf[32] = {0};
    const bool got = std::fgets(buf, sizeof buf, f) != nullptr;
    std::fclose(f);
    return got && (std::strcmp(buf, "tsc\n") == 0 || std::strcmp(buf, "tsc") == 0);
}
#else
inline uint64_t ticks() { return 0; }
inline bool tsc_usable() { return false; }
#endif

// One (steady_clock, tsc) pair: the tsc the middle of two reads around the
// clock's. Returns the ticks between the two (a pair taken across a
// preemption is wide).
inline uint64_t take_pair(int64_t* ns, uint64_t* tsc) {
    const uint64_t a = ticks();
    *ns = to_ns(steady::now());
    const uint64_t b = ticks();
    *tsc = a + (b - a) / 2;
    return b - a;
}
// The narrowest of five.
inline void best_pair(int64_t* ns, uint64_t* tsc) {
    uint64_t best = UINT64_MAX;
    for (int i = 0; i < 5; ++i) {
        int64_t n;
        uint64_t t;
        const uint64_t w = take_pair(&n, &t);
        if (w < best) best = w, *ns = n, *tsc = t;
    }
}

// A new anchor, unless another writer is in or the anchor is newer already.
inline void reanchor(int64_t ns, uint64_t tsc) {
    uint32_t s = g.seq.load(std::memory_order_relaxed);
    if ((s & 1u) || !g.seq.compare_exchange_strong(s, s + 1, std::memory_order_acq_rel, std::memory_order_relaxed)) return;
    if ((int64_t)(tsc - g.a_tsc.load(std::memory_order_relaxed)) > 0) {
        // (release: behind the CAS that made seq odd)
        g.a_ns.store(ns, std::memory_order_release);
        g.a_tsc.store(tsc, std::memory_order_release);
    }
    g.seq.store(s + 2, std::memory_order_release);
}

// Once per process, off every hot path (engine creation): the first pair was
// taken when the library was loaded, the second here, 10 ms or more later
// (slept for where the process is younger than that).
struct FirstPair {
    int64_t ns = 0;
    uint64_t tsc = 0;
    bool usable = false;
    FirstPair() {
        usable = tsc_usable();
        if (usable) best_pair(&ns, &tsc);
    }
};
inline const FirstPair g_first;

inline void calibrate() {
    std::call_once(g.once, [] {
        if (!g_first.usable) return;
        constexpr int64_t kWindowNs = 10 * 1000 * 1000;
        int64_t ns = 0;
        uint64_t tsc = 0;
        for (;;) {
            best_pair(&ns, &tsc);
            const int64_t left = kWindowNs - (ns - g_first.ns);
            if (left <= 0) break;
            std::this_thread::sleep_for(std::chrono::nanoseconds(left));
        }
        const uint64_t dt = tsc - g_first.tsc;
        const uint64_t dn = (uint64_t)(ns - g_first.ns);
        // 0.1 .. 10 GHz, or the TSC is not what it claims
        if ((int64_t)dt <= 0 || dt < dn / 10 || dt / 10 > dn) return;
        const unsigned __int128 m = ((unsigned __int128)dn << 32) / dt;
        const uint64_t per_s = (uint64_t)(((unsigned __int128)dt * 1000000000ull) / dn);
        g.a_ns.store(ns, std::memory_order_relaxed);
        g.a_tsc.store(tsc, std::memory_order_relaxed);
        g.sec_ticks.store(per_s, std::memory_order_relaxed);
        g.pair_ticks.store(per_s / 500000, std::memory_order_relaxed);
        g.mult.store((uint64_t)m, std::memory_order_release);
    });
}

inline bool tsc_in_use() { return g.mult.load(std::memory_order_acquire) != 0; }

// A real steady_clock read that refreshes the anchor (where the pair is
// narrow enough to be one): for the caller that reads the clock anyway.
inline steady::time_point anchor_now() {
    if (!g.mult.load(std::memory_order_acquire)) return steady::now();
    int64_t ns;
    uint64_t tsc;
    if (take_pair(&ns, &tsc) <= g.pair_ticks.load(std::memory_order_relaxed)) reanchor(ns, tsc);
    return from_ns(clamp_thread(ns));
}

inline steady::time_point fast_now() {
    const uint64_t mult = g.mult.load(std::memory_order_acquire);
    if (!mult) return steady::now();
    const uint32_t s = g.seq.load(std::memory_order_acquire);
    if (!(s & 1u)) {
        // (acquire: the second read of seq stays behind them)
        const int64_t a_ns = g.a_ns.load(std::memory_order_acquire);
        const uint64_t a_tsc = g.a_tsc.load(std::memory_order_acquire);
        if (g.seq.load(std::memory_order_relaxed) == s) {
            // (rdtsc is not ordered with the loads: a hair before the anchor's counts as at it)
            const int64_t d = std::max<int64_t>((int64_t)(ticks() - a_tsc), 0);
            if ((uint64_t)d <= g.sec_ticks.load(std::memory_order_relaxed))
                return from_ns(clamp_thread(a_ns + (int64_t)(((unsigned __int128)(uint64_t)d * mult) >> 32)));
        }
    }
    // a writer is in, or the anchor is older than 1 s (a caller that idle is
    // not hot): the real clock, and a new anchor from it
    return anchor_now();
}

}  // namespace jsp_clock

#endif  // JSP_CLOCK_H
