// jsp_wait.h -- the host's guarded spin wait ("The waits'
// one loop"): spin on host-visible words, and now and then ask whether the
// stream that is to write them still runs. Plain C++, no HIP and nothing of
// the engine: the stream query is a callable, so that tools/wait_check.cc
// drives every branch on the CPU with a scripted query and a clock of its own.
#ifndef JSP_WAIT_H
#define JSP_WAIT_H

#include <chrono>
#include <cstdint>
#if defined(__x86_64__) || defined(__i386__)
#include <emmintrin.h>
#endif

// A wait's occasional status query (has the stream finished, or failed?):
// at most once per 20 us, the first no sooner than 20 us after construction.
// A query is a runtime call whose code and data a cold host core must first
// fetch, and the waits it guards mostly end within a few microseconds.
template <class Clock = std::chrono::steady_clock>
struct QueryPacer {
    typename Clock::time_point next = Clock::now() + std::chrono::microseconds(20);
    bool due() {
        const auto t = Clock::now();
        if (t < next) return false;
        next = t + std::chrono::microseconds(20);
        return true;
    }
};

// On guarded_wait, and on a site's progress step too large for the compiler to
// inline at both of the loop's calls by itself: [&](uint64_t) JSP_WAIT_INLINE {...}
#define JSP_WAIT_INLINE __attribute__((always_inline))

enum class StreamState { running, finished, failed };  // a stream query's answer

enum class WaitResult {
    ready,      // the answer is in
    abandoned,  // the side check said stop
    gone,       // the stream finished, and one more progress step still did not complete
    failed,     // the query reported an error (the query callable keeps which)
    late,       // the bound passed
};

// A wait's time bound: late once a query said running and now - start > limit.
template <class Clock = std::chrono::steady_clock>
struct WaitBound {
    typename Clock::time_point start;
    typename Clock::duration limit;
};

enum class WaitPause { no, yes };  // a pause instruction between spins

struct NoSideCheck {
    bool operator()() const { return false; }
};

// The loop. Every spin, counted from 1: step(spins), the site's own progress
// (advance, copy out, prefetch on its own cadence); true ends the wait, ready.
// Every 256th spin: side(), true abandons the wait; then, when the pacer is
// due, query(). A finished stream gets one last step(spins) before it counts
// as gone; a running one is held against the bound, if there is one -- the
// bound is looked at nowhere else. Holds no state beyond the pacer and sets
// no error: the caller maps the result to its own code and text.
template <class Clock = std::chrono::steady_clock, class Step, class Side, class Query>
inline JSP_WAIT_INLINE WaitResult guarded_wait(Step&& step, Side&& side, Query&& query,
                                               WaitPause pause = WaitPause::no,
                                               const WaitBound<Clock>* bound = nullptr) {
    QueryPacer<Clock> qp;
    for (uint64_t spins = 1;; ++spins) {
        if (step(spins)) return WaitResult::ready;
        if ((spins & 255) == 0) {
            if (side()) return WaitResult::abandoned;
            if (qp.due()) {
                const StreamState q = query();
                if (q == StreamState::finished) return step(spins) ? WaitResult::ready : WaitResult::gone;
                if (q == StreamState::failed) return WaitResult::failed;
                if (bound && Clock::now() - bound->start > bound->limit) return WaitResult::late;
            }
        }
#if defined(__x86_64__) || defined(__i386__)
        if (pause == WaitPause::yes) _mm_pause();
#endif
    }
}

#endif  // JSP_WAIT_H
