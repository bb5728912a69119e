// clock_check -- the entry stamps' clock (jsp_clock.h) and the leased answers'
// metrics (jsp_leased_metrics.h) under threads, stand-alone on the CPU: built
// with ASan + UBSan and with TSan by `make clock-asan` / `make clock-tsan`.
//
// 1. Four threads call fast_now() for 2 s while a fifth re-anchors every
//    100 us: no thread ever sees its clock go back, and every value is within
//    50 us of steady_clock read around it.
// 2. One writer records 100,000 leased placements (serialised as the engine's
//    lock serialises them) while two readers add the accumulator to a
//    jsp_metrics, one of them resetting now and then: a reader's count never
//    decreases except across a reset, a snapshot's buckets sum to its count,
//    and the periods between resets add up to exactly what was written.
#include <atomic>
#include <cinttypes>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>

#include "../jobset_amd/csrc/jsp_clock.h"
#include "../jobset_amd/csrc/jsp_leased_metrics.h"

static std::atomic<int> g_failed{0};
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);         \
            g_failed.fetch_add(1);            \
        }                                     \
    } while (0)

static int clock_threads() {
    using clk = std::chrono::steady_clock;
    jsp_clock::calibrate();
    std::printf("clock: TSC %s\n", jsp_clock::tsc_in_use() ? "in use" : "not in use (fast_now is steady_clock)");
    std::atomic<bool> stop{false};
    std::atomic<uint64_t> reads{0}, anchors{0};
    std::atomic<int64_t> worst{0};
    std::vector<std::thread> th;
    for (int k = 0; k < 4; ++k)
        th.emplace_back([&] {
            int64_t last = INT64_MIN, w = 0;
            uint64_t n = 0;
            while (!stop.load(std::memory_order_relaxed)) {
                const int64_t s0 = jsp_clock::to_ns(clk::now());
                const int64_t f = jsp_clock::to_ns(jsp_clock::fast_now());
                const int64_t s1 = jsp_clock::to_ns(clk::now());
                CHECK(f >= last, "fast_now went back by %" PRId64 " ns", last - f);
                last = f;
                // outside [s0, s1] by: (a preempted triple is wide, never wrong)
                const int64_t off = f < s0 ? s0 - f : f > s1 ? f - s1 : 0;
                if (off > w) w = off;
                ++n;
            }
            reads.fetch_add(n);
            int64_t cur = worst.load();
            while (w > cur && !worst.compare_exchange_weak(cur, w)) {}
        });
    std::thread anchor([&] {
        while (!stop.load(std::memory_order_relaxed)) {
            (void)jsp_clock::anchor_now();
            anchors.fetch_add(1, std::memory_order_relaxed);
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
    });
    std::this_thread::sleep_for(std::chrono::seconds(2));
    stop.store(true);
    for (auto& t : th) t.join();
    anchor.join();
    std::printf("clock: %" PRIu64 " reads on 4 threads, %" PRIu64 " re-anchors, worst offset %" PRId64 " ns\n",
                reads.load(), anchors.load(), worst.load());
    CHECK(worst.load() <= 50000, "fast_now was %" PRId64 " ns from steady_clock", worst.load());
    return 0;
}

static uint64_t buckets(const jsp_hist& h) {
    uint64_t n = 0;
    for (int i = 0; i < JSP_HIST_BUCKETS; ++i) n += h.bucket[i];
    return n;
}

static void metrics_threads() {
    constexpr uint32_t kCalls = 100000;
    LeasedMetrics acc;
    std::mutex met_mu;  // the readers', as the engine's met_mu
    std::atomic<bool> done{false};
    // what the periods closed by a reset held (under met_mu)
    uint64_t closed_count = 0, closed_placed = 0, closed_unplaceable = 0, closed_svc = 0, closed_jobs_count = 0;
    double closed_sum = 0.0;
    uint64_t resets = 0, scrapes = 0;

    std::thread writer([&] {
        // paced as calls are: a call's other work lies between two records (a
        // reader needs a gap as long as its own pass over the fields, and a
        // sanitizer slows the pass and these loads alike)
        std::atomic<uint32_t> work{0};
        uint32_t sink = 0;
        for (uint32_t i = 0; i < kCalls; ++i) {
            for (int k = 0; k < 600; ++k) sink += work.load(std::memory_order_relaxed);
            acc.record(0.25 * (1 + i % 8), 10, i % 11 < 10 ? i % 11 : 10);
        }
        work.store(sink);
        done.store(true);
    });
    auto reader = [&](bool resetting) {
        uint64_t last = 0;
        for (uint64_t n = 0; !done.load(); ++n) {
            jsp_metrics m{};
            const bool reset = resetting && n % 64 == 63;
            {
                std::lock_guard<std::mutex> l(met_mu);
                acc.add_to(&m, reset);
                if (reset) {
                    closed_count += m.place_us.count;
                    closed_jobs_count += m.batch_jobs.count;
                    closed_sum += m.place_us.sum;
                    closed_placed += m.placed;
                    closed_unplaceable += m.unplaceable;
                    closed_svc += m.svc_calls;
                    resets += 1;
                }
                scrapes += 1;
            }
            CHECK(buckets(m.place_us) == m.place_us.count, "place_us: %" PRIu64 " in buckets, count %" PRIu64,
                  buckets(m.place_us), m.place_us.count);
            CHECK(buckets(m.batch_jobs) == m.batch_jobs.count, "batch_jobs: buckets and count differ");
            CHECK(m.svc_calls == m.place_us.count && m.placed + m.unplaceable == 10 * m.place_us.count,
                  "a snapshot holds part of a call");
            CHECK(m.place_us.max <= 2.0, "max %g above every value written", m.place_us.max);
            // (the other reader's resets take the count down: only the resetting reader knows when)
            if (resetting) {
                CHECK(m.place_us.count >= last, "count fell from %" PRIu64 " to %" PRIu64 " without a reset", last,
                      m.place_us.count);
                last = reset ? 0 : m.place_us.count;
            }
        }
    };
    std::thread r1(reader, true), r2(reader, false);
    writer.join();
    r1.join();
    r2.join();

    jsp_metrics m{};
    acc.add_to(&m, false);
    uint64_t want_placed = 0;
    double want_sum = 0.0;
    for (uint32_t i = 0; i < kCalls; ++i) {
        want_placed += i % 11 < 10 ? i % 11 : 10;
        want_sum += 0.25 * (1 + i % 8);  // (multiples of 0.25: every partial sum is exact)
    }
    std::printf("metrics: %u calls, %" PRIu64 " scrapes, %" PRIu64 " resets\n", kCalls, scrapes, resets);
    CHECK(closed_count + m.place_us.count == kCalls, "place_us.count %" PRIu64 " of %u", closed_count + m.place_us.count,
          kCalls);
    CHECK(closed_jobs_count + m.batch_jobs.count == kCalls, "batch_jobs.count is not the calls'");
    CHECK(closed_svc + m.svc_calls == kCalls, "svc_calls is not the calls'");
    CHECK(closed_placed + m.placed == want_placed, "placed is not the calls'");
    CHECK(closed_unplaceable + m.unplaceable == 10ull * kCalls - want_placed, "unplaceable is not the calls'");
    CHECK(closed_sum + m.place_us.sum == want_sum, "place_us.sum %.17g, written %.17g", closed_sum + m.place_us.sum,
          want_sum);
    CHECK(buckets(m.place_us) == m.place_us.count, "the last period's buckets and count differ");
}

int main() {
    clock_threads();
    metrics_threads();
    if (g_failed.load()) {
        std::fprintf(stderr, "clock_check: %d checks failed\n", g_failed.load());
        return 1;
    }
    std::printf("clock_check: ok\n");
    return 0;
}
