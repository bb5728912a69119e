// wait_check -- every branch of the host's guarded spin wait
// (jobset_amd/csrc/jsp_wait.h) on the CPU, for the AddressSanitizer + UBSan
// build (make wait-asan): a scripted stream query (a list of answers, one per
// call, the calls counted) and a clock that only the cases advance, so that
// nothing sleeps and the engine's 10 s and 2 s bounds cost nothing. Includes
// jsp_wait.h alone: no GPU, no engine. Exit status 0 and "wait_check: ok"
// when every case holds.
#include <cstdio>
#include <functional>
#include <vector>

#include "../jobset_amd/csrc/jsp_wait.h"

namespace {
int failures = 0;

#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                           \
            std::printf("\n");                                  \
            ++failures;                                         \
        }                                                       \
    } while (0)

struct FakeClock {
    using duration = std::chrono::nanoseconds;
    using rep = duration::rep;
    using period = duration::period;
    using time_point = std::chrono::time_point<FakeClock>;
    static constexpr bool is_steady = true;
    static time_point t;
    static time_point now() { return t; }
    static void reset() { t = time_point(std::chrono::hours(1)); }
    static void advance(duration d) { t += d; }
};
FakeClock::time_point FakeClock::t{};

using std::chrono::microseconds;
using std::chrono::seconds;
const StreamState kRun = StreamState::running, kFin = StreamState::finished, kFail = StreamState::failed;

// The answers in order, one per call; a call past the script fails the case
// and ends the wait. `stored` stands for the engine callable's kept hipError_t.
struct Script {
    std::vector<StreamState> answers;
    unsigned calls = 0;
    int stored = 0;
    uint64_t steps_at_last_call = 0;
    const uint64_t* steps = nullptr;
    StreamState operator()() {
        if (steps) steps_at_last_call = *steps;
        if (calls >= answers.size()) {
            ++calls;
            CHECK(false, "query %u past a script of %zu", calls, answers.size());
            return kFail;
        }
        const StreamState a = answers[calls++];
        stored = a == kFail ? 700 + (int)calls : 0;
        return a;
    }
};

// One wait: `done(spins)` is the progress step's answer, `per_spin` runs in
// every step first (the cases move the clock there).
struct Run {
    uint64_t steps = 0, sides = 0, last_spins = 0;
    Script q;
    WaitResult r = WaitResult::ready;
    bool in_order = true;  // the step saw spins 1, 2, 3, ... (the last look repeats its spin)
};
Run run(std::vector<StreamState> answers, const std::function<bool(uint64_t, const Run&)>& done,
        const std::function<void(uint64_t)>& per_spin = nullptr, const std::function<bool(const Run&)>& side = nullptr,
        const WaitBound<FakeClock>* bound = nullptr, WaitPause pause = WaitPause::no) {
    Run x;
    x.q.answers = std::move(answers);
    x.q.steps = &x.steps;
    auto step = [&](uint64_t spins) {
        x.in_order = x.in_order && (spins == x.last_spins + 1 || (spins == x.last_spins && (spins & 255) == 0));
        x.last_spins = spins;
        ++x.steps;
        if (per_spin) per_spin(spins);
        return done(spins, x);
    };
    if (side)
        x.r = guarded_wait<FakeClock>(step, [&] { ++x.sides; return side(x); }, x.q, pause, bound);
    else
        x.r = guarded_wait<FakeClock>(step, NoSideCheck{}, x.q, pause, bound);
    CHECK(x.in_order, "the step's spin counts are out of order");
    return x;
}
auto at(uint64_t n) {  // the answer is in on spin n
    return [n](uint64_t spins, const Run&) { return spins >= n; };
}
const char* name(WaitResult r) {
    switch (r) {
        case WaitResult::ready: return "ready";
        case WaitResult::abandoned: return "abandoned";
        case WaitResult::gone: return "gone";
        case WaitResult::failed: return "failed";
        case WaitResult::late: return "late";
    }
    return "?";
}

void ready_cases() {
    FakeClock::reset();
    Run x = run({}, at(1));
    CHECK(x.r == WaitResult::ready && x.steps == 1 && x.q.calls == 0, "first spin: %s, %llu steps, %u queries", name(x.r),
          (unsigned long long)x.steps, x.q.calls);
    // N spins without the answer, the clock standing still: the pacer is never due
    for (uint64_t n : {1, 255, 256, 257, 1000}) {
        FakeClock::reset();
        uint64_t sides = 0;
        x = run({}, at(n + 1), nullptr, [&](const Run&) { ++sides; return false; });
        CHECK(x.r == WaitResult::ready && x.steps == n + 1 && x.q.calls == 0, "N=%llu: %s, %llu steps, %u queries",
              (unsigned long long)n, name(x.r), (unsigned long long)x.steps, x.q.calls);
        CHECK(sides == n / 256 && x.sides == sides, "N=%llu: %llu side checks", (unsigned long long)n,
              (unsigned long long)sides);
    }
    // the pause between spins changes nothing else
    FakeClock::reset();
    x = run({kRun}, at(300), [](uint64_t) { FakeClock::advance(microseconds(20)); }, nullptr, nullptr, WaitPause::yes);
    CHECK(x.r == WaitResult::ready && x.steps == 300 && x.q.calls == 1, "paused: %s, %llu steps, %u queries", name(x.r),
          (unsigned long long)x.steps, x.q.calls);
}

void beat_cases() {
    // 20 us per spin: the pacer is due at every beat, so one query per 256 spins
    FakeClock::reset();
    Run x = run({kRun, kRun, kRun, kRun}, at(1025), [](uint64_t) { FakeClock::advance(microseconds(20)); });
    CHECK(x.r == WaitResult::ready && x.steps == 1025 && x.q.calls == 4, "20 us a spin: %s, %llu steps, %u queries",
          name(x.r), (unsigned long long)x.steps, x.q.calls);
    // 10 us per beat: the first query no sooner than 20 us in, then every 20 us
    FakeClock::reset();
    x = run({kRun, kRun}, at(1025), [](uint64_t s) { if ((s & 255) == 0) FakeClock::advance(microseconds(10)); });
    CHECK(x.r == WaitResult::ready && x.q.calls == 2, "10 us a beat: %s, %u queries", name(x.r), x.q.calls);
    // one tick short of the period at the first beat: not due
    FakeClock::reset();
    x = run({kRun}, at(600), [](uint64_t s) {
        if (s == 256) FakeClock::advance(microseconds(20) - FakeClock::duration(1));
        if (s == 512) FakeClock::advance(FakeClock::duration(1));
    });
    CHECK(x.r == WaitResult::ready && x.q.calls == 1 && x.q.steps_at_last_call == 512, "pacer edge: %s, %u queries at %llu",
          name(x.r), x.q.calls, (unsigned long long)x.q.steps_at_last_call);
    // the side check on spin 256 comes before any query
    FakeClock::reset();
    x = run({}, at(5000), [](uint64_t) { FakeClock::advance(microseconds(20)); }, [](const Run&) { return true; });
    CHECK(x.r == WaitResult::abandoned && x.steps == 256 && x.sides == 1 && x.q.calls == 0,
          "side check: %s, %llu steps, %llu checks, %u queries", name(x.r), (unsigned long long)x.steps,
          (unsigned long long)x.sides, x.q.calls);
    // ... and on every beat, due or not, until it fires
    FakeClock::reset();
    x = run({}, at(5000), nullptr, [](const Run& r) { return r.sides == 3; });
    CHECK(x.r == WaitResult::abandoned && x.steps == 768 && x.q.calls == 0, "third side check: %s, %llu steps", name(x.r),
          (unsigned long long)x.steps);
}

void stream_cases() {
    const auto tick = [](uint64_t) { FakeClock::advance(microseconds(20)); };
    // finished, and the last look finds the answer
    FakeClock::reset();
    Run x = run({kFin}, [](uint64_t, const Run& r) { return r.q.calls > 0; }, tick);
    CHECK(x.r == WaitResult::ready && x.steps == 257 && x.q.calls == 1, "finished, answer in: %s, %llu steps", name(x.r),
          (unsigned long long)x.steps);
    // finished without it: gone, after exactly one more step
    FakeClock::reset();
    x = run({kRun, kFin}, at(5000), tick);
    CHECK(x.r == WaitResult::gone && x.q.calls == 2 && x.q.steps_at_last_call == 512 && x.steps == 513,
          "finished, no answer: %s, %u queries, %llu steps before and %llu after", name(x.r), x.q.calls,
          (unsigned long long)x.q.steps_at_last_call, (unsigned long long)x.steps);
    // failed: no further step, and what the callable kept is as it left it
    FakeClock::reset();
    x = run({kRun, kRun, kFail}, at(5000), tick);
    CHECK(x.r == WaitResult::failed && x.q.calls == 3 && x.steps == 768 && x.q.stored == 703,
          "failed: %s, %u queries, %llu steps, stored %d", name(x.r), x.q.calls, (unsigned long long)x.steps, x.q.stored);
}

void bound_cases() {
    // exactly at the bound on the querying spin: not late (strict >)
    for (const auto limit : {FakeClock::duration(seconds(10)), FakeClock::duration(seconds(2))}) {
        FakeClock::reset();
        WaitBound<FakeClock> b{FakeClock::now(), limit};
        Run x = run({kRun}, at(700), [&](uint64_t s) { if (s == 256) FakeClock::t = b.start + limit; }, nullptr, &b);
        CHECK(x.r == WaitResult::ready && x.q.calls == 1 && x.steps == 700, "at the bound: %s, %u queries", name(x.r),
              x.q.calls);
        // one tick past it: late, on that spin
        FakeClock::reset();
        b.start = FakeClock::now();
        x = run({kRun}, at(700), [&](uint64_t s) { if (s == 256) FakeClock::t = b.start + limit + FakeClock::duration(1); },
                nullptr, &b);
        CHECK(x.r == WaitResult::late && x.q.calls == 1 && x.steps == 256, "a tick past: %s, %u queries, %llu steps",
              name(x.r), x.q.calls, (unsigned long long)x.steps);
    }
    // past the bound between beats: seen on the next spin that queries, not before
    FakeClock::reset();
    WaitBound<FakeClock> b{FakeClock::now(), seconds(10)};
    Run x = run({kRun}, at(5000), [](uint64_t s) { if (s == 257) FakeClock::advance(seconds(11)); }, nullptr, &b);
    CHECK(x.r == WaitResult::late && x.q.calls == 1 && x.steps == 512, "late between beats: %s, %llu steps", name(x.r),
          (unsigned long long)x.steps);
    // ... and an answer that comes before that spin is ready, however late
    FakeClock::reset();
    b.start = FakeClock::now();
    x = run({}, at(255), [](uint64_t s) { if (s == 1) FakeClock::advance(seconds(11)); }, nullptr, &b);
    CHECK(x.r == WaitResult::ready && x.q.calls == 0, "late but answered: %s", name(x.r));
    // a bound that began long ago (svc_wait_ready's start is the launch), the
    // pacer not due: no query, so not late
    FakeClock::reset();
    b.start = FakeClock::now() - seconds(11);
    x = run({}, at(1000), nullptr, nullptr, &b);
    CHECK(x.r == WaitResult::ready && x.q.calls == 0 && x.steps == 1000, "old bound, no query: %s", name(x.r));
    // a finished or failed stream is that, not late
    FakeClock::reset();
    b.start = FakeClock::now() - seconds(11);
    x = run({kFin}, at(5000), [](uint64_t) { FakeClock::advance(microseconds(20)); }, nullptr, &b);
    CHECK(x.r == WaitResult::gone, "finished past the bound: %s", name(x.r));
    FakeClock::reset();
    x = run({kFail}, at(5000), [](uint64_t) { FakeClock::advance(microseconds(20)); }, nullptr, &b);
    CHECK(x.r == WaitResult::failed, "failed past the bound: %s", name(x.r));
    // no bound: never late, however far the clock runs
    FakeClock::reset();
    x = run(std::vector<StreamState>(7, kRun), at(2000), [](uint64_t) { FakeClock::advance(std::chrono::hours(1)); });
    CHECK(x.r == WaitResult::ready && x.q.calls == 7 && x.steps == 2000, "unbounded: %s, %u queries", name(x.r), x.q.calls);
}
}  // namespace

int main() {
    ready_cases();
    beat_cases();
    stream_cases();
    bound_cases();
    if (failures) {
        std::printf("wait_check: %d case(s) FAILED\n", failures);
        return 1;
    }
    std::printf("wait_check: ok\n");
    return 0;
}
