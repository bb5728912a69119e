// select_bench -- the timing loops' median / p99 selection (jsp_select.h)
// against the std::sort of the converted samples it replaces, stand-alone on
// the CPU, on samples shaped like a loop of leased jsp_place answers: ties at
// 120 / 130 ns (the clock's 10 ns steps), 0.5 % outliers of 1..30 us. Prints
// both at n = 20 (the driver's flags) and n = 2,000 (the bench's default), and
// checks the two give the same bits.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../jobset_amd/csrc/jsp_select.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

static std::vector<int64_t> leased_samples(size_t n) {
    std::vector<int64_t> ns(n);
    for (auto& v : ns) {
        const uint64_t r = rnd();
        v = r % 200 == 0 ? 1000 + (int64_t)((r >> 16) % 29000) : r % 3 == 0 ? 130 : 120;
    }
    return ns;
}

static void sorted_median_p99(const std::vector<int64_t>& ns, double* out) {
    std::vector<double> us(ns.size());
    for (size_t i = 0; i < ns.size(); ++i) us[i] = ns_to_us(ns[i]);
    const auto t0 = std::chrono::steady_clock::now();
    std::sort(us.begin(), us.end());
    out[0] = us[us.size() / 2];
    out[1] = us[std::min<size_t>(us.size() - 1, (size_t)(0.99 * us.size()))];
    out[2] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

int main() {
    int bad = 0;
    for (size_t n : {(size_t)20, (size_t)2000}) {
        const int reps = 2000;
        double t_sort = 0.0, t_sel = 0.0;
        for (int r = 0; r < reps; ++r) {
            const std::vector<int64_t> ns = leased_samples(n);
            double a[3], b[2];
            sorted_median_p99(ns, a);
            const auto t0 = std::chrono::steady_clock::now();
            select_median_p99(ns.data(), ns.size(), b);
            t_sel += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            t_sort += a[2];
            if (std::memcmp(a, b, 2 * sizeof(double)) != 0) {
                std::fprintf(stderr, "n=%zu rep %d: sort %.17g %.17g, selection %.17g %.17g\n", n, r, a[0], a[1], b[0], b[1]);
                bad = 1;
            }
        }
        std::printf("n=%zu: std::sort %.3f us, selection %.3f us (%.1fx), mean of %d\n", n, t_sort / reps, t_sel / reps,
                    t_sort / t_sel, reps);
    }
    return bad;
}
