// lines_bench -- the host's three line functions (jobset_amd/csrc/jsp_lines.h)
// timed alone on cfg2's line shape: 1,000 racks in 15 tiles of at most 68, ten
// racks infeasible, 990 jobs. expand_lines decodes the lines into the answer
// (what every host answer under the lease did), lines_tagged + list_answer are
// what an answer from the kept list does (DESIGN.md §4.3 "the kept list").
// A stand-alone CPU program: no GPU, no engine. Usage: lines_bench [calls]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../jobset_amd/csrc/jsp_lines.h"

namespace {
using clk = std::chrono::steady_clock;

template <class F>
double ns_per_call(uint32_t calls, F&& f) {
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
        const auto t0 = clk::now();
        for (uint32_t i = 0; i < calls; ++i) f();
        best = std::min(best, std::chrono::duration<double, std::nano>(clk::now() - t0).count() / calls);
    }
    return best;
}
}  // namespace

int main(int argc, char** argv) {
    const uint32_t calls = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 0) : 200000u;
    const uint32_t racks = 1000, per_tile = 68, n = (racks + per_tile - 1) / per_tile, seq = 0x1234567u, J = 990;
    std::vector<unsigned long long> lines(8u * n, (unsigned long long)seq << 32);
    std::vector<uint32_t> l0(n);
    uint32_t nF = 0;
    for (uint32_t r = 0; r < racks; ++r) {
        const uint32_t t = r / per_tile, bit = r % per_tile;
        l0[t] = t * per_tile;
        if (r % 100 == 37) continue;  // ten infeasible racks, spread as cfg2's
        lines[8u * t + bit / 32] |= 1ull << (bit % 32);
        ++nF;
    }
    std::vector<int32_t> out(J), out2(J), list(256u * n);
    uint32_t t = 0, j = 0;
    if (!expand_lines(lines.data(), n, l0.data(), 0, seq, 256u * n, list.data(), &t, &j, [] {}) || j != nF) return 1;
    const uint32_t n_list = j;
    volatile uint32_t sink = 0;
    const double ns_expand = ns_per_call(calls, [&] {
        uint32_t tt = 0, jj = 0;
        (void)expand_lines(lines.data(), n, l0.data(), 0, seq, J, out.data(), &tt, &jj, [] {});
        for (uint32_t i = jj; i < J; ++i) out[i] = -1;
        sink = sink + (uint32_t)out[jj - 1];
        __asm__ volatile("" ::: "memory");
    });
    const double ns_tag = ns_per_call(calls, [&] {
        sink = sink + (lines_tagged(lines.data(), n, seq) ? 1u : 0u);
        __asm__ volatile("" ::: "memory");
    });
    const double ns_copy = ns_per_call(calls, [&] {
        uint32_t placed = 0;
        list_answer(list.data(), n_list, J, out2.data(), &placed);
        sink = sink + placed;
        __asm__ volatile("" ::: "memory");
    });
    const double ns_clock = ns_per_call(calls, [&] { sink = sink + (uint32_t)clk::now().time_since_epoch().count(); });
    const bool same = out == out2;
    std::printf("lines_bench: %u tiles, %u feasible leaves, J = %u, %u calls (best of 5 runs)\n", n, nF, J, calls);
    std::printf("expand_lines %.1f ns | lines_tagged %.1f ns | list_answer %.1f ns | tagged + answer %.1f ns | "
                "steady_clock read %.1f ns | outputs %s\n",
                ns_expand, ns_tag, ns_copy, ns_tag + ns_copy, ns_clock, same ? "identical" : "DIFFER");
    return same ? 0 : 1;
}
