// lines_check -- the CPU cases of tests/test_lines_memo.py in C++, for the
// AddressSanitizer + UBSan build (make lines-asan): every output buffer is
// allocated at exactly J ints, so a store past out[J - 1] is caught. Includes
// jobset_amd/csrc/jsp_lines.h alone: no GPU, no engine. Exit status 0 and
// "lines_check: ok" when every case holds.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "../jobset_amd/csrc/jsp_lines.h"

namespace {
constexpr uint32_t kSeq = 0x1234567u, kBase = 7;
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

struct Rng {
    uint64_t s;
    double next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) / (double)(1ull << 53);
    }
};

using Bits = std::vector<std::vector<bool>>;  // [tiles][256]

std::vector<unsigned long long> pack(const Bits& bits, uint32_t seq = kSeq) {
    std::vector<unsigned long long> w(8 * bits.size(), (unsigned long long)seq << 32);
    for (size_t t = 0; t < bits.size(); ++t)
        for (uint32_t i = 0; i < 256; ++i)
            if (bits[t][i]) w[8 * t + i / 32] |= 1ull << (i % 32);
    return w;
}

std::vector<std::pair<std::string, Bits>> patterns(uint32_t n) {
    Rng rng{100 + n};
    const Bits zeros(n, std::vector<bool>(256, false));
    Bits ones(n, std::vector<bool>(256, true)), bit0 = zeros, bit63 = zeros, runs = zeros, racks = zeros,
                                                 random = zeros, sparse = zeros;
    for (uint32_t t = 0; t < n; ++t) {
        bit0[t][0] = true;
        bit63[t][63] = true;
        for (auto ab : {std::pair<int, int>{20, 45}, {50, 80}, {120, 200}, {250, 256}})
            for (int i = ab.first; i < ab.second; ++i) runs[t][i] = true;
        if (t % 2 == 0) runs[t][31] = runs[t][32] = true;
        for (uint32_t i = 0; i < 68; ++i) racks[t][i] = rng.next() > 0.03;
        for (uint32_t i = 0; i < 256; ++i) {
            random[t][i] = rng.next() > 0.5;
            sparse[t][i] = rng.next() > 0.97;
        }
    }
    bit63[n - 1][255] = true;
    return {{"ones", ones}, {"zeros", zeros}, {"bit0", bit0}, {"bit63", bit63},
            {"runs", runs}, {"racks", racks}, {"random", random}, {"sparse", sparse}};
}

// expand_lines into a buffer of exactly J ints, with the -1 tail; nullptr when not whole
std::unique_ptr<int32_t[]> expand(const std::vector<unsigned long long>& lines, const std::vector<uint32_t>& l0,
                                  uint32_t J, uint32_t* placed) {
    std::unique_ptr<int32_t[]> out(new int32_t[J]);
    uint32_t t = 0, j = 0;
    const bool whole = expand_lines(lines.data(), (uint32_t)l0.size(), l0.data(), kBase, kSeq, J, out.get(), &t, &j, [] {});
    *placed = j;
    if (!whole) return nullptr;
    for (uint32_t i = j; i < J; ++i) out[i] = -1;
    return out;
}

bool same_answer(const int32_t* list, uint32_t n_list, const std::vector<unsigned long long>& lines,
                 const std::vector<uint32_t>& l0, uint32_t J, uint32_t want_placed) {
    uint32_t fresh_placed = 0, placed = ~0u;
    const auto fresh = expand(lines, l0, J, &fresh_placed);
    std::unique_ptr<int32_t[]> got(new int32_t[J]);
    list_answer(list, n_list, J, got.get(), &placed);
    if (!fresh || placed != fresh_placed || placed != want_placed) return false;
    for (uint32_t i = 0; i < J; ++i)
        if (got[i] != fresh[i]) return false;
    return true;
}
}  // namespace

int main() {
    for (uint32_t n : {1u, 2u, 8u, 9u, 15u}) {
        for (const auto& [name, bits] : patterns(n)) {
            std::vector<uint32_t> l0(n);
            uint32_t nF = 0;
            for (uint32_t t = 0; t < n; ++t) {
                l0[t] = t * (name == "racks" ? 68u : 256u);
                for (uint32_t i = 0; i < 256; ++i) nF += bits[t][i] ? 1u : 0u;
            }
            const auto lines = pack(bits);
            // the whole list, then every J of the issue's set
            uint32_t n_list = 0;
            const auto list = expand(lines, l0, 256 * n, &n_list);
            CHECK(list && n_list == nF, "%s n=%u", name.c_str(), n);
            if (!list) continue;
            for (uint32_t J : std::set<uint32_t>{1, nF - 1, nF, nF + 1, 256 * n}) {
                if (J < 1 || J > 256 * n + 1) continue;  // (nF - 1 wrapped for nF = 0)
                CHECK(same_answer(list.get(), n_list, lines, l0, J, std::min(J, nF)), "%s n=%u J=%u", name.c_str(), n, J);
            }
            // a list built for J_b < nF jobs answers every J <= J_b
            for (uint32_t J_b : std::set<uint32_t>{1, nF / 2, nF - 1}) {
                if (J_b < 1 || J_b >= nF) continue;
                uint32_t nb = 0;
                const auto shortlist = expand(lines, l0, J_b, &nb);
                CHECK(shortlist && nb == J_b, "%s n=%u J_b=%u", name.c_str(), n, J_b);
                if (!shortlist) continue;
                for (uint32_t J : std::set<uint32_t>{1, std::max(J_b / 2, 1u), std::max(J_b - 1, 1u), J_b})
                    CHECK(same_answer(shortlist.get(), nb, lines, l0, J, J), "%s n=%u J_b=%u J=%u", name.c_str(), n,
                          J_b, J);
            }
            // the tag check: whole lines, every single half retagged, a prefix of the lines
            if (name != "racks" || (n != 1 && n != 15)) continue;
            // the lines in a buffer of exactly 8 n words: a read past them is caught
            std::unique_ptr<unsigned long long[]> b(new unsigned long long[8 * n]);
            std::copy(lines.begin(), lines.end(), b.get());
            CHECK(lines_tagged(b.get(), n, kSeq), "n=%u", n);
            CHECK(!lines_tagged(b.get(), n, kSeq + 1), "n=%u", n);
            CHECK(lines_tagged(b.get(), 0, kSeq), "n=%u", n);
            for (uint32_t h = 0; h < 8 * n; ++h) {
                for (uint32_t other : {kSeq + 1, kSeq ^ 0x80000000u, 0u}) {
                    const unsigned long long keep = b[h];
                    b[h] = ((unsigned long long)other << 32) | (keep & 0xFFFFFFFFull);
                    CHECK(!lines_tagged(b.get(), n, kSeq), "n=%u half %u", n, h);
                    for (uint32_t k : {0u, h / 8, h / 8 + 1, n})
                        CHECK(lines_tagged(b.get(), k, kSeq) == (k <= h / 8), "n=%u half %u k=%u", n, h, k);
                    b[h] = keep;
                }
            }
        }
    }
    // no list, no jobs
    {
        uint32_t placed = ~0u;
        std::unique_ptr<int32_t[]> out(new int32_t[3]);
        list_answer(nullptr, 0, 3, out.get(), &placed);
        CHECK(placed == 0 && out[0] == -1 && out[1] == -1 && out[2] == -1, "empty list");
        std::unique_ptr<int32_t[]> none(new int32_t[0]);
        const int32_t five[5] = {1, 2, 3, 4, 5};
        list_answer(five, 5, 0, none.get(), &placed);
        CHECK(placed == 0, "no jobs");
    }
    if (failures) std::printf("lines_check: %d FAILED\n", failures);
    else std::printf("lines_check: ok\n");
    return failures ? 1 : 0;
}
