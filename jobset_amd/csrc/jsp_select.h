// jsp_select.h -- the timing loops' two order statistics without a full sort
// (timed_calls, jspb_assume_forget_loop): the median and the p99 of per-call
// durations kept as integer nanoseconds. No HIP and nothing of the engine
// (tools/select_bench.cc times it alone).
//
// Samples below kSelectTable ns are counted into a table, the others go to a
// vector that is sorted, and the two ranks are read off the table's running
// sum. A loop of leased answers (0.1 us calls, a handful of outliers) sorts
// next to nothing; a loop of 34 us steps sorts everything, as before.
// The selected nanoseconds become microseconds by the same conversion
// us_between applies to a difference of two stamps, so the results are
// bit-identical to sorting the converted samples.
#ifndef JSP_SELECT_H
#define JSP_SELECT_H

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int64_t kSelectTable = 16384;

inline double ns_to_us(int64_t ns) {
    return std::chrono::duration<double, std::micro>(std::chrono::nanoseconds(ns)).count();
}

// The sample of each (ascending, 0-based) rank. Count: the table's counters,
// wide enough for n.
template <class Count>
inline void select_ranks_counted(const int64_t* ns, size_t n, const size_t* rank, size_t n_ranks, int64_t* out) {
    std::vector<Count> table((size_t)kSelectTable, (Count)0);
    std::vector<int64_t> over;
    bool negative = false;
    int64_t lo = kSelectTable, hi = -1;
    for (size_t i = 0; i < n; ++i) {
        const int64_t v = ns[i];
        if ((uint64_t)v < (uint64_t)kSelectTable) {
            table[(size_t)v] += 1;
            lo = std::min(lo, v);
            hi = std::max(hi, v);
        } else {
            negative |= v < 0;
            over.push_back(v);
        }
    }
    if (negative) {  // (no steady clock gives one: plainly sorted)
        std::vector<int64_t> all(ns, ns + n);
        std::sort(all.begin(), all.end());
        for (size_t r = 0; r < n_ranks; ++r) out[r] = all[rank[r]];
        return;
    }
    std::sort(over.begin(), over.end());
    const size_t in_table = n - over.size();
    for (size_t r = 0; r < n_ranks; ++r) {
        if (rank[r] >= in_table) {
            out[r] = over[rank[r] - in_table];
            continue;
        }
        size_t seen = 0;
        int64_t v = lo;
        for (; v <= hi; ++v) {
            seen += table[(size_t)v];
            if (seen > rank[r]) break;
        }
        out[r] = v;
    }
}

// (a few samples -- the driver's 20 steps: sorting them costs less than the
// table's 32 KiB; up to 65,535 the table counts in 16 bits)
inline void select_ranks(const int64_t* ns, size_t n, const size_t* rank, size_t n_ranks, int64_t* out) {
    if (n <= 256) {
        int64_t all[256];
        std::copy(ns, ns + n, all);
        std::sort(all, all + n);
        for (size_t r = 0; r < n_ranks; ++r) out[r] = all[rank[r]];
    } else if (n <= 65535) {
        select_ranks_counted<uint16_t>(ns, n, rank, n_ranks, out);
    } else {
        select_ranks_counted<uint32_t>(ns, n, rank, n_ranks, out);
    }
}

// out[0] the median (rank n / 2) and out[1] the p99 (rank min(n - 1,
// (size_t)(0.99 n))) of n >= 1 samples, in microseconds.
inline void select_median_p99(const int64_t* ns, size_t n, double* out) {
    const size_t rank[2] = {n / 2, std::min<size_t>(n - 1, (size_t)(0.99 * n))};
    int64_t v[2];
    select_ranks(ns, n, rank, 2, v);
    out[0] = ns_to_us(v[0]);
    out[1] = ns_to_us(v[1]);
}

#endif  // JSP_SELECT_H
