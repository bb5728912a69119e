// jsp_lines.h -- the bitmap answer's lines on the host: pure
// functions of host memory, no HIP and nothing of the engine, so that the
// stand-alone programs under tools/ (lines_bench, lines_check) compile them
// alone. A line is 8 words: tile t's 256 leaf bits as four 64-bit words, each
// stored as two halves (seq << 32 | 32 bits), low half first.
#ifndef JSP_LINES_H
#define JSP_LINES_H

#include <algorithm>
#include <cstdint>
#include <cstring>

constexpr uint32_t kPrefetchAhead = 8;  // answer lines in flight ahead of the one expanded

// The expansion itself, a pure host function of the lines (svc_wait_bits as
// they arrive, the host lease over the lines of the last answer,
// jspb_expand_lines): from tile *t and job *j on, every line whose 8 halves
// carry seq is expanded into out[] until J jobs have a leaf or the lines run
// out; a line with any other tag stops it, with nothing of that line written.
// true: the answer is complete (out[*j..J) is the caller's to fill with -1).
// on_line0 runs when tile 0's line is found whole.
template <class F>
inline bool expand_lines(const unsigned long long* b, uint32_t n, const uint32_t* l0, uint32_t base, uint32_t seq,
                         uint32_t J, int32_t* out, uint32_t* tp, uint32_t* jp, F&& on_line0) {
    uint32_t t = *tp, j = *jp;
    while (t < n && j < J) {
        const unsigned long long* L = b + 8u * t;
        unsigned long long x[8];
        uint32_t bad = 0;
        for (int k = 0; k < 8; ++k) {
            x[k] = __atomic_load_n(L + k, __ATOMIC_ACQUIRE);
            bad |= (uint32_t)(x[k] >> 32) ^ seq;
        }
        if (bad) break;
        if (t == 0) on_line0();
        // the tiles answer within ~0.1 us of each other: once a line is in,
        // the next ones have landed too (and the copies the spin's
        // prefetches brought in before they landed are gone). Keep the
        // lines kPrefetchAhead ahead in flight while this one is expanded.
        if (t == 0)
            for (uint32_t u = 1; u < n && u <= kPrefetchAhead; ++u) __builtin_prefetch(b + 8u * u, 0, 3);
        else if (t + kPrefetchAhead < n)
            __builtin_prefetch(b + 8u * (t + kPrefetchAhead), 0, 3);
        const uint32_t d0 = base + l0[t];
        for (uint32_t w = 0; w < 4 && j < J; ++w) {
            // run by run: feasible leaves come in long runs (a word of 64
            // is the common case), each written by a loop that vectorizes
            uint64_t m = (x[2 * w] & 0xFFFFFFFFull) | (x[2 * w + 1] << 32);
            const int32_t dw = (int32_t)(d0 + 64u * w);
            while (m != 0ull && j < J) {
                const uint32_t s0 = (uint32_t)__builtin_ctzll(m);
                const uint64_t sh = m >> s0;
                const uint32_t r = ~sh == 0ull ? 64u - s0 : (uint32_t)__builtin_ctzll(~sh);
                const uint32_t take = std::min(r, J - j);
                int32_t* o = out + j;
                const int32_t d = dw + (int32_t)s0;
                for (uint32_t k = 0; k < take; ++k) o[k] = d + (int32_t)k;
                j += take;
                m = s0 + r >= 64u ? 0ull : m & (~0ull << (s0 + r));
            }
        }
        ++t;
    }
    *tp = t;
    *jp = j;
    return t == n || j == J;
}

// Whether all 8 * n_lines halves of the first n_lines lines carry seq: one
// OR-reduce over the words, no branch inside (the compiler vectorizes it).
// The lease's kept list is checked with it on every answer: a line the
// device rewrote since the list was built has another tag.
inline bool lines_tagged(const unsigned long long* b, uint32_t n_lines, uint32_t seq) {
    const size_t n = 8u * (size_t)n_lines;
    uint32_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad |= (uint32_t)(b[i] >> 32) ^ seq;
    return bad == 0;
}

// The answer for J jobs from a kept list of feasible leaves (in answer
// order): the first min(J, n_list) of them, then -1. Writes out[0..J) and
// nothing behind it.
inline void list_answer(const int32_t* list, uint32_t n_list, uint32_t J, int32_t* out, uint32_t* placed) {
    const uint32_t n = std::min(J, n_list);
    if (n > 0) std::memcpy(out, list, (size_t)n * 4);
    for (uint32_t i = n; i < J; ++i) out[i] = -1;
    *placed = n;
}

#endif  // JSP_LINES_H
