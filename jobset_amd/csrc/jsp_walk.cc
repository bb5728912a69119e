// jsp_walk.cc — host half of the split placement service (jsp_walk.h).
//
// Feasibility: a leaf-level class's domain (leaf) is feasible
// when its capacity covers the job's pods and no foreign exclusive job covers
// one of its rows: the tiles' ballots give the first, the group-0 tiles'
// occupancy ballots the second. An upper-level class's domain is feasible
// when the sum over its leaves of min(cap, pods) reaches pods (the tiles'
// clamped partial sums per domain, added here) and none of its leaves is
// occupied. The walk is the lowest-index rule of oracle/cpu_ref.c: jobs in
// global order, each takes the lowest feasible domain at its class's level
// not yet taken; taking a domain takes its ancestors and descendants.
#include "jsp_walk.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <functional>
#include <utility>

namespace jsp {

namespace {

inline void set_range(uint64_t* t, uint32_t lo, uint32_t hi) {
    while (lo < hi) {
        const uint32_t w = lo >> 6, b = lo & 63u;
        const uint32_t n = (hi - lo) < (64u - b) ? (hi - lo) : (64u - b);
        t[w] |= (n == 64u) ? ~0ull : (((1ull << n) - 1ull) << b);
        lo += n;
    }
}

// any bit of g in [lo, hi)
inline bool any_bits(const uint64_t* g, uint32_t lo, uint32_t hi) {
    while (lo < hi) {
        const uint32_t w = lo >> 6, b = lo & 63u;
        const uint32_t n = (hi - lo) < (64u - b) ? (hi - lo) : (64u - b);
        const uint64_t m = (n == 64u) ? ~0ull : (((1ull << n) - 1ull) << b);
        if (g[w] & m) return true;
        lo += n;
    }
    return false;
}

}  // namespace

void HostWalk::set_topology(uint32_t K, const uint32_t* D, const std::vector<uint32_t>* fl,
                            const std::vector<uint32_t>* cs, const std::vector<int32_t>* par) {
    K_ = K;
    uint32_t off = 0;
    toff_.assign(K + 1, 0);
    for (uint32_t k = 0; k < kMaxLevels; ++k) {
        D_[k] = k < K ? D[k] : 0;
        fl_[k] = k < K ? fl[k] : std::vector<uint32_t>();
        cs_[k] = k + 1 < K ? cs[k] : std::vector<uint32_t>();
        par_[k] = k >= 1 && k < K ? par[k] : std::vector<int32_t>();
        if (k < K) {
            toff_[k] = off;
            off += (D_[k] + 63) / 64;
        }
    }
    toff_[K] = off;
    L_ = D_[K - 1];
    taken_.assign(off + 1, 0);
    occ_lvl_.assign(off + 1, 0);
    occ_.assign((L_ + 63) / 64 + 1, 0);
}

void HostWalk::set_classes(const std::vector<DevClass>& cls) {
    C_ = (uint32_t)cls.size();
    level_.resize(C_);
    pods_.resize(C_);
    woff_.assign(C_ + 1, 0);
    uoff_.assign(C_ + 1, 0);
    any_upper_ = false;
    for (uint32_t c = 0; c < C_; ++c) {
        level_[c] = cls[c].level;
        pods_[c] = cls[c].pods;
        const uint32_t D = D_[level_[c]];
        woff_[c + 1] = woff_[c] + (D + 63) / 64;
        const bool upper = level_[c] + 1 < K_;
        uoff_[c + 1] = uoff_[c] + (upper ? D : 0u);
        any_upper_ |= upper;
    }
    feas_.assign(woff_[C_] + 1, 0);
    sums_.assign(uoff_[C_] + 1, 0);
    cw_.assign(C_, ClassWalk{});
}

void HostWalk::set_tiles(const std::vector<uint32_t>& blk_l0, const std::vector<uint32_t>& blk_l1, uint32_t groups,
                         uint32_t cpg) {
    l0_ = blk_l0;
    l1_ = blk_l1;
    groups_ = groups;
    cpg_ = cpg;
    nw_ = split_waves(blk_l0, blk_l1);
}

uint32_t split_waves(const std::vector<uint32_t>& blk_l0, const std::vector<uint32_t>& blk_l1) {
    uint32_t m = 1;
    for (size_t b = 0; b < blk_l0.size() && b < blk_l1.size(); ++b) m = std::max(m, blk_l1[b] - blk_l0[b]);
    return std::min<uint32_t>((m + 63) / 64, 4u);
}

void HostWalk::prefetch_tile(const uint64_t* slots, uint32_t t) const {
    const uint32_t b = t / groups_;
    if (b >= l0_.size()) return;
    const uint64_t* s = slots + (size_t)t * split_tile_words(cpg_, nw_);
    const uint32_t n_line = split_line_words(cpg_, nw_);
    for (uint32_t i = 0; i < n_line; i += 8) __builtin_prefetch(s + i, 0, 3);
    if (!any_upper_) return;
    const uint32_t nl = l1_[b] - l0_[b], g = t % groups_;
    for (uint32_t j = 0; j < cpg_; ++j) {
        const uint32_t c = g * cpg_ + j;
        if (c >= C_ || level_[c] + 1 == K_) continue;
        for (uint32_t w = 0; 64 * w < nl; ++w)
            __builtin_prefetch(s + n_line + ((size_t)j * nw_ + w) * kSplitRecs, 0, 3);
    }
}

bool HostWalk::tile_ready(const uint64_t* slots, uint32_t t, uint32_t seq) const {
    const uint64_t* s = slots + (size_t)t * split_tile_words(cpg_, nw_);
    const uint32_t n_line = split_line_words(cpg_, nw_);
    uint32_t bad = 0;
    for (uint32_t i = 0; i < n_line; ++i) bad |= (uint32_t)(__atomic_load_n(s + i, __ATOMIC_ACQUIRE) >> 32) ^ seq;
    if (bad) return false;
    if (!any_upper_) return true;
    const uint32_t b = t / groups_, g = t % groups_;
    const uint32_t nl = l1_[b] - l0_[b];
    const uint64_t rtag = split_rec_tag(seq);
    for (uint32_t j = 0; j < cpg_; ++j) {
        const uint32_t c = g * cpg_ + j;
        if (c >= C_ || level_[c] + 1 == K_) continue;
        for (uint32_t w = 0; 64 * w < nl; ++w) {
            const uint32_t n = std::min<uint32_t>((uint32_t)s[2 * (j * nw_ + w)], kSplitRecs);
            const uint64_t* r = s + n_line + ((size_t)j * nw_ + w) * kSplitRecs;
            for (uint32_t i = 0; i < n; ++i)
                if ((__atomic_load_n(r + i, __ATOMIC_ACQUIRE) >> 50) != rtag) return false;
        }
    }
    return true;
}

// A ballot word of a tile's lines: class slot j, wave w's halves (the low 32
// bits of entries 2 (j nw + w) and + 1).
static inline uint64_t line_word(const uint64_t* lines, uint32_t nw, uint32_t j, uint32_t w) {
    const uint64_t* p = lines + 2 * (j * nw + w);
    return (p[0] & 0xFFFFFFFFull) | (p[1] << 32);
}

// Bitmap words built from 64-bit pieces at nondecreasing bit positions (the
// tiles' ballots, in leaf order) into a zeroed bitmap: the two words a piece
// touches are kept in registers and written once they are passed, instead of
// a read-modify-write per piece (cfg3's 80 tiles: a store-to-load chain).
struct BitAppender {
    uint64_t* g;
    uint32_t w = 0;
    uint64_t a0 = 0, a1 = 0;
    explicit BitAppender(uint64_t* g_) : g(g_) {}
    inline void add(uint32_t pos, uint64_t x) {
        const uint32_t pw = pos >> 6, b = pos & 63u;
        if (pw != w) {
            g[w] |= a0;
            if (pw == w + 1) {
                a0 = a1;
            } else {
                g[w + 1] |= a1;
                a0 = 0;
            }
            a1 = 0;
            w = pw;
        }
        a0 |= x << b;
        if (b != 0) a1 |= x >> (64u - b);
    }
    inline void flush() {
        g[w] |= a0;
        g[w + 1] |= a1;
    }
};

void HostWalk::build_feasibility(const uint64_t* slots) {
    const size_t tile_words = split_tile_words(cpg_, nw_);
    const uint32_t n_line = split_line_words(cpg_, nw_);
    const uint32_t nb = (uint32_t)l0_.size();
    // occupied leaves, from the group-0 tiles
    std::fill(occ_.begin(), occ_.end(), 0ull);
    {
        BitAppender ap(occ_.data());
        for (uint32_t b = 0; b < nb; ++b) {
            const uint64_t* s = slots + (size_t)(b * groups_) * tile_words;
            const uint32_t nl = l1_[b] - l0_[b];
            for (uint32_t w = 0; 64 * w < nl; ++w) ap.add(l0_[b] + 64 * w, line_word(s, nw_, cpg_, w));
        }
        ap.flush();
    }
    // occupied domains above the leaves (only levels some class places at)
    if (any_upper_) {
        std::fill(occ_lvl_.begin(), occ_lvl_.end(), 0ull);
        for (uint32_t k = 0; k + 1 < K_; ++k) {
            bool used = false;
            for (uint32_t c = 0; c < C_ && !used; ++c) used = level_[c] == k;
            if (!used) continue;
            uint64_t* o = occ_lvl_.data() + toff_[k];
            const uint32_t* fl = fl_[k].data();
            for (uint32_t d = 0; d < D_[k]; ++d)
                if (any_bits(occ_.data(), fl[d], fl[d + 1])) o[d >> 6] |= 1ull << (d & 63);
        }
    }
    std::fill(feas_.begin(), feas_.end(), 0ull);
    for (uint32_t c = 0; c < C_; ++c) {
        const uint32_t g = c / cpg_, j = c % cpg_, k = level_[c], pods = pods_[c];
        uint64_t* F = feas_.data() + woff_[c];
        if (k + 1 == K_) {
            BitAppender ap(F);
            for (uint32_t b = 0; b < nb; ++b) {
                const uint64_t* s = slots + (size_t)(b * groups_ + g) * tile_words;
                const uint32_t nl = l1_[b] - l0_[b];
                for (uint32_t w = 0; 64 * w < nl; ++w) ap.add(l0_[b] + 64 * w, line_word(s, nw_, j, w));
            }
            ap.flush();
            const uint32_t nw = woff_[c + 1] - woff_[c];
            for (uint32_t w = 0; w < nw; ++w) F[w] &= ~occ_[w];
        } else {
            uint64_t* S = sums_.data() + uoff_[c];
            std::fill(S, S + D_[k], 0ull);
            for (uint32_t b = 0; b < nb; ++b) {
                const uint64_t* s = slots + (size_t)(b * groups_ + g) * tile_words;
                const uint32_t nl = l1_[b] - l0_[b];
                for (uint32_t w = 0; 64 * w < nl; ++w) {
                    const uint32_t n = std::min<uint32_t>((uint32_t)s[2u * (j * nw_ + w)], kSplitRecs);
                    const uint64_t* q = s + n_line + ((size_t)j * nw_ + w) * kSplitRecs;
                    for (uint32_t i = 0; i < n; ++i) {
                        const uint64_t r = q[i];
                        const uint32_t d = (uint32_t)(r >> 30) & (kSplitMaxDomains - 1u);
                        if (d < D_[k]) S[d] += (uint32_t)(r & 0x3FFFFFFFull);
                    }
                }
            }
            const uint64_t* O = occ_lvl_.data() + toff_[k];
            for (uint32_t d = 0; d < D_[k]; ++d)
                if (S[d] >= pods && !((O[d >> 6] >> (d & 63)) & 1ull)) F[d >> 6] |= 1ull << (d & 63);
        }
    }
}

// Taking domain d at level k (its own bit is set by the caller) takes its
// ancestors and its descendants at every other level.
// (the per-level table pointers are set up by walk(): raw pointers, not a
// vector lookup per level and job)
void HostWalk::take_marks(uint32_t d, uint32_t k) {
    if (k + 1 < K_ && lv_fl_[k][d] == lv_fl_[k][d + 1]) return;  // an empty domain intersects nothing
    uint32_t dd = d;
    for (int kk = (int)k - 1; kk >= 0; --kk) {
        dd = (uint32_t)lv_par_[kk + 1][dd];
        lv_t_[kk][dd >> 6] |= 1ull << (dd & 63);
    }
    uint32_t lo = d, hi = d + 1;
    for (uint32_t kk = k + 1; kk < K_; ++kk) {
        lo = lv_cs_[kk - 1][lo];
        hi = lv_cs_[kk - 1][hi];
        set_range(lv_t_[kk], lo, hi);
    }
}

uint32_t HostWalk::place(const uint64_t* slots, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                         int32_t* assign) {
    build_feasibility(slots);
    return walk(feas_.data(), run_class, run_len, n_runs, assign);
}

static inline void prefetch_vec(const void* p, size_t bytes) {
    const char* c = static_cast<const char*>(p);
    for (size_t i = 0; c && i < bytes; i += 64) __builtin_prefetch(c + i, 0, 3);
}

void HostWalk::prefetch_state() const {
    prefetch_vec(taken_.data(), taken_.size() * 8);
    prefetch_vec(feas_.data(), feas_.size() * 8);
    prefetch_vec(occ_.data(), occ_.size() * 8);
    prefetch_vec(sums_.data(), std::min<size_t>(sums_.size() * 8, 65536));
    prefetch_vec(cw_.data(), cw_.size() * sizeof(ClassWalk));
    prefetch_vec(level_.data(), level_.size() * 4);
    prefetch_vec(pods_.data(), pods_.size() * 4);
    prefetch_vec(woff_.data(), woff_.size() * 4);
    prefetch_vec(uoff_.data(), uoff_.size() * 4);
    prefetch_vec(l0_.data(), l0_.size() * 4);
    prefetch_vec(l1_.data(), l1_.size() * 4);
    for (uint32_t k = 0; k < K_; ++k) {
        prefetch_vec(fl_[k].data(), std::min<size_t>(fl_[k].size() * 4, 65536));
        prefetch_vec(cs_[k].data(), std::min<size_t>(cs_[k].size() * 4, 65536));
        prefetch_vec(par_[k].data(), std::min<size_t>(par_[k].size() * 4, 65536));
    }
}

uint32_t HostWalk::walk(const uint64_t* feas, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                        int32_t* assign) {
    std::fill(taken_.begin(), taken_.end(), 0ull);
    for (uint32_t k = 0; k < K_; ++k) {
        lv_t_[k] = taken_.data() + toff_[k];
        lv_fl_[k] = fl_[k].data();
        lv_cs_[k] = cs_[k].data();
        lv_par_[k] = par_[k].data();
    }
    // per class, everything a run needs in one record (cfg5: ~500 runs of one
    // job each, so the per-run set-up is most of the walk)
    cw_.resize(C_);
    for (uint32_t c = 0; c < C_; ++c) {
        const uint32_t k = level_[c];
        cw_[c] = ClassWalk{feas + woff_[c], taken_.data() + toff_[k], D_[k], (D_[k] + 63) / 64, k, 0u};
    }
    uint32_t placed = 0;
    size_t j = 0;
    const bool marks = K_ > 1;
    for (uint32_t r = 0; r < n_runs; ++r) {
        ClassWalk& cw = cw_[run_class[r]];
        const uint32_t n = run_len[r];
        uint32_t cur = cw.cursor, i = 0;
        if (cur < cw.D) {
            // The run's jobs take the free feasible bits in order. Taking a
            // domain marks other levels only (ancestors above, descendants
            // below), so at this level the only bits that change are the ones
            // the run itself takes: the current word's free bits are kept
            // across jobs and re-read only when a new word starts.
            const uint64_t* F = cw.F;
            uint64_t* T = cw.T;
            uint32_t w = cur >> 6;
            uint64_t bits = F[w] & ~T[w] & (~0ull << (cur & 63));
            for (; i < n; ++i) {
                while (bits == 0 && ++w < cw.nw) bits = F[w] & ~T[w];
                if (bits == 0) break;
                const uint32_t b = (uint32_t)__builtin_ctzll(bits);
                const uint32_t d = w * 64 + b;
                bits &= bits - 1;
                assign[j + i] = (int32_t)d;
                T[w] |= 1ull << b;
                if (marks) take_marks(d, cw.k);
                cur = d + 1;
            }
            placed += i;
            cw.cursor = i < n ? cw.D : cur;
        }
        for (; i < n; ++i) assign[j + i] = -1;
        j += n;
    }
    return placed;
}

// ---- the fit walk (DESIGN.md §2 "Fit placement") ----
uint32_t HostWalk::walk_fit(const uint32_t* order, const uint32_t* nf, const uint32_t* fit_off, const uint32_t* fitv,
                            const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, int32_t* assign,
                            uint64_t* slack) {
    std::fill(taken_.begin(), taken_.end(), 0ull);
    for (uint32_t k = 0; k < K_; ++k) {
        lv_t_[k] = taken_.data() + toff_[k];
        lv_fl_[k] = fl_[k].data();
        lv_cs_[k] = cs_[k].data();
        lv_par_[k] = par_[k].data();
    }
    cw_.resize(C_);
    for (uint32_t c = 0; c < C_; ++c) {
        const uint32_t k = level_[c];
        cw_[c] = ClassWalk{nullptr, taken_.data() + toff_[k], D_[k], (D_[k] + 63) / 64, k, 0u};
    }
    uint32_t placed = 0;
    uint64_t sl = 0;
    size_t j = 0;
    const bool marks = K_ > 1;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint32_t c = run_class[r];
        ClassWalk& cw = cw_[c];
        const uint32_t n = run_len[r], end = nf[c];
        const uint32_t* list = order + fit_off[c];
        uint64_t* T = cw.T;
        uint32_t cur = cw.cursor, i = 0;
        for (; i < n; ++i) {
            while (cur < end && ((T[list[cur] >> 6] >> (list[cur] & 63)) & 1ull)) ++cur;
            if (cur == end) break;
            const uint32_t d = list[cur++];
            assign[j + i] = (int32_t)d;
            T[d >> 6] |= 1ull << (d & 63);
            if (marks) take_marks(d, cw.k);
            if (fitv) sl += (uint64_t)fitv[fit_off[c] + d] - pods_[c];
        }
        placed += i;
        cw.cursor = cur;
        for (; i < n; ++i) assign[j + i] = -1;
        j += n;
    }
    if (slack) *slack = sl;
    return placed;
}

// ---- the gang walk (DESIGN.md §2 "Gang placement") ----
// Its state lives in a GangState the caller owns: HostWalk keeps the layout
// the placement path was measured with.
void HostWalk::gang_layout(GangState& st) const {
    st.doff.assign(K_ + 1, 0);
    for (uint32_t k = 0; k < K_; ++k) st.doff[k + 1] = st.doff[k] + D_[k];
    st.coff.assign(C_ + 1, 0);
    for (uint32_t c = 0; c < C_; ++c) st.coff[c + 1] = st.coff[c] + st.doff[level_[c] + 1];
}

// A trial's writes to the taken words go through mark_word, which keeps the
// old value of every word it changes: a failed trial puts them back in
// reverse order, a successful one drops the log.
inline void HostWalk::mark_word(GangState& st, uint64_t* p, uint64_t m) {
    const uint64_t old = *p;
    if ((old & m) == m) return;
    st.log.emplace_back(p, old);
    *p = old | m;
}

// take_marks with the log
void HostWalk::take_marks_logged(GangState& st, uint32_t d, uint32_t k) {
    if (k + 1 < K_ && lv_fl_[k][d] == lv_fl_[k][d + 1]) return;
    uint32_t dd = d;
    for (int kk = (int)k - 1; kk >= 0; --kk) {
        dd = (uint32_t)lv_par_[kk + 1][dd];
        mark_word(st, lv_t_[kk] + (dd >> 6), 1ull << (dd & 63));
    }
    uint32_t lo = d, hi = d + 1;
    for (uint32_t kk = k + 1; kk < K_; ++kk) {
        lo = lv_cs_[kk - 1][lo];
        hi = lv_cs_[kk - 1][hi];
        for (uint32_t a = lo; a < hi;) {
            const uint32_t w = a >> 6, b = a & 63u;
            const uint32_t n = (hi - a) < (64u - b) ? (hi - a) : (64u - b);
            mark_word(st, lv_t_[kk] + w, (n == 64u) ? ~0ull : (((1ull << n) - 1ull) << b));
            a += n;
        }
    }
}

// One trial of the gang whose runs are given, inside S at level s (any: the
// whole cluster). Its jobs in global order: each takes the lowest domain of
// its class's level inside S that is feasible, has leaves and is not taken.
// Within a trial the taken set only grows, so a class's cursor never goes back.
bool HostWalk::gang_trial(GangState& st, uint32_t S, bool any, uint32_t s, const uint32_t* run_class, const uint32_t* run_len,
                          uint32_t n_runs, int32_t* assign) {
    for (uint32_t c : st.cls) {
        const uint32_t k = level_[c];
        uint32_t lo = 0, hi = D_[k];
        if (!any) {
            lo = S;
            hi = S + 1;
            for (uint32_t kk = s; kk < k; ++kk) {
                lo = lv_cs_[kk][lo];
                hi = lv_cs_[kk][hi];
            }
        }
        st.lo[c] = lo;
        st.hi[c] = hi;
        st.cur[c] = lo;
    }
    st.log.clear();
    size_t j = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint32_t c = run_class[r], k = level_[c], hi = st.hi[c];
        const uint64_t* F = st.feas + woff_[c];
        uint64_t* T = lv_t_[k];
        for (uint32_t q = 0; q < run_len[r]; ++q, ++j) {
            uint32_t cur = st.cur[c];
            bool got = false;
            while (cur < hi) {
                const uint32_t w = cur >> 6;
                const uint64_t bits = F[w] & ~T[w] & (~0ull << (cur & 63));
                if (bits == 0) {
                    cur = (w + 1) * 64u;
                    continue;
                }
                const uint32_t d = w * 64u + (uint32_t)__builtin_ctzll(bits);
                if (d >= hi) break;
                cur = d + 1;
                if (k + 1 < K_ && lv_fl_[k][d] == lv_fl_[k][d + 1]) continue;  // a domain without leaves
                assign[j] = (int32_t)d;
                mark_word(st, T + w, 1ull << (d & 63));
                if (K_ > 1) take_marks_logged(st, d, k);
                got = true;
                break;
            }
            st.cur[c] = cur;
            if (!got) {
                for (size_t i = st.log.size(); i-- > 0;) *st.log[i].first = st.log[i].second;
                st.log.clear();
                return false;
            }
        }
    }
    return true;
}

uint32_t HostWalk::walk_gangs(GangState& st, const uint64_t* feas, const uint32_t* cnt, const uint32_t* run_class,
                              const uint32_t* run_len, uint32_t n_runs, const uint32_t* gang_runs,
                              const uint32_t* gang_span, uint32_t n_gangs, int32_t* assign, int32_t* span_out,
                              uint32_t* gangs_placed) {
    std::fill(taken_.begin(), taken_.end(), 0ull);
    for (uint32_t k = 0; k < K_; ++k) {
        lv_t_[k] = taken_.data() + toff_[k];
        lv_fl_[k] = fl_[k].data();
        lv_cs_[k] = cs_[k].data();
        lv_par_[k] = par_[k].data();
    }
    st.feas = feas;
    st.gone.assign(st.span_total() + 1, 0u);
    st.need.assign(C_, 0u);
    st.lo.assign(C_, 0u);
    st.hi.assign(C_, 0u);
    st.cur.assign(C_, 0u);
    st.all.assign(C_, 0ull);
    st.gone_all.assign(C_, 0ull);
    st.have_all.assign(C_, 0);
    uint32_t placed = 0, g_placed = 0, r0 = 0;
    size_t j0 = 0;
    for (uint32_t g = 0; g < n_gangs; ++g) {
        const uint32_t nr = gang_runs[g] < n_runs - r0 ? gang_runs[g] : n_runs - r0;
        const uint32_t s = gang_span[g];
        const bool any = s == kSpanAny;
        const uint32_t* rc = run_class + r0;
        const uint32_t* rl = run_len + r0;
        st.cls.clear();
        uint32_t n = 0;
        for (uint32_t r = 0; r < nr; ++r) {
            if (rl[r] == 0) continue;
            if (st.need[rc[r]] == 0) st.cls.push_back(rc[r]);
            st.need[rc[r]] += rl[r];
            n += rl[r];
        }
        int32_t got = -1;
        if (n > 0) {
            if (any)
                for (uint32_t c : st.cls)
                    if (!st.have_all[c]) {  // the whole cluster's count: the sum over the coarsest level's domains
                        uint64_t t = 0;
                        for (uint32_t S = 0; S < D_[0]; ++S) t += cnt[st.span_off(c, 0) + S];
                        st.all[c] = t;
                        st.have_all[c] = 1;
                    }
            const uint32_t nS = any ? 1u : D_[s];
            for (uint32_t S = 0; S < nS && got < 0; ++S) {
                bool may = true;
                for (uint32_t c : st.cls) {
                    const uint64_t left = any ? st.all[c] - st.gone_all[c]
                                              : (uint64_t)cnt[st.span_off(c, s) + S] - st.gone[st.span_off(c, s) + S];
                    if (left < st.need[c]) {
                        may = false;
                        break;
                    }
                }
                if (may && gang_trial(st, S, any, s, rc, rl, nr, assign + j0)) got = (int32_t)S;
            }
        }
        if (got >= 0) {
            // what the gang took is gone from the counts of every class at the
            // same level that held it feasible, at each span level above it
            size_t i = 0;
            for (uint32_t r = 0; r < nr; ++r)
              for (uint32_t q = 0; q < rl[r]; ++q, ++i) {
                const uint32_t d = (uint32_t)assign[j0 + i];
                const uint32_t k = level_[rc[r]];
                uint32_t anc[kMaxLevels];
                anc[k] = d;
                for (int kk = (int)k - 1; kk >= 0; --kk) anc[kk] = (uint32_t)lv_par_[kk + 1][anc[kk + 1]];
                for (uint32_t c = 0; c < C_; ++c) {
                    if (level_[c] != k || !((feas[woff_[c] + (d >> 6)] >> (d & 63)) & 1ull)) continue;
                    for (uint32_t kk = 0; kk <= k; ++kk) st.gone[st.span_off(c, kk) + anc[kk]] += 1;
                    st.gone_all[c] += 1;
                }
            }
            placed += n;
            g_placed += 1;
        } else {
            for (uint32_t i = 0; i < n; ++i) assign[j0 + i] = -1;
        }
        if (span_out) span_out[g] = got;
        for (uint32_t c : st.cls) st.need[c] = 0;
        r0 += nr;
        j0 += n;
    }
    st.log.clear();
    *gangs_placed = g_placed;
    return placed;
}

// ---- the spread walk (DESIGN.md §2 "Spread placement") ----
uint32_t HostWalk::walk_spread(SpreadState& st, const uint64_t* feas, const uint32_t* cnt_feas, const uint32_t* cnt_fits,
                               const uint32_t* peers, uint32_t s, uint32_t max_skew, const uint32_t* run_class,
                               const uint32_t* run_len, uint32_t n_runs, int32_t* assign, int32_t* spread_out,
                               uint32_t* count_out, uint32_t* refused, uint32_t* skew) {
    std::fill(taken_.begin(), taken_.end(), 0ull);
    for (uint32_t k = 0; k < K_; ++k) {
        lv_t_[k] = taken_.data() + toff_[k];
        lv_fl_[k] = fl_[k].data();
        lv_cs_[k] = cs_[k].data();
        lv_par_[k] = par_[k].data();
    }
    const uint32_t Ds = D_[s];
    const auto later = std::greater<uint64_t>();
    st.n.assign(peers, peers + Ds);
    st.gone.assign((size_t)C_ * Ds, 0u);
    st.cur.assign((size_t)C_ * Ds, SpreadState::kUnset);
    st.cand.resize(C_);
    st.elig.resize(C_);
    st.begun.assign(C_, 0);
    st.seen.assign(Ds, 0);
    uint32_t placed = 0, n_refused = 0;
    size_t j = 0;
    const bool marks = K_ > 1;
    // the heap's top with its key brought up to n[S]; false when the heap is empty
    const auto settle = [&](std::vector<uint64_t>& h) {
        while (!h.empty()) {
            const uint32_t S = (uint32_t)h.front();
            const uint64_t now = ((uint64_t)st.n[S] << 32) | S;
            if (h.front() == now) return true;
            std::pop_heap(h.begin(), h.end(), later);
            h.back() = now;
            std::push_heap(h.begin(), h.end(), later);
        }
        return false;
    };
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint32_t c = run_class[r], k = level_[c], len = run_len[r];
        if (len == 0) continue;
        const uint32_t* cf = cnt_feas + (size_t)c * Ds;
        const uint32_t* ce = cnt_fits + (size_t)c * Ds;
        uint32_t* gone = st.gone.data() + (size_t)c * Ds;
        uint32_t* curs = st.cur.data() + (size_t)c * Ds;
        std::vector<uint64_t>& cand = st.cand[c];
        std::vector<uint64_t>& elig = st.elig[c];
        if (!st.begun[c]) {
            cand.clear();
            elig.clear();
            for (uint32_t S = 0; S < Ds; ++S) {
                if (ce[S] == 0) continue;
                st.seen[S] = 1;
                const uint64_t key = ((uint64_t)st.n[S] << 32) | S;
                elig.push_back(key);
                if (cf[S] > gone[S]) cand.push_back(key);
            }
            std::make_heap(elig.begin(), elig.end(), later);
            std::make_heap(cand.begin(), cand.end(), later);
            st.begun[c] = 1;
        }
        const uint64_t* F = feas + woff_[c];
        uint64_t* T = lv_t_[k];
        for (uint32_t q = 0; q < len; ++q, ++j) {
            int32_t got_d = -1, got_S = -1;
            if (settle(elig)) {
                const uint64_t m = elig.front() >> 32;
                while (settle(cand)) {
                    const uint32_t S = (uint32_t)cand.front();
                    // the lowest free feasible domain of S's segment at the class's level
                    uint32_t hi = S + 1, lo = S;
                    for (uint32_t kk = s; kk < k; ++kk) {
                        lo = lv_cs_[kk][lo];
                        hi = lv_cs_[kk][hi];
                    }
                    uint32_t cur = curs[S] == SpreadState::kUnset ? lo : curs[S];
                    int32_t d = -1;
                    if (cf[S] > gone[S])
                        while (cur < hi) {
                            const uint32_t w = cur >> 6;
                            const uint64_t bits = F[w] & ~T[w] & (~0ull << (cur & 63));
                            if (bits == 0) {
                                cur = (w + 1) * 64u;
                                continue;
                            }
                            const uint32_t b = w * 64u + (uint32_t)__builtin_ctzll(bits);
                            if (b < hi) d = (int32_t)b;
                            cur = b < hi ? b : hi;
                            break;
                        }
                    else
                        cur = hi;
                    curs[S] = cur < hi ? cur : hi;
                    if (d < 0) {  // nothing left in S for this class, now or later
                        std::pop_heap(cand.begin(), cand.end(), later);
                        cand.pop_back();
                        continue;
                    }
                    if (max_skew != 0 && (uint64_t)st.n[S] + 1 - m > max_skew) {
                        n_refused += 1;  // the smallest n among the S with room: every other fails too
                        break;
                    }
                    got_d = d;
                    got_S = (int32_t)S;
                    break;
                }
            }
            assign[j] = got_d;
            if (spread_out) spread_out[j] = got_S;
            if (got_d < 0) continue;
            const uint32_t d = (uint32_t)got_d;
            T[d >> 6] |= 1ull << (d & 63);
            if (marks) take_marks(d, k);
            curs[got_S] = d + 1;
            st.n[got_S] += 1;
            placed += 1;
            // the domain is gone from the counts of every class of this level that held it feasible
            for (uint32_t c2 = 0; c2 < C_; ++c2)
                if (level_[c2] == k && ((feas[woff_[c2] + (d >> 6)] >> (d & 63)) & 1ull))
                    st.gone[(size_t)c2 * Ds + (uint32_t)got_S] += 1;
        }
    }
    uint32_t mn = 0xFFFFFFFFu, mx = 0;
    for (uint32_t S = 0; S < Ds; ++S) {
        if (count_out) count_out[S] = st.n[S];
        if (!st.seen[S]) continue;
        mn = std::min(mn, st.n[S]);
        mx = std::max(mx, st.n[S]);
    }
    *refused = n_refused;
    *skew = mx >= mn ? mx - mn : 0u;
    return placed;
}

}  // namespace jsp

// Internal entries for the CPU tests of the host walk (tests/test_host_walk.py)
// and its timing (tools/walk_bench.py): not part of include/jsplace.h. The
// hierarchy tables are derived from first_leaf as jsp_topology_upload derives
// them.
static bool walk_setup(jsp::HostWalk& w, uint32_t K, const uint32_t* D, const uint32_t* const* first_leaf, uint32_t C,
                       const uint32_t* cls_level, const uint32_t* cls_pods, uint32_t n_blocks, const uint32_t* blk_l0,
                       const uint32_t* blk_l1, uint32_t groups, uint32_t cpg) {
    using jsp::kMaxLevels;
    if (K < 1 || K > kMaxLevels) return false;
    std::vector<uint32_t> fl[kMaxLevels], cs[kMaxLevels];
    std::vector<int32_t> par[kMaxLevels];
    for (uint32_t k = 0; k < K; ++k) fl[k].assign(first_leaf[k], first_leaf[k] + D[k] + 1);
    for (uint32_t k = 0; k < K; ++k) {
        if (k + 1 < K) {
            cs[k].resize(D[k] + 1);
            for (uint32_t d = 0; d <= D[k]; ++d)
                cs[k][d] = (uint32_t)(std::lower_bound(fl[k + 1].begin(), fl[k + 1].end(), fl[k][d]) - fl[k + 1].begin());
        }
        if (k > 0) {
            par[k].resize(std::max<uint32_t>(D[k], 1));
            for (uint32_t d = 0; d < D[k]; ++d)
                par[k][d] = (int32_t)(std::upper_bound(fl[k - 1].begin(), fl[k - 1].end(), fl[k][d]) - fl[k - 1].begin()) - 1;
        }
    }
    std::vector<jsp::DevClass> cls(C);
    for (uint32_t c = 0; c < C; ++c) {
        std::memset(&cls[c], 0, sizeof cls[c]);
        cls[c].level = cls_level[c];
        cls[c].pods = cls_pods[c];
    }
    w.set_topology(K, D, fl, cs, par);
    w.set_classes(cls);
    w.set_tiles(std::vector<uint32_t>(blk_l0, blk_l0 + n_blocks), std::vector<uint32_t>(blk_l1, blk_l1 + n_blocks),
                groups, cpg);
    return true;
}

extern "C" int jspi_walk_test(uint32_t K, const uint32_t* D, const uint32_t* const* first_leaf, uint32_t C,
                              const uint32_t* cls_level, const uint32_t* cls_pods, uint32_t n_blocks,
                              const uint32_t* blk_l0, const uint32_t* blk_l1, uint32_t groups, uint32_t cpg,
                              const uint64_t* slots, const uint32_t* run_class, const uint32_t* run_len,
                              uint32_t n_runs, int32_t* assign) {
    jsp::HostWalk w;
    if (!walk_setup(w, K, D, first_leaf, C, cls_level, cls_pods, n_blocks, blk_l0, blk_l1, groups, cpg)) return -1;
    return (int)w.place(slots, run_class, run_len, n_runs, assign);
}

// The same walk `iters` times on one set-up walker: mean ns per place() in
// out_ns[0], and in out_ns[1] the feasibility build alone.
extern "C" int jspi_walk_bench(uint32_t K, const uint32_t* D, const uint32_t* const* first_leaf, uint32_t C,
                               const uint32_t* cls_level, const uint32_t* cls_pods, uint32_t n_blocks,
                               const uint32_t* blk_l0, const uint32_t* blk_l1, uint32_t groups, uint32_t cpg,
                               const uint64_t* slots, const uint32_t* run_class, const uint32_t* run_len,
                               uint32_t n_runs, int32_t* assign, uint32_t iters, double* out_ns) {
    jsp::HostWalk w;
    if (!walk_setup(w, K, D, first_leaf, C, cls_level, cls_pods, n_blocks, blk_l0, blk_l1, groups, cpg)) return -1;
    uint32_t placed = 0;
    auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < iters; ++i) placed = w.place(slots, run_class, run_len, n_runs, assign);
    auto t1 = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < iters; ++i) w.feasibility_only(slots);
    auto t2 = std::chrono::steady_clock::now();
    out_ns[0] = std::chrono::duration<double, std::nano>(t1 - t0).count() / std::max<uint32_t>(iters, 1);
    out_ns[1] = std::chrono::duration<double, std::nano>(t2 - t1).count() / std::max<uint32_t>(iters, 1);
    return (int)placed;
}

// The gang walk alone over given feasibility words (the engine's word_off
// layout), for the CPU tests (tests/test_gang.py): the span counts are the
// kernel's definition restated on the host -- the set bits of the class's
// words inside the range child_start gives for S -- or, with all_ones, the
// loosest sound counts (every domain of the range), so that the test shows
// the answer does not depend on how tight the prefilter is.
extern "C" int jspi_gang_walk_test(uint32_t K, const uint32_t* D, const uint32_t* const* first_leaf, uint32_t C,
                                   const uint32_t* cls_level, const uint32_t* cls_pods, const uint64_t* feas,
                                   int all_ones, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                                   const uint32_t* gang_runs, const uint32_t* gang_span, uint32_t n_gangs,
                                   int32_t* assign, int32_t* span_out, uint32_t* gangs_placed) {
    jsp::HostWalk w;
    const uint32_t zero = 0;
    if (!walk_setup(w, K, D, first_leaf, C, cls_level, cls_pods, 0, &zero, &zero, 1, 1)) return -1;
    std::vector<uint32_t> fl[jsp::kMaxLevels];
    for (uint32_t k = 0; k < K; ++k) fl[k].assign(first_leaf[k], first_leaf[k] + D[k] + 1);
    jsp::GangState wst;
    w.gang_layout(wst);
    std::vector<uint32_t> cnt(wst.span_total() + 1, 0u);
    uint32_t woff = 0;
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t lc = cls_level[c];
        for (uint32_t s = 0; s <= lc; ++s)
            for (uint32_t S = 0; S < D[s]; ++S) {
                uint32_t lo = S, hi = S + 1;
                for (uint32_t k = s; k < lc; ++k) {
                    lo = (uint32_t)(std::lower_bound(fl[k + 1].begin(), fl[k + 1].end(), fl[k][lo]) - fl[k + 1].begin());
                    hi = (uint32_t)(std::lower_bound(fl[k + 1].begin(), fl[k + 1].end(), fl[k][hi]) - fl[k + 1].begin());
                }
                uint32_t n = 0;
                for (uint32_t d = lo; d < hi; ++d) n += all_ones ? 1u : (uint32_t)((feas[woff + (d >> 6)] >> (d & 63)) & 1ull);
                cnt[wst.span_off(c, s) + S] = n;
            }
        woff += (D[lc] + 63) / 64;
    }
    uint32_t gp = 0;
    const uint32_t placed = w.walk_gangs(wst, feas, cnt.data(), run_class, run_len, n_runs, gang_runs, gang_span, n_gangs,
                                         assign, span_out, &gp);
    if (gangs_placed) *gangs_placed = gp;
    return (int)placed;
}

// The fit walk alone over given candidate lists (the engine's layout: class
// c's segment of D[level[c]] entries behind those of the classes before it,
// its nf[c] candidates first), for the CPU tests (tests/test_fit.py). fitv
// (nullable) and slack_out (nullable) as HostWalk::walk_fit takes them.
extern "C" int jspi_fit_walk_test(uint32_t K, const uint32_t* D, const uint32_t* const* first_leaf, uint32_t C,
                                  const uint32_t* cls_level, const uint32_t* cls_pods, const uint32_t* order,
                                  const uint32_t* nf, const uint32_t* fitv, const uint32_t* run_class,
                                  const uint32_t* run_len, uint32_t n_runs, int32_t* assign, uint64_t* slack_out) {
    jsp::HostWalk w;
    const uint32_t zero = 0;
    if (!walk_setup(w, K, D, first_leaf, C, cls_level, cls_pods, 0, &zero, &zero, 1, 1)) return -1;
    std::vector<uint32_t> off(C + 1, 0u);
    for (uint32_t c = 0; c < C; ++c) {
        if (cls_level[c] >= K) return -1;
        off[c + 1] = off[c] + D[cls_level[c]];
    }
    for (uint32_t r = 0; r < n_runs; ++r)
        if (run_class[r] >= C) return -1;
    return (int)w.walk_fit(order, nf, off.data(), fitv, run_class, run_len, n_runs, assign, slack_out);
}

// The spread walk alone over given feasibility and fits words (the engine's
// word_off layout) and peer counts, for the CPU tests (tests/test_spread.py):
// the two span-count tables are the kernel's definition restated on the host
// (the set bits of the class's words inside the range child_start gives for S),
// one row per class at span level s; a class finer than s gets zero rows.
extern "C" int jspi_spread_walk_test(uint32_t K, const uint32_t* D, const uint32_t* const* first_leaf, uint32_t C,
                                     const uint32_t* cls_level, const uint32_t* cls_pods, const uint64_t* feas,
                                     const uint64_t* fits, const uint32_t* peers, uint32_t s, uint32_t max_skew,
                                     const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                                     int32_t* assign, int32_t* spread_out, uint32_t* count_out, uint32_t* refused,
                                     uint32_t* skew) {
    jsp::HostWalk w;
    const uint32_t zero = 0;
    if (!walk_setup(w, K, D, first_leaf, C, cls_level, cls_pods, 0, &zero, &zero, 1, 1)) return -1;
    if (s >= K) return -1;
    for (uint32_t r = 0; r < n_runs; ++r)
        if (run_class[r] >= C || (run_len[r] != 0 && cls_level[run_class[r]] < s)) return -1;
    std::vector<uint32_t> fl[jsp::kMaxLevels];
    for (uint32_t k = 0; k < K; ++k) fl[k].assign(first_leaf[k], first_leaf[k] + D[k] + 1);
    const uint32_t Ds = D[s];
    std::vector<uint32_t> cf((size_t)C * Ds + 1, 0u), ce((size_t)C * Ds + 1, 0u);
    uint32_t woff = 0;
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t lc = cls_level[c];
        for (uint32_t S = 0; lc >= s && S < Ds; ++S) {
            uint32_t lo = S, hi = S + 1;
            for (uint32_t k = s; k < lc; ++k) {
                lo = (uint32_t)(std::lower_bound(fl[k + 1].begin(), fl[k + 1].end(), fl[k][lo]) - fl[k + 1].begin());
                hi = (uint32_t)(std::lower_bound(fl[k + 1].begin(), fl[k + 1].end(), fl[k][hi]) - fl[k + 1].begin());
            }
            for (uint32_t d = lo; d < hi; ++d) {
                cf[(size_t)c * Ds + S] += (uint32_t)((feas[woff + (d >> 6)] >> (d & 63)) & 1ull);
                ce[(size_t)c * Ds + S] += (uint32_t)((fits[woff + (d >> 6)] >> (d & 63)) & 1ull);
            }
        }
        woff += (D[lc] + 63) / 64;
    }
    jsp::SpreadState st;
    uint32_t ref = 0, sk = 0;
    const uint32_t placed = w.walk_spread(st, feas, cf.data(), ce.data(), peers, s, max_skew, run_class, run_len, n_runs,
                                          assign, spread_out, count_out, &ref, &sk);
    if (refused) *refused = ref;
    if (skew) *skew = sk;
    return (int)placed;
}
