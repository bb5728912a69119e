// jsp_walk.h — host half of the split placement service: the lowest-index
// 1:1 greedy over the feasibility the
// resident tiles hand back. The tiles do the streaming part (predicate +
// capacity tally over every node row, per-leaf feasibility, partial sums per
// upper-level domain); what is left is sequential across jobs and small
// (O(J + C D / 64) word operations), so it runs on the host, next to the
// caller, instead of on one GPU wave.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

#include "jsp_internal.h"

namespace jsp {

// The waves of the largest tally row block that hold leaves (64 leaves each,
// at most 4): the split service's line layout (jsp_internal.h SplitArgs).
uint32_t split_waves(const std::vector<uint32_t>& blk_l0, const std::vector<uint32_t>& blk_l1);

// The gang walk's state (HostWalk::walk_gangs), owned by the caller so that
// HostWalk itself keeps its size and layout. The span counts' layout: class
// c's counts of span level s <= level[c] start at span_off(c, s), one per
// level-s domain; span_total() in all.
struct GangState {
    std::vector<uint32_t> doff;              // domains of the levels before k
    std::vector<uint32_t> coff;              // span counts before class c (its levels 0..level[c])
    std::vector<uint32_t> gone;              // per span count: feasible domains the walk has taken there since
    std::vector<uint32_t> need, lo, hi, cur;  // per class: the gang's jobs, its segment of S, its cursor
    std::vector<uint64_t> all, gone_all;     // per class: the count over the whole cluster (lazily), taken since
    std::vector<uint8_t> have_all;
    std::vector<uint32_t> cls;               // the gang's classes
    std::vector<std::pair<uint64_t*, uint64_t>> log;  // a trial's changed taken words and their old values
    const uint64_t* feas = nullptr;
    uint32_t span_off(uint32_t c, uint32_t s) const { return coff[c] + doff[s]; }
    uint32_t span_total() const { return coff.empty() ? 0u : coff.back(); }
};

// The spread walk's state (HostWalk::walk_spread), owned by the caller as
// GangState is. Counts and cursors are laid out per class and level-s domain:
// class c's entry for S is c * D[s] + S.
struct SpreadState {
    std::vector<uint32_t> n;                 // [D_s] peers(S) plus the jobs the walk has put into S
    std::vector<uint32_t> gone;              // per (c, S): feasible domains of c's level the walk has taken there
    std::vector<uint32_t> cur;               // per (c, S): first domain of S's segment not yet passed (kUnset: not begun)
    std::vector<std::vector<uint64_t>> cand; // per class: min-heap of (n[S] << 32) | S over the S that may hold a free
                                             // feasible domain; an entry whose n is stale is re-keyed when it surfaces
    std::vector<std::vector<uint64_t>> elig; // per class: the same over every eligible S (the minimum m)
    std::vector<uint8_t> begun;              // per class: its heaps are built
    std::vector<uint8_t> seen;               // [D_s] eligible for a class of a non-empty run (stats.skew)
    static constexpr uint32_t kUnset = 0xFFFFFFFFu;
};

class HostWalk {
public:
    // topology: first_leaf per level (identity at the leaves), child_start
    // per level k < K-1, parent per level k >= 1 (the engine's upload tables)
    void set_topology(uint32_t K, const uint32_t* D, const std::vector<uint32_t>* fl,
                      const std::vector<uint32_t>* cs, const std::vector<int32_t>* par);
    // classes: level and pods of each (the engine's class upload)
    void set_classes(const std::vector<DevClass>& cls);
    // tiles of the split service: row block leaf ranges (blk table, first and
    // end leaf per block), class groups and classes per group
    void set_tiles(const std::vector<uint32_t>& blk_l0, const std::vector<uint32_t>& blk_l1, uint32_t groups,
                   uint32_t cpg);

    // One request: feasibility from the tiles' slots (jsp_internal.h
    // SplitArgs), then the walk over runs in global order. Returns the
    // number of placed jobs; assign[j] = domain at the job's class level or -1.
    uint32_t place(const uint64_t* slots, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                   int32_t* assign);

    // The walk alone over feasibility bitmaps the GPU built (feas_kernel's
    // layout: class c's words at the cumulative offset of (D[level] + 63) / 64
    // words per class -- the engine's word_off). The device paths' walk for
    // the shapes whose GPU walk is a one-wave dependent chain.
    uint32_t walk(const uint64_t* feas, const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs,
                  int32_t* assign);
    // The gang walk (DESIGN.md §2 "Gang placement") over the same bitmaps:
    // gang g is the next gang_runs[g] runs and is placed whole inside one
    // domain of level gang_span[g] (kSpanAny: the whole cluster), or not at
    // all. Candidates S in ascending order; one whose span count (cnt, the
    // GPU's: span_off's layout) minus what the walk has taken there since
    // falls short of the gang's jobs of some class is skipped, the others are
    // tried: the gang's jobs in global order each take the lowest free
    // feasible domain of S, and a trial that fails is rolled back word by
    // word. assign[j] as walk(); span_out[g] = S (0 for kSpanAny) or -1.
    // Returns the placed jobs, *gangs_placed the gangs that got a domain.
    static constexpr uint32_t kSpanAny = 0xFFFFFFFFu;
    uint32_t walk_gangs(GangState& st, const uint64_t* feas, const uint32_t* cnt, const uint32_t* run_class,
                        const uint32_t* run_len, uint32_t n_runs, const uint32_t* gang_runs, const uint32_t* gang_span,
                        uint32_t n_gangs, int32_t* assign, int32_t* span_out, uint32_t* gangs_placed);
    // The spread walk (DESIGN.md §2 "Spread placement") over the same bitmaps:
    // every job takes, among the level-s domains S eligible for its class
    // (cnt_fits[c * D[s] + S] > 0) that hold a free feasible domain and pass
    // the skew test n[S] + 1 - m <= max_skew (m: the smallest n over the
    // eligible S; max_skew 0 skips the test), the one with the smallest
    // (n[S], S), and inside it the lowest free feasible domain. cnt_feas and
    // cnt_fits: the GPU's span counts of the feasibility and the fits words,
    // one row per class at span level s; peers [D[s]]: n's start. Per class a
    // heap of (n[S], S) over the S that may still hold a domain and one over
    // the eligible S, both re-keyed lazily (n only grows), and a cursor per
    // (class, S) (the taken set only grows): O(log D[s]) per job amortised,
    // plus every segment's words once. Classes of non-empty runs must have
    // level >= s. assign[j] as walk(); spread_out[j] (nullable) = S or -1;
    // count_out (nullable) [D[s]] = the final n; *refused: the jobs that got
    // -1 by the skew test alone; *skew: max n - min n over the S eligible for
    // a class of a non-empty run. Returns the placed jobs.
    uint32_t walk_spread(SpreadState& st, const uint64_t* feas, const uint32_t* cnt_feas, const uint32_t* cnt_fits,
                         const uint32_t* peers, uint32_t s, uint32_t max_skew, const uint32_t* run_class,
                         const uint32_t* run_len, uint32_t n_runs, int32_t* assign, int32_t* spread_out,
                         uint32_t* count_out, uint32_t* refused, uint32_t* skew);
    // The span counts' layout for the current topology and classes, into st
    // (GangState::span_off): call after every class upload, before walk_gangs.
    void gang_layout(GangState& st) const;
    // The fit walk (DESIGN.md §2 "Fit placement") over the candidate lists
    // the GPU ordered: class c's list is order[fit_off[c] .. + nf[c]), its
    // feasible domains in ascending (key, id). One cursor per class; a job
    // moves its class's cursor past the entries whose bit is set in the
    // level's taken words, takes the next one and marks what intersects it.
    // Taken bits are never cleared, so a cursor never moves back: O(J + sum of
    // nf). fitv (nullable): fit(c, d) at fit_off[c] + d, summed over the taken
    // entries minus the class's pods into *slack. assign[j] as walk();
    // returns the placed jobs.
    uint32_t walk_fit(const uint32_t* order, const uint32_t* nf, const uint32_t* fit_off, const uint32_t* fitv,
                      const uint32_t* run_class, const uint32_t* run_len, uint32_t n_runs, int32_t* assign,
                      uint64_t* slack);
    // start loading the walk's own state (cold host core: the call after a
    // sleep), while the device works
    void prefetch_state() const;

    // Tile t (= row block t / groups, class group t % groups) has answered:
    // start loading its slot lines into the host cache while the other tiles
    // finish (pinned memory the device just wrote misses every cache level;
    // read one by one in the walk, the misses cost cfg3 ~3.9 us, cfg5 ~7.4 us).
    void prefetch_tile(const uint64_t* slots, uint32_t t) const;

    // Tile t's answer to request seq has arrived whole: every entry of its
    // lines carries seq and every record its wave counts carries the
    // request's record tag (jsp_internal.h SplitArgs).
    bool tile_ready(const uint64_t* slots, uint32_t t, uint32_t seq) const;

    // The feasibility bitmaps of the last request (tests / diagnostics):
    // words [woff[c], woff[c+1]) of class c.
    const std::vector<uint64_t>& feas() const { return feas_; }
    // the feasibility build alone (timing: tools/walk_bench.py)
    void feasibility_only(const uint64_t* slots) { build_feasibility(slots); }

private:
    void build_feasibility(const uint64_t* slots);
    void take_marks(uint32_t d, uint32_t k);
    bool gang_trial(GangState& st, uint32_t S, bool any, uint32_t s, const uint32_t* run_class, const uint32_t* run_len,
                    uint32_t n_runs, int32_t* assign);
    void mark_word(GangState& st, uint64_t* p, uint64_t m);
    void take_marks_logged(GangState& st, uint32_t d, uint32_t k);

    struct ClassWalk {
        const uint64_t* F;  // feasibility words
        uint64_t* T;        // taken words at the class's level
        uint32_t D, nw, k;  // domains at that level, their words, the level
        uint32_t cursor;    // first domain not yet passed
    };

    uint32_t K_ = 0, L_ = 0, C_ = 0, groups_ = 1, cpg_ = 1, nw_ = 1;
    uint32_t D_[kMaxLevels] = {0, 0, 0, 0};
    std::vector<uint32_t> fl_[kMaxLevels], cs_[kMaxLevels];
    std::vector<int32_t> par_[kMaxLevels];
    std::vector<uint32_t> level_, pods_, woff_, toff_, uoff_;
    std::vector<uint32_t> l0_, l1_;          // per row block
    std::vector<uint64_t> occ_;              // occupied leaves (bitmap)
    std::vector<uint64_t> occ_lvl_;          // occupied domains per level above the leaves (toff_ layout)
    std::vector<uint64_t> feas_;             // feasibility words of every class (woff_ layout)
    std::vector<uint64_t> sums_;             // clamped capacity sums of every upper class's domains (uoff_ layout)
    std::vector<uint64_t> taken_;            // taken domains per level (toff_ layout)
    std::vector<ClassWalk> cw_;              // per class, set up per request
    // per level, set up per walk: taken words, first leaf, child start, parent
    uint64_t* lv_t_[kMaxLevels] = {nullptr, nullptr, nullptr, nullptr};
    const uint32_t* lv_fl_[kMaxLevels] = {nullptr, nullptr, nullptr, nullptr};
    const uint32_t* lv_cs_[kMaxLevels] = {nullptr, nullptr, nullptr, nullptr};
    const int32_t* lv_par_[kMaxLevels] = {nullptr, nullptr, nullptr, nullptr};
    bool any_upper_ = false;
};

}  // namespace jsp
