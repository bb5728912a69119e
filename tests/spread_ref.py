"""The yardstick of the spread-placement tests (DESIGN.md §2 "Spread
placement"): the rule restated in numpy over the CPU oracle's tallies
(O.place_c). It never calls the engine.

fits(c, d) is capsum(c, d) >= pods[c] (an int64 sum over the domain's leaves),
feasible(c, d) adds occsum(d) == 0. The taken set is an array of used leaves,
as in gang_ref: a domain is taken iff one of its leaves is used. Every job
looks at every level-s domain S: a literal O(J D) walk without heaps, cursors
or counts.

Also here: peers_ref (the peer owner segments per S, row by row), the tables
in the engine's layout (fits_words, count_tables), check_spread (the answer's
invariants), the hand cases and the sweep generator, shared by the CPU tests,
which assert the coverage floors on this reference's own output, and the GPU
tests, which compare the engine with it."""
import dataclasses

import numpy as np

from jobset_amd import synth
from jobset_amd.snapshot import Nodes, job_runs
from oracle import oracle as O
from bind_ref import cls, flat, nested
from gang_ref import feasibility, reduction_problem, sweep_case  # noqa: F401  (the tests' inputs)

SOFT = 0
INT32_MIN = -(1 << 31)


def fits_table(p, cap):
    """fits[c]: bool [D[level[c]]]: capsum(c, d) >= pods[c], occupancy ignored."""
    out = []
    for c, jc in enumerate(p.classes):
        fl = np.asarray(p.topology.first_leaf[jc.level], dtype=np.int64)
        cs = np.concatenate([[0], np.cumsum(cap[c].astype(np.int64))])
        out.append((cs[fl[1:]] - cs[fl[:-1]]) >= jc.pods)
    return out


def peers_ref(p, s, peer_ids):
    """int64 [D_s]: the rows n of S, rows [r0, r1), whose owner is a peer and
    (n == r0 or excl[n - 1] != excl[n])."""
    ids = set(int(x) for x in np.asarray(peer_ids, dtype=np.int64).reshape(-1))
    assert -1 not in ids
    excl = np.asarray(p.nodes.excl, dtype=np.int64)
    fl, ls = p.topology.first_leaf[s], p.nodes.leaf_start
    out = np.zeros(p.topology.n_domains[s], dtype=np.int64)
    for S in range(out.shape[0]):
        r0, r1 = int(ls[int(fl[S])]), int(ls[int(fl[S + 1])])
        for n in range(r0, r1):
            if int(excl[n]) in ids and (n == r0 or excl[n - 1] != excl[n]):
                out[S] += 1
    return out


def spread_ref(p, s, max_skew, peer_ids, tallies=None):
    """(assign int32 [J], spread_out int32 [J], count uint32 [D_s], stats dict,
    flags dict) of the rule for problem p (jobs p.job_class in global order).
    flags: pinned -- for some job every eligible S attaining the minimum m held
    no free feasible domain while another eligible S did; cross -- a job of a
    class above the leaf level took a domain that intersected a free feasible
    domain of another class."""
    cap, occ = tallies if tallies is not None else O.place_c(p)[1:]
    topo = p.topology
    K = topo.n_levels
    fl = [np.asarray(f, dtype=np.int64) for f in topo.first_leaf]
    feas, fits = feasibility(p, cap, occ), fits_table(p, cap)
    Ds = topo.n_domains[s]
    aS, bS = fl[s][:-1], fl[s][1:]
    n = peers_ref(p, s, peer_ids)
    J = p.n_jobs
    assign = np.full(J, -1, dtype=np.int32)
    spread = np.full(J, -1, dtype=np.int32)
    used = np.zeros(topo.n_leaves, dtype=bool)
    refused = 0
    seen = np.zeros(Ds, dtype=bool)
    pinned = cross = False

    def home(c):
        """int64 [D]: the S whose leaf range holds domain d's non-empty one, else -1."""
        f = fl[p.classes[c].level]
        a, b = f[:-1], f[1:]
        S = np.searchsorted(bS, a, side="right")          # the first S that ends behind a
        S = np.minimum(S, Ds - 1)
        return np.where((a < b) & (a >= aS[S]) & (b <= bS[S]), S, -1)

    homes = {}

    def inside(c, S):
        if c not in homes:
            homes[c] = home(c)
        return homes[c] == S

    def per_S(c, mask):
        """bool [D_s]: S holds a domain of `mask`."""
        inside(c, 0)
        h = homes[c][mask]
        return np.bincount(h[h >= 0], minlength=Ds) > 0

    def free_feasible(c, ucs):
        f = fl[p.classes[c].level]
        return feas[c] & ((ucs[f[1:]] - ucs[f[:-1]]) == 0) & (f[:-1] < f[1:])

    for j in range(J):
        c = int(p.job_class[j])
        lvl = p.classes[c].level
        assert lvl >= s, "the spread level is finer than the class's"
        ucs = np.concatenate([[0], np.cumsum(used)])
        open_c = free_feasible(c, ucs)
        elig = per_S(c, fits[c])
        seen |= elig
        if not elig.any():
            continue
        m = int(n[elig].min())
        room = elig & per_S(c, open_c)
        cand = room & ((n + 1 - m <= max_skew) if max_skew >= 1 else True)
        if room.any() and not (room & (n == m)).any():
            pinned = True
        if not cand.any():
            refused += int(room.any())
            continue
        S = min((int(n[x]), int(x)) for x in np.nonzero(cand)[0])[1]
        d = int(np.nonzero(open_c & inside(c, S))[0][0])
        f = fl[lvl]
        if lvl < K - 1:
            for c2 in range(len(p.classes)):
                if c2 == c:
                    continue
                f2 = fl[p.classes[c2].level]
                hit = free_feasible(c2, ucs) & (f2[:-1] < f[d + 1]) & (f2[1:] > f[d])
                cross |= bool(hit.any())
        used[f[d]:f[d + 1]] = True
        assign[j] = d
        spread[j] = S
        n[S] += 1
    skew = int(n[seen].max() - n[seen].min()) if seen.any() else 0
    stats = dict(jobs=J, placed=int((assign >= 0).sum()), refused=refused, skew=skew,
                 runs=int(job_runs(p.job_class)[0].shape[0]), fused=7)
    return assign, spread, n.astype(np.uint32), stats, dict(pinned=pinned, cross=cross)


def check_spread(p, s, max_skew, peer_ids, assign, spread, count, tallies=None):
    """The invariants of an answer: the taken domains are feasible, pairwise
    disjoint, inside their S; count is peers plus the jobs per S; with a
    positive max_skew every take kept n[S] + 1 - m <= max_skew for its class's
    eligible minimum at that moment."""
    cap, occ = tallies if tallies is not None else O.place_c(p)[1:]
    topo = p.topology
    fl = [np.asarray(f, dtype=np.int64) for f in topo.first_leaf]
    feas, fits = feasibility(p, cap, occ), fits_table(p, cap)
    n = peers_ref(p, s, peer_ids)
    used = np.zeros(topo.n_leaves, dtype=bool)
    for j in range(p.n_jobs):
        d, S = int(assign[j]), int(spread[j])
        assert (d < 0) == (S < 0)
        if d < 0:
            continue
        c = int(p.job_class[j])
        f = fl[p.classes[c].level]
        a, b = int(f[d]), int(f[d + 1])
        assert a < b and feas[c][d] and not used[a:b].any(), f"job {j}"
        assert fl[s][S] <= a and b <= fl[s][S + 1], f"job {j}: domain {d} is outside S {S}"
        if max_skew >= 1:
            elig = [x for x in range(n.shape[0])
                    if (fits[c] & (f[:-1] < f[1:]) & (f[:-1] >= fl[s][x]) & (f[1:] <= fl[s][x + 1])).any()]
            assert n[S] + 1 - min(n[x] for x in elig) <= max_skew, f"job {j}: skew"
        used[a:b] = True
        n[S] += 1
    np.testing.assert_array_equal(n, count)


# ---- the tables in the engine's layout
def words_of(table):
    out = []
    for f in table:
        bits = np.zeros(((f.shape[0] + 63) // 64) * 64, dtype=np.uint8)
        bits[:f.shape[0]] = f
        out.append(np.packbits(bits, bitorder="little").view(np.uint64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def fits_words(p, cap):
    """jspb_spread_tables' fits words: class c's (D + 63) // 64 words behind
    those of the classes before it, padding bits zero."""
    return words_of(fits_table(p, cap))


def count_tables(p, s, cap, occ):
    """(cnt_feas, cnt_fits) uint32 [C, D_s]: the set bits of the class's words
    inside S's child range followed down to level[c] (first_leaf lower bounds,
    as the engine's child_start); zero rows for a class finer than s."""
    topo = p.topology
    fl = [np.asarray(f, dtype=np.int64) for f in topo.first_leaf]
    Ds = topo.n_domains[s]
    out = []
    for table in (feasibility(p, cap, occ), fits_table(p, cap)):
        t = np.zeros((len(p.classes), Ds), dtype=np.uint32)
        for c, f in enumerate(table):
            lc = p.classes[c].level
            if lc < s:
                continue
            fcs = np.concatenate([[0], np.cumsum(f.astype(np.int64))])
            lo = np.arange(Ds + 1, dtype=np.int64)
            for k in range(s, lc):
                lo = np.searchsorted(fl[k + 1], fl[k][lo], side="left")
            t[c] = fcs[lo[1:]] - fcs[lo[:-1]]
        out.append(t)
    return out[0], out[1]


def stats_dict(st):
    return dict(jobs=int(st.jobs), placed=int(st.placed), refused=int(st.refused), skew=int(st.skew),
                runs=int(st.runs), fused=int(st.fused))


# ---- hand cases: name -> (problem, s, max_skew, peers, assign, spread_out, count, refused)
def hand_cases():
    A, B = 7, 9
    rack = cls(1, 2)
    zr = [[0, 2, 4], np.arange(5)]          # two zones of two racks
    two = lambda **kw: nested(zr, [2, 2, 2, 2], [rack], [0, 0, 0, 0], **kw)  # noqa: E731
    # zone 0 = racks 0-2, zone 1 = rack 3
    lop = lambda jobs, **kw: nested([[0, 3, 4], np.arange(5)], [2, 2, 2, 2], [rack], jobs, **kw)  # noqa: E731
    # zone 1's racks are too small for the class: not eligible
    small = nested(zr, [2, 2, 1, 1], [rack], [0, 0, 0])
    # zone 1's racks fit and are held by B, who is no peer: eligible and full
    full = nested(zr, [2, 2, 2, 2], [rack], [0, 0, 0], excl=[-1, -1, -1, -1, B, B, B, B])
    # A zone class over racks: zone-level job then rack jobs
    mixed = nested(zr, [2, 2, 2, 2], [cls(0, 4), rack], [0, 1, 1])
    return {
        # alternate between the zones, the lower id first
        "alternate": (two(), 0, 1, [], [0, 2, 1, 3], [0, 1, 0, 1], [2, 2], 0),
        # plain placement would fill zone 0 first; SOFT alternates as well
        "alternate-soft": (two(), 0, SOFT, [], [0, 2, 1, 3], [0, 1, 0, 1], [2, 2], 0),
        # a peer in zone 0 (rack 0, which it occupies): zone 1 first
        "peer": (two(excl=[A, A, -1, -1, -1, -1, -1, -1]), 0, 1, [A], [2, 1, 3, -1], [1, 0, 1, -1], [2, 2], 0),
        # the same owner is no peer when it is not in the list: zone 0's free rack first
        "no-peer": (two(excl=[A, A, -1, -1, -1, -1, -1, -1]), 0, 1, [], [1, 2, 3, -1], [0, 1, 1, -1], [1, 2], 0),
        # three racks against one: zone 1 is full after one job and pins m at 1, the fourth job would make the skew 2
        "refused": (lop([0, 0, 0, 0]), 0, 1, [], [0, 3, 1, -1], [0, 1, 0, -1], [2, 1], 1),
        # with max_skew 2 the third and fourth jobs go to zone 0
        "skew-2": (lop([0, 0, 0, 0]), 0, 2, [], [0, 3, 1, 2], [0, 1, 0, 0], [3, 1], 0),
        "soft-fills": (lop([0, 0, 0, 0]), 0, SOFT, [], [0, 3, 1, 2], [0, 1, 0, 0], [3, 1], 0),
        # a zone that could never host the class does not pin the minimum
        "not-eligible": (small, 0, 1, [], [0, 1, -1], [0, 0, -1], [2, 0], 0),
        # a zone that is merely full does: the second job is refused by the skew test
        "full-pins": (full, 0, 1, [], [0, -1, -1], [0, -1, -1], [1, 0], 2),
        # the zone job takes zone 0 (its racks with it); the rack jobs spread over what is left
        "mixed-levels": (mixed, 0, SOFT, [], [0, 2, 3], [0, 1, 1], [1, 2], 0),
        # s == level[c] without peers: jsp_place's answer
        "own-level": (two(), 1, 1, [], [0, 1, 2, 3], [0, 1, 2, 3], [1, 1, 1, 1], 0),
        # A's segment crosses the zone boundary (racks 1 and 2): it counts in both zones
        "peer-crosses": (two(excl=[-1, -1, A, A, A, A, -1, -1]), 0, 1, [A], [0, 3, -1, -1], [0, 1, -1, -1], [2, 2], 0),
        # special ids; INT32_MIN holds rack 0, 0 holds rack 2, 0x40000000 is nowhere
        "special-ids": (two(excl=[INT32_MIN, INT32_MIN, -1, -1, 0, 0, -1, -1]), 0, 1, [0x40000000, 0, INT32_MIN],
                        [1, 3, -1, -1], [0, 1, -1, -1], [2, 2], 0),
    }


# ---------------------------------------------------------------- sweep inputs
SWEEP_SEEDS = range(60)
SWEEP_SKEWS = (1, SOFT, 1, 3)
FIRST_ID = 5000


def sweep(seed):
    """(problem, s, max_skew, peer_ids): gang_ref.sweep_case's problem with the
    jobs' classes kept to the coarsest spread level that has more than one
    domain where there is one (else level 0), so that the level's domains
    differ in what they can host, max_skew by seed, and as peers a seeded half
    of the owners in the snapshot, the fresh owners laid over a few leaves, and
    one id that owns nothing."""
    base = sweep_case(seed)[0]
    r = 55_000 + seed
    topo = base.topology
    s = next((k for k in range(topo.n_levels) if topo.n_domains[k] > 1), 0)
    ok = np.array([c for c, jc in enumerate(base.classes) if jc.level >= s], dtype=np.int64)
    if ok.size == 0:
        s = 0
        ok = np.arange(len(base.classes))
    n_jobs = int(synth.uniform_int(r, 1, 1, 4, 96)[0])
    pick = synth.uniform_int(r, 2, n_jobs, 0, ok.size - 1)
    jc = ok[pick].astype(np.uint32)
    # runs of a few jobs per class, as a JobSet's replicated jobs come
    jc = np.repeat(jc[::3], 3)[:n_jobs] if n_jobs >= 3 else jc
    owners = np.unique(base.nodes.excl[base.nodes.excl != -1]).astype(np.int32)
    keep = synth.bernoulli(r, 3, owners.shape[0], 0.5) if owners.size else np.zeros(0, dtype=bool)
    # running peers: fresh ids on all rows of up to four leaves of one level-s
    # domain (so that its count starts ahead of the others') and of up to two
    # leaves anywhere
    n = base.nodes
    ls = np.asarray(n.leaf_start, dtype=np.int64)
    fl = np.asarray(topo.first_leaf[s], dtype=np.int64)
    excl = n.excl.copy()
    S0 = int(synth.uniform_int(r, 4, 1, 0, topo.n_domains[s] - 1)[0])
    lo, hi = int(fl[S0]), int(fl[S0 + 1])
    leaves = []
    if hi > lo:
        leaves += list(lo + synth.uniform_int(r, 5, int(synth.uniform_int(r, 6, 1, 1, 4)[0]), 0, hi - lo - 1))
    leaves += list(synth.uniform_int(r, 7, int(synth.uniform_int(r, 8, 1, 0, 2)[0]), 0, topo.n_leaves - 1))
    fresh = []
    for i, leaf in enumerate(leaves):
        r0, r1 = int(ls[int(leaf)]), int(ls[int(leaf) + 1])
        if r1 > r0:
            excl[r0:r1] = FIRST_ID + i
            fresh.append(FIRST_ID + i)
    peers = np.concatenate([owners[keep], np.array(fresh + [0x40000000], dtype=np.int32)])
    peers = peers[np.isin(peers, excl) | (peers == 0x40000000)]
    nodes = Nodes(leaf_start=n.leaf_start, labels=n.labels, taints=n.taints, free=n.free, excl=excl,
                  leaf_begin=n.leaf_begin)
    p = dataclasses.replace(base, nodes=nodes, job_class=jc, job_names=None, name=f"spread-sweep-{seed}")
    return p, s, SWEEP_SKEWS[seed % len(SWEEP_SKEWS)], peers


# ---------------------------------------------------------------- reduction inputs
def rooted(p):
    """Problem p under one more, coarsest level that holds the whole cluster in
    one domain (every class one level deeper), or None at four levels."""
    from jobset_amd.snapshot import Topology
    topo = p.topology
    if topo.n_levels >= 4:
        return None
    root = np.array([0, topo.n_leaves], dtype=np.uint32)
    t = Topology(level_keys=["example.com/root"] + list(topo.level_keys), n_domains=[1] + list(topo.n_domains),
                 first_leaf=[root] + [np.asarray(f, dtype=np.uint32) for f in topo.first_leaf])
    t.validate()
    classes = [dataclasses.replace(jc, level=jc.level + 1) for jc in p.classes]
    return dataclasses.replace(p, topology=t, classes=classes, name=p.name + "-rooted")


def one_class(p):
    """Problem p with the jobs of its first job's class only."""
    jc = p.job_class[p.job_class == p.job_class[0]] if p.n_jobs else p.job_class
    return dataclasses.replace(p, job_class=jc, job_names=None)


def owners_of(p):
    return np.unique(p.nodes.excl[p.nodes.excl != -1]).astype(np.int32)
