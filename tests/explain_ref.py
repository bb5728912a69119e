"""The yardstick of the jsp_explain tests (DESIGN.md §2 "Why a job has no
domain"): the rule restated in vectorised numpy. It never calls the engine.
Its cap / occ are cross-checked against cpu_ref.c where a test uses it."""
import numpy as np

from jobset_amd.snapshot import Problem

M64 = (1 << 64) - 1


def _segsum(x, bounds):
    """Sums of x over [bounds[i], bounds[i+1]) (np.add.reduceat, but an empty
    segment sums to 0)."""
    pre = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
    b = np.asarray(bounds, dtype=np.int64)
    return pre[b[1:]] - pre[b[:-1]]


def reference(p: Problem):
    """The rule of DESIGN.md §2, vectorised. Returns (records, cap [C, L], occ [L])."""
    nd, topo = p.nodes, p.topology
    N, W, R, Kl = nd.n_nodes, nd.n_label_words, nd.n_res, topo.n_levels
    free = nd.free.astype(np.int64)
    occupied = nd.excl != -1
    occ = _segsum(occupied, nd.leaf_start)
    recs, caps = [], []
    for jc in p.classes:
        req, fb = jc.words(4)
        sel = np.ones(N, dtype=bool)
        for w in range(W):  # jsplace.h: two tests, every required bit set and every forbidden bit clear
            rq, fw = np.uint64(req[w] & M64), np.uint64(fb[w] & M64)
            sel &= ((nd.labels[w] & rq) == rq) & ((nd.labels[w] & fw) == 0)
        tnt = (nd.taints & np.uint32(~jc.tolerated_taints & 0xFFFFFFFF)) == 0
        rr = jc.res()[:R]
        short = np.stack([(free[r] < rr[r]) if rr[r] > 0 else np.zeros(N, dtype=bool) for r in range(R)])
        ok = sel & tnt
        cap_n = np.full(N, jc.pods, dtype=np.int64)
        for r in range(R):
            if rr[r] > 0:
                cap_n = np.minimum(cap_n, free[r] // rr[r])
        cap_n = np.where(ok, cap_n, 0)
        cap = _segsum(cap_n, nd.leaf_start)
        fl = np.arange(topo.n_leaves + 1) if jc.level == Kl - 1 else topo.first_leaf[jc.level]
        capsum, occsum = _segsum(cap, fl), _segsum(occ, fl)
        is_short = (occsum == 0) & (capsum < jc.pods)
        best_cap = int(capsum[is_short].max()) if is_short.any() else 0
        rec = dict(rows=N, rows_selector=int((~sel).sum()), rows_taint=int((sel & ~tnt).sum()),
                   rows_no_capacity=int((ok & short.any(axis=0)).sum()),
                   rows_insufficient=[int((ok & short[r]).sum()) for r in range(R)] + [0] * (4 - R),
                   rows_fit=int((ok & ~short.any(axis=0)).sum()), rows_occupied=int(occupied.sum()),
                   domains=topo.n_domains[jc.level], dom_occupied=int((occsum > 0).sum()),
                   dom_short=int(is_short.sum()), dom_feasible=int(((occsum == 0) & (capsum >= jc.pods)).sum()),
                   best_short_cap=best_cap,
                   best_short_domain=int(np.nonzero(is_short & (capsum == best_cap))[0][0]) if is_short.any() else -1)
        # rows_no_capacity is cap(c, n) == 0 among the rows that pass (pods >= 1)
        assert rec["rows_no_capacity"] == int((ok & (cap_n == 0)).sum())
        recs.append(rec)
        caps.append(cap)
    return recs, np.array(caps, dtype=np.int64).reshape(len(p.classes), topo.n_leaves), occ
