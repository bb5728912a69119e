"""The yardstick of the preferred-placement tests (DESIGN.md §2 "Preferred
placement"): the rule taken literally in int64 numpy, bind_ref.row_caps for cap(c, n), oracle.place_c's tallies
for B. It never calls the engine. Terms are (cls, weight, req_words, forbid_words) tuples, as Engine takes them."""
import numpy as np

from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from bind_ref import M64, nested, row_caps
from gang_ref import feasibility, sweep_case

CLAMP = 0xFFFFFFFF
SWEEP = range(8)


def row_weights(p, terms, c):
    """w(c, n), int64 [N]: the two tests of the class selector, per term of class c."""
    nd = p.nodes
    w = np.zeros(nd.n_nodes, dtype=np.int64)
    for _, weight, req, forbid in (t for t in terms if t[0] == c):
        ok = np.ones(nd.n_nodes, dtype=bool)
        for k in range(nd.n_label_words):  # words at and past n_label_words are ignored
            rq, fb = (np.uint64((m[k] if k < len(m) else 0) & M64) for m in (req, forbid))
            ok &= ((nd.labels[k] & rq) == rq) & ((nd.labels[k] & fb) == 0)
        w += np.where(ok, weight, 0)
    return w


def scores(p, terms, cap):
    """sc[c]: int64 [D[level[c]]]. cap: the oracle's u32 tallies [C, L]."""
    ls = p.nodes.leaf_start.astype(np.int64)
    leaf_of = np.repeat(np.arange(ls.shape[0] - 1), np.diff(ls))
    out = []
    for c, jc in enumerate(p.classes):
        fl = np.asarray(p.topology.first_leaf[jc.level], dtype=np.int64)
        rc = row_caps(p, c)[0]
        rows_cs = np.concatenate([[0], np.cumsum(rc)])
        leaf_cs = np.concatenate([[0], np.cumsum(cap[c].astype(np.int64))])
        dom_of_leaf = np.searchsorted(fl, np.arange(ls.shape[0] - 1), side="right") - 1
        B = leaf_cs[:-1] - leaf_cs[fl[dom_of_leaf]]          # the tallies of the domain's leaves before each leaf
        pre = np.minimum(jc.pods, B[leaf_of] + rows_cs[:-1] - rows_cs[ls[leaf_of]])
        take = np.minimum(rc, jc.pods - pre)
        part = np.concatenate([[0], np.cumsum(row_weights(p, terms, c) * take)])
        out.append(np.minimum(part[ls[fl[1:]]] - part[ls[fl[:-1]]], CLAMP))
    return out


def ranked(cand, sc):  # cand in ascending (0xFFFFFFFF - sc, d)
    return cand[np.lexsort((cand, CLAMP - sc[cand]))]


def order_ref(p, terms, tallies):  # (order, nf, sc) in jspb_prefer_order's layout
    feas, sc = feasibility(p, *tallies), scores(p, terms, tallies[0])
    order = [np.full(f.shape[0], 0xFFFFFFFF, dtype=np.uint32) for f in feas]
    for seg, f, s in zip(order, feas, sc):
        seg[:int(f.sum())] = ranked(np.nonzero(f)[0], s)
    return np.concatenate(order), np.array([f.sum() for f in feas], dtype=np.uint32), np.concatenate(sc).astype(np.uint32)


def prefer_ref(p, terms, tallies=None):
    """(assign, score, stats): a job takes the first feasible domain with no used leaf in ranked() order."""
    cap, occ = tallies if tallies is not None else O.place_c(p)[1:]
    fl = [np.asarray(f, dtype=np.int64) for f in p.topology.first_leaf]
    feas, sc = feasibility(p, cap, occ), scores(p, terms, cap)
    J = p.n_jobs
    assign, score = np.full(J, -1, dtype=np.int32), np.zeros(J, dtype=np.uint32)
    used = np.zeros(p.topology.n_leaves, dtype=bool)
    for j in range(J):
        c = int(p.job_class[j])
        f = fl[p.classes[c].level]
        ucs = np.concatenate([[0], np.cumsum(used)])
        cand = np.nonzero(feas[c] & ((ucs[f[1:]] - ucs[f[:-1]]) == 0))[0]
        if cand.size:
            d = int(ranked(cand, sc[c])[0])
            used[f[d]:f[d + 1]] = True
            assign[j], score[j] = d, sc[c][d]
    return assign, score, dict(jobs=J, placed=int((assign >= 0).sum()), runs=int(job_runs(p.job_class)[0].shape[0]),
                               fused=7, score=int(score.astype(np.int64).sum()))


def problem(first_leaf, rows_per_leaf, classes, W=1, R=1, seed=0):
    """bind_ref.nested with seeded rows: label bits 0..3 of W words, taint bit 0 on a fifth of the
    rows, 0..6 free units of R resources, every 41st leaf's rows held by another job."""
    rng = np.random.default_rng(1000 + seed)
    N = int(np.sum(rows_per_leaf))
    leaf_of = np.repeat(np.arange(len(rows_per_leaf)), rows_per_leaf)
    p = nested(first_leaf, rows_per_leaf, classes, [], taints=rng.random(N) < 0.2,
               excl=np.where(leaf_of % 41 == 40, 900, -1), free=rng.integers(0, 7, (R, N)))
    p.nodes.labels = rng.integers(0, 16, (W, N)).astype(np.uint64)
    return p


def seeded_terms(C, seed):
    """3 terms for each of C classes over label bits 0..3 of word 0: one required, at most one forbidden."""
    r = np.random.default_rng(5000 + seed).integers
    return [(c // 3, int(r(1, 101)), (1 << int(r(0, 4)),), ((1 << int(r(0, 4))) * int(r(0, 2)),)) for c in range(3 * C)]


def sweep(seed):  # gang_ref.sweep_case's problem with label bits 0..3 of word 0 at random, and seeded terms
    p = sweep_case(seed)[0]
    p.nodes.labels[0] |= np.random.default_rng(seed).integers(0, 16, p.nodes.n_nodes).astype(np.uint64)
    return p, seeded_terms(len(p.classes), seed)
