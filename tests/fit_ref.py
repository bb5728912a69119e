"""The yardstick of the fit-placement tests (DESIGN.md §2 "Fit placement"):
the rule taken literally over the CPU oracle's tallies. It never calls the
engine.

cap / occ come from oracle.place_c. capsum is an int64 sum by cumulative
sums, fit its clamp at 0xFFFFFFFF, and every job takes the argmin of
(key, d) over the feasible domains of its class's level none of whose leaves
is used (a take marks every intersecting domain at every level, and two
domains of a nested hierarchy intersect iff they share a leaf).

Also here: order_ref, the candidate lists in the engine's layout, and the
hand cases of the tests."""
import numpy as np

from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from bind_ref import cls, flat, nested
from gang_ref import feasibility, reduction_problem, sweep_case  # noqa: F401  (the tests' inputs)

LOWEST, TIGHTEST, ROOMIEST = 0, 1, 2
POLICIES = (LOWEST, TIGHTEST, ROOMIEST)
CLAMP = 0xFFFFFFFF
TAIL = 0xFFFFFFFF


def fits(p, cap):
    """fit[c]: int64 [D[level[c]]], min(capsum(c, d), 0xFFFFFFFF)."""
    out = []
    for c, jc in enumerate(p.classes):
        fl = np.asarray(p.topology.first_leaf[jc.level], dtype=np.int64)
        cs = np.concatenate([[0], np.cumsum(cap[c].astype(np.int64))])
        out.append(np.minimum(cs[fl[1:]] - cs[fl[:-1]], CLAMP))
    return out


def keys_of(fit, policy):
    if policy == LOWEST:
        return np.zeros_like(fit)
    return fit if policy == TIGHTEST else CLAMP - fit


def _tallies(p, tallies):
    return tallies if tallies is not None else O.place_c(p)[1:]


def fit_ref(p, policy, tallies=None):
    """fit_ref_literal's answer for large batches (config4's 40,000 jobs): the
    same argmin per job, over a per-class array of (key << 32 | d) in which a
    take overwrites the domains that share a leaf with it (every class's range
    of intersecting domains, by searchsorted on first_leaf) instead of
    recomputing every domain's used-leaf count per job. tests/test_fit.py
    checks it against fit_ref_literal on every small input."""
    assert policy in POLICIES
    cap, occ = _tallies(p, tallies)
    topo = p.topology
    fl = [np.asarray(f, dtype=np.int64) for f in topo.first_leaf]
    feas = feasibility(p, cap, occ)
    fit = fits(p, cap)
    gone = np.uint64(0xFFFFFFFFFFFFFFFF)
    work = []
    for c in range(len(p.classes)):
        comp = (keys_of(fit[c], policy).astype(np.uint64) << np.uint64(32)) | np.arange(fit[c].shape[0], dtype=np.uint64)
        work.append(np.where(feas[c], comp, gone))
    levels = [jc.level for jc in p.classes]
    J = p.n_jobs
    assign = np.full(J, -1, dtype=np.int32)
    used = np.zeros(topo.n_leaves, dtype=bool)
    slack = 0
    for j in range(J):
        c = int(p.job_class[j])
        w = work[c]
        if w.shape[0] == 0:
            continue
        d = int(w.argmin())
        if w[d] == gone:
            continue
        a, b = int(fl[levels[c]][d]), int(fl[levels[c]][d + 1])
        assert not used[a:b].any()
        used[a:b] = True
        assign[j] = d
        slack += int(fit[c][d]) - min(int(p.classes[c].pods), CLAMP)
        for c2, k2 in enumerate(levels):  # the domains [lo, hi) of level k2 that share a leaf with [a, b)
            lo = int(np.searchsorted(fl[k2][1:], a, side="right"))
            hi = int(np.searchsorted(fl[k2][:-1], b, side="left"))
            work[c2][lo:hi] = gone
    stats = dict(jobs=J, placed=int((assign >= 0).sum()), runs=int(job_runs(p.job_class)[0].shape[0]), fused=7,
                 slack=slack)
    return assign, stats


def fit_ref_literal(p, policy, tallies=None):
    """(assign [J], stats dict) of the rule for problem p (jobs p.job_class in
    global order). tallies: (cap, occ) of O.place_c(p)."""
    assert policy in POLICIES
    cap, occ = _tallies(p, tallies)
    topo = p.topology
    fl = [np.asarray(f, dtype=np.int64) for f in topo.first_leaf]
    feas = feasibility(p, cap, occ)
    fit = fits(p, cap)
    key = [keys_of(f, policy) for f in fit]
    J = p.n_jobs
    assign = np.full(J, -1, dtype=np.int32)
    used = np.zeros(topo.n_leaves, dtype=bool)
    slack = 0
    for j in range(J):
        c = int(p.job_class[j])
        f = fl[p.classes[c].level]
        a, b = f[:-1], f[1:]
        ucs = np.concatenate([[0], np.cumsum(used)])
        cand = np.nonzero(feas[c] & ((ucs[b] - ucs[a]) == 0))[0]
        if cand.size == 0:
            continue
        d = int(cand[np.lexsort((cand, key[c][cand]))[0]])  # the smallest (key, d)
        used[a[d]:b[d]] = True
        assign[j] = d
        slack += int(fit[c][d]) - min(int(p.classes[c].pods), CLAMP)
    stats = dict(jobs=J, placed=int((assign >= 0).sum()), runs=int(job_runs(p.job_class)[0].shape[0]), fused=7,
                 slack=slack)
    return assign, stats


def order_ref(p, policy, tallies=None):
    """(order uint32 [sum of D[level[c]]], nf uint32 [C]) in the engine's
    layout: class c's segment follows those of the classes before it, its nf[c]
    feasible domains in ascending (key, d) first, 0xFFFFFFFF behind them."""
    cap, occ = _tallies(p, tallies)
    feas = feasibility(p, cap, occ)
    fit = fits(p, cap)
    order, nf = [], []
    for c in range(len(p.classes)):
        cand = np.nonzero(feas[c])[0]
        cand = cand[np.lexsort((cand, keys_of(fit[c], policy)[cand]))]
        seg = np.full(feas[c].shape[0], TAIL, dtype=np.uint32)
        seg[:cand.shape[0]] = cand
        order.append(seg)
        nf.append(cand.shape[0])
    return (np.concatenate(order) if order else np.zeros(0, dtype=np.uint32)), np.array(nf, dtype=np.uint32)


def fitv_ref(p, tallies=None):
    """fit(c, d) in the order lists' layout (by domain id), uint32."""
    cap, _ = _tallies(p, tallies)
    f = fits(p, cap)
    return np.concatenate(f).astype(np.uint32) if f else np.zeros(0, dtype=np.uint32)


def stats_dict(st):
    return dict(jobs=int(st.jobs), placed=int(st.placed), runs=int(st.runs), fused=int(st.fused), slack=int(st.slack))


# ---- hand cases: name -> (problem, {policy: assign})
def hand_cases():
    return {
        # a small job on the big rack strands it: best fit places both
        "A": (flat([8, 2, 4, 2], [cls(0, 2), cls(0, 6)], [0, 1]),
              {LOWEST: [0, -1], TIGHTEST: [1, 0], ROOMIEST: [0, -1]}),
        # ties go to the lowest id, in both directions
        "B": (flat([4, 2, 2, 4], [cls(0, 2)], [0] * 5),
              {LOWEST: [0, 1, 2, 3, -1], TIGHTEST: [1, 2, 0, 3, -1], ROOMIEST: [0, 3, 1, 2, -1]}),
        # two levels: a rack job, a zone job, a rack job; marks cross the levels
        "C": (nested([[0, 3, 5], np.arange(6)], [4, 1, 4, 2, 2], [cls(1, 2), cls(0, 4)], [0, 1, 0]),
              {LOWEST: [0, 1, 2], TIGHTEST: [3, 0, 4], ROOMIEST: [0, 1, 2]}),
        # the clamp: capsums 3 * 2^31 and 5 * 2^31 both clamp to 0xFFFFFFFF and tie, 2^31 does not
        "D": (nested([[0, 3, 8, 9], np.arange(10)], [1] * 9, [cls(0, 1 << 31, req=0)], [0, 0, 0]),
              {LOWEST: [0, 1, 2], TIGHTEST: [2, 0, 1], ROOMIEST: [0, 1, 2]}),
        # D inside the engine's contract (pods <= 2^22, a leaf's sum of cap < 2^32; jsp_classes_upload refuses
        # D's 2^31 pods): 512 rows of 2^22 per leaf give the same per-leaf tallies, capsums and answers
        "D22": (nested([[0, 3, 8, 9], np.arange(10)], [512] * 9, [cls(0, 1 << 22, req=0)], [0, 0, 0]),
                {LOWEST: [0, 1, 2], TIGHTEST: [2, 0, 1], ROOMIEST: [0, 1, 2]}),
    }
