"""Seeded call sequences on one engine against a plain host model.

Every call of the ABI has a suite of its own that loads a problem and checks
one call. This module drives ONE engine through a long mixed script -- row
patches of every size, assume / forget, re-uploads, service mode changes, idle
gaps, and every placement and planner call in between -- and compares every
reply with a model that carries the same state on the host: a Problem copy
the mutating ops are applied to with numpy, and the references the per-call
suites already use (oracle.place_c, sticky_ref, gang_ref, fit_ref, spread_ref,
preempt_ref, whatif_ref, bind_ref, assume_ref / forget_ref, explain_ref, and
row_domain below for the two webhook calls). A stale table, a patch one
reader does not wait for, or a call that moves something it promises to
leave, fails at a named step of a named seed.

    script(seed, world)   -> (Problem, [op, ...])     ops are plain dicts
    expected(problem, ops) -> [reply, ...]             host only
    replay(engine, problem, ops, replies, ...)         engine only

Scripts are dealt from a deck (deck()) so that the coverage conditions
tests/test_call_sequences.py asserts hold by construction: the script of seed
s takes rotation s % 12, and the twelve rotations together put every reading
kind directly behind a patch, an assume, a forget and every planner kind.
Every script also holds two fixed blocks: place, assume, a reader, place,
forget, a reader, place (owners held and released with nothing in between
that writes the owner column; the last placement differs from the one in
front of the forget), and place, a one-row patch of a domain it gave out,
fit (the patch is still held back for the next request when fit reads).

Worlds: `launch` (gang_ref.sweep_case's problem, service off), `split` (the
same, service AUTO), `compact` (its first class moved to the leaf level, all
jobs of it, service AUTO: the compaction service and the host lease answer),
`set` (the launch problem on a device-set engine).

A row patch carries a non-empty subset of the four columns (a patch without
a column writes nothing) over distinct rows in any order. jsp_place is asked
for the whole batch, its first job, no job, the batch with tallies, and the
batch repeated up to TILED_JOBS jobs: from 256 jobs on the launch path walks
a batch of several levels on the host (stats.fused 7 or 8), which none of
these small problems' own batches reaches.

    python tests/call_sequences.py --seed S --world W [--upto K]

replays the first K ops on a fresh engine, for looking at one failing step.
"""
import dataclasses
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from jobset_amd import synth  # noqa: E402
from jobset_amd.snapshot import Nodes, job_runs  # noqa: E402
from oracle import oracle as O  # noqa: E402

import assume_ref  # noqa: E402
import bind_ref  # noqa: E402
import explain_ref  # noqa: E402
import fit_ref  # noqa: E402
import gang_ref  # noqa: E402
import preempt_ref  # noqa: E402
import spread_ref  # noqa: E402
import sticky_ref  # noqa: E402
import whatif_ref  # noqa: E402

WORLDS = ("launch", "split", "compact", "set")
READ = ("place", "place_device", "sticky", "gangs", "fit", "spread", "preempt", "whatif", "bind", "explain",
        "resolve", "audit")
PLANNER = ("sticky", "gangs", "fit", "spread", "preempt", "whatif", "bind")
SET_READ = ("place", "explain", "resolve", "audit")
MUTATING = ("patch", "assume", "forget", "classes", "reupload", "service", "sleep")
ROW_READERS = tuple(k for k in READ if k not in ("resolve", "audit"))
SIZES = ("one", "two", "few", "many", "all")
PLACE_VARIANTS = ("all", "first", "none", "tally", "tiled")
TILED_JOBS = 300                         # past the 256 jobs from which the launch path walks on the host
ROTATIONS = 12

FIRST_OWNER = 0x40000000
NOBODY = 0x7F000001                      # an owner id that never holds a row
EINVAL, ESTATE = -1, -4

# the jsp_metrics totals the model carries (svc_* and the histograms' sums are timing)
METRICS = ("place_us.count", "batch_jobs.count", "placed", "unplaceable", "place_errors", "patch_us.count",
           "patch_errors")

# Twelve seeds per world, one per rotation of the deck (seed % 12), taken from
# gang_ref's sweep seeds 0-59: those whose problem neither places every job nor
# none, so that the replies can differ (tests/test_call_sequences.py).
SEEDS = {
    "launch": (36, 13, 2, 3, 16, 29, 6, 19, 8, 33, 10, 59),
    "split": (36, 13, 2, 3, 16, 29, 6, 19, 8, 33, 10, 47),
    "compact": (48, 13, 14, 3, 4, 29, 6, 43, 20, 33, 34, 47),
    "set": (12, 13, 2, 3, 4, 29, 6, 7, 8, 33, 34, 47),
}

IDLE_S = float(os.environ.get("JSP_SERVICE_IDLE_MS", "50")) / 1e3


# ---------------------------------------------------------------- the webhook calls' reference
def row_domain(p, rows, levels):
    """int32 [n]: the domain at levels[i] of row rows[i]; -1 for a row below 0
    or past the snapshot and for a level the topology does not have."""
    rows, levels = np.asarray(rows, dtype=np.int64).reshape(-1), np.asarray(levels, dtype=np.int64).reshape(-1)
    ok = (rows >= 0) & (rows < p.nodes.n_nodes) & (levels < p.topology.n_levels)
    leaf = np.searchsorted(np.asarray(p.nodes.leaf_start, dtype=np.int64), np.where(ok, rows, 0), side="right") - 1
    out = np.full(rows.shape, -1, dtype=np.int32)
    for k in range(p.topology.n_levels):
        m = ok & (levels == k)
        out[m] = np.searchsorted(np.asarray(p.topology.first_leaf[k], dtype=np.int64), leaf[m], side="right") - 1
    return out


def audit_ref(p, rows, levels, off, fd):
    """uint32 [n]: the followers of job i whose domain differs from the
    leader's, 0xFFFFFFFF where the leader has none."""
    ld = row_domain(p, rows, levels)
    off, fd = np.asarray(off, dtype=np.int64), np.asarray(fd, dtype=np.int64)
    return np.array([0xFFFFFFFF if ld[i] < 0 else int((fd[off[i]:off[i + 1]] != ld[i]).sum())
                     for i in range(ld.shape[0])], dtype=np.uint32)


# ---------------------------------------------------------------- seeded draws
class Draws:
    """synth's counter-based draws, one fresh stream per call."""

    def __init__(self, seed):
        self.seed, self.stream = int(seed), 0

    def _next(self):
        self.stream += 1
        return self.stream

    def ints(self, n, lo, hi):
        return synth.uniform_int(self.seed, self._next(), int(n), int(lo), int(hi))

    def one(self, lo, hi):
        return int(self.ints(1, lo, hi)[0])

    def coins(self, n, p):
        return synth.bernoulli(self.seed, self._next(), int(n), p)

    def perm(self, n):
        return synth.permutation(self.seed, self._next(), int(n))

    def raw(self, n):
        return synth.draws(self.seed, self._next(), int(n))


# ---------------------------------------------------------------- worlds
def world_problem(seed, world):
    """(problem, gang_jobs, gang_span) of a world's script."""
    p, gang_jobs, gang_span = gang_ref.sweep_case(seed)
    if world == "compact":
        from test_service_gpu import one_leaf_class    # the service suite's reduction to the compaction shape
        p = dataclasses.replace(one_leaf_class(p), name=p.name + "-compact")
    return p, gang_jobs, gang_span


def split_shape(seed):
    """A `split` seed's problem has at least 2 classes or at least 2 levels."""
    p = gang_ref.sweep_case(seed)[0]
    return len(p.classes) >= 2 or p.topology.n_levels >= 2


def copy_nodes(n):
    return Nodes(leaf_start=n.leaf_start, labels=n.labels.copy(), taints=n.taints.copy(), free=n.free.copy(),
                 excl=n.excl.copy(), leaf_begin=n.leaf_begin)


# ---------------------------------------------------------------- the model
class Model:
    """The engine's state on the host: the snapshot's columns, the classes,
    the metrics totals, and what the argument builders aim with (the last
    whole-batch placement, the owners assume handed out)."""

    def __init__(self, p, gang_jobs, gang_span):
        self.p = dataclasses.replace(p, nodes=copy_nodes(p.nodes), classes=list(p.classes), job_names=None)
        self.base = np.ascontiguousarray(p.job_class, dtype=np.uint32)
        self.gang_jobs, self.gang_span = np.asarray(gang_jobs), np.asarray(gang_span)
        self.last = None
        self.held = []
        self.next_owner = FIRST_OWNER
        self.met = dict.fromkeys(METRICS, 0)
        self.top = p.nodes.free.max(axis=1).astype(np.int64)
        self.leaf = p.nodes.leaf_of_row()

    def view(self, jobs):
        return dataclasses.replace(self.p, job_class=np.ascontiguousarray(jobs, dtype=np.uint32))

    def _placement(self, jobs, placed, ok=True):
        self.met["place_us.count"] += 1
        if not ok:
            self.met["place_errors"] += 1
            return
        self.met["batch_jobs.count"] += 1
        self.met["placed"] += int(placed)
        self.met["unplaceable"] += int(jobs) - int(placed)

    # -- one op: the reply, and the state after it
    def apply(self, op):
        return getattr(self, "_" + op["kind"])(op)

    def _patch(self, op):
        n, rows = self.p.nodes, np.asarray(op["rows"], dtype=np.int64)
        if op.get("labels") is not None:
            n.labels[:, rows] = op["labels"]
        if op.get("taints") is not None:
            n.taints[rows] = op["taints"]
        if op.get("free") is not None:
            n.free[:, rows] = op["free"]
        if op.get("excl") is not None:
            n.excl[rows] = op["excl"]
        self.met["patch_us.count"] += 1
        return None

    def _assume(self, op):
        new, committed, stats = assume_ref.assume_ref(self.view(op["jobs"]), op["assign"], op["owner"])
        self.p.nodes.excl[:] = new
        self.held += [int(o) for o in np.asarray(op["owner"])[committed]]
        return dict(committed=committed, stats=stats)

    def _forget(self, op):
        new, cleared = assume_ref.forget_ref(self.p.nodes.excl, op["owners"])
        self.p.nodes.excl[:] = new
        gone = set(int(o) for o in op["owners"])
        self.held = [o for o in self.held if o not in gone]
        return dict(cleared=cleared)

    def _classes(self, op):
        self.p.classes = list(op["classes"])
        return None

    def _reupload(self, op):
        n = self.p.nodes
        self.p.nodes = Nodes(leaf_start=n.leaf_start, labels=op["labels"].copy(), taints=op["taints"].copy(),
                             free=op["free"].copy(), excl=op["excl"].copy(), leaf_begin=n.leaf_begin)
        self.held = []
        return None

    def _service(self, op):
        return None

    def _sleep(self, op):
        return None

    def _refusal(self, op):
        if op["family"] in ("place", "sticky", "gangs", "fit", "spread"):
            self._placement(0, 0, ok=False)
        if op["family"] == "patch":
            self.met["patch_us.count"] += 1
            self.met["patch_errors"] += 1
        return dict(code=op["code"])

    def _place(self, op):
        q = self.view(op["jobs"])
        a, cap, occ = O.place_c(q)
        out = dict(assign=a.copy(), stats=dict(jobs=q.n_jobs, placed=int((a >= 0).sum()),
                                               runs=int(job_runs(q.job_class)[0].shape[0])))
        if op["tally"]:
            out.update(cap=cap.copy(), occ=occ.copy())
        if q.n_jobs == self.base.shape[0]:
            self.last = a.copy()
        self._placement(q.n_jobs, out["stats"]["placed"])
        return out

    def _place_device(self, op):
        return dict(assign=O.place_c(self.view(op["jobs"]))[0].copy())

    def _sticky(self, op):
        q = self.view(op["jobs"])
        a, kept = sticky_ref.sticky_ref(q, op["prev"])
        stats = dict(jobs=q.n_jobs, placed=int((a >= 0).sum()), hinted=int((np.asarray(op["prev"]) >= 0).sum()),
                     kept=int(kept.sum()), runs=int(job_runs(q.job_class)[0].shape[0]))
        self._placement(q.n_jobs, stats["placed"])
        return dict(assign=a, stats=stats)

    def _gangs(self, op):
        q = self.view(op["jobs"])
        a, span = gang_ref.gang_ref(q, op["gang_jobs"], op["gang_span"])
        stats = dict(jobs=q.n_jobs, placed=int((a >= 0).sum()), gangs=len(op["gang_jobs"]),
                     gangs_placed=int((span >= 0).sum()),
                     runs=int(gang_ref.gang_runs_of(q.job_class, op["gang_jobs"])[0].shape[0]))
        self._placement(q.n_jobs, stats["placed"])
        return dict(assign=a, span=span, stats=stats)

    def _fit(self, op):
        q = self.view(op["jobs"])
        a, stats = fit_ref.fit_ref_literal(q, op["policy"])
        stats = {k: v for k, v in stats.items() if k != "fused"}
        self._placement(q.n_jobs, stats["placed"])
        return dict(assign=a, stats=stats)

    def _spread(self, op):
        q = self.view(op["jobs"])
        a, sp, cnt, stats, _ = spread_ref.spread_ref(q, op["level"], op["max_skew"], op["peers"])
        stats = {k: v for k, v in stats.items() if k != "fused"}
        self._placement(q.n_jobs, stats["placed"])
        return dict(assign=a, spread=sp, count=cnt, stats=stats)

    def _preempt(self, op):
        q = self.view(op["jobs"])
        a, off, vic, stats = preempt_ref.preempt_ref(q, op["prio"], op["owners"], op["ranks"], op["evict_free"])
        return dict(assign=a, victim_off=off, victims=vic, stats={k: v for k, v in stats.items() if k != "fused"})

    def _whatif(self, op):
        q = self.view(op["jobs"])
        a, placed, flips, _, _ = whatif_ref.whatif_ref(q, op["scenarios"])
        stats = dict(jobs=q.n_jobs, scenarios=len(op["scenarios"]),
                     rows=int(sum(len(sc["rows"]) for sc in op["scenarios"])),
                     runs=int(job_runs(q.job_class)[0].shape[0]), flips=int(flips))
        return dict(assign=a, placed=placed, stats=stats)

    def _bind(self, op):
        pod_row, pod_off, stats = bind_ref.bind_ref(self.view(op["jobs"]), op["assign"])
        return dict(pod_row=pod_row, pod_off=pod_off, stats=stats)

    def _explain(self, op):
        return dict(records=explain_ref.reference(self.p)[0])

    def _resolve(self, op):
        return dict(domains=row_domain(self.p, op["rows"], op["levels"]))

    def _audit(self, op):
        return dict(bad=audit_ref(self.p, op["rows"], op["levels"], op["off"], op["fd"]))


# ---------------------------------------------------------------- argument builders
def _values(m, d, rows, aimed=False):
    """Column values for `rows`: labels, taints, free [R, n], excl. Owners come
    leaf by leaf (a fifth of the leaves held), so that a large patch leaves
    domains to place in; a taint is 16 bits wide, now and then one nobody
    tolerates. aimed: the first row loses everything a class could want -- a
    taint nobody tolerates, no free resource, an owner."""
    n, nd = rows.shape[0], m.p.nodes
    lab = np.stack([d.raw(n) & d.raw(n) | d.raw(n) for _ in range(nd.n_label_words)])
    tn = np.where(d.coins(n, 0.2), np.where(d.coins(n, 0.15), 1 << 20, d.ints(n, 0, 0xFFFF)), 0).astype(np.uint32)
    fr = np.stack([d.ints(n, 0, int(m.top[r])) for r in range(nd.n_res)]).astype(np.uint32)
    held = d.coins(m.p.topology.n_leaves, 0.2)
    leaf = m.leaf[rows]
    ex = np.where(held[leaf], 900 + leaf, -1).astype(np.int32)
    if aimed:
        tn[0], fr[:, 0], ex[0] = 1 << 20, 0, 900 + leaf[0]
    return lab, tn, fr, ex


def _patch_rows(m, d, size):
    """The rows of a patch of a size class, distinct, in any order. A small
    patch starts with a row of a domain the last whole-batch placement gave
    out (where it gave one out), so that the next reader's answer depends on it."""
    N = m.p.nodes.n_nodes
    order = d.perm(N)
    if size in ("one", "two", "few") and m.last is not None and (m.last >= 0).any():
        placed = np.nonzero(m.last >= 0)[0]
        j = int(placed[d.one(0, placed.shape[0] - 1)])
        r0, r1 = bind_ref.domain_rows(m.p, m.p.classes[int(m.base[j])].level, int(m.last[j]))
        if r1 > r0:
            row = r0 + d.one(0, r1 - r0 - 1)
            order = np.concatenate([[row], order[order != row]])
    if size == "one":
        return order[:1]
    if size == "two":  # two rows in two leaves (where the snapshot has two leaves with rows)
        other = order[m.leaf[order] != m.leaf[order[0]]]
        return np.concatenate([order[:1], other[:1] if other.size else order[1:2]])
    if size == "few":
        return order[:min(N, d.one(3, 16))]
    if size == "many":
        return order[:min(N, d.one(280, 320))]
    return order


def build(kind, arg, m, d, world):
    """One op of `kind` aimed at the model's state now."""
    p = m.p
    N, K, C = p.nodes.n_nodes, p.topology.n_levels, len(p.classes)
    if kind == "patch":
        size, mask = arg
        rows = _patch_rows(m, d, size).astype(np.uint32)
        lab, tn, fr, ex = _values(m, d, rows.astype(np.int64), aimed=size in ("one", "two", "few"))
        return dict(kind="patch", size=size, mask=mask, rows=rows, labels=lab if mask & 1 else None, taints=tn if mask & 2 else None,
                    free=fr if mask & 4 else None, excl=ex if mask & 8 else None)
    if kind == "assume":
        keep = d.coins(m.base.shape[0], 0.5)
        assign = np.where(keep, m.last, -1).astype(np.int32)
        owner = (m.next_owner + np.arange(m.base.shape[0])).astype(np.int32)
        m.next_owner += m.base.shape[0]
        return dict(kind="assume", jobs=m.base, assign=assign, owner=owner)
    if kind == "forget":
        held = np.array(m.held, dtype=np.int64)
        some = held[d.coins(held.shape[0], 0.8)] if held.size else held
        if held.size and not some.size:
            some = held[:1]
        owners = np.concatenate([some, [NOBODY], some[:1] if some.size else [NOBODY]]).astype(np.int32)
        return dict(kind="forget", owners=owners)
    if kind == "classes":
        c = d.one(0, C - 1)
        sizes = np.diff(np.asarray(p.nodes.leaf_start, dtype=np.int64))
        pods = d.one(1, max(1, int(sizes.max()) // 2))
        if pods == p.classes[c].pods:
            pods = pods % max(1, int(sizes.max()) // 2) + 1
        classes = list(p.classes)
        classes[c] = dataclasses.replace(classes[c], pods=pods)
        return dict(kind="classes", classes=classes)
    if kind == "reupload":
        lab, tn, fr, ex = _values(m, d, np.arange(N, dtype=np.int64))
        return dict(kind="reupload", labels=lab, taints=tn, free=fr, excl=ex)
    if kind == "service":
        return dict(kind="service", mode=arg)
    if kind == "sleep":
        return dict(kind="sleep")
    if kind == "refusal":
        code = ESTATE if world == "set" and arg in PLANNER + ("assume", "forget") else EINVAL
        args = build(arg, d.one(0, 2) if arg == "fit" else None, m, d, world) if arg in PLANNER else None
        return dict(kind="refusal", family=arg, code=code, args=args)
    if kind == "place":
        jobs = {"all": m.base, "tally": m.base, "first": m.base[:1], "none": m.base[:0],
                "tiled": np.resize(m.base, TILED_JOBS)}[arg]
        return dict(kind="place", variant=arg, jobs=jobs, tally=arg == "tally")
    if kind == "place_device":
        return dict(kind="place_device", jobs=m.base)
    if kind == "sticky":
        prev = m.last.astype(np.int32).copy()
        hit = d.ints(prev.shape[0], 0, 2) == 0
        gone = d.coins(prev.shape[0], 0.5)
        Dj = np.array([p.topology.n_domains[p.classes[int(c)].level] for c in m.base], dtype=np.int64)
        moved = (d.raw(prev.shape[0]) % Dj.astype(np.uint64)).astype(np.int32)
        prev[hit] = np.where(gone, -1, moved)[hit]
        return dict(kind="sticky", jobs=m.base, prev=prev)
    if kind == "gangs":
        return dict(kind="gangs", jobs=m.base, gang_jobs=m.gang_jobs, gang_span=m.gang_span)
    if kind == "fit":
        return dict(kind="fit", jobs=m.base, policy=int(arg))
    if kind == "spread":
        s = next((k for k in range(K) if p.topology.n_domains[k] > 1), 0)
        ok = np.array([p.classes[int(c)].level >= s for c in m.base], dtype=bool)
        if not ok.any():
            s, ok = 0, np.ones(m.base.shape[0], dtype=bool)
        owners = spread_ref.owners_of(p)
        peers = np.concatenate([owners[d.coins(owners.shape[0], 0.5)], [NOBODY]]).astype(np.int32)
        return dict(kind="spread", jobs=m.base[ok], level=s, max_skew=(1, 0, 1, 3)[d.one(0, 3)], peers=peers)
    if kind == "preempt":
        owners = spread_ref.owners_of(p)
        owners = owners[~d.coins(owners.shape[0], 0.15)]
        ranks = d.ints(owners.shape[0], 0, 3).astype(np.uint32)
        ef = None
        if d.one(0, 1):
            ef = np.maximum(p.nodes.free.astype(np.int64), (m.top * 3 // 4)[:, None]).astype(np.uint32)
        return dict(kind="preempt", jobs=m.base, prio=(1, 2, 4)[d.one(0, 2)], owners=owners, ranks=ranks, evict_free=ef)
    if kind == "whatif":
        scen = []
        for i in range(d.one(1, 4)):
            if i == 2:
                scen.append(whatif_ref.EMPTY)
                continue
            rows = np.sort(d.perm(N)[:min(N, d.one(1, 40))])
            lab, tn, fr, ex = _values(m, d, rows)
            scen.append(whatif_ref.edit(p, rows, labels=lab, taints=tn, free_res=fr, excl_owner=ex))
        return dict(kind="whatif", jobs=m.base, scenarios=scen)
    if kind == "bind":
        return dict(kind="bind", jobs=m.base, assign=m.last.astype(np.int32).copy())
    if kind == "explain":
        return dict(kind="explain")
    if kind in ("resolve", "audit"):
        n = d.one(1, 300) if kind == "resolve" else d.one(1, 40)
        rows = d.ints(n, 0, N - 1).astype(np.int32)
        edge = np.array([-1, N, N - 1, 0, -(1 << 31)], dtype=np.int64)
        pick = d.coins(n, 0.15)
        rows[pick] = edge[d.ints(n, 0, edge.shape[0] - 1)][pick].astype(np.int32)
        levels = d.ints(n, 0, K).astype(np.uint32)          # K itself: no such level
        if kind == "resolve":
            return dict(kind="resolve", rows=rows, levels=levels)
        cnt = np.array([0, 1, 3, 63, 64, 65, 200], dtype=np.int64)[d.ints(n, 0, 6)]
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        ld = np.repeat(row_domain(p, rows, levels), cnt)
        how = d.ints(ld.shape[0], 0, 9)
        fd = np.where(how == 0, -1, np.where(how == 1, ld + 1, ld)).astype(np.int32)
        return dict(kind="audit", rows=rows, levels=levels, off=off, fd=fd)
    raise ValueError(kind)


# ---------------------------------------------------------------- the deck
def deck(world, rot):
    """The (kind, argument) list of rotation `rot` (0..11) of a world, as
    segments that stay together; script() shuffles the segments."""
    read = SET_READ if world == "set" else READ
    planner = () if world == "set" else PLANNER
    resident = world in ("split", "compact")
    n = len(read)

    def reader(i, variant="all"):
        k = read[i % n]
        if k == "place":
            return ("place", variant)
        if k == "fit":
            return ("fit", (rot + i) % 3)
        return (k, None)

    opening = [("place", "all")] * (3 if resident else 2)
    segs = []
    # every reading kind directly behind a patch (the three larger sizes reach every kind over the twelve
    # rotations), an assume, a forget; every patch with its own subset of the columns, all 15 four times a world
    for k, size in enumerate(SIZES):
        patch = ("patch", (size, 1 + (5 * rot + k + 1) % 15))   # (the one-row patch never labels alone)
        if k == 0 and world != "set":
            # a placement that finds or brings the service up, one row of a domain it gave out, and a fit at
            # once: the patch is still held back for the next request when the fit reads the rows
            segs.append([("place", "all"), patch, ("fit", (rot + 1) % 3)])
        else:
            segs.append([patch, reader(rot + 2 * k + 1)])
    if world != "set":
        # The owners of a fresh placement assumed and, two calls on, forgotten, with nothing in between that
        # writes the owner column. The placement in front of the forget is answered with the service up, so
        # the lease holds its answer: the forget must give it up, and the placement at the end shows it.
        segs.append([("place", "all"), ("assume", None), reader(rot), ("place", "all"), ("forget", None),
                     reader(rot + 5), ("place", "all")])
    segs.append([("classes", None)])
    segs.append([("reupload", None)])
    # every reading kind directly behind every other planner kind
    for k, x in enumerate(planner):
        others = [r for r in read if r != x]
        y = others[(rot + k) % len(others)]
        yi = read.index(y)
        segs.append([("fit", rot % 3) if x == "fit" else (x, None), reader(yi, PLACE_VARIANTS[(rot + k) % 5])])
    if world != "set":
        segs.append([("fit", (rot + 2) % 3)])
        segs.append([("place", PLACE_VARIANTS[1 + rot % 4])])
        segs.append([("sleep", None)])
        fam = ("place", "patch") + PLANNER + ("assume", "forget")
        # (every family at least once a world: 11 families, 12 rotations)
        segs += [[("refusal", fam[(rot + 6 * t) % len(fam)])] for t in range(1 if resident else 2)]
    else:
        # (jsp_place in every form a device set serves: one job, no job, with tallies, the repeated batch)
        segs += [[reader(rot + t, PLACE_VARIANTS[1 + (rot + t // 4) % 4])] for t in range(8)]
        segs += [[("refusal", f)] for f in PLANNER + ("place", "patch")]
    if resident:
        which = rot % 3
        if which == 0:
            segs.append([("service", "off"), ("place", "all"), ("service", "auto")])
            segs.append([("service", "stop"), ("place", "all")])
        elif which == 1:
            segs.append([("service", "stop"), ("place", "all")])
            segs.append([("service", "parked"), ("place", "all"), ("service", "stop"), ("service", "auto")])
        else:
            segs.append([("service", "off"), ("place", "all"), ("service", "parked"), ("place", "all"),
                         ("service", "stop"), ("service", "auto")])
    elif world == "launch":
        segs.append([("service", "off")])
        segs.append([("service", "stop")])
    return opening, segs, [("service", "stop")]


def script(seed, world):
    """(Problem, ops): the script of `seed` in `world`. The arguments are aimed
    at the model's state at each step, so the model walks along."""
    assert world in WORLDS
    p, gang_jobs, gang_span = world_problem(seed, world)
    d = Draws(31_000_000 + 1000 * WORLDS.index(world) + seed)
    opening, segs, closing = deck(world, seed % ROTATIONS)
    order = [segs[i] for i in d.perm(len(segs))]
    m = Model(p, gang_jobs, gang_span)
    ops = []
    for kind, arg in opening + [x for s in order for x in s] + closing:
        op = build(kind, arg, m, d, world)
        m.apply(op)
        ops.append(op)
    return p, ops


def expected(problem, ops):
    """The reply of every op (None where a call returns nothing), on the host alone."""
    m = Model(problem, [], [])
    return [m.apply(op) for op in ops]


def expected_totals(problem, ops):
    """How far the ops move the jsp_metrics totals the model carries (METRICS)."""
    m = Model(problem, [], [])
    for op in ops:
        m.apply(op)
    return dict(m.met)


# ---------------------------------------------------------------- comparing
def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and a and not isinstance(a[0], (int, np.integer)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, str) or dataclasses.is_dataclass(a):
        return a == b
    x, y = np.asarray(a), np.asarray(b)
    wide = np.uint64 if np.uint64 in (x.dtype, y.dtype) else np.int64
    return x.shape == y.shape and bool(np.array_equal(x.astype(wide), y.astype(wide)))


def brief(op):
    """An op in one line: its kind and its small arguments."""
    out = [op["kind"]]
    for k, v in op.items():
        if k in ("kind", "args") or v is None:
            continue
        if isinstance(v, np.ndarray):
            out.append(f"{k}[{'x'.join(str(s) for s in v.shape)}]" if v.size > 6 else f"{k}={v.tolist()}")
        elif isinstance(v, (int, str)):
            out.append(f"{k}={v}")
        elif isinstance(v, list):
            out.append(f"{k}({len(v)})")
    return " ".join(out)


class SequenceError(AssertionError):
    pass


# ---------------------------------------------------------------- the replay
def setup(engine, world):
    """The world's service mode and launch shapes (a device-set engine has neither)."""
    if world == "set":
        return
    engine.set_service(world in ("split", "compact"))
    engine.set_fused(True)


def _metrics(engine):
    x = engine.metrics()
    return {"place_us.count": int(x.place_us.count), "batch_jobs.count": int(x.batch_jobs.count),
            "placed": int(x.placed), "unplaceable": int(x.unplaceable), "place_errors": int(x.place_errors),
            "patch_us.count": int(x.patch_us.count), "patch_errors": int(x.patch_errors)}


def _stats(st, names):
    return {k: int(getattr(st, k)) for k in names}


def _explain_dict(x):
    names = ("rows", "rows_selector", "rows_taint", "rows_no_capacity", "rows_fit", "rows_occupied", "domains",
             "dom_occupied", "dom_short", "dom_feasible", "best_short_cap", "best_short_domain")
    out = {f: int(getattr(x, f)) for f in names}
    out["rows_insufficient"] = [int(v) for v in x.rows_insufficient]
    return out


def _refuse(engine, op):
    """The refused call of an op's family: flags = 1 or a run class out of
    range on a single engine, the call as it is on a device set."""
    fam, a = op["family"], op["args"]
    C = engine.n_classes
    bad_runs = (np.array([C], dtype=np.uint32), np.array([1], dtype=np.uint32))
    flags = 0 if op["code"] == ESTATE else 1
    if fam == "place":
        return engine.place(np.array([C], dtype=np.uint32))
    if fam == "patch":
        n = engine.nodes.n_nodes
        return engine.patch_rows(np.array([0, n], dtype=np.uint32), taints=np.zeros(2, dtype=np.uint32))
    if fam == "sticky":
        if op["code"] == ESTATE:
            return engine.place_sticky(a["jobs"], a["prev"])
        return engine.place_sticky_runs(*bad_runs, None)
    rc, rl = job_runs(a["jobs"]) if a is not None and "jobs" in a else (None, None)
    if fam == "gangs":
        grc, grl, gr = gang_ref.gang_runs_of(a["jobs"], a["gang_jobs"])
        return engine.place_gangs_runs(grc, grl, gr, a["gang_span"], flags=flags)
    if fam == "fit":
        return engine.place_fit_runs(rc, rl, a["policy"], flags=flags)
    if fam == "spread":
        return engine.place_spread_runs(rc, rl, a["level"], a["max_skew"], a["peers"], flags=flags)
    if fam == "preempt":
        return engine.place_preempt_runs(rc, rl, a["prio"], a["owners"], a["ranks"], a["evict_free"], flags=flags)
    if fam == "whatif":
        so, rows, lab, tn, fr, ex = whatif_ref.concat(a["scenarios"])
        return engine.place_whatif_runs(rc, rl, so, rows, lab, tn, fr, ex, flags=flags)
    if fam == "bind":
        return engine.bind_pods_runs(rc, rl, a["assign"], flags=flags)
    if fam == "assume":
        jobs = np.zeros(1, dtype=np.uint32)
        return engine.assume_runs(*job_runs(jobs), np.array([-1], dtype=np.int32), np.array([5], dtype=np.int32),
                                  flags=flags)
    if fam == "forget":
        return engine.forget(np.array([5, -1] if op["code"] == EINVAL else [5], dtype=np.int32))
    raise ValueError(fam)


class _Device:
    """The device buffers of a script's place_device ops, made before the
    first engine call (a pageable copy can stall behind a resident service)."""

    def __init__(self, ops):
        import torch
        self.torch = torch
        self.side = torch.cuda.Stream()
        self.buf = {}
        for i, op in enumerate(ops):
            if op["kind"] == "place_device":
                rc, rl = job_runs(op["jobs"])
                J = int(op["jobs"].shape[0])
                self.buf[i] = (torch.from_numpy(rc.astype(np.int32)).cuda(), torch.from_numpy(rl.astype(np.int32)).cuda(),
                               torch.full((max(J, 1),), -7, dtype=torch.int32, device="cuda"),
                               torch.empty(max(J, 1), dtype=torch.int32).pin_memory(), rc.shape[0], J)
        if self.buf:
            torch.cuda.current_stream().synchronize()

    def place(self, engine, i):
        torch = self.torch
        rct, rlt, out, host, n_runs, J = self.buf[i]
        with torch.cuda.stream(self.side):  # torch's current stream, and not the null stream
            engine.place_device(rct.data_ptr(), rlt.data_ptr(), n_runs, J, out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
            host.copy_(out, non_blocking=True)
        self.side.synchronize()
        return host.numpy()[:J].copy()


def run_op(engine, op, i, dev):
    """(reply, fused or None) of one op on the engine."""
    k = op["kind"]
    if k == "patch":
        engine.patch_rows(op["rows"], labels=op["labels"], taints=op["taints"], free=op["free"], excl=op["excl"])
        return None, None
    if k == "assume":
        committed, st = engine.assume(op["jobs"], op["assign"], op["owner"])
        return dict(committed=committed, stats=assume_ref.stats_dict(st)), None
    if k == "forget":
        return dict(cleared=engine.forget(op["owners"])), None
    if k == "classes":
        engine.upload_classes(op["classes"])
        return None, None
    if k == "reupload":
        n = engine.nodes
        engine.upload_snapshot(Nodes(leaf_start=n.leaf_start, labels=op["labels"], taints=op["taints"], free=op["free"],
                                     excl=op["excl"], leaf_begin=n.leaf_begin))
        return None, None
    if k == "service":
        if op["mode"] == "stop":
            engine.service_stop()
        else:
            engine.set_service(op["mode"] != "off", parked=op["mode"] == "parked")
        return None, None
    if k == "sleep":
        time.sleep(1.6 * IDLE_S)
        return None, None
    if k == "refusal":
        from jobset_amd.native import JspError
        try:
            _refuse(engine, op)
        except JspError as e:
            return dict(code=int(e.code)), None
        return dict(code=0), None
    if k == "place":
        r = engine.place(op["jobs"], want_tally=op["tally"])
        out = dict(assign=r.assign, stats=dict(jobs=r.jobs, placed=r.placed, runs=r.runs))
        if op["tally"]:
            out.update(cap=r.cap, occ=r.occ)
        return out, r.fused
    if k == "place_device":
        return dict(assign=dev.place(engine, i)), None
    if k == "sticky":
        a, st = engine.place_sticky(op["jobs"], op["prev"])
        return dict(assign=a, stats=_stats(st, ("jobs", "placed", "hinted", "kept", "runs"))), int(st.fused)
    if k == "gangs":
        rc, rl, gr = gang_ref.gang_runs_of(op["jobs"], op["gang_jobs"])
        a, span, st = engine.place_gangs_runs(rc, rl, gr, op["gang_span"])
        return dict(assign=a, span=span, stats=_stats(st, ("jobs", "placed", "gangs", "gangs_placed", "runs"))), \
            int(st.fused)
    if k == "fit":
        a, st = engine.place_fit(op["jobs"], op["policy"])
        return dict(assign=a, stats=_stats(st, ("jobs", "placed", "runs", "slack"))), int(st.fused)
    if k == "spread":
        a, sp, cnt, st = engine.place_spread(op["jobs"], op["level"], op["max_skew"], op["peers"])
        return dict(assign=a, spread=sp, count=cnt,
                    stats=_stats(st, ("jobs", "placed", "refused", "skew", "runs"))), int(st.fused)
    if k == "preempt":
        a, off, vic, st = engine.place_preempt(op["jobs"], op["prio"], op["owners"], op["ranks"], op["evict_free"])
        return dict(assign=a, victim_off=off, victims=vic,
                    stats=_stats(st, ("jobs", "placed", "preempting", "victims", "runs"))), int(st.fused)
    if k == "whatif":
        a, placed, st = engine.place_whatif(op["jobs"], op["scenarios"])
        return dict(assign=a, placed=placed, stats=_stats(st, ("jobs", "scenarios", "rows", "runs", "flips"))), \
            int(st.fused)
    if k == "bind":
        pod_row, pod_off, st = engine.bind_pods(op["jobs"], op["assign"])
        return dict(pod_row=pod_row, pod_off=pod_off, stats=bind_ref.stats_dict(st)), None
    if k == "explain":
        return dict(records=[_explain_dict(x) for x in engine.explain()]), None
    if k == "resolve":
        return dict(domains=engine.resolve_leader_domains(op["rows"], op["levels"])), None
    if k == "audit":
        return dict(bad=engine.audit_placements(op["rows"], op["levels"], op["off"], op["fd"])), None
    raise ValueError(k)


def replay(engine, problem, ops, replies, totals=None, seed=None, world=None, upto=None):
    """Load the problem and run the ops back to back, every reply compared with
    `replies` (all computed beforehand: the service stays up and the lease
    held between ops). Stops at the first mismatch or error and raises; at the
    end the metrics must have moved by `totals`. Returns who answered, per op:
    (kind, fused or None, answers the lease gave during the op)."""
    from jobset_amd.native import JspError
    ops = ops if upto is None else ops[:upto]
    engine.load(problem)
    dev = _Device(ops) if any(op["kind"] == "place_device" for op in ops) else None
    m0 = _metrics(engine)
    lease = world != "set"
    l0 = engine.lease_counters()["answered"] if lease else 0
    who, since = [], []

    def fail(i, what):
        return SequenceError(f"seed {seed} world {world} op {i}: {brief(ops[i])}: {what}; mutating ops since the last "
                             f"reply that matched: {since or 'none'}")

    for i, (op, want) in enumerate(zip(ops, replies)):
        try:
            got, fused = run_op(engine, op, i, dev)
        except JspError as e:
            raise fail(i, f"JspError {e}") from None
        if not same(got, want):
            diff = [k for k in (want or {}) if not same((got or {}).get(k), want[k])]
            show = lambda r: str({k: (r or {}).get(k) for k in diff})[:600]  # noqa: E731
            raise fail(i, f"the reply differs from the model in {diff}: got {show(got)}, want {show(want)}")
        l1 = engine.lease_counters()["answered"] if lease else 0
        who.append((op["kind"], fused, l1 - l0))
        l0 = l1
        if op["kind"] in MUTATING:
            since.append(f"{i}:{brief(op)}")
        elif want is not None and op["kind"] != "refusal":
            since = []
    if totals is not None and upto is None:
        m1 = _metrics(engine)
        moved = {k: m1[k] - m0[k] for k in METRICS}
        if moved != totals:
            raise SequenceError(f"seed {seed} world {world}: the metrics moved by {moved}, the model's by {totals}")
    return who


def main(argv=None):
    import argparse
    from jobset_amd.engine import Engine
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--world", choices=WORLDS, required=True)
    ap.add_argument("--upto", type=int, default=None, help="replay the first K ops only")
    a = ap.parse_args(argv)
    p, ops = script(a.seed, a.world)
    replies, totals = expected(p, ops), expected_totals(p, ops)
    eng = Engine(devices=[0, 0, 0]) if a.world == "set" else Engine(0)
    try:
        setup(eng, a.world)
        t0 = time.perf_counter()
        try:
            who = replay(eng, p, ops, replies, totals, seed=a.seed, world=a.world, upto=a.upto)
        finally:
            eng.service_stop()
        dt = time.perf_counter() - t0
        for i, (kind, fused, leased) in enumerate(who):
            print(f"{i:3d} {brief(ops[i])}" + (f"  fused={fused}" if fused is not None else "") +
                  (f"  lease+{leased}" if leased else ""))
        print(f"seed {a.seed} world {a.world}: {len(who)} ops matched the model in {dt:.2f} s")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
