"""The launch-shape thresholds of jsp_place as data (DESIGN.md section 4
"Launch-shape thresholds and their tests"): one deterministic Problem per side
of each threshold, and the plan (Engine.last_plan() fields) that side must take.

A plain module, no engine: tests/test_dispatch.py checks on the oracle that no
case passes vacuously, tests/test_dispatch_gpu.py runs them on the GPU.

Build rules: one-row leaves unless the pair is about rows per leaf; rows that
differ by selector bit, taint, free capacity and occupancy, so the classes
differ in feasibility; the last row clean for every class; more jobs than
domains, so some run walks to the last bitmap word of its level.

The plans are literals worked out from the constants of jsp_internal.h and
the predicates of jsp_engine.cc, for an MI355X (256 CUs: the one-set wave
tally holds up to 256 * 24 wave tiles)."""
from __future__ import annotations

from dataclasses import asdict, dataclass, field, replace
from typing import Dict, List, Optional, Tuple

import numpy as np

from jobset_amd.snapshot import JobClass, Nodes, Problem, Topology

# Engine.last_plan() codes (jsplace_bench.h)
IN_TILE, WAVE_ONE, WAVE_DB, BLOCK = 0, 1, 2, 3
WALK_NONE, LEVEL, ASSIGN, FUSED_TAIL, COMPACT, HOST, SPLIT_HOST = 0, 1, 2, 3, 4, 5, 6

MAX_TAKEN_WORDS = 16384  # kMaxTakenWords


@dataclass(frozen=True)
class Dims:
    """Everything a side is built from; the sides of a pair differ in one field."""
    leaves: int = 1000                      # leaves (one row each unless `sizes` says otherwise)
    upper: Tuple[int, ...] = ()             # domains of the levels above the leaves, coarsest first
    sizes: Tuple[Tuple[int, int], ...] = () # (leaf, rows) overrides of the one-row rule (0: empty)
    empty_from: int = 0                     # leaves [empty_from, empty_from + empty_n) are empty
    empty_n: int = 0
    classes: int = 2
    levels: Tuple[int, ...] = ()            # class c's level is levels[c % len]; (): the leaf level
    runs: int = 32
    jobs: int = 0                           # 0: the domains of the first class's level + 37
    fused: bool = False                     # JSP_FUSED_AUTO (else the three-launch shape)
    service: bool = False
    tally: bool = True                      # ask for the tallies (keeps the service and shape 8 out)
    hooks: str = ""                         # JSP_TEST_HOOKS at the snapshot upload


@dataclass(frozen=True)
class Side:
    dims: Dims
    plan: Dict[str, int]
    # the plan through jsp_place_device where it differs: the device path never wants tallies, so
    # under AUTO it takes the split tiles for one request (shape 8) from 256 to 65,536 jobs
    device_plan: Optional[Dict[str, int]] = None

    @property
    def on_device(self) -> Dict[str, int]:
        return self.plan if self.device_plan is None else self.device_plan


@dataclass(frozen=True)
class Case:
    name: str
    axis: str          # A..G of the issue
    dim: str           # the Dims field the sides differ in
    sides: Tuple[Side, ...]
    device: bool = field(default=False)  # also through jsp_place_device


def topology(d: Dims) -> Topology:
    L = d.leaves
    fls = [np.arange(L + 1, dtype=np.int64)]
    for D in reversed(d.upper):  # each level's boundaries are a subset of the finer level's
        finer = fls[0]
        fls.insert(0, finer[(np.arange(D + 1, dtype=np.int64) * (finer.shape[0] - 1)) // D])
    K = len(fls)
    return Topology(level_keys=[f"k{k}" for k in range(K)], n_domains=[int(f.shape[0] - 1) for f in fls],
                    first_leaf=[f.astype(np.uint32) for f in fls])


def build(d: Dims) -> Problem:
    topo = topology(d)
    K, L = topo.n_levels, d.leaves
    rows = np.ones(L, dtype=np.int64)
    rows[d.empty_from:d.empty_from + d.empty_n] = 0
    for leaf, n in d.sizes:
        rows[leaf] = n
    ls = np.zeros(L + 1, dtype=np.uint32)
    np.cumsum(rows, out=ls[1:])
    N = int(ls[-1])
    i = np.arange(N, dtype=np.int64)
    labels = np.full((1, N), ~np.uint64(0), dtype=np.uint64)
    labels[0] &= ~(np.uint64(1) << (i % 61).astype(np.uint64))  # row i lacks selector bit i % 61
    taints = (i % 11 == 5).astype(np.uint32)                    # tainted rows: odd classes tolerate them
    free = ((i * 7) % 9).astype(np.uint32)[None, :].copy()      # 0..8 against a request of 2 x 2 pods
    excl = np.where(i % 17 == 3, 7, -1).astype(np.int32)        # occupied rows
    labels[0, N - 1], taints[N - 1], free[0, N - 1], excl[N - 1] = ~np.uint64(0), 0, 8, -1
    nodes = Nodes(leaf_start=ls, labels=labels, taints=taints, free=free, excl=excl)
    lv = d.levels or (K - 1,)
    # 2 pods on a leaf; above the leaves about what a domain's rows hold on average (16 / 9 a row), so that
    # the rows a class cannot use decide
    pods = [2 if k == K - 1 else max(2, int(1.9 * L / topo.n_domains[k])) for k in range(K)]
    classes = [JobClass(req_labels=(1 << (c % 61),), tolerated_taints=c & 1, level=lv[c % len(lv)],
                        pods=pods[lv[c % len(lv)]], req_res=(2,)) for c in range(d.classes)]
    J = d.jobs or topo.n_domains[classes[0].level] + 37
    run_len = np.full(d.runs, J // d.runs, dtype=np.int64)
    run_len[:J % d.runs] += 1
    job_class = np.repeat(np.arange(d.runs, dtype=np.int64) % d.classes, run_len).astype(np.uint32)
    return Problem(topology=topo, nodes=nodes, classes=classes, job_class=job_class)


PATCH_OWNER = 9


def patched(p: Problem, assign: np.ndarray) -> Tuple[int, Problem]:
    """The one-row patch of the GPU test: the first row of the domain that the
    last placed job of `assign` (p's answer) took becomes occupied by another
    exclusive job, so that domain is infeasible for every class and the answer
    must change. Returns the row and the patched problem (p is not touched)."""
    j = int(np.nonzero(assign >= 0)[0][-1])
    k = p.classes[int(p.job_class[j])].level
    fl = p.topology.first_leaf[k]
    d = int(assign[j])
    ls = p.nodes.leaf_start
    row = int(ls[int(fl[d])])
    assert row < int(ls[int(fl[d + 1])])  # a placed domain has rows
    n = p.nodes
    excl = n.excl.copy()
    excl[row] = PATCH_OWNER
    nodes = Nodes(leaf_start=n.leaf_start, labels=n.labels, taints=n.taints, free=n.free, excl=excl)
    return row, Problem(topology=p.topology, nodes=nodes, classes=p.classes, job_class=p.job_class)


def _pair(name, axis, dim, base: Dims, a, b, plan_a, plan_b, device=False, dev_a=None, dev_b=None) -> Case:
    return Case(name, axis, dim, (Side(replace(base, **{dim: a}), plan_a, dev_a),
                                  Side(replace(base, **{dim: b}), plan_b, dev_b)), device)


def _s8(groups, cpg, **kw):
    """The split tiles launched for one request, the walk on the host."""
    return dict(shape=8, walker=SPLIT_HOST, tally=IN_TILE, groups=groups, cpg=cpg, **kw)


def _one(name, axis, dims: Dims, plan, device=False) -> Case:
    return Case(name, axis, "", (Side(dims, plan),), device)


def _lvl(wpt, nt, **kw):
    return dict(shape=0, walker=LEVEL, level_wpt=wpt, level_threads=nt, **kw)


def _cases() -> List[Case]:
    out: List[Case] = []
    wave = dict(tally=WAVE_ONE, tally_passes=1, folded=1)
    blk1 = dict(tally=BLOCK, tally_passes=1, folded=0)

    # ---- A. level walker templates (three launches, one level, 32 runs)
    a = Dims()
    out += [
        _pair("A_256_1024", "A", "leaves", a, 16384, 16385, _lvl(1, 256, **wave), _lvl(1, 1024, **wave), True),
        _pair("A_w1_w2", "A", "leaves", a, 65536, 65537, _lvl(1, 1024, **wave), _lvl(2, 1024, **wave), True),
        # 2049 words: assign_kernel, the bitmaps of 2 classes staged (stage: (160 KiB - 75324 B) / 4, whole waves)
        _pair("A_w2_assign", "A", "leaves", a, 131072, 131073, _lvl(2, 1024, **wave),
              dict(shape=0, walker=ASSIGN, feas_in_lds=1, topo_in_lds=0, stage_cap=22080, **wave), True),
        # the walker's 128 KiB of LDS: C x threads x words x 8 B
        _pair("A_lds_1024", "A", "classes", replace(a, leaves=16385), 16, 17, _lvl(1, 1024, **blk1),
              dict(shape=0, walker=ASSIGN, feas_in_lds=1, tally=BLOCK, tally_passes=2), True),
        _pair("A_lds_2x1024", "A", "classes", replace(a, leaves=65537), 8, 9, _lvl(2, 1024, **blk1),
              dict(shape=0, walker=ASSIGN, feas_in_lds=1, tally=BLOCK, tally_passes=1), True),
        # 64 classes fit the 256-thread walker alone; one word more and not even assign_kernel stages them
        _pair("A_c64", "A", "leaves", replace(a, classes=64), 16384, 16385, _lvl(1, 256, tally=BLOCK, tally_passes=4),
              dict(shape=0, walker=ASSIGN, feas_in_lds=0, stage_cap=32768, tally=BLOCK, tally_passes=4), True),
        # plan_assign's staging: 6 x 2049 words fit beside kMinStage, 7 x 2049 do not
        _pair("A_stage", "A", "classes", replace(a, leaves=131073), 6, 7,
              dict(shape=0, walker=ASSIGN, feas_in_lds=1), dict(shape=0, walker=ASSIGN, feas_in_lds=0, stage_cap=30272),
              True),
        # the walker at level 0 of two: 70,000 domains of 1-2 leaves (1094 words, no fold above the leaves)
        _one("A_upper", "A", replace(a, leaves=105000, upper=(70000,), levels=(0,)),
             _lvl(2, 1024, tally=WAVE_ONE, tally_passes=1, folded=0), True),
    ]

    # ---- B. runs
    out += [
        _pair("B_off", "B", "runs", replace(a, leaves=4096), 32, 33, _lvl(1, 256, **wave),
              dict(shape=0, walker=ASSIGN, feas_in_lds=1, **wave), True),
        # AUTO, too many row blocks for the fused launch, J >= 256: the level walker, or the walk on the host
        _pair("B_auto", "B", "runs", replace(a, leaves=70000, jobs=60000, fused=True), 32, 33, _lvl(2, 1024, **wave),
              dict(shape=7, walker=HOST, **wave), True),
    ]

    # ---- C. jobs (two levels, classes on both: no level walker)
    c = Dims(leaves=300, upper=(20,), levels=(1, 0), runs=4, fused=True)
    fused = dict(shape=1, walker=FUSED_TAIL, tally=IN_TILE, groups=1)
    host = dict(shape=7, walker=HOST, tally=WAVE_ONE, folded=0)
    split = dict(shape=8, walker=SPLIT_HOST, tally=IN_TILE, groups=1)
    nt = replace(c, tally=False)
    out += [
        _pair("C_min", "C", "jobs", c, 255, 256, fused, host, True, None, split),
        _pair("C_max", "C", "jobs", c, 65536, 65537, host, fused, True, split, None),
        _pair("C_min_split", "C", "jobs", nt, 255, 256, fused, split, True),
        _pair("C_max_split", "C", "jobs", nt, 65536, 65537, split, fused, True),
    ]

    # ---- D. the fused launch (AUTO, one level, 32 runs: the level walker is the alternative)
    f = Dims(fused=True)
    ft = dict(shape=1, walker=FUSED_TAIL, tally=IN_TILE)
    out += [
        _pair("D_c16", "D", "classes", f, 16, 17, dict(groups=4, cpg=4, **ft), _lvl(1, 256, tally=BLOCK, tally_passes=2),
              True, _s8(4, 4), _s8(4, 5)),
        # past kHostWalkMaxJobs the device path has no split tiles either: fused_ok's limits decide there too
        _pair("D_c16_far", "D", "classes", replace(f, jobs=70000), 16, 17, dict(groups=4, cpg=4, **ft),
              _lvl(1, 256, tally=BLOCK, tally_passes=2), True),
        _pair("D_blocks", "D", "leaves", f, 65536, 65537, dict(n_blocks=256, groups=1, **ft),
              _lvl(2, 1024, n_blocks=257, **wave), True),
        # 17 x 361 = 6137 words fit kFusedMaxWords, 17 x 362 = 6154 do not
        _pair("D_words", "D", "leaves", replace(f, classes=16), 23104, 23105, dict(groups=1, **ft),
              _lvl(1, 1024, **blk1), True, _s8(1, 16), _s8(1, 16)),
        _pair("D_words_far", "D", "leaves", replace(f, classes=16, jobs=70000), 23104, 23105, dict(groups=1, **ft),
              _lvl(1, 1024, **blk1), True),
        _pair("D_g1_g2", "D", "classes", f, 2, 3, dict(groups=1, cpg=2, **ft), dict(groups=2, cpg=2, **ft), True,
              _s8(1, 2), _s8(2, 2)),
        _pair("D_g2_g3", "D", "classes", f, 4, 5, dict(groups=2, cpg=2, **ft), dict(groups=3, cpg=2, **ft), True,
              _s8(2, 2), _s8(3, 2)),
        _pair("D_g3_g4", "D", "classes", f, 6, 7, dict(groups=3, cpg=2, **ft), dict(groups=4, cpg=2, **ft), True,
              _s8(3, 2), _s8(4, 2)),
    ]
    f8 = replace(f, classes=8, hooks="block_rows=60")  # 60 one-row leaves per block: groups <= 128 / blocks
    for nb, ga, gb in ((32, 4, 3), (42, 3, 2), (64, 2, 1)):  # (the split tiles group alike: 8 classes over the groups)
        out.append(_pair(f"D_tiles_{nb}", "D", "leaves", f8, 60 * nb, 60 * nb + 1,
                         dict(n_blocks=nb, groups=ga, **ft), dict(n_blocks=nb + 1, groups=gb, **ft), True,
                         _s8(ga, (8 + ga - 1) // ga, n_blocks=nb), _s8(gb, (8 + gb - 1) // gb, n_blocks=nb + 1)))
    out += [
        # the hierarchy tables: (100 + 1) child starts + L parents against kFusedTopoMax = 8192 words
        _pair("D_topo", "D", "leaves", replace(f, upper=(100,)), 8091, 8092, dict(topo_in_lds=1, fscr_words=0, **ft),
              dict(topo_in_lds=0, fscr_words=0, **ft), True, _s8(1, 2), _s8(1, 2)),
        # classes above the leaves: 2 x 100 sums + 2 words of occupancy bits of scratch
        _pair("D_fscr", "D", "levels", replace(f, upper=(100,)), (1,), (0,), dict(topo_in_lds=1, fscr_words=0, **ft),
              dict(topo_in_lds=1, fscr_words=202, **ft), True, _s8(1, 2), None),
    ]

    # ---- E. the services (AUTO, no tallies)
    s = Dims(fused=True, service=True, tally=False)
    out += [
        # the same choice on the launch path (service off): the compaction launch, or the split tiles for one request
        _pair("E_launch", "E", "classes", replace(s, service=False), 1, 2, dict(shape=2, walker=COMPACT, tally=IN_TILE),
              dict(shape=8, walker=SPLIT_HOST, groups=1), True),
        _pair("E_compact_split", "E", "classes", s, 1, 2, dict(shape=3, walker=COMPACT), dict(shape=5, walker=SPLIT_HOST)),
        _pair("E_leaf_upper", "E", "levels", replace(s, classes=1, upper=(100,)), (1,), (0,),
              dict(shape=3, walker=COMPACT), dict(shape=5, walker=SPLIT_HOST, groups=1)),
        # kSvcMaxBlocks: 255 tiles and the dispatcher are resident; one block more and svc_shape has no service
        # shape, so the launch path answers (no service was tried: svc_fallbacks stays 0)
        _pair("E_blocks_compact", "E", "leaves", replace(s, classes=1, hooks="block_rows=60"), 255 * 60, 255 * 60 + 1,
              dict(shape=3, walker=COMPACT, n_blocks=255), dict(shape=2, walker=COMPACT, tally=IN_TILE, n_blocks=256)),
        _pair("E_blocks_split", "E", "leaves", replace(s, classes=2, hooks="block_rows=60"), 255 * 60, 255 * 60 + 1,
              dict(shape=5, walker=SPLIT_HOST, groups=1, n_blocks=255),
              dict(shape=1, walker=FUSED_TAIL, tally=IN_TILE, groups=1, n_blocks=256)),
        # 64 classes: 4 groups of 16 up to 32 blocks; 3 groups of 22 are refused, the launch path answers
        _pair("E_c64", "E", "leaves", replace(s, classes=64, hooks="block_rows=60"), 1920, 1921,
              dict(shape=5, walker=SPLIT_HOST, groups=4, cpg=16, n_blocks=32),
              _lvl(1, 256, tally=BLOCK, tally_passes=4, n_blocks=33)),
    ]

    # ---- F. tally kernels (three launches)
    out.append(_pair("F_c4_c5", "F", "classes", a, 4, 5, _lvl(1, 256, **wave), _lvl(1, 256, **blk1)))
    for ca, cb, pa in ((16, 17, 1), (32, 33, 2), (48, 49, 3)):
        out.append(_pair(f"F_pass{pa}", "F", "classes", a, ca, cb, _lvl(1, 256, tally=BLOCK, tally_passes=pa),
                         _lvl(1, 256, tally=BLOCK, tally_passes=pa + 1)))
    big = replace(a, leaves=40, empty_from=7, empty_n=1)
    out += [
        # a leaf at the wave tile's 252 rows, and one past it (no wave tiles: the workgroup tally)
        _pair("F_leaf252", "F", "sizes", big, ((9, 252),), ((9, 253),), _lvl(1, 256, **wave),
              _lvl(1, 256, n_wtiles=0, **blk1)),
        # a leaf at the block's 1,020 rows, one past it, and one of three chunks
        _pair("F_leaf1020", "F", "sizes", big, ((9, 1020),), ((9, 1021),), _lvl(1, 256, n_wtiles=0, n_blocks=3, **blk1),
              _lvl(1, 256, n_wtiles=0, n_blocks=3, **blk1)),
        _one("F_leaf2049", "F", replace(big, sizes=((9, 2049),)), _lvl(1, 256, n_wtiles=0, n_blocks=3, **blk1)),
        _pair("F_tile64", "F", "leaves", a, 64, 65, _lvl(1, 256, n_wtiles=1, **wave), _lvl(1, 256, n_wtiles=2, **wave)),
        _pair("F_blk256", "F", "leaves", replace(a, hooks="tally_block=1"), 256, 257, _lvl(1, 256, n_blocks=1, **blk1),
              _lvl(1, 256, n_blocks=2, **blk1)),
        # 257 empty leaves in a row: a whole block (and four whole wave tiles) without a row
        _pair("F_empty257", "F", "classes", replace(a, leaves=700, empty_from=300, empty_n=257), 4, 5,
              _lvl(1, 256, **wave), _lvl(1, 256, **blk1)),
        _one("F_double", "F", replace(a, hooks="tally_one=0"), _lvl(1, 256, tally=WAVE_DB, tally_passes=1, folded=1)),
    ]

    # ---- G. the taken-set limit: exactly kMaxTakenWords words over all levels
    out += [
        _one("G_flat", "G", replace(a, leaves=64 * MAX_TAKEN_WORDS),
             dict(shape=0, walker=ASSIGN, feas_in_lds=0, stage_cap=1600, tally=WAVE_DB, tally_passes=1, folded=1)),
        _one("G_three", "G", replace(a, leaves=64 * 16000, upper=(64 * 64, 64 * 320), levels=(2, 1, 0)),
             dict(shape=0, walker=ASSIGN, feas_in_lds=0, topo_in_lds=0, tally=WAVE_DB, tally_passes=1, folded=0)),
    ]
    return out


CASES: List[Case] = _cases()
# one word more than G_three: refused at the topology upload (JSP_ERANGE)
G_OVER = replace(CASES[-1].sides[0].dims, upper=(64 * 64 + 1, 64 * 320))

# what the GPU run must see at least once (test_dispatch_gpu.py's last test)
REQUIRED_SHAPES = {0, 1, 2, 3, 5, 7, 8}


def sides() -> List[Tuple[str, int]]:
    return [(c.name, i) for c in CASES for i in range(len(c.sides))]


def case(name: str) -> Case:
    return next(c for c in CASES if c.name == name)


def differing(c: Case) -> List[str]:
    if len(c.sides) < 2:
        return []
    a, b = asdict(c.sides[0].dims), asdict(c.sides[1].dims)
    return [k for k in a if a[k] != b[k]]
