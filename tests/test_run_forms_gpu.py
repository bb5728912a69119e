"""Raw run lists on every placement path of the GPU (tests/run_forms.py;
DESIGN.md section 4.2b "Raw run lists"): the forms a caller sends -- adjacent
runs of one class, empty runs, runs of one job, thousands of runs -- through
jsp_place, jsp_place_device, jsp_tally_device + jsp_assign_device, the
resident services, the device set, and the entry points that take runs
(sticky, fit, gangs, bind, assume). Every answer is compared with the per-job
reference of the canonical problem (oracle.place_c, tests/*_ref.py), which is
the same for every form of one job sequence. There is no tolerance.

Every placement checks assign[], placed == (a >= 0).sum(), stats.jobs == J,
stats.runs == n_runs as passed (empty runs included) and, where tallies are
requested, cap and occ. After every host-API call (stats.fused,
last_plan()["walker"]) must be what the engine's own predicates give for that
n_runs and J (want_path: level_walk_ok, host_walk_ok, split_oneshot_ok,
compact_ok restated), so no form is quietly answered by an easier path; the
last test checks the set of paths seen with a non-canonical form.

The snapshots are dispatch_cases.build's (rows that differ per class, the
last row clean, more jobs than domains) with runs=8, so canonical runs are
about 130 jobs long and the forms to32 / to33 exist."""
import contextlib
import dataclasses
import functools

import numpy as np
import pytest

import dispatch_cases as DC
import run_forms as RF
from dispatch_cases import ASSIGN, COMPACT, FUSED_TAIL, HOST, LEVEL, SPLIT_HOST, Dims
from jobset_amd import synth
from jobset_amd.engine import Engine
from jobset_amd.native import JSP_EHIP, JSP_EINVAL, JspError
from oracle import oracle as O
from assume_ref import assume_ref
from assume_ref import stats_dict as assume_stats
from bind_ref import bind_ref
from bind_ref import stats_dict as bind_stats
from fit_ref import ROOMIEST, TIGHTEST, fit_ref
from fit_ref import stats_dict as fit_stats
from gang_ref import ANY, gang_ref, gang_runs_of
from gang_ref import sweep_case as gang_sweep_case
from sticky_ref import sticky_ref

pytestmark = pytest.mark.gpu

SEEN = set()   # (shape, walker) of every placement of a non-canonical form (the device set: (6, None))
RAN = set()    # cases that ran

ONE = Dims(leaves=1000, classes=2, runs=8)                        # one level, 16 taken words: register mode
WIDE = Dims(leaves=8192, classes=3, runs=8)                       # one level, 128 taken words: the bitmaps in LDS
TWO = Dims(leaves=300, upper=(20,), levels=(1, 0), runs=4)        # two levels, classes on both
TWO_WIDE = Dims(leaves=6000, upper=(64,), levels=(1, 0), runs=4)  # two levels, 95 taken words
SOLO = Dims(leaves=1000, classes=1, runs=8)                       # one leaf-level class: the compaction shapes


@functools.lru_cache(maxsize=None)
def solved(dims):
    """(problem, oracle answer, cap, occ, forms) of a snapshot, computed once."""
    p = DC.build(dims)
    a, cap, occ = O.place_c(p)
    return p, a, cap, occ, RF.forms(p.job_class, len(p.classes), seed=p.n_jobs)


def want_path(p, n_runs, J, auto, tally, assign_only=False):
    """(stats.fused, walker) by the engine's predicates (jsp_engine.cc place_impl
    / assign_impl) for a whole small snapshot: one row per leaf, at most 255
    row blocks, at most 16 classes and 6144 bitmap words, so fused_ok and
    split_ok hold whenever JSP_FUSED_AUTO is set. assign_only: jsp_assign_device."""
    K, C = p.topology.n_levels, len(p.classes)
    lv = [c.level for c in p.classes]
    words = sum((p.topology.n_domains[k] + 63) // 64 for k in lv) + sum((d + 63) // 64 for d in p.topology.n_domains)
    assert p.topology.n_leaves <= 255 * 256 and C <= 16 and words <= 6144
    nw = (p.topology.n_domains[lv[0]] + 63) // 64
    wpt, nt = (1, 256) if nw <= 256 else (1, 1024) if nw <= 1024 else (2, 1024) if nw <= 2048 else (0, 256)
    level_ok = n_runs <= RF.LEVEL_MAX_RUNS and len(set(lv)) == 1 and 1 <= nw and 0 < C * nt * wpt * 8 <= 128 * 1024
    in_host = auto and n_runs > 0 and 256 <= J <= 65536            # kHostWalkMinJobs .. kHostWalkMaxJobs
    if not assign_only:
        if auto and C == 1 and lv[0] + 1 == K:
            return 2, COMPACT                                      # compact_ok
        if in_host and not tally:
            return 8, SPLIT_HOST                                   # split_oneshot_ok
    if in_host and not level_ok:
        return 7, HOST                                             # host_walk_ok
    if auto and not assign_only:
        return 1, FUSED_TAIL                                       # fused_ok
    return 0, (LEVEL if level_ok else ASSIGN)                      # level_walk_ok


def verify(got, a, cap, occ, n_runs, tally, what):
    if tally:
        np.testing.assert_array_equal(got.occ, occ, err_msg=what)
        np.testing.assert_array_equal(got.cap, cap, err_msg=what)
    np.testing.assert_array_equal(got.assign, a, err_msg=what)
    assert got.placed == int((a >= 0).sum()), what
    assert got.jobs == a.shape[0], what
    assert got.runs == n_runs, (what, got.runs, n_runs)


@contextlib.contextmanager
def guarded(engine, monkeypatch, name):
    """A failing case must not leave a doubtful GPU in use: a JSP_EHIP that is
    not a launch the runtime refused on the host ("invalid argument") ends the
    session; the engine's switches are restored whatever happened."""
    RAN.add(name)
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    try:
        yield
    except JspError as err:
        if err.code == JSP_EHIP and "invalid argument" not in str(err):
            pytest.exit(f"{name}: {err}", returncode=3)
        raise
    finally:
        monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
        engine.set_timing(False)
        engine.set_fused(True)
        engine.set_service(True)
        engine.service_stop()


def setup(engine, dims, auto, service=False, jobs=None):
    """The snapshot loaded under the switches; (p, a, cap, occ, forms), with
    `jobs` for the first `jobs` jobs of the snapshot's batch."""
    p, a, cap, occ, fs = solved(dims)
    if jobs is not None:
        p = dataclasses.replace(p, job_class=p.job_class[:jobs].copy(), job_names=None)
        a = O.place_c(p)[0]
        fs = RF.forms(p.job_class, len(p.classes), seed=jobs)
    engine.set_timing(False)
    engine.set_fused(auto)
    engine.set_service(service)
    engine.load(p)
    return p, a, cap, occ, fs


def host_call(engine, p, a, cap, occ, name, form, auto, tally, want=None):
    """One jsp_place of a form: the answer, the stats, and the path."""
    rc, rl, _ = form
    what = f"{name} ({rc.shape[0]} runs, J={a.shape[0]})"
    got = engine.place_runs(rc, rl, want_tally=tally)
    verify(got, a, cap, occ, rc.shape[0], tally, what)
    path = (got.fused, engine.last_plan()["walker"])
    assert path == (want or want_path(p, rc.shape[0], a.shape[0], auto, tally)), (what, path)
    if name != "canonical":
        SEEN.add(path)
    return path


def device_call(engine, p, a, cap, occ, name, form, auto, how):
    """The same list with the run arrays on the device and out[] pre-filled
    with -7, through jsp_place_device (how == "place") or jsp_tally_device +
    jsp_assign_device ("assign"); one spare element behind out[J) stays -7."""
    import torch
    rc, rl, _ = form
    n, J, C, L = rc.shape[0], a.shape[0], len(p.classes), p.topology.n_leaves
    what = f"{name} on the device ({how}; {n} runs, J={J})"
    rct = torch.from_numpy(np.concatenate([rc, [0]]).astype(np.int32)).cuda()
    rlt = torch.from_numpy(np.concatenate([rl, [0]]).astype(np.int32)).cuda()
    out = torch.full((J + 1,), -7, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if how == "place":
        engine.place_device(rct.data_ptr(), rlt.data_ptr(), n, J, out.data_ptr(), s)
        want = want_path(p, n, J, auto, False)
    else:
        ld = L + 3
        dcap = torch.full((C + 1, ld), 77, dtype=torch.int32, device="cuda")
        engine.tally_device(dcap.data_ptr(), dcap[-1].data_ptr(), ld, s)
        engine.assign_device(dcap.data_ptr(), dcap[-1].data_ptr(), ld, rct.data_ptr(), rlt.data_ptr(), n, J,
                             out.data_ptr(), s)
        want = want_path(p, n, J, auto, True, assign_only=True)
    engine.check()
    h = out.cpu().numpy()
    assert h[J] == -7, what
    np.testing.assert_array_equal(h[:J], a, err_msg=what)
    plan = engine.last_plan()
    assert (plan["shape"], plan["walker"]) == want, (what, plan)
    if how == "assign":
        tal = dcap.cpu().numpy().astype(np.uint32)
        np.testing.assert_array_equal(tal[:C, :L], cap, err_msg=what)
        np.testing.assert_array_equal(tal[C, :L], occ, err_msg=what)


def sweep(engine, dims, auto, tally, names=None, jobs=None, device=("place",)):
    """Every named form (None: all) of the snapshot's batch through jsp_place
    and the device paths; returns {form name: path of the host call}."""
    p, a, cap, occ, fs = setup(engine, dims, auto, jobs=jobs)
    out = {}
    for name in names or list(fs):
        out[name] = host_call(engine, p, a, cap, occ, name, fs[name], auto, tally)
        for how in device:
            device_call(engine, p, a, cap, occ, name, fs[name], auto, how)
    return out, fs


# ------------------------------------------------------------------ the cases
def case_level_and_register(engine):
    """Shape 0 on one level of 1000 leaves, three launches: up to 32 runs the
    level walker (its 32-entry LDS run table), above assign_kernel in register
    mode; to33 flips the walker from the to32 call before it."""
    p, a, cap, occ, fs = setup(engine, ONE, False)
    order = ["canonical", "to32", "to33"] + [n for n in fs if n not in ("canonical", "to32", "to33")]
    paths = {}
    for name in order:
        paths[name] = host_call(engine, p, a, cap, occ, name, fs[name], False, True)
        for how in ("place", "assign"):
            device_call(engine, p, a, cap, occ, name, fs[name], False, how)
    assert paths["canonical"] == paths["to32"] == (0, LEVEL) and paths["to33"] == (0, ASSIGN)
    p32 = RF.trimmed(fs["padded"], RF.LEVEL_MAX_RUNS)
    assert p32[0].shape[0] > 8 and (p32[1] == 0).any()
    assert host_call(engine, p, a, cap, occ, "padded32", p32, False, True) == (0, LEVEL)
    device_call(engine, p, a, cap, occ, "padded32", p32, False, "place")
    # a walker that is wrong only behind another form's call: to32, to33, to32 again
    for name in ("to32", "to33", "to32"):
        host_call(engine, p, a, cap, occ, name, fs[name], False, True)
    many = {n for n in fs if fs[n][0].shape[0] > RF.LEVEL_MAX_RUNS}
    assert many >= {"ones", "padded_split", "gap", "to33"}
    assert all(paths[n] == (0, ASSIGN) for n in many)


def case_assign_lds(engine):
    """Shape 0, assign_kernel with the taken bitmaps in LDS (8192 leaves): its
    1024-run tiles, short and long runs side by side, a whole tile of empty runs."""
    names = ["ones", "split64", "split65", "padded_split", "gap"]
    paths, fs = sweep(engine, WIDE, False, True, names, device=("place", "assign"))
    assert set(paths.values()) == {(0, ASSIGN)}
    assert fs["ones"][0].shape[0] > 8 * RF.ASSIGN_TILE
    assert (fs["split64"][1] == 64).any() and (fs["split65"][1] == 65).any()
    assert RF.empty_tile(fs["gap"][1]) >= 0


def case_assign_levels(engine):
    """Shape 0, assign_kernel over two levels: in register mode (300 leaves)
    and with the marks in LDS (6000 leaves), every form."""
    for dims in (TWO, TWO_WIDE):
        paths, _ = sweep(engine, dims, False, True, device=("place", "assign"))
        assert set(paths.values()) == {(0, ASSIGN)}, dims


def case_fused_tail(engine):
    """Shape 1: below kHostWalkMinJobs the fused tail keeps any run count (its
    256-run tiles; the gap form spans several of them)."""
    for dims in (ONE, TWO):
        paths, fs = sweep(engine, dims, True, True, ["ones", "padded_split", "gap"], jobs=200)
        assert set(paths.values()) == {(1, FUSED_TAIL)}, dims
        assert fs["gap"][0].shape[0] > 8 * RF.FUSED_TILE


def case_host_walk(engine):
    """Shape 7 (tallies requested) and shape 8 (none): the walk on the host,
    from 256 jobs on, for more than 32 runs or two levels."""
    for dims in (ONE, TWO):
        paths, fs = sweep(engine, dims, True, True, device=("place", "assign"))
        for name, path in paths.items():
            one_level_few = dims is ONE and fs[name][0].shape[0] <= RF.LEVEL_MAX_RUNS
            assert path == ((1, FUSED_TAIL) if one_level_few else (7, HOST)), (dims, name)
        paths, _ = sweep(engine, dims, True, False, device=())
        assert set(paths.values()) == {(8, SPLIT_HOST)}, dims


def feasible_leaves(p, cap, occ):
    return int(((cap[0] >= p.classes[0].pods) & (occ == 0)).sum())


def case_compaction(engine):
    """Shape 2: one leaf-level class, J below, at and above the feasible leaf
    count. The compaction reads J alone; the list still goes through check_runs
    and the stats."""
    p, _, cap, occ, _ = solved(SOLO)
    nf = feasible_leaves(p, cap, occ)
    assert 3 < nf < p.n_jobs - 3
    for J in (nf - 1, nf, nf + 3):
        paths, _ = sweep(engine, SOLO, True, False, ["canonical", "ones", "gap", "padded"], jobs=J)
        assert set(paths.values()) == {(2, COMPACT)}, J


def through_service(engine, a, cap, occ, name, form, shape, walker):
    """jsp_place until the service answers (the first call after an upload is
    answered on the launch path while the service comes up); every answer on
    the way is checked too."""
    rc, rl, _ = form
    for _ in range(4):
        got = engine.place_runs(rc, rl)
        verify(got, a, cap, occ, rc.shape[0], False, name)
        if got.fused == shape:
            break
    path = (got.fused, engine.last_plan()["walker"])
    assert path == (shape, walker), (name, path)
    if name != "canonical":
        SEEN.add(path)


def case_services(engine):
    """Shapes 3 and 5: the resident compaction and split services. Then forms
    A, B, A of one job sequence back to back inside the lease window and a
    list of the same n_runs and J for another job sequence (the classes of
    `ones` permuted): every answer is its own oracle answer, and the lease's
    counter shows that the host answered at least one of them from the kept
    lines. (The lease belongs to the compaction service, whose one class has
    one job sequence per J: the other sequence goes to the split service.)"""
    p, a, cap, occ, fs = setup(engine, SOLO, True, service=True)
    for name in fs:
        through_service(engine, a, cap, occ, name, fs[name], 3, COMPACT)
    for attempt in range(3):  # (a slow box: the four calls must fit a quarter of the idle limit)
        through_service(engine, a, cap, occ, "ones", fs["ones"], 3, COMPACT)
        before = engine.lease_counters()["answered"]
        for name in ("gap", "ones", "gap", "split_rand"):
            through_service(engine, a, cap, occ, name, fs[name], 3, COMPACT)
        if engine.lease_counters()["answered"] - before >= 1:
            break
    assert engine.lease_counters()["answered"] - before >= 1
    for dims in (ONE, TWO):
        p, a, cap, occ, fs = setup(engine, dims, True, service=True)
        for name in fs:
            through_service(engine, a, cap, occ, name, fs[name], 5, SPLIT_HOST)
        # the same n_runs and J, another job sequence: a reversed class order per job
        q = dataclasses.replace(p, job_class=p.job_class[::-1].copy(), job_names=None)
        assert not np.array_equal(q.job_class, p.job_class)
        b = O.place_c(q)[0]
        assert not np.array_equal(a, b)
        ones_q = RF.forms(q.job_class, len(q.classes), 1)["ones"]
        assert ones_q[0].shape == fs["ones"][0].shape
        for name, form, want in (("ones", fs["ones"], a), ("gap", fs["gap"], a), ("ones", fs["ones"], a),
                                 ("ones permuted", ones_q, b), ("ones", fs["ones"], a)):
            through_service(engine, want, cap, occ, name, form, 5, SPLIT_HOST)


def case_device_set(engine):
    """Shape 6: three shards on one device, the walk in jspi_assign."""
    with Engine(devices=[0, 0, 0]) as multi:
        for dims in (ONE, TWO):
            p, a, cap, occ, fs = solved(dims)
            multi.load(p)
            for name, (rc, rl, _) in fs.items():
                got = multi.place_runs(rc, rl, want_tally=True)
                verify(got, a, cap, occ, rc.shape[0], True, f"device set {name}")
                assert got.fused == 6
                if name != "canonical":
                    SEEN.add((6, None))
            for rc, rl in (no_runs(), empties(p)):
                got = multi.place_runs(rc, rl, want_tally=True)
                verify(got, a[:0], cap, occ, rc.shape[0], True, "device set without jobs")
            bad_class_is_refused(multi, p, a)


def no_runs():
    return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)


def empties(p):
    rc, rl, _ = RF.forms(p.job_class[:0], len(p.classes), 3)["empties_only"]
    assert rc.shape[0] == 3 and not rl.any()
    return rc, rl


def case_no_jobs(engine):
    """J == 0 on every path above, as three empty runs and as no run at all:
    JSP_OK, placed == 0, jobs == 0; the device paths leave out[] at -7."""
    for dims, auto, service in ((ONE, False, False), (WIDE, False, False), (TWO, False, False), (ONE, True, False),
                                (TWO, True, False), (SOLO, True, False), (SOLO, True, True), (ONE, True, True)):
        p, a, cap, occ, _ = setup(engine, dims, auto, service=service)
        for rc, rl in (empties(p), no_runs()):
            for tally in (True, False):
                for _ in range(2):  # (with the service on: the launch path first, then the service)
                    got = engine.place_runs(rc, rl, want_tally=tally)
                    verify(got, a[:0], cap, occ, rc.shape[0], tally, f"{dims} J=0 n_runs={rc.shape[0]}")
            if not service:
                for how in ("place", "assign"):
                    device_call(engine, p, a[:0], cap, occ, "no jobs", (rc, rl, None), auto, how)
        # and the batch is placed as before
        host_call(engine, p, a, cap, occ, "canonical", solved(dims)[4]["canonical"], auto, True)


def bad_class_is_refused(engine, p, a):
    """An empty run with a class id >= C is JSP_EINVAL (check_runs); the next
    call answers correctly."""
    C = len(p.classes)
    rc, rl = RF.forms(p.job_class, C, 2)["canonical"][:2]
    bad_rc = np.concatenate([rc[:1], [C], rc[1:]]).astype(np.uint32)
    bad_rl = np.concatenate([rl[:1], [0], rl[1:]]).astype(np.uint32)
    with pytest.raises(JspError) as ei:
        engine.place_runs(bad_rc, bad_rl)
    assert ei.value.code == JSP_EINVAL and "run 1" in str(ei.value)
    got = engine.place_runs(rc, rl)
    np.testing.assert_array_equal(got.assign, a)


def case_bad_class(engine):
    for dims, auto, service in ((ONE, False, False), (TWO, True, False), (ONE, True, True)):
        p, a, _, _, _ = setup(engine, dims, auto, service=service)
        bad_class_is_refused(engine, p, a)


CASES = {f.__name__[5:]: f for f in (case_level_and_register, case_assign_lds, case_assign_levels, case_fused_tail,
                                     case_host_walk, case_compaction, case_services, case_device_set, case_no_jobs,
                                     case_bad_class)}


@pytest.mark.parametrize("name", list(CASES))
def test_forms(engine, monkeypatch, name):
    with guarded(engine, monkeypatch, name):
        CASES[name](engine)


# ------------------------------------------------------------------ the other entry points that take runs
def gang_cut(p, seed):
    """Gangs of 1-3 consecutive canonical runs, each with a span among the
    levels not finer than its classes', or ANY (gang_ref.sweep_case's rule)."""
    from jobset_amd.snapshot import job_runs
    rng = np.random.default_rng(seed)
    rc, rl = job_runs(p.job_class)
    gr, gj, gs = [], [], []
    r = 0
    while r < rc.shape[0]:
        n = min(int(rng.integers(1, 4)), rc.shape[0] - r)
        lv = min(p.classes[int(c)].level for c in rc[r:r + n])
        pick = int(rng.integers(0, lv + 2))
        gr.append(n)
        gj.append(int(rl[r:r + n].sum()))
        gs.append(ANY if pick == lv + 1 else pick)
        r += n
    if not gr:  # a batch without jobs: one gang without runs, which a form's empty runs join
        gr, gj, gs = [0], [0], [ANY]
    return np.array(gr, dtype=np.uint32), np.array(gj, dtype=np.int64), np.array(gs, dtype=np.int64)


def entry_problems():
    yield "config5", synth.config5()
    for seed in range(8):
        yield f"random{seed}", synth.random_problem(seed, max_nodes=3000, max_levels=3, max_leaves=150)


@functools.lru_cache(maxsize=None)
def entry_problem(name):
    return dict(entry_problems())[name]


ENTRY_NAMES = ["config5"] + [f"random{seed}" for seed in range(8)]


def same(first, other, what):
    """Outputs equal across forms."""
    for x, y in zip(first, other):
        if isinstance(x, np.ndarray):
            np.testing.assert_array_equal(x, y, err_msg=what)
        else:
            assert x == y, what


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_entry_points(engine, monkeypatch, name):
    """jsp_place_sticky, jsp_place_fit, jsp_place_gangs, jsp_bind_pods and
    jsp_assume + jsp_forget with every form: each equals its reference, all
    forms agree, and stats.runs is the non-empty count, as the header says."""
    p = entry_problem(name)
    J, C = p.n_jobs, len(p.classes)
    a0, cap, occ = O.place_c(p)
    tl = (cap, occ)
    fs = RF.forms(p.job_class, C, 11)
    rng = np.random.default_rng(17)
    # the previous placement with a third of it scrambled
    prev = a0.astype(np.int32).copy()
    for j in range(0, J, 3):
        prev[j] = int(rng.integers(-1, p.topology.n_domains[p.classes[int(p.job_class[j])].level]))
    want_sticky, kept = sticky_ref(p, prev, tl)
    want_fit = {policy: fit_ref(p, policy, tl) for policy in (TIGHTEST, ROOMIEST)}
    want_rows, want_off, want_bind = bind_ref(p, a0)
    owner = (0x40000000 + np.arange(J)).astype(np.int32)
    _, want_committed, want_assume = assume_ref(p, a0, owner)
    gr0, gj, gs = gang_cut(p, 23)
    want_gang, want_span = gang_ref(p, gj, gs, tl)
    with guarded(engine, monkeypatch, f"entry {name}"):
        engine.set_service(False)
        engine.load(p)
        first = {}
        for fname, (rc, rl, src) in fs.items():
            what = f"{name} {fname}"
            nonempty = int((rl > 0).sum())
            got, st = engine.place_sticky_runs(rc, rl, prev)
            np.testing.assert_array_equal(got, want_sticky, err_msg=what)
            assert (st.jobs, st.kept, st.placed, st.hinted) == (J, int(kept.sum()), int((want_sticky >= 0).sum()),
                                                                int((prev >= 0).sum())), what
            assert st.runs == nonempty, (what, st.runs, nonempty)
            out = [got, int(st.kept)]
            for policy in (TIGHTEST, ROOMIEST):
                got, st = engine.place_fit_runs(rc, rl, policy)
                want, want_st = want_fit[policy]
                np.testing.assert_array_equal(got, want, err_msg=what)
                assert fit_stats(st) == dict(want_st, runs=nonempty), what
                out += [got, int(st.slack)]
            gr = RF.regroup(gr0, src)
            got, span, st = engine.place_gangs_runs(rc, rl, gr, gs)
            np.testing.assert_array_equal(got, want_gang, err_msg=what)
            np.testing.assert_array_equal(span, want_span, err_msg=what)
            assert (st.jobs, st.placed, st.gangs, st.gangs_placed) == (J, int((want_gang >= 0).sum()), len(gs),
                                                                      int((want_span >= 0).sum())), what
            assert st.runs == nonempty, (what, st.runs, nonempty)
            out += [got, span]
            rows, off, st = engine.bind_pods_runs(rc, rl, a0)
            np.testing.assert_array_equal(rows, want_rows, err_msg=what)
            np.testing.assert_array_equal(off, want_off, err_msg=what)
            assert bind_stats(st) == want_bind, what
            out += [rows, off]
            committed, st = engine.assume_runs(rc, rl, a0, owner)
            np.testing.assert_array_equal(committed, want_committed, err_msg=what)
            assert assume_stats(st) == want_assume, what
            assert engine.forget(owner) == want_assume["rows_marked"], what
            out += [committed, int(st.committed), int(st.rows_marked)]
            same(first.setdefault("out", out), out, what)
        # the forgotten rows are free again: the plain placement as before
        np.testing.assert_array_equal(engine.place(p.job_class).assign, a0)


@pytest.mark.parametrize("seed", range(8))
def test_gangs_on_the_sweep_inputs(engine, monkeypatch, seed):
    """jsp_place_gangs on gang_ref.sweep_case's problems, gangs and spans
    (runs that never cross a gang boundary), every form, regrouped."""
    p, gj, gs = gang_sweep_case(seed)
    tl = O.place_c(p)[1:]
    want, want_span = gang_ref(p, gj, gs, tl)
    rc0, rl0, gr0 = gang_runs_of(p.job_class, gj)
    with guarded(engine, monkeypatch, f"gang sweep {seed}"):
        engine.load(p)
        for fname, (rc, rl, src) in RF.forms_of_runs(rc0, rl0, len(p.classes), seed).items():
            got, span, st = engine.place_gangs_runs(rc, rl, RF.regroup(gr0, src), gs)
            np.testing.assert_array_equal(got, want, err_msg=fname)
            np.testing.assert_array_equal(span, want_span, err_msg=fname)
            assert st.runs == int((rl > 0).sum()) and st.gangs_placed == int((want_span >= 0).sum()), fname


# ------------------------------------------------------------------ coverage
def test_every_path_saw_a_raw_list(engine, monkeypatch):
    """The (shape, walker) pairs seen with a non-canonical form cover every
    walker the forms can reach, so taking a case out cannot silently drop one.
    (Cases that a test selection left out run here first.)"""
    for name, fn in CASES.items():
        if name not in RAN:
            with guarded(engine, monkeypatch, name):
                fn(engine)
    need = {(0, LEVEL), (0, ASSIGN), (1, FUSED_TAIL), (2, COMPACT), (3, COMPACT), (5, SPLIT_HOST), (7, HOST),
            (8, SPLIT_HOST), (6, None)}
    assert SEEN >= need, need - SEEN
