"""Every kernel path that evaluates rows, against the row predicate as
include/jsplace.h states it (tests/contract_ref.py, which never folds req and
forbid into one compare): classes whose selector requires and forbids the same
bit, taint bits 16..31, excl_owner values other than -1 and small ids, class
words and requests past the snapshot's W and R, divisor 1 up to 2^32 - 1.
All values are integers and every comparison is exact. Each test asserts the
launch shape (stats.fused) it meant to reach."""
import numpy as np
import pytest

from jobset_amd import synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import job_runs

import contract_ref as CR
from bind_ref import bind_ref, stats_dict
from sticky_ref import sticky_ref

pytestmark = pytest.mark.gpu

PROBLEMS = CR.contract_problems()
IDS = [p.name for p in PROBLEMS]
MULTI = [p for p in PROBLEMS if len(p.classes) > 16]        # 22 classes, 300 jobs, both levels
SIXTEEN = [p for p in PROBLEMS if len(p.classes) <= 16]     # 16 classes, 100 jobs: one fused launch takes them
LEAF_NAMES = list(CR.contract_classes(1, 1))
CONTROLS = ("w0b0", "hi63", "0b11")

_refs = {}


def ref_of(p):
    """The reference of a fixed problem, computed once and left unchanged."""
    if p.name not in _refs:
        _refs[p.name] = CR.evaluate(p)
    return _refs[p.name]


def assert_equal(got, ref, tallies=True):
    if tallies:
        np.testing.assert_array_equal(got.occ, ref.occ)
        np.testing.assert_array_equal(got.cap, ref.cap)
    np.testing.assert_array_equal(got.assign, ref.assign)
    assert got.placed == int((ref.assign >= 0).sum())


def assert_overlaps_dead(p, got):
    """What the contract says in words: no overlap class has capacity anywhere
    and none of its jobs has a domain; its control has capacity."""
    for c in CR.overlap_ids(p):
        assert not got.cap[c].any(), p.meta["class_names"][c]
        assert got.cap[CR.control_of(p, c)].any()
        assert (got.assign[p.job_class == c] == -1).all(), p.meta["class_names"][c]


@pytest.fixture
def private_engine(monkeypatch):
    """An engine of the test's own, created under the given test hooks."""
    made = []

    def make(hooks):
        if hooks:
            monkeypatch.setenv("JSP_TEST_HOOKS", hooks)
        else:
            monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
        made.append(Engine(0))
        return made[-1]
    yield make
    for e in made:
        e.close()


@pytest.fixture
def launch_engine(engine):
    """The session engine on the launch path: no resident service."""
    engine.set_service(False)
    engine.set_fused(True)
    yield engine
    engine.set_fused(True)
    engine.set_service(True)
    engine.service_stop()


@pytest.fixture
def svc_engine(engine):
    """The session engine with the resident service parked: it does not idle
    out while the test computes a reference between two requests."""
    engine.set_service(True, parked=True)
    engine.set_fused(True)
    yield engine
    engine.service_stop()
    engine.set_service(True)


def warm(engine, job_class):
    """Place until a resident shape answers (the first call after an upload is
    answered on the launch path while the service comes up)."""
    for _ in range(4):
        got = engine.place(job_class)
        if got.fused in (3, 5):
            break
    return got


# ------------------------------------------------------------------ workgroup tally (tally_block)
@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_workgroup_tally_three_launch(private_engine, p):
    """tally -> feasibility -> assign with the workgroup tally forced; the
    22-class problems take two tally passes of 16 classes."""
    e = private_engine("tally_block=1")
    e.set_fused(False)
    e.load(p)
    got = e.place(p.job_class, want_tally=True)
    assert got.fused == 0
    assert_equal(got, ref_of(p))
    assert_overlaps_dead(p, got)


@pytest.mark.parametrize("p", SIXTEEN, ids=[p.name for p in SIXTEEN])
def test_fused_launch(launch_engine, p):
    launch_engine.load(p)
    for want_tally in (True, False):
        got = launch_engine.place(p.job_class, want_tally=want_tally)
        assert got.fused == 1
        assert_equal(got, ref_of(p), tallies=want_tally)
        if want_tally:
            assert_overlaps_dead(p, got)


# ------------------------------------------------------------------ wave tallies (wave_eval)
@pytest.mark.parametrize("group", range(len(CR.WAVE_GROUPS)))
@pytest.mark.parametrize("WR", [1, 4])
@pytest.mark.parametrize("hooks", ["", "tally_one=0"], ids=["one-tile", "double-buffered"])
def test_wave_tallies(private_engine, hooks, WR, group):
    """Up to 4 leaf-level classes on a snapshot whose leaves all fit a wave
    tile (<= 252 rows; one larger leaf sends every tally to the workgroup
    kernel): the three-launch shape's wave tally with the folded feasibility,
    and jsp_tally_device into a caller's buffer wider than the leaves."""
    import torch
    p = CR.contract_problem(WR, WR, names=CR.WAVE_GROUPS[group], levels=(1,), jobs=60, big=CR.WAVE_BIG)
    C, L = len(p.classes), p.topology.n_leaves
    sizes = np.diff(p.nodes.leaf_start.astype(np.int64))
    assert C <= 4 and sizes.max() <= 252 and sizes.sum() > 256 and all(c.level == 1 for c in p.classes)
    ref = ref_of(p)
    e = private_engine(hooks)
    e.set_fused(False)
    e.load(p)
    got = e.place(p.job_class, want_tally=True)
    assert got.fused == 0
    assert_equal(got, ref)
    for c, nm in enumerate(p.meta["class_names"]):
        if nm.split("@")[0].endswith("!"):
            assert not got.cap[c].any() and got.cap[CR.control_of(p, c)].any()
    ld = L + 5
    dcap = torch.full((C + 1, ld), 77, dtype=torch.int32, device="cuda")
    e.tally_device(dcap.data_ptr(), dcap[-1].data_ptr(), ld, 0)
    torch.cuda.synchronize()
    out = dcap.cpu().numpy().astype(np.uint32)
    np.testing.assert_array_equal(out[:C, :L], ref.cap)
    np.testing.assert_array_equal(out[C, :L], ref.occ)
    assert (out[:, L:] == 77).all()  # only the leaves' columns are written


# ------------------------------------------------------------------ one-class compaction (and resident_eval)
@pytest.mark.parametrize("name", LEAF_NAMES)
@pytest.mark.parametrize("WR", [1, 4])
def test_one_class_compaction(engine, WR, name):
    """Each contract class alone at the leaf level: the compaction launch
    (fused 2) and the resident compaction service (fused 3)."""
    p = CR.contract_problem(WR, WR, names=(name,), levels=(1,), jobs=20)
    ref = ref_of(p)
    if name.endswith("!"):
        assert (ref.assign == -1).all()
    else:
        assert (ref.assign >= 0).any()
    engine.set_fused(True)
    engine.set_service(False)
    try:
        engine.load(p)
        got = engine.place(p.job_class, want_tally=True)
        assert got.fused == 2
        assert_equal(got, ref)
        got = engine.place(p.job_class)
        assert got.fused == 2
        assert_equal(got, ref, tallies=False)
    finally:
        engine.set_service(True)
    try:
        engine.load(p)
        got = warm(engine, p.job_class)
        assert got.fused == 3
        assert_equal(got, ref, tallies=False)
        got = engine.place(p.job_class)
        assert got.fused == 3
        assert_equal(got, ref, tallies=False)
    finally:
        engine.service_stop()


# ------------------------------------------------------------------ split service and the host walk
@pytest.mark.parametrize("p", MULTI, ids=[p.name for p in MULTI])
def test_split_service_and_host_walk(engine, p):
    """22 classes at both levels, 300 jobs: the resident split tiles (fused 5),
    the same tiles launched once (8), and the tally + feasibility launches
    walked on the host (7); the device path of the same shape."""
    import torch
    ref = ref_of(p)
    engine.set_fused(True)
    engine.set_service(True)
    try:
        engine.load(p)
        got = warm(engine, p.job_class)
        assert got.fused == 5
        assert_equal(got, ref, tallies=False)
        got = engine.place(p.job_class, want_tally=True)
        assert got.fused == 7
        assert_equal(got, ref)
        assert_overlaps_dead(p, got)
        engine.set_service(False)
        got = engine.place(p.job_class)
        assert got.fused == 8
        assert_equal(got, ref, tallies=False)
        rc, rl = job_runs(p.job_class)
        rct, rlt = torch.from_numpy(rc.astype(np.int32)).cuda(), torch.from_numpy(rl.astype(np.int32)).cuda()
        out = torch.full((p.n_jobs,), -7, dtype=torch.int32, device="cuda")
        engine.place_device(rct.data_ptr(), rlt.data_ptr(), rc.shape[0], p.n_jobs, out.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
        engine.check()
        np.testing.assert_array_equal(out.cpu().numpy(), ref.assign)
    finally:
        engine.set_service(True)
        engine.service_stop()


# ------------------------------------------------------------------ resident rows after a patch
def _flip_bit0(p, rows):
    lab = p.nodes.labels[:, rows].copy()
    lab[0] ^= np.uint64(1)
    return lab


@pytest.mark.parametrize("shape", ["overlap-alone", "control-alone", "all-classes"])
def test_resident_rows_after_patch(svc_engine, shape):
    """With the service up, one row patched (it rides in the next request) and
    then every row (the staged delta): rows gain and lose the bit an overlap
    class requires and forbids. The resident tiles answer from the patched
    rows; the launch path's tallies agree."""
    if shape == "all-classes":
        p, fused = CR.contract_problem(4, 4), 5
    else:
        p, fused = CR.contract_problem(1, 1, names=("w0b0!" if shape == "overlap-alone" else "w0b0",),
                                       levels=(1,), jobs=20), 3
    N = p.nodes.n_nodes   # (p is built afresh: the patches below edit its rows in place)
    svc_engine.load(p)
    got = warm(svc_engine, p.job_class)
    assert got.fused == fused
    before = CR.evaluate(p)
    assert_equal(got, before, tallies=False)
    # one row of the 4-row leaf that carries bit 0 loses it; then every row flips
    # it: the rows that had it lose it, the others gain it
    one = next(int(r) for r in range(int(p.nodes.leaf_start[3]), int(p.nodes.leaf_start[4]))
               if int(p.nodes.labels[0, r]) & 1)
    steps = [np.array([one], dtype=np.uint32), np.arange(N, dtype=np.uint32)]
    changed = False
    for rows in steps:
        lab = _flip_bit0(p, rows)
        svc_engine.patch_rows(rows, labels=lab)
        p.nodes.labels[:, rows] = lab
        ref = CR.evaluate(p)
        got = svc_engine.place(p.job_class)
        assert got.fused == fused
        assert_equal(got, ref, tallies=False)
        changed |= not np.array_equal(ref.cap, before.cap)
    assert changed == (shape != "overlap-alone")  # an overlap class has no capacity whatever the rows hold
    got = svc_engine.place(p.job_class, want_tally=True)
    assert got.fused == (7 if fused == 5 else 2)
    assert_equal(got, ref)


# ------------------------------------------------------------------ jsp_explain
def explain_dict(x):
    d = {f: int(getattr(x, f)) for f in ("rows", "rows_selector", "rows_taint", "rows_no_capacity", "rows_fit",
                                         "rows_occupied", "domains", "dom_occupied", "dom_short", "dom_feasible",
                                         "best_short_cap", "best_short_domain")}
    d["rows_insufficient"] = [int(v) for v in x.rows_insufficient]
    return d


def assert_explain(e, p):
    ref = ref_of(p)
    got = [explain_dict(x) for x in e.explain()]
    assert len(got) == len(ref.explain)
    for c, (g, w) in enumerate(zip(got, ref.explain)):
        assert g == w, (p.meta["class_names"][c], g, w)
    for c in CR.overlap_ids(p):
        assert got[c]["rows_selector"] == p.nodes.n_nodes and got[c]["dom_feasible"] == 0
        assert got[CR.control_of(p, c)]["dom_feasible"] > 0


@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_explain(launch_engine, p):
    launch_engine.load(p)
    assert_explain(launch_engine, p)


# ------------------------------------------------------------------ jsp_bind_pods, jsp_place_sticky
def control_and_overlap(WR, jobs=40):
    """The same jobs under the control classes and under their overlap twins
    (class ids correspond)."""
    ctl = CR.contract_problem(WR, WR, names=CONTROLS, jobs=jobs)
    ovl = CR.contract_problem(WR, WR, names=[n + "!" for n in CONTROLS], jobs=jobs)
    np.testing.assert_array_equal(ctl.job_class, ovl.job_class)
    return ctl, ovl


@pytest.mark.parametrize("WR", [1, 4])
@pytest.mark.parametrize("form", ["auto", "wg"])
def test_bind_pods(launch_engine, monkeypatch, form, WR):
    """Assignments taken under the control classes bind under them; under the
    overlap classes every job is stale and every pod is -1."""
    if form == "wg":
        monkeypatch.setenv("JSP_TEST_HOOKS", "bind_wg=1")   # read at every snapshot upload
    else:
        monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    ctl, ovl = control_and_overlap(WR)
    assign = ref_of(ctl).assign
    n_placed = int((assign >= 0).sum())
    assert n_placed >= 3
    for p in (ctl, ovl):
        want_rows, want_off, want = bind_ref(p, assign)
        launch_engine.load(p)
        rows, off, st = launch_engine.bind_pods(p.job_class, assign)
        np.testing.assert_array_equal(off, want_off)
        np.testing.assert_array_equal(rows, want_rows)
        assert stats_dict(st) == want
        if p is ctl:
            assert st.bound == n_placed and st.stale == 0 and (rows >= 0).any()
        else:
            assert st.bound == 0 and st.stale == n_placed and st.pods_bound == 0 and (rows == -1).all()


@pytest.mark.parametrize("WR", [1, 4])
@pytest.mark.parametrize("form", ["one", "grid"])
def test_place_sticky(launch_engine, monkeypatch, form, WR):
    """Previous domains taken under the control classes are all kept under
    them; under the overlap classes none is kept and the fill places nothing."""
    if form == "grid":
        monkeypatch.setenv("JSP_TEST_HOOKS", "sticky_grid=1")  # read at every snapshot upload
    else:
        monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    ctl, ovl = control_and_overlap(WR)
    prev = ref_of(ctl).assign
    n_hint = int((prev >= 0).sum())
    assert n_hint >= 3
    for p in (ctl, ovl):
        ref = ref_of(p)
        want, kept = sticky_ref(p, prev, (ref.cap, ref.occ))
        launch_engine.load(p)
        got, st = launch_engine.place_sticky(p.job_class, prev)
        np.testing.assert_array_equal(got, want)
        assert (st.jobs, st.hinted, st.kept, st.placed) == (p.n_jobs, n_hint, int(kept.sum()), int((want >= 0).sum()))
        assert st.fused == 0   # 40 jobs: the fill walks on the GPU
        if p is ctl:
            assert st.kept == n_hint and np.array_equal(got, prev)
        else:
            assert st.kept == 0 and st.placed == 0 and (got == -1).all()


# ------------------------------------------------------------------ device set
@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_device_set(p):
    """Two shards on one GPU get the same class encoding: the combined
    tallies, the assignment and jsp_explain equal the reference."""
    with Engine(devices=[0, 0]) as e:
        assert e.shards() == (2, 1)
        e.load(p)
        got = e.place(p.job_class, want_tally=True)
        assert got.fused == 6
        assert_equal(got, ref_of(p))
        assert_overlaps_dead(p, got)
        got = e.place(p.job_class)
        assert got.fused == 6
        assert_equal(got, ref_of(p), tallies=False)
        assert_explain(e, p)


# ------------------------------------------------------------------ random problems with overlaps
@pytest.mark.parametrize("seed", CR.SWEEP_SEEDS[:24])
@pytest.mark.parametrize("shape", ["fused", "three-launch"])
def test_overlap_sweep(launch_engine, shape, seed):
    p = CR.with_overlaps(synth.random_problem(seed), seed)
    ref = CR.evaluate(p)
    launch_engine.set_fused(shape == "fused")
    launch_engine.load(p)
    got = launch_engine.place(p.job_class, want_tally=True)
    if shape == "three-launch":
        assert got.fused == 0
    else:  # one class at the leaf level: 2; from 256 jobs on, where the GPU level walker does not apply: 7; else 1
        assert got.fused in (1, 2, 7)
        if len(p.classes) == 1 and p.classes[0].level == p.topology.n_levels - 1:
            assert got.fused == 2
        elif p.n_jobs < 256:
            assert got.fused == 1
    assert_equal(got, ref)
    for c in p.meta["overlapped"]:
        assert not got.cap[c].any() and (got.assign[p.job_class == c] == -1).all()
