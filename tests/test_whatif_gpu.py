"""jsp_place_whatif on the GPU against the rule taken literally over the CPU
oracle (tests/whatif_ref.py; it never calls the engine). Every comparison is
exact: assign[S][J] bit for bit, placed[S] and the flip count (tests/
test_whatif.py asserts the sweep's coverage floors on the yardstick's own
output). Shapes are small: at most a few thousand rows, 8 classes, 300 jobs."""
import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import JobClass, Nodes, Problem, Topology, job_runs
from oracle import oracle as O
from bind_ref import cls, flat, nested
from test_service_standing_gpu import snapshot, warm
from whatif_ref import EMPTY, SWEEP_SEEDS, concat, edit, hand_cases, only, patched, sweep, whatif_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["service", "launch"])
def mode(request, engine):
    """The resident service on (AUTO) or off: the call itself never uses it."""
    engine.set_service(request.param == "service")
    engine.set_fused(True)
    yield request.param
    engine.set_service(True)
    engine.service_stop()


@pytest.fixture
def svc_engine(engine):
    engine.set_service(True)
    engine.set_fused(True)
    yield engine
    engine.set_timing(False)
    engine.service_stop()


def run(engine, p, scenarios, load=True, what=""):
    """Load p, ask the scenarios, compare everything with the yardstick."""
    if load:
        engine.load(p)
    want, want_placed, want_flips, _, _ = whatif_ref(p, scenarios)
    got, placed, st = engine.place_whatif(p.job_class, scenarios)
    assert got.shape == want.shape
    for s in range(len(scenarios)):
        np.testing.assert_array_equal(got[s], want[s], err_msg=f"{what or p.name} scenario {s}")
    np.testing.assert_array_equal(placed, want_placed)
    rc, _ = job_runs(p.job_class)
    assert (st.jobs, st.scenarios, st.rows, st.runs, st.fused) == \
        (p.n_jobs, len(scenarios), sum(len(sc["rows"]) for sc in scenarios), len(rc), 7)
    assert st.flips == want_flips, (what or p.name, st.flips, want_flips)
    return got, st


def owner(p, row, who=77):
    return only(edit(p, [row], excl_owner=[who]), "excl_owner")


# ------------------------------------------------------------------ 1. the baseline
def test_baseline_empty_scenario_is_jsp_place(engine, mode):
    p, scenarios = sweep(2)
    engine.load(p)
    plain = engine.place(p.job_class).assign.copy()
    got, _ = run(engine, p, [scenarios[0], EMPTY, scenarios[5]], load=False)
    np.testing.assert_array_equal(got[1], plain)
    np.testing.assert_array_equal(plain, O.place_c(p)[0])


# ------------------------------------------------------------------ 2./3. one row in both directions; sums in a domain
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(engine, mode, name):
    p, scenarios, want, flips = hand_cases()[name]
    got, st = run(engine, p, scenarios, what=name)
    np.testing.assert_array_equal(got, want)
    assert st.flips == flips


def test_sums_within_a_domain(engine, mode):
    """Two zones of two racks of three rows. A zone job wants 9 pods (a zone
    holds 6), a rack job 6 (a rack holds 3): no single edit opens a domain,
    the sum of two rows in two leaves of a zone, and of three rows in one
    leaf, does; and one edit that closes what another opened."""
    p = nested([[0, 2, 4], np.arange(5)], [3, 3, 3, 3], [cls(0, 9), cls(1, 6)], [0, 1, 0, 1])
    free = lambda rows, vals: only(edit(p, rows, free_res=[vals]), "free_res")  # noqa: E731
    scenarios = [free([0], [3]), free([3], [2]), free([0, 3], [3, 2]),            # two leaves of zone 0: 8, 7, 9
                 free([6, 7], [2, 2]), free([6, 7, 8], [2, 2, 2]),                 # one leaf: two rows (5), three (6)
                 free([0, 3, 5], [3, 2, 0]),                                       # opened by two, closed by the third
                 free([0, 1, 2, 3], [3, 3, 2, 0])]                                 # rack 0 opens (8), zone 0 too (10)
    got, st = run(engine, p, scenarios)
    want = whatif_ref(p, scenarios)
    assert list(want[3]) == [0, 0, 1, 0, 2, 0, 2] and list(want[4]) == [0] * 7
    assert (got[0] == -1).all() and got[2][0] == 0 and got[4][0] == 1


# ------------------------------------------------------------------ 4. edges
def ident(n):
    return np.arange(n + 1)


def edges(n):
    """level-0 boundaries at and one off the 64-bit word boundaries below n"""
    return np.array(sorted({0, n} | {b for b in (1, 63, 64, 65, 127, 128, 129) if b < n}))


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_word_boundaries(engine, mode, n):
    """n racks (the class level's domain count) of 1-4 rows, a zone level on
    top with boundaries at the word boundaries; an owner on a row of the
    racks around every word boundary, on row 0 and on row N - 1, one scenario
    each, and n jobs, so that every bit shows in the answer."""
    sizes = synth.uniform_int(n, 5, n, 1, 4)
    p = nested([edges(n), ident(n)], sizes, [cls(1, 1), cls(0, 2)], [0] * n + [1] * 3)
    N = p.nodes.n_nodes
    ls = p.nodes.leaf_start
    scenarios = [owner(p, 0), owner(p, N - 1)]
    for d in (62, 63, 64, 65, 127, 128):
        if d < n:
            scenarios.append(owner(p, int(ls[d])))              # the first row of the leaf
            scenarios.append(owner(p, int(ls[d + 1]) - 1))      # the last
    got, st = run(engine, p, scenarios)
    assert st.flips >= len(scenarios)


def test_single_row_leaves_and_three_levels(engine, mode):
    """K = 3 with classes on all three levels (a take marks across the
    levels), leaves of one row among them, rowless leaves too."""
    sizes = [1, 2, 1, 0, 3, 1, 1, 2, 0, 1, 4, 1]
    p = nested([[0, 6, 12], [0, 2, 4, 6, 8, 10, 12], ident(12)], sizes,
               [cls(2, 1), cls(1, 2), cls(0, 5)], [2, 1, 0, 0, 1, 0, 2, 0, 1])
    N = p.nodes.n_nodes
    both = lambda rows, **kw: only(edit(p, rows, **kw), "free_res", "excl_owner")  # noqa: E731
    scenarios = [both([0], excl_owner=[77]), both([3], excl_owner=[77]), both([N - 1], excl_owner=[77]), EMPTY,
                 both([0, 3, 9], free_res=[[0, 0, 0]]),
                 both([2, 8, 16], free_res=[[5, 5, 5]], excl_owner=[-1, 3, -1])]
    got, st = run(engine, p, scenarios)
    assert st.flips > 0 and len({tuple(a) for a in got}) > 2


# ------------------------------------------------------------------ 5./6. class forms and delta forms
def forms_problem():
    """300 rows in 30 racks of 10 in 5 zones, W = 4 label words, R = 4
    resources; classes: a selector in word 3 with requests of 1 and 2 (the
    reciprocal path); four requests >= 2; more pods than rows; a contradictory
    selector; a class that requests nothing; forbidden labels."""
    s, N, L = 4242, 300, 30
    topo = Topology(level_keys=["example.com/zone", "example.com/rack"], n_domains=[5, L],
                    first_leaf=[np.arange(0, L + 1, 6, dtype=np.uint32), np.arange(L + 1, dtype=np.uint32)])
    labels = np.stack([synth.draws(s, 10 + w, N) | synth.draws(s, 14 + w, N) for w in range(4)])
    free = np.stack([synth.uniform_int(s, 20 + r, N, 0, 20) for r in range(4)]).astype(np.uint32)
    taints = np.where(synth.bernoulli(s, 30, N, 0.2), 2, 0).astype(np.uint32)
    excl = np.full(N, -1, dtype=np.int32)
    excl[70:80] = 9
    nodes = Nodes(leaf_start=np.arange(0, N + 1, 10, dtype=np.uint32), labels=labels, taints=taints, free=free, excl=excl)
    classes = [JobClass(req_labels=(0, 0, 0, 5), tolerated_taints=2, level=1, pods=12, req_res=(1, 0, 2, 0)),
               JobClass(tolerated_taints=0, level=0, pods=40, req_res=(3, 5, 7, 2)),
               JobClass(tolerated_taints=2, level=0, pods=400, req_res=(0, 1, 0, 0)),
               JobClass(req_labels=(8,), forbid_labels=(8,), tolerated_taints=0xFFFF, level=1, pods=1, req_res=(0,)),
               JobClass(tolerated_taints=0xFFFF, level=1, pods=5, req_res=(0, 0, 0, 0)),
               JobClass(forbid_labels=(0, 3), tolerated_taints=2, level=1, pods=3, req_res=(0, 0, 0, 4))]
    jc = np.array([0, 0, 1, 2, 3, 4, 4, 5, 0, 1, 5, 4, 2, 0, 0, 5, 5, 4], dtype=np.uint32)
    return Problem(topology=topo, nodes=nodes, classes=classes, job_class=jc, name="forms")


def forms_scenarios(p):
    N = p.nodes.n_nodes
    s = 777
    out = []
    for i in range(4):
        k = 20 + 10 * i
        rows = np.sort(synth.permutation(s + i, 1, N)[:k])
        lab = np.stack([synth.draws(s + i, 10 + w, k) & synth.draws(s + i, 14 + w, k) for w in range(4)])
        fr = np.stack([synth.uniform_int(s + i, 20 + r, k, 0, 40) for r in range(4)])
        tn = np.where(synth.bernoulli(s + i, 30, k, 0.5), synth.uniform_int(s + i, 31, k, 0, 7), 0)
        ex = np.where(synth.bernoulli(s + i, 32, k, 0.1), 700, -1)
        out.append(edit(p, rows, labels=lab, taints=tn, free_res=fr, excl_owner=ex))
    rows = np.arange(70, 80)                              # the held rack given back, full
    out.append(edit(p, rows, excl_owner=np.full(10, -1), free_res=np.full((4, 10), 40), taints=np.zeros(10),
                    labels=np.tile(np.array([[0], [0], [0], [5]], dtype=np.uint64), (1, 10))))
    return out


def test_class_forms_all_columns(engine, mode):
    p = forms_problem()
    got, st = run(engine, p, forms_scenarios(p))
    assert st.flips > 0 and (got[:, 4] == -1).all()      # the contradictory selector never places


@pytest.mark.parametrize("column", ["labels", "taints", "free_res", "excl_owner"])
def test_each_column_alone(engine, mode, column):
    """The other three columns NULL: they keep the resident values."""
    p = forms_problem()
    scenarios = [only(sc, column) for sc in forms_scenarios(p)]
    so, rows, lab, tn, fr, ex = concat(scenarios)
    assert sum(a is not None for a in (lab, tn, fr, ex)) == 1
    got, st = run(engine, p, scenarios, what=column)
    assert st.flips > 0


# ------------------------------------------------------------------ 7. scenario forms
def test_same_row_edited_differently(engine, mode):
    p = forms_problem()
    base = edit(p, [5, 75, 299])
    a = dict(base, excl_owner=np.array([4, 9, -1], dtype=np.int32))
    b = dict(base, excl_owner=np.array([-1, -1, 4], dtype=np.int32), free_res=np.full((4, 3), 40, dtype=np.uint32))
    c = dict(base, taints=np.array([1, 1, 1], dtype=np.uint32))
    got, st = run(engine, p, [a, b, c, a])
    np.testing.assert_array_equal(got[0], got[3])
    assert not np.array_equal(got[0], got[1])


def test_64_scenarios(engine, mode):
    n = 70
    p = flat(synth.uniform_int(64, 5, n, 1, 3), [cls(0, 1)], [0] * n)
    ls = p.nodes.leaf_start
    scenarios = [owner(p, int(ls[d])) if d % 9 else EMPTY for d in range(64)]
    got, st = run(engine, p, scenarios)
    assert st.scenarios == 64 and st.flips == sum(1 for d in range(64) if d % 9)


def test_65536_rows(engine, mode):
    """n_total = JSP_WHATIF_MAX_ROWS: 16 scenarios of 4096 rows on 8192 rows
    (2048 racks of 4 in 32 zones); every slice of a scenario's rows is taken."""
    L, N = 2048, 8192
    p = nested([np.arange(0, L + 1, 64), ident(L)], [4] * L, [cls(1, 3), cls(0, 200)], [1, 0] * 40 + [0] * 100,
               free=synth.uniform_int(9, 1, N, 0, 1))
    scenarios = []
    for s in range(16):
        rows = np.sort(synth.permutation(100 + s, 1, N)[:4096])
        scenarios.append(only(edit(p, rows, free_res=[synth.uniform_int(100 + s, 2, 4096, 0, 2)],
                                   excl_owner=np.where(synth.bernoulli(100 + s, 3, 4096, 0.002), 5, -1)),
                              "free_res", "excl_owner"))
    got, st = run(engine, p, scenarios)
    assert st.rows == native.JSP_WHATIF_MAX_ROWS and st.flips > 1000


# ------------------------------------------------------------------ 8. the seeded sweep
@pytest.mark.parametrize("seed", list(SWEEP_SEEDS))
def test_sweep(engine, mode, seed):
    p, scenarios = sweep(seed)
    run(engine, p, scenarios)
    # the same jobs as runs, the scenarios as raw buffers
    rc, rl = job_runs(p.job_class)
    got, placed, st = engine.place_whatif_runs(rc, rl, *concat(scenarios))
    np.testing.assert_array_equal(got, whatif_ref(p, scenarios)[0])


# ------------------------------------------------------------------ 9. nothing moved
def test_nothing_moved_behind_the_service(svc_engine, monkeypatch):
    """Tallies, the service's starts and fallbacks, jsp_explain and the metrics
    are the same before and after a what-if call, and a leased placement after
    it is still answered from the lease."""
    engine = svc_engine
    monkeypatch.setenv("JSP_TEST_HOOKS", "")
    p = snapshot(120)
    engine.load(p)
    warm(engine, p)
    want = O.place_c(p)[0]
    scenarios = [owner(p, int(15 * want[0])), EMPTY, owner(p, int(15 * want[3]) + 14)]
    ref = whatif_ref(p, scenarios)
    before = engine.place(p.job_class, want_tally=True)
    b_assign, b_cap, b_occ = before.assign.copy(), before.cap.copy(), before.occ.copy()
    ex0 = [bytes(x) for x in engine.explain()]
    warm(engine, p)
    engine.timing(reset=True)
    m0 = engine.metrics()
    engine.place_whatif(p.job_class, scenarios)          # (the call's buffers exist from here on)
    # the lease: a crossing, a placement answered on the host, the what-if call, another one answered on the host
    assert engine.place(p.job_class[:0]).fused == 3
    lc0 = engine.lease_counters()
    np.testing.assert_array_equal(engine.place(p.job_class).assign, want)
    lc1 = engine.lease_counters()
    got, placed, st = engine.place_whatif(p.job_class, scenarios)
    after = engine.place(p.job_class)
    lc2 = engine.lease_counters()
    assert lc1["answered"] == lc0["answered"] + 1, (lc0, lc1)
    assert lc2["answered"] == lc1["answered"] + 1 and lc2["dropped"] == lc1["dropped"], (lc1, lc2)
    assert after.fused == 3
    np.testing.assert_array_equal(after.assign, want)
    np.testing.assert_array_equal(got, ref[0])
    assert st.flips == ref[2] == 2
    t = engine.timing(reset=True)
    assert t.svc_starts == 0 and t.svc_fallbacks == 0
    m1 = engine.metrics()
    assert m1.place_us.count == m0.place_us.count + 3    # the three jsp_place calls: the what-if call is not counted
    assert m1.placed == m0.placed + 2 * int((want >= 0).sum())
    again = engine.place(p.job_class, want_tally=True)
    np.testing.assert_array_equal(again.assign, b_assign)
    np.testing.assert_array_equal(again.cap, b_cap)
    np.testing.assert_array_equal(again.occ, b_occ)
    assert [bytes(x) for x in engine.explain()] == ex0


# ------------------------------------------------------------------ 10. ordering behind a patch
def test_a_patch_is_seen_at_once(engine, mode):
    p = snapshot(120)
    engine.load(p)
    if mode == "service":
        warm(engine, p)
    want0 = O.place_c(p)[0]
    row = int(15 * want0[2]) + 3
    engine.patch_rows(np.array([row], dtype=np.uint32), taints=np.array([1 << 31], dtype=np.uint32))
    p.nodes.taints[row] = 1 << 31
    scenarios = [EMPTY, only(edit(p, [int(15 * want0[0])], excl_owner=[77]), "taints", "excl_owner"),
                 only(edit(p, [row], taints=[0]), "taints", "excl_owner")]   # the patch undone, hypothetically
    got, st = run(engine, p, scenarios, load=False)
    np.testing.assert_array_equal(got[2], want0)
    assert not np.array_equal(got[0], want0)
    np.testing.assert_array_equal(engine.place(p.job_class).assign, got[0])


# ------------------------------------------------------------------ 11. refusals, each followed by a correct call
def refused(engine, code, word, *args, **kw):
    with pytest.raises(native.JspError) as ei:
        engine.place_whatif_runs(*args, **kw)
    assert ei.value.code == code, str(ei.value)
    assert word in str(ei.value), str(ei.value)


def test_refusals_leave_the_engine_usable(engine, mode):
    p, scenarios, want, _ = hand_cases()["close"]
    engine.load(p)
    rc, rl = job_runs(p.job_class)
    so, rows, lab, tn, fr, ex = concat(scenarios)
    lib = native.lib()
    out = np.zeros(2 * p.n_jobs, dtype=np.int32)
    N = p.nodes.n_nodes

    def ok():
        got, _, _ = engine.place_whatif_runs(rc, rl, so, rows, excl_owner=ex)
        np.testing.assert_array_equal(got, want)

    def raw(rc_=rc, rl_=rl, so_=so, S=len(scenarios), rows_=rows, ex_=ex, out_=out, flags=0):
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return lib.jsp_place_whatif(engine._h, ptr(rc_), ptr(rl_), len(rl), ptr(so_), S, ptr(rows_), None, None, None,
                                    ptr(ex_), flags, ptr(out_), None, None)

    ok()
    for kw, word in ((dict(rc_=None), "run buffers are NULL"), (dict(out_=None), "assign_out is NULL"),
                     (dict(so_=None), "scen_off is NULL"), (dict(rows_=None), "rows is NULL"),
                     (dict(ex_=None), "all four delta columns are NULL"), (dict(flags=2), "flags 2")):
        assert raw(**kw) == native.JSP_EINVAL, kw
        assert word.encode() in lib.jsp_last_error(), (kw, lib.jsp_last_error())
        ok()
    refused(engine, native.JSP_EINVAL, "run 1", [0, 2], [1, 1], so, rows, excl_owner=ex)         # no such class
    ok()
    refused(engine, native.JSP_EINVAL, "scen_off[0] is 1", rc, rl, [1, 1, 1], rows, excl_owner=ex)
    ok()
    refused(engine, native.JSP_EINVAL, "scenario 1: scen_off decreases", rc, rl, [0, 1, 0], rows, excl_owner=ex)
    ok()
    refused(engine, native.JSP_EINVAL, f"scenario 1: position 1: row {N}", rc, rl, [0, 1, 3], [0, 0, N],
            excl_owner=[1, 1, 1])
    ok()
    refused(engine, native.JSP_EINVAL, "scenario 1: position 2: row 2 after row 2 is not strictly ascending", rc, rl,
            [0, 2, 5], [0, 1, 1, 2, 2], excl_owner=[1] * 5)
    ok()
    refused(engine, native.JSP_EINVAL, "scenario 0: position 1: row 0 after row 1", rc, rl, [0, 2], [1, 0],
            excl_owner=[1, 1])
    ok()
    refused(engine, native.JSP_ERANGE, "limit of 65536", [0], [native.JSP_WHATIF_MAX_JOBS + 1], so, rows, excl_owner=ex)
    ok()
    refused(engine, native.JSP_ERANGE, "65 scenarios exceed the limit of 64", rc, rl, np.zeros(66), [], excl_owner=None)
    ok()
    big = native.JSP_WHATIF_MAX_ROWS + 1
    refused(engine, native.JSP_ERANGE, "65537 rows in the scenarios exceed the limit of 65536", rc, rl, [0, big],
            np.zeros(big), excl_owner=np.zeros(big))
    ok()
    # n_scen == 0 and J == 0: JSP_OK, nothing written
    got, placed, st = engine.place_whatif_runs(rc, rl, [0], [])
    assert got.shape == (0, p.n_jobs) and (st.scenarios, st.jobs, st.flips, st.fused) == (0, p.n_jobs, 0, 7)
    got, placed, st = engine.place_whatif_runs([], [], so, rows, excl_owner=ex)
    assert got.shape == (2, 0) and (st.scenarios, st.jobs, st.rows) == (2, 0, 1)
    out[:] = -7
    assert raw(S=0) == native.JSP_OK and (out == -7).all()
    ok()


def test_device_set_sharded_and_unloaded_engines_are_estate():
    from jobset_amd.snapshot import shard_problem
    p = synth.config5()
    rc, rl = job_runs(p.job_class)
    args = (rc, rl, [0, 1], [0])
    with Engine(devices=[0, 0]) as multi:
        multi.load(p)
        refused(multi, native.JSP_ESTATE, "device-set", *args, excl_owner=[3])
    with Engine(0) as e:
        e.upload_topology(p.topology)
        e.upload_snapshot(shard_problem(p, 0, 2))
        e.upload_classes(p.classes)
        refused(e, native.JSP_ESTATE, "sharded", *args, excl_owner=[3])
    with Engine(0) as e:
        refused(e, native.JSP_ESTATE, "no topology", *args, excl_owner=[3])
        e.upload_topology(p.topology)
        refused(e, native.JSP_ESTATE, "no snapshot", *args, excl_owner=[3])
        e.upload_snapshot(p.nodes)
        refused(e, native.JSP_ESTATE, "no job classes", *args, excl_owner=[3])
        e.upload_classes(p.classes)
        got, placed, st = e.place_whatif_runs(*args, excl_owner=[3])
        np.testing.assert_array_equal(got, whatif_ref(p, [owner(p, 0, 3)])[0])


# ------------------------------------------------------------------ 12. the old way gives the same answer
def test_patch_place_patch_back_agrees(engine, mode):
    p = forms_problem()
    engine.load(p)
    scenarios = forms_scenarios(p)
    got, _, _ = engine.place_whatif(p.job_class, scenarios)
    n = p.nodes
    for s, sc in enumerate(scenarios):
        rows = sc["rows"]
        engine.patch_rows(rows, labels=sc["labels"], taints=sc["taints"], free=sc["free_res"], excl=sc["excl_owner"])
        old = engine.place(p.job_class).assign.copy()
        engine.patch_rows(rows, labels=n.labels[:, rows], taints=n.taints[rows], free=n.free[:, rows], excl=n.excl[rows])
        np.testing.assert_array_equal(old, got[s], err_msg=f"scenario {s}")
        np.testing.assert_array_equal(old, O.place_c(patched(p, sc))[0])
    np.testing.assert_array_equal(engine.place(p.job_class).assign, O.place_c(p)[0])


def test_timed_loop(engine, mode):
    p, scenarios = sweep(5)
    engine.load(p)
    rc, rl = job_runs(p.job_class)
    total, med, p99 = engine.place_whatif_loop(rc, rl, *concat(scenarios), iters=10)
    assert 0 < med <= p99 and total > 0
