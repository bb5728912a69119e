"""jsp_bind_pods_even on the GPU against the rule in int64 numpy (tests/bind_even_ref.py), exactly: pod_row,
pod_off, level, every stats field. The rule's properties are asserted on the output without the reference too."""
import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import job_runs, shard_problem
from oracle import oracle as O
from bind_ref import cls, domain_rows, flat, row_caps
from bind_even_ref import bind_even_ref, even_stats_dict, even_takes

pytestmark = pytest.mark.gpu
LEAD = 3  # rows of another leaf in front: every domain starts off a 4-row boundary
# the wave form's first and last size, the first workgroup size, one chunk exactly, two chunks (twice), three
SIZES = [5, 256 - LEAD, 257 - LEAD, 1024 - LEAD, 1025 - LEAD, 1025, 2051]
FORMS = [(n, "") for n in SIZES] + [(n, "bind_wg=1") for n in SIZES[:2]]


def checked(engine, p, assign):
    """Every output against the yardstick, then the properties; (rows, jsp_bind_pods' rows)."""
    assign = np.asarray(assign, dtype=np.int32)
    want_rows, want_off, want_level, want = bind_even_ref(p, assign)
    rows, off, level, st = engine.bind_pods_even(p.job_class, assign)
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(level, want_level)
    np.testing.assert_array_equal(rows, want_rows)
    assert even_stats_dict(st) == want and st.reserved == 0
    first = engine.bind_pods(p.job_class, assign)[0]
    for j in range(p.n_jobs):
        got = rows[int(off[j]):int(off[j + 1])].astype(np.int64)
        if assign[j] < 0 or got[0] < 0:
            assert (got == -1).all() and level[j] == 0
            continue
        c = int(p.job_class[j])
        r0, r1 = domain_rows(p, p.classes[c].level, int(assign[j]))
        cap = row_caps(p, c)[0][r0:r1]
        cnt = np.bincount(got - r0, minlength=r1 - r0)
        assert (cnt <= cap).all() and cnt.sum() == p.classes[c].pods and cnt.max() == level[j]
        share = -(-p.classes[c].pods // int((cap > 0).sum()))
        assert cap[cap > 0].min() < share or cnt.max() <= share
        assert got[0] == first[int(off[j])]
    return rows, first


def one_domain(n, kind, seed=0):
    """One job on leaf 1 of [LEAD, n, 2] rows; the class requests one unit, so cap = min(pods, free)."""
    rng = np.random.default_rng(seed + n)
    free = np.ones(LEAD + n + 2, dtype=np.int64)
    taints = np.zeros_like(free)
    dom = slice(LEAD, LEAD + n)
    no_label = []
    if kind == "ones":
        pods = n // 2 + 1
    elif kind in ("exact", "one", "early", "late"):
        free[dom] = rng.integers(0, 8, n)
        free[LEAD] = 7
        pods = 1 if kind == "one" else int(free[dom].sum())
        if kind in ("early", "late"):  # rows that fail the taints and the selector; L = 4 with rem inside the high rows
            taints[dom] = rng.random(n) < 0.1
            tail = [LEAD + n - 1] if n == 5 else [LEAD + n - 2, LEAD + n - 1]  # the last two rows are high
            free[[LEAD + 2] + tail] = 5
            taints[[LEAD, LEAD + 2] + tail] = 0
            taints[LEAD + 1] = 1
            no_label = [LEAD + 3]
            eff = np.where(taints[dom] != 0, 0, free[dom])
            eff[3] = 0
            rem = 2 if kind == "early" else int((eff >= 4).sum()) - 1
            pods = int(np.minimum(eff, 3).sum()) + rem
            assert even_takes(eff, pods)[1:] == (4, rem) and 0 < rem < int((eff >= 4).sum())
            last = LEAD + int(np.flatnonzero(np.cumsum(eff >= 4) == rem)[0])  # the last row that gets the extra pod
            assert (last >= 1024) == (kind == "late" and LEAD + n - 2 >= 1024)  # in the first chunk / a later one
    else:  # big1 / big2: rows of capacity pods among rows of capacity 3
        pods = 70000
        free[dom] = 3
        free[LEAD + n // 2] = pods
        if kind == "big2":
            free[LEAD + n - 2] = pods
            taints[LEAD + 1] = 1
    p = flat([LEAD, n, 2], [cls(0, pods)], [0], taints=taints, free=[free])
    p.nodes.labels[0, no_label] = 0
    return p


@pytest.mark.parametrize("kind", ["ones", "exact", "early", "late", "one"])
@pytest.mark.parametrize("n,hooks", FORMS)
def test_forms_and_capacities(engine, monkeypatch, n, hooks, kind):
    monkeypatch.setenv("JSP_TEST_HOOKS", hooks)  # read again at every snapshot upload
    p = one_domain(n, kind)
    engine.load(p)
    rows, first = checked(engine, p, [1])
    assert rows[0] == LEAD
    if kind in ("ones", "exact"):
        np.testing.assert_array_equal(rows, first)


@pytest.mark.parametrize("kind", ["big1", "big2"])
@pytest.mark.parametrize("n", [1024 - LEAD, 2051])
def test_a_large_row_among_small_ones(engine, monkeypatch, n, kind):
    """pods = 70000: L above 2^16 in the single chunk; with two large rows rem = 2 ends on the second."""
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    p = one_domain(n, kind)
    cap = row_caps(p, 0)[0][LEAD:LEAD + n]
    _, L, rem = even_takes(cap, 70000)
    assert (L > 65536) == (n < 1024 and kind == "big1") and rem == (2 if kind == "big2" else 1)
    engine.load(p)
    checked(engine, p, [1])


def states_problem():
    """Leaves of 8 rows, pods = 12, 4 units per row (L = 2); leaf 2 has an owned row, leaf 3 holds 11 pods: stale."""
    N = LEAD + 32
    free, taints, excl = np.full(N, 4), np.zeros(N), np.full(N, -1)
    excl[LEAD + 8 + 5] = 7
    taints[LEAD + 16 + 3:LEAD + 24] = 1
    free[LEAD + 16 + 2] = 3
    free[LEAD + 24:] = [0, 9, 1, 2, 9, 0, 1, 9]
    return flat([LEAD, 8, 8, 8, 8], [cls(0, 12)], [0] * 5, taints=taints, excl=excl, free=[free])


@pytest.mark.parametrize("what", ["states", "conflict", "flags", "range", "erange", "sharded"])
def test_states_and_refusals(engine, monkeypatch, what):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    p, good = states_problem(), [1, 2, -1, 3, 4]
    target, assign, kw, code, text = engine, good, {}, native.JSP_EINVAL, None
    if what == "conflict":
        assign, text = [1, 2, 4, 2, 4], "job 3:"
    elif what == "flags":
        kw, text = dict(flags=1), "flags"
    elif what == "range":
        assign, text = [1, 2, -1, 6, 4], "job 3:"
    elif what == "erange":
        p, assign, code = flat([4], [cls(0, 1 << 22, req=0), cls(0, 1)], [0, 0, 0, 0, 1]), [-1] * 5, native.JSP_ERANGE
    if what == "sharded":
        code, text = native.JSP_ESTATE, "sharded"
        p, target = synth.config5(), Engine(0)
        assign = O.place_c(p)[0]
        target.upload_topology(p.topology)
        target.upload_snapshot(shard_problem(p, 0, 2))
        target.upload_classes(p.classes)
    else:
        engine.load(p)
    if what != "states":
        with pytest.raises(native.JspError) as ei:
            target.bind_pods_even_runs(*job_runs(p.job_class), np.asarray(assign, dtype=np.int32), **kw)
        assert ei.value.code == code and (text is None or text in str(ei.value)), str(ei.value)
    if what == "sharded":
        target.close()
    p = states_problem()
    engine.load(p)  # the engine is usable afterwards
    assert checked(engine, p, good)[0][12] == -1 and bind_even_ref(p, np.array(good))[3]["max_per_row"] == 3


def test_nothing_moves(engine, monkeypatch):
    """Behind a placement the resident service answered: its answer, stats.fused and the metrics stay."""
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    engine.set_service(True)
    engine.set_fused(True)
    try:
        p = synth.config2()
        engine.load(p)
        for _ in range(4):
            if engine.place(p.job_class).fused == 3:
                break
        before = engine.place(p.job_class)
        assert before.fused == 3
        np.testing.assert_array_equal(before.assign, O.place_c(p)[0])
        checked(engine, p, before.assign)
        m0 = bytes(engine.metrics())
        engine.bind_pods_even(p.job_class, before.assign)
        assert bytes(engine.metrics()) == m0
        after = engine.place(p.job_class)
        assert after.fused == before.fused
        np.testing.assert_array_equal(after.assign, before.assign)
    finally:
        engine.service_stop()
