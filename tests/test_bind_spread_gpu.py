"""jsp_bind_pods_spread on the GPU against the rule in int64 numpy (tests/bind_spread_ref.py), exactly: pod_row,
pod_off, level and every stats field but wall_us, at every size where a pass takes another form."""
import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import job_runs, shard_problem
from oracle import oracle as O
from bind_ref import cls, nested
from bind_even_ref import even_takes
from bind_spread_ref import bind_spread_ref, group_caps, spread_stats_dict

pytestmark = pytest.mark.gpu
LEAD = 3  # rows of another domain in front, then a group of 4 rows: the middle group starts at row 7 (7 & 3 == 3)
# the wave form's first and last size, the first workgroup size, one chunk exactly, two chunks
SIZES = [5, 256 - LEAD, 257 - LEAD, 1024 - LEAD, 1025]
FORMS = [(n, "") for n in SIZES] + [(n, "bind_wg=1") for n in SIZES[:2]]
GROUPS = [1, 3, 64, 65, 1024, 1025]  # one lane's 4 words, a wave's 256, the registers' 1024, then digits


def checked(engine, p, assign, s):
    """Every output against the yardstick; pod 0 of a bound job is jsp_bind_pods'. (rows, jsp_bind_pods' rows, level)."""
    assign = np.asarray(assign, dtype=np.int32)
    want_rows, want_off, want_level, want = bind_spread_ref(p, assign, s)
    rows, off, level, st = engine.bind_pods_spread(p.job_class, assign, s)
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(level, want_level)
    np.testing.assert_array_equal(rows, want_rows)
    assert spread_stats_dict(st) == want
    first = engine.bind_pods(p.job_class, assign)[0]
    heads = off[:-1][np.diff(off.astype(np.int64)) > 0].astype(np.int64)
    np.testing.assert_array_equal(rows[heads], first[heads])
    return rows, first, level


def three_groups(n, seed=0):
    """Domain 1 of level 0 holds groups of [4, n, 5] rows. The middle group's capacities are random in 0..7 with
    rows that fail the taint and the selector (S in all); every row of the first holds S, the last group 4."""
    rng = np.random.default_rng(seed + n)
    N = LEAD + 4 + n + 5
    mid = slice(LEAD + 4, LEAD + 4 + n)
    free, taints = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    free[LEAD + 4 + n:] = [2, 0, 1, 1, 0]
    free[mid] = rng.integers(0, 8, n)
    free[[LEAD + 4, LEAD + 3 + n]] = 7
    taints[mid] = rng.random(n) < 0.1
    taints[[LEAD + 4, LEAD + 6, LEAD + 3 + n]] = 0
    taints[LEAD + 5] = 1
    S = int(np.where(taints[mid] != 0, 0, free[mid]).sum()) - int(free[LEAD + 6])  # row LEAD + 6 loses its label
    free[LEAD:LEAD + 4] = S
    p = nested([[0, 1, 4], np.arange(5)], [LEAD, 4, n, 5], [cls(0, 4 + 2 * S - 1)], [0], taints=taints, free=[free])
    p.nodes.labels[0, LEAD + 6] = 0
    return p


@pytest.mark.parametrize("n,hooks", FORMS)
def test_group_and_fill_forms(engine, monkeypatch, n, hooks):
    monkeypatch.setenv("JSP_TEST_HOOKS", hooks)  # read again at every snapshot upload
    p = three_groups(n)
    G = group_caps(p, 0, 1, 1)[0]
    _, L, rem = even_takes(G, p.classes[0].pods)
    assert G.min() < L < G.max() and 0 < rem < int((G >= L).sum())
    engine.load(p)
    rows, first, _ = checked(engine, p, [1], 1)
    assert rows[0] == LEAD and (rows != first).any()
    np.testing.assert_array_equal(checked(engine, p, [1], 0)[0], first)  # spread_level == level[c]: one group


def many_groups(g, kind, seed=0):
    """One level-0 domain of g groups of 1 or 2 rows behind LEAD rows of another."""
    rng = np.random.default_rng(seed + g)
    sizes = 1 + (np.arange(g) & 1)
    N = LEAD + int(sizes.sum())
    free = np.concatenate([np.ones(LEAD, dtype=np.int64), rng.integers(0, 8, N - LEAD)])
    free[LEAD] = 5
    pods = max(int(free[LEAD:].sum()) // 2, 1)
    if kind == "exact":
        pods = int(free[LEAD:].sum())
    elif kind == "big":  # one group of capacity pods among groups of capacity 3: L is above 2^16
        pods = 70000
        start = LEAD + np.cumsum(sizes) - sizes
        free[LEAD:] = 1
        free[start] = 4 - sizes
        free[start[g // 2]] = pods
    return nested([[0, 1, g + 1], np.arange(g + 2)], [LEAD] + list(sizes), [cls(0, pods)], [0], free=[free])


@pytest.mark.parametrize("hooks", ["", "spread_digits=1"])
@pytest.mark.parametrize("g,kind", [(g, "half") for g in GROUPS] + [(65, "big"), (65, "exact")])
def test_level_forms(engine, monkeypatch, g, kind, hooks):
    monkeypatch.setenv("JSP_TEST_HOOKS", hooks)
    p = many_groups(g, kind)
    engine.load(p)
    rows, first, level = checked(engine, p, [1], 1)
    if kind == "big":
        assert level[0] > 65536
    if kind == "exact":
        np.testing.assert_array_equal(rows, first)


def test_one_row_per_leaf_is_the_even_rule(engine, monkeypatch):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    rng = np.random.default_rng(7)
    p = nested([[0, 1, 301], np.arange(302)], [1] * 301, [cls(0, 700)], [0], free=[rng.integers(0, 8, 301)])
    engine.load(p)
    rows, _, level = checked(engine, p, [1], 1)
    even = engine.bind_pods_even(p.job_class, np.array([1], dtype=np.int32))
    np.testing.assert_array_equal(rows, even[0])
    np.testing.assert_array_equal(level, even[2])


def states_problem():
    """Three levels: 2 x 4 x 2 leaves. Class 0 (level 0, 20 pods) spreads over the 8 leaves of domain 0, one
    without rows and one tainted; class 1 (level 1, 6 pods) over the 2 leaves of domains 4..7 of level 1:
    bound, stale by an owned row, stale by one pod too few, bound; job 2 is not placed."""
    sizes = [3, 0, 2, 4, 1, 2, 3, 2] + [2, 3, 2, 2, 3, 1, 2, 2]
    N = sum(sizes)
    free, taints, excl = np.full(N, 2), np.zeros(N), np.full(N, -1)
    taints[3:5] = 1               # leaf 2: no capacity
    free[5:9] = [7, 0, 5, 1]      # leaf 3
    excl[17 + 5 + 1] = 9          # level-1 domain 5 (leaves 10, 11): an owned row
    free[17 + 9:17 + 13] = [2, 1, 1, 1]  # level-1 domain 6 (leaves 12, 13): 5 < 6
    free[17 + 13:] = [4, 0, 1, 3]        # level-1 domain 7: L = 3, groups of 4 and 4
    fl = [[0, 8, 16], np.arange(0, 17, 2), np.arange(17)]
    return nested(fl, sizes, [cls(0, 20), cls(1, 6)], [0, 1, 1, 1, 1, 1], taints=taints, excl=excl, free=[free])


GOOD = [0, 4, -1, 5, 6, 7]


@pytest.mark.parametrize("what", ["states", "conflict", "flags", "range", "level", "coarser", "erange", "sharded"])
def test_states_and_refusals(engine, monkeypatch, what):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    p, assign, s = states_problem(), GOOD, 2
    target, kw, code, text = engine, {}, native.JSP_EINVAL, None
    if what == "conflict":
        assign, text = [0, 4, 5, 4, 6, 7], "job 3:"
    elif what == "flags":
        kw, text = dict(flags=1), "flags"
    elif what == "range":
        assign, text = [0, 4, -1, 8, 6, 7], "job 3:"
    elif what == "level":
        s, text = 3, "spread_level"
    elif what == "coarser":
        s, text = 0, "run 1:"
    elif what == "erange":
        p = nested([np.arange(2)], [4], [cls(0, 1 << 22, req=0), cls(0, 1)], [0, 0, 0, 0, 1])
        assign, s, code = [-1] * 5, 0, native.JSP_ERANGE
    if what == "sharded":
        code, text = native.JSP_ESTATE, "sharded"
        p, target, s = synth.config5(), Engine(0), 1
        assign = O.place_c(p)[0]
        target.upload_topology(p.topology)
        target.upload_snapshot(shard_problem(p, 0, 2))
        target.upload_classes(p.classes)
    else:
        engine.load(p)
    if what != "states":
        with pytest.raises(native.JspError) as ei:
            target.bind_pods_spread_runs(*job_runs(p.job_class), np.asarray(assign, dtype=np.int32), s, **kw)
        assert ei.value.code == code and (text is None or text in str(ei.value)), str(ei.value)
    if what == "sharded":
        target.close()
    p = states_problem()
    engine.load(p)  # the engine is usable afterwards
    rows, _, level = checked(engine, p, GOOD, 2)
    want = bind_spread_ref(p, np.array(GOOD), 2)[3]
    assert (want["bound"], want["stale"], want["groups_used"]) == (3, 2, 6 + 2 + 2) and list(level) == [4, 3, 0, 0, 0, 3]
    assert (rows[20 + 6:20 + 24] == -1).all()


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
        checked(engine, p, before.assign, 0)
        m0 = bytes(engine.metrics())
        engine.bind_pods_spread(p.job_class, before.assign, 0)
        assert bytes(engine.metrics()) == m0
        after = engine.place(p.job_class)
        assert after.fused == before.fused
        np.testing.assert_array_equal(after.assign, before.assign)
    finally:
        engine.service_stop()
