"""jsp_resolve_leader_domains and jsp_audit_placements at their edges, on a
single engine and on a device set of three shards. The yardstick is
call_sequences.row_domain / audit_ref (searchsorted on leaf_start, then on the
level's first_leaf; tests/test_call_sequences.py checks it against a table
built row by row). resolve_kernel takes 256 rows per workgroup; audit_kernel
packs 4 jobs per workgroup, one wave each, 64 lanes striding over the job's
followers: the batch sizes and follower counts sit on both sides of each."""
import numpy as np
import pytest

from jobset_amd import native
from bind_ref import cls, nested
from call_sequences import audit_ref, row_domain, world_problem
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INT32_MIN = -(1 << 31)
NO_LEVEL = 0xFFFFFFFF
COUNTS = (0, 1, 63, 64, 65, 200)


def topo(first_leaf, sizes):
    return nested(first_leaf, sizes, [cls(len(first_leaf) - 1, 1)], [])


def topologies():
    big = [1 + (7 * i) % 11 for i in range(48)]                  # 48 leaves, 288 rows
    return {
        "K1": topo([np.arange(5)], [4, 1, 7, 2]),
        # four levels, the upper ones cut at uneven places
        "K4": topo([[0, 5, 12], [0, 2, 5, 9, 12], [0, 1, 2, 4, 5, 7, 9, 10, 12], np.arange(13)],
                   [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]),
        # leaves without rows at the front, in the middle and at the end; zone 0 holds none at all
        "empty": topo([[0, 2, 4, 8, 10], np.arange(11)], [0, 0, 3, 0, 2, 5, 0, 0, 1, 0]),
        "one-row": topo([np.arange(2)], [1]),
        "one-row-K2": topo([[0, 3], np.arange(4)], [0, 1, 0]),
        # three levels, 288 rows: every shard of a device set holds several zones
        "big": topo([[0, 6, 13, 20, 29, 35, 41, 48], [0, 2, 6, 9, 13, 17, 20, 25, 29, 33, 35, 38, 41, 44, 48],
                     np.arange(49)], big),
    }


TOPOS = topologies()


@pytest.fixture(scope="module")
def device_set():
    from jobset_amd.engine import Engine
    e = Engine(devices=[0, 0, 0])
    yield e
    e.close()


@pytest.fixture(params=["single", "device-set"])
def eng(request, engine):
    if request.param == "single":
        engine.service_stop()
        return engine
    return request.getfixturevalue("device_set")


def leaders(p, n):
    """n leader rows and levels: every row of the snapshot in turn (so every
    shard and both sides of every shard boundary), the edge rows -1, INT32_MIN,
    N, N - 1 and 0 in between, every level, and the two that do not exist."""
    N, K = p.nodes.n_nodes, p.topology.n_levels
    i = np.arange(n, dtype=np.int64)
    rows = (i * 5) % N if N > 1 else np.zeros(n, dtype=np.int64)
    edge = np.array([-1, INT32_MIN, N, N - 1, 0], dtype=np.int64)
    rows = np.where(i % 4 == 3, edge[(i // 4) % 5], rows)
    lv = np.array(list(range(K)) + [K, NO_LEVEL], dtype=np.int64)[(i // 2) % (K + 2)]
    lv = np.where(i % 7 == 0, i % K, lv)                          # enough valid ones
    return rows.astype(np.int32), lv.astype(np.uint32)


def followers(p, rows, levels, shift):
    """Follower lists with COUNTS[(i + shift) % 6] entries: the leader's
    domain, now and then another one or -1; every twelfth job's only wrong
    follower sits at position 64."""
    ld = row_domain(p, rows, levels).astype(np.int64)
    cnt = np.array([COUNTS[(i + shift) % 6] for i in range(rows.shape[0])], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    fd = np.repeat(ld, cnt)
    job = np.repeat(np.arange(rows.shape[0]), cnt)
    pos = np.arange(fd.shape[0]) - off[:-1].astype(np.int64)[job]
    wrong = (job * 7 + pos * 3) % 11 == 0
    none = (job + pos) % 13 == 0
    lone = (job + shift) % 12 == 4                                # a job of 65 followers
    fd = np.where(lone, np.where(pos == 64, fd + 1, fd), np.where(none, -1, np.where(wrong, fd + 1, fd)))
    return off, fd.astype(np.int32)


# ------------------------------------------------------------------ 1. resolve
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
@pytest.mark.parametrize("name", list(TOPOS))
def test_resolve(eng, name, n):
    p = TOPOS[name]
    eng.load(p)
    rows, lv = leaders(p, n)
    want = row_domain(p, rows, lv)
    got = eng.resolve_leader_domains(rows, lv)
    np.testing.assert_array_equal(got, want)
    if n >= 255:
        assert (want >= 0).sum() > n // 4 and (want < 0).sum() > n // 8


def test_resolve_every_row_every_level(eng):
    """K = 4: every row at every level, and at the two levels that do not exist."""
    p = TOPOS["K4"]
    eng.load(p)
    N = p.nodes.n_nodes
    for k in (0, 1, 2, 3, 4, NO_LEVEL):
        rows = np.arange(-1, N + 1, dtype=np.int32)
        lv = np.full(rows.shape, k, dtype=np.uint32)
        np.testing.assert_array_equal(eng.resolve_leader_domains(rows, lv), row_domain(p, rows, lv))


# ------------------------------------------------------------------ 2. audit
@pytest.mark.parametrize("n_jobs,shift", [(1, 5), (3, 2), (4, 0), (5, 0), (5, 1), (1000, 0)])
@pytest.mark.parametrize("name", list(TOPOS))
def test_audit(eng, name, n_jobs, shift):
    p = TOPOS[name]
    eng.load(p)
    rows, lv = leaders(p, n_jobs)
    if n_jobs <= 5:
        rows, lv = rows.copy(), lv.copy()
        rows[:3], lv[:3] = p.nodes.n_nodes - 1, p.topology.n_levels - 1       # leaders that have a domain
    off, fd = followers(p, rows, lv, shift)
    want = audit_ref(p, rows, lv, off, fd)
    got = eng.audit_placements(rows, lv, off, fd)
    np.testing.assert_array_equal(got, want)
    if n_jobs == 1000:
        assert (want == 0).any() and (want == 0xFFFFFFFF).any() and ((want > 0) & (want < 200)).any()


def test_audit_lone_wrong_follower_at_position_64(eng):
    """65 followers, the 65th alone names another domain (the second trip of
    lane 0); beside it the same job with the 64th, and one all right."""
    p = TOPOS["K4"]
    eng.load(p)
    rows = np.array([20, 20, 20, 20, 20], dtype=np.int32)
    lv = np.array([2, 2, 2, 2, 2], dtype=np.uint32)
    d = int(row_domain(p, rows[:1], lv[:1])[0])
    lists = [np.full(65, d), np.full(65, d), np.full(65, d), np.full(200, d), np.full(64, d)]
    lists[0][64] = d + 1
    lists[1][63] = -1
    lists[3][[64, 128, 192, 199]] = [d - 1, -1, d + 1, 0 if d else 1]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    fd = np.concatenate(lists).astype(np.int32)
    np.testing.assert_array_equal(audit_ref(p, rows, lv, off, fd), [1, 1, 0, 4, 0])
    np.testing.assert_array_equal(eng.audit_placements(rows, lv, off, fd), [1, 1, 0, 4, 0])


def test_device_set_keeps_the_order_of_jobs(device_set, engine):
    """Leaders dealt over the shards in an order that interleaves them: the
    answers come back by job, and equal the single engine's."""
    p = TOPOS["big"]
    engine.service_stop()
    N = p.nodes.n_nodes
    order = (np.arange(N, dtype=np.int64) * 101) % N              # 101 and 288 are coprime: every row once
    rows = order.astype(np.int32)
    lv = (np.arange(N) % 3).astype(np.uint32)
    off, fd = followers(p, rows, lv, 3)
    for e in (device_set, engine):
        e.load(p)
        np.testing.assert_array_equal(e.resolve_leader_domains(rows, lv), row_domain(p, rows, lv))
        np.testing.assert_array_equal(e.audit_placements(rows, lv, off, fd), audit_ref(p, rows, lv, off, fd))
    assert device_set.shards() == (3, 1)


# ------------------------------------------------------------------ 3. refusals, each followed by a correct call
def raw(eng, fn, *args):
    return getattr(eng._lib, fn)(eng._h, *args)


def test_refusals_then_a_correct_call(eng):
    p = TOPOS["K4"]
    eng.load(p)
    rows, lv = leaders(p, 9)
    off, fd = followers(p, rows, lv, 1)
    out_i = np.full(9, 77, dtype=np.int32)
    out_u = np.full(9, 77, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data  # noqa: E731

    def good():
        np.testing.assert_array_equal(eng.resolve_leader_domains(rows, lv), row_domain(p, rows, lv))
        np.testing.assert_array_equal(eng.audit_placements(rows, lv, off, fd), audit_ref(p, rows, lv, off, fd))

    good()
    for args in ((None, ptr(lv), 9, ptr(out_i)), (ptr(rows), None, 9, ptr(out_i)), (ptr(rows), ptr(lv), 9, None)):
        assert raw(eng, "jsp_resolve_leader_domains", *args) == native.JSP_EINVAL
        good()
    for args in ((None, ptr(lv), ptr(off), ptr(fd), 9, ptr(out_u)), (ptr(rows), None, ptr(off), ptr(fd), 9, ptr(out_u)),
                 (ptr(rows), ptr(lv), None, ptr(fd), 9, ptr(out_u)), (ptr(rows), ptr(lv), ptr(off), ptr(fd), 9, None)):
        assert raw(eng, "jsp_audit_placements", *args) == native.JSP_EINVAL
        good()
    assert (out_i == 77).all() and (out_u == 77).all()            # a refused call writes nothing
    # follower_off[0] != 0
    with pytest.raises(native.JspError) as ei:
        eng.audit_placements(rows, lv, off + np.uint32(1), np.concatenate([fd, fd[:1]]))
    assert ei.value.code == native.JSP_EINVAL and "follower_off[0]" in str(ei.value)
    good()
    # offsets that go down
    down = off.copy()
    down[4] = down[3] - 1
    with pytest.raises(native.JspError) as ei:
        eng.audit_placements(rows, lv, down, fd)
    assert ei.value.code == native.JSP_EINVAL and "monotone" in str(ei.value)
    good()
    # followers, and no list of their domains
    with pytest.raises(native.JspError) as ei:
        eng.audit_placements(rows, lv, off, np.zeros(0, dtype=np.int32))
    assert ei.value.code == native.JSP_EINVAL and "follower_domains" in str(ei.value)
    good()
    # no jobs: nothing is read
    assert raw(eng, "jsp_resolve_leader_domains", None, None, 0, None) == native.JSP_OK
    assert raw(eng, "jsp_audit_placements", None, None, None, None, 0, None) == native.JSP_OK
    good()


# ------------------------------------------------------------------ 4. with the resident service up
def test_with_the_resident_service_up(engine):
    """Both calls between two placements the compaction service answers: the
    service keeps its tiles and the placement its answer."""
    p = world_problem(13, "compact")[0]
    want = O.place_c(p)[0]
    rows, lv = leaders(p, 600)
    off, fd = followers(p, rows, lv, 0)
    want_d, want_b = row_domain(p, rows, lv), audit_ref(p, rows, lv, off, fd)
    engine.set_service(True)
    engine.set_fused(True)
    try:
        engine.load(p)
        for _ in range(4):
            if engine.place(p.job_class).fused == 3:
                break
        before = engine.place(p.job_class)
        got_d = engine.resolve_leader_domains(rows, lv)
        mid = engine.place(p.job_class)
        got_b = engine.audit_placements(rows, lv, off, fd)
        after = engine.place(p.job_class)
    finally:
        engine.service_stop()
    assert before.fused == 3 and mid.fused == 3 and after.fused == 3
    for r in (before, mid, after):
        np.testing.assert_array_equal(r.assign, want)
    np.testing.assert_array_equal(got_d, want_d)
    np.testing.assert_array_equal(got_b, want_b)
