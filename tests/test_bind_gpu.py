"""jsp_bind_pods on the GPU against the rule restated in plain numpy
(tests/bind_ref.py; it never calls the engine). Every comparison is exact:
pod_row, pod_off and every stats field. Cases run in both forms of the bind
kernel: the default (one wave per job for domains of up to 256 rows, one
workgroup per job above) and, forced by the bind_wg hook, the workgroup form
for every job."""
import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import JobClass, Nodes, Problem, shard_problem
from oracle import oracle as O
from bind_ref import (BindConflict, bind_ref, case1, case2, case3, check_bind, cls, flat, leaf_sums, nested,
                      stats_dict)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["auto", "wg"])
def form(request, monkeypatch):
    """The bind form: the hook string is read again at every snapshot upload."""
    if request.param == "wg":
        monkeypatch.setenv("JSP_TEST_HOOKS", "bind_wg=1")
    else:
        monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    return request.param


def bind_checked(engine, p, assign):
    """engine.bind_pods of the loaded problem p, every output against the yardstick."""
    assign = np.asarray(assign, dtype=np.int32)
    want_rows, want_off, want = bind_ref(p, assign)
    rows, off, st = engine.bind_pods(p.job_class, assign)
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(rows, want_rows)
    assert stats_dict(st) == want
    return rows, off, st


def run(engine, p, assign):
    engine.load(p)
    return bind_checked(engine, p, assign)


# ------------------------------------------------------------------ 1-3. the hand-computed cases
def test_job_order_is_not_domain_order(engine, form):
    p, assign = case1()
    rows, off, st = run(engine, p, assign)
    np.testing.assert_array_equal(rows, [4, 5, -1, -1, 0, 1])
    np.testing.assert_array_equal(off, [0, 2, 4, 6])
    assert (st.bound, st.stale, st.rows_used, st.pods_bound) == (2, 0, 4, 4)


def test_uneven_caps_and_the_clamp(engine, form):
    rows, _, _ = run(engine, *case2(pods=5, free=3))
    np.testing.assert_array_equal(rows, [0, 0, 0, 2, 2])
    rows, _, st = run(engine, *case2(pods=2, free=5))
    np.testing.assert_array_equal(rows, [0, 0])
    assert st.rows_used == 1


def test_requests_nothing(engine, form):
    rows, _, st = run(engine, *case3())
    assert rows.shape == (4096,) and (rows == 1).all() and st.rows_used == 1


# ------------------------------------------------------------------ 4. saturation
def test_saturation(engine, form):
    """A class that requests nothing with 2^20 pods on a zone of 5 x 1,000 rows:
    the sum of cap is 5,000 x 2^20 > 2^32; row 0 is tainted."""
    taints = np.zeros(5000, dtype=np.uint32)
    taints[0] = 1
    p = nested([[0, 5], np.arange(6)], [1000] * 5, [cls(0, 1 << 20, req=0)], [0], taints=taints)
    rows, off, st = run(engine, p, [0])
    assert int(off[1]) == 1 << 20 == st.pods == st.pods_bound and st.bound == 1
    assert (rows == 1).all() and st.rows_used == 1


# ------------------------------------------------------------------ 5. domain sizes at the edges of both forms
@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_domain_size_edges(engine, form, rows, lead):
    """One pod per row, the middle row tainted, pods = rows - 1 (one row: no
    taint and one pod -- a class has at least one); `lead` rows of another
    leaf in front, so the domain starts on and off a 4-row boundary."""
    sizes = ([lead] if lead else []) + [rows, 2]
    d = 1 if lead else 0
    taints = np.zeros(sum(sizes), dtype=np.uint32)
    if rows > 1:
        taints[lead + rows // 2] = 1
    p = flat(sizes, [cls(0, max(rows - 1, 1))], [0], taints=taints)
    got, _, st = run(engine, p, [d])
    assert st.bound == 1 and st.rows_used == max(rows - 1, 1)
    assert got[0] == lead


def test_empty_leaves_and_empty_domain(engine, form):
    """Zone 0 = two empty leaves, a full one and another empty one; zone 1 has no rows at all."""
    p = nested([[0, 4, 6, 7], np.arange(8)], [0, 0, 5, 0, 0, 0, 3], [cls(0, 5), cls(0, 3)], [0, 1, 1])
    rows, _, st = run(engine, p, [0, 1, 2])
    np.testing.assert_array_equal(rows, [0, 1, 2, 3, 4, -1, -1, -1, 5, 6, 7])
    assert (st.bound, st.stale) == (2, 1)


# ------------------------------------------------------------------ 6. stale
def test_stale_occupied_and_short(engine, form):
    excl = [-1, -1, -1, 7, -1, -1]     # leaf 1 holds a row of another exclusive job
    taints = [0, 0, 0, 0, 0, 1]        # leaf 2 is one pod short
    p = flat([2, 2, 2], [cls(0, 2)], [0, 0, 0], taints=taints, excl=excl)
    rows, _, st = run(engine, p, [1, 0, 2])
    np.testing.assert_array_equal(rows, [-1, -1, 0, 1, -1, -1])
    assert (st.bound, st.stale, st.pods_bound) == (1, 2, 2)


def test_service_patch_then_bind(engine, form):
    """A placement answered by the resident service, a patch, then the bind:
    ordered after the patch, and the service stays up with its tiles."""
    engine.set_service(True)
    engine.set_fused(True)
    try:
        p = synth.config2()
        engine.load(p)
        for _ in range(4):
            if engine.place(p.job_class).fused == 3:
                break
        placed = engine.place(p.job_class)
        assert placed.fused == 3
        assign = placed.assign.copy()
        np.testing.assert_array_equal(assign, O.place_c(p)[0])
        _, _, st = bind_checked(engine, p, assign)
        assert st.stale == 0 and st.bound == int((assign >= 0).sum())
        r = int(assign[5])
        row = next(n for n in range(r * 15, r * 15 + 15) if p.nodes.taints[n] == 0)
        engine.patch_rows(np.array([row], dtype=np.uint32), taints=np.array([1], dtype=np.uint32))
        before = bind_ref(p, assign)[0]
        p.nodes.taints[row] = 1
        rows, off, st = bind_checked(engine, p, assign)          # at once: ordered after the patch
        assert st.stale == 1 and (rows[int(off[5]):int(off[6])] == -1).all()
        keep = np.ones(rows.shape[0], dtype=bool)
        keep[int(off[5]):int(off[6])] = False
        np.testing.assert_array_equal(rows[keep], before[keep])  # the other jobs are unchanged
        after = engine.place(p.job_class)                        # the service kept its tiles
        assert after.fused == 3
        np.testing.assert_array_equal(after.assign, O.place_c(p)[0])
    finally:
        engine.service_stop()


# ------------------------------------------------------------------ 7. nested
def tree8():
    """2 zones x 2 racks x 2 leaves, one row per leaf; a zone job needs its 4 rows, a rack job 2, a leaf job 1."""
    return [np.array([0, 4, 8]), np.array([0, 2, 4, 6, 8]), np.arange(9)], [cls(0, 4), cls(1, 2), cls(2, 1)]


def test_nested(engine, form):
    fl, classes = tree8()
    p = nested(fl, [1] * 8, classes, [1, 2, 0, 2, 1])
    engine.load(p)
    assign = engine.place(p.job_class).assign
    np.testing.assert_array_equal(assign, O.place_c(p)[0])
    assert (assign >= 0).sum() >= 3
    _, _, st = bind_checked(engine, p, assign)
    assert st.bound == int((assign >= 0).sum())


def test_nested_hand_permuted(engine, form):
    fl, classes = tree8()
    p = nested(fl, [1] * 8, classes, [2, 1, 0, 2, 1])
    rows, _, st = run(engine, p, [7, 2, 0, 6, -1])              # leaf 7, rack 2, zone 0, leaf 6
    np.testing.assert_array_equal(rows, [7, 4, 5, 0, 1, 2, 3, 6, -1, -1])
    assert (st.bound, st.rows_used) == (4, 8)


# ------------------------------------------------------------------ 8. refusals
def refused(engine, p, assign, code, text=None, **kw):
    with pytest.raises(native.JspError) as ei:
        rc, rl = synth_runs(p.job_class)
        engine.bind_pods_runs(rc, rl, np.asarray(assign, dtype=np.int32), **kw)
    assert ei.value.code == code, str(ei.value)
    if text is not None:
        assert text in str(ei.value), str(ei.value)


def synth_runs(job_class):
    from jobset_amd.snapshot import job_runs
    return job_runs(job_class)


def test_refusals_leave_the_engine_usable(engine, form):
    fl, classes = tree8()
    p = nested(fl, [1] * 8, classes, [1, 2, 1, 0, 1])
    engine.load(p)
    good = [3, 0, 2, -1, 1]
    for assign, bad in (([2, 0, 2, -1, -1], 2),       # the same rack twice
                        ([2, 0, 3, 1, -1], 3),        # zone 1 after racks 2 and 3 inside it
                        ([0, 5, 3, 0, -1], 3),        # zone 0 after rack 0
                        ([-1, 1, 0, 1, 3], 2),        # rack 0 after its leaf 1 (job 4, in zone 1, is later still)
                        ([-1, 5, -1, 1, 3], 3)):      # zone 1 after its leaf 5 (and before its rack 3: job 4)
        with pytest.raises(BindConflict) as ei:
            bind_ref(p, np.array(assign))
        assert ei.value.job == bad
        refused(engine, p, assign, native.JSP_EINVAL, f"job {bad}:")
        bind_checked(engine, p, good)
    refused(engine, p, [3, 8, 2, -1, 1], native.JSP_EINVAL, "job 1:")      # leaves are 0..7
    refused(engine, p, [3, 0, 2, 2, 1], native.JSP_EINVAL, "job 3:")       # zones are 0..1
    refused(engine, p, [3, 0, -2, -1, 1], native.JSP_EINVAL, "job 2:")
    refused(engine, p, good, native.JSP_EINVAL, "flags", flags=1)
    bind_checked(engine, p, good)


def test_domains_without_leaves_intersect_nothing(engine, form):
    """Rack 2 has no leaves (it sits at leaf 4, where zone 1 begins): bound
    twice and beside zone 1 it conflicts with nothing and is stale. Rack 3,
    leaves 4-5, does conflict with zone 1."""
    fl = [np.array([0, 4, 8]), np.array([0, 2, 4, 4, 6, 8]), np.arange(9)]
    classes = [cls(0, 4), cls(1, 2), cls(2, 1)]
    p = nested(fl, [1] * 8, classes, [0, 1, 1, 1])
    rows, _, st = run(engine, p, [1, 2, 2, 0])
    np.testing.assert_array_equal(rows, [4, 5, 6, 7, -1, -1, -1, -1, 0, 1])
    assert (st.bound, st.stale) == (2, 2)
    with pytest.raises(BindConflict) as ei:
        bind_ref(p, np.array([1, 2, 2, 3]))
    assert ei.value.job == 3
    refused(engine, p, [1, 2, 2, 3], native.JSP_EINVAL, "job 3:")
    # the last rack has no leaves and no leaf position inside any zone
    fl = [np.array([0, 4, 8]), np.array([0, 2, 4, 6, 8, 8]), np.arange(9)]
    p = nested(fl, [1] * 8, classes, [1, 1, 0, 1])
    rows, _, st = run(engine, p, [4, 0, 1, 4])
    np.testing.assert_array_equal(rows, [-1, -1, 0, 1, 4, 5, 6, 7, -1, -1])
    assert (st.bound, st.stale) == (2, 2)


def test_kernel_loop_after_a_refused_call_is_estate(engine, form):
    """jspb_bind_kernel_loop repeats the last successful call's launches; a
    refused call rewrites their staging, so there is nothing to repeat."""
    p, assign = case1()
    run(engine, p, assign)
    assert all(t > 0 for t in engine.bind_kernel_loop(2))
    refused(engine, p, [2, 3, 0], native.JSP_EINVAL, "job 1:")
    with pytest.raises(native.JspError) as ei:
        engine.bind_kernel_loop(2)
    assert ei.value.code == native.JSP_ESTATE
    refused(engine, p, [2, 2, 0], native.JSP_EINVAL, "job 1:")   # a conflict, found after the launches
    with pytest.raises(native.JspError) as ei:
        engine.bind_kernel_loop(2)
    assert ei.value.code == native.JSP_ESTATE
    bind_checked(engine, p, assign)
    assert all(t > 0 for t in engine.bind_kernel_loop(2))


def test_zone_and_rack_in_either_order(engine, form):
    fl, classes = tree8()
    for job_class, assign in (([0, 1, 2], [1, 3, 0]), ([2, 1, 0], [0, 3, 1])):
        p = nested(fl, [1] * 8, classes, job_class)
        engine.load(p)
        refused(engine, p, assign, native.JSP_EINVAL, "job 1:" if job_class[0] == 0 else "job 2:")
        bind_checked(engine, p, [-1, assign[1], -1])


def test_too_many_pods_is_erange(engine):
    """One pod over the limit. A class holds at most 2^22 pods, so it takes five jobs."""
    p = flat([4], [cls(0, 1 << 22, req=0), cls(0, 1)], [0, 0, 0, 0, 1])
    engine.load(p)
    assert 4 * (1 << 22) + 1 == native.JSP_BIND_MAX_PODS + 1
    refused(engine, p, [-1] * 5, native.JSP_ERANGE)
    q = flat([4], [cls(0, 2)], [0])
    np.testing.assert_array_equal(run(engine, q, [0])[0], [0, 1])


def test_device_set_and_sharded_engines_are_estate():
    p = synth.config5()
    assign = O.place_c(p)[0]
    with Engine(devices=[0, 0]) as multi:
        multi.load(p)
        refused(multi, p, assign, native.JSP_ESTATE, "device-set")
    with Engine(0) as e:
        e.upload_topology(p.topology)
        e.upload_snapshot(shard_problem(p, 0, 2))
        e.upload_classes(p.classes)
        refused(e, p, assign, native.JSP_ESTATE, "sharded")
    lib = native.lib()
    with Engine(0) as e:
        out = np.zeros(4, dtype=np.int32)
        one = np.ones(1, dtype=np.uint32)
        zero = np.zeros(1, dtype=np.uint32)
        assert lib.jsp_bind_pods(e._h, zero.ctypes.data, one.ctypes.data, 1, out.ctypes.data, 0, out.ctypes.data,
                                 None, None) == native.JSP_ESTATE   # no topology yet


# ------------------------------------------------------------------ 9. every (W, R) instantiation
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_all_label_and_resource_widths(engine, form, W, R):
    """2 leaves, 5 rows; the class selects on the last label word and requests the last resource."""
    N = 5
    labels = np.zeros((W, N), dtype=np.uint64)
    labels[W - 1] = [1, 1, 0, 1, 1]                    # row 2 fails the selector
    free = np.full((R, N), 9, dtype=np.uint32)
    free[R - 1] = [4, 1, 9, 5, 2]
    base = flat([3, 2], [cls(0, 1)], [0])
    nodes = Nodes(leaf_start=base.nodes.leaf_start, labels=labels, taints=np.zeros(N, dtype=np.uint32), free=free,
                  excl=np.full(N, -1, dtype=np.int32))
    jc = JobClass(req_labels=(0,) * (W - 1) + (1,), level=0, pods=3, req_res=(0,) * (R - 1) + (2,))
    p = Problem(topology=base.topology, nodes=nodes, classes=[jc], job_class=np.array([0, 0], dtype=np.uint32))
    rows, _, st = run(engine, p, [1, 0])
    np.testing.assert_array_equal(rows, [3, 3, 4, -1, -1, -1])   # leaf 1: caps 2, 1; leaf 0: caps 2, 0, (0): short
    assert (st.bound, st.stale) == (1, 1)


# ------------------------------------------------------------------ 10. random sweep
def test_random_sweep(engine, form):
    """seeds 0-59 with the CPU oracle's placement: 44 seeds place a job (998
    jobs, 44,368 pods, the largest placed domain 329 rows)."""
    bound = pods = seeds = want_bound = want_pods = 0
    for seed in range(60):
        p = synth.random_problem(seed)
        assign, cap_c, occ_c = O.place_c(p)
        cap, occ = leaf_sums(p)                                   # keeps the yardstick honest
        np.testing.assert_array_equal(cap, cap_c)
        np.testing.assert_array_equal(occ, occ_c)
        rows, off, st = run(engine, p, assign)
        assert check_bind(p, assign, rows, off) == (st.bound, st.pods_bound)
        want = bind_ref(p, assign)[2]
        want_bound += want["bound"]
        want_pods += want["pods_bound"]
        bound += st.bound
        pods += st.pods_bound
        seeds += 1 if st.bound else 0
    assert (bound, pods) == (want_bound, want_pods) and bound > 0
    assert seeds >= 40


# ------------------------------------------------------------------ 11. mid-size
def test_config5(engine, form):
    """Rack jobs of 16 rows beside zone jobs of 2,048 rows and 2,048 pods (the
    workgroup form in either case). The config's own zones are each a few
    nodes short, so its placement leaves the zone jobs out; with zone 1 made
    whole the first zone job is placed there and bound."""
    p = synth.config5()
    engine.load(p)
    assign = engine.place(p.job_class).assign
    np.testing.assert_array_equal(assign, O.place_c(p)[0])
    _, _, st = bind_checked(engine, p, assign)
    assert st.bound == int((assign >= 0).sum()) == 496
    r0, r1 = 2048, 4096
    p.nodes.taints[r0:r1] = 0
    p.nodes.excl[r0:r1] = -1
    p.nodes.labels[0, r0:r1] |= np.uint64(1)
    p.nodes.free[:, r0:r1] = p.nodes.free.max(axis=1)[:, None]
    engine.load(p)
    assign = engine.place(p.job_class).assign
    np.testing.assert_array_equal(assign, O.place_c(p)[0])
    assert assign[1] == 1 and p.classes[int(p.job_class[1])].level == 0
    rows, off, st = bind_checked(engine, p, assign)
    np.testing.assert_array_equal(rows[int(off[1]):int(off[2])], np.arange(r0, r1))
    assert st.bound == 497 and st.pods_bound == 9984


def test_config4_reduced(engine, form):
    """40,000 jobs: above 1,024 the kernels read the input's device copy."""
    p = synth.config4(n_nodes=1 << 17, n_domains=6000)
    engine.load(p)
    assign = engine.place(p.job_class).assign
    _, _, st = bind_checked(engine, p, assign)
    assert st.bound == int((assign >= 0).sum()) > 0


# ------------------------------------------------------------------ 12. the timed loop
def test_bind_loop_leaves_the_last_answer(engine, form):
    p = synth.config2()
    engine.load(p)
    assign = O.place_c(p)[0]
    rows, _, st = bind_checked(engine, p, assign)
    from jobset_amd.snapshot import job_runs
    rc, rl = job_runs(p.job_class)
    (total, med, p99), loop_rows, loop_st = engine.bind_loop(rc, rl, assign, iters=5)
    np.testing.assert_array_equal(loop_rows, rows)
    assert stats_dict(loop_st) == stats_dict(st)
    assert 0 < med <= p99 <= total
