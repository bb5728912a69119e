"""jsp_explain on the GPU (DESIGN.md §2 "Why a job has no domain"): per class,
the rows that fail its selector, its tolerations or its requests and the
domains of its level that are occupied, too small or feasible. Every count is
an exact integer; the yardstick is explain_ref.reference, a numpy restatement of
the rule (its cap / occ are cross-checked against cpu_ref.c in the random
sweep). Nothing compares the engine with itself."""
import dataclasses

import numpy as np
import pytest

from jobset_amd import host, native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import JobClass, Nodes, Problem, Topology
from oracle import oracle as O

import k8s_fixtures as K
from explain_ref import reference

pytestmark = pytest.mark.gpu

ROW_FIELDS = ("rows", "rows_selector", "rows_taint", "rows_no_capacity", "rows_fit", "rows_occupied")
DOM_FIELDS = ("domains", "dom_occupied", "dom_short", "dom_feasible", "best_short_cap", "best_short_domain")


def as_dict(x: native.JspClassExplain):
    d = {f: int(getattr(x, f)) for f in ROW_FIELDS + DOM_FIELDS}
    d["rows_insufficient"] = [int(v) for v in x.rows_insufficient]
    return d


def check_identities(d):
    assert d["rows"] == d["rows_selector"] + d["rows_taint"] + d["rows_no_capacity"] + d["rows_fit"]
    assert d["domains"] == d["dom_occupied"] + d["dom_short"] + d["dom_feasible"]


def explain_checked(eng, p: Problem):
    """eng.explain() of the loaded problem, every field against the reference."""
    got = [as_dict(x) for x in eng.explain()]
    want = reference(p)[0]
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert g == w, (c, g, w)
        check_identities(g)
    return got


# ------------------------------------------------------------------ 1. random sweep
@pytest.mark.parametrize("seed", range(24))
def test_random_sweep(engine, seed):
    p = synth.random_problem(seed)
    _, cap, occ = reference(p)
    _, cap_c, occ_c = O.place_c(p)  # keeps the reference honest
    np.testing.assert_array_equal(cap, cap_c)
    np.testing.assert_array_equal(occ, occ_c)
    engine.load(p)
    explain_checked(engine, p)


# ------------------------------------------------------------------ 2. padding rows do not count
def flat_problem(N, per, W=1, R=1, classes=None):
    L = (N + per - 1) // per
    sizes = np.full(L, per, dtype=np.int64)
    sizes[-1] = N - per * (L - 1)
    topo, leaf_start = synth._flat_topology(synth.RACK_KEY, sizes)
    nodes = Nodes(leaf_start=leaf_start, labels=np.zeros((W, N), dtype=np.uint64), taints=np.zeros(N, dtype=np.uint32),
                  free=np.zeros((R, N), dtype=np.uint32), excl=np.full(N, -1, dtype=np.int32))
    return Problem(topology=topo, nodes=nodes, classes=classes or [JobClass(pods=1)],
                   job_class=np.zeros(0, dtype=np.uint32))


@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027])
def test_padding_rows_do_not_count(engine, N):
    """The snapshot is padded with rows of labels 0, taints 0, free 0: a class
    with an empty selector, nothing to tolerate and no requests passes them."""
    p = flat_problem(N, 100)
    engine.load(p)
    got = explain_checked(engine, p)
    assert got[0]["rows"] == N and got[0]["rows_fit"] == N


# ------------------------------------------------------------------ 3. many classes
def synthetic(N=3000, per=30, zones=10, W=2, R=2, C=64, seed=11):
    rng = np.random.default_rng(seed)
    L = N // per
    fl0 = (np.arange(zones + 1) * (L // zones)).astype(np.uint32)
    topo = Topology(level_keys=[synth.ZONE_KEY, synth.RACK_KEY], n_domains=[zones, L],
                    first_leaf=[fl0, np.arange(L + 1, dtype=np.uint32)])
    labels = rng.integers(0, 1 << 16, size=(W, N), dtype=np.uint64)
    taints = np.where(rng.random(N) < 0.2, rng.integers(0, 16, size=N), 0).astype(np.uint32)
    free = rng.integers(0, 100, size=(R, N)).astype(np.uint32)
    excl = np.full(N, -1, dtype=np.int32)
    excl[7 * per:9 * per] = 5
    nodes = Nodes(leaf_start=(np.arange(L + 1) * per).astype(np.uint32), labels=labels, taints=taints, free=free,
                  excl=excl)
    classes = []
    for c in range(C):
        req = tuple(int(1 << rng.integers(0, 16)) if rng.random() < 0.5 else 0 for _ in range(W))
        fb = tuple(int(1 << rng.integers(0, 16)) & ~req[w] if rng.random() < 0.3 else 0 for w in range(W))
        level = int(rng.integers(0, 2))
        classes.append(JobClass(req_labels=req, forbid_labels=fb, tolerated_taints=int(rng.integers(0, 16)),
                                level=level, pods=int(rng.integers(1, 40 if level else 400)),
                                req_res=tuple(int(rng.integers(0, 60)) for _ in range(R))))
    return Problem(topology=topo, nodes=nodes, classes=classes, job_class=np.zeros(0, dtype=np.uint32))


def test_many_classes(engine):
    """17 classes (two tally passes) and 64 (the limit): class c's record is
    the one it gets uploaded alone, and the reference's."""
    p = synthetic()
    engine.load(p)
    alone = []
    for jc in p.classes:
        engine.upload_classes([jc])
        alone.append(as_dict(engine.explain()[0]))
    want = reference(p)[0]
    assert alone == want
    for C in (17, 64):
        q = dataclasses.replace(p, classes=p.classes[:C])
        engine.upload_classes(q.classes)
        assert explain_checked(engine, q) == alone[:C]


# ------------------------------------------------------------------ 4. widths
def test_widths_w4_r4(engine):
    """W = 4, R = 4 with the predicate bits in word 3 and the request on resource 3."""
    N = 300
    cls = [JobClass(req_labels=(0, 0, 0, 1 << 63), forbid_labels=(0, 0, 0, 1 << 5), tolerated_taints=1, level=0,
                    pods=2, req_res=(0, 0, 0, 7)),
           JobClass(req_labels=(1, 0, 0, 0), level=0, pods=1, req_res=(0, 0, 0, 0))]
    p = flat_problem(N, 40, W=4, R=4, classes=cls)
    i = np.arange(N)
    p.nodes.labels[3] = np.where(i % 2 == 0, np.uint64(1 << 63), np.uint64(0)) | \
        np.where(i % 10 == 0, np.uint64(1 << 5), np.uint64(0))
    p.nodes.labels[0] = np.uint64(1)
    p.nodes.taints[:] = np.where(i % 3 == 0, 1, 0) | np.where(i % 7 == 0, 2, 0)
    p.nodes.free[3] = i % 15
    engine.load(p)
    got = explain_checked(engine, p)
    sel = (i % 2 == 0) & (i % 10 != 0)
    tnt = i % 7 != 0
    assert got[0]["rows_selector"] == int((~sel).sum())
    assert got[0]["rows_taint"] == int((sel & ~tnt).sum())
    assert got[0]["rows_insufficient"] == [0, 0, 0, int((sel & tnt & (i % 15 < 7)).sum())]
    assert got[1]["rows_taint"] == int((p.nodes.taints != 0).sum())


# ------------------------------------------------------------------ 5. resource edges
@pytest.mark.parametrize("req", [1, 2, 1 << 31, (1 << 32) - 1])
def test_resource_edges(engine, req):
    """free = req - 1, req, min(req + 1, 2^32 - 1) on resource 0 crossed with
    4, 5, 6 against a request of 5 on resource 1; resource 2 has no request
    and no free units. Integers are compared, not the f64 capacity."""
    top = (1 << 32) - 1
    f0 = [req - 1, req, min(req + 1, top)]
    p = flat_problem(9, 3, R=3, classes=[JobClass(pods=1, req_res=(req, 5, 0))])
    p.nodes.free[0] = np.repeat(np.array(f0, dtype=np.uint32), 3)
    p.nodes.free[1] = np.tile(np.array([4, 5, 6], dtype=np.uint32), 3)
    engine.load(p)
    g = explain_checked(engine, p)[0]
    assert g["rows_insufficient"] == [3, 3, 0, 0]     # a row short on both counts in both ...
    assert g["rows_no_capacity"] == 5                 # ... and once here
    assert g["rows_fit"] == 4


# ------------------------------------------------------------------ 6. domains
def three_levels(free_gpu):
    """2 zones x 2 blocks x 2 racks x 4 nodes; block 1 (racks 2, 3) is held by
    another exclusive job."""
    topo = Topology(level_keys=[synth.ZONE_KEY, "block", synth.RACK_KEY], n_domains=[2, 4, 8],
                    first_leaf=[np.array([0, 4, 8], dtype=np.uint32), np.array([0, 2, 4, 6, 8], dtype=np.uint32),
                                np.arange(9, dtype=np.uint32)])
    N = 32
    excl = np.full(N, -1, dtype=np.int32)
    excl[8:16] = 77
    nodes = Nodes(leaf_start=(np.arange(9) * 4).astype(np.uint32), labels=np.zeros((1, N), dtype=np.uint64),
                  taints=np.zeros(N, dtype=np.uint32), free=np.asarray(free_gpu, dtype=np.uint32).reshape(1, N),
                  excl=excl)
    return topo, nodes


def test_domains(engine):
    free = np.full(32, 8)
    free[[16, 24]] = 0                                  # racks 4 and 6 hold 3 pods of 8 GPUs
    topo, nodes = three_levels(free)
    mk = lambda level, pods: JobClass(level=level, pods=pods, req_res=(8,))  # noqa: E731
    classes = [mk(0, 16), mk(1, 8), mk(2, 4), mk(2, 1), mk(2, 5), mk(1, 7)]
    p = Problem(topology=topo, nodes=nodes, classes=classes, job_class=np.zeros(0, dtype=np.uint32))
    engine.load(p)
    g = explain_checked(engine, p)
    assert [x["dom_occupied"] for x in g] == [1, 1, 2, 2, 2, 1]
    # zone 1 holds 14 < 16 pods
    assert (g[0]["dom_short"], g[0]["best_short_cap"], g[0]["best_short_domain"]) == (1, 14, 1)
    # blocks 2 and 3 hold 7 each: equal capacity, the lower id
    assert (g[1]["dom_short"], g[1]["dom_feasible"], g[1]["best_short_cap"], g[1]["best_short_domain"]) == (2, 1, 7, 2)
    # racks 4 and 6 hold 3 each
    assert (g[2]["dom_short"], g[2]["dom_feasible"], g[2]["best_short_cap"], g[2]["best_short_domain"]) == (2, 4, 3, 4)
    # no short domain
    assert (g[3]["dom_short"], g[3]["best_short_cap"], g[3]["best_short_domain"]) == (0, 0, -1)
    # every free domain short: the largest (4 pods), lowest id
    assert (g[4]["dom_short"], g[4]["dom_feasible"], g[4]["best_short_cap"], g[4]["best_short_domain"]) == (6, 0, 4, 0)
    # dom_feasible = the distinct domains jsp_place hands out to more jobs of
    # that one class than there are domains
    for c, jc in enumerate(classes):
        engine.upload_classes([jc])
        a = engine.place(np.zeros(topo.n_domains[jc.level] + 2, dtype=np.uint32)).assign
        assert len(set(a[a >= 0].tolist())) == g[c]["dom_feasible"], c


# ------------------------------------------------------------------ 7. several workgroups
def test_multi_workgroup(engine):
    p = synth.config4(n_nodes=1 << 17, n_domains=6000)
    engine.load(p)
    explain_checked(engine, p)


def test_rows_loop_times_both_kernels(engine):
    """jspb_explain_rows_loop (the measurement of DESIGN.md §4) runs the row
    pass and the tally and leaves the engine answering as before."""
    p = synth.config1()
    engine.load(p)
    rows_us, tally_us = engine.explain_rows_loop(3)
    assert rows_us > 0 and tally_us > 0
    explain_checked(engine, p)


# ------------------------------------------------------------------ 8. patches and the resident service
@pytest.mark.parametrize("parked", [False, True])
def test_patch_and_service(engine, parked):
    p = synth.config2()
    bad = set(p.meta["bad_racks"].tolist())
    rack = next(r for r in range(1000) if r not in bad)
    row = rack * 15 + 4
    q = synth.config2()
    q.nodes.taints[row] = 1                             # the class tolerates nothing
    before, after = reference(p)[0][0], reference(q)[0][0]
    a_q = O.place_c(q)[0]
    assert after["rows_taint"] == before["rows_taint"] + 1 and after["dom_short"] == before["dom_short"] + 1
    engine.set_fused(True)
    engine.set_service(True, parked=parked)
    try:
        engine.load(p)
        for _ in range(4):
            got = engine.place(p.job_class)
            if got.fused == 3:
                break
        assert got.fused == 3
        assert as_dict(engine.explain()[0]) == before
        assert engine.place(p.job_class).fused == 3     # the service stayed up through the call
        engine.patch_rows(np.array([row], dtype=np.uint32), taints=np.array([1], dtype=np.uint32))
        assert as_dict(engine.explain()[0]) == after
        got = engine.place(p.job_class)
        assert got.fused == 3
        np.testing.assert_array_equal(got.assign, a_q)
    finally:
        engine.service_stop()
        engine.set_service(True)


# ------------------------------------------------------------------ 9. device set
def test_device_set(engine):
    with Engine(devices=[0, 0]) as multi:
        for p in [synth.config5()] + [synth.random_problem(s) for s in range(4)]:
            engine.load(p)
            multi.load(p)
            one = explain_checked(engine, p)
            assert [as_dict(x) for x in multi.explain()] == one


# ------------------------------------------------------------------ 10. errors
def test_errors():
    lib = native.lib()
    p = synth.config1()
    with Engine(0) as e:
        out = (native.JspClassExplain * 4)()
        e.upload_topology(p.topology)
        assert lib.jsp_explain(e._h, out, 0) == native.JSP_ESTATE      # no snapshot
        e.upload_snapshot(p.nodes)
        assert lib.jsp_explain(e._h, out, 1) == native.JSP_ESTATE      # no classes
        e.upload_classes(p.classes)
        assert lib.jsp_explain(e._h, out, 2) == native.JSP_EINVAL      # one class was uploaded
        assert lib.jsp_explain(e._h, None, 1) == native.JSP_EINVAL
        assert lib.jsp_explain(e._h, out, 1) == native.JSP_OK
        assert as_dict(out[0]) == reference(p)[0][0]


# ------------------------------------------------------------------ 11. host mirror
def test_host_mirror(engine):
    """cfg1's node pools as Node objects and one more job than pools: the
    fifth job is explained, and planner.plan answers as before."""
    p = synth.config1()
    pools = p.topology.n_domains[0]
    p.job_class = np.zeros(pools + 1, dtype=np.uint32)
    c = host.Cache()
    K.load_cache(c, p)
    res = K.res_names(p.nodes.n_res)
    c.planner_new(engine, [K.level_key(0)], res)
    jobs = K.job_objects(p)
    assert c.plan(jobs)[1] is None                     # the first plan uploads the snapshot
    plan1 = c.plan(jobs)
    r, err = c.explain(jobs)
    assert err is None
    assert len(r["unplaceable"]) == 1
    (x,) = r["explanations"]
    assert x["jobs"] == r["unplaceable"] and x["class"] == 0
    assert x["counts"]["domFeasible"] == pools and x["counts"]["domains"] == pools
    assert x["counts"]["rows"] == p.nodes.n_nodes
    assert x["message"] == host.explainMessage(x["counts"], K.level_key(0), p.classes[0].pods, res, "")
    assert x["message"].startswith(f"{pools}/{pools} {K.level_key(0)} domains can hold a job of 3 pods.")
    assert {k: v for k, v in r.items() if k != "explanations"} == plan1[0]
    assert c.plan(jobs) == plan1
