"""jsp_place_fit on the GPU against the rule restated over the CPU oracle
(tests/fit_ref.py; it never calls the engine). Every comparison is exact:
assign[] bit for bit, the stats field by field, the candidate lists word for
word with numpy, tails included (tests/test_fit.py asserts the sweep's
coverage floors on the reference's own output). The order step's two forms
are forced through the test hooks, which the engine reads again at every
snapshot upload: fit_form=1 the rank form, fit_form=2 the block form, with
fit_block=64 so that segments of 65 domains and more merge several blocks."""
import dataclasses

import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from bind_ref import cls, nested
from fit_ref import (LOWEST, POLICIES, ROOMIEST, TIGHTEST, fit_ref, hand_cases, order_ref, reduction_problem,
                     stats_dict, sweep_case)

pytestmark = pytest.mark.gpu

FORMS = {"rank": "fit_form=1", "block": "fit_form=2,fit_block=64"}


@pytest.fixture(params=list(FORMS))
def form(request, monkeypatch):
    """The order form: the hook string is read again at every snapshot upload."""
    monkeypatch.setenv("JSP_TEST_HOOKS", FORMS[request.param])
    return request.param


@pytest.fixture
def own_choice(monkeypatch):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)


def run(engine, p, policies=POLICIES, load=True, tallies=None):
    """Load p, place its jobs under each policy, compare with the yardstick."""
    if load:
        engine.load(p)
    tl = tallies if tallies is not None else O.place_c(p)[1:]
    out = {}
    for policy in policies:
        want, want_st = fit_ref(p, policy, tl)
        got, st = engine.place_fit(p.job_class, policy)
        np.testing.assert_array_equal(got, want, err_msg=f"{p.name} policy {policy}")
        assert stats_dict(st) == want_st, (p.name, policy)
        out[policy] = (got, st)
    return out


# ------------------------------------------------------------------ 1. the sweep, once per order form
@pytest.mark.parametrize("seed", range(60))
def test_sweep(engine, form, seed):
    p = sweep_case(seed)[0]
    ans = run(engine, p)
    O.check_invariants(p, ans[TIGHTEST][0], *O.place_c(p)[1:])
    # the same jobs as runs
    rc, rl = job_runs(p.job_class)
    got, st = engine.place_fit_runs(rc, rl, ROOMIEST)
    np.testing.assert_array_equal(got, ans[ROOMIEST][0])
    assert st.runs == len(rc) and st.fused == 7


# ------------------------------------------------------------------ 2. the reduction, on the engine's own jsp_place
@pytest.mark.parametrize("i", range(0, 60, 2))
def test_lowest_is_jsp_place(engine, own_choice, i):
    p = reduction_problem(i)
    engine.load(p)
    plain = engine.place(p.job_class).assign.copy()
    got, st = engine.place_fit(p.job_class, LOWEST)
    np.testing.assert_array_equal(got, plain)
    assert st.placed == int((plain >= 0).sum()) and st.jobs == p.n_jobs


# ------------------------------------------------------------------ 3. the hand cases
@pytest.mark.parametrize("name", ["A", "B", "C", "D22"])
def test_hand_cases(engine, form, name):
    """D runs as D22: the same per-leaf tallies, capsums and answers with
    pods inside the class contract (test_case_d_is_outside_the_class_contract)."""
    p, want = hand_cases()[name]
    ans = run(engine, p)
    for policy in POLICIES:
        np.testing.assert_array_equal(ans[policy][0], want[policy], err_msg=f"case {name} policy {policy}")
    if name == "D22":
        assert want == hand_cases()["D"][1]
        # every job placed: two clamped fits and 2^31, minus three times the pods
        assert [int(ans[q][1].slack) for q in POLICIES] == [2 * 0xFFFFFFFF + (1 << 31) - 3 * (1 << 22)] * 3


def test_case_d_is_outside_the_class_contract(engine, own_choice):
    """Case D's class asks for 2^31 pods; jsp_classes_upload takes at most
    2^22 (jsplace.h), so the engine never sees D itself."""
    p, _ = hand_cases()["D"]
    with pytest.raises(native.JspError) as ei:
        engine.load(p)
    assert ei.value.code == native.JSP_ERANGE and "2^22" in str(ei.value)
    run(engine, hand_cases()["A"][0])


# ------------------------------------------------------------------ 4. the order lists against numpy
def order_case(first_leaf, levels, rows=None, seed=1, pods=(1, 3), taint_p=0.4, held=True, extra=()):
    """rows[l] rows per leaf (default: 1 to 4, by the seed), a share of the
    rows tainted with bit 0; per level in `levels` one class per pods value,
    alternately tolerating nothing and bit 0; every 37th leaf's rows held by
    another job."""
    L = len(first_leaf[-1]) - 1
    rows = synth.uniform_int(seed, 5, L, 1, 4) if rows is None else np.asarray(rows, dtype=np.int64)
    N = int(rows.sum())
    taints = synth.bernoulli(seed, 11, N, taint_p).astype(np.uint32)
    leaf_of = np.repeat(np.arange(L), rows)
    excl = np.where((leaf_of % 37 == 36) & held, 900, -1)
    classes = [cls(k, n, tol=i % 2) for k in levels for i, n in enumerate(pods)] + list(extra)
    p = nested(first_leaf, rows, classes, [], taints=taints, excl=excl)
    p.topology.validate()
    return p


def ident(n):
    return np.arange(n + 1)


def edges(n):
    """level-0 boundaries at and one off the 64-bit word boundaries below n"""
    return np.array(sorted({0, n} | {b for b in (1, 63, 64, 65, 127, 128, 129) if b < n}))


ORDER_CASES = {
    # K = 1 around the word, the tile (256) and the block (64) boundaries
    **{f"K1-D{n}": lambda n=n: order_case([ident(n)], [0]) for n in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)},
    # a class with no feasible domain (nf == 0) beside one that has some
    "K1-none-feasible": lambda: order_case([ident(130)], [0], extra=[cls(0, 1 << 20, tol=1)]),
    # all keys equal: ascending ids
    "K1-equal-keys": lambda: order_case([ident(130)], [0], rows=[2] * 130, pods=(1,), taint_p=0.0, held=False),
    # strictly descending keys: TIGHTEST reverses the ids
    "K1-descending": lambda: order_case([ident(130)], [0], rows=np.arange(130, 0, -1), pods=(1,), taint_p=0.0,
                                        held=False),
    # nested, classes at every level in one upload
    **{f"K2-D{n}": lambda n=n: order_case([edges(n), ident(n)], [1, 0]) for n in (65, 129, 257)},
    # childless domains in front, in the middle and at the end
    "K2-empty-domains": lambda: order_case([[0, 0, 64, 64, 64, 130, 130], ident(130)], [1, 0]),
    # leaves without rows
    "K2-rowless": lambda: order_case([[0, 3, 70, 140], ident(140)], [1, 0],
                                     rows=[0, 0, 0] + [1] * 61 + [0] * 6 + [2] * 70),
    "K3": lambda: order_case([[0, 50, 50, 192, 200],
                              sorted(set(range(0, 50, 2)) | set(range(50, 192, 7)) | {192, 200}), ident(200)], [2, 0, 1]),
    "K4": lambda: order_case([[0, 75, 75, 200], np.arange(0, 201, 25), np.arange(0, 201, 5), ident(200)],
                             [3, 1, 0, 2]),
    # long upper domains: several lanes sum one domain's leaves (2 zones x 700 racks)
    "K3-long": lambda: order_case([[0, 700, 1400], np.r_[np.arange(0, 700, 7), np.arange(700, 1401, 350)],
                                   ident(1400)], [2, 1, 0]),
}


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_order_lists_match_numpy(engine, monkeypatch, name):
    monkeypatch.setenv("JSP_TEST_HOOKS", "fit_block=64")
    p = ORDER_CASES[name]()
    engine.load(p)
    tl = O.place_c(p)[1:]
    some = 0
    for policy in POLICIES:
        want, want_nf = order_ref(p, policy, tl)
        assert want.shape[0] == sum(p.topology.n_domains[jc.level] for jc in p.classes)
        some += int(want_nf.sum())
        for f in (1, 2, 0):
            got, nf, _ = engine.fit_order(policy, form=f)
            np.testing.assert_array_equal(nf, want_nf, err_msg=f"{name} policy {policy} form {f}")
            np.testing.assert_array_equal(got, want, err_msg=f"{name} policy {policy} form {f}")
    assert some > 0  # the case is not empty
    if name == "K1-none-feasible":
        assert want_nf[-1] == 0 and want_nf[0] > 0
    if name == "K1-equal-keys":
        np.testing.assert_array_equal(order_ref(p, TIGHTEST, tl)[0], np.arange(130))
    if name == "K1-descending":
        np.testing.assert_array_equal(order_ref(p, TIGHTEST, tl)[0], np.arange(129, -1, -1))
        np.testing.assert_array_equal(order_ref(p, ROOMIEST, tl)[0], np.arange(130))


def test_fit_order_refusals_and_timing(engine, own_choice):
    p = ORDER_CASES["K3-long"]()
    engine.load(p)
    lib = native.lib()
    n = sum(p.topology.n_domains[jc.level] for jc in p.classes)
    order = np.zeros(n + 1, dtype=np.uint32)
    nf = np.zeros(len(p.classes), dtype=np.uint32)
    us = np.zeros(2)
    for args in ((3, 0, order.ctypes.data, n, nf.ctypes.data, 0, us.ctypes.data),        # policy
                 (0, 3, order.ctypes.data, n, nf.ctypes.data, 0, us.ctypes.data),        # form
                 (0, 0, order.ctypes.data, n + 1, nf.ctypes.data, 0, us.ctypes.data),    # n_order
                 (0, 0, None, n, nf.ctypes.data, 0, us.ctypes.data),                     # order_out
                 (0, 0, order.ctypes.data, n, None, 0, us.ctypes.data)):                 # nf_out
        assert lib.jspb_fit_order(engine._h, *args) == native.JSP_EINVAL
    _, _, (med, mean) = engine.fit_order(TIGHTEST, iters=20)
    assert 0 < med < 1e4 and 0 < mean < 1e4


# ------------------------------------------------------------------ 5. behind the service and behind patches
def rows_of(p, level, d):
    fl = p.topology.first_leaf[level]
    ls = p.nodes.leaf_start
    return np.arange(int(ls[int(fl[d])]), int(ls[int(fl[d + 1])]))


def test_behind_the_service_and_a_patch(engine, own_choice):
    engine.set_service(True)
    engine.set_fused(True)
    try:
        p = synth.config2()
        engine.load(p)
        for _ in range(4):
            if engine.place(p.job_class).fused == 3:
                break
        assert engine.place(p.job_class).fused == 3
        m0 = engine.metrics()
        # one row of a placed rack gets a taint nobody tolerates: the rack's fit drops by one node's pods
        r = int(O.place_c(p)[0][5])
        row = next(n for n in range(r * 15, r * 15 + 15) if p.nodes.taints[n] == 0)
        engine.patch_rows(np.array([row], dtype=np.uint32), taints=np.array([1], dtype=np.uint32))
        p.nodes.taints[row] = 1
        ans = run(engine, p, policies=(TIGHTEST,), load=False)   # at once: behind the patch the dispatcher holds
        _, st = ans[TIGHTEST]
        m1 = engine.metrics()
        assert m1.place_us.count == m0.place_us.count + 1 and m1.batch_jobs.count == m0.batch_jobs.count + 1
        assert m1.placed == m0.placed + st.placed and m1.unplaceable == m0.unplaceable + (st.jobs - st.placed)
        after = engine.place(p.job_class)                        # the service kept its tiles
        assert after.fused == 3
        np.testing.assert_array_equal(after.assign, O.place_c(p)[0])
        run(engine, p, policies=(ROOMIEST, LOWEST), load=False)
        with pytest.raises(native.JspError):
            engine.place_fit_runs([0], [990], TIGHTEST, flags=1)
        assert engine.metrics().place_errors == m1.place_errors + 1
    finally:
        engine.service_stop()


def test_assumed_domains_are_avoided(engine, form):
    p = sweep_case(3)[0]
    got1, _ = run(engine, p, policies=(TIGHTEST,))[TIGHTEST]
    assert (got1 >= 0).any()
    own = 0x40000000 + np.arange(p.n_jobs)
    committed, _ = engine.assume(p.job_class, got1, own)
    assert committed.sum() == (got1 >= 0).sum() > 0
    for jj in np.nonzero(got1 >= 0)[0]:
        p.nodes.excl[rows_of(p, p.classes[int(p.job_class[jj])].level, int(got1[jj]))] = own[jj]
    for policy in POLICIES:
        got2, _ = run(engine, p, policies=(policy,), load=False)[policy]
        held = {(p.classes[int(p.job_class[jj])].level, int(got1[jj])) for jj in np.nonzero(got1 >= 0)[0]}
        assert not held & {(p.classes[int(p.job_class[jj])].level, int(got2[jj])) for jj in np.nonzero(got2 >= 0)[0]}
    engine.forget(own)


# ------------------------------------------------------------------ 6. refusals, each followed by a correct call
def refused(engine, code, word, *args, **kw):
    with pytest.raises(native.JspError) as ei:
        engine.place_fit_runs(*args, **kw)
    assert ei.value.code == code, str(ei.value)
    assert word in str(ei.value), str(ei.value)


def test_refusals_leave_the_engine_usable(engine, own_choice):
    p, want = hand_cases()["C"]
    engine.load(p)
    tl = O.place_c(p)[1:]
    rc, rl = job_runs(p.job_class)
    lib = native.lib()
    one = np.ones(1, dtype=np.uint32)
    out = np.zeros(4, dtype=np.int32)

    def ok():
        run(engine, p, load=False, tallies=tl)

    refused(engine, native.JSP_EINVAL, "policy 3", rc, rl, 3)
    ok()
    refused(engine, native.JSP_EINVAL, "flags 1", rc, rl, TIGHTEST, flags=1)
    ok()
    refused(engine, native.JSP_EINVAL, "run 1", [0, 2, 0], [1, 1, 1], TIGHTEST)       # a class that does not exist
    ok()
    assert lib.jsp_place_fit(engine._h, one.ctypes.data, one.ctypes.data, 1, 1, 0, None, None) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()                                             # assign_out
    ok()
    assert lib.jsp_place_fit(engine._h, None, one.ctypes.data, 1, 1, 0, out.ctypes.data, None) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()                                             # run_class
    ok()
    refused(engine, native.JSP_ERANGE, "limit of 65536", [0], [native.JSP_FIT_MAX_JOBS + 1], TIGHTEST)
    ok()
    got, st = engine.place_fit_runs([], [], TIGHTEST)                                  # J == 0 launches nothing
    assert got.shape == (0,) and (st.jobs, st.placed, st.runs, st.slack, st.fused) == (0, 0, 0, 0, 7)
    got, st = engine.place_fit_runs([0, 1, 0], [1, 0, 1], TIGHTEST)                    # an empty run is not counted
    np.testing.assert_array_equal(got, [3, 4])
    assert (st.jobs, st.placed, st.runs) == (2, 2, 2)


def test_device_set_sharded_and_unloaded_engines_are_estate():
    from jobset_amd.snapshot import shard_problem
    p = synth.config5()
    rc, rl = job_runs(p.job_class)
    with Engine(devices=[0, 0]) as multi:
        multi.load(p)
        refused(multi, native.JSP_ESTATE, "device-set", rc, rl, TIGHTEST)
        with pytest.raises(native.JspError) as ei:
            multi.fit_order(TIGHTEST)
        assert ei.value.code == native.JSP_ESTATE
    with Engine(0) as e:
        e.upload_topology(p.topology)
        e.upload_snapshot(shard_problem(p, 0, 2))
        e.upload_classes(p.classes)
        refused(e, native.JSP_ESTATE, "sharded", rc, rl, TIGHTEST)
        with pytest.raises(native.JspError) as ei:
            e.fit_order(TIGHTEST)
        assert ei.value.code == native.JSP_ESTATE
    lib = native.lib()
    with Engine(0) as e:
        a = np.zeros(1, dtype=np.int32)
        one, zero = np.ones(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        call = lambda: lib.jsp_place_fit(e._h, zero.ctypes.data, one.ctypes.data, 1, 1, 0, a.ctypes.data,  # noqa: E731
                                         None)
        assert call() == native.JSP_ESTATE               # no topology yet
        e.upload_topology(p.topology)
        assert call() == native.JSP_ESTATE               # no snapshot yet
        e.upload_snapshot(p.nodes)
        assert call() == native.JSP_ESTATE               # no classes yet
        e.upload_classes(p.classes)
        assert call() == native.JSP_OK
        np.testing.assert_array_equal(a, fit_ref(dataclasses.replace(p, job_class=zero), TIGHTEST)[0])


def test_class_reupload_with_the_same_geometry(engine, own_choice):
    """The order step's rows and segments follow the classes: a second upload
    with the same class count and levels but other pods is ordered afresh."""
    p = order_case([edges(129), ident(129)], [1, 0])
    run(engine, dataclasses.replace(p, job_class=np.array([0, 2, 1, 3] * 6, dtype=np.uint32)))
    q = dataclasses.replace(p, classes=[dataclasses.replace(jc, pods=jc.pods + 1) for jc in p.classes],
                            job_class=np.array([0, 2, 1, 3] * 6, dtype=np.uint32))
    engine.upload_classes(q.classes)
    run(engine, q, load=False)


# ------------------------------------------------------------------ 7. the real shapes
@pytest.mark.parametrize("cfg", [5, 2])
def test_configs_once_per_policy(engine, own_choice, cfg):
    p = synth.CONFIGS[cfg]()
    ans = run(engine, p)
    assert ans[TIGHTEST][1].placed > 0
    rc, rl = job_runs(p.job_class)
    total, med, p99 = engine.place_fit_loop(rc, rl, TIGHTEST, iters=20)
    assert 0 < med <= p99 and total > 0


@pytest.fixture(scope="module")
def cfg4():
    p = synth.config4(n_nodes=1 << 17, n_domains=6000)
    return p, O.place_c(p)[1:]


@pytest.mark.parametrize("policy", POLICIES)
def test_config4_reduced(engine, own_choice, cfg4, policy):
    """40,000 jobs over 6,000 domains: the block form by the engine's own choice."""
    p, tl = cfg4
    engine.load(p)
    ans = run(engine, p, policies=(policy,), load=False, tallies=tl)
    assert ans[policy][1].placed > 0
    want, want_nf = order_ref(p, policy, tl)
    got, nf, _ = engine.fit_order(policy)
    np.testing.assert_array_equal(nf, want_nf)
    np.testing.assert_array_equal(got, want)
