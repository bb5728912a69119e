"""jsp_place_preempt on the GPU against the rule taken literally in numpy
(tests/preempt_ref.py; it never calls the engine). Every comparison is exact:
assign[] bit for bit, the victim offsets and the victim list entry for entry,
the stats field by field, the candidate lists, keys and seg word for word
(tests/test_preempt.py asserts the sweep's coverage floors on the reference's
own output). The order step's two forms are forced through the fit test
hooks, which the engine reads again at every snapshot upload: fit_form=1 the
rank form, fit_form=2 the block form, with fit_block=64 so that segments of 65
domains and more merge several blocks."""
import ctypes
import dataclasses

import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.native import JspPreemptStats
from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from bind_ref import cls, flat, nested
from preempt_ref import (BLOCKER, SWEEP_PRIOS, SWEEP_SEEDS, check_preempt, domain_table, hand_cases, order_ref, overlay,
                         preempt_ref, reduction_problem, row_codes, stats_dict, sweep)

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


def run(engine, p, prio, ids, rk, ef=None, load=True, tab=None):
    """Load p, place its jobs at prio, compare everything with the yardstick."""
    if load:
        engine.load(p)
    want = preempt_ref(p, prio, ids, rk, ef, tab=tab)
    a, off, v, st = engine.place_preempt(p.job_class, prio, ids, rk, ef)
    np.testing.assert_array_equal(a, want[0], err_msg=f"{p.name} prio {prio}")
    np.testing.assert_array_equal(off, want[1], err_msg=f"{p.name} prio {prio}")
    np.testing.assert_array_equal(v, want[2], err_msg=f"{p.name} prio {prio}")
    assert stats_dict(st) == want[3], (p.name, prio)
    return a, off, v, st


# ------------------------------------------------------------------ 1. the sweep, once per order form
@pytest.mark.parametrize("seed", list(SWEEP_SEEDS))
def test_sweep(engine, form, seed):
    p, ids, rk, ef = sweep(seed)
    engine.load(p)
    for prio in SWEEP_PRIOS:
        tab = domain_table(p, prio, ids, rk, ef)
        a, off, v, st = run(engine, p, prio, ids, rk, ef, load=False, tab=tab)
        check_preempt(p, prio, ids, rk, ef, a, off, v, tab=tab)
        # the same jobs as raw runs
        rc, rl = job_runs(p.job_class)
        a2, off2, v2, st2 = engine.place_preempt_runs(rc, rl, prio, ids, rk, ef)
        np.testing.assert_array_equal(a2, a)
        np.testing.assert_array_equal(off2, off)
        np.testing.assert_array_equal(v2, v)
        assert st2.runs == len(rc) and st2.fused == 7 and stats_dict(st2) == stats_dict(st)
    # without evict_free the resident free column stands on the victim rows too
    run(engine, p, 4, ids, rk, None, load=False)


# ------------------------------------------------------------------ 2. the reductions, on the engine's own jsp_place
@pytest.mark.parametrize("i", range(0, 60, 2))
def test_reductions_are_jsp_place(engine, own_choice, i):
    p = reduction_problem(i)
    engine.load(p)
    plain = engine.place(p.job_class).assign.copy()
    ids = np.unique(p.nodes.excl[p.nodes.excl != -1])
    ef = np.full_like(p.nodes.free, 0xFFFFFFFF)            # never read: no row is a victim
    for prio, ow, pr in ((9, [], []), (0, ids, np.zeros(ids.shape[0], dtype=np.uint32))):
        for e in (None, ef):
            a, off, v, st = engine.place_preempt(p.job_class, prio, ow, pr, e)
            np.testing.assert_array_equal(a, plain)
            assert not off.any() and v.shape[0] == 0
            assert (st.jobs, st.placed, st.preempting, st.victims) == (p.n_jobs, int((plain >= 0).sum()), 0, 0)


# ------------------------------------------------------------------ 3. the hand cases
@pytest.mark.parametrize("name", list(hand_cases()))
def test_hand_cases(engine, form, name):
    p, prio, ow, pr, ef, want, want_v = hand_cases()[name]
    a, off, v, st = run(engine, p, prio, ow, pr, ef)
    np.testing.assert_array_equal(a, want)
    assert [v[off[j]:off[j + 1]].tolist() for j in range(p.n_jobs)] == want_v
    if name == "zone-owner":
        assert st.victims == 2 and np.unique(v).shape[0] == 1


# ------------------------------------------------------------------ 4. the lists, keys and seg against numpy
def order_case(first_leaf, levels, rows=None, seed=1, pods=(1, 3), taint_p=0.4, held=True, extra=(), jobs=(), **ov):
    """test_fit_gpu's order cases (rows[l] rows per leaf, default 1 to 4 by the
    seed; a share of the rows tainted with bit 0; per level in `levels` one
    class per pods value, alternately tolerating nothing and bit 0; every 37th
    leaf's rows held by a job that is in no table) with preempt_ref.overlay's
    owners on top: (problem, owners, owner_prio, evict_free)."""
    L = len(first_leaf[-1]) - 1
    rows = synth.uniform_int(seed, 5, L, 1, 4) if rows is None else np.asarray(rows, dtype=np.int64)
    N = int(rows.sum())
    taints = synth.bernoulli(seed, 11, N, taint_p).astype(np.uint32)
    leaf_of = np.repeat(np.arange(L), rows)
    excl = np.where((leaf_of % 37 == 36) & held, 900, -1)
    classes = [cls(k, n, tol=i % 2) for k in levels for i, n in enumerate(pods)] + list(extra)
    p = nested(first_leaf, rows, classes, list(jobs), taints=taints, excl=excl)
    p.topology.validate()
    return overlay(p, seed, **ov)


def ident(n):
    return np.arange(n + 1)


def edges(n):
    """level-0 boundaries at and one off the 64-bit word boundaries below n"""
    return np.array(sorted({0, n} | {b for b in (1, 63, 64, 65, 127, 128, 129) if b < n}))


def chunks_case():
    """Domains of 1, 65 and 300 rows: the gather takes 1, 2 and 5 chunks of 64
    rows; in the last domain (rows 66..365) owners change at the chunk edges
    (rows 66 + 63, + 64, + 65, + 127, + 128, + 256) and free rows lie between."""
    p = flat([1, 65, 300], [cls(0, 1)], [0, 0, 0, 0])
    ex = np.full(366, -1, dtype=np.int32)
    ex[0] = 10
    ex[1:66] = 11
    r0 = 66
    cuts = [0, 63, 64, 65, 127, 128, 200, 256, 300]
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        ex[r0 + a:r0 + b] = -1 if i == 6 else 20 + i
    p.nodes.excl[:] = ex
    ids = np.array([10, 11] + [20 + i for i in range(8) if i != 6], dtype=np.int32)
    return p, ids, np.arange(ids.shape[0], dtype=np.uint32) % 3, None


ORDER_CASES = {
    # K = 1 around the word, the tile (256) and the block (64) boundaries
    **{f"K1-D{n}": lambda n=n: order_case([ident(n)], [0]) for n in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)},
    # a class with no reachable domain beside one that has some
    "K1-none-reachable": lambda: order_case([ident(130)], [0], extra=[cls(0, 1 << 20, tol=1)]),
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
                                   ident(1400)], [2, 1, 0], p_upper=0.02, p_leaf=0.05),
    # long leaves: several lanes of the leaf pass share one leaf
    "K1-long-leaves": lambda: order_case([ident(9)], [0], rows=[200, 1, 0, 130, 64, 65, 300, 2, 90], held=False),
    "chunks": chunks_case,
    # 4,200 racks of one row, each with its own owner: a table of 4,097 and more entries
    "K1-D4200": lambda: order_case([ident(4200)], [0], rows=[1] * 4200, pods=(1,), held=False, p_leaf=1.0, absent=0.0),
}


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_order_lists_match_numpy(engine, monkeypatch, name):
    monkeypatch.setenv("JSP_TEST_HOOKS", "fit_block=64")
    p, ids, rk, ef = ORDER_CASES[name]()
    engine.load(p)
    sizes = (4097, 0, 1, 2, ids.shape[0]) if name == "K1-D4200" else (ids.shape[0], 0, 1, 2)
    sizes = list(dict.fromkeys(min(n, ids.shape[0]) for n in sizes))   # the whole table first, then its prefixes
    some = 0
    for n_tab in sizes:
        for prio, e in ((4, ef), (2, None)):
            want = order_ref(p, prio, ids[:n_tab], rk[:n_tab], e)
            assert want[0].shape[0] == sum(p.topology.n_domains[jc.level] for jc in p.classes)
            some += int(want[1].sum())
            for f in ((1, 2, 0) if n_tab == sizes[0] else (0,)):
                got = engine.preempt_order(prio, ids[:n_tab], rk[:n_tab], e, form=f)
                for g, w, what in zip(got, want, ("order", "nf", "key", "seg")):
                    np.testing.assert_array_equal(g, w, err_msg=f"{name} table {n_tab} prio {prio} form {f}: {what}")
    assert some > 0  # the case is not empty
    if name == "K1-none-reachable":
        nf = order_ref(p, 4, ids, rk, ef)[1]
        assert nf[-1] == 0 and nf[0] > 0
    if name == "K1-D4200":
        assert ids.shape[0] >= 4097
    if name == "chunks":
        np.testing.assert_array_equal(order_ref(p, 4, ids, rk, ef)[3], [1, 1, 7])


def test_gather_over_several_chunks(engine, own_choice):
    """The victims of domains of 1, 65 and 300 rows, heads at the chunk edges."""
    p, ids, rk, ef = chunks_case()
    a, off, v, st = run(engine, p, 4, ids, rk, ef)
    assert sorted(a.tolist()) == [-1, 0, 1, 2] and st.victims == 9
    assert v[off[list(a).index(2)]:off[list(a).index(2) + 1]].tolist() == [20, 21, 22, 23, 24, 25, 27]


def test_preempt_order_refusals_and_timing(engine, own_choice):
    p, ids, rk, ef = ORDER_CASES["K3-long"]()
    engine.load(p)
    lib = native.lib()
    n = sum(p.topology.n_domains[jc.level] for jc in p.classes)
    order, key, seg = (np.zeros(n + 1, dtype=np.uint32) for _ in range(3))
    nf = np.zeros(len(p.classes), dtype=np.uint32)
    us = np.zeros(2)
    ow, pr = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(rk, dtype=np.uint32)
    o, k, s_, f = order.ctypes.data, key.ctypes.data, seg.ctypes.data, nf.ctypes.data
    tabargs = (ow.ctypes.data, pr.ctypes.data, ow.shape[0], None)
    for args in ((4, *tabargs, 3, o, n, f, k, s_, 0, us.ctypes.data),          # form
                 (65536, *tabargs, 0, o, n, f, k, s_, 0, us.ctypes.data),      # prio
                 (4, *tabargs, 0, o, n + 1, f, k, s_, 0, us.ctypes.data),      # n_order
                 (4, *tabargs, 0, None, n, f, k, s_, 0, us.ctypes.data),       # order_out
                 (4, *tabargs, 0, o, n, None, k, s_, 0, us.ctypes.data),       # nf_out
                 (4, *tabargs, 0, o, n, f, None, s_, 0, us.ctypes.data),       # key_out
                 (4, *tabargs, 0, o, n, f, k, None, 0, us.ctypes.data)):       # seg_out
        assert lib.jspb_preempt_order(engine._h, *args) == native.JSP_EINVAL
    for e in (None, ef):
        *_, (med, mean) = engine.preempt_order(4, ids, rk, e, iters=20)
        assert 0 < med < 1e4 and 0 < mean < 1e4


# ------------------------------------------------------------------ 5. victims_cap
def test_victims_cap(engine, own_choice):
    p, ids, rk, ef = sweep(3)
    engine.load(p)
    want = preempt_ref(p, 4, ids, rk, ef)
    total = want[3]["victims"]
    assert total >= 2
    rc, rl = job_runs(p.job_class)
    a, off, v, st = engine.place_preempt_runs(rc, rl, 4, ids, rk, ef, victims_cap=total)          # exact
    np.testing.assert_array_equal(v, want[2])
    with pytest.raises(native.JspError) as ei:
        engine.place_preempt_runs(rc, rl, 4, ids, rk, ef, victims_cap=total - 1)                  # one short
    assert ei.value.code == native.JSP_ERANGE and str(total) in str(ei.value)
    a, off, v, st = engine.place_preempt_runs(rc, rl, 4, ids, rk, ef, want_victims=False)         # no list wanted
    np.testing.assert_array_equal(a, want[0])
    np.testing.assert_array_equal(off, want[1])
    assert v.shape[0] == 0 and stats_dict(st) == want[3]
    a, off, v, st = engine.place_preempt_runs(rc, rl, 4, ids, rk, ef, victims_cap=0, want_victims=False)
    assert stats_dict(st) == want[3]
    run(engine, p, 4, ids, rk, ef, load=False)


# ------------------------------------------------------------------ 6. behind the service and a patch
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
        # two placed racks get owners: one in the table, one not
        base = O.place_c(p)[0]
        for r, owner in ((int(base[5]), 777), (int(base[6]), 778)):
            rows = rows_of(p, 0, r)
            engine.patch_rows(rows.astype(np.uint32), excl=np.full(rows.shape[0], owner, dtype=np.int32))
            p.nodes.excl[rows] = owner
        a, off, v, st = run(engine, p, 1, [777], [0], load=False)   # at once: behind the patches the dispatcher holds
        assert st.victims == 1 and v.tolist() == [777] and int(base[5]) in a.tolist() and int(base[6]) not in a.tolist()
        m1 = engine.metrics()                                        # not counted
        assert m1.place_us.count == m0.place_us.count and m1.batch_jobs.count == m0.batch_jobs.count
        assert m1.placed == m0.placed and m1.unplaceable == m0.unplaceable and m1.place_errors == m0.place_errors
        after = engine.place(p.job_class)                            # the service kept its tiles
        assert after.fused == 3
        np.testing.assert_array_equal(after.assign, O.place_c(p)[0])
        with pytest.raises(native.JspError):
            engine.place_preempt_runs([0], [990], 1, [777], [0], flags=1)
        assert engine.metrics().place_errors == m1.place_errors
        run(engine, p, 1, [777, 778], [0, 0], load=False)
    finally:
        engine.service_stop()


# ------------------------------------------------------------------ 7. the loop closed on the engine
def test_evict_patch_assume_forget(engine, form):
    p, ids, rk, ef = sweep(3)
    a, off, v, st = run(engine, p, 4, ids, rk, ef)
    assert st.preempting > 0
    code = row_codes(p.nodes.excl, 4, ids, rk)
    rows = []
    for j in np.nonzero(a >= 0)[0]:
        r = rows_of(p, p.classes[int(p.job_class[j])].level, int(a[j]))
        assert not (code[r] == BLOCKER).any()
        rows.append(r[code[r] != 0])
    rows = np.unique(np.concatenate(rows))
    assert set(np.unique(p.nodes.excl[rows]).tolist()) == set(np.unique(v).tolist())
    # the informer's view once the victims are gone
    engine.patch_rows(rows.astype(np.uint32), free=np.ascontiguousarray(ef[:, rows]),
                      excl=np.full(rows.shape[0], -1, dtype=np.int32))
    own = 0x40000000 + np.arange(p.n_jobs)
    committed, _ = engine.assume(p.job_class, a, own)
    assert committed.sum() == st.placed > 0
    engine.forget(own)


# ------------------------------------------------------------------ 8. refusals, each followed by a correct call
def refused(engine, code, word, *args, **kw):
    with pytest.raises(native.JspError) as ei:
        engine.place_preempt_runs(*args, **kw)
    assert ei.value.code == code, str(ei.value)
    assert word in str(ei.value), str(ei.value)


def test_refusals_leave_the_engine_usable(engine, own_choice):
    p, prio, ow, pr, ef, want, _ = hand_cases()["flat3"]
    engine.load(p)
    tab = domain_table(p, prio, ow, pr, ef)
    rc, rl = job_runs(p.job_class)
    lib = native.lib()
    one = np.ones(1, dtype=np.uint32)
    zero = np.zeros(1, dtype=np.uint32)
    out = np.zeros(4, dtype=np.int32)
    own = np.array([7], dtype=np.int32)

    def ok():
        np.testing.assert_array_equal(run(engine, p, prio, ow, pr, ef, load=False, tab=tab)[0], want)

    def raw(*args):
        return lib.jsp_place_preempt(engine._h, *args)

    refused(engine, native.JSP_EINVAL, "flags 1", rc, rl, prio, ow, pr, flags=1)
    ok()
    refused(engine, native.JSP_EINVAL, "run 1", [0, 1, 0], [1, 1, 1], prio, ow, pr)               # a class that does not exist
    ok()
    refused(engine, native.JSP_EINVAL, "prio 65536", rc, rl, 65536, ow, pr)
    ok()
    refused(engine, native.JSP_EINVAL, "table index 1", rc, rl, prio, ow, [0, 65535])             # a rank out of range
    ok()
    refused(engine, native.JSP_EINVAL, "table index 1", rc, rl, prio, [7, -1], pr)                # -1 names no owner
    ok()
    refused(engine, native.JSP_EINVAL, "table index 2", rc, rl, prio, [7, 9, 7], [0, 0, 1])       # the same id twice
    ok()
    refused(engine, native.JSP_ERANGE, "limit of 65536", [0], [native.JSP_PREEMPT_MAX_JOBS + 1], prio, ow, pr)
    ok()
    big = np.arange(100, 100 + native.JSP_PREEMPT_MAX_OWNERS + 1, dtype=np.int32)     # ids nobody holds
    refused(engine, native.JSP_ERANGE, "limit of 65536", rc, rl, prio, big, np.zeros(big.shape[0], dtype=np.uint32))
    ok()
    a, off, v, st = engine.place_preempt_runs(rc, rl, prio, big[:-1], np.zeros(big.shape[0] - 1, dtype=np.uint32))
    assert st.placed == 1                                                                          # 65536 owners, none held
    assert raw(zero.ctypes.data, one.ctypes.data, 1, 1, None, None, 0, None, 0, None, None, None, 0, None) == \
        native.JSP_EINVAL and b"NULL" in lib.jsp_last_error()                                      # assign_out
    ok()
    assert raw(None, one.ctypes.data, 1, 1, None, None, 0, None, 0, out.ctypes.data, None, None, 0, None) == \
        native.JSP_EINVAL and b"NULL" in lib.jsp_last_error()                                      # run_class
    ok()
    assert raw(zero.ctypes.data, one.ctypes.data, 1, 1, None, zero.ctypes.data, 1, None, 0, out.ctypes.data, None, None, 0,
               None) == native.JSP_EINVAL and b"NULL" in lib.jsp_last_error()                      # owner_ids
    assert raw(zero.ctypes.data, one.ctypes.data, 1, 1, own.ctypes.data, None, 1, None, 0, out.ctypes.data, None, None, 0,
               None) == native.JSP_EINVAL and b"NULL" in lib.jsp_last_error()                      # owner_prio
    ok()
    assert raw(zero.ctypes.data, one.ctypes.data, 1, 2, own.ctypes.data, one.ctypes.data, 1, None, 0, out.ctypes.data,
               None, None, 0, None) == native.JSP_OK                                               # every nullable NULL
    assert out[0] == 2
    a, off, v, st = engine.place_preempt_runs([], [], prio, ow, pr)                                # J == 0 launches nothing
    assert a.shape == (0,) and off.tolist() == [0] and v.shape == (0,)
    assert (st.jobs, st.placed, st.preempting, st.victims, st.runs, st.fused) == (0, 0, 0, 0, 0, 7)
    a, off, v, st = engine.place_preempt_runs([0, 0, 0], [1, 0, 1], prio, ow, pr)                  # an empty run is not counted
    np.testing.assert_array_equal(a, [2, 1])
    assert (st.jobs, st.placed, st.runs) == (2, 2, 2)


def test_device_set_sharded_and_unloaded_engines_are_estate():
    from jobset_amd.snapshot import shard_problem
    p = synth.config5()
    rc, rl = job_runs(p.job_class)
    with Engine(devices=[0, 0]) as multi:
        multi.load(p)
        refused(multi, native.JSP_ESTATE, "device-set", rc, rl, 1, [5], [0])
        with pytest.raises(native.JspError) as ei:
            multi.preempt_order(1, [5], [0])
        assert ei.value.code == native.JSP_ESTATE
    with Engine(0) as e:
        e.upload_topology(p.topology)
        e.upload_snapshot(shard_problem(p, 0, 2))
        e.upload_classes(p.classes)
        refused(e, native.JSP_ESTATE, "sharded", rc, rl, 1, [5], [0])
        with pytest.raises(native.JspError) as ei:
            e.preempt_order(1, [5], [0])
        assert ei.value.code == native.JSP_ESTATE
    lib = native.lib()
    with Engine(0) as e:
        a = np.zeros(1, dtype=np.int32)
        one, zero = np.ones(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        call = lambda: lib.jsp_place_preempt(e._h, zero.ctypes.data, one.ctypes.data, 1, 1, None, None, 0,  # noqa: E731
                                             None, 0, a.ctypes.data, None, None, 0, None)
        assert call() == native.JSP_ESTATE               # no topology yet
        e.upload_topology(p.topology)
        assert call() == native.JSP_ESTATE               # no snapshot yet
        e.upload_snapshot(p.nodes)
        assert call() == native.JSP_ESTATE               # no classes yet
        e.upload_classes(p.classes)
        assert call() == native.JSP_OK
        np.testing.assert_array_equal(a, O.place_c(dataclasses.replace(p, job_class=zero))[0])


def test_class_reupload_with_the_same_geometry(engine, own_choice):
    """The order step's rows and segments follow the classes: a second upload
    with the same class count and levels but other pods is ordered afresh."""
    jobs = [0, 2, 1, 3] * 6
    p, ids, rk, ef = order_case([edges(129), ident(129)], [1, 0], jobs=jobs)
    run(engine, p, 4, ids, rk, ef)
    q = dataclasses.replace(p, classes=[dataclasses.replace(jc, pods=jc.pods + 1) for jc in p.classes])
    engine.upload_classes(q.classes)
    run(engine, q, 4, ids, rk, ef, load=False)


# ------------------------------------------------------------------ 9. the real shapes
@pytest.mark.parametrize("cfg", [5, 2])
def test_configs_once(engine, own_choice, cfg):
    """30 % of the racks held by owners of a seeded overlay."""
    p, ids, rk, ef = overlay(synth.CONFIGS[cfg](), cfg, p_upper=0.0, p_leaf=0.3)
    a, off, v, st = run(engine, p, 4, ids, rk, ef)
    assert st.placed > 0 and ids.shape[0] > 200
    if cfg == 2:   # 990 jobs over 1,000 racks, 300 of them held: some jobs preempt (config5's 496 rack jobs find free racks)
        assert st.preempting > 0
    run(engine, p, 2, ids, rk, None, load=False)
    rc, rl = job_runs(p.job_class)
    total, med, p99 = engine.place_preempt_loop(rc, rl, 4, ids, rk, ef, iters=20)
    assert 0 < med <= p99 and total > 0
