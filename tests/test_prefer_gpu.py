"""jsp_place_prefer on the GPU against the rule in numpy (tests/prefer_ref.py;
it never calls the engine). Every comparison is exact: the sc table, the
candidate lists with their tails, nf, assign[], score_out and the stats."""
import dataclasses

import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import job_runs, shard_problem
from oracle import oracle as O
from bind_ref import cls, flat
from gang_ref import reduction_problem
from prefer_ref import SWEEP, order_ref, prefer_ref, problem, row_weights, seeded_terms, sweep

pytestmark = pytest.mark.gpu

# the order step's forms: forced rank, forced block (blocks of 64 keys), the engine's own choice by size
FORMS = {"rank": "fit_form=1", "block": "fit_form=2,fit_block=64", "own": ""}
EDGE_ROWS = [1, 3, 4, 5, 0, 64, 65, 255, 256, 257]
# one class, 8 terms: weights 1 and 100, an empty term, a term matching nothing (bit 60 is never set), a bit in both masks
EIGHT = [(0, 1, (1,), (0,)), (0, 100, (2,), (0,)), (0, 1, (0,), (0,)), (0, 100, (1 << 60,), (0,)), (0, 100, (4,), (4,)),
         (0, 100, (0,), (8,)), (0, 1, (3,), (4,)), (0, 100, (8,), (1,))]


ident = lambda n: np.arange(n + 1)  # noqa: E731

TABLE_CASES = {
    # pods below the first row's cap, inside the leaves, above every capsum (infeasible: sc must still match)
    "edges": lambda: (problem([ident(10)], EDGE_ROWS, [cls(0, n, tol=n % 2) for n in (1, 2, 7, 40, 300, 5000)]),
                      EIGHT + [(c, 10 * c, (1 << (c % 4),), (0,)) for c in range(1, 6)]),
    "edges-no-terms": lambda: (problem([ident(10)], EDGE_ROWS, [cls(0, 7), cls(0, 40)]), []),
    # the leaf carry crosses chunks; the upper class's base crosses the long leaves
    "long": lambda: (problem([[0, 2, 5], ident(5)], [1030, 2050, 7, 0, 3],
                             [cls(k, n, tol=1) for k in (1, 0) for n in (1, 900, 4000, 20000)], seed=2),
                     [(c, 1 + 12 * c, (1 << (c % 4),), (2,)) for c in range(8)]),
    # upper domains of 2, 64, 65 and 129 leaves, childless domains, one level-0 domain of 300 leaves (two row blocks)
    "K4": lambda: (problem([[0, 300], [0, 2, 131, 131, 300], [0, 2, 66, 131, 260, 260, 300], ident(300)],
                           np.random.default_rng(7).integers(1, 5, 300),
                           [cls(k, n, tol=k % 2) for k in range(4) for n in (1, 5, 12 * (4 - k))], seed=4),
                   seeded_terms(12, 4)),
    # terms for 17 classes in one upload (two passes), every term's bit in word W - 1
    "17-classes": lambda: (problem([[0, 3, 9], ident(9)], [3, 0, 5, 2, 7, 1, 4, 4, 6],
                                   [cls(c % 2, 1 + c, tol=1) for c in range(17)], W=2),
                           [(c, 1 + 5 * c, (0, 1 << (c % 4)), (0, 0)) for c in range(17)]),
}


def check_tables(engine, p, terms):
    engine.load(p)
    order, nf, sc = order_ref(p, terms, O.place_c(p)[1:])
    for f in (1, 2, 0):
        got, got_nf, got_sc, _ = engine.prefer_order(terms, form=f)
        for a, b in ((got_sc, sc), (got_nf, nf), (got, order)):
            np.testing.assert_array_equal(a, b, err_msg=f"form {f}")
    return nf, sc


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_tables_match_numpy(engine, monkeypatch, name):
    monkeypatch.setenv("JSP_TEST_HOOKS", "fit_block=64")
    p, terms = TABLE_CASES[name]()
    nf, sc = check_tables(engine, p, terms)
    assert nf.sum() > 0 and (sc.any() or not terms)
    if name == "edges":
        assert nf[-1] == 0 and sc[-10:].any()      # 5000 pods fit nowhere, and still score


@pytest.mark.parametrize("W,R", [(w, r) for w in (1, 2, 3, 4) for r in (1, 2, 3, 4)])
def test_every_instantiated_pair(engine, monkeypatch, W, R):
    monkeypatch.setenv("JSP_TEST_HOOKS", "fit_block=64")
    classes = [dataclasses.replace(cls(k, 3 + k, tol=k), req_res=(1,) * R) for k in (0, 1)]
    p = problem([[0, 2, 5], ident(5)], [3, 4, 5, 1, 2], classes, W=W, R=R, seed=W * 8 + R)
    word = (0,) * (W - 1)
    assert check_tables(engine, p, [(0, 7, word + (1,), word + (2,)), (1, 100, word + (4,), ()), (1, 3, (1,), ())])[1].any()


def run(engine, p, terms, load=True):
    if load:
        engine.load(p)
    want, want_sc, want_st = prefer_ref(p, terms)
    got, got_sc, st = engine.place_prefer(p.job_class, terms)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_sc, want_sc)
    assert {k: int(getattr(st, k)) for k in want_st} == want_st
    return got, got_sc


@pytest.mark.parametrize("form", list(FORMS))
def test_hand_positions(engine, monkeypatch, form):
    """Two racks of 3 rows, free = [3, 2, 4 | 1, 1, 4], weight 10 on rows 1, 2 and 5. 2 pods stay on the first
    row (sc 0 | 0), 5 end at a row's end in rack 0 (20 | 30), 6 end inside its last row (30 | 40), 10 fit nowhere
    (60 | 40). The 5-pod job takes rack 1 for its score, not the lowest id."""
    monkeypatch.setenv("JSP_TEST_HOOKS", FORMS[form])
    p = flat([3, 3], [cls(0, n) for n in (2, 5, 6, 10)], [1, 0, 2, 3], free=[3, 2, 4, 1, 1, 4])
    p.nodes.labels[0] = np.array([1, 3, 3, 1, 1, 3], dtype=np.uint64)
    terms = [(c, 10, (2,), ()) for c in range(4)]
    got, got_sc = run(engine, p, terms)
    np.testing.assert_array_equal(got, [1, 0, -1, -1])
    np.testing.assert_array_equal(got_sc, [30, 0, 0, 0])
    np.testing.assert_array_equal(engine.prefer_order(terms)[2], [0, 0, 20, 30, 30, 40, 60, 40])


def test_sweep_inputs_cover_the_rule():
    """On the yardstick's own output: half of the seeds differ from jsp_place, and some job stays unplaced."""
    want = [(prefer_ref(p, terms)[0], O.place_c(p)[0]) for p, terms in map(sweep, SWEEP)]
    assert 2 * sum(not np.array_equal(a, b) for a, b in want) >= len(SWEEP) and any((a < 0).any() for a, _ in want)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("seed", SWEEP)
def test_sweep(engine, monkeypatch, form, seed):
    monkeypatch.setenv("JSP_TEST_HOOKS", FORMS[form])
    p, terms = sweep(seed)
    got, got_sc = run(engine, p, terms)
    # jsp_bind_pods puts a placed job's pods on rows whose weights sum to its score
    pod_row, pod_off, _ = engine.bind_pods(p.job_class, got)
    for j in np.nonzero(got >= 0)[0]:
        w = row_weights(p, terms, int(p.job_class[j]))
        assert int(w[pod_row[int(pod_off[j]):int(pod_off[j + 1])]].sum()) == int(got_sc[j]), j


@pytest.mark.parametrize("i", range(0, 60, 6))
def test_reductions_are_jsp_place(engine, monkeypatch, i):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    p = reduction_problem(i)
    engine.load(p)
    plain = engine.place(p.job_class).assign.copy()
    every_row = [(c, 1 + c % 100, (), ()) for c in range(len(p.classes)) for _ in range(2)]
    for terms in ([], every_row):
        got, sc, st = engine.place_prefer(p.job_class, terms)
        np.testing.assert_array_equal(got, plain)
        assert st.placed == int((plain >= 0).sum()) and (terms or not sc.any())


def refused(engine, code, word, *args, **kw):
    with pytest.raises(native.JspError) as ei:
        engine.place_prefer_runs(*args, **kw)
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def test_refusals_leave_the_engine_usable(engine, monkeypatch):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    p, terms = sweep(1)
    engine.load(p)
    rc, rl = job_runs(p.job_class)
    C = len(p.classes)
    lib, zero, one, out = native.lib(), np.zeros(1, np.uint32), np.ones(1, np.uint32), np.zeros(4, np.int32)
    cases = [(native.JSP_EINVAL, "flags 1", (rc, rl, terms), dict(flags=1)),
             (native.JSP_EINVAL, "run 1", ([0, C, 0], [1, 1, 1], terms), {}),
             (native.JSP_EINVAL, "term 2", (rc, rl, terms[:2] + [(C, 5, (), ())]), {}),
             (native.JSP_EINVAL, "term 0", (rc, rl, [(0, 0, (), ())]), {}),
             (native.JSP_EINVAL, "term 1", (rc, rl, [(0, 100, (), ()), (0, 101, (), ())]), {}),
             (native.JSP_ERANGE, "limit of 65536", ([0], [native.JSP_PREFER_MAX_JOBS + 1], terms), {}),
             (native.JSP_ERANGE, "limit of 8", (rc, rl, [(C - 1, 1, (), ())] * 9), {})]
    for code, word, args, kw in cases:
        refused(engine, code, word, *args, **kw)
        run(engine, p, terms, load=False)
    for args in ((zero.ctypes.data, one.ctypes.data, 1, None, 0, 0, None, None, None),               # assign_out
                 (None, one.ctypes.data, 1, None, 0, 0, out.ctypes.data, None, None),                # run_class
                 (zero.ctypes.data, one.ctypes.data, 1, None, 1, 0, out.ctypes.data, None, None)):   # terms
        assert lib.jsp_place_prefer(engine._h, *args) == native.JSP_EINVAL and b"NULL" in lib.jsp_last_error()
        run(engine, p, terms, load=False)
    got, sc, st = engine.place_prefer_runs([], [], terms)                                            # nothing launched
    assert got.shape == (0,) and (st.jobs, st.placed, st.runs, st.fused, st.score) == (0, 0, 0, 7, 0)


def test_device_set_sharded_and_unloaded_engines_are_estate():
    p = synth.config5()
    rc, rl = job_runs(p.job_class)
    with Engine(devices=[0, 0]) as multi:
        multi.load(p)
        refused(multi, native.JSP_ESTATE, "device-set", rc, rl)
    with Engine(0) as e:
        refused(e, native.JSP_ESTATE, "no topology", rc, rl)
        e.upload_topology(p.topology)
        e.upload_snapshot(shard_problem(p, 0, 2))
        e.upload_classes(p.classes)
        refused(e, native.JSP_ESTATE, "sharded", rc, rl)


def test_behind_the_service_and_a_patch(engine, monkeypatch):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    engine.set_service(True)
    engine.set_fused(True)
    try:
        p = synth.config2()
        terms = synth.prefer_racks(p, 3)
        engine.load(p)
        for _ in range(5):
            if engine.place(p.job_class).fused == 3:
                break
        assert engine.place(p.job_class).fused == 3
        m0 = engine.metrics()
        row = int(np.nonzero(p.nodes.labels[0] >> np.uint64(62) == 0)[0][0])   # one more row gets the label, at once
        p.nodes.labels[0, row] |= np.uint64(1 << 62)
        engine.patch_rows(np.array([row], dtype=np.uint32), labels=p.nodes.labels[:, row].copy())
        got, _ = run(engine, p, terms, load=False)
        m1 = engine.metrics()
        assert m1.place_us.count == m0.place_us.count + 1 and m1.batch_jobs.count == m0.batch_jobs.count + 1
        assert m1.placed == m0.placed + int((got >= 0).sum()) and m1.unplaceable == m0.unplaceable + int((got < 0).sum())
        after = engine.place(p.job_class)                                       # the service kept its tiles
        assert after.fused == 3
        np.testing.assert_array_equal(after.assign, O.place_c(p)[0])
        refused(engine, native.JSP_EINVAL, "flags", *job_runs(p.job_class), terms, flags=2)
        assert engine.metrics().place_errors == m1.place_errors + 1
    finally:
        engine.service_stop()


@pytest.mark.parametrize("cfg", [2, 5])
def test_configs_once(engine, monkeypatch, cfg):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    p = synth.CONFIGS[cfg]()
    terms = synth.prefer_racks(p, cfg)
    got, sc = run(engine, p, terms)
    assert (got >= 0).any() and sc.any()
    total, med, p99 = engine.place_prefer_loop(*job_runs(p.job_class), terms, iters=20)
    assert 0 < med <= p99 and total > 0
