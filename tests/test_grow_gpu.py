"""jsp_place_grow on the GPU against the rule in int64 numpy (tests/grow_ref.py), exactly: the table (lists, nf, need,
plan records) in every form of the keys kernel, then assign, need, the plan pairs and every stats field."""
import dataclasses

import numpy as np
import pytest

from jobset_amd import native, synth
from jobset_amd.engine import Engine
from jobset_amd.snapshot import job_runs, shard_problem
from oracle import oracle as O
from grow_ref import CASES, NO_LIMIT, domain_table, grow_ref, stats_dict, table_ref

pytestmark = pytest.mark.gpu
_TABS = {}


def loaded(engine, case):
    p, t = CASES[case]()
    if case not in _TABS:
        _TABS[case] = domain_table(p, t)  # the reference once per case, never changed
    engine.load(p)
    return p, t, _TABS[case]


def checked(engine, p, t, tab, budget=NO_LIMIT):
    want = grow_ref(p, t, budget, tab)
    got = engine.place_grow(p.job_class, t, budget)
    for g, w in zip(got[:5], want[:5]):
        np.testing.assert_array_equal(g, w)
    assert stats_dict(got[5]) == want[5] and got[5].fused == 7 and got[5].runs == job_runs(p.job_class)[0].shape[0]
    return want


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_table_in_every_form(engine, monkeypatch, case, form):
    """form 0: the leaf form for the leaf-level class and, for the level-0 classes, what their largest domain asks for
    (grow_ref.SHAPES: the group form with 1, 8, 16 and 64 lanes per domain, the block form from 513 leaves); 1: the
    group form for the leaf-level class too; 2: every class in the block form."""
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    p, t, tab = loaded(engine, case)
    order, nf, need, rec = table_ref(p, t, tab)
    got = engine.grow_table(t, form)
    np.testing.assert_array_equal(got[2], need)
    np.testing.assert_array_equal(got[3], rec.reshape(-1, 4))
    np.testing.assert_array_equal(got[1], nf)
    np.testing.assert_array_equal(got[0], order)


@pytest.mark.parametrize("case", list(CASES))
def test_placement_budgets_and_reductions(engine, monkeypatch, case):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    p, t, tab = loaded(engine, case)
    free = checked(engine, p, t, tab)
    assert free[5]["grown"] > 0
    assert checked(engine, p, t, tab, free[5]["nodes"] // 2)[5]["over_budget"] > 0  # runs out mid-batch
    place = engine.place(p.job_class).assign
    np.testing.assert_array_equal(place, O.place_c(p)[0])
    np.testing.assert_array_equal(checked(engine, p, t, tab, 0)[0], place)
    fixed = dataclasses.replace(t, max_add=np.zeros_like(t.max_add))
    np.testing.assert_array_equal(checked(engine, p, fixed, domain_table(p, fixed))[0], place)
    rc, rl = job_runs(p.job_class)
    a, n, off, leaf, nodes, st = engine.place_grow_runs(rc, rl, t, want_plan=False)  # offsets and stats without the lists
    np.testing.assert_array_equal(off, free[2])
    assert leaf.shape == (0,) and stats_dict(st) == free[5]


@pytest.mark.parametrize("what", ["flags", "class", "leaves", "plan_cap", "jobs", "sharded"])
def test_refusals(engine, monkeypatch, what):
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    p, t, tab = loaded(engine, "wide")
    rc, rl = job_runs(p.job_class)
    target, kw, code, text = engine, {}, native.JSP_EINVAL, what
    if what == "flags":
        kw = dict(flags=1)
    elif what == "class":
        rc, text = rc + 4, "class 5"
    elif what == "leaves":
        t = dataclasses.replace(t, labels=t.labels[:, :3], taints=t.taints[:3], free=t.free[:, :3], max_add=t.max_add[:3])
    elif what == "plan_cap":
        kw, code, text = dict(plan_cap=1), native.JSP_ERANGE, "2 plan pairs"
    elif what == "jobs":
        rl, code = rl * 0 + 10000, native.JSP_ERANGE
    else:
        code = native.JSP_ESTATE
        q, target = synth.config5(), Engine(0)
        target.upload_topology(q.topology)
        target.upload_snapshot(shard_problem(q, 0, 2))
        target.upload_classes(q.classes)
        rc, rl = job_runs(q.job_class)
        t = synth.grow_templates(q, 1)
    with pytest.raises(native.JspError) as ei:
        target.place_grow_runs(rc, rl, t, **kw)
    assert ei.value.code == code and text in str(ei.value), str(ei.value)
    if what == "sharded":
        target.close()
    checked(engine, p, CASES["wide"]()[1], tab)  # the engine is usable afterwards


def test_nothing_moves(engine, monkeypatch):
    """Behind a placement the resident service answered: its answer, stats.fused and the metrics stay."""
    monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    engine.set_service(True)
    engine.set_fused(True)
    try:
        p = synth.config2()
        t = synth.grow_templates(p, 3)
        engine.load(p)
        for _ in range(4):
            if engine.place(p.job_class).fused == 3:
                break
        before = engine.place(p.job_class)
        assert before.fused == 3
        m0 = bytes(engine.metrics())
        got = engine.place_grow(p.job_class, t)
        want = grow_ref(p, t)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[4], want[4])
        assert stats_dict(got[5]) == want[5] and bytes(engine.metrics()) == m0
        after = engine.place(p.job_class)
        assert after.fused == before.fused
        np.testing.assert_array_equal(after.assign, before.assign)
    finally:
        engine.service_stop()
