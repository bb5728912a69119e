"""CPU tests of the row predicate as include/jsplace.h states it (tests/
contract_ref.py): the reference against cpu_ref.c and the literal Python
loop, the optimized CPU evaluator against the reference, on the fixed contract
problems and on random problems with contradictory selectors; and the planner
producing such a selector from ordinary Kubernetes input."""
import numpy as np
import pytest

from jobset_amd import host, synth
from oracle import oracle as O

import contract_ref as CR
import k8s_fixtures as K

PROBLEMS = CR.contract_problems()
IDS = [p.name for p in PROBLEMS]


@pytest.fixture(scope="module")
def refs():
    return {p.name: CR.evaluate(p) for p in PROBLEMS}


def sweep_problem(seed):
    return CR.with_overlaps(synth.random_problem(seed), seed)


def assert_equal(ref, a, cap, occ):
    np.testing.assert_array_equal(occ, ref.occ)
    np.testing.assert_array_equal(cap, ref.cap)
    np.testing.assert_array_equal(a, ref.assign)


@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_reference_equals_cpu_ref_on_contract_problems(p, refs):
    assert_equal(refs[p.name], *O.place_c(p))
    a, cap, occ = O.place_py(p)
    assert_equal(refs[p.name], a, cap, occ)
    O.check_invariants(p, refs[p.name].assign, refs[p.name].cap, refs[p.name].occ)


@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_contract_problems_hold_what_they_claim(p, refs):
    """An overlap class passes no row although rows carry its required bits;
    its control (the same req, forbid = 0) has capacity and feasible domains,
    so a failure elsewhere points at the overlap and not at an empty snapshot."""
    r = refs[p.name]
    nd = p.nodes
    W, R = nd.n_label_words, nd.n_res
    assert len(CR.overlap_ids(p)) == 6
    for c in CR.overlap_ids(p):
        k = CR.control_of(p, c)
        assert not r.selector_ok[c].any() and r.cap[c].sum() == 0 and not r.feasible[c].any()
        assert r.selector_ok[k].any() and not r.selector_ok[k].all()
        assert r.cap[k].sum() > 0 and r.feasible[k].any()
        assert r.explain[c]["rows_selector"] == nd.n_nodes and r.explain[c]["dom_feasible"] == 0
    names = p.meta["class_names"]
    # taint bits 16 and 31 are on rows, and the three tolerations tell them apart
    assert (nd.taints & (1 << 16)).any() and (nd.taints & (1 << 31)).any()
    if "tolhi@1" in names:
        t31, thi, t0 = (r.taint_ok[names.index(f"{n}@1")].sum() for n in ("tol31", "tolhi", "tol0"))
        assert t0 < t31 < thi < nd.n_nodes
    # every excl_owner but -1 occupies its leaf
    for leaf, owner in CR.EXCL_LEAVES.items():
        assert nd.excl[nd.leaf_start[leaf]] == owner and r.occ[leaf] == 1
    assert r.occ.sum() == 3
    # divisor 1 at the edges of 32 bits: cap = min(free, 2^22)
    d = names.index("div1@1")
    r0 = int(nd.leaf_start[CR.DIV1_LEAF])
    np.testing.assert_array_equal(r.cap_row[d, r0:r0 + 6], [0, 1, (1 << 22) - 1, 1 << 22, 1 << 22, 1 << 22])
    if "past@1" in names and W < 4:
        x = p.classes[names.index("past@1")]
        assert any(x.req_labels[W:]) and any(x.forbid_labels[W:]) and any(x.req_res[R:])
        assert any(a & b for a, b in zip(x.req_labels[W:], x.forbid_labels[W:]))
        assert r.cap[names.index("past@1")].sum() > 0
    sizes = np.diff(nd.leaf_start.astype(np.int64))
    assert {0, 1, 3, 4, 5} <= set(sizes.tolist()) and sizes.max() > 256


@pytest.mark.parametrize("seed", CR.SWEEP_SEEDS)
def test_reference_equals_cpu_ref_on_overlap_sweep(seed):
    p = sweep_problem(seed)
    assert_equal(CR.evaluate(p), *O.place_c(p))


def test_overlap_sweep_is_not_vacuous():
    """In every sweep problem a class that had capacity got an overlap, and at
    least half of the classes that had capacity before the edit still have it."""
    assert len(CR.SWEEP_SEEDS) == 40 and len(set(CR.SWEEP_SEEDS)) == 40
    for seed in CR.SWEEP_SEEDS:
        p0 = synth.random_problem(seed)
        p1 = CR.with_overlaps(p0, seed)
        before = CR.evaluate(p0, walk=False).cap.astype(np.int64).sum(axis=1) > 0
        r1 = CR.evaluate(p1, walk=False)
        after = r1.cap.astype(np.int64).sum(axis=1) > 0
        edited = p1.meta["overlapped"]
        assert not after[edited].any(), seed
        assert before[edited].any(), seed
        assert 2 * int((before & after).sum()) >= int(before.sum()) > 0, seed
        for c in edited:
            rq, fb = p1.classes[c].words(4)
            assert any(a & b for a, b in zip(rq[:p1.nodes.n_label_words], fb[:p1.nodes.n_label_words]))
        assert synth.random_problem(seed).classes == p0.classes  # the generator's own classes are untouched


@pytest.fixture(scope="module")
def fast():
    f = O.FastCPU(threads=2)
    yield f
    f.close()


def run_fast(fast, p):
    fast.prepare(p)
    a, cap, occ, placed = fast.run(want_tally=True)
    assert placed == int((a >= 0).sum())
    return a, cap, occ


@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_fast_cpu_equals_reference_on_contract_problems(fast, p, refs):
    assert_equal(refs[p.name], *run_fast(fast, p))


@pytest.mark.parametrize("seed", CR.SWEEP_SEEDS)
def test_fast_cpu_equals_reference_on_overlap_sweep(fast, seed):
    p = sweep_problem(seed)
    assert_equal(CR.evaluate(p), *run_fast(fast, p))


def test_issue_example_four_rows():
    """4 one-row leaves, labels 0..3, req = 1 with forbid = 1 and with forbid = 3:
    no row passes either class."""
    from jobset_amd.snapshot import JobClass, Nodes, Problem, Topology
    topo = Topology(level_keys=["k"], n_domains=[4], first_leaf=[np.arange(5, dtype=np.uint32)])
    nodes = Nodes(leaf_start=np.arange(5, dtype=np.uint32), labels=np.arange(4, dtype=np.uint64)[None, :],
                  taints=np.zeros(4, dtype=np.uint32), free=np.ones((1, 4), dtype=np.uint32),
                  excl=np.full(4, -1, dtype=np.int32))
    p = Problem(topology=topo, nodes=nodes, classes=[JobClass(req_labels=(1,), forbid_labels=(1,)),
                                                     JobClass(req_labels=(1,), forbid_labels=(3,))],
                job_class=np.array([0, 1, 0, 1], dtype=np.uint32))
    r = CR.evaluate(p)
    assert (r.assign == -1).all() and r.cap.sum() == 0
    assert_equal(r, *O.place_c(p))
    f = O.FastCPU(threads=1)
    try:
        assert_equal(r, *run_fast(f, p))
    finally:
        f.close()


def test_planner_encodes_selector_and_notin_as_an_overlap():
    """nodeSelector {pool: a} plus matchExpressions pool NotIn [a] is ordinary
    input (kube-scheduler leaves such a pod Pending): the planner interns both
    as the same predicate, so the encoded class names one bit in reqLabels and
    in forbidLabels, and the contract gives its jobs no node."""
    c = host.Cache()
    for i, pool in enumerate(["a", "a", "b"]):
        c.add_node({"metadata": {"name": f"n{i}", "labels": {"rack": f"r{i}", "pool": pool}}, "spec": {},
                    "status": {"allocatable": {"cpu": "8"}}})
    c.planner_new(None, ["rack"], ["cpu"])
    notin = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [{
        "matchExpressions": [{"key": "pool", "operator": "NotIn", "values": ["a"]}]}]}}}

    def job(name, spec):
        return {"metadata": {"name": name, "namespace": "default", "labels": {K.RJOB: name},
                             "annotations": {K.EXCL: "rack"}},
                "spec": {"parallelism": 1, "template": {"spec": spec}}}
    enc = c.planner_encode([job("both", {"nodeSelector": {"pool": "a"}, "affinity": notin}),
                            job("sel", {"nodeSelector": {"pool": "a"}})])
    both, sel = enc["classes"][enc["jobClass"][0]], enc["classes"][enc["jobClass"][1]]
    req = [int(x, 16) for x in both["reqLabels"]]
    fb = [int(x, 16) for x in both["forbidLabels"]]
    assert any(req) and [a & b for a, b in zip(req, fb)] == req
    assert [int(x, 16) for x in sel["reqLabels"]] == req and not any(int(x, 16) for x in sel["forbidLabels"])
    q = K.problem_from_planner(synth.config1(), c.planner_columns(), enc)
    r = CR.evaluate(q)
    assert r.cap[enc["jobClass"][0]].sum() == 0 and r.assign[0] == -1
    np.testing.assert_array_equal(r.cap[enc["jobClass"][1]] > 0, [True, True, False])
    assert r.assign[1] == 0
    assert_equal(r, *O.place_c(q))
