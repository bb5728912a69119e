"""CPU checks of tests/dispatch_cases.py on the oracle alone: no case may pass
test_dispatch_gpu.py vacuously. For every case and side: jobs are placed and
jobs are left over; the highest placed domain of each level that placed a job
lies in that level's last 64-bit bitmap word; at least two classes differ in
feasibility; the one-row patch of the GPU test changes the oracle's answer;
the sides of a pair differ in the pair's dimension only; and the two CPU
evaluators agree."""
import functools

import numpy as np
import pytest

import dispatch_cases as DC
from oracle import oracle as O


@functools.lru_cache(maxsize=2)
def solved(dims):
    p = DC.build(dims)
    return (p,) + tuple(O.place_c(p))


@pytest.mark.parametrize("name,i", DC.sides())
def test_side_is_not_vacuous(name, i):
    p, a, cap, occ = solved(DC.case(name).sides[i].dims)
    topo = p.topology
    placed = a >= 0
    assert placed.any() and (~placed).any()
    lvl = np.array([p.classes[c].level for c in p.job_class])
    for k in set(lvl[placed].tolist()):
        assert int(a[placed & (lvl == k)].max()) // 64 == (topo.n_domains[k] - 1) // 64, f"level {k}"
    if len(p.classes) >= 2:
        feas = []
        for c, jc in enumerate(p.classes):
            fl = np.asarray(topo.first_leaf[jc.level], dtype=np.int64)
            cs = np.concatenate([[0], np.cumsum(cap[c].astype(np.int64))])
            os_ = np.concatenate([[0], np.cumsum(occ.astype(np.int64))])
            feas.append(((cs[fl[1:]] - cs[fl[:-1]] >= jc.pods) & (os_[fl[1:]] == os_[fl[:-1]])).tobytes())
        assert len(set(feas)) >= 2


@pytest.mark.parametrize("name,i", DC.sides())
def test_patch_changes_the_answer(name, i):
    """The GPU test's one-row patch is not vacuous: the oracle's answer moves."""
    p, a, cap, occ = solved(DC.case(name).sides[i].dims)
    row, q = DC.patched(p, a)
    assert p.nodes.excl[row] == -1 and q.nodes.excl[row] == DC.PATCH_OWNER
    assert not np.array_equal(O.place_c(q)[0], a)


@pytest.mark.parametrize("name,i", DC.sides())
def test_cpu_evaluators_agree(name, i):
    p, a, cap, occ = solved(DC.case(name).sides[i].dims)
    f = O.FastCPU(2)
    try:
        f.prepare(p)
        fa, fcap, focc, _ = f.run(want_tally=True)
        np.testing.assert_array_equal(fa, a)
        np.testing.assert_array_equal(fcap, cap)
        np.testing.assert_array_equal(focc, occ)
    finally:
        f.close()


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.name)
def test_pair_differs_in_its_dimension_only(case):
    assert len(case.sides) in (1, 2)
    if len(case.sides) == 2:
        assert DC.differing(case) == [case.dim]


def test_names_are_unique_and_axes_complete():
    names = [c.name for c in DC.CASES]
    assert len(set(names)) == len(names)
    assert {c.axis for c in DC.CASES} == set("ABCDEFG")


def test_taken_limit_cases_sit_at_the_limit():
    for name in ("G_flat", "G_three"):
        t = DC.topology(DC.case(name).sides[0].dims)
        assert sum((d + 63) // 64 for d in t.n_domains) == DC.MAX_TAKEN_WORDS
    over = DC.topology(DC.G_OVER)
    over.validate()
    assert sum((d + 63) // 64 for d in over.n_domains) == DC.MAX_TAKEN_WORDS + 1
