"""The forms of a run list (tests/run_forms.py) without a GPU: the generator
keeps its promises on the sweeps' inputs, and the three host walks of
jsp_walk.cc -- the split service's walk (HostWalk::walk through
jspi_walk_test), the fit walk and the gang walk -- give the per-job
references' answers for every form of every job sequence: empty runs,
adjacent runs of one class, runs of one job, a gap of 2100 empty runs.
One spare element behind assign[J) stays untouched (the helpers assert it).

The sweeps are those of test_host_walk.py, test_fit.py and test_gang.py."""
import dataclasses

import numpy as np
import pytest

import run_forms as RF
from jobset_amd import synth
from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from fit_ref import POLICIES, fit_ref, fitv_ref, order_ref
from fit_ref import sweep_case as fit_sweep_case
from gang_ref import SWEEP_SEEDS, gang_ref, gang_runs_of
from gang_ref import sweep_case as gang_sweep_case
from test_fit import _walk as fit_walk
from test_gang import _walk as gang_walk
from test_host_walk import emulate_tiles, host_walk


def forms_of(p, seed=0):
    return RF.forms(p.job_class, len(p.classes), seed)


# ------------------------------------------------------------------ the generator
def check_generator(p, seed):
    jc = np.asarray(p.job_class, dtype=np.uint32)
    C = len(p.classes)
    fs = forms_of(p, seed)
    rc0, rl0 = job_runs(jc)
    n0 = rc0.shape[0]
    want = {"canonical", "ones", "split_rand", "split64", "split65", "padded", "padded_split", "gap"}
    want |= {"to32", "to33"} if n0 <= RF.LEVEL_MAX_RUNS else set()
    want |= {"empties_only"} if jc.shape[0] == 0 else set()
    assert set(fs) == want
    for name, (rc, rl, src) in fs.items():
        assert rc.dtype == rl.dtype == src.dtype == np.uint32 and rc.shape == rl.shape == src.shape, name
        np.testing.assert_array_equal(np.repeat(rc, rl), jc, err_msg=name)
        assert rc.size == 0 or int(rc.max()) < C, name
        # src: nondecreasing, and a real run carries its canonical run's class
        assert np.all(np.diff(src.astype(np.int64)) >= 0), name
        real = rl > 0
        np.testing.assert_array_equal(rc[real], rc0[src[real]], err_msg=name)
        # the real runs of each canonical run add up to it
        np.testing.assert_array_equal(np.bincount(src[real], weights=rl[real], minlength=n0)[:n0], rl0, err_msg=name)
    np.testing.assert_array_equal(fs["canonical"][0], rc0)
    np.testing.assert_array_equal(fs["canonical"][1], rl0)
    assert fs["ones"][0].shape[0] == jc.shape[0] and np.all(fs["ones"][1] == 1)
    for name in ("split_rand", "split64", "split65"):
        assert np.all(fs[name][1] >= 1), name
    assert jc.shape[0] == 0 or np.any(fs["split_rand"][1] == 1)
    for k, name in ((64, "split64"), (65, "split65")):
        assert int(fs[name][1].max(initial=0)) <= k
        if rl0.size and int(rl0.max()) >= k:
            assert np.any(fs[name][1] == k), name
    for name in ("padded", "padded_split"):
        rl = fs[name][1]
        assert rl[0] == 0 and rl[-1] == 0, name
        # at most 2 empty runs before a real run, at least one behind the last
        lead = [len(s) for s in "".join("0" if n == 0 else "1" for n in rl.tolist()).split("1")]
        assert max(lead[:-1], default=0) <= 2 and lead[-1] >= 1, name
    rl = fs["gap"][1]
    assert rl.shape[0] == n0 + RF.GAP
    assert RF.empty_tile(rl, RF.ASSIGN_TILE) >= 0
    assert sum(1 for k in range(rl.shape[0] // RF.FUSED_TILE)
               if not rl[RF.FUSED_TILE * k:RF.FUSED_TILE * (k + 1)].any()) >= 4
    if n0 >= 2:
        assert rl[n0 // 2] > 0 and rl[n0 // 2 + 1] == 0                  # after run n_runs // 2
        assert n0 < 3 or rl[-1] > 0                                      # inside the list
    if "to32" in fs:
        assert fs["to32"][0].shape[0] == 32 and fs["to33"][0].shape[0] == 33
    if "empties_only" in fs:
        assert fs["empties_only"][0].shape[0] == 3 and not fs["empties_only"][1].any()
    # deterministic
    again = forms_of(p, seed)
    for name in fs:
        for a, b in zip(fs[name], again[name]):
            np.testing.assert_array_equal(a, b, err_msg=name)
    return fs


@pytest.mark.parametrize("seed", range(20))
def test_generator_random(seed):
    check_generator(synth.random_problem(seed, max_nodes=3000, max_leaves=150), seed)


def test_generator_config5_and_the_edges():
    p = synth.config5()
    check_generator(p, 5)
    # runs of exactly 64 and 65 jobs, a batch without jobs, a batch of one job
    C = len(p.classes)
    for jc in ([0] * 64 + [1] * 65 + [0] * 130, [], [2], [1] * 129):
        fs = check_generator(_with_jobs(p, jc), 1)
        assert len(jc) > 0 or set(fs) >= {"empties_only", "to32", "to33"}
    assert C >= 2


def _with_jobs(p, jc):
    return dataclasses.replace(p, job_class=np.array(jc, dtype=np.uint32), job_names=None)


def test_regroup():
    jc = np.array([0, 0, 1, 1, 1, 0, 2, 2], dtype=np.uint32)       # canonical runs: 0 1 0 2
    gang_runs = np.array([1, 0, 2, 1], dtype=np.uint32)             # the second gang is empty
    for name, (rc, rl, src) in RF.forms(jc, 3, 4).items():
        gr = RF.regroup(gang_runs, src)
        assert gr.shape == (4,) and int(gr.sum()) == rc.shape[0], name
        assert gr[1] == 0, name                                     # no canonical run: no form run
        ends = [0] + np.cumsum(gr).tolist()
        jobs = [int(rl[a:b].sum()) for a, b in zip(ends[:-1], ends[1:])]
        assert jobs == [2, 0, 4, 2], name                           # each gang keeps its jobs
    np.testing.assert_array_equal(RF.regroup(gang_runs, np.arange(4)), gang_runs)
    assert RF.regroup([], []).shape == (0,)


# ------------------------------------------------------------------ HostWalk::walk
def check_walk(p, seed):
    a, cap, occ = O.place_c(p)
    slots, blocks, groups, cpg = emulate_tiles(p, cap, occ)
    for name, (rc, rl, _) in forms_of(p, seed).items():
        got, placed = host_walk(p, slots, blocks, groups, cpg, runs=(rc, rl))
        np.testing.assert_array_equal(got, a, err_msg=name)
        assert placed == int((a >= 0).sum()), name


@pytest.mark.parametrize("cfg", [1, 2, 3, 5])
def test_host_walk_configs(cfg):
    check_walk(synth.CONFIGS[cfg](), cfg)


@pytest.mark.parametrize("seed", range(40))
def test_host_walk_random(seed):
    check_walk(synth.random_problem(seed, max_nodes=3000, max_leaves=150), seed)


@pytest.mark.parametrize("seed", range(8))
def test_host_walk_deep_levels(seed):
    check_walk(synth.random_problem(5000 + seed, max_nodes=6000, max_levels=4, max_leaves=400, max_jobs=500), seed)


def test_host_walk_many_blocks():
    check_walk(synth.random_problem(77, max_nodes=40_000, max_levels=2, max_leaves=600), 77)


def test_host_walk_without_jobs():
    """n_runs == 0 and three empty runs: nothing placed, nothing written."""
    p = _with_jobs(synth.config5(), [])
    _, cap, occ = O.place_c(p)
    slots, blocks, groups, cpg = emulate_tiles(p, cap, occ)
    fs = forms_of(p)
    for name in ("canonical", "empties_only", "gap"):
        rc, rl, _ = fs[name]
        got, placed = host_walk(p, slots, blocks, groups, cpg, runs=(rc, rl))
        assert got.shape == (0,) and placed == 0, name


# ------------------------------------------------------------------ the fit walk
@pytest.mark.parametrize("seed", range(60))
def test_fit_walk(seed):
    p = fit_sweep_case(seed)[0]
    _, cap, occ = O.place_c(p)
    fitv = fitv_ref(p, (cap, occ))
    fs = forms_of(p, seed)
    for policy in POLICIES:
        order, nf = order_ref(p, policy, (cap, occ))
        a, st = fit_ref(p, policy, (cap, occ))
        for name, (rc, rl, _) in fs.items():
            out, placed, slack = fit_walk(p, order, nf, fitv, runs=(rc, rl))
            np.testing.assert_array_equal(out, a, err_msg=f"{p.name} policy {policy} {name}")
            assert placed == st["placed"] and slack == st["slack"], (p.name, policy, name)


# ------------------------------------------------------------------ the gang walk
@pytest.mark.parametrize("seed", list(SWEEP_SEEDS))
def test_gang_walk(seed):
    p, gj, gs = gang_sweep_case(seed)
    _, cap, occ = O.place_c(p)
    a, so = gang_ref(p, gj, gs, (cap, occ))
    rc0, rl0, gr0 = gang_runs_of(p.job_class, gj)
    # the forms of the gangs' own run list (runs never cross a gang boundary): cut from it, src into it
    fs = RF.forms_of_runs(rc0, rl0, len(p.classes), seed)
    for name, (rc, rl, src) in fs.items():
        gr = RF.regroup(gr0, src)
        assert int(gr.sum()) == rc.shape[0]
        for all_ones in (0, 1):
            out, sout, placed, gp = gang_walk(p, cap, occ, gj, gs, all_ones, runs=(rc, rl, gr))
            np.testing.assert_array_equal(out, a, err_msg=f"{p.name} {name}")
            np.testing.assert_array_equal(sout, so, err_msg=f"{p.name} {name}")
            assert placed == int((a >= 0).sum()) and gp == int((so >= 0).sum()), (p.name, name)
