"""jsp_place_fit without a GPU: the header declares it, the 32-byte struct and
the four defines, header / library / bindings agree, a NULL engine is
JSP_EINVAL and an engine without a GPU fails loudly; the tests' yardstick
(tests/fit_ref.py) reduces to the plain placement under JSP_FIT_LOWEST, holds
I1 / I2 under every policy and gives the hand cases' answers; the sweep's
inputs reach the coverage floors on the yardstick's own output, so no GPU
sweep is vacuous; and the host fit walk (jsp_walk.cc walk_fit), fed the
yardstick's candidate lists, gives the yardstick's answer."""
import ctypes
import os
import re

import numpy as np
import pytest

from jobset_amd import native
from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from fit_ref import (LOWEST, POLICIES, ROOMIEST, TIGHTEST, feasibility, fit_ref, fit_ref_literal, fits, fitv_ref,
                     hand_cases, order_ref, reduction_problem, sweep_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_jsp_place_fit():
    src = header("jsplace.h")
    assert re.search(r"^int\s+jsp_place_fit\s*\(\s*jsp_engine\s*\*\s*e\s*,\s*const\s+uint32_t\s*\*\s*run_class\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*run_len\s*,\s*uint32_t\s+n_runs\s*,\s*uint32_t\s+policy\s*,"
                     r"\s*uint32_t\s+flags\s*,\s*int32_t\s*\*\s*assign_out\s*,\s*jsp_fit_stats\s*\*\s*stats\s*\)\s*;",
                     src, flags=re.M)
    assert re.search(r"typedef\s+struct\s+jsp_fit_stats\s*\{\s*uint32_t\s+jobs\s*;\s*uint32_t\s+placed\s*;"
                     r"\s*uint32_t\s+runs\s*;\s*uint32_t\s+fused\s*;\s*uint64_t\s+slack\s*;\s*double\s+wall_us\s*;"
                     r"\s*\}\s*jsp_fit_stats\s*;", src)
    assert re.search(r"#define\s+JSP_FIT_LOWEST\s+0u", src)
    assert re.search(r"#define\s+JSP_FIT_TIGHTEST\s+1u", src)
    assert re.search(r"#define\s+JSP_FIT_ROOMIEST\s+2u", src)
    assert re.search(r"#define\s+JSP_FIT_MAX_JOBS\s+65536u", src)
    assert "#define JSP_ABI_VERSION 7" in src  # additive: a caller detects it by symbol
    bench = header("jsplace_bench.h")
    assert re.search(r"^int\s+jspb_place_fit_loop\s*\(", bench, flags=re.M)
    assert re.search(r"^int\s+jspb_fit_order\s*\(", bench, flags=re.M)


def test_struct_size_is_32():
    assert ctypes.sizeof(native.JspFitStats) == 32
    assert [f[0] for f in native.JspFitStats._fields_] == ["jobs", "placed", "runs", "fused", "slack", "wall_us"]
    assert native.JspFitStats.slack.offset == 16
    assert native.JspFitStats.wall_us.offset == 24
    assert (native.JSP_FIT_LOWEST, native.JSP_FIT_TIGHTEST, native.JSP_FIT_ROOMIEST) == (0, 1, 2)
    assert native.JSP_FIT_MAX_JOBS == 65536


def test_library_and_bindings_have_the_entry_points():
    lib = native.lib()
    bound = {n: (res, args) for n, res, args in native.SIGNATURES}
    for name, nargs in (("jsp_place_fit", 8), ("jspb_place_fit_loop", 8), ("jspb_fit_order", 8)):
        assert hasattr(lib, name), name
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs
    assert hasattr(lib, "jspi_fit_walk_test")
    assert lib.jsp_abi_version() == 7


def test_null_engine_is_einval():
    lib = native.lib()
    out = np.zeros(4, dtype=np.int32)
    st = native.JspFitStats()
    assert lib.jsp_place_fit(None, None, None, 0, 0, 0, out.ctypes.data, ctypes.byref(st)) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()
    us = np.zeros(3)
    assert lib.jspb_place_fit_loop(None, None, None, 0, 0, out.ctypes.data, 1, us.ctypes.data) == native.JSP_EINVAL
    assert lib.jspb_fit_order(None, 0, 0, None, 0, None, 0, None) == native.JSP_EINVAL


def test_no_gpu_fails_loudly():
    """No CPU fallback behind the new entry point either: without a GPU there
    is no engine to call it on."""
    if native.device_count() > 0:
        pytest.skip("a GPU is present")
    from jobset_amd.engine import Engine
    with pytest.raises(native.JspError) as ei:
        Engine(0).place_fit(np.zeros(1, dtype=np.uint32), native.JSP_FIT_TIGHTEST)
    assert ei.value.code == native.JSP_EHIP
    assert "no HIP device" in str(ei.value)


@pytest.mark.parametrize("i", range(60))
def test_reference_lowest_is_the_plain_placement(i):
    """JSP_FIT_LOWEST is the plain placement bit for bit; I1 / I2 and greedy
    maximality (oracle.check_invariants) on every policy's answer."""
    p = reduction_problem(i)
    plain, cap, occ = O.place_c(p)
    for policy in POLICIES:
        a, st = fit_ref_literal(p, policy, (cap, occ))
        if policy == LOWEST:
            np.testing.assert_array_equal(a, plain)
        O.check_invariants(p, a, cap, occ)
        assert st["jobs"] == p.n_jobs and st["placed"] == int((a >= 0).sum())
        fast, fast_st = fit_ref(p, policy, (cap, occ))   # the incremental form the large GPU cases use
        np.testing.assert_array_equal(fast, a)
        assert fast_st == st


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "D22"])
def test_reference_hand_cases(name):
    p, want = hand_cases()[name]
    plain, cap, occ = O.place_c(p)
    np.testing.assert_array_equal(plain, want[LOWEST])
    for policy in POLICIES:
        a, st = fit_ref_literal(p, policy, (cap, occ))
        np.testing.assert_array_equal(a, want[policy], err_msg=f"case {name} policy {policy}")
        O.check_invariants(p, a, cap, occ)
        fast, fast_st = fit_ref(p, policy, (cap, occ))
        np.testing.assert_array_equal(fast, a)
        assert fast_st == st


@pytest.mark.parametrize("name", ["D", "D22"])
def test_case_d_exercises_the_clamp(name):
    """D and its twin inside the engine's class contract have the same
    per-leaf tallies: capsums 3 * 2^31 and 5 * 2^31 clamp and tie."""
    p, _ = hand_cases()[name]
    cap = O.place_c(p)[1]
    np.testing.assert_array_equal(cap[0], [1 << 31] * 9)
    capsum = [int(cap[0, a:b].astype(np.int64).sum()) for a, b in ((0, 3), (3, 8), (8, 9))]
    assert capsum == [3 << 31, 5 << 31, 1 << 31]
    np.testing.assert_array_equal(fits(p, cap)[0], [0xFFFFFFFF, 0xFFFFFFFF, 1 << 31])


@pytest.fixture(scope="module")
def sweep():
    out = []
    for seed in range(60):
        p = sweep_case(seed)[0]
        plain, cap, occ = O.place_c(p)
        ans = {policy: fit_ref_literal(p, policy, (cap, occ)) for policy in POLICIES}
        for policy in POLICIES:
            fast, fast_st = fit_ref(p, policy, (cap, occ))
            np.testing.assert_array_equal(fast, ans[policy][0], err_msg=p.name)
            assert fast_st == ans[policy][1]
        out.append((p, plain, cap, occ, ans))
    return out


def test_sweep_answers_hold_the_invariants(sweep):
    for p, plain, cap, occ, ans in sweep:
        np.testing.assert_array_equal(ans[LOWEST][0], plain, err_msg=p.name)
        for policy in POLICIES:
            O.check_invariants(p, ans[policy][0], cap, occ)


def test_sweep_coverage_floors(sweep):
    """On the reference's own output over the 60 sweep inputs: the tightest
    and the roomiest answers differ from the plain one on >= 45 inputs each,
    the tightest rule places more jobs on >= 10 and fewer on >= 1 (both rules
    are greedy), and on >= 40 some class has two feasible domains of equal fit
    (the tie rule is exercised)."""
    t_diff = r_diff = more = fewer = ties = 0
    for p, plain, cap, occ, ans in sweep:
        t, r = ans[TIGHTEST][0], ans[ROOMIEST][0]
        t_diff += int(not np.array_equal(t, plain))
        r_diff += int(not np.array_equal(r, plain))
        more += int((t >= 0).sum() > (plain >= 0).sum())
        fewer += int((t >= 0).sum() < (plain >= 0).sum())
        tie = False
        for f, ok in zip(fits(p, cap), feasibility(p, cap, occ)):
            v = f[ok]
            tie |= np.unique(v).shape[0] < v.shape[0]
        ties += int(tie)
    print(f"tightest differs {t_diff}, roomiest differs {r_diff}, more {more}, fewer {fewer}, ties {ties}")
    assert t_diff >= 45 and r_diff >= 45
    assert more >= 10 and fewer >= 1
    assert ties >= 40


def _walk(p, order, nf, fitv, runs=None):
    lib = native.lib()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    fn = lib.jspi_fit_walk_test
    fn.restype = ctypes.c_int
    fn.argtypes = [u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
    topo = p.topology
    K = topo.n_levels
    D = (u32 * 4)(*([topo.n_domains[k] for k in range(K)] + [0] * (4 - K)))
    fls = [np.ascontiguousarray(topo.first_leaf[k], dtype=np.uint32) for k in range(K)]
    flp = (vp * 4)(*([f.ctypes.data for f in fls] + [None] * (4 - K)))
    lv = np.array([c.level for c in p.classes], dtype=np.uint32)
    pods = np.array([c.pods for c in p.classes], dtype=np.uint32)
    order = np.ascontiguousarray(np.concatenate([order, np.zeros(1, dtype=np.uint32)]))
    fitv = np.ascontiguousarray(np.concatenate([fitv, np.zeros(1, dtype=np.uint32)]))
    nf = np.ascontiguousarray(nf, dtype=np.uint32)
    rc, rl = job_runs(p.job_class) if runs is None else runs  # (another form of the same jobs: tests/run_forms.py)
    rc, rl = np.ascontiguousarray(rc, dtype=np.uint32), np.ascontiguousarray(rl, dtype=np.uint32)
    out = np.full(p.n_jobs + 1, -7, dtype=np.int32)           # one spare element, which must stay as it is
    slack = ctypes.c_uint64(0)
    placed = fn(K, D, flp, len(p.classes), lv.ctypes.data, pods.ctypes.data, order.ctypes.data, nf.ctypes.data,
                fitv.ctypes.data, rc.ctypes.data, rl.ctypes.data, len(rc), out.ctypes.data, ctypes.byref(slack))
    assert out[p.n_jobs] == -7, "the walk wrote behind assign[J)"
    return out[:p.n_jobs], placed, slack.value


def test_host_fit_walk_matches_the_reference(sweep):
    """The walk the engine runs on the host, on the reference's candidate
    lists: the reference's answer, placed count and slack."""
    for p, _, cap, occ, ans in sweep:
        fitv = fitv_ref(p, (cap, occ))
        for policy in POLICIES:
            order, nf = order_ref(p, policy, (cap, occ))
            out, placed, slack = _walk(p, order, nf, fitv)
            a, st = ans[policy]
            np.testing.assert_array_equal(out, a, err_msg=f"{p.name} policy {policy}")
            assert placed == st["placed"] and slack == st["slack"]


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "D22"])
def test_host_fit_walk_hand_cases(name):
    p, want = hand_cases()[name]
    _, cap, occ = O.place_c(p)
    for policy in POLICIES:
        order, nf = order_ref(p, policy, (cap, occ))
        out, placed, slack = _walk(p, order, nf, fitv_ref(p, (cap, occ)))
        np.testing.assert_array_equal(out, want[policy], err_msg=f"case {name} policy {policy}")
        assert slack == fit_ref(p, policy, (cap, occ))[1]["slack"]


def test_order_reference_layout(sweep):
    """order_ref: a segment per class, nf feasible ids in ascending (key, id),
    then 0xFFFFFFFF; LOWEST lists the feasible ids in ascending order."""
    for p, _, cap, occ, _ in sweep:
        feas = feasibility(p, cap, occ)
        order, nf = order_ref(p, LOWEST, (cap, occ))
        off = 0
        for c, f in enumerate(feas):
            seg = order[off:off + f.shape[0]]
            np.testing.assert_array_equal(seg[:nf[c]], np.nonzero(f)[0])
            assert np.all(seg[nf[c]:] == 0xFFFFFFFF) and nf[c] == int(f.sum())
            off += f.shape[0]
        assert off == order.shape[0]
