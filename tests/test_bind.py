"""jsp_bind_pods without a GPU: the header declares it with its signature, the
ctypes struct has the ABI's size, JSP_ABI_VERSION is still 7, a NULL engine is
JSP_EINVAL, and the tests' yardstick (tests/bind_ref.py) gives the hand-computed
answers of the small cases and agrees with the CPU oracle's per-leaf sums."""
import ctypes
import os
import re

import numpy as np
import pytest

from jobset_amd import native, synth
from oracle import oracle as O
from bind_ref import BindConflict, bind_ref, case1, case2, case3, check_bind, cls, leaf_sums, nested

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_jsp_bind_pods():
    src = header("jsplace.h")
    assert re.search(r"^int\s+jsp_bind_pods\s*\(\s*jsp_engine\s*\*\s*e\s*,\s*const\s+uint32_t\s*\*\s*run_class\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*run_len\s*,\s*uint32_t\s+n_runs\s*,\s*const\s+int32_t\s*\*\s*assign"
                     r"\s*,\s*uint32_t\s+flags\s*,\s*int32_t\s*\*\s*pod_row_out\s*,\s*uint64_t\s*\*\s*pod_off_out\s*,"
                     r"\s*jsp_bind_stats\s*\*\s*stats\s*\)\s*;", src, flags=re.M)
    assert "typedef struct jsp_bind_stats" in src
    assert "#define JSP_ABI_VERSION 7" in src  # additive: a caller detects it by symbol
    m = re.search(r"^#define\s+JSP_BIND_MAX_PODS\s+\(1u\s*<<\s*(\d+)\)", src, flags=re.M)
    assert m and (1 << int(m.group(1))) == native.JSP_BIND_MAX_PODS >= 1 << 24
    assert re.search(r"^int\s+jspb_bind_loop\s*\(", header("jsplace_bench.h"), flags=re.M)


def test_struct_size_is_40():
    assert ctypes.sizeof(native.JspBindStats) == 40
    assert [f[0] for f in native.JspBindStats._fields_] == ["jobs", "bound", "stale", "rows_used", "pods",
                                                            "pods_bound", "wall_us"]
    assert native.JspBindStats.pods.offset == 16
    assert native.JspBindStats.wall_us.offset == 32


def test_library_and_bindings_have_the_entry_points():
    lib = native.lib()
    bound = {n: (res, args) for n, res, args in native.SIGNATURES}
    for name, nargs in (("jsp_bind_pods", 9), ("jspb_bind_loop", 9)):
        assert hasattr(lib, name), name
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs
    assert lib.jsp_abi_version() == 7


def test_null_engine_is_einval():
    lib = native.lib()
    out = np.zeros(4, dtype=np.int32)
    st = native.JspBindStats()
    assert lib.jsp_bind_pods(None, None, None, 0, None, 0, out.ctypes.data, None, ctypes.byref(st)) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()
    us = np.zeros(3)
    assert lib.jspb_bind_loop(None, None, None, 0, None, out.ctypes.data, None, 1, us.ctypes.data) == native.JSP_EINVAL


# ------------------------------------------------------------------ the yardstick on hand-computed cases
def test_ref_case1_job_order_is_not_domain_order():
    p, assign = case1()
    rows, off, st = bind_ref(p, assign)
    np.testing.assert_array_equal(rows, [4, 5, -1, -1, 0, 1])
    np.testing.assert_array_equal(off, [0, 2, 4, 6])
    assert st == dict(jobs=3, bound=2, stale=0, rows_used=4, pods=6, pods_bound=4)
    assert check_bind(p, assign, rows, off) == (2, 4)


def test_ref_case2_uneven_caps_and_the_clamp():
    p, assign = case2(pods=5, free=3)
    rows, _, st = bind_ref(p, assign)
    np.testing.assert_array_equal(rows, [0, 0, 0, 2, 2])
    assert (st["bound"], st["rows_used"]) == (1, 2)
    p, assign = case2(pods=2, free=5)
    rows, _, st = bind_ref(p, assign)
    np.testing.assert_array_equal(rows, [0, 0])  # cap is clamped to pods: both on row 0
    assert (st["bound"], st["rows_used"]) == (1, 1)
    p, assign = case2(pods=7, free=3)           # one pod short: stale
    rows, _, st = bind_ref(p, assign)
    assert (rows == -1).all() and (st["bound"], st["stale"], st["pods_bound"]) == (0, 1, 0)


def test_ref_case3_requests_nothing():
    p, assign = case3()
    rows, _, st = bind_ref(p, assign)
    assert rows.shape == (4096,) and (rows == 1).all()  # row 0 is tainted
    assert (st["bound"], st["rows_used"], st["pods_bound"]) == (1, 1, 4096)


def test_ref_conflicts_name_the_lowest_later_job():
    fl = [np.array([0, 4, 8]), np.array([0, 2, 4, 6, 8]), np.arange(9)]
    classes = [cls(0, 4), cls(1, 2), cls(2, 1)]
    for job_class, assign, bad in (([1, 1, 1], [2, 0, 2], 2), ([0, 2, 1], [1, 0, 3], 2), ([1, 2, 0], [3, 0, 1], 2),
                                   ([2, 0, 1, 1], [0, 1, 1, 2], 3)):
        p = nested(fl, [1] * 8, classes, job_class)
        with pytest.raises(BindConflict) as ei:
            bind_ref(p, np.array(assign))
        assert ei.value.job == bad
    p = nested(fl, [1] * 8, classes, [0, 1, 2])
    rows, _, st = bind_ref(p, np.array([1, 0, 3]))  # zone 1, rack 0, leaf 3: disjoint
    np.testing.assert_array_equal(rows, [4, 5, 6, 7, 0, 1, 3])
    with pytest.raises(ValueError):
        bind_ref(p, np.array([2, 0, 3]))


# ------------------------------------------------------------------ the yardstick against the CPU oracle
@pytest.mark.parametrize("seed", range(60))
def test_ref_sums_equal_the_oracle(seed):
    p = synth.random_problem(seed)
    assign, cap_c, occ_c = O.place_c(p)
    cap, occ = leaf_sums(p)
    np.testing.assert_array_equal(cap, cap_c)
    np.testing.assert_array_equal(occ, occ_c)
    rows, off, st = bind_ref(p, assign)  # the oracle's placement: disjoint, and every placed job is bound
    assert check_bind(p, assign, rows, off) == (st["bound"], st["pods_bound"])
    assert st["bound"] == int((assign >= 0).sum()) and st["stale"] == 0
