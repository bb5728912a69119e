"""jsp_assume / jsp_forget without a GPU: the header declares both with their
signatures, the ctypes struct has the ABI's size, JSP_ABI_VERSION is still 7, a
NULL engine is JSP_EINVAL, and the tests' yardstick (tests/assume_ref.py) does
what the feature is for: on its snapshot the CPU oracle never hands a second
batch a domain that intersects a committed one, and forgetting every owner
restores the column."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

from jobset_amd import native, synth
from oracle import oracle as O
from assume_ref import BindConflict, assume_ref, domains_intersect, forget_ref, with_excl
from bind_ref import cls, flat, nested

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_both_entry_points():
    src = header("jsplace.h")
    assert re.search(r"^int\s+jsp_assume\s*\(\s*jsp_engine\s*\*\s*e\s*,\s*const\s+uint32_t\s*\*\s*run_class\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*run_len\s*,\s*uint32_t\s+n_runs\s*,\s*const\s+int32_t\s*\*\s*assign"
                     r"\s*,\s*const\s+int32_t\s*\*\s*owner\s*,\s*uint32_t\s+flags\s*,\s*uint8_t\s*\*\s*committed_out\s*,"
                     r"\s*jsp_assume_stats\s*\*\s*stats\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^int\s+jsp_forget\s*\(\s*jsp_engine\s*\*\s*e\s*,\s*const\s+int32_t\s*\*\s*owners\s*,"
                     r"\s*uint32_t\s+n_owners\s*,\s*uint64_t\s*\*\s*rows_cleared_out\s*\)\s*;", src, flags=re.M)
    assert "typedef struct jsp_assume_stats" in src
    assert "#define JSP_ABI_VERSION 7" in src  # additive: a caller detects them by symbol
    m = re.search(r"^#define\s+JSP_FORGET_MAX_OWNERS\s+(\d+)u", src, flags=re.M)
    assert m and int(m.group(1)) == native.JSP_FORGET_MAX_OWNERS == 65536
    assert re.search(r"^int\s+jspb_assume_forget_loop\s*\(", header("jsplace_bench.h"), flags=re.M)


def test_struct_size_is_32():
    assert ctypes.sizeof(native.JspAssumeStats) == 32
    assert [f[0] for f in native.JspAssumeStats._fields_] == ["jobs", "committed", "stale", "reserved", "rows_marked",
                                                              "wall_us"]
    assert native.JspAssumeStats.rows_marked.offset == 16
    assert native.JspAssumeStats.wall_us.offset == 24


def test_library_and_bindings_have_the_entry_points():
    lib = native.lib()
    bound = {n: (res, args) for n, res, args in native.SIGNATURES}
    for name, nargs in (("jsp_assume", 9), ("jsp_forget", 4), ("jspb_assume_forget_loop", 10)):
        assert hasattr(lib, name), name
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs
    assert lib.jsp_abi_version() == 7


def test_null_engine_is_einval():
    lib = native.lib()
    a = np.zeros(4, dtype=np.int32)
    st = native.JspAssumeStats()
    assert lib.jsp_assume(None, None, None, 0, a.ctypes.data, a.ctypes.data, 0, None,
                          ctypes.byref(st)) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()
    n = ctypes.c_uint64(7)
    assert lib.jsp_forget(None, a.ctypes.data, 1, ctypes.byref(n)) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()
    us = np.zeros(4)
    assert lib.jspb_assume_forget_loop(None, None, None, 0, None, None, 1, None, None,
                                       us.ctypes.data) == native.JSP_EINVAL


# ------------------------------------------------------------------ the yardstick on hand-computed cases
def test_ref_hand_case():
    p = flat([2, 2, 2], [cls(0, 2)], [0, 0, 0])
    new, committed, st = assume_ref(p, [1, 0, -1], [7, 9, 5])
    np.testing.assert_array_equal(new, [9, 9, 7, 7, -1, -1])
    np.testing.assert_array_equal(committed, [True, True, False])
    assert st == dict(jobs=3, committed=2, stale=0, reserved=0, rows_marked=4)
    np.testing.assert_array_equal(p.nodes.excl, [-1] * 6)                      # the input is left as it is
    back, cleared = forget_ref(new, [9])
    np.testing.assert_array_equal(back, [-1, -1, 7, 7, -1, -1])
    assert cleared == 2
    assert forget_ref(new, [5])[1] == 0
    assert forget_ref(new, [9, 7, 9])[1] == 4


def test_ref_stale_and_refusals():
    excl = [-1, -1, -1, 7, -1, -1]     # leaf 1 holds a row of another exclusive job
    taints = [0, 0, 0, 0, 0, 1]        # leaf 2 is one pod short
    p = flat([2, 2, 2], [cls(0, 2)], [0, 0, 0], taints=taints, excl=excl)
    new, committed, st = assume_ref(p, [1, 0, 2], [11, 12, 13])
    np.testing.assert_array_equal(new, [12, 12, -1, 7, -1, -1])
    np.testing.assert_array_equal(committed, [False, True, False])
    assert (st["committed"], st["stale"], st["rows_marked"]) == (1, 2, 2)
    with pytest.raises(BindConflict) as ei:
        assume_ref(p, [0, 1, 1], [1, 2, 3])
    assert ei.value.job == 2
    with pytest.raises(ValueError):
        assume_ref(p, [0, 3, -1], [1, 2, 3])
    with pytest.raises(ValueError):
        assume_ref(p, [0, 1, -1], [1, -1, 3])
    assume_ref(p, [0, 1, -1], [1, 2, -1])                                       # the owner of an unplaced job is ignored


def test_ref_nested_closes_ancestors_and_descendants():
    fl = [np.array([0, 4, 8]), np.array([0, 2, 4, 6, 8]), np.arange(9)]
    classes = [cls(0, 4), cls(1, 2), cls(2, 1)]
    p = nested(fl, [1] * 8, classes, [1])
    new, _, _ = assume_ref(p, [0], [99])                                       # rack 0 of zone 0
    q = with_excl(nested(fl, [1] * 8, classes, [0, 1, 1]), new)
    # zone 0 is closed to the zone job, its rack 1 is not; zone 1's racks go with the zone job
    np.testing.assert_array_equal(O.place_c(q)[0], [1, 1, -1])


# ------------------------------------------------------------------ what the feature is for, on the CPU oracle
def small_nested(seed):
    """A small random nested problem whose batch is split in two."""
    p = synth.random_problem(seed, max_nodes=600, max_leaves=60, max_jobs=60)
    J = p.n_jobs
    first = dataclasses.replace(p, job_class=p.job_class[:J // 2])
    second = dataclasses.replace(p, job_class=p.job_class[J // 2:])
    return p, first, second


@pytest.mark.parametrize("seed", range(40))
def test_second_batch_never_meets_a_committed_domain(seed):
    p, first, second = small_nested(seed)
    a1 = O.place_c(first)[0]
    owner = 0x40000000 + np.arange(first.n_jobs)
    new, committed, st = assume_ref(first, a1, owner)
    np.testing.assert_array_equal(committed, a1 >= 0)                          # the oracle's placement is feasible now
    assert st["stale"] == 0
    a2 = O.place_c(with_excl(second, new))[0]
    assert domains_intersect(p, first.job_class, np.where(committed, a1, -1), second.job_class, a2) == []
    again, committed2, st2 = assume_ref(with_excl(first, new), a1, owner)      # a repeated assume is stale
    assert not committed2.any() and st2["stale"] == int((a1 >= 0).sum())
    np.testing.assert_array_equal(again, new)


@pytest.mark.parametrize("seed", range(40))
def test_forget_of_all_owners_restores_the_column(seed):
    p, first, _ = small_nested(seed)
    a1 = O.place_c(first)[0]
    owner = 0x40000000 + np.arange(first.n_jobs)
    new, committed, st = assume_ref(first, a1, owner)
    back, cleared = forget_ref(new, owner[::-1])
    np.testing.assert_array_equal(back, p.nodes.excl)
    assert cleared == st["rows_marked"] == int((new != p.nodes.excl).sum())
    half = owner[committed][::2]
    part, cleared = forget_ref(new, half)
    assert cleared == int(np.isin(new, half).sum())
    np.testing.assert_array_equal(part[~np.isin(new, half)], new[~np.isin(new, half)])
