"""jsp_place_sticky without a GPU: the header declares it, the ctypes struct has
the ABI's size, a NULL engine is JSP_EINVAL, header / library / bindings agree,
and the tests' yardstick (tests/sticky_ref.py) satisfies the rule's own
identities on random problems: no hints == the plain placement, the plain
placement as hints is a fixed point with kept <=> assign == prev >= 0, a kept job holds its hint."""
import ctypes
import os
import re

import numpy as np
import pytest

from jobset_amd import native, synth
from oracle import oracle as O
from sticky_ref import check_sticky, greedy_keep, sticky_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_jsp_place_sticky():
    src = header("jsplace.h")
    assert re.search(r"^int\s+jsp_place_sticky\s*\(\s*jsp_engine\s*\*\s*e\s*,\s*const\s+uint32_t\s*\*\s*run_class\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*run_len\s*,\s*uint32_t\s+n_runs\s*,\s*const\s+int32_t\s*\*\s*prev_assign"
                     r"\s*,\s*int32_t\s*\*\s*assign_out\s*,\s*jsp_sticky_stats\s*\*\s*stats\s*\)\s*;", src, flags=re.M)
    assert "typedef struct jsp_sticky_stats" in src
    assert "#define JSP_ABI_VERSION 7" in src  # additive: a caller detects it by symbol
    assert re.search(r"^int\s+jspb_place_sticky_loop\s*\(", header("jsplace_bench.h"), flags=re.M)


def test_struct_size_is_32():
    assert ctypes.sizeof(native.JspStickyStats) == 32
    assert [f[0] for f in native.JspStickyStats._fields_] == ["jobs", "placed", "hinted", "kept", "runs", "fused",
                                                              "wall_us"]
    assert native.JspStickyStats.kept.offset == 12
    assert native.JspStickyStats.wall_us.offset == 24


def test_library_and_bindings_have_the_entry_points():
    lib = native.lib()
    bound = {n: (res, args) for n, res, args in native.SIGNATURES}
    for name, nargs in (("jsp_place_sticky", 7), ("jspb_place_sticky_loop", 8)):
        assert hasattr(lib, name), name
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs
    assert lib.jsp_abi_version() == 7


def test_null_engine_is_einval():
    lib = native.lib()
    out = np.zeros(4, dtype=np.int32)
    st = native.JspStickyStats()
    assert lib.jsp_place_sticky(None, None, None, 0, None, out.ctypes.data, ctypes.byref(st)) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()
    us = np.zeros(3)
    assert lib.jspb_place_sticky_loop(None, None, None, 0, None, out.ctypes.data, 1, us.ctypes.data) == native.JSP_EINVAL


@pytest.mark.parametrize("seed", range(24))
def test_reference_identities(seed):
    p = synth.random_problem(seed, max_nodes=600, max_leaves=40)
    plain, cap, occ = O.place_c(p)
    none, kept = sticky_ref(p, None, (cap, occ))
    np.testing.assert_array_equal(none, plain)
    assert not kept.any()
    minus, _ = sticky_ref(p, np.full(p.n_jobs, -1), (cap, occ))
    np.testing.assert_array_equal(minus, plain)
    fix, kept = sticky_ref(p, plain, (cap, occ))
    np.testing.assert_array_equal(fix, plain)
    np.testing.assert_array_equal(kept, plain >= 0)
    # random in-range hints: I1 / I2, and a kept job holds its hint. (The converse holds for
    # pairwise disjoint hints, above; with garbage hints a job that lost its claim to a claimant
    # that lost its own can be filled back onto its hinted domain by the lowest-index rule.)
    lvl = np.array([p.classes[int(c)].level for c in p.job_class], dtype=np.int64)
    nd = np.array(p.topology.n_domains, dtype=np.int64)[lvl] if p.n_jobs else np.zeros(0, dtype=np.int64)
    prev = synth.uniform_int(seed, 7001, p.n_jobs, 0, 1 << 30) % np.maximum(nd, 1)
    a, kept = sticky_ref(p, prev, (cap, occ))
    check_sticky(p, prev, a, (cap, occ))
    assert np.all(a[kept] == prev[kept])
    # pairwise disjoint hints (an earlier placement): the rule is the sequential greedy
    np.testing.assert_array_equal(sticky_ref(p, plain, (cap, occ))[1], greedy_keep(p, plain, (cap, occ)))
