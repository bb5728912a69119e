"""jsp_place_whatif without a GPU: the header declares it, the 32-byte struct
and the three defines within ABI v7, header / library / bindings agree, a NULL
engine is JSP_EINVAL and there is no fallback behind the call; the tests'
yardstick (tests/whatif_ref.py) gives the plain placement for a scenario
without rows and the hand cases' stated answers; and the sweep's inputs reach
the coverage floors on the yardstick's own output, so no GPU sweep is vacuous."""
import ctypes
import os
import re

import numpy as np
import pytest

from jobset_amd import native
from oracle import oracle as O
from whatif_ref import EMPTY, SWEEP_SCENARIOS, SWEEP_SEEDS, concat, hand_cases, patched, sweep, whatif_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_jsp_place_whatif():
    src = header("jsplace.h")
    u32p, s = r"const\s+uint32_t\s*\*\s*", r"\s*,\s*"
    assert re.search(r"^int\s+jsp_place_whatif\s*\(\s*jsp_engine\s*\*\s*e" + s + u32p + "run_class" + s + u32p +
                     "run_len" + s + r"uint32_t\s+n_runs" + s + u32p + "scen_off" + s + r"uint32_t\s+n_scen" + s + u32p +
                     "rows" + s + r"const\s+uint64_t\s*\*\s*labels" + s + u32p + "taints" + s + u32p + "free_res" + s +
                     r"const\s+int32_t\s*\*\s*excl_owner" + s + r"uint32_t\s+flags" + s + r"int32_t\s*\*\s*assign_out" +
                     s + r"uint32_t\s*\*\s*placed_out" + s + r"jsp_whatif_stats\s*\*\s*stats\s*\)\s*;", src, flags=re.M)
    assert re.search(r"typedef\s+struct\s+jsp_whatif_stats\s*\{\s*uint32_t\s+jobs\s*;\s*uint32_t\s+scenarios\s*;"
                     r"\s*uint32_t\s+rows\s*;\s*uint32_t\s+runs\s*;\s*uint32_t\s+fused\s*;\s*uint32_t\s+flips\s*;"
                     r"\s*double\s+wall_us\s*;\s*\}\s*jsp_whatif_stats\s*;", src)
    assert re.search(r"#define\s+JSP_WHATIF_MAX_JOBS\s+65536u", src)
    assert re.search(r"#define\s+JSP_WHATIF_MAX_SCENARIOS\s+64u", src)
    assert re.search(r"#define\s+JSP_WHATIF_MAX_ROWS\s+65536u", src)
    assert "#define JSP_ABI_VERSION 7" in src  # additive: a caller detects it by symbol
    assert re.search(r"^int\s+jspb_place_whatif_loop\s*\(", header("jsplace_bench.h"), flags=re.M)


def test_struct_size_is_32():
    assert ctypes.sizeof(native.JspWhatifStats) == 32
    assert [f[0] for f in native.JspWhatifStats._fields_] == ["jobs", "scenarios", "rows", "runs", "fused", "flips",
                                                              "wall_us"]
    assert native.JspWhatifStats.flips.offset == 20
    assert native.JspWhatifStats.wall_us.offset == 24
    assert (native.JSP_WHATIF_MAX_JOBS, native.JSP_WHATIF_MAX_SCENARIOS, native.JSP_WHATIF_MAX_ROWS) == (65536, 64, 65536)


def test_library_and_bindings_have_the_entry_points():
    lib = native.lib()
    bound = {n: (res, args) for n, res, args in native.SIGNATURES}
    for name, nargs in (("jsp_place_whatif", 15), ("jspb_place_whatif_loop", 14)):
        assert hasattr(lib, name), name
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs
    assert lib.jsp_abi_version() == 7


def test_null_engine_is_einval():
    lib = native.lib()
    out = np.zeros(4, dtype=np.int32)
    so = np.zeros(2, dtype=np.uint32)
    st = native.JspWhatifStats()
    assert lib.jsp_place_whatif(None, None, None, 0, so.ctypes.data, 1, None, None, None, None, None, 0,
                                out.ctypes.data, None, ctypes.byref(st)) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()
    us = np.zeros(3)
    assert lib.jspb_place_whatif_loop(None, None, None, 0, so.ctypes.data, 1, None, None, None, None, None,
                                      out.ctypes.data, 1, us.ctypes.data) == native.JSP_EINVAL


def test_no_fallback_behind_the_entry_point():
    """No CPU fallback behind the new entry point either: without a GPU there
    is no engine to call it on, and with one an engine that holds no snapshot
    refuses the call."""
    from jobset_amd.engine import Engine
    with pytest.raises(native.JspError) as ei:
        with Engine(0) as e:
            e.place_whatif(np.zeros(1, dtype=np.uint32), [EMPTY])
    if native.device_count() > 0:
        assert ei.value.code == native.JSP_ESTATE
    else:
        assert ei.value.code == native.JSP_EHIP
        assert "no HIP device" in str(ei.value)


@pytest.mark.parametrize("seed", range(0, 24, 3))
def test_empty_scenario_is_the_plain_placement(seed):
    p = sweep(seed)[0]
    a, placed, flips, opened, closed = whatif_ref(p, [EMPTY, EMPTY])
    plain = O.place_c(p)[0]
    np.testing.assert_array_equal(a[0], plain)
    np.testing.assert_array_equal(a[1], plain)
    assert flips == 0 and list(placed) == [int((plain >= 0).sum())] * 2


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(name):
    p, scenarios, want, flips = hand_cases()[name]
    a, placed, got_flips, _, _ = whatif_ref(p, scenarios)
    np.testing.assert_array_equal(a, want, err_msg=name)
    assert got_flips == flips
    np.testing.assert_array_equal(placed, (np.asarray(want) >= 0).sum(axis=1))


def test_patched_leaves_the_problem_as_it_is():
    p, scenarios = sweep(2)
    before = [c.copy() for c in (p.nodes.labels, p.nodes.taints, p.nodes.free, p.nodes.excl)]
    q = patched(p, scenarios[2])
    for b, c in zip(before, (p.nodes.labels, p.nodes.taints, p.nodes.free, p.nodes.excl)):
        np.testing.assert_array_equal(b, c)
    rows = scenarios[2]["rows"]
    np.testing.assert_array_equal(q.nodes.free[:, rows], scenarios[2]["free_res"])
    np.testing.assert_array_equal(q.nodes.excl[rows], scenarios[2]["excl_owner"])
    so, allrows, lab, tn, fr, ex = concat(scenarios)
    assert so[0] == 0 and so[-1] == allrows.shape[0] == tn.shape[0] == ex.shape[0]
    assert lab.shape == (p.nodes.n_label_words, allrows.shape[0]) and fr.shape == (p.nodes.n_res, allrows.shape[0])


def test_sweep_coverage_floors():
    """On the yardstick's own output over the sweep: at most half of the
    scenarios answer as the unedited snapshot does, at least a quarter hold a
    bit that goes from infeasible to feasible and at least a quarter one that
    goes from feasible to infeasible."""
    total = same = opens = closes = 0
    for seed in SWEEP_SEEDS:
        p, scenarios = sweep(seed)
        assert len(scenarios) == SWEEP_SCENARIOS
        plain = O.place_c(p)[0]
        a, _, _, opened, closed = whatif_ref(p, scenarios)
        for s in range(len(scenarios)):
            total += 1
            same += int(np.array_equal(a[s], plain))
            opens += int(opened[s] > 0)
            closes += int(closed[s] > 0)
    print(f"scenarios {total}, same as the baseline {same}, with an opened bit {opens}, with a closed bit {closes}")
    assert 2 * same <= total
    assert 4 * opens >= total
    assert 4 * closes >= total
