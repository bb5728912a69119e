"""jsp_place_preempt without a GPU: the header declares it, the 32-byte struct
and the three defines, header / library / bindings agree, a NULL engine is
JSP_EINVAL and an engine without a GPU fails loudly; the tests' yardstick
(tests/preempt_ref.py) reduces to the plain placement with an empty table and
at prio 0, gives the hand cases' answers and holds check_preempt on every
sweep answer; the sweep's inputs reach the coverage floors on the yardstick's
own output, so no GPU sweep is vacuous; and the host fit walk (jsp_walk.cc
walk_fit), fed the yardstick's candidate lists, gives the yardstick's answer."""
import ctypes
import os
import re

import numpy as np
import pytest

from jobset_amd import native
from jobset_amd.native import JspPreemptStats   # the binding this file is about
from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from preempt_ref import (BLOCKER, SWEEP_PRIOS, SWEEP_SEEDS, check_preempt, domain_table, hand_cases, order_ref,
                         preempt_ref, reduction_problem, row_codes, sweep)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_jsp_place_preempt():
    src = header("jsplace.h")
    ws = r"\s*"
    decl = ws.join([r"^int\s+jsp_place_preempt", r"\(", r"jsp_engine", r"\*", r"e", ",",
                    r"const\s+uint32_t", r"\*", "run_class", ",", r"const\s+uint32_t", r"\*", "run_len", ",",
                    r"uint32_t\s+n_runs", ",", r"uint32_t\s+prio", ",", r"const\s+int32_t", r"\*", "owner_ids", ",",
                    r"const\s+uint32_t", r"\*", "owner_prio", ",", r"uint32_t\s+n_owners", ",",
                    r"const\s+uint32_t", r"\*", "evict_free", ",", r"uint32_t\s+flags", ",",
                    r"int32_t", r"\*", "assign_out", ",", r"uint32_t", r"\*", "victim_off_out", ",",
                    r"int32_t", r"\*", "victims_out", ",", r"uint32_t\s+victims_cap", ",",
                    r"jsp_preempt_stats", r"\*", "stats", r"\)", ";"])
    assert re.search(decl, src, flags=re.M)
    assert re.search(r"typedef\s+struct\s+jsp_preempt_stats\s*\{\s*uint32_t\s+jobs\s*;\s*uint32_t\s+placed\s*;"
                     r"\s*uint32_t\s+preempting\s*;\s*uint32_t\s+victims\s*;\s*uint32_t\s+runs\s*;"
                     r"\s*uint32_t\s+fused\s*;\s*double\s+wall_us\s*;\s*\}\s*jsp_preempt_stats\s*;", src)
    assert re.search(r"#define\s+JSP_PREEMPT_MAX_JOBS\s+65536u", src)
    assert re.search(r"#define\s+JSP_PREEMPT_MAX_OWNERS\s+65536u", src)
    assert re.search(r"#define\s+JSP_PREEMPT_MAX_PRIO\s+65535u", src)
    assert "#define JSP_ABI_VERSION 7" in src  # additive: a caller detects it by symbol
    bench = header("jsplace_bench.h")
    assert re.search(r"^int\s+jspb_place_preempt_loop\s*\(", bench, flags=re.M)
    assert re.search(r"^int\s+jspb_preempt_order\s*\(", bench, flags=re.M)


def test_struct_size_is_32():
    S = JspPreemptStats
    assert ctypes.sizeof(S) == 32
    assert [f[0] for f in S._fields_] == ["jobs", "placed", "preempting", "victims", "runs", "fused", "wall_us"]
    assert [getattr(S, f).offset for f in ("jobs", "placed", "preempting", "victims", "runs", "fused", "wall_us")] == \
        [0, 4, 8, 12, 16, 20, 24]
    assert (native.JSP_PREEMPT_MAX_JOBS, native.JSP_PREEMPT_MAX_OWNERS, native.JSP_PREEMPT_MAX_PRIO) == \
        (65536, 65536, 65535)


def test_library_and_bindings_have_the_entry_points():
    lib = native.lib()
    bound = {n: (res, args) for n, res, args in native.SIGNATURES}
    for name, nargs in (("jsp_place_preempt", 15), ("jspb_place_preempt_loop", 16), ("jspb_preempt_order", 14)):
        assert hasattr(lib, name), name
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs
    assert lib.jsp_abi_version() == 7


def test_null_engine_is_einval():
    lib = native.lib()
    out = np.zeros(4, dtype=np.int32)
    off = np.zeros(5, dtype=np.uint32)
    st = JspPreemptStats()
    assert lib.jsp_place_preempt(None, None, None, 0, 1, None, None, 0, None, 0, out.ctypes.data, off.ctypes.data, None,
                                 0, ctypes.byref(st)) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()
    us = np.zeros(3)
    assert lib.jspb_place_preempt_loop(None, None, None, 0, 1, None, None, 0, None, out.ctypes.data, None, None, 0, None,
                                       1, us.ctypes.data) == native.JSP_EINVAL
    assert lib.jspb_preempt_order(None, 1, None, None, 0, None, 0, None, 0, None, None, None, 0, None) == native.JSP_EINVAL


def test_no_gpu_fails_loudly():
    """No CPU fallback behind the new entry point either: without a GPU there
    is no engine to call it on."""
    if native.device_count() > 0:
        pytest.skip("a GPU is present")
    from jobset_amd.engine import Engine
    with pytest.raises(native.JspError) as ei:
        Engine(0).place_preempt(np.zeros(1, dtype=np.uint32), 1, [5], [0])
    assert ei.value.code == native.JSP_EHIP
    assert "no HIP device" in str(ei.value)


@pytest.mark.parametrize("i", range(60))
def test_reference_reductions_are_the_plain_placement(i):
    """An empty table, and prio 0 with every owner in the table, give the plain
    placement bit for bit, without victims."""
    p = reduction_problem(i)
    plain = O.place_c(p)[0]
    ids = np.unique(p.nodes.excl[p.nodes.excl != -1])
    for prio, ow, pr in ((7, [], []), (0, ids, np.zeros(ids.shape[0], dtype=np.uint32))):
        a, off, v, st = preempt_ref(p, prio, ow, pr)
        np.testing.assert_array_equal(a, plain)
        assert v.shape[0] == 0 and not off.any()
        assert st == dict(jobs=p.n_jobs, placed=int((plain >= 0).sum()), preempting=0, victims=0, runs=st["runs"],
                          fused=7)


@pytest.mark.parametrize("name", list(hand_cases()))
def test_reference_hand_cases(name):
    p, prio, ow, pr, ef, want, want_v = hand_cases()[name]
    a, off, v, st = preempt_ref(p, prio, ow, pr, ef)
    np.testing.assert_array_equal(a, want)
    assert [v[off[j]:off[j + 1]].tolist() for j in range(p.n_jobs)] == want_v
    assert st["victims"] == sum(len(x) for x in want_v) and st["preempting"] == sum(1 for x in want_v if x)
    check_preempt(p, prio, ow, pr, ef, a, off, v)
    if name == "zone-owner":
        assert st["victims"] == 2 and np.unique(v).shape[0] == 1   # named twice, one to evict
    if name == "split-owner":
        assert domain_table(p, prio, ow, pr, ef)[0][2].tolist() == [3]
    if name == "leaf-boundary-taken":
        assert domain_table(p, prio, ow, pr, ef)[0][2].tolist() == [1, 0]   # one segment over two leaves
    if name == "domain-boundary":
        assert domain_table(p, prio, ow, pr, ef)[0][2].tolist() == [1, 1]   # and one in each of two domains


def _walk(p, order, nf):
    """jspi_fit_walk_test on the lists, without fit values: (assign, placed)."""
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
    nf = np.ascontiguousarray(nf, dtype=np.uint32)
    rc, rl = job_runs(p.job_class)
    rc, rl = np.ascontiguousarray(rc, dtype=np.uint32), np.ascontiguousarray(rl, dtype=np.uint32)
    out = np.full(p.n_jobs + 1, -7, dtype=np.int32)           # one spare element, which must stay as it is
    placed = fn(K, D, flp, len(p.classes), lv.ctypes.data, pods.ctypes.data, order.ctypes.data, nf.ctypes.data,
                None, rc.ctypes.data, rl.ctypes.data, len(rc), out.ctypes.data, None)
    assert out[p.n_jobs] == -7, "the walk wrote behind assign[J)"
    return out[:p.n_jobs], placed


@pytest.fixture(scope="module")
def swept():
    out = []
    for seed in SWEEP_SEEDS:
        p, ids, rk, ef = sweep(seed)
        ans = {}
        for prio in SWEEP_PRIOS:
            tab = domain_table(p, prio, ids, rk, ef)
            ans[prio] = (tab, preempt_ref(p, prio, ids, rk, ef, tab=tab))
        out.append((p, ids, rk, ef, ans))
    return out


def test_sweep_answers_hold_check_preempt(swept):
    for p, ids, rk, ef, ans in swept:
        for prio, (tab, (a, off, v, st)) in ans.items():
            check_preempt(p, prio, ids, rk, ef, a, off, v, tab=tab)


def test_sweep_coverage_floors(swept):
    """On the reference's own output at prio 4 over the 40 sweep inputs: more
    jobs placed than the plain placement on >= 20, some job with victims on
    >= 20, two reachable domains of one class sharing a non-zero key on >= 25,
    zero-victim and preempting jobs in one answer on >= 15, some owner a
    blocker on >= 25, and the empty table giving O.place_c on all 40."""
    more = vict = ties = mixed = block = red = 0
    for p, ids, rk, ef, ans in swept:
        tab, (a, off, v, st) = ans[4]
        plain = O.place_c(p)[0]
        red += int(np.array_equal(preempt_ref(p, 4, [], [], ef)[0], plain))
        more += int((a >= 0).sum() > (plain >= 0).sum())
        vict += int(st["victims"] > 0)
        tie = False
        for reach, key, _ in tab:
            k = key[reach]
            k = k[k != 0]
            tie |= np.unique(k).shape[0] < k.shape[0]
        ties += int(tie)
        n_v = np.diff(off.astype(np.int64))
        mixed += int(bool(((a >= 0) & (n_v == 0)).any()) and bool((n_v > 0).any()))
        block += int((row_codes(p.nodes.excl, 4, ids, rk) == BLOCKER).any())
    print(f"more {more}, victims {vict}, key ties {ties}, mixed {mixed}, blockers {block}, reduction {red}")
    assert more >= 20 and vict >= 20 and ties >= 25 and mixed >= 15 and block >= 25 and red == 40


def test_host_walk_matches_the_reference(swept):
    """The walk the engine runs on the host (walk_fit without fit values), on
    the reference's candidate lists: the reference's answer."""
    for p, ids, rk, ef, ans in swept:
        for prio, (tab, (a, off, v, st)) in ans.items():
            order, nf, key, seg = order_ref(p, prio, ids, rk, ef, tab=tab)
            out, placed = _walk(p, order, nf)
            np.testing.assert_array_equal(out, a, err_msg=f"{p.name} prio {prio}")
            assert placed == st["placed"]


@pytest.mark.parametrize("name", list(hand_cases()))
def test_host_walk_hand_cases(name):
    p, prio, ow, pr, ef, want, _ = hand_cases()[name]
    order, nf, key, seg = order_ref(p, prio, ow, pr, ef)
    out, placed = _walk(p, order, nf)
    np.testing.assert_array_equal(out, want)
