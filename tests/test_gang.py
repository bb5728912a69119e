"""jsp_place_gangs without a GPU: the header declares it and the 32-byte
struct, header / library / bindings agree, a NULL engine is JSP_EINVAL and an
engine without a GPU fails loudly; the tests' yardstick (tests/gang_ref.py)
reduces to the plain placement in the two ways DESIGN.md §2 "Gang placement"
states and satisfies I1 / I2 / whole-or-nothing on random problems; the
sweeps' inputs reach the coverage floors on the yardstick's own output, so no
GPU sweep is vacuous; and the host gang walk (jsp_walk.cc walk_gangs), fed the
yardstick's feasibility words, gives the yardstick's answer with exact span
counts and with the loosest sound ones."""
import ctypes
import os
import re

import numpy as np
import pytest

from jobset_amd import native, synth
from oracle import oracle as O
from gang_ref import (ANY, SWEEP_SEEDS, check_gangs, feas_words, gang_ref, gang_runs_of, reduction_problem,
                      span_counts_ref, sweep_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_jsp_place_gangs():
    src = header("jsplace.h")
    assert re.search(r"^int\s+jsp_place_gangs\s*\(\s*jsp_engine\s*\*\s*e\s*,\s*const\s+uint32_t\s*\*\s*run_class\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*run_len\s*,\s*uint32_t\s+n_runs\s*,\s*const\s+uint32_t\s*\*\s*gang_runs"
                     r"\s*,\s*const\s+uint32_t\s*\*\s*gang_span\s*,\s*uint32_t\s+n_gangs\s*,\s*uint32_t\s+flags\s*,"
                     r"\s*int32_t\s*\*\s*assign_out\s*,\s*int32_t\s*\*\s*gang_span_out\s*,\s*jsp_gang_stats\s*\*\s*stats"
                     r"\s*\)\s*;", src, flags=re.M)
    assert "typedef struct jsp_gang_stats" in src
    assert re.search(r"#define\s+JSP_SPAN_ANY\s+0xFFFFFFFFu", src)
    assert re.search(r"#define\s+JSP_GANG_MAX_JOBS\s+65536u", src)
    assert "#define JSP_ABI_VERSION 7" in src  # additive: a caller detects it by symbol
    bench = header("jsplace_bench.h")
    assert re.search(r"^int\s+jspb_place_gangs_loop\s*\(", bench, flags=re.M)
    assert re.search(r"^int\s+jspb_span_counts\s*\(", bench, flags=re.M)


def test_struct_size_is_32():
    assert ctypes.sizeof(native.JspGangStats) == 32
    assert [f[0] for f in native.JspGangStats._fields_] == ["jobs", "placed", "gangs", "gangs_placed", "runs", "fused",
                                                            "wall_us"]
    assert native.JspGangStats.gangs_placed.offset == 12
    assert native.JspGangStats.wall_us.offset == 24
    assert native.JSP_SPAN_ANY == 0xFFFFFFFF and native.JSP_GANG_MAX_JOBS == 65536


def test_library_and_bindings_have_the_entry_points():
    lib = native.lib()
    bound = {n: (res, args) for n, res, args in native.SIGNATURES}
    for name, nargs in (("jsp_place_gangs", 11), ("jspb_place_gangs_loop", 11), ("jspb_span_counts", 6)):
        assert hasattr(lib, name), name
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs
    assert lib.jsp_abi_version() == 7


def test_null_engine_is_einval():
    lib = native.lib()
    out = np.zeros(4, dtype=np.int32)
    st = native.JspGangStats()
    assert lib.jsp_place_gangs(None, None, None, 0, None, None, 0, 0, out.ctypes.data, None,
                               ctypes.byref(st)) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()
    us = np.zeros(3)
    assert lib.jspb_place_gangs_loop(None, None, None, 0, None, None, 0, out.ctypes.data, None, 1,
                                     us.ctypes.data) == native.JSP_EINVAL
    assert lib.jspb_span_counts(None, 0, None, 0, 0, None) == native.JSP_EINVAL


def test_no_gpu_fails_loudly():
    """No CPU fallback behind the new entry point either: without a GPU there
    is no engine to call it on."""
    if native.device_count() > 0:
        pytest.skip("a GPU is present")
    from jobset_amd.engine import Engine
    with pytest.raises(native.JspError) as ei:
        Engine(0).place_gangs(np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int64), [ANY])
    assert ei.value.code == native.JSP_EHIP
    assert "no HIP device" in str(ei.value)


@pytest.mark.parametrize("i", range(60))
def test_reference_reductions(i):
    """One gang per job with ANY is the plain placement bit for bit; one gang
    over the whole batch with ANY is the plain placement if that places every
    job, else all -1. I1 / I2 / whole-or-nothing on every answer."""
    p = reduction_problem(i)
    plain, cap, occ = O.place_c(p)
    J = p.n_jobs
    ones = np.ones(J, dtype=np.int64)
    a, so = gang_ref(p, ones, np.full(J, ANY), (cap, occ))
    np.testing.assert_array_equal(a, plain)
    np.testing.assert_array_equal(so, np.where(plain >= 0, 0, -1))
    check_gangs(p, ones, np.full(J, ANY), a, so, (cap, occ))
    a, so = gang_ref(p, [J], [ANY], (cap, occ))
    if J > 0 and np.all(plain >= 0):
        np.testing.assert_array_equal(a, plain)
        assert so[0] == 0
    else:
        assert np.all(a == -1) and so[0] == -1
    check_gangs(p, [J], [ANY], a, so, (cap, occ))
    # a span at the job's own level, one gang per job: the span domain is the job's domain
    lvl = np.array([p.classes[int(c)].level for c in p.job_class], dtype=np.int64)
    a, so = gang_ref(p, ones, lvl, (cap, occ))
    np.testing.assert_array_equal(a, plain)
    np.testing.assert_array_equal(so, plain)


def test_reference_reductions_cover_both_outcomes():
    """The whole-batch reduction sees batches that place whole and batches that do not."""
    whole = 0
    for i in range(60):
        p = reduction_problem(i)
        whole += int(p.n_jobs > 0 and np.all(O.place_c(p)[0] >= 0))
    print(f"{whole} of 60 batches place whole")
    assert 10 <= whole <= 50, whole


@pytest.fixture(scope="module")
def sweep():
    out = []
    for seed in SWEEP_SEEDS:
        p, gj, gs = sweep_case(seed)
        plain, cap, occ = O.place_c(p)
        a, so = gang_ref(p, gj, gs, (cap, occ))
        out.append((p, gj, gs, plain, cap, occ, a, so))
    return out


def test_sweep_answers_hold_the_invariants(sweep):
    for p, gj, gs, _, cap, occ, a, so in sweep:
        check_gangs(p, gj, gs, a, so, (cap, occ))


def test_sweep_coverage_floors(sweep):
    """On the reference's own output: >= 25 % of gangs placed and >= 25 %
    refused; >= 10 % of the placed spanned gangs on a span domain other than
    0; >= 10 % of all gangs refused although the plain placement places at
    least one of their jobs. Measured with this generator over the 60 seeds:
    43 % placed, 57 % refused, 91 % off domain 0, 30 % refused-but-partly-placeable."""
    G = placed = spanned = off0 = partly = 0
    for p, gj, gs, plain, _, _, a, so in sweep:
        j0 = 0
        for g, n in enumerate(gj):
            G += 1
            if so[g] >= 0:
                placed += 1
                if gs[g] != ANY:
                    spanned += 1
                    off0 += int(so[g] != 0)
            else:
                partly += int(np.any(plain[j0:j0 + n] >= 0))
            j0 += int(n)
    print(f"gangs {G}: placed {placed / G:.2f}, refused {(G - placed) / G:.2f}, "
          f"off domain 0 {off0 / max(spanned, 1):.2f} of {spanned}, refused-but-partly-placeable {partly / G:.2f}")
    assert placed >= 0.25 * G and G - placed >= 0.25 * G
    assert spanned > 0 and off0 >= 0.10 * spanned
    assert partly >= 0.10 * G
    # every span kind occurs: ANY, the coarsest level, a finer one
    kinds = {("any" if s == ANY else "0" if s == 0 else "finer") for _, _, gs, *_ in sweep for s in gs}
    assert kinds == {"any", "0", "finer"}


def _walk(p, cap, occ, gj, gs, all_ones, runs=None):
    lib = native.lib()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    fn = lib.jspi_gang_walk_test
    fn.restype = ctypes.c_int
    fn.argtypes = [u32, vp, vp, u32, vp, vp, vp, ctypes.c_int, vp, vp, u32, vp, vp, u32, vp, vp, vp]
    topo = p.topology
    K = topo.n_levels
    D = (u32 * 4)(*([topo.n_domains[k] for k in range(K)] + [0] * (4 - K)))
    fls = [np.ascontiguousarray(topo.first_leaf[k], dtype=np.uint32) for k in range(K)]
    flp = (vp * 4)(*([f.ctypes.data for f in fls] + [None] * (4 - K)))
    lv = np.array([c.level for c in p.classes], dtype=np.uint32)
    pods = np.array([c.pods for c in p.classes], dtype=np.uint32)
    fw = np.ascontiguousarray(np.concatenate([feas_words(p, cap, occ), np.zeros(1, dtype=np.uint64)]))
    # runs: (run_class, run_len, gang_runs) of the same jobs and gangs in another form (tests/run_forms.py)
    rc, rl, gr = gang_runs_of(p.job_class, gj) if runs is None else (np.ascontiguousarray(a, dtype=np.uint32) for a in runs)
    sp = np.ascontiguousarray(np.asarray(gs, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    out = np.full(p.n_jobs + 1, -7, dtype=np.int32)          # one spare element each, which must stay as it is
    sout = np.full(len(gr) + 1, -7, dtype=np.int32)
    gp = u32(0)
    placed = fn(K, D, flp, len(p.classes), lv.ctypes.data, pods.ctypes.data, fw.ctypes.data, all_ones, rc.ctypes.data,
                rl.ctypes.data, len(rc), gr.ctypes.data, sp.ctypes.data, len(gr), out.ctypes.data, sout.ctypes.data,
                ctypes.byref(gp))
    assert out[p.n_jobs] == -7 and sout[len(gr)] == -7, "the walk wrote behind assign[J) or gang_span_out[G)"
    return out[:p.n_jobs], sout[:len(gr)], placed, gp.value


@pytest.mark.parametrize("all_ones", [0, 1])
def test_host_gang_walk_matches_the_reference(sweep, all_ones):
    """The walk the engine runs on the host, on the reference's feasibility:
    bit-equal with exact span counts and with counts that filter nothing out
    (the prefilter is sound, and the answer does not depend on its tightness)."""
    for p, gj, gs, _, cap, occ, a, so in sweep:
        out, sout, placed, gp = _walk(p, cap, occ, gj, gs, all_ones)
        np.testing.assert_array_equal(out, a, err_msg=p.name)
        np.testing.assert_array_equal(sout, so, err_msg=p.name)
        assert placed == int((a >= 0).sum()) and gp == int((so >= 0).sum())


def test_host_gang_walk_reductions():
    """Both reductions through the host walk on random_problem's own classes."""
    for i in range(60):
        p = reduction_problem(i)
        plain, cap, occ = O.place_c(p)
        J = p.n_jobs
        out, sout, _, _ = _walk(p, cap, occ, np.ones(J, dtype=np.int64), np.full(J, ANY), 0)
        np.testing.assert_array_equal(out, plain)
        out, sout, _, gp = _walk(p, cap, occ, [J], [ANY], 0)
        if J > 0 and np.all(plain >= 0):
            np.testing.assert_array_equal(out, plain)
        else:
            assert np.all(out == -1) and sout[0] == -1 and gp == 0


def test_span_counts_reference_is_consistent(sweep):
    """The numpy span counts the GPU test compares with: at s == level the
    count is the feasibility bit, and a level's counts sum to the feasible total."""
    for p, _, _, _, cap, occ, _, _ in sweep:
        cnt = span_counts_ref(p, cap, occ)
        words = feas_words(p, cap, occ)
        off = woff = 0
        for c, jc in enumerate(p.classes):
            D = p.topology.n_domains[jc.level]
            nw = (D + 63) // 64
            bits = np.unpackbits(words[woff:woff + nw].view(np.uint8), bitorder="little")[:D]
            for s in range(jc.level + 1):
                Ds = p.topology.n_domains[s]
                assert int(cnt[off:off + Ds].sum()) == int(bits.sum())
                if s == jc.level:
                    np.testing.assert_array_equal(cnt[off:off + Ds], bits)
                off += Ds
            woff += nw
        assert off == cnt.shape[0]
