"""jsp_place_spread without a GPU: the header declares it, the 32-byte struct
and the three defines, header / library / bindings agree, a NULL engine is
JSP_EINVAL and an engine without a GPU fails loudly; the tests' yardstick
(tests/spread_ref.py) gives the hand-computed answers, reduces to the oracle's
jsp_place in the four ways DESIGN.md §2 "Spread placement" names, and holds
check_spread on every sweep answer; the sweep's inputs reach the coverage
floors on the yardstick's own output, so no GPU sweep is vacuous; and the host
spread walk (jsp_walk.cc walk_spread), fed the yardstick's words and peer
counts, gives the yardstick's answer."""
import ctypes
import os
import re

import numpy as np
import pytest

from jobset_amd import native
from jobset_amd.native import JspSpreadStats   # the binding this file is about
from jobset_amd.snapshot import job_runs
from oracle import oracle as O
from gang_ref import feas_words
from spread_ref import (SOFT, SWEEP_SEEDS, check_spread, fits_table, fits_words, hand_cases, one_class, owners_of,
                        peers_ref, reduction_problem, rooted, spread_ref, sweep)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_jsp_place_spread():
    src = header("jsplace.h")
    ws = r"\s*"
    decl = ws.join([r"^int\s+jsp_place_spread", r"\(", r"jsp_engine", r"\*", r"e", ",",
                    r"const\s+uint32_t", r"\*", "run_class", ",", r"const\s+uint32_t", r"\*", "run_len", ",",
                    r"uint32_t\s+n_runs", ",", r"uint32_t\s+spread_level", ",", r"uint32_t\s+max_skew", ",",
                    r"const\s+int32_t", r"\*", "peer_ids", ",", r"uint32_t\s+n_peers", ",", r"uint32_t\s+flags", ",",
                    r"int32_t", r"\*", "assign_out", ",", r"int32_t", r"\*", "spread_out", ",",
                    r"uint32_t", r"\*", "count_out", ",", r"jsp_spread_stats", r"\*", "stats", r"\)", ";"])
    assert re.search(decl, src, flags=re.M)
    assert re.search(r"typedef\s+struct\s+jsp_spread_stats\s*\{\s*uint32_t\s+jobs\s*;\s*uint32_t\s+placed\s*;"
                     r"\s*uint32_t\s+refused\s*;\s*uint32_t\s+skew\s*;\s*uint32_t\s+runs\s*;"
                     r"\s*uint32_t\s+fused\s*;\s*double\s+wall_us\s*;\s*\}\s*jsp_spread_stats\s*;", src)
    assert re.search(r"#define\s+JSP_SPREAD_SOFT\s+0u", src)
    assert re.search(r"#define\s+JSP_SPREAD_MAX_JOBS\s+65536u", src)
    assert re.search(r"#define\s+JSP_SPREAD_MAX_PEERS\s+65536u", src)
    assert "#define JSP_ABI_VERSION 7" in src  # additive: a caller detects it by symbol
    bench = header("jsplace_bench.h")
    assert re.search(r"^int\s+jspb_place_spread_loop\s*\(", bench, flags=re.M)
    assert re.search(r"^int\s+jspb_spread_tables\s*\(", bench, flags=re.M)


def test_struct_size_is_32():
    S = JspSpreadStats
    assert ctypes.sizeof(S) == 32
    assert [f[0] for f in S._fields_] == ["jobs", "placed", "refused", "skew", "runs", "fused", "wall_us"]
    assert [getattr(S, f).offset for f in ("jobs", "placed", "refused", "skew", "runs", "fused", "wall_us")] == \
        [0, 4, 8, 12, 16, 20, 24]
    assert (native.JSP_SPREAD_SOFT, native.JSP_SPREAD_MAX_JOBS, native.JSP_SPREAD_MAX_PEERS) == (0, 65536, 65536)


def test_library_and_bindings_have_the_entry_points():
    lib = native.lib()
    bound = {n: (res, args) for n, res, args in native.SIGNATURES}
    for name, nargs in (("jsp_place_spread", 13), ("jspb_place_spread_loop", 14), ("jspb_spread_tables", 14)):
        assert hasattr(lib, name), name
        assert bound[name][0] is ctypes.c_int and len(bound[name][1]) == nargs
    assert hasattr(lib, "jspi_spread_walk_test")
    assert lib.jsp_abi_version() == 7


def test_null_engine_is_einval():
    lib = native.lib()
    out = np.zeros(4, dtype=np.int32)
    st = JspSpreadStats()
    assert lib.jsp_place_spread(None, None, None, 0, 0, 1, None, 0, 0, out.ctypes.data, None, None,
                                ctypes.byref(st)) == native.JSP_EINVAL
    assert b"NULL" in lib.jsp_last_error()
    us = np.zeros(4)
    assert lib.jspb_place_spread_loop(None, None, None, 0, 0, 1, None, 0, out.ctypes.data, None, None, None, 1,
                                      us.ctypes.data) == native.JSP_EINVAL
    assert lib.jspb_spread_tables(None, 0, None, 0, 0, -1, None, None, 0, None, None, None, 0, None) == native.JSP_EINVAL


def test_no_gpu_fails_loudly():
    """No CPU fallback behind the new entry point either: without a GPU there
    is no engine to call it on."""
    if native.device_count() > 0:
        pytest.skip("a GPU is present")
    from jobset_amd.engine import Engine
    with pytest.raises(native.JspError) as ei:
        Engine(0).place_spread(np.zeros(1, dtype=np.uint32), 0, 1, [5])
    assert ei.value.code == native.JSP_EHIP
    assert "no HIP device" in str(ei.value)


@pytest.mark.parametrize("name", list(hand_cases()))
def test_reference_hand_cases(name):
    p, s, k, peers, want, want_s, want_n, want_refused = hand_cases()[name]
    a, sp, cnt, st, _ = spread_ref(p, s, k, peers)
    np.testing.assert_array_equal(a, want)
    np.testing.assert_array_equal(sp, want_s)
    np.testing.assert_array_equal(cnt, want_n)
    assert st["refused"] == want_refused and st["placed"] == sum(1 for x in want if x >= 0)
    check_spread(p, s, k, peers, a, sp, cnt)
    if name == "peer-crosses":
        assert peers_ref(p, 0, peers).tolist() == [1, 1] and peers_ref(p, 1, peers).tolist() == [0, 1, 1, 0]
    if name == "not-eligible":
        assert st["skew"] == 0       # zone 1 is not eligible: it does not enter the skew either
    if name == "full-pins":
        assert st["skew"] == 1


# ---- the four reductions against the oracle's jsp_place
ROOTABLE = [i for i in range(60) if reduction_problem(i).topology.n_levels < 4]
WITH_JOBS = [i for i in range(60) if reduction_problem(i).n_jobs > 0]


@pytest.mark.parametrize("i", ROOTABLE)
def test_one_spread_domain_is_the_plain_placement(i):
    """A topology with one level-s domain: jsp_place's answer bit for bit, for
    every max_skew and peer list."""
    p = rooted(reduction_problem(i))
    plain, cap, occ = O.place_c(p)
    own = owners_of(p)
    for k in (SOFT, 1, 3):
        for peers in ([], own, own[::2]):
            a, sp, cnt, st, _ = spread_ref(p, 0, k, peers, (cap, occ))
            np.testing.assert_array_equal(a, plain)
            assert st["refused"] == 0 and st["skew"] == 0 and st["placed"] == int((plain >= 0).sum())
            assert cnt.tolist() == [int(peers_ref(p, 0, peers)[0]) + st["placed"]]
            assert np.array_equal(sp, np.where(plain >= 0, 0, -1))


@pytest.mark.parametrize("i", WITH_JOBS)
def test_own_level_without_peers_is_the_plain_placement(i):
    """One class with level[c] == s and no peers: jsp_place's answer."""
    p = one_class(reduction_problem(i))
    plain, cap, occ = O.place_c(p)
    s = p.classes[int(p.job_class[0])].level
    for k in (SOFT, 1, 3):
        a, sp, cnt, st, _ = spread_ref(p, s, k, [], (cap, occ))
        np.testing.assert_array_equal(a, plain)
        np.testing.assert_array_equal(sp, plain)
        assert st["refused"] == 0


@pytest.mark.parametrize("i", WITH_JOBS)
def test_soft_places_as_many_as_the_plain_placement(i):
    """SOFT and a one-class batch: `placed` equals jsp_place's, whatever the
    level and the peers."""
    p = one_class(reduction_problem(i))
    plain, cap, occ = O.place_c(p)
    for s in range(p.classes[int(p.job_class[0])].level + 1):
        for peers in ([], owners_of(p)):
            a, sp, cnt, st, _ = spread_ref(p, s, SOFT, peers, (cap, occ))
            assert st["placed"] == int((plain >= 0).sum()) and st["refused"] == 0


@pytest.mark.parametrize("i", WITH_JOBS)
def test_skew_bound_holds_after_every_prefix(i):
    """max_skew = k, one class, no peers: after every prefix of the jobs
    max n - min n over the eligible S is at most k."""
    p = one_class(reduction_problem(i))
    cap, occ = O.place_c(p)[1:]
    c = int(p.job_class[0])
    lvl = p.classes[c].level
    f = np.asarray(p.topology.first_leaf[lvl], dtype=np.int64)
    fits = fits_table(p, cap)[c] & (f[:-1] < f[1:])
    for s in range(lvl + 1):
        fs = np.asarray(p.topology.first_leaf[s], dtype=np.int64)
        elig = np.array([bool((fits & (f[:-1] >= fs[S]) & (f[1:] <= fs[S + 1])).any())
                         for S in range(p.topology.n_domains[s])], dtype=bool)
        for k in (1, 3):
            a, sp, cnt, st, _ = spread_ref(p, s, k, [], (cap, occ))
            n = np.zeros(elig.shape[0], dtype=np.int64)
            for S in sp:
                if S >= 0:
                    assert elig[S]
                    n[S] += 1
                    assert n[elig].max() - n[elig].min() <= k
            assert st["skew"] <= k


# ---- the sweep
@pytest.fixture(scope="module")
def swept():
    out = []
    for seed in SWEEP_SEEDS:
        p, s, k, peers = sweep(seed)
        plain, cap, occ = O.place_c(p)
        out.append((p, s, k, peers, plain, (cap, occ), spread_ref(p, s, k, peers, (cap, occ))))
    return out


def test_sweep_answers_hold_check_spread(swept):
    for p, s, k, peers, plain, tallies, (a, sp, cnt, st, _) in swept:
        check_spread(p, s, k, peers, a, sp, cnt, tallies)


def test_sweep_coverage_floors(swept):
    """On the yardstick's own output over the sweep's cases: an answer that
    differs from jsp_place's on at least a third, refused > 0 on at least a
    fifth, peers that change the answer compared with an empty peer list on at
    least a fifth, an eligible-but-full S pinning m on at least a tenth, and a
    class above the leaf level whose take removes another class's candidates
    on at least a tenth."""
    n = len(swept)
    diff = refused = peer = pinned = cross = 0
    for p, s, k, peers, plain, tallies, (a, sp, cnt, st, fl) in swept:
        diff += int(not np.array_equal(a, plain))
        refused += int(st["refused"] > 0)
        peer += int(not np.array_equal(a, spread_ref(p, s, k, [], tallies)[0]))
        pinned += int(fl["pinned"])
        cross += int(fl["cross"])
    print(f"{n} cases: differ {diff}, refused {refused}, peers matter {peer}, pinned {pinned}, cross {cross}")
    assert 3 * diff >= n and 5 * refused >= n and 5 * peer >= n and 10 * pinned >= n and 10 * cross >= n


# ---- the host walk
def _walk(p, s, k, peers, tallies=None):
    """jspi_spread_walk_test on the yardstick's words and peer counts:
    (assign, spread, count, placed, refused, skew)."""
    lib = native.lib()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    fn = lib.jspi_spread_walk_test
    fn.restype = ctypes.c_int
    fn.argtypes = [u32, vp, vp, u32, vp, vp, vp, vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, vp, vp]
    cap, occ = tallies if tallies is not None else O.place_c(p)[1:]
    topo = p.topology
    K = topo.n_levels
    D = (u32 * 4)(*([topo.n_domains[q] for q in range(K)] + [0] * (4 - K)))
    fls = [np.ascontiguousarray(topo.first_leaf[q], dtype=np.uint32) for q in range(K)]
    flp = (vp * 4)(*([f.ctypes.data for f in fls] + [None] * (4 - K)))
    lv = np.array([c.level for c in p.classes], dtype=np.uint32)
    pods = np.array([c.pods for c in p.classes], dtype=np.uint32)
    feas = np.ascontiguousarray(np.concatenate([feas_words(p, cap, occ), np.zeros(1, dtype=np.uint64)]))
    fits = np.ascontiguousarray(np.concatenate([fits_words(p, cap), np.zeros(1, dtype=np.uint64)]))
    pr = np.ascontiguousarray(np.concatenate([peers_ref(p, s, peers), [0]]).astype(np.uint32))
    rc, rl = job_runs(p.job_class)
    rc, rl = np.ascontiguousarray(rc, dtype=np.uint32), np.ascontiguousarray(rl, dtype=np.uint32)
    Ds = topo.n_domains[s]
    out = np.full(p.n_jobs + 1, -7, dtype=np.int32)           # one spare element each, which must stay as it is
    sp = np.full(p.n_jobs + 1, -7, dtype=np.int32)
    cnt = np.full(Ds + 1, 0xABCD, dtype=np.uint32)
    ref, sk = u32(0), u32(0)
    placed = fn(K, D, flp, len(p.classes), lv.ctypes.data, pods.ctypes.data, feas.ctypes.data, fits.ctypes.data,
                pr.ctypes.data, s, k, rc.ctypes.data, rl.ctypes.data, len(rc), out.ctypes.data, sp.ctypes.data,
                cnt.ctypes.data, ctypes.addressof(ref), ctypes.addressof(sk))
    assert out[p.n_jobs] == -7 and sp[p.n_jobs] == -7 and cnt[Ds] == 0xABCD, "the walk wrote behind its outputs"
    return out[:p.n_jobs], sp[:p.n_jobs], cnt[:Ds], placed, ref.value, sk.value


def _same(got, want):
    a, sp, cnt, st, _ = want
    np.testing.assert_array_equal(got[0], a)
    np.testing.assert_array_equal(got[1], sp)
    np.testing.assert_array_equal(got[2], cnt)
    assert got[3:] == (st["placed"], st["refused"], st["skew"])


def test_host_walk_matches_the_reference(swept):
    for p, s, k, peers, plain, tallies, want in swept:
        _same(_walk(p, s, k, peers, tallies), want)
        for k2 in (SOFT, 1, 3):
            if k2 != k:
                _same(_walk(p, s, k2, [], tallies), spread_ref(p, s, k2, [], tallies))


@pytest.mark.parametrize("name", list(hand_cases()))
def test_host_walk_hand_cases(name):
    p, s, k, peers, want, want_s, want_n, want_refused = hand_cases()[name]
    a, sp, cnt, placed, refused, skew = _walk(p, s, k, peers)
    np.testing.assert_array_equal(a, want)
    np.testing.assert_array_equal(sp, want_s)
    np.testing.assert_array_equal(cnt, want_n)
    assert refused == want_refused


def test_host_walk_reductions():
    """The walk itself on the first two reductions' inputs."""
    for i in range(60):
        q = reduction_problem(i)
        p = rooted(q)
        if p is not None:
            plain, cap, occ = O.place_c(p)
            for k in (SOFT, 1):
                np.testing.assert_array_equal(_walk(p, 0, k, owners_of(p), (cap, occ))[0], plain)
        p = one_class(q)
        if p.n_jobs:
            plain, cap, occ = O.place_c(p)
            np.testing.assert_array_equal(_walk(p, p.classes[int(p.job_class[0])].level, 1, [], (cap, occ))[0], plain)
