"""Both sides of every launch-shape threshold of jsp_place on the GPU
(tests/dispatch_cases.py; DESIGN.md section 4 "Launch-shape thresholds and
their tests"). Every side is placed through the host API and compared bit for
bit with the oracle -- assign[], the tallies and occupancy where the case asks
for them, placed, runs -- and Engine.last_plan() and stats.fused must equal
the plan the case names: a correct answer from another path fails.

Each pair runs a, b, a on the session engine (state carried across a shape
change: LDS plans, staging, the level walker's ready word, tickets), then a
one-row patch occupies the domain the last placed job took, and the answer
must follow the oracle's, which moves. Axes A-D (and E's launch-path pair) run
again through jsp_place_device with the device path's own plan asserted; axis
C also through jsp_tally_device + jsp_assign_device.
There is no tolerance anywhere."""
import functools

import numpy as np
import pytest

import dispatch_cases as DC
from jobset_amd.native import JSP_EHIP, JSP_ERANGE, JspError
from jobset_amd.snapshot import job_runs
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEEN = []     # every plan observed after a host-API placement
RAN = set()   # cases that ran


@functools.lru_cache(maxsize=2)
def solved(dims):
    p = DC.build(dims)
    return (p,) + tuple(O.place_c(p))


def check_answer(got, a, cap, occ, n_runs, tally):
    if tally:
        np.testing.assert_array_equal(got.occ, occ)
        np.testing.assert_array_equal(got.cap, cap)
    np.testing.assert_array_equal(got.assign, a)
    assert got.placed == int((a >= 0).sum())
    assert got.runs == n_runs


def check_plan(plan, want, what):
    bad = {k: (plan[k], v) for k, v in want.items() if plan[k] != v}
    assert not bad, f"{what}: (got, want) {bad} in {plan}"


def place(engine, rc, rl, dims, shape):
    got = engine.place_runs(rc, rl, want_tally=dims.tally)
    # the first call after an upload is answered on the launch path while the service comes up
    for _ in range(3):
        if shape not in (3, 5) or got.fused == shape:
            break
        got = engine.place_runs(rc, rl)
    return got


def run_side(engine, monkeypatch, case, i, device=False):
    side = case.sides[i]
    d = side.dims
    p, a, cap, occ = solved(d)
    if d.hooks:
        monkeypatch.setenv("JSP_TEST_HOOKS", d.hooks)  # read at the snapshot upload
    else:
        monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
    engine.set_fused(d.fused)
    engine.set_service(d.service)
    engine.load(p)
    rc, rl = job_runs(p.job_class)
    assert rc.shape[0] == d.runs or d.classes == 1
    what = f"{case.name}[{i}]"
    engine.timing(reset=True)
    got = place(engine, rc, rl, d, side.plan["shape"])
    # whichever path the case names answered at once: no service was tried and given up
    assert engine.timing(reset=False).svc_fallbacks == 0, what
    check_answer(got, a, cap, occ, rc.shape[0], d.tally)
    plan = engine.last_plan()
    SEEN.append(plan)
    assert got.fused == side.plan["shape"], what
    check_plan(plan, side.plan, what)
    if device:
        import torch
        rct, rlt = torch.from_numpy(rc.astype(np.int32)).cuda(), torch.from_numpy(rl.astype(np.int32)).cuda()
        out = torch.full((max(p.n_jobs, 1),), -7, dtype=torch.int32, device="cuda")
        engine.place_device(rct.data_ptr(), rlt.data_ptr(), rc.shape[0], p.n_jobs, out.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
        engine.check()
        np.testing.assert_array_equal(out.cpu().numpy()[:p.n_jobs], a)
        # (the side's own device plan where the device path, which never wants tallies, chooses otherwise)
        check_plan(engine.last_plan(), side.on_device, what + " device")
    return p, a


def run_case(engine, monkeypatch, case):
    RAN.add(case.name)
    try:
        order = (0, 1, 0) if len(case.sides) == 2 else (0, 0)
        for n, i in enumerate(order):
            p, base = run_side(engine, monkeypatch, case, i, device=case.device and n < len(case.sides))
        side = case.sides[order[-1]]
        # the domain of the last placed job becomes occupied (test_dispatch.py: the oracle's answer moves)
        row, q = DC.patched(p, base)
        engine.patch_rows(np.array([row], dtype=np.uint32), excl=np.array([DC.PATCH_OWNER], dtype=np.int32))
        a, cap, occ = O.place_c(q)
        assert not np.array_equal(a, base)
        rc, rl = job_runs(p.job_class)
        got = place(engine, rc, rl, side.dims, side.plan["shape"])
        check_answer(got, a, cap, occ, rc.shape[0], side.dims.tally)
        assert got.fused == side.plan["shape"]
    except JspError as err:
        # A launch the runtime refused on the host ("invalid argument": a shape
        # that does not fit) never reached the GPU: this case fails and the
        # others run. Any other JSP_EHIP -- a kernel fault, a wait that gave
        # up, a stream that failed -- leaves the GPU in doubt: nothing more
        # runs on it in this session.
        if err.code == JSP_EHIP and "invalid argument" not in str(err):
            pytest.exit(f"{case.name}: {err}", returncode=3)
        raise
    finally:
        monkeypatch.delenv("JSP_TEST_HOOKS", raising=False)
        engine.set_fused(True)
        engine.set_service(True)
        engine.service_stop()


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.name)
def test_threshold(engine, monkeypatch, case):
    run_case(engine, monkeypatch, case)


@pytest.mark.parametrize("name", ["C_min", "C_max"])
def test_jobs_threshold_tally_then_assign_device(engine, name):
    """Axis C through jsp_tally_device + jsp_assign_device: the walk on the
    host from 256 to 65,536 jobs, assign_kernel on either side. Each side
    starts behind a placement the split service answered: the tally alone
    then reports a plan of its own (no shape, no walker), not that service's."""
    import torch
    case = DC.case(name)
    try:
        for side in case.sides:
            d = side.dims
            p, a, cap, occ = solved(d)
            engine.set_fused(d.fused)
            engine.set_service(True)
            engine.load(p)
            rc, rl = job_runs(p.job_class)
            assert place(engine, rc, rl, DC.replace(d, tally=False), 5).fused == 5
            assert engine.last_plan()["walker"] == DC.SPLIT_HOST
            engine.set_service(False)
            C, L = len(p.classes), p.topology.n_leaves
            ld = L + 3
            dcap = torch.full((C + 1, ld), 77, dtype=torch.int32, device="cuda")
            rct, rlt = torch.from_numpy(rc.astype(np.int32)).cuda(), torch.from_numpy(rl.astype(np.int32)).cuda()
            out = torch.full((p.n_jobs,), -7, dtype=torch.int32, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            engine.tally_device(dcap.data_ptr(), dcap[-1].data_ptr(), ld, s)
            check_plan(engine.last_plan(), dict(shape=0, walker=DC.WALK_NONE, tally=DC.WAVE_ONE, tally_passes=1, folded=0,
                                                level_threads=0, stage_cap=0, groups=1), f"{name} tally alone")
            engine.assign_device(dcap.data_ptr(), dcap[-1].data_ptr(), ld, rct.data_ptr(), rlt.data_ptr(), rc.shape[0],
                                 p.n_jobs, out.data_ptr(), s)
            engine.check()
            host = 256 <= d.jobs <= 65536
            check_plan(engine.last_plan(), dict(shape=7 if host else 0, walker=DC.HOST if host else DC.ASSIGN,
                                                tally=DC.WAVE_ONE, tally_passes=1, folded=0), f"{name} J={d.jobs}")
            tal = dcap.cpu().numpy().astype(np.uint32)
            np.testing.assert_array_equal(tal[:C, :L], cap)
            np.testing.assert_array_equal(tal[C, :L], occ)
            np.testing.assert_array_equal(out.cpu().numpy(), a)
    finally:
        engine.set_fused(True)
        engine.set_service(True)
        engine.service_stop()


def test_one_word_past_the_taken_limit_is_refused(engine, monkeypatch):
    """kMaxTakenWords + 1 words over three levels: JSP_ERANGE at the topology
    upload, and the engine places the next snapshot as before."""
    with pytest.raises(JspError) as ei:
        engine.upload_topology(DC.topology(DC.G_OVER))
    assert ei.value.code == JSP_ERANGE
    run_case(engine, monkeypatch, DC.case("F_tile64"))


def test_every_path_was_taken(engine, monkeypatch):
    """The plans seen above cover every kernel path the thresholds choose
    between, so taking a case out cannot silently drop one. (Cases that a
    test selection left out run here first.)"""
    for case in DC.CASES:
        if case.name not in RAN:
            run_case(engine, monkeypatch, case)
    level = {(p["level_wpt"], p["level_threads"]) for p in SEEN if p["walker"] == DC.LEVEL}
    assert level >= {(1, 256), (1, 1024), (2, 1024)}, level
    assert {p["feas_in_lds"] for p in SEEN if p["walker"] == DC.ASSIGN} == {0, 1}
    assert {p["tally_passes"] for p in SEEN if p["tally"] != DC.IN_TILE} >= {1, 2, 3, 4}
    assert {p["tally"] for p in SEEN} >= {DC.WAVE_ONE, DC.WAVE_DB, DC.BLOCK}
    assert {p["groups"] for p in SEEN if p["walker"] in (DC.FUSED_TAIL, DC.SPLIT_HOST)} >= {1, 2, 3, 4}
    assert {p["shape"] for p in SEEN} >= DC.REQUIRED_SHAPES
