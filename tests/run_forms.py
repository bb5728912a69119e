"""The forms a caller's run list takes, as data (DESIGN.md section 4.2b "Raw
run lists"): one job sequence written as canonical runs, as one run per job,
cut into fragments, padded with empty runs, with a gap of empty runs as long
as two of assign_block's tiles. A plain module, no engine, like
dispatch_cases.py: tests/test_run_forms.py feeds the forms to the host walks,
tests/test_run_forms_gpu.py to every placement path on the GPU.

The oracle and every tests/*_ref.py rule work per job, so all forms of one
job sequence have the same expected answer, bit for bit.

A form is (run_class, run_len, src), all uint32: src[i] is the index of the
canonical run that form run i comes from; an inserted empty run takes the src
of the next real run (at the tail: of the last real run), so a cut of the
canonical runs into gangs carries over to the form (regroup)."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from jobset_amd.snapshot import job_runs

WAVE_RUN_MAX = 64     # jsp_kernels.hip kWaveRunMax: the longest run wave 0 places alone
LEVEL_MAX_RUNS = 32   # jsp_internal.h kLevelMaxRuns: the level walker's LDS run table
ASSIGN_TILE = 1024    # assign_kernel's run tile (assign_block<kAssignThreads>)
FUSED_TILE = 256      # the fused tail's run tile (assign_block<kTallyThreads>)
GAP = 2100            # consecutive empty runs of the `gap` form: > 2 * ASSIGN_TILE

Form = Tuple[np.ndarray, np.ndarray, np.ndarray]


def _u32(*arrays) -> Tuple[np.ndarray, ...]:
    return tuple(np.ascontiguousarray(a, dtype=np.uint32) for a in arrays)


def _cut(form: Form, pieces) -> Form:
    """Every run of `form` cut into the fragment lengths pieces(run length)."""
    rc, rl, src = form
    oc, ol, os_ = [], [], []
    for c, n, s in zip(rc.tolist(), rl.tolist(), src.tolist()):
        for m in pieces(n):
            oc.append(c)
            ol.append(m)
            os_.append(s)
    return _u32(oc, ol, os_)


def _greedy(k: int):
    return lambda n: [k] * (n // k) + ([n % k] if n % k else [])


def _split_rand(form: Form, rng) -> Form:
    """Random cut points inside every run (fragments >= 1 job); some fragment
    has exactly one job whenever the form has a job."""
    rc, rl, _ = form
    forced = int(np.argmax(rl)) if rl.size and int(rl.max()) >= 1 else -1
    state = {"i": 0}

    def pieces(n):
        i = state["i"]
        state["i"] += 1
        if n <= 1:
            return [n]
        k = int(rng.integers(0, min(n - 1, 6) + 1))          # cuts
        cuts = set(rng.choice(np.arange(1, n), size=k, replace=False).tolist()) if k else set()
        if i == forced:
            cuts.add(1)                                      # a fragment of one job
        b = [0] + sorted(cuts) + [n]
        return [b[q + 1] - b[q] for q in range(len(b) - 1)]

    return _cut(form, pieces)


def _insert(form: Form, where: Dict[int, np.ndarray]) -> Form:
    """Empty runs of the classes where[i] in front of run i (i == n_runs: at the tail)."""
    rc, rl, src = form
    n = rc.shape[0]
    oc, ol, os_ = [], [], []
    for i in range(n + 1):
        for c in where.get(i, ()):
            oc.append(int(c))
            ol.append(0)
            os_.append(int(src[i]) if i < n else (int(src[-1]) if n else 0))
        if i < n:
            oc.append(int(rc[i]))
            ol.append(int(rl[i]))
            os_.append(int(src[i]))
    return _u32(oc, ol, os_)


def _padded(form: Form, n_classes: int, rng) -> Form:
    """Up to 2 empty runs before each run, at least one at the head and one at
    the tail; their classes uniform in [0, n_classes)."""
    n = form[0].shape[0]
    cnt = rng.integers(0, 3, size=n + 1)
    cnt[0] = max(int(cnt[0]), 1)
    cnt[n] = max(int(cnt[n]), 1) if n else cnt[n]
    if n == 0:
        cnt[0] = max(int(cnt[0]), 2)                         # head and tail
    return _insert(form, {i: rng.integers(0, n_classes, size=int(k)) for i, k in enumerate(cnt) if k})


def _pad_to(form: Form, total: int, n_classes: int, rng) -> Form:
    """Empty runs at random places until the list has `total` runs."""
    n = form[0].shape[0]
    at = rng.integers(0, n + 1, size=total - n)
    return _insert(form, {int(i): rng.integers(0, n_classes, size=int((at == i).sum())) for i in np.unique(at)})


def forms(job_class, n_classes: int, seed: int) -> Dict[str, Form]:
    """name -> (run_class, run_len, src) of every form of the job sequence
    job_class over classes [0, n_classes); deterministic in `seed`."""
    assert n_classes >= 1
    jc = np.ascontiguousarray(job_class, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    rc, rl = job_runs(jc)
    canon: Form = _u32(rc, rl, np.arange(rc.shape[0]))
    out: Dict[str, Form] = {"canonical": canon}
    out["ones"] = _cut(canon, lambda n: [1] * n)
    out["split_rand"] = _split_rand(canon, rng)
    out["split64"] = _cut(canon, _greedy(WAVE_RUN_MAX))
    out["split65"] = _cut(canon, _greedy(WAVE_RUN_MAX + 1))
    out["padded"] = _padded(canon, n_classes, rng)
    out["padded_split"] = _padded(out["split_rand"], n_classes, rng)
    n = rc.shape[0]
    out["gap"] = _insert(canon, {min(n // 2 + 1, n): rng.integers(0, n_classes, size=GAP)})
    if n <= LEVEL_MAX_RUNS:
        out["to32"] = _pad_to(canon, LEVEL_MAX_RUNS, n_classes, rng)
        out["to33"] = _pad_to(canon, LEVEL_MAX_RUNS + 1, n_classes, rng)
    if jc.shape[0] == 0:
        out["empties_only"] = _u32(rng.integers(0, n_classes, size=3), np.zeros(3), np.zeros(3))
    for name, (c, l, s) in out.items():
        assert c.shape == l.shape == s.shape and c.dtype == l.dtype == s.dtype == np.uint32, name
        np.testing.assert_array_equal(np.repeat(c, l), jc, err_msg=name)
    return out


def forms_of_runs(run_class, run_len, n_classes: int, seed: int) -> Dict[str, Form]:
    """forms() of the jobs of a run list that need not be canonical -- a gang
    call's, in which two adjacent runs of one class may stand on either side of
    a gang boundary -- with every fragment cut again at that list's run
    boundaries and src indexing ITS runs, so regroup carries its gangs over."""
    rc0, rl0 = _u32(run_class, run_len)
    assert np.all(rl0 > 0)
    jc = np.repeat(rc0, rl0)
    fs = forms(jc, n_classes, seed)
    if fs["canonical"][0].shape[0] == rc0.shape[0]:
        return fs
    bounds = np.cumsum(rl0.astype(np.int64))
    out: Dict[str, Form] = {}
    for name, (rc, rl, _) in fs.items():
        oc, ol, os_ = [], [], []
        j = 0
        for c, n in zip(rc.tolist(), rl.tolist()):
            if n == 0:  # an empty run: the run of the next job (at the tail: the last run)
                oc.append(c)
                ol.append(0)
                os_.append(min(int(np.searchsorted(bounds, j, side="right")), rc0.shape[0] - 1))
            while n > 0:
                k = int(np.searchsorted(bounds, j, side="right"))
                m = min(n, int(bounds[k]) - j)
                oc.append(c)
                ol.append(m)
                os_.append(k)
                j += m
                n -= m
        out[name] = _u32(oc, ol, os_)
        np.testing.assert_array_equal(np.repeat(out[name][0], out[name][1]), jc, err_msg=name)
    return out


def trimmed(form: Form, total: int) -> Form:
    """`form` without its last empty runs until at most `total` runs are left
    (the padded form for the level walker's 32 runs)."""
    rc, rl, src = form
    drop = max(rc.shape[0] - total, 0)
    empty = np.nonzero(rl == 0)[0]
    assert empty.shape[0] >= drop, "more real runs than the total asked for"
    keep = np.ones(rc.shape[0], dtype=bool)
    keep[empty[empty.shape[0] - drop:]] = False
    return rc[keep].copy(), rl[keep].copy(), src[keep].copy()


def regroup(gang_runs, src) -> np.ndarray:
    """The gang run counts of a form: gang g holds the canonical runs
    [sum(gang_runs[:g]), sum(gang_runs[:g + 1])); how many form runs have their
    src in each gang."""
    gr = np.asarray(gang_runs, dtype=np.int64)
    ends = np.cumsum(gr)
    src = np.asarray(src, dtype=np.int64)
    if gr.shape[0] == 0:
        assert src.shape[0] == 0
        return np.zeros(0, dtype=np.uint32)
    g = np.searchsorted(ends, src, side="right")
    # (a form of an empty batch carries src 0 with no canonical run: its runs join the last gang)
    g = np.minimum(g, gr.shape[0] - 1)
    return np.bincount(g, minlength=gr.shape[0]).astype(np.uint32)


def empty_tile(run_len, tile: int = ASSIGN_TILE) -> int:
    """The first k with run_len[tile k : tile (k + 1)] all zero (a whole tile), or -1."""
    rl = np.asarray(run_len)
    for k in range(rl.shape[0] // tile):
        if not rl[tile * k:tile * (k + 1)].any():
            return k
    return -1
