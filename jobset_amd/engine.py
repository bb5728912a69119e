"""Python host mirror of the engine interface the Go `pkg/placement` package
exposes: `Engine.place(problem) -> assign[]`.

In the reference the domain for each child Job is chosen by kube-scheduler
from the leader's exclusive affinity terms (pkg/webhooks/
pod_mutating_webhook.go:95-135); this engine computes it deterministically for
all Jobs of a JobSet at once, at first admission and at full recreate
(pkg/controllers/failure_policy.go:155-175). Every call goes through the C ABI
of include/jsplace.h into the gfx950 kernels; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import native
from .native import (JspAssumeStats, JspBindStats, JspClassExplain, JspFitStats, JspGangStats, JspJobClass, JspNodes,
                     JspPreemptStats, JspSpreadStats, JspStats, JspStickyStats, JspTiming, JspTopology, JspWhatifStats,
                     check)
from .snapshot import JobClass, Nodes, Problem, Topology, job_runs


def _p(a: Optional[np.ndarray]) -> Optional[int]:
    return None if a is None else a.ctypes.data


@dataclass
class PlaceResult:
    assign: np.ndarray           # int32 [J], domain id at the job's class level, -1 unplaceable
    cap: Optional[np.ndarray]    # uint32 [C, L] per-(class, leaf) pod capacity
    occ: Optional[np.ndarray]    # uint32 [L] rows covered by other exclusive jobs
    placed: int
    runs: int
    wall_us: float
    jobs: int = 0                # J as the library counted it (jsp_stats.jobs)
    fused: int = 0               # launch shape: 0 three launches, 1 fused tail, 2 one-class compaction, 3/4 the resident service (compaction / fused), 5 the split service (host walk)


class Engine:
    """One engine per GPU (device id = local rank), or -- with `devices`, a
    list of device ids (repeats allowed) -- one device-set engine over several
    shards (jsp_engine_create_multi)."""

    def __init__(self, device: int = 0, devices: Optional[Sequence[int]] = None):
        self._lib = native.lib()
        h = ctypes.c_void_p()
        if devices is not None:
            ids = (ctypes.c_int * len(devices))(*devices)
            check(self._lib.jsp_engine_create_multi(ids, len(devices), ctypes.byref(h)))
            device = int(devices[0]) if len(devices) else 0
        else:
            check(self._lib.jsp_engine_create(device, ctypes.byref(h)))
        self._h = h
        self.device = device
        self._keep: List[object] = []
        self.topology: Optional[Topology] = None
        self.nodes: Optional[Nodes] = None
        self.n_classes = 0
        self._class_pods = np.zeros(0, dtype=np.int64)  # pods per uploaded class (bind_pods sizes its output)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.jsp_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---------------------------------------------------------------- snapshot
    def upload_topology(self, topo: Topology) -> None:
        t = JspTopology()
        t.n_levels = topo.n_levels
        keep = []
        for k in range(topo.n_levels):
            t.n_domains[k] = topo.n_domains[k]
            fl = np.ascontiguousarray(topo.first_leaf[k], dtype=np.uint32)
            keep.append(fl)
            t.first_leaf[k] = fl.ctypes.data
        check(self._lib.jsp_topology_upload(self._h, ctypes.byref(t)))
        self.topology = topo
        self.nodes = None
        self.n_classes = 0

    def upload_snapshot(self, nodes: Nodes) -> None:
        cols = dict(
            leaf_start=np.ascontiguousarray(nodes.leaf_start, dtype=np.uint32),
            labels=np.ascontiguousarray(nodes.labels, dtype=np.uint64),
            taints=np.ascontiguousarray(nodes.taints, dtype=np.uint32),
            free=np.ascontiguousarray(nodes.free, dtype=np.uint32),
            excl=np.ascontiguousarray(nodes.excl, dtype=np.int32),
        )
        n = JspNodes()
        n.n_nodes = nodes.n_nodes
        n.leaf_begin = nodes.leaf_begin
        n.n_leaves = nodes.n_leaves
        n.leaf_start = _p(cols["leaf_start"])
        n.n_label_words = cols["labels"].shape[0]
        n.labels = _p(cols["labels"])
        n.taints = _p(cols["taints"])
        n.n_res = cols["free"].shape[0]
        n.free_res = _p(cols["free"])
        n.excl_owner = _p(cols["excl"])
        check(self._lib.jsp_snapshot_upload(self._h, ctypes.byref(n)))
        self.nodes = nodes

    def patch_rows(self, rows: np.ndarray, labels: Optional[np.ndarray] = None, taints: Optional[np.ndarray] = None,
                   free: Optional[np.ndarray] = None, excl: Optional[np.ndarray] = None) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=dt)
                for a, dt in ((labels, np.uint64), (taints, np.uint32), (free, np.uint32), (excl, np.int32))]
        check(self._lib.jsp_snapshot_patch(self._h, _p(rows), rows.shape[0], *[_p(a) for a in arrs]))

    def upload_classes(self, classes: Sequence[JobClass]) -> None:
        arr = (JspJobClass * max(len(classes), 1))()
        for i, jc in enumerate(classes):
            req, fb = jc.words(4)
            for w in range(4):
                arr[i].req_labels[w] = req[w] & ((1 << 64) - 1)
                arr[i].forbid_labels[w] = fb[w] & ((1 << 64) - 1)
            arr[i].tolerated_taints = jc.tolerated_taints & 0xFFFFFFFF
            arr[i].level = jc.level
            arr[i].pods = jc.pods
            for r, v in enumerate(jc.res()):
                arr[i].req_res[r] = v
        check(self._lib.jsp_classes_upload(self._h, arr, len(classes)))
        self.n_classes = len(classes)
        self._class_pods = np.array([jc.pods for jc in classes], dtype=np.int64)
        self._class_level = [int(jc.level) for jc in classes]

    def load(self, p: Problem, nodes: Optional[Nodes] = None) -> None:
        self.upload_topology(p.topology)
        self.upload_snapshot(nodes if nodes is not None else p.nodes)
        self.upload_classes(p.classes)

    # ---------------------------------------------------------------- placement
    def place_runs(self, run_class: np.ndarray, run_len: np.ndarray, want_tally: bool = False) -> PlaceResult:
        """Jobs as replicated-job runs in global order: run i = run_len[i] jobs of
        class run_class[i] (a ReplicatedJob's replicas share one template)."""
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        J = int(rl.astype(np.int64).sum())
        L = self.topology.n_leaves if self.topology is not None else 0
        assign = np.empty(max(J, 1), dtype=np.int32)
        cap = np.empty((max(self.n_classes, 1), max(L, 1)), dtype=np.uint32) if want_tally else None
        occ = np.empty(max(L, 1), dtype=np.uint32) if want_tally else None
        st = JspStats()
        check(self._lib.jsp_place(self._h, _p(rc), _p(rl), rc.shape[0], _p(assign), _p(cap), _p(occ),
                                  ctypes.byref(st)))
        return PlaceResult(assign=assign[:J], cap=None if cap is None else cap[:self.n_classes, :L],
                           occ=None if occ is None else occ[:L], placed=st.placed, runs=st.runs,
                           wall_us=st.wall_us, jobs=int(st.jobs), fused=int(st.fused))

    def place(self, job_class: np.ndarray, want_tally: bool = False) -> PlaceResult:
        """One class id per job (global order); run-length encoded in the library."""
        jc = np.ascontiguousarray(job_class, dtype=np.uint32)
        J = jc.shape[0]
        L = self.topology.n_leaves if self.topology is not None else 0
        assign = np.empty(max(J, 1), dtype=np.int32)
        cap = np.empty((max(self.n_classes, 1), max(L, 1)), dtype=np.uint32) if want_tally else None
        occ = np.empty(max(L, 1), dtype=np.uint32) if want_tally else None
        st = JspStats()
        check(self._lib.jsp_place_jobs(self._h, _p(jc), J, _p(assign), _p(cap), _p(occ), ctypes.byref(st)))
        return PlaceResult(assign=assign[:J], cap=None if cap is None else cap[:self.n_classes, :L],
                           occ=None if occ is None else occ[:L], placed=st.placed, runs=st.runs,
                           wall_us=st.wall_us, jobs=int(st.jobs), fused=int(st.fused))

    # ---------------------------------------------------------------- sticky placement (jsp_place_sticky)
    def place_sticky_runs(self, run_class: np.ndarray, run_len: np.ndarray,
                          prev: Optional[np.ndarray]) -> Tuple[np.ndarray, JspStickyStats]:
        """jsp_place_sticky: the runs of place_runs plus prev[J], each job's
        previous domain at its class's level or -1 (None: no hints). A job
        whose previous domain is still feasible, and which no lower-indexed
        claimant of an intersecting domain outranks, keeps it; the others are
        placed lowest-index around the kept ones. Returns the
        assignment and the stats (jsplace.h jsp_sticky_stats)."""
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        J = int(rl.astype(np.int64).sum())
        pv = None if prev is None else np.ascontiguousarray(prev, dtype=np.int32)
        if pv is not None and pv.shape[0] != J:
            raise ValueError(f"prev has {pv.shape[0]} entries for {J} jobs")
        assign = np.empty(max(J, 1), dtype=np.int32)
        st = JspStickyStats()
        check(self._lib.jsp_place_sticky(self._h, _p(rc), _p(rl), rc.shape[0], _p(pv), _p(assign), ctypes.byref(st)))
        return assign[:J], st

    def place_sticky(self, job_class: np.ndarray, prev: Optional[np.ndarray]) -> Tuple[np.ndarray, JspStickyStats]:
        """place_sticky_runs with one class id per job (global order)."""
        rc, rl = job_runs(job_class)
        return self.place_sticky_runs(rc, rl, prev)

    def place_sticky_loop(self, run_class: np.ndarray, run_len: np.ndarray, prev: Optional[np.ndarray],
                          iters: int = 200) -> Tuple[float, float, float]:
        """`iters` jsp_place_sticky calls back to back timed in C
        (jspb_place_sticky_loop): total, median and p99 per call, microseconds."""
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        J = int(rl.astype(np.int64).sum())
        pv = None if prev is None else np.ascontiguousarray(prev, dtype=np.int32)
        assign = np.empty(max(J, 1), dtype=np.int32)
        out = np.zeros(3, dtype=np.float64)
        check(self._lib.jspb_place_sticky_loop(self._h, _p(rc), _p(rl), rc.shape[0], _p(pv), _p(assign), int(iters),
                                               _p(out)))
        return float(out[0]), float(out[1]), float(out[2])

    # ---------------------------------------------------------------- gang placement (jsp_place_gangs)
    @staticmethod
    def _gang_buffers(run_class, run_len, gang_runs, gang_span):
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        gr = np.ascontiguousarray(gang_runs, dtype=np.uint32)
        gs = np.ascontiguousarray(np.asarray(gang_span, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32)
        if gr.shape[0] != gs.shape[0]:
            raise ValueError(f"gang_runs has {gr.shape[0]} and gang_span {gs.shape[0]} entries")
        J = int(rl.astype(np.int64).sum())
        # the library refuses J above its limit before it writes anything
        assign = np.empty(max(min(J, native.JSP_GANG_MAX_JOBS), 1), dtype=np.int32)
        span = np.empty(max(gr.shape[0], 1), dtype=np.int32)
        return rc, rl, gr, gs, J, assign, span

    def place_gangs_runs(self, run_class: np.ndarray, run_len: np.ndarray, gang_runs: np.ndarray,
                         gang_span: np.ndarray, flags: int = 0) -> Tuple[np.ndarray, np.ndarray, JspGangStats]:
        """jsp_place_gangs: the runs of place_runs cut into gangs -- gang g is
        the next gang_runs[g] runs -- each placed whole inside one domain of
        level gang_span[g] (native.JSP_SPAN_ANY or -1: the whole cluster), or
        not at all (DESIGN.md §2 "Gang placement"). Returns (assign [J],
        gang_span_out [G]: the span domain, 0 for JSP_SPAN_ANY, -1 refused,
        stats)."""
        rc, rl, gr, gs, J, assign, span = self._gang_buffers(run_class, run_len, gang_runs, gang_span)
        st = JspGangStats()
        check(self._lib.jsp_place_gangs(self._h, _p(rc), _p(rl), rc.shape[0], _p(gr), _p(gs), gr.shape[0], int(flags),
                                        _p(assign), _p(span), ctypes.byref(st)))
        return assign[:J], span[:gr.shape[0]], st

    def place_gangs(self, job_class: np.ndarray, gang_of_job: np.ndarray,
                    gang_span: np.ndarray) -> Tuple[np.ndarray, np.ndarray, JspGangStats]:
        """place_gangs_runs with one class id and one gang id per job (global
        order): gang ids are nondecreasing from 0, gang g's span level is
        gang_span[g]; a gang id no job carries is an empty gang."""
        jc = np.ascontiguousarray(job_class, dtype=np.uint32)
        gj = np.asarray(gang_of_job, dtype=np.int64)
        G = len(gang_span)
        if gj.shape[0] != jc.shape[0]:
            raise ValueError(f"gang_of_job has {gj.shape[0]} entries for {jc.shape[0]} jobs")
        if gj.size and (np.any(np.diff(gj) < 0) or gj[0] < 0 or gj[-1] >= G):
            raise ValueError("gang_of_job must be nondecreasing within [0, len(gang_span))")
        # runs: maximal stretches of one class inside one gang
        if jc.size:
            cut = np.nonzero((np.diff(jc.astype(np.int64)) != 0) | (np.diff(gj) != 0))[0] + 1
            start = np.concatenate([[0], cut])
            rc = jc[start]
            rl = np.diff(np.concatenate([start, [jc.shape[0]]])).astype(np.uint32)
            gr = np.bincount(gj[start], minlength=G).astype(np.uint32)
        else:
            rc, rl, gr = jc, jc, np.zeros(G, dtype=np.uint32)
        return self.place_gangs_runs(rc, rl, gr, gang_span)

    def place_gangs_loop(self, run_class: np.ndarray, run_len: np.ndarray, gang_runs: np.ndarray,
                         gang_span: np.ndarray, iters: int = 200) -> Tuple[float, float, float]:
        """`iters` jsp_place_gangs calls back to back timed in C
        (jspb_place_gangs_loop): total, median and p99 per call, microseconds."""
        rc, rl, gr, gs, J, assign, span = self._gang_buffers(run_class, run_len, gang_runs, gang_span)
        out = np.zeros(3, dtype=np.float64)
        check(self._lib.jspb_place_gangs_loop(self._h, _p(rc), _p(rl), rc.shape[0], _p(gr), _p(gs), gr.shape[0],
                                              _p(assign), _p(span), int(iters), _p(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def span_counts(self, n_cnt: int, form: int = 0, iters: int = 0) -> Tuple[np.ndarray, Tuple[float, float]]:
        """jspb_span_counts: the gang walk's prefilter counts on the current
        snapshot (layout: jsplace_bench.h), n_cnt of them; form 0 as
        jsp_place_gangs launches them, 1 / 2 the thread / the wave form
        everywhere. With iters, (median, mean) device us of the count launches."""
        cnt = np.zeros(max(int(n_cnt), 1), dtype=np.uint32)
        out = np.zeros(2, dtype=np.float64)
        check(self._lib.jspb_span_counts(self._h, int(form), _p(cnt), int(n_cnt), int(iters), _p(out)))
        return cnt[:int(n_cnt)], (float(out[0]), float(out[1]))

    # ---------------------------------------------------------------- fit placement (jsp_place_fit)
    @staticmethod
    def _fit_buffers(run_class, run_len):
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        J = int(rl.astype(np.int64).sum())
        # the library refuses J above its limit before it writes anything
        return rc, rl, J, np.empty(max(min(J, native.JSP_FIT_MAX_JOBS), 1), dtype=np.int32)

    def place_fit_runs(self, run_class: np.ndarray, run_len: np.ndarray, policy: int,
                       flags: int = 0) -> Tuple[np.ndarray, JspFitStats]:
        """jsp_place_fit: the runs of place_runs; every job takes, among the
        feasible domains of its class's level not yet taken, the one with the
        smallest (key, id) under `policy` -- native.JSP_FIT_LOWEST (place's
        answer), JSP_FIT_TIGHTEST (the least clamped pod capacity that still
        fits) or JSP_FIT_ROOMIEST (the most) (DESIGN.md §2 "Fit placement").
        Returns (assign [J], stats: jsplace.h jsp_fit_stats)."""
        rc, rl, J, assign = self._fit_buffers(run_class, run_len)
        st = JspFitStats()
        check(self._lib.jsp_place_fit(self._h, _p(rc), _p(rl), rc.shape[0], int(policy), int(flags), _p(assign),
                                      ctypes.byref(st)))
        return assign[:J], st

    def place_fit(self, job_class: np.ndarray, policy: int) -> Tuple[np.ndarray, JspFitStats]:
        """place_fit_runs with one class id per job (global order)."""
        rc, rl = job_runs(job_class)
        return self.place_fit_runs(rc, rl, policy)

    def place_fit_loop(self, run_class: np.ndarray, run_len: np.ndarray, policy: int,
                       iters: int = 200) -> Tuple[float, float, float]:
        """`iters` jsp_place_fit calls back to back timed in C
        (jspb_place_fit_loop): total, median and p99 per call, microseconds."""
        rc, rl, J, assign = self._fit_buffers(run_class, run_len)
        out = np.zeros(3, dtype=np.float64)
        check(self._lib.jspb_place_fit_loop(self._h, _p(rc), _p(rl), rc.shape[0], int(policy), _p(assign), int(iters),
                                            _p(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def fit_order(self, policy: int, form: int = 0,
                  iters: int = 0) -> Tuple[np.ndarray, np.ndarray, Tuple[float, float]]:
        """jspb_fit_order: the fit walk's candidate lists on the current
        snapshot (layout: jsplace_bench.h) and the feasible count per class;
        form 0 as jsp_place_fit orders them, 1 / 2 the rank / the block form
        everywhere. With iters, (median, mean) device us of the order launches."""
        n = sum(int(self.topology.n_domains[k]) for k in self._class_level)
        order = np.zeros(max(n, 1), dtype=np.uint32)
        nf = np.zeros(max(self.n_classes, 1), dtype=np.uint32)
        out = np.zeros(2, dtype=np.float64)
        check(self._lib.jspb_fit_order(self._h, int(policy), int(form), _p(order), n, _p(nf), int(iters), _p(out)))
        return order[:n], nf[:self.n_classes], (float(out[0]), float(out[1]))

    # ---------------------------------------------------------------- what-if placement (jsp_place_whatif)
    @staticmethod
    def _whatif_buffers(run_class, run_len, scen_off, rows, labels, taints, free_res, excl_owner):
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        so = np.ascontiguousarray(scen_off, dtype=np.uint32)
        rw = np.ascontiguousarray(rows, dtype=np.uint32)
        cols = [None if a is None else np.ascontiguousarray(a, dtype=dt)
                for a, dt in ((labels, np.uint64), (taints, np.uint32), (free_res, np.uint32), (excl_owner, np.int32))]
        J = int(rl.astype(np.int64).sum())
        S = max(so.shape[0] - 1, 0)
        # the library refuses J and S above its limits before it writes anything
        assign = np.empty((max(min(S, native.JSP_WHATIF_MAX_SCENARIOS), 1),
                           max(min(J, native.JSP_WHATIF_MAX_JOBS), 1)), dtype=np.int32)
        return rc, rl, so, rw, cols, J, S, assign

    def place_whatif_runs(self, run_class: np.ndarray, run_len: np.ndarray, scen_off: np.ndarray, rows: np.ndarray,
                          labels: Optional[np.ndarray] = None, taints: Optional[np.ndarray] = None,
                          free_res: Optional[np.ndarray] = None, excl_owner: Optional[np.ndarray] = None,
                          flags: int = 0) -> Tuple[np.ndarray, np.ndarray, JspWhatifStats]:
        """jsp_place_whatif: the runs of place_runs placed under S hypothetical
        row edits, none of which is written. Scenario s is the rows
        rows[scen_off[s]:scen_off[s + 1]] (strictly ascending) with its slice
        of the delta columns, laid out as patch_rows' over all the rows
        (labels [W, n], free_res [R, n]); None keeps the resident column
        (DESIGN.md §2 "What-if placement"). Returns (assign [S, J]: what place
        would answer on the snapshot patched with scenario s, placed [S],
        stats: jsplace.h jsp_whatif_stats)."""
        rc, rl, so, rw, cols, J, S, assign = self._whatif_buffers(run_class, run_len, scen_off, rows, labels, taints,
                                                                  free_res, excl_owner)
        placed = np.zeros(max(S, 1), dtype=np.uint32)
        st = JspWhatifStats()
        check(self._lib.jsp_place_whatif(self._h, _p(rc), _p(rl), rc.shape[0], _p(so) if so.shape[0] else None, S,
                                         _p(rw) if rw.shape[0] else None, *[_p(a) for a in cols], int(flags),
                                         _p(assign.reshape(-1)[:max(S * J, 1)]), _p(placed), ctypes.byref(st)))
        return assign.reshape(-1)[:S * J].reshape(S, J), placed[:S], st

    def place_whatif(self, job_class: np.ndarray,
                     scenarios: Sequence[dict]) -> Tuple[np.ndarray, np.ndarray, JspWhatifStats]:
        """place_whatif_runs with one class id per job (global order) and one
        dict per scenario: {"rows": [n_s], and any of "labels" [W, n_s],
        "taints" [n_s], "free_res" [R, n_s], "excl_owner" [n_s]}. A column is
        either in every scenario that has rows or in none."""
        rc, rl = job_runs(job_class)
        rows = [np.asarray(sc.get("rows", ()), dtype=np.uint32).reshape(-1) for sc in scenarios]
        so = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.uint32)
        cols = {}
        for name, axis in (("labels", 1), ("taints", 0), ("free_res", 1), ("excl_owner", 0)):
            parts = [np.asarray(sc[name]) for sc, r in zip(scenarios, rows) if r.shape[0] and sc.get(name) is not None]
            have = sum(1 for r in rows if r.shape[0])
            if parts and len(parts) != have:
                raise ValueError(f"column {name!r} is in {len(parts)} of the {have} scenarios that have rows")
            cols[name] = np.concatenate(parts, axis=axis) if parts else None
        allrows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint32)
        return self.place_whatif_runs(rc, rl, so, allrows, cols["labels"], cols["taints"], cols["free_res"],
                                      cols["excl_owner"])

    def place_whatif_loop(self, run_class: np.ndarray, run_len: np.ndarray, scen_off: np.ndarray, rows: np.ndarray,
                          labels: Optional[np.ndarray] = None, taints: Optional[np.ndarray] = None,
                          free_res: Optional[np.ndarray] = None, excl_owner: Optional[np.ndarray] = None,
                          iters: int = 200) -> Tuple[float, float, float]:
        """`iters` jsp_place_whatif calls back to back timed in C
        (jspb_place_whatif_loop): total, median and p99 per call, microseconds."""
        rc, rl, so, rw, cols, J, S, assign = self._whatif_buffers(run_class, run_len, scen_off, rows, labels, taints,
                                                                  free_res, excl_owner)
        out = np.zeros(3, dtype=np.float64)
        check(self._lib.jspb_place_whatif_loop(self._h, _p(rc), _p(rl), rc.shape[0], _p(so) if so.shape[0] else None, S,
                                               _p(rw) if rw.shape[0] else None, *[_p(a) for a in cols], _p(assign),
                                               int(iters), _p(out)))
        return float(out[0]), float(out[1]), float(out[2])

    # ---------------------------------------------------------------- preemptive placement (jsp_place_preempt)
    @staticmethod
    def _preempt_buffers(run_class, run_len, owners, owner_prio, evict_free):
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        ow = np.ascontiguousarray(owners, dtype=np.int32).reshape(-1)
        op = np.ascontiguousarray(owner_prio, dtype=np.uint32).reshape(-1)
        if ow.shape != op.shape:
            raise ValueError(f"{ow.shape[0]} owners with {op.shape[0]} ranks")
        ef = None if evict_free is None else np.ascontiguousarray(evict_free, dtype=np.uint32)
        J = int(rl.astype(np.int64).sum())
        # the library refuses J above its limit before it writes anything
        Jb = max(min(J, native.JSP_PREEMPT_MAX_JOBS), 1)
        return rc, rl, ow, op, ef, J, np.empty(Jb, dtype=np.int32), np.zeros(Jb + 1, dtype=np.uint32)

    def _snapshot_rows(self) -> int:
        return int(self.nodes.n_nodes) if self.nodes is not None else 0

    def _check_evict_free(self, ef):
        """evict_free must hold the snapshot's [R, N] values: the library reads them all."""
        if ef is not None and self.nodes is not None and ef.size != self.nodes.n_res * self.nodes.n_nodes:
            raise ValueError(f"evict_free has {ef.size} values, the snapshot [R, N] = "
                             f"[{self.nodes.n_res}, {self.nodes.n_nodes}]")

    def place_preempt_runs(self, run_class: np.ndarray, run_len: np.ndarray, prio: int, owners: np.ndarray,
                           owner_prio: np.ndarray, evict_free: Optional[np.ndarray] = None, flags: int = 0,
                           victims_cap: Optional[int] = None, want_victims: bool = True
                           ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, JspPreemptStats]:
        """jsp_place_preempt: the runs of place_runs placed at priority rank
        `prio`; a domain whose owned rows all belong to owners of the table
        (owners [n] int32 ids, owner_prio [n] ranks) with a rank below prio is
        reachable when it has room with evict_free [R, N] on those rows (None:
        the resident free column), and every job takes the reachable domain
        with the smallest (highest victim rank, owner segments, id) (DESIGN.md
        §2 "Preemptive placement"). Nothing is written. victims_cap: the room
        of the victim list (default: the snapshot's rows, which always
        suffices); want_victims=False passes no list. Returns (assign [J],
        victim_off [J + 1], victims [victim_off[J]], stats: jsplace.h
        jsp_preempt_stats)."""
        rc, rl, ow, op, ef, J, assign, off = self._preempt_buffers(run_class, run_len, owners, owner_prio, evict_free)
        self._check_evict_free(ef)
        cap = int(self._snapshot_rows() if victims_cap is None else victims_cap)
        vic = np.zeros(max(cap, 1), dtype=np.int32) if want_victims else None
        st = JspPreemptStats()
        check(self._lib.jsp_place_preempt(self._h, _p(rc), _p(rl), rc.shape[0], int(prio), _p(ow) if ow.shape[0] else None,
                                          _p(op) if op.shape[0] else None, ow.shape[0], _p(ef), int(flags), _p(assign),
                                          _p(off), _p(vic), cap, ctypes.byref(st)))
        n = int(off[J]) if J else 0
        return assign[:J], off[:J + 1], (vic[:n] if want_victims else np.zeros(0, dtype=np.int32)), st

    def place_preempt(self, job_class: np.ndarray, prio: int, owners: np.ndarray, owner_prio: np.ndarray,
                      evict_free: Optional[np.ndarray] = None
                      ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, JspPreemptStats]:
        """place_preempt_runs with one class id per job (global order)."""
        rc, rl = job_runs(job_class)
        return self.place_preempt_runs(rc, rl, prio, owners, owner_prio, evict_free)

    def place_preempt_loop(self, run_class: np.ndarray, run_len: np.ndarray, prio: int, owners: np.ndarray,
                           owner_prio: np.ndarray, evict_free: Optional[np.ndarray] = None,
                           iters: int = 200) -> Tuple[float, float, float]:
        """`iters` jsp_place_preempt calls back to back timed in C
        (jspb_place_preempt_loop): total, median and p99 per call, microseconds."""
        rc, rl, ow, op, ef, J, assign, off = self._preempt_buffers(run_class, run_len, owners, owner_prio, evict_free)
        self._check_evict_free(ef)
        vic = np.zeros(max(self._snapshot_rows(), 1), dtype=np.int32)
        out = np.zeros(3, dtype=np.float64)
        check(self._lib.jspb_place_preempt_loop(self._h, _p(rc), _p(rl), rc.shape[0], int(prio),
                                                _p(ow) if ow.shape[0] else None, _p(op) if op.shape[0] else None,
                                                ow.shape[0], _p(ef), _p(assign), _p(off), _p(vic), self._snapshot_rows(), None,
                                                int(iters), _p(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def preempt_order(self, prio: int, owners: np.ndarray, owner_prio: np.ndarray,
                      evict_free: Optional[np.ndarray] = None, form: int = 0, iters: int = 0
                      ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, Tuple[float, float]]:
        """jspb_preempt_order: the preempt walk's candidate lists on the
        current snapshot (layout: jsplace_bench.h), the reachable count per
        class, and key(c, d) and seg(d) by domain id; form as fit_order's.
        With iters, (median, mean) device us of the launches."""
        ow = np.ascontiguousarray(owners, dtype=np.int32).reshape(-1)
        op = np.ascontiguousarray(owner_prio, dtype=np.uint32).reshape(-1)
        if ow.shape != op.shape:
            raise ValueError(f"{ow.shape[0]} owners with {op.shape[0]} ranks")
        ef = None if evict_free is None else np.ascontiguousarray(evict_free, dtype=np.uint32)
        self._check_evict_free(ef)
        n = sum(int(self.topology.n_domains[k]) for k in self._class_level)
        order, key, seg = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        nf = np.zeros(max(self.n_classes, 1), dtype=np.uint32)
        out = np.zeros(2, dtype=np.float64)
        check(self._lib.jspb_preempt_order(self._h, int(prio), _p(ow) if ow.shape[0] else None,
                                           _p(op) if op.shape[0] else None, ow.shape[0], _p(ef), int(form), _p(order), n,
                                           _p(nf), _p(key), _p(seg), int(iters), _p(out)))
        return order[:n], nf[:self.n_classes], key[:n], seg[:n], (float(out[0]), float(out[1]))

    # ---------------------------------------------------------------- spread placement (jsp_place_spread)
    def _spread_buffers(self, run_class, run_len, spread_level, peers):
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        pe = np.ascontiguousarray(peers if peers is not None else [], dtype=np.int32).reshape(-1)
        J = int(rl.astype(np.int64).sum())
        # the library refuses J above its limit before it writes anything
        Jb = max(min(J, native.JSP_SPREAD_MAX_JOBS), 1)
        lv = int(spread_level)
        Ds = int(self.topology.n_domains[lv]) if self.topology is not None and 0 <= lv < self.topology.n_levels else 0
        return (rc, rl, pe, J, Ds, np.empty(Jb, dtype=np.int32), np.empty(Jb, dtype=np.int32),
                np.zeros(max(Ds, 1), dtype=np.uint32))

    def place_spread_runs(self, run_class: np.ndarray, run_len: np.ndarray, spread_level: int, max_skew: int,
                          peers: Optional[np.ndarray] = None, flags: int = 0
                          ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, JspSpreadStats]:
        """jsp_place_spread: the runs of place_runs spread evenly over the
        domains of `spread_level` (DESIGN.md §2 "Spread placement"): every job
        goes to the level's domain S with the fewest jobs so far (peers: the
        excl_owner ids that count as already placed), lowest id first, that
        holds a free feasible domain of its class and, with max_skew >= 1,
        keeps n[S] + 1 - min n within max_skew (native.JSP_SPREAD_SOFT: no
        test). Returns (assign [J], spread [J]: the level's domain per job or
        -1, count [D_s]: the final jobs per domain, stats: jsplace.h
        jsp_spread_stats)."""
        rc, rl, pe, J, Ds, assign, spread, count = self._spread_buffers(run_class, run_len, spread_level, peers)
        st = JspSpreadStats()
        check(self._lib.jsp_place_spread(self._h, _p(rc), _p(rl), rc.shape[0], int(spread_level), int(max_skew),
                                         _p(pe) if pe.shape[0] else None, pe.shape[0], int(flags), _p(assign), _p(spread),
                                         _p(count), ctypes.byref(st)))
        return assign[:J], spread[:J], count[:Ds], st

    def place_spread(self, job_class: np.ndarray, spread_level: int, max_skew: int,
                     peers: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, JspSpreadStats]:
        """place_spread_runs with one class id per job (global order)."""
        rc, rl = job_runs(job_class)
        return self.place_spread_runs(rc, rl, spread_level, max_skew, peers)

    def place_spread_loop(self, run_class: np.ndarray, run_len: np.ndarray, spread_level: int, max_skew: int,
                          peers: Optional[np.ndarray] = None, iters: int = 200) -> Tuple[float, float, float, float]:
        """`iters` jsp_place_spread calls back to back timed in C
        (jspb_place_spread_loop): total, median and p99 per call and the median
        host walk inside a call, microseconds."""
        rc, rl, pe, J, Ds, assign, spread, count = self._spread_buffers(run_class, run_len, spread_level, peers)
        out = np.zeros(4, dtype=np.float64)
        check(self._lib.jspb_place_spread_loop(self._h, _p(rc), _p(rl), rc.shape[0], int(spread_level), int(max_skew),
                                               _p(pe) if pe.shape[0] else None, pe.shape[0], _p(assign), _p(spread),
                                               _p(count), None, int(iters), _p(out)))
        return float(out[0]), float(out[1]), float(out[2]), float(out[3])

    def spread_tables(self, spread_level: int, peers: Optional[np.ndarray] = None, form: int = 0, shift: int = -1,
                      iters: int = 0):
        """jspb_spread_tables: the spread walk's tables on the current snapshot
        (layout: jsplace_bench.h): (fits words, feasibility words, peers [D_s],
        cnt_feas [C, D_s], cnt_fits [C, D_s], (median, mean) device us of the
        launches with iters). form: the span counts' form, shift: the leaf
        pass's lanes per leaf (-1: as the call picks them)."""
        pe = np.ascontiguousarray(peers if peers is not None else [], dtype=np.int32).reshape(-1)
        nw = sum((int(self.topology.n_domains[k]) + 63) // 64 for k in self._class_level)
        Ds, C = int(self.topology.n_domains[int(spread_level)]), self.n_classes
        fits, feas = (np.zeros(max(nw, 1), dtype=np.uint64) for _ in range(2))
        pr = np.zeros(max(Ds, 1), dtype=np.uint32)
        cf, ce = (np.zeros(max(C * Ds, 1), dtype=np.uint32) for _ in range(2))
        out = np.zeros(2, dtype=np.float64)
        check(self._lib.jspb_spread_tables(self._h, int(spread_level), _p(pe) if pe.shape[0] else None, pe.shape[0],
                                           int(form), int(shift), _p(fits), _p(feas), nw, _p(pr), _p(cf), _p(ce),
                                           int(iters), _p(out)))
        return (fits[:nw], feas[:nw], pr[:Ds], cf[:C * Ds].reshape(C, Ds), ce[:C * Ds].reshape(C, Ds),
                (float(out[0]), float(out[1])))

    # ---------------------------------------------------------------- pod binding (jsp_bind_pods)
    def _bind_buffers(self, run_class, run_len, assign):
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        J = int(rl.astype(np.int64).sum())
        av = np.ascontiguousarray(assign, dtype=np.int32)
        if av.shape[0] != J:
            raise ValueError(f"assign has {av.shape[0]} entries for {J} jobs")
        pods = self._class_pods
        if rc.size and int(rc.max()) >= pods.shape[0]:
            raise ValueError("a run class is out of range")
        P = int((pods[rc] * rl.astype(np.int64)).sum()) if rc.size else 0
        # the library refuses P above its limit before it writes anything
        pod_row = np.empty(max(min(P, native.JSP_BIND_MAX_PODS), 1), dtype=np.int32)
        return rc, rl, J, av, P, pod_row

    def bind_pods_runs(self, run_class: np.ndarray, run_len: np.ndarray, assign: np.ndarray,
                       flags: int = 0) -> Tuple[np.ndarray, np.ndarray, JspBindStats]:
        """jsp_bind_pods: the runs of place_runs plus assign[J], each job's
        domain at its class's level or -1 (any assignment without intersecting
        domains). Every pod of a job whose domain is feasible now gets a row
        of it, first fit by row (DESIGN.md §2 "Pod binding"); the pods of the
        other jobs get -1. Returns (pod_row [P], pod_off [J + 1], stats):
        pod p of job j is pod_row[pod_off[j] + p]."""
        rc, rl, J, av, P, pod_row = self._bind_buffers(run_class, run_len, assign)
        pod_off = np.zeros(J + 1, dtype=np.uint64)
        st = JspBindStats()
        check(self._lib.jsp_bind_pods(self._h, _p(rc), _p(rl), rc.shape[0], _p(av), int(flags), _p(pod_row),
                                      _p(pod_off), ctypes.byref(st)))
        return pod_row[:P], pod_off, st

    def bind_pods(self, job_class: np.ndarray, assign: np.ndarray) -> Tuple[np.ndarray, np.ndarray, JspBindStats]:
        """bind_pods_runs with one class id per job (global order)."""
        rc, rl = job_runs(job_class)
        return self.bind_pods_runs(rc, rl, assign)

    def bind_loop(self, run_class: np.ndarray, run_len: np.ndarray, assign: np.ndarray,
                  iters: int = 200) -> Tuple[Tuple[float, float, float], np.ndarray, JspBindStats]:
        """`iters` jsp_bind_pods calls back to back timed in C (jspb_bind_loop):
        (total, median, p99 per call in microseconds), the last call's
        pod_row and its stats."""
        rc, rl, J, av, P, pod_row = self._bind_buffers(run_class, run_len, assign)
        st = JspBindStats()
        out = np.zeros(3, dtype=np.float64)
        check(self._lib.jspb_bind_loop(self._h, _p(rc), _p(rl), rc.shape[0], _p(av), _p(pod_row), ctypes.byref(st),
                                       int(iters), _p(out)))
        return (float(out[0]), float(out[1]), float(out[2])), pod_row[:P], st

    def bind_kernel_loop(self, iters: int = 200) -> Tuple[float, float, float]:
        """Device us per repetition of the last bind_pods call's stream work
        (tables' fill + claim + bind launches), of its bind launches alone,
        and of the tally (jspb_bind_kernel_loop)."""
        out = np.zeros(3, dtype=np.float64)
        check(self._lib.jspb_bind_kernel_loop(self._h, int(iters), _p(out)))
        return float(out[0]), float(out[1]), float(out[2])

    # ---------------------------------------------------------------- assume and forget (jsp_assume / jsp_forget)
    def _assume_buffers(self, run_class, run_len, assign, owner):
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        J = int(rl.astype(np.int64).sum())
        av = np.ascontiguousarray(assign, dtype=np.int32)
        ov = np.ascontiguousarray(owner, dtype=np.int32)
        if av.shape[0] != J or ov.shape[0] != J:
            raise ValueError(f"assign has {av.shape[0]} and owner {ov.shape[0]} entries for {J} jobs")
        return rc, rl, J, av, ov

    def assume_runs(self, run_class: np.ndarray, run_len: np.ndarray, assign: np.ndarray, owner: np.ndarray,
                    flags: int = 0) -> Tuple[np.ndarray, JspAssumeStats]:
        """jsp_assume: the runs of place_runs, assign[J] and owner[J]. Every
        row of a job's domain that is feasible now gets excl_owner = owner[j]
        in the resident snapshot, so no later placement hands the domain out
        again (DESIGN.md §2 "Assume and forget"); nothing is written for the
        other jobs, and nothing at all when the call is refused. Returns
        (committed [J] bool, stats)."""
        rc, rl, J, av, ov = self._assume_buffers(run_class, run_len, assign, owner)
        committed = np.zeros(max(J, 1), dtype=np.uint8)
        st = JspAssumeStats()
        check(self._lib.jsp_assume(self._h, _p(rc), _p(rl), rc.shape[0], _p(av), _p(ov), int(flags), _p(committed),
                                   ctypes.byref(st)))
        return committed[:J].astype(bool), st

    def assume(self, job_class: np.ndarray, assign: np.ndarray, owner: np.ndarray) -> Tuple[np.ndarray, JspAssumeStats]:
        """assume_runs with one class id per job (global order)."""
        rc, rl = job_runs(job_class)
        return self.assume_runs(rc, rl, assign, owner)

    def forget(self, owners) -> int:
        """jsp_forget: every row whose excl_owner is one of `owners` is free
        again (-1). Returns the number of rows cleared."""
        ov = np.ascontiguousarray(owners, dtype=np.int32).reshape(-1)
        cleared = ctypes.c_uint64(0)
        check(self._lib.jsp_forget(self._h, _p(ov) if ov.size else None, ov.shape[0], ctypes.byref(cleared)))
        return int(cleared.value)

    def assume_forget_loop(self, run_class: np.ndarray, run_len: np.ndarray, assign: np.ndarray, owner: np.ndarray,
                           iters: int = 200) -> Tuple[Tuple[float, float, float, float], JspAssumeStats, int]:
        """`iters` times jsp_assume then jsp_forget of its owners, each half
        timed in C (jspb_assume_forget_loop): (assume median, assume p99,
        forget median, forget p99 in microseconds), the last assume's stats and
        the last forget's cleared rows."""
        rc, rl, J, av, ov = self._assume_buffers(run_class, run_len, assign, owner)
        st = JspAssumeStats()
        cleared = ctypes.c_uint64(0)
        out = np.zeros(4, dtype=np.float64)
        check(self._lib.jspb_assume_forget_loop(self._h, _p(rc), _p(rl), rc.shape[0], _p(av), _p(ov), int(iters),
                                                ctypes.byref(st), ctypes.byref(cleared), _p(out)))
        return (float(out[0]), float(out[1]), float(out[2]), float(out[3])), st, int(cleared.value)

    def host_placer(self, run_class: np.ndarray, run_len: np.ndarray):
        """A pre-bound jsp_place call for one run list (host buffers allocated
        once): what a caller that places the same JobSet repeatedly -- the
        recovery path, the benchmark -- binds. Returns a callable; its
        `.assign` array and `.stats` struct hold the last call's results."""
        rc = np.ascontiguousarray(run_class, dtype=np.uint32)
        rl = np.ascontiguousarray(run_len, dtype=np.uint32)
        J = int(rl.astype(np.int64).sum())
        assign = np.empty(max(J, 1), dtype=np.int32)
        st = JspStats()
        fn = self._lib.jsp_place
        args = (self._h, rc.ctypes.data, rl.ctypes.data, rc.shape[0], assign.ctypes.data, None, None,
                ctypes.byref(st))

        def call() -> JspStats:
            r = fn(*args)
            if r:
                check(r)
            return st
        loop_out = np.zeros(3, dtype=np.float64)

        def recovery(trials: int, idle_us: float, gap_us: float, patch_rows: np.ndarray, patch_taints: np.ndarray,
                     spin: bool = False) -> np.ndarray:
            """The cold recovery timed in C (jspb_recovery_loop): per trial the
            idle wait, a one-row patch, the gap, jsp_place. [trials, 3] µs:
            patch call, place call, gap."""
            pr = np.ascontiguousarray(patch_rows, dtype=np.uint32)
            pt = np.ascontiguousarray(patch_taints, dtype=np.uint32)
            out = np.zeros((int(trials), 3), dtype=np.float64)
            check(self._lib.jspb_recovery_loop(self._h, rc.ctypes.data, rl.ctypes.data, rc.shape[0], assign.ctypes.data,
                                              int(trials), float(idle_us), float(gap_us), 1 if spin else 0, _p(pr),
                                              _p(pt), int(pr.shape[0]), out.ctypes.data))
            return out

        def loop(iters: int, patch_rows: Optional[np.ndarray] = None,
                 patch_taints: Optional[np.ndarray] = None) -> Tuple[float, float, float]:
            """`iters` calls back to back timed in C (jspb_place_loop), each
            after a one-row taint patch when rows are given: total, median and
            p99 per step, microseconds."""
            pr = None if patch_rows is None else np.ascontiguousarray(patch_rows, dtype=np.uint32)
            pt = None if patch_taints is None else np.ascontiguousarray(patch_taints, dtype=np.uint32)
            check(self._lib.jspb_place_loop(self._h, rc.ctypes.data, rl.ctypes.data, rc.shape[0], assign.ctypes.data,
                                           int(iters), _p(pr), _p(pt), 0 if pr is None else int(pr.shape[0]),
                                           loop_out.ctypes.data))
            return float(loop_out[0]), float(loop_out[1]), float(loop_out[2])
        call.assign = assign[:J]
        call.stats = st
        call.loop = loop
        call.recovery = recovery
        call.keep = (rc, rl, assign, loop_out)
        return call

    def host_patcher(self, rows: np.ndarray, labels: Optional[np.ndarray] = None,
                     taints: Optional[np.ndarray] = None, free: Optional[np.ndarray] = None,
                     excl: Optional[np.ndarray] = None):
        """A pre-bound jsp_snapshot_patch for one delta (arrays converted once):
        what a watch-event handler that patches the same rows repeatedly binds
        (the bench's recovery legs). Returns a callable."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=dt)
                for a, dt in ((labels, np.uint64), (taints, np.uint32), (free, np.uint32), (excl, np.int32))]
        fn = self._lib.jsp_snapshot_patch
        args = (self._h, rows.ctypes.data, rows.shape[0], *[_p(a) for a in arrs])

        def call() -> None:
            r = fn(*args)
            if r:
                check(r)
        call.keep = (rows, arrs)
        return call

    def shards(self) -> Tuple[int, int]:
        """(shards, distinct devices) of this engine (1, 1 unless a device set)."""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        check(self._lib.jsp_engine_shards(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def check(self) -> None:
        """jsp_engine_check: wait for the engine's launches, raise if one failed."""
        check(self._lib.jsp_engine_check(self._h))

    def place_device(self, d_run_class: int, d_run_len: int, n_runs: int, n_jobs: int, d_assign: int,
                     stream: Optional[int] = None) -> None:
        check(self._lib.jsp_place_device(self._h, d_run_class, d_run_len, n_runs, n_jobs, d_assign, stream))

    def tally_device(self, d_cap: int, d_occ: int, ld: int, stream: Optional[int] = None) -> None:
        check(self._lib.jsp_tally_device(self._h, d_cap, d_occ, ld, stream))

    def assign_device(self, d_cap: int, d_occ: int, ld: int, d_run_class: int, d_run_len: int, n_runs: int,
                      n_jobs: int, d_assign: int, stream: Optional[int] = None) -> None:
        check(self._lib.jsp_assign_device(self._h, d_cap, d_occ, ld, d_run_class, d_run_len, n_runs, n_jobs,
                                          d_assign, stream))

    def tally_device_timed(self, d_cap: int, d_occ: int, ld: int, iters: int, scrub: int = 0,
                           scrub_bytes: int = 0) -> Tuple[float, float]:
        """(median, mean) device µs of `iters` back-to-back tallies on the
        engine stream, timed by events on the dispatches themselves
        (jspb_tally_device_timed); with a scrub buffer, each one cold."""
        out = np.zeros(2, dtype=np.float64)
        check(self._lib.jspb_tally_device_timed(self._h, d_cap, d_occ, ld, iters, scrub or None, scrub_bytes,
                                               _p(out)))
        return float(out[0]), float(out[1])

    def place_device_timed(self, d_run_class: int, d_run_len: int, n_runs: int, n_jobs: int, d_assign: int,
                           iters: int, scrub: int = 0, scrub_bytes: int = 0) -> Tuple[float, float]:
        """(median, mean) device µs of `iters` back-to-back device-path
        placements (first dispatch start -> last dispatch end each;
        jspb_place_device_timed); with a scrub buffer, each one cold."""
        out = np.zeros(2, dtype=np.float64)
        check(self._lib.jspb_place_device_timed(self._h, d_run_class, d_run_len, n_runs, n_jobs, d_assign, iters,
                                               scrub or None, scrub_bytes, _p(out)))
        return float(out[0]), float(out[1])

    def tally_device_spans(self, d_cap: int, d_occ: int, ld: int,
                           iters: int) -> Tuple[float, float, float, float]:
        """In-kernel span of the one-tile wave tally (first wave start -> last
        wave end, device clock; jspb_tally_device_spans): (median, mean) us,
        the dispatch-event time of an empty one-workgroup launch, and the
        back-to-back launches' period by the kernels' own clock."""
        out = np.zeros(4, dtype=np.float64)
        check(self._lib.jspb_tally_device_spans(self._h, d_cap, d_occ, ld, int(iters), _p(out)))
        return float(out[0]), float(out[1]), float(out[2]), float(out[3])

    def explain_rows_loop(self, iters: int = 200) -> Tuple[float, float]:
        """(row pass of jsp_explain, tally) device us per launch: one event
        pair around `iters` back-to-back launches each, after a warm-up
        (jspb_explain_rows_loop)."""
        out = np.zeros(2, dtype=np.float64)
        check(self._lib.jspb_explain_rows_loop(self._h, int(iters), _p(out)))
        return float(out[0]), float(out[1])

    def link_floor(self, iters: int = 2000) -> Tuple[float, float, float]:
        """Host -> device -> host round trip through pinned memory with the
        resident service's polling (jspb_link_floor): (p50, p99, mean) us."""
        out = np.zeros(3, dtype=np.float64)
        check(self._lib.jspb_link_floor(self._h, int(iters), _p(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def set_fused(self, enable: bool) -> None:
        check(self._lib.jspb_set_fused(self._h, native.JSP_FUSED_AUTO if enable else native.JSP_FUSED_OFF))

    def set_service(self, enable: bool, parked: bool = False) -> None:
        """Resident placement service for host-API placements
        (jsp_engine_set_service; on by default). parked: it never idles out
        (JSP_SERVICE_PARKED, a dedicated GPU)."""
        mode = (native.JSP_SERVICE_PARKED if parked else native.JSP_SERVICE_AUTO) if enable else native.JSP_SERVICE_OFF
        check(self._lib.jsp_engine_set_service(self._h, mode))

    def service_stop(self) -> None:
        """Stop the resident service now (before a device-wide synchronize)."""
        check(self._lib.jsp_engine_service_stop(self._h))

    def service_counters(self) -> dict:
        """Totals of the service that left last (jspb_service_counters): its
        tiles, requests its dispatcher answered from the standing lines, clean
        requests it handed to the tiles, evaluate-rings. Stop the service first."""
        out = np.zeros(4, dtype=np.uint64)
        check(self._lib.jspb_service_counters(self._h, _p(out)))
        return dict(zip(("tiles", "answered", "handed", "evals"), (int(x) for x in out)))

    def lease_counters(self, reset: bool = False) -> dict:
        """The host lease's totals (jspb_lease_counters): placements answered
        on the host from the last answer's lines, leases taken, leases dropped.
        Readable while the service runs."""
        out = np.zeros(3, dtype=np.uint64)
        check(self._lib.jspb_lease_counters(self._h, _p(out), 1 if reset else 0))
        return dict(zip(("answered", "taken", "dropped"), (int(x) for x in out)))

    def lease_memo_counters(self, reset: bool = False) -> dict:
        """The lease's kept list (jspb_lease_memo_counters): host answers
        copied from a kept list (the call that built it included), lists
        built. Readable while the service runs."""
        out = np.zeros(2, dtype=np.uint64)
        check(self._lib.jspb_lease_memo_counters(self._h, _p(out), 1 if reset else 0))
        return dict(zip(("answered", "built"), (int(x) for x in out)))

    def service_clock(self) -> np.ndarray:
        """The last timed service request's per-tile 100 MHz stamps [tiles, 8]
        (jspb_service_clock); empty when none is held."""
        return self.service_clock_rows()[0]

    def service_clock_rows(self) -> Tuple[np.ndarray, np.ndarray]:
        """(the tiles' stamps [tiles, 8], the dispatcher's row [8]: 0 request
        seen in the mailbox, 1 bell rung) of the last timed service request."""
        out = np.zeros(257 * 8, dtype=np.uint32)
        n = ctypes.c_uint32(0)
        check(self._lib.jspb_service_clock(self._h, _p(out), out.shape[0], ctypes.byref(n)))
        k = n.value
        return out[:k * 8].reshape(k, 8), out[k * 8:(k + 1) * 8]

    # ---------------------------------------------------------------- webhook / reconciler batches
    def resolve_leader_domains(self, leader_rows: np.ndarray, levels: np.ndarray) -> np.ndarray:
        rows = np.ascontiguousarray(leader_rows, dtype=np.int32)
        lv = np.ascontiguousarray(levels, dtype=np.uint32)
        out = np.empty(max(rows.shape[0], 1), dtype=np.int32)
        check(self._lib.jsp_resolve_leader_domains(self._h, _p(rows), _p(lv), rows.shape[0], _p(out)))
        return out[:rows.shape[0]]

    def audit_placements(self, leader_rows: np.ndarray, levels: np.ndarray, follower_off: np.ndarray,
                         follower_domains: np.ndarray) -> np.ndarray:
        rows = np.ascontiguousarray(leader_rows, dtype=np.int32)
        lv = np.ascontiguousarray(levels, dtype=np.uint32)
        off = np.ascontiguousarray(follower_off, dtype=np.uint32)
        fd = np.ascontiguousarray(follower_domains, dtype=np.int32)
        out = np.empty(max(rows.shape[0], 1), dtype=np.uint32)
        check(self._lib.jsp_audit_placements(self._h, _p(rows), _p(lv), _p(off), _p(fd) if fd.size else None,
                                             rows.shape[0], _p(out)))
        return out[:rows.shape[0]]

    # ---------------------------------------------------------------- diagnosis (jsp_explain)
    def explain(self) -> List[JspClassExplain]:
        """Per uploaded class, why jobs of it cannot be placed: the rows that
        fail its selector, its tolerations or its requests, and its level's
        domains that are occupied, too small or feasible (jsplace.h
        jsp_class_explain)."""
        arr = (JspClassExplain * max(self.n_classes, 1))()
        check(self._lib.jsp_explain(self._h, arr, self.n_classes))
        return [arr[c] for c in range(self.n_classes)]

    # ---------------------------------------------------------------- metrics (jsp_engine_get_metrics)
    def metrics(self, reset: bool = False) -> native.JspMetrics:
        """The engine's histograms and counters (jsplace.h jsp_metrics)."""
        m = native.JspMetrics()
        check(self._lib.jsp_engine_get_metrics(self._h, ctypes.byref(m), 1 if reset else 0))
        return m

    # ---------------------------------------------------------------- instrumentation (jsplace_bench.h)
    def set_timing(self, enable: bool) -> None:
        check(self._lib.jspb_set_timing(self._h, 1 if enable else 0))

    def timing(self, reset: bool = True) -> JspTiming:
        t = JspTiming()
        check(self._lib.jspb_get_timing(self._h, ctypes.byref(t), 1 if reset else 0))
        return t

    def last_plan(self) -> dict:
        """The launch plan of the last placement, tally or assignment
        (jspb_last_plan; fields: jsplace_bench.h jspb_plan): which tally
        kernel, which walker and template, the LDS staging, the class groups.
        A call the resident service answered reports that service's start."""
        pl = native.JspbPlan()
        check(self._lib.jspb_last_plan(self._h, ctypes.byref(pl)))
        return {n: int(getattr(pl, n)) for n, _ in native.JspbPlan._fields_}

    @property
    def stream(self) -> int:
        return self._lib.jsp_engine_stream(self._h) or 0

    def sync(self) -> None:
        check(self._lib.jsp_engine_sync(self._h))
